// Pose graph: keyframe poses optimised on the device after a loop closure.  Definitions: include/lidar_odometry_amd.h
// ("pose graph"); kernels: k_graph.hpp; host math (checks, Cholesky, gauge, CSR, LM policy): graph_host.cpp; DESIGN.md 7g.
// New code beside the align path: nothing here touches a map handle, and no default path launches any of it.
//
// The host copy of nodes and edges is the record: adds, set_pose and get_poses work on it alone, and the device copy is
// brought up to date at the next call that computes (sync_device).  An optimisation reads the poses back.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "graph_host.hpp"
#include "k_graph.hpp"
#include "lom_internal.hpp"

using namespace lom;

namespace {

// device buffers: per node, per edge, or fixed size
enum {
    G_POSE = 0, G_CAND, G_FIXED, G_ROW, G_G, G_HD, G_D, G_MINV, G_X, G_R, G_ZV, G_P, G_Y, G_PART_A, G_PART_B,  // per node
    G_IJ, G_Z, G_U, G_DELTA, G_E, G_S, G_W, G_COST, G_COSTC, G_B, G_C, G_UE, G_ENT,                            // per edge
    G_SCAL,
    G_COUNT
};
constexpr int kFirstEdgeBuf = G_IJ;
// bytes per node / per edge (G_ROW holds one word more, G_PART_* one double per 16 nodes, rounded up)
constexpr size_t kBytesPer[G_COUNT] = {56, 56, 4, 4, 48, 288, 48, 288, 48, 48, 48, 48, 48, 1, 1,
                                       8, 56, 168, 8, 48, 8, 8, 8, 8, 576, 48, 48, 8, 0};
constexpr int64_t kGraphMax = 1ll << 27;  // nodes, edges: indices and n * 6 stay inside 32 bits

}  // namespace

// The graph owns its stream and every buffer below; calls on one graph are serialised by `lock`.
struct lom_graph : DeviceHandle {
    std::mutex lock;
    // the record
    std::vector<double> poses, Z, U, delta;  // [n][7], [m][7], [m][21], [m]
    std::vector<int32_t> fixed, ij;          // [n], [m][2]
    // the device copy
    bool nodes_dirty = true, edges_dirty = true;
    size_t cap_n = 0, cap_m = 0;
    DeviceBuf buf[G_COUNT];
    PinnedBuf report;  // GraphReport: h_report the host's view, d_report the device's
    GraphReport *h_report = nullptr, *d_report = nullptr;

    size_t n() const { return fixed.size(); }
    size_t m() const { return delta.size(); }
    template <typename T>
    T *dev(int which) const
    {
        return buf[which].as<T>();
    }
};

namespace {

thread_local std::string g_graph_create_error;

uint32_t blocks_of(size_t count, size_t per) { return (uint32_t)std::max<size_t>((count + per - 1) / per, 1); }

// room on the device for cap_n nodes / cap_m edges: geometric growth; nothing is carried over (the host copy is the record)
int reserve_device(lom_graph *g, size_t need_n, size_t need_m)
{
    const bool grow_n = need_n > g->cap_n, grow_m = need_m > g->cap_m;
    if (!grow_n && !grow_m && g->buf[G_SCAL].p) return LOM_OK;
    const size_t cap_n = grow_n ? std::max(need_n, g->cap_n * 2) : g->cap_n;
    const size_t cap_m = grow_m ? std::max(need_m, g->cap_m * 2) : g->cap_m;
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    for (int b = 0; b < G_COUNT; b++) {
        const bool per_edge = b >= kFirstEdgeBuf && b != G_SCAL;
        if (b == G_SCAL ? g->buf[b].p != nullptr : !(per_edge ? grow_m : grow_n)) continue;
        size_t bytes;
        if (b == G_SCAL)
            bytes = sizeof(GraphScalars);
        else if (b == G_ROW)
            bytes = (cap_n + 1) * 4;
        else if (b == G_PART_A || b == G_PART_B)
            bytes = (cap_n / kGraphRowsPerBlock + 2) * 8;
        else
            bytes = (per_edge ? cap_m : cap_n) * kBytesPer[b];
        release(g->buf[b]);  // exactly this size, not 1.5 times the old one: the capacities above are the growth rule
        if (ensure(g, g->buf[b], std::max<size_t>(bytes, 8)) != LOM_OK) {
            if (per_edge) g->cap_m = 0; else g->cap_n = 0;  // the next call allocates afresh
            g->nodes_dirty = g->edges_dirty = true;
            return fail(g, LOM_ERR_OOM, "hipMalloc (pose graph)");
        }
    }
    if (grow_n) g->cap_n = cap_n, g->nodes_dirty = true;
    if (grow_m) g->cap_m = cap_m, g->edges_dirty = true;
    return LOM_OK;
}

// the device copy up to date with the record (enqueued; the CSR of incident edges is built here, on the host)
int sync_device(lom_graph *g)
{
    const size_t n = g->n(), m = g->m();
    int rc = reserve_device(g, std::max<size_t>(n, 1), std::max<size_t>(m, 1));
    if (rc != LOM_OK) return rc;
    if (g->nodes_dirty && n) {
        LOM_HIP(g, hipMemcpyAsync(g->buf[G_POSE].p, g->poses.data(), n * 56, hipMemcpyHostToDevice, g->stream));
        LOM_HIP(g, hipMemcpyAsync(g->buf[G_FIXED].p, g->fixed.data(), n * 4, hipMemcpyHostToDevice, g->stream));
    }
    if ((g->edges_dirty || g->nodes_dirty) && n) {  // (more nodes: a longer row_ptr)
        std::vector<uint32_t> row_ptr, entries;
        graph::build_csr((int64_t)n, (int64_t)m, g->ij.data(), row_ptr, entries);
        LOM_HIP(g, hipMemcpyAsync(g->buf[G_ROW].p, row_ptr.data(), (n + 1) * 4, hipMemcpyHostToDevice, g->stream));
        if (m) LOM_HIP(g, hipMemcpyAsync(g->buf[G_ENT].p, entries.data(), m * 8, hipMemcpyHostToDevice, g->stream));
        LOM_HIP(g, hipStreamSynchronize(g->stream));  // the vectors go out of scope
    }
    if (g->edges_dirty && m) {
        LOM_HIP(g, hipMemcpyAsync(g->buf[G_IJ].p, g->ij.data(), m * 8, hipMemcpyHostToDevice, g->stream));
        LOM_HIP(g, hipMemcpyAsync(g->buf[G_Z].p, g->Z.data(), m * 56, hipMemcpyHostToDevice, g->stream));
        LOM_HIP(g, hipMemcpyAsync(g->buf[G_U].p, g->U.data(), m * 168, hipMemcpyHostToDevice, g->stream));
        LOM_HIP(g, hipMemcpyAsync(g->buf[G_DELTA].p, g->delta.data(), m * 8, hipMemcpyHostToDevice, g->stream));
    }
    LOM_HIP(g, hipStreamSynchronize(g->stream));  // pageable sources: the record may change as soon as this returns
    g->nodes_dirty = g->edges_dirty = false;
    return LOM_OK;
}

int enqueue_linearise(lom_graph *g)
{
    const uint32_t m = (uint32_t)g->m();
    hipLaunchKernelGGL(k_graph_linearise, dim3(blocks_of(m, kGraphThreads)), dim3(kGraphThreads), 0, g->stream, m,
                       g->dev<const double>(G_POSE), g->dev<const int32_t>(G_IJ), g->dev<const double>(G_Z),
                       g->dev<const double>(G_U), g->dev<const double>(G_DELTA), g->dev<double>(G_E), g->dev<double>(G_S),
                       g->dev<double>(G_W), g->dev<double>(G_COST), g->dev<double>(G_B), g->dev<double>(G_C));
    LOM_HIP(g, hipGetLastError());
    return LOM_OK;
}

int enqueue_gather(lom_graph *g, double lambda)
{
    const uint32_t n = (uint32_t)g->n();
    hipLaunchKernelGGL(k_graph_node_gather, dim3(blocks_of(n, kGraphRowsPerBlock)), dim3(kGraphThreads), 0, g->stream, n,
                       g->dev<const int32_t>(G_FIXED), g->dev<const uint32_t>(G_ROW), g->dev<const uint32_t>(G_ENT),
                       g->dev<const double>(G_B), g->dev<const double>(G_C), lambda, g->dev<double>(G_G), g->dev<double>(G_HD),
                       g->dev<double>(G_D), g->dev<double>(G_MINV));
    LOM_HIP(g, hipGetLastError());
    return LOM_OK;
}

// y = (H_ff + lambda D) p and the partials of p^T y into G_PART_A
int enqueue_matvec(lom_graph *g, double lambda)
{
    const uint32_t n = (uint32_t)g->n(), m = (uint32_t)g->m();
    const GraphScalars *sc = g->dev<const GraphScalars>(G_SCAL);
    hipLaunchKernelGGL(k_graph_mv_edge, dim3(blocks_of(m, kGraphThreads)), dim3(kGraphThreads), 0, g->stream, m,
                       g->dev<const int32_t>(G_IJ), g->dev<const int32_t>(G_FIXED), g->dev<const double>(G_B),
                       g->dev<const double>(G_P), g->dev<double>(G_UE), sc);
    LOM_HIP(g, hipGetLastError());
    hipLaunchKernelGGL(k_graph_mv_node, dim3(blocks_of(n, kGraphRowsPerBlock)), dim3(kGraphThreads), 0, g->stream, n,
                       g->dev<const int32_t>(G_FIXED), g->dev<const uint32_t>(G_ROW), g->dev<const uint32_t>(G_ENT),
                       g->dev<const double>(G_B), g->dev<const double>(G_UE), g->dev<const double>(G_D), lambda,
                       g->dev<const double>(G_P), g->dev<double>(G_Y), g->dev<double>(G_PART_A), sc);
    LOM_HIP(g, hipGetLastError());
    return LOM_OK;
}

int enqueue_scalar(lom_graph *g, int mode, uint32_t count, int part, double rtol2)
{
    hipLaunchKernelGGL(k_graph_cg_scalar, dim3(1), dim3(kGraphThreads), 0, g->stream, mode, count,
                       g->dev<const double>(part), rtol2, g->dev<GraphScalars>(G_SCAL));
    LOM_HIP(g, hipGetLastError());
    return LOM_OK;
}

// the whole solve of (H_ff + lambda D) d = -g_f, enqueued ahead: d in G_X.  Once the scalars say done, every later
// kernel of the chain returns at once.
int enqueue_pcg(lom_graph *g, double lambda, const lom_graph_params *prm)
{
    const uint32_t n = (uint32_t)g->n();
    const uint32_t nb = blocks_of(n, kGraphThreads), nrows = blocks_of(n, kGraphRowsPerBlock);
    const GraphScalars *sc = g->dev<const GraphScalars>(G_SCAL);
    const double rtol2 = prm->pcg_rtol * prm->pcg_rtol;
    hipLaunchKernelGGL(k_graph_cg_init, dim3(nb), dim3(kGraphThreads), 0, g->stream, n, g->dev<const double>(G_G),
                       g->dev<const double>(G_MINV), g->dev<double>(G_X), g->dev<double>(G_R), g->dev<double>(G_ZV),
                       g->dev<double>(G_P), g->dev<double>(G_PART_B));
    LOM_HIP(g, hipGetLastError());
    int rc = enqueue_scalar(g, GRAPH_SCALAR_INIT, nb, G_PART_B, rtol2);
    for (int it = 0; it < prm->max_pcg && rc == LOM_OK; it++) {
        if ((rc = enqueue_matvec(g, lambda)) != LOM_OK) break;
        if ((rc = enqueue_scalar(g, GRAPH_SCALAR_ALPHA, nrows, G_PART_A, rtol2)) != LOM_OK) break;
        hipLaunchKernelGGL(k_graph_cg_update, dim3(nb), dim3(kGraphThreads), 0, g->stream, n, g->dev<const double>(G_MINV),
                           g->dev<const double>(G_P), g->dev<const double>(G_Y), g->dev<double>(G_X), g->dev<double>(G_R),
                           g->dev<double>(G_ZV), g->dev<double>(G_PART_B), sc);
        LOM_HIP(g, hipGetLastError());
        if ((rc = enqueue_scalar(g, GRAPH_SCALAR_BETA, nb, G_PART_B, rtol2)) != LOM_OK) break;
        hipLaunchKernelGGL(k_graph_cg_dir, dim3(blocks_of((size_t)n * 6, kGraphThreads)), dim3(kGraphThreads), 0, g->stream,
                           n * 6, g->dev<const double>(G_ZV), g->dev<double>(G_P), sc);
        LOM_HIP(g, hipGetLastError());
    }
    return rc;
}

int enqueue_report(lom_graph *g, double lambda, int with_step)
{
    hipLaunchKernelGGL(k_graph_report, dim3(1), dim3(64), 0, g->stream, (uint32_t)g->n(), (uint32_t)g->m(),
                       g->dev<const double>(G_COST), g->dev<const double>(G_COSTC), g->dev<const double>(G_G),
                       g->dev<const double>(G_D), g->dev<const double>(G_X), lambda, with_step,
                       g->dev<const GraphScalars>(G_SCAL), g->d_report);
    LOM_HIP(g, hipGetLastError());
    return LOM_OK;
}

// linearisation, gather and the report of cost and max|g| at the current poses; the host waits
int evaluate_now(lom_graph *g, double lambda)
{
    int rc = enqueue_linearise(g);
    if (rc == LOM_OK) rc = enqueue_gather(g, lambda);
    if (rc == LOM_OK) rc = enqueue_report(g, lambda, 0);
    if (rc != LOM_OK) return rc;
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    return LOM_OK;
}

bool edge_ok(const lom_graph *g, int64_t i, int64_t j, const lom_graph_pose *z, const double *omega, double delta, double U[21])
{
    const int64_t n = (int64_t)g->n();
    return i != j && i >= 0 && j >= 0 && i < n && j < n && graph::pose_ok(z) && std::isfinite(delta) && delta >= 0.0 &&
           graph::cholesky6_upper(omega, U);
}

}  // namespace

extern "C" {

int lom_graph_create(int device, size_t node_hint, size_t edge_hint, lom_graph **out)
{
    if (!out) return LOM_ERR_ARG;
    *out = nullptr;
    if (node_hint > (size_t)kGraphMax || edge_hint > (size_t)kGraphMax)
        return create_fail(g_graph_create_error, LOM_ERR_ARG, "node_hint, edge_hint <= 2^27");
    if (const int rc = check_device(device, g_graph_create_error); rc != LOM_OK) return rc;
    lom_graph *g = new (std::nothrow) lom_graph();
    if (!g) return create_fail(g_graph_create_error, LOM_ERR_OOM, "host allocation");
    g->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = alloc(g->report, sizeof(GraphReport), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&g->d_report, g->report.h, 0);
    g->h_report = g->report.as<GraphReport>();
    int rc = e == hipSuccess ? LOM_OK : create_fail(g_graph_create_error, LOM_ERR_HIP, "pose graph setup", e);
    if (rc == LOM_OK) {
        rc = reserve_device(g, std::max<size_t>(node_hint, 1), std::max<size_t>(edge_hint, 1));
        if (rc != LOM_OK) g_graph_create_error = g->error;
    }
    if (rc != LOM_OK) {
        lom_graph_destroy(g);
        return rc;
    }
    g->poses.reserve(node_hint * 7), g->fixed.reserve(node_hint);
    g->ij.reserve(edge_hint * 2), g->Z.reserve(edge_hint * 7), g->U.reserve(edge_hint * 21), g->delta.reserve(edge_hint);
    *out = g;
    return LOM_OK;
}

void lom_graph_destroy(lom_graph *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;  // the buffers go with it
}

const char *lom_graph_last_error(const lom_graph *g) { return g ? g->error.c_str() : g_graph_create_error.c_str(); }

int lom_graph_clear(lom_graph *g)
{
    if (!g) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(g->lock);
    g->poses.clear(), g->fixed.clear(), g->ij.clear(), g->Z.clear(), g->U.clear(), g->delta.clear();
    g->nodes_dirty = g->edges_dirty = true;
    return LOM_OK;
}

void *lom_graph_stream(lom_graph *g) { return g ? (void *)g->stream : nullptr; }
int lom_graph_device(const lom_graph *g) { return g ? g->device : LOM_ERR_ARG; }

int64_t lom_graph_add_nodes(lom_graph *g, const lom_graph_pose *poses, const int32_t *fixed, size_t n)
{
    if (!g || (n && (!poses || !fixed))) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(g->lock);
    if (n > (size_t)kGraphMax || g->n() + n > (size_t)kGraphMax) return fail(g, LOM_ERR_ARG, "more than 2^27 nodes");
    for (size_t k = 0; k < n; k++)
        if (!graph::pose_ok(poses + k)) return fail(g, LOM_ERR_ARG, "a pose is not finite or its quaternion is zero");
    const int64_t first = (int64_t)g->n();
    for (size_t k = 0; k < n; k++) {
        double x[7];
        graph::normalised(poses + k, x);
        g->poses.insert(g->poses.end(), x, x + 7);
        g->fixed.push_back(fixed[k] ? 1 : 0);
    }
    if (n) g->nodes_dirty = true;
    return first;
}

int64_t lom_graph_add_node(lom_graph *g, const lom_graph_pose *pose, int fixed)
{
    const int32_t f = fixed;
    if (!pose) return LOM_ERR_ARG;
    return lom_graph_add_nodes(g, pose, &f, 1);
}

int64_t lom_graph_add_edges(lom_graph *g, const int32_t *ij, const lom_graph_pose *z, const double *omega36,
                            const double *delta, size_t n)
{
    if (!g || (n && (!ij || !z || !omega36 || !delta))) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(g->lock);
    if (n > (size_t)kGraphMax || g->m() + n > (size_t)kGraphMax) return fail(g, LOM_ERR_ARG, "more than 2^27 edges");
    std::vector<double> U(n * 21);
    for (size_t k = 0; k < n; k++)
        if (!edge_ok(g, ij[2 * k], ij[2 * k + 1], z + k, omega36 + k * 36, delta[k], U.data() + k * 21))
            return fail(g, LOM_ERR_ARG,
                        ("edge " + std::to_string(k) + " of the call: i == j, a node that does not exist, a bad pose, an "
                         "Omega that is not positive definite, or a negative delta").c_str());
    const int64_t first = (int64_t)g->m();
    for (size_t k = 0; k < n; k++) {
        double x[7];
        graph::normalised(z + k, x);
        g->ij.push_back(ij[2 * k]), g->ij.push_back(ij[2 * k + 1]);
        g->Z.insert(g->Z.end(), x, x + 7);
        g->delta.push_back(delta[k]);
    }
    g->U.insert(g->U.end(), U.begin(), U.end());
    if (n) g->edges_dirty = true;
    return first;
}

int64_t lom_graph_add_edge(lom_graph *g, int64_t i, int64_t j, const lom_graph_pose *z, const double omega36[36], double delta)
{
    if (!g || !z || !omega36) return LOM_ERR_ARG;
    if (i < 0 || j < 0 || i >= kGraphMax || j >= kGraphMax) {
        std::lock_guard<std::mutex> lk(g->lock);
        return fail(g, LOM_ERR_ARG, "an edge names a node that does not exist");
    }
    const int32_t ij[2] = {(int32_t)i, (int32_t)j};
    return lom_graph_add_edges(g, ij, z, omega36, &delta, 1);
}

int64_t lom_graph_node_count(const lom_graph *g)
{
    if (!g) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(const_cast<lom_graph *>(g)->lock);
    return (int64_t)g->n();
}

int64_t lom_graph_edge_count(const lom_graph *g)
{
    if (!g) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(const_cast<lom_graph *>(g)->lock);
    return (int64_t)g->m();
}

int lom_graph_get_poses(lom_graph *g, int64_t first, int64_t n, lom_graph_pose *out)
{
    if (!g || n < 0 || first < 0 || (n && !out)) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(g->lock);
    if (first > (int64_t)g->n() || n > (int64_t)g->n() - first) return fail(g, LOM_ERR_ARG, "no node with this id");
    if (n) std::memcpy(out, g->poses.data() + first * 7, (size_t)n * 56);
    return LOM_OK;
}

int lom_graph_set_pose(lom_graph *g, int64_t id, const lom_graph_pose *pose)
{
    if (!g || !pose) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(g->lock);
    if (id < 0 || id >= (int64_t)g->n()) return fail(g, LOM_ERR_ARG, "no node with this id");
    if (!graph::pose_ok(pose)) return fail(g, LOM_ERR_ARG, "a pose is not finite or its quaternion is zero");
    graph::normalised(pose, g->poses.data() + id * 7);
    g->nodes_dirty = true;
    return LOM_OK;
}

int lom_graph_set_fixed(lom_graph *g, int64_t id, int fixed)
{
    if (!g) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(g->lock);
    if (id < 0 || id >= (int64_t)g->n()) return fail(g, LOM_ERR_ARG, "no node with this id");
    g->fixed[(size_t)id] = fixed ? 1 : 0;
    g->nodes_dirty = true;
    return LOM_OK;
}

int lom_graph_optimize(lom_graph *g, const lom_graph_params *params, lom_graph_stats *stats)
{
    if (!g || !params) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(g->lock);
    if (!graph::params_ok(params))
        return fail(g, LOM_ERR_ARG, "lambda0, gtol, xtol, pcg_rtol finite and > 0; max_outer, max_pcg > 0");
    int64_t bad = -1;
    if (graph::check_gauge((int64_t)g->n(), g->fixed.data(), (int64_t)g->m(), g->ij.data(), &bad) != LOM_OK)
        return fail(g, LOM_ERR_ARG, ("gauge: the component of free node " + std::to_string(bad) + " holds no fixed node").c_str());
    lom_graph_stats st;
    std::memset(&st, 0, sizeof st);
    st.lambda_final = params->lambda0;
    st.stop_reason = LOM_GRAPH_STOP_GRADIENT;
    if (g->m() == 0) {  // nothing to weigh: cost 0, gradient 0
        if (stats) *stats = st;
        return LOM_OK;
    }
    LOM_HIP(g, hipSetDevice(g->device));
    int rc = sync_device(g);
    if (rc != LOM_OK) return rc;
    const uint32_t n = (uint32_t)g->n(), m = (uint32_t)g->m();
    double lambda = params->lambda0, nu = 2.0;
    bool linearise = true, first = true;
    for (;;) {
        // one outer iteration, enqueued whole: [linearise,] gather, the PCG chain, the candidate and its cost, the report
        if (linearise) rc = enqueue_linearise(g);
        if (rc == LOM_OK) rc = enqueue_gather(g, lambda);
        if (rc == LOM_OK) rc = enqueue_pcg(g, lambda, params);
        if (rc != LOM_OK) return rc;
        hipLaunchKernelGGL(k_graph_retract_cost, dim3(blocks_of(std::max(n, m), kGraphThreads)), dim3(kGraphThreads), 0,
                           g->stream, n, m, g->dev<const double>(G_POSE), g->dev<const int32_t>(G_FIXED),
                           g->dev<const double>(G_X), g->dev<double>(G_CAND), g->dev<const int32_t>(G_IJ),
                           g->dev<const double>(G_Z), g->dev<const double>(G_U), g->dev<const double>(G_DELTA),
                           g->dev<double>(G_COSTC));
        LOM_HIP(g, hipGetLastError());
        if ((rc = enqueue_report(g, lambda, 1)) != LOM_OK) return rc;
        LOM_HIP(g, hipStreamSynchronize(g->stream));  // the one wait of this outer iteration
        const GraphReport rep = *g->h_report;
        if (first) st.cost_initial = rep.cost;
        first = false;
        st.cost_final = rep.cost, st.grad_max = rep.grad_max, st.lambda_final = lambda;
        if (rep.grad_max <= params->gtol) {  // the poses in hand are the answer; the step solved beside the check is dropped
            st.stop_reason = LOM_GRAPH_STOP_GRADIENT;
            break;
        }
        if (st.outer == params->max_outer) {
            st.stop_reason = LOM_GRAPH_STOP_MAX_OUTER;
            break;
        }
        st.outer++;
        st.pcg_total += rep.pcg_iters;
        if (rep.pcg_done == 0) st.pcg_capped++;
        double rho_gain = 0.0;
        const int accepted = lom_graph_lm_policy(rep.cost, rep.cost_new, rep.denom, &lambda, &nu, &rho_gain);
        st.lambda_final = lambda;
        if (accepted) {
            std::swap(g->buf[G_POSE], g->buf[G_CAND]);
            st.accepted++;
        }
        linearise = accepted != 0;
        if (rep.step_max <= params->xtol) {
            st.stop_reason = LOM_GRAPH_STOP_STEP;
            if (accepted) {  // cost and gradient at the poses the step led to
                if ((rc = evaluate_now(g, lambda)) != LOM_OK) return rc;
                st.cost_final = g->h_report->cost, st.grad_max = g->h_report->grad_max;
            }
            break;
        }
    }
    LOM_HIP(g, hipMemcpyAsync(g->poses.data(), g->buf[G_POSE].p, (size_t)n * 56, hipMemcpyDeviceToHost, g->stream));
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    if (stats) *stats = st;
    return LOM_OK;
}

int lom_graph_evaluate(lom_graph *g, double lambda, double *e_out, double *w_out, double *cost_out, double *g_out,
                       double *hdiag_out)
{
    if (!g || !std::isfinite(lambda) || lambda < 0.0) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(g->lock);
    const size_t n = g->n(), m = g->m();
    if (cost_out) *cost_out = 0.0;
    if (n == 0) return LOM_OK;
    if (m == 0) {  // no edge: every sum is empty
        if (g_out) std::memset(g_out, 0, n * 48);
        if (hdiag_out) std::memset(hdiag_out, 0, n * 288);
        return LOM_OK;
    }
    LOM_HIP(g, hipSetDevice(g->device));
    int rc = sync_device(g);
    if (rc == LOM_OK) rc = evaluate_now(g, lambda);
    if (rc != LOM_OK) return rc;
    if (cost_out) *cost_out = g->h_report->cost;
    if (e_out) LOM_HIP(g, hipMemcpyAsync(e_out, g->buf[G_E].p, m * 48, hipMemcpyDeviceToHost, g->stream));
    if (w_out) LOM_HIP(g, hipMemcpyAsync(w_out, g->buf[G_W].p, m * 8, hipMemcpyDeviceToHost, g->stream));
    if (g_out) LOM_HIP(g, hipMemcpyAsync(g_out, g->buf[G_G].p, n * 48, hipMemcpyDeviceToHost, g->stream));
    if (hdiag_out) LOM_HIP(g, hipMemcpyAsync(hdiag_out, g->buf[G_HD].p, n * 288, hipMemcpyDeviceToHost, g->stream));
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    return LOM_OK;
}

int lom_graph_debug_matvec(lom_graph *g, double lambda, const double *p, double *y_out)
{
    if (!g || !p || !y_out || !std::isfinite(lambda) || lambda < 0.0) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(g->lock);
    const size_t n = g->n(), m = g->m();
    if (n == 0) return LOM_OK;
    if (m == 0) {
        std::memset(y_out, 0, n * 48);
        return LOM_OK;
    }
    LOM_HIP(g, hipSetDevice(g->device));
    int rc = sync_device(g);
    if (rc == LOM_OK) rc = enqueue_linearise(g);
    if (rc == LOM_OK) rc = enqueue_gather(g, lambda);
    if (rc != LOM_OK) return rc;
    LOM_HIP(g, hipMemsetAsync(g->buf[G_SCAL].p, 0, sizeof(GraphScalars), g->stream));  // done = 0: the kernels run
    LOM_HIP(g, hipMemcpyAsync(g->buf[G_P].p, p, n * 48, hipMemcpyHostToDevice, g->stream));
    if ((rc = enqueue_matvec(g, lambda)) != LOM_OK) return rc;
    LOM_HIP(g, hipMemcpyAsync(y_out, g->buf[G_Y].p, n * 48, hipMemcpyDeviceToHost, g->stream));
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    return LOM_OK;
}

int lom_graph_edge_chi2(lom_graph *g, int64_t first, int64_t n, double *out)
{
    if (!g || first < 0 || n < 0 || (n && !out)) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(g->lock);
    if (first > (int64_t)g->m() || n > (int64_t)g->m() - first) return fail(g, LOM_ERR_ARG, "no edge with this id");
    if (n == 0) return LOM_OK;
    LOM_HIP(g, hipSetDevice(g->device));
    int rc = sync_device(g);
    if (rc == LOM_OK) rc = enqueue_linearise(g);
    if (rc != LOM_OK) return rc;
    LOM_HIP(g, hipMemcpyAsync(out, g->dev<double>(G_S) + first, (size_t)n * 8, hipMemcpyDeviceToHost, g->stream));
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    return LOM_OK;
}

}  // extern "C"
