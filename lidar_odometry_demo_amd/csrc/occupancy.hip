// Occupancy grid: every scan at its pose votes once per cell of a dense 2-D grid -- passed through, or hit -- and a rule on
// the two counts classifies free / occupied / unknown.  Definitions: include/lidar_odometry_amd.h ("occupancy grid");
// kernels: k_occupancy.hpp; host planning (parameter ranges, start cells, slices, boxes, step bound): occupancy_host.cpp;
// DESIGN.md 7j.  A handle family of its own beside the map path: the descriptors are the assembly's, the clouds an
// archive's or the caller's, and no default path launches any of this.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "archive_internal.hpp"
#include "k_occupancy.hpp"
#include "occupancy_host.hpp"

using namespace lom;

// The grid owns its stream and every buffer below.  free / seen hold the counts; the bitmaps are scratch at rest (zero)
// between calls.
struct lom_occupancy : lom::DeviceHandle {
    lom_occupancy_geometry geo{};
    lom::DeviceBuf free_votes, seen_votes;  // width * height u32 each
    lom::DeviceBuf bitmaps;                 // [scan of a slice][pass, hit][row][word], grow-only
    lom::DeviceBuf desc, cells, words;      // descriptors and start cells of a call; the status words
    lom::DeviceBuf cloud;                   // a host cloud on its way in, packed
    lom::DeviceBuf cls;                     // the classification, int8 per cell
    lom::PinnedBuf h_words;                 // the status words on their way out
    hipEvent_t done_ev = nullptr;           // recorded behind a call's kernels, for the archive's stream to wait on
    uint32_t test_slice_max = 0;            // LOM_OCC_OPT_TEST_SLICE_MAX
    uint32_t window = occupancy::kWindowMax;  // LOM_OCC_OPT_TEST_WINDOW

    size_t n_cells() const { return (size_t)geo.width * geo.height; }
};

namespace {

thread_local std::string g_occupancy_create_error;

bool stride_ok(size_t stride) { return stride >= 12 && (stride & 3) == 0; }

// Every slice's walk and fold, then the one read-back: the status words.  xyz: device memory, records of stride_floats;
// the caller has ordered g->stream behind whoever produced it.
int run(lom_occupancy *g, const occupancy::Plan &plan, const float *xyz, uint32_t stride_floats,
        const lom_occupancy_ray_params &p, lom_occupancy_stats &st)
{
    int rc;
    const std::vector<assemble::AsmScan> &scans = plan.scans.scans;
    uint32_t s_max = 0;
    for (const occupancy::Slice &s : plan.slices) s_max = std::max(s_max, s.count);
    const size_t map_words = occupancy::map_words(g->geo);
    // grow-only and at rest: a fresh block is zeroed once, in stream order before its first use
    const size_t bm_bytes = (size_t)s_max * 2 * map_words * 4;
    if (bm_bytes > g->bitmaps.bytes) {
        if ((rc = ensure(g, g->bitmaps, bm_bytes)) != LOM_OK) return rc;
        LOM_HIP(g, hipMemsetAsync(g->bitmaps.p, 0, g->bitmaps.bytes, g->stream));
    }
    const size_t desc_bytes = scans.size() * sizeof(assemble::AsmScan), cell_bytes = plan.cells.size() * 4;
    if ((rc = ensure(g, g->desc, desc_bytes)) != LOM_OK) return rc;
    if ((rc = ensure(g, g->cells, cell_bytes)) != LOM_OK) return rc;
    LOM_HIP(g, hipMemsetAsync(g->words.p, 0, (size_t)OW_COUNT * 4, g->stream));
    // (the plan outlives the copies: the call waits for the stream before it returns)
    LOM_HIP(g, hipMemcpyAsync(g->desc.p, scans.data(), desc_bytes, hipMemcpyHostToDevice, g->stream));
    LOM_HIP(g, hipMemcpyAsync(g->cells.p, plan.cells.data(), cell_bytes, hipMemcpyHostToDevice, g->stream));
    OccArgs a;
    a.resolution = g->geo.resolution, a.origin_x = g->geo.origin_x, a.origin_y = g->geo.origin_y;
    a.width = g->geo.width, a.height = g->geo.height, a.wpr = occupancy::words_per_row(g->geo.width);
    a.z_lo = p.z_lo, a.z_hi = p.z_hi, a.margin = p.margin, a.min_range = p.min_range, a.max_range = p.max_range;
    a.max_steps = occupancy::max_steps(p.max_range, g->geo.resolution);
    a.window = g->window;
    a.stride = stride_floats;
    const size_t lds = (size_t)g->window * g->window / 8;
    for (const occupancy::Slice &s : plan.slices) {
        hipLaunchKernelGGL(k_occ_walk, dim3(s.grid_x, s.count), dim3(kAsmThreads), lds, g->stream,
                           g->desc.as<const AsmScan>() + s.first, g->cells.as<const int32_t>() + (size_t)s.first * 2, xyz, a,
                           g->bitmaps.as<uint32_t>(), g->words.as<uint32_t>());
        LOM_HIP(g, hipGetLastError());
        if (!s.box.empty()) {
            const uint32_t wx0 = s.box.x0 / 32u, wx1 = (s.box.x1 + 31u) / 32u;
            const size_t threads = (size_t)(wx1 - wx0) * 32u * (s.box.y1 - s.box.y0);
            hipLaunchKernelGGL(k_occ_fold, dim3((uint32_t)((threads + kOccThreads - 1) / kOccThreads)), dim3(kOccThreads), 0,
                               g->stream, g->bitmaps.as<uint32_t>(), s.count, a.width, a.height, a.wpr, wx0, wx1, s.box.y0,
                               s.box.y1, g->free_votes.as<uint32_t>(), g->seen_votes.as<uint32_t>());
            LOM_HIP(g, hipGetLastError());
        }
    }
    LOM_HIP(g, hipMemcpyAsync(g->h_words.h, g->words.p, (size_t)OW_COUNT * 4, hipMemcpyDeviceToHost, g->stream));
    LOM_HIP(g, hipEventRecord(g->done_ev, g->stream));
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    const uint32_t *got = g->h_words.as<uint32_t>();
    st.rays_walked = (uint64_t)got[OW_WALKED] | ((uint64_t)got[OW_WALKED + 1] << 32);
    st.rays_skipped = plan.scans.points_in - st.rays_walked;
    st.cells_visited = (uint64_t)got[OW_VISITED] | ((uint64_t)got[OW_VISITED + 1] << 32);
    st.endpoints_marked = (uint64_t)got[OW_MARKED] | ((uint64_t)got[OW_MARKED + 1] << 32);
    return LOM_OK;
}

// one scan that is not in an archive: a table of one entry, id 0
int plan_cloud(lom_occupancy *g, size_t n, const lom_graph_pose *pose, const lom_occupancy_ray_params *p, occupancy::Plan &plan)
{
    if (n > assemble::kAsmMaxPoints) return fail(g, LOM_ERR_ARG, "occupancy: more than 2^31 - 2 points in one cloud");
    const assemble::ScanEntry e{0, (uint32_t)n};
    const int64_t id = 0;
    std::string why;
    const int rc = occupancy::plan(&e, 1, &id, pose, 1, g->geo, p, g->test_slice_max, plan, why);
    return rc == LOM_OK ? LOM_OK : fail(g, rc, ("occupancy: " + why).c_str());
}

int classify_on_device(lom_occupancy *g, const lom_occupancy_rule *rule)
{
    if (!occupancy::rule_ok(rule)) return fail(g, LOM_ERR_ARG, "occupancy rule: min_free_scans >= 1, min_seen_scans >= 1");
    LOM_HIP(g, hipSetDevice(g->device));
    const uint32_t n = (uint32_t)g->n_cells();
    LOM_HIP(g, hipMemsetAsync(g->words.p, 0, (size_t)OC_COUNT * 4, g->stream));
    hipLaunchKernelGGL(k_occ_classify, dim3((n + kOccThreads - 1) / kOccThreads), dim3(kOccThreads), 0, g->stream,
                       g->free_votes.as<const uint32_t>(), g->seen_votes.as<const uint32_t>(), n, rule->min_free_scans,
                       rule->free_per_seen, rule->min_seen_scans, g->cls.as<int8_t>(), g->words.as<uint32_t>());
    LOM_HIP(g, hipGetLastError());
    return LOM_OK;
}

}  // namespace

extern "C" {

int lom_occupancy_create(const lom_occupancy_geometry *geometry, int device, lom_occupancy **out)
{
    if (!out) return LOM_ERR_ARG;
    *out = nullptr;
    if (!occupancy::geometry_ok(geometry))
        return create_fail(g_occupancy_create_error, LOM_ERR_ARG,
                           "occupancy geometry: resolution > 0 and finite, a finite origin, 1 <= width, height <= 16384");
    if (const int rc = check_device(device, g_occupancy_create_error); rc != LOM_OK) return rc;
    lom_occupancy *g = new (std::nothrow) lom_occupancy();
    if (!g) return create_fail(g_occupancy_create_error, LOM_ERR_OOM, "host allocation");
    g->device = device;
    g->geo = *geometry;
    const size_t count_bytes = g->n_cells() * 4;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&g->done_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = alloc(g->h_words, 64, hipHostMallocDefault);
    int rc = e == hipSuccess ? LOM_OK : create_fail(g_occupancy_create_error, LOM_ERR_HIP, "occupancy grid setup", e);
    if (rc == LOM_OK && (alloc(g->free_votes, count_bytes) != hipSuccess || alloc(g->seen_votes, count_bytes) != hipSuccess ||
                         alloc(g->cls, g->n_cells()) != hipSuccess || alloc(g->words, 64) != hipSuccess))
        rc = create_fail(g_occupancy_create_error, LOM_ERR_OOM, "hipMalloc (occupancy grid)");
    if (rc == LOM_OK) {
        e = hipMemsetAsync(g->free_votes.p, 0, count_bytes, g->stream);
        if (e == hipSuccess) e = hipMemsetAsync(g->seen_votes.p, 0, count_bytes, g->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
        if (e != hipSuccess) rc = create_fail(g_occupancy_create_error, LOM_ERR_HIP, "occupancy grid setup", e);
    }
    if (rc != LOM_OK) {
        lom_occupancy_destroy(g);
        return rc;
    }
    *out = g;
    return LOM_OK;
}

void lom_occupancy_destroy(lom_occupancy *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    if (g->done_ev) (void)hipEventDestroy(g->done_ev);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;  // the buffers go with it
}

const char *lom_occupancy_last_error(const lom_occupancy *g) { return g ? g->error.c_str() : g_occupancy_create_error.c_str(); }

int lom_occupancy_clear(lom_occupancy *g)
{
    if (!g) return LOM_ERR_ARG;
    LOM_HIP(g, hipSetDevice(g->device));
    LOM_HIP(g, hipMemsetAsync(g->free_votes.p, 0, g->n_cells() * 4, g->stream));
    LOM_HIP(g, hipMemsetAsync(g->seen_votes.p, 0, g->n_cells() * 4, g->stream));
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    return LOM_OK;
}

int lom_occupancy_get_geometry(const lom_occupancy *g, lom_occupancy_geometry *out)
{
    if (!g || !out) return LOM_ERR_ARG;
    *out = g->geo;
    return LOM_OK;
}

void *lom_occupancy_stream(lom_occupancy *g) { return g ? (void *)g->stream : nullptr; }
int lom_occupancy_device(const lom_occupancy *g) { return g ? g->device : LOM_ERR_ARG; }

int lom_occupancy_wait_event(lom_occupancy *g, void *hip_event)
{
    if (!g || !hip_event) return LOM_ERR_ARG;
    LOM_HIP(g, hipSetDevice(g->device));
    LOM_HIP(g, hipStreamWaitEvent(g->stream, (hipEvent_t)hip_event, 0));
    return LOM_OK;
}

int lom_occupancy_set_option(lom_occupancy *g, int option, int64_t value)
{
    if (!g) return LOM_ERR_ARG;
    switch (option) {
    case LOM_OCC_OPT_TEST_SLICE_MAX:
        if (value < 0 || value > (int64_t)occupancy::kSliceScans) return fail(g, LOM_ERR_ARG, "LOM_OCC_OPT_TEST_SLICE_MAX: 0 .. 64");
        g->test_slice_max = (uint32_t)value;
        return LOM_OK;
    case LOM_OCC_OPT_TEST_WINDOW:
        if (value > (int64_t)occupancy::kWindowMax || (value > 0 && (value & 31)))
            return fail(g, LOM_ERR_ARG, "LOM_OCC_OPT_TEST_WINDOW: a multiple of 32 up to 512, 0, or < 0 for the default");
        g->window = value < 0 ? occupancy::kWindowMax : (uint32_t)value;
        return LOM_OK;
    default:
        return fail(g, LOM_ERR_ARG, "unknown occupancy option");
    }
}

int lom_occupancy_integrate(lom_occupancy *g, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses, size_t count,
                            const lom_occupancy_ray_params *p, lom_occupancy_stats *stats)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (!g || !a) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(a->lock);
    if (g->device != a->device) return fail(g, LOM_ERR_ARG, "occupancy: the grid and the archive live on different devices");
    occupancy::Plan plan;
    std::string why;
    int rc = occupancy::plan(a->table.data(), a->table.size(), ids, poses, count, g->geo, p, g->test_slice_max, plan, why);
    if (rc != LOM_OK) return fail(g, rc, ("occupancy: " + why).c_str());
    lom_occupancy_stats st;
    std::memset(&st, 0, sizeof st);
    st.scans = count;
    if (!plan.slices.empty()) {
        LOM_HIP(g, hipSetDevice(g->device));
        // the archive's clouds are complete when its stream is (an add waits for its own copy; this orders the rest)
        LOM_HIP(g, hipEventRecord(a->ready_ev, a->stream));
        LOM_HIP(g, hipStreamWaitEvent(g->stream, a->ready_ev, 0));
        if ((rc = run(g, plan, a->d_xyz(), 3, *p, st)) != LOM_OK) return rc;
        // and what the archive does next comes behind this call's reads
        LOM_HIP(g, hipStreamWaitEvent(a->stream, g->done_ev, 0));
    }
    if (stats) *stats = st;
    return LOM_OK;
}

int lom_occupancy_integrate_cloud_device(lom_occupancy *g, const float *d_xyz, size_t n, size_t stride_bytes,
                                         const lom_graph_pose *pose, const lom_occupancy_ray_params *p, void *hip_event_or_null,
                                         lom_occupancy_stats *stats)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (!g) return LOM_ERR_ARG;
    if ((n && !d_xyz) || !pose || !stride_ok(stride_bytes))
        return fail(g, LOM_ERR_ARG, "occupancy: a cloud, a pose and a stride >= 12 that is a multiple of 4");
    occupancy::Plan plan;
    int rc = plan_cloud(g, n, pose, p, plan);
    if (rc != LOM_OK) return rc;
    lom_occupancy_stats st;
    std::memset(&st, 0, sizeof st);
    st.scans = 1;
    if (!plan.slices.empty()) {
        LOM_HIP(g, hipSetDevice(g->device));
        if (hip_event_or_null) LOM_HIP(g, hipStreamWaitEvent(g->stream, (hipEvent_t)hip_event_or_null, 0));
        if ((rc = run(g, plan, d_xyz, (uint32_t)(stride_bytes / 4), *p, st)) != LOM_OK) return rc;
    }
    if (stats) *stats = st;
    return LOM_OK;
}

int lom_occupancy_integrate_cloud(lom_occupancy *g, const float *xyz, size_t n, size_t stride_bytes, const lom_graph_pose *pose,
                                  const lom_occupancy_ray_params *p, lom_occupancy_stats *stats)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (!g) return LOM_ERR_ARG;
    if ((n && !xyz) || !pose || !stride_ok(stride_bytes))
        return fail(g, LOM_ERR_ARG, "occupancy: a cloud, a pose and a stride >= 12 that is a multiple of 4");
    occupancy::Plan plan;
    int rc = plan_cloud(g, n, pose, p, plan);  // every refusal before the upload
    if (rc != LOM_OK) return rc;
    if (n) {
        LOM_HIP(g, hipSetDevice(g->device));
        if ((rc = ensure(g, g->cloud, n * 12)) != LOM_OK) return rc;
        if (stride_bytes == 12)
            LOM_HIP(g, hipMemcpyAsync(g->cloud.p, xyz, n * 12, hipMemcpyHostToDevice, g->stream));
        else
            LOM_HIP(g, hipMemcpy2DAsync(g->cloud.p, 12, xyz, stride_bytes, 12, n, hipMemcpyHostToDevice, g->stream));
    }
    return lom_occupancy_integrate_cloud_device(g, g->cloud.as<const float>(), n, 12, pose, p, nullptr, stats);
}

int64_t lom_occupancy_counts(lom_occupancy *g, uint32_t *free_out, uint32_t *seen_out, size_t cap)
{
    if (!g) return LOM_ERR_ARG;
    const size_t n = std::min(cap, g->n_cells());
    if (n && (free_out || seen_out)) {
        LOM_HIP(g, hipSetDevice(g->device));
        if (free_out) LOM_HIP(g, hipMemcpyAsync(free_out, g->free_votes.p, n * 4, hipMemcpyDeviceToHost, g->stream));
        if (seen_out) LOM_HIP(g, hipMemcpyAsync(seen_out, g->seen_votes.p, n * 4, hipMemcpyDeviceToHost, g->stream));
        LOM_HIP(g, hipStreamSynchronize(g->stream));
    }
    return (int64_t)g->n_cells();
}

int lom_occupancy_classify(lom_occupancy *g, const lom_occupancy_rule *rule, int8_t *out, size_t cap,
                           lom_occupancy_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!g || (cap && !out)) return LOM_ERR_ARG;
    const int rc = classify_on_device(g, rule);
    if (rc != LOM_OK) return rc;
    const size_t n = std::min(cap, g->n_cells());
    if (n) LOM_HIP(g, hipMemcpyAsync(out, g->cls.p, n, hipMemcpyDeviceToHost, g->stream));
    LOM_HIP(g, hipMemcpyAsync(g->h_words.h, g->words.p, (size_t)OC_COUNT * 4, hipMemcpyDeviceToHost, g->stream));
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    if (summary) {
        const uint32_t *t = g->h_words.as<uint32_t>();
        summary->cells_free = t[OC_FREE], summary->cells_occupied = t[OC_OCCUPIED], summary->cells_unknown = t[OC_UNKNOWN];
    }
    return LOM_OK;
}

int lom_occupancy_classify_device(lom_occupancy *g, const lom_occupancy_rule *rule, const int8_t **d_out)
{
    if (!g || !d_out) return LOM_ERR_ARG;
    *d_out = nullptr;
    const int rc = classify_on_device(g, rule);
    if (rc != LOM_OK) return rc;
    *d_out = g->cls.as<const int8_t>();
    return LOM_OK;
}

}  // extern "C"
