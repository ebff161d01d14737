// Scan-matching kernels: the MI355X counterpart of
//   VoxelGrid::getCorrespondence / findMatchingPairs  (src/voxel_grid.h:164-234)
//   PointToPlaneErrorAnalytic::Evaluate               (src/cloud_matcher.cpp:38-103)
// plus the reduction of the robustified normal equations that Ceres performs
// inside ceres::Solve (DENSE_QR) for the reference.
//
//   k_match   per source point: f64 transform -> f32 query -> 27-neighbour
//             voxel lookup -> nearest stored point (strict-min, scan order
//             ix,iy,iz then insertion order) -> winner's point+normal.
//             A gather that is VALU-issue- and latency-bound at scan sizes;
//             no MFMA (nothing here is a contraction).
//   k_lm      single GPU: one whole ceres::Solve per launch.  Per evaluation and valid
//             correspondence: r = (q*p + t - o).n, 1x6 tangent Jacobian, Huber(0.15) IRLS
//             weight; f64 reduction of sum w J J^T (21), sum w J r (6), sum 0.5 rho (1) per
//             workgroup, exchange between the workgroups through HBM, then the
//             Levenberg-Marquardt policy of lm_core.hpp on one wave.  The pose of the next
//             k_match travels through AlignState in HBM: no host round trip inside an align.
//   k_eval_server / k_eval
//             the same evaluation for the host-driven loop (ranks that exchange sums,
//             LOM_HOST_LM=1): the <= 64 records land in pinned host memory and the host adds
//             them in workgroup order, or stay in HBM for the RCCL all-gather.
//
//   k_quality the quality report of a pose (lom_match_quality*): one more evaluation over a search's records -- the
//             align's 28 sums plus weights, residual statistics and counts -- reduced in a fixed order.
//             k_quality_batch / k_quality_batch_sum: the same for the K (scan, pose) problems of a round of
//             lom_match_quality_batch*, blockIdx.y the problem, behind the batch form of k_match.
//
// The kernels live in k_match.hpp, k_eval.hpp, k_lm.hpp, k_quality.hpp and k_policy_probe.hpp (a test probe); this file is the one translation unit that instantiates
// and launches them: the kernel tables, the chained single and batched align, the host-driven path, the C entry points.
//
// Built with -ffp-contract=off (see voxel_map.hip).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <vector>

#include "k_eval.hpp"
#include "k_lm.hpp"
#include "k_match.hpp"
#include "k_policy_probe.hpp"
#include "k_quality.hpp"
#include "lm_core.hpp"
#include "lm_wave.hpp"
#include "lom_internal.hpp"
#include "pose_math.hpp"

namespace lom {

// max_sq: the f32 threshold the f32 squared distances are compared with (strictly below).  findMatchingPairs forms it
// as max_dist * max_dist in f32 (voxel_grid.h:215); getCorrespondence takes a double (:164), see threshold_f32()
static void pose_args(const float t[3], const float q[4], float max_sq, PoseArgs &P)
{
    float R[9];
    rotation_matrix(q, R);  // voxel_grid.h:212 transform.rotationMatrix().cast<double>()
    for (int i = 0; i < 9; i++) P.R[i] = (double)R[i];
    for (int i = 0; i < 3; i++) P.t[i] = (double)t[i];
    P.max_sq = max_sq;
}

// a scan as the entry points take it: a stride that holds three floats and keeps them aligned, a count k_match's 32-bit
// indices cover
constexpr size_t kMaxScanPoints = 0x7FFFFFFFull;
static inline bool stride_ok(size_t stride) { return stride >= 12 && !(stride & 3); }
static inline bool scan_args_ok(size_t n, size_t stride) { return stride_ok(stride) && n < kMaxScanPoints; }

static inline float sq_f32(float max_dist) { return max_dist * max_dist; }  // voxel_grid.h:215

// voxel_grid.h:184-186 compares the f32 squared norm, widened to double, with a double threshold: (double)d2 < max_sq.
// For f32 d2 that is d2 < the smallest f32 that is >= max_sq (equal to max_sq where that is an f32 value itself, as
// findMatchingPairs' always is): the kernel's f32 compare with THAT threshold decides every case the same way.
static inline float threshold_f32(double max_sq)
{
    if (!(max_sq > 0.0)) return 0.f;                 // nothing is < 0 (NaN: every compare false)
    if (max_sq >= (double)FLT_MAX) return INFINITY;  // every finite d2 passes (an infinite d2 does only below an infinite threshold: not reproduced)
    float f = (float)max_sq;                         // round to nearest
    if ((double)f < max_sq) f = std::nextafterf(f, INFINITY);
    return f;
}

constexpr uint32_t kMaxMatchBlocks = 256u * (uint32_t)kMatchMinWaves;  // one resident round: kMatchMinWaves workgroups of 4 waves per CU
// (a context on a partition of the GPU: one resident round of ITS compute units)
static uint32_t match_grid(uint32_t n, uint32_t partition_cus = 0)
{
    const uint32_t per_block = (uint32_t)(kMatchThreads / kMatchG);
    const uint32_t need = (n + per_block - 1) / per_block;
    const uint32_t cap = partition_cus ? partition_cus * (uint32_t)kMatchMinWaves : kMaxMatchBlocks;
    return std::max(1u, std::min(need, cap));
}

constexpr uint32_t kMaxEvalBlocks = 64;  // records per launch (the host polls this many words)
static uint32_t eval_grid(uint32_t n)
{
    const uint32_t need = (n + kEvalThreads - 1) / kEvalThreads;
    return std::max(1u, std::min(need, kMaxEvalBlocks));
}

struct ScanCtx {
    lom_map *m;
    const char *d_src;
    size_t stride;
    uint32_t n;
    uint32_t match_blocks;
    // the records of a previous search of THIS scan against this map are at scan_on (outer iterations >= 2 of an align):
    // the next search may take its temporal pruning bound from them (k_match<..., kPrev>)
    bool have_prev = false;
    bool counted = false;  // the last launch produced the reference-algorithm counts
    int prof_used = 0;
    double launch_s = 0.0, wait_s = 0.0;  // host time inside launch calls / polling for results
};

static inline double now_s()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static int scan_buffers(lom_map *m, uint32_t n, bool want_stats)
{
    int rc;
    const size_t nn = std::max<uint32_t>(n, 1);
    if ((rc = ensure(m, m->scan_idx, nn * 4)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->scan_on, nn * sizeof(MatchRec))) != LOM_OK) return rc;
    if (want_stats && (rc = ensure(m, m->scan_stats, nn * sizeof(QStat))) != LOM_OK) return rc;
    if ((rc = ensure(m, m->partials, (size_t)kMaxEvalBlocks * kRecWords * 8)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->results, 1024 + (size_t)kMaxMatchBlocks * 16)) != LOM_OK) return rc;
    return LOM_OK;
}

static uint32_t *d_block_counters(lom_map *m) { return (uint32_t *)((char *)m->results.p + 1024); }
static double *d_sums(lom_map *m) { return (double *)m->results.p; }

static void server_stop(lom_map *m);

// The k_match instantiation of a launch (every instantiation has the same signature).
// <lanes per query, candidates per lane and trip, min waves per SIMD>: measured on C2 / C3
// (tools/ab_match.py): <16,1,8> 9.2 / 37.3 us, <16,2,1> 8.9 / 41.0, <16,4,1> 10.0 / 43.5,
// <16,2,8> and <16,4,8> spill and lose; 8 lanes per query 12.3 / 44.1, 32 lanes 10.1 / 44.5.
// Round 2 (query preparation split over the row's lanes, -15 % VALU instructions): 70 VGPRs, so 7 waves
// per SIMD and a grid capped at one resident round of that; held to 64 VGPRs it spills 4 and loses
// (C2 / C3 in the loop: 8.5 / 33.3 us at 7 waves, 9.3 / 36.5 at 8).  Four candidate loads in flight per lane
// (<16,4,4>, 74 VGPRs) on C2 / C3: 9.3 / 39.3 us -- it pays only where few waves share a SIMD (C5's 8k-point
// matching cloud: frame 0.329 -> 0.295 ms; eight in flight: the same).  With the candidate search at three
// LDS round trips instead of six (C2 / C3 / C4 8.3 / 33.9 / 58.1 -> 7.7 / 31.0 / 54.3 us, 68 VGPRs) two loads
// in flight fit the 7-wave budget (66 VGPRs): C2 the same, C3 31.6 -> 30.3 us.
// A small cloud leaves the SIMDs with two or three waves each: nothing hides a round trip, so each lane keeps
// four candidate loads in flight (<16,4,4>: 128-VGPR budget, one resident round up to 16384 queries).
using MatchKernel = decltype(&k_match<kMatchG, kMatchRows, kMatchMinWaves>);
static MatchKernel match_kernel(bool chained, bool prev, bool count, bool batch)
{
    constexpr int G = kMatchG, U = kMatchRows, W = kMatchMinWaves;
    // [chained][prev][count]; the batch form is always chained: [prev][count]
    static const MatchKernel single[8] = {
        k_match<G, U, W, false, false, false, false>, k_match<G, U, W, false, false, false, true>,
        k_match<G, U, W, false, false, true, false>,  k_match<G, U, W, false, false, true, true>,
        k_match<G, U, W, false, true, false, false>,  k_match<G, U, W, false, true, false, true>,
        k_match<G, U, W, false, true, true, false>,   k_match<G, U, W, false, true, true, true>};
    static const MatchKernel batched[4] = {
        k_match<G, U, W, false, true, false, false, true>, k_match<G, U, W, false, true, false, true, true>,
        k_match<G, U, W, false, true, true, false, true>,  k_match<G, U, W, false, true, true, true, true>};
    return batch ? batched[(prev ? 2 : 0) + (count ? 1 : 0)] : single[(chained ? 4 : 0) + (prev ? 2 : 0) + (count ? 1 : 0)];
}

// chained: the pose comes from the AlignState in HBM (t, q unused)
// count_mode: -1 = as the handle says (LOM_OPT_COUNT_CANDIDATES), 0 / 1 = without / with the reference-algorithm counts
static int launch_match(ScanCtx &c, const float t[3], const float q[4], float max_sq, bool stats,
                        bool chained = false, int count_mode = -1)
{
    lom_map *m = c.m;
    PoseArgs P;
    std::memset(&P, 0, sizeof P);
    if (!chained) pose_args(t, q, max_sq, P);
    c.match_blocks = c.n ? match_grid(c.n, m->stream == m->own_stream ? m->partition_cus : 0u) : 0;
    server_stop(m);  // the previous outer iteration's evaluation server leaves before the new search
    const double t_launch = now_s();
    if (c.n) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (m->profiling) {
            // three events per (k_match, k_lm) pair -- before, between, behind --, read back once at the end of the align
            while (m->prof_events.size() < (size_t)(c.prof_used + 1) * 3) {
                hipEvent_t e;
                LOM_HIP(m, hipEventCreate(&e));
                m->prof_events.push_back(e);
            }
            e0 = m->prof_events[(size_t)c.prof_used * 3];
            e1 = m->prof_events[(size_t)c.prof_used * 3 + 1];
            c.prof_used++;
            LOM_HIP(m, hipEventRecord(e0, m->stream));
        }
        QStat *st = (stats && !chained) ? (QStat *)m->scan_stats.p : (QStat *)nullptr;
        // (a chained launch always follows a search of the same scan: launch_pair's first pair is not chained)
        const bool prev = (chained || c.have_prev) && !m->opt_no_temporal;
        const bool count = count_mode < 0 ? m->opt_count : count_mode != 0;
        const AlignState *as = chained ? (const AlignState *)m->align_state.p : (const AlignState *)nullptr;
        hipLaunchKernelGGL(match_kernel(chained, prev, count, false), dim3(c.match_blocks), dim3(kMatchThreads), 0, m->stream,
                           view_of(m), c.d_src, c.stride, c.n, P, (int32_t *)m->scan_idx.p, (MatchRec *)m->scan_on.p, st,
                           d_block_counters(m), (unsigned long long *)nullptr, as, (const BatchProblem *)nullptr);
        LOM_HIP(m, hipGetLastError());
        c.counted = count;
        c.have_prev = true;
        if (m->profiling) LOM_HIP(m, hipEventRecord(e1, m->stream));
    }
    c.launch_s += now_s() - t_launch;
    return LOM_OK;
}

constexpr size_t kEvalLdsBytes = (size_t)28 * kAccStride * sizeof(double);
// Every in-kernel wait is bounded by the handle's patience (lom_map::patience_ticks, 50 ms unless
// LOM_OPT_DEVICE_PATIENCE_TICKS changed it; tests shorten it to exercise the give-up paths).

static int eval_kernel_attrs(lom_map *m)
{
    if (m->eval_attr_set) return LOM_OK;
    LOM_HIP(m, hipFuncSetAttribute(reinterpret_cast<const void *>(k_eval), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)kEvalLdsBytes));
    LOM_HIP(m, hipFuncSetAttribute(reinterpret_cast<const void *>(k_eval_server),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEvalLdsBytes));
    m->eval_attr_set = true;
    return LOM_OK;
}

// tell a resident evaluation server to leave (it exits within one poll of the command word)
static void server_stop(lom_map *m)
{
    if (!m->server_alive) return;
    EvalCmd *cmd = reinterpret_cast<EvalCmd *>(m->h_cmd);
    cmd->op = kCmdStop;
    __atomic_store_n(&cmd->seq, ++m->mail_seq, __ATOMIC_RELEASE);
    m->server_alive = false;
}

// wait for the nb records of evaluation `seq` and add them in workgroup order.
// returns LOM_OK, a negative status, or 1 when the stream went idle without the records
// (the server timed out and left; the caller relaunches)
static int collect_records(lom_map *m, uint32_t nb, unsigned long long seq, double out[LOM_NSUMS])
{
    uint64_t spins = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const double *rec = m->h_mail + (size_t)b * kRecWords;
        volatile const unsigned long long *flag = reinterpret_cast<volatile const unsigned long long *>(rec + 31);
        while (*flag != seq) {
            __builtin_ia32_pause();
            if ((++spins & 0x3FFF) == 0) {
                const hipError_t e = hipStreamQuery(m->stream);
                if (e == hipSuccess) {
                    if (*flag == seq) break;
                    return 1;
                } else if (e != hipErrorNotReady) {
                    return set_error(m, LOM_ERR_HIP, "stream failed while waiting for an evaluation", e);
                }
            }
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        for (int k = 0; k < 31; k++) out[k] += rec[k];
    }
    return LOM_OK;
}

// evaluation at (q,t) -> host sums (rank-local, or rank-ordered total with a communicator)
static int launch_eval(ScanCtx &c, const double q[4], const double t[3], bool fresh_match, double out[LOM_NSUMS])
{
    lom_map *m = c.m;
    EvalArgs E;
    for (int i = 0; i < 4; i++) E.q[i] = q[i];
    for (int i = 0; i < 3; i++) E.t[i] = t[i];
    const uint32_t nb = c.n ? eval_grid(c.n) : 0;
    const bool mailbox = (m->comm == nullptr);
    std::memset(out, 0, LOM_NSUMS * 8);
    int rc = eval_kernel_attrs(m);
    if (rc != LOM_OK) return rc;
    const double t_launch = now_s();
    if (!mailbox) {
        const unsigned long long seq = ++m->mail_seq;
        if (nb) {
            hipLaunchKernelGGL(k_eval, dim3(nb), dim3(kEvalThreads), kEvalLdsBytes, m->stream,
                               (const MatchRec *)m->scan_on.p, c.n, E, (const uint32_t *)d_block_counters(m),
                               fresh_match ? c.match_blocks : 0u, (double *)m->partials.p, seq);
        }
        hipLaunchKernelGGL(k_sum_records, dim3(1), dim3(64), 0, m->stream, (const double *)m->partials.p, nb, c.n,
                           d_sums(m));
        LOM_HIP(m, hipGetLastError());
        c.launch_s += now_s() - t_launch;
        const double t_wait = now_s();
        rc = ensure(m, m->gather, (size_t)m->nranks * LOM_NSUMS * 8);
        if (rc != LOM_OK) return rc;
        rc = comm_allgather_sums(m, d_sums(m), (double *)m->gather.p, LOM_NSUMS);
        if (rc != LOM_OK) return rc;
        LOM_HIP(m, hipMemcpyAsync(m->h_results, m->gather.p, (size_t)m->nranks * LOM_NSUMS * 8,
                                  hipMemcpyDeviceToHost, m->stream));
        LOM_HIP(m, hipStreamSynchronize(m->stream));
        for (int k = 0; k < LOM_NSUMS; k++) {
            double v = 0.0;
            for (int r = 0; r < m->nranks; r++) v += m->h_results[(size_t)r * LOM_NSUMS + k];  // rank order
            out[k] = v;
        }
        c.wait_s += now_s() - t_wait;
    } else if (nb) {
        for (int attempt = 0;; attempt++) {
            unsigned long long seq;
            const double t_l = now_s();
            if (fresh_match || !m->server_alive) {
                // (re)start the evaluation server of this outer iteration; its first evaluation is this one
                EvalCmd *cmd = reinterpret_cast<EvalCmd *>(m->h_cmd);
                seq = ++m->mail_seq;
                hipLaunchKernelGGL(k_eval_server, dim3(nb), dim3(kEvalThreads), kEvalLdsBytes, m->stream,
                                   (const MatchRec *)m->scan_on.p, c.n, E, (const uint32_t *)d_block_counters(m),
                                   fresh_match ? c.match_blocks : 0u, m->d_mail, seq,
                                   reinterpret_cast<const EvalCmd *>(m->d_cmd), (unsigned long long)cmd->seq,
                                   m->patience_ticks);
                LOM_HIP(m, hipGetLastError());
                m->server_alive = true;
            } else {
                EvalCmd *cmd = reinterpret_cast<EvalCmd *>(m->h_cmd);
                for (int a = 0; a < 4; a++) cmd->q[a] = q[a];
                for (int a = 0; a < 3; a++) cmd->t[a] = t[a];
                cmd->op = kCmdEval;
                seq = ++m->mail_seq;
                __atomic_store_n(&cmd->seq, seq, __ATOMIC_RELEASE);  // payload before the sequence word
            }
            const double t_w = now_s();
            c.launch_s += t_w - t_l;
            std::memset(out, 0, LOM_NSUMS * 8);
            rc = collect_records(m, nb, seq, out);
            c.wait_s += now_s() - t_w;
            if (m->opt_debug_timing)
                fprintf(stderr, "eval %s launch %.1f us wait %.1f us\n", fresh_match ? "fresh" : "fixed",
                        (t_w - t_l) * 1e6, (now_s() - t_w) * 1e6);
            if (rc == LOM_OK) break;
            if (rc < 0) return rc;
            m->server_alive = false;  // the server timed out and left (host was away > 50 ms): start another
            fresh_match = false;      // counters were already folded, or are folded again below
            if (attempt >= 3) return set_error(m, LOM_ERR_HIP, "evaluation server did not answer");
        }
        out[31] = (double)c.n;
    }
    // counters of the last k_match are summed on its first evaluation only
    if (fresh_match) {
        for (int k = 0; k < 4; k++) m->last_counters[k] = out[28 + k];
    } else {
        for (int k = 0; k < 3; k++) out[28 + k] = m->last_counters[k];
    }
    if (m->host_comm) {  // ranks of one node: the hosts exchange their 32 sums through shared memory
        double mine[LOM_NSUMS];
        std::memcpy(mine, out, sizeof mine);
        const double t_x = now_s();
        rc = host_exchange_sums(m, mine, out);
        c.wait_s += now_s() - t_x;
        if (rc != LOM_OK) return rc;
    }
    return LOM_OK;
}

static int hook_match_eval(void *user, const float pt[3], const float pq[4], const double q[4], const double t[3],
                           double out[LOM_NSUMS])
{
    ScanCtx &c = *(ScanCtx *)user;
    int rc = launch_match(c, pt, pq, sq_f32(0.3f), false);  // cloud_matcher.cpp:139
    if (rc != LOM_OK) return rc;
    return launch_eval(c, q, t, true, out);
}

static int hook_eval_fixed(void *user, const double q[4], const double t[3], double out[LOM_NSUMS])
{
    ScanCtx &c = *(ScanCtx *)user;
    return launch_eval(c, q, t, false, out);
}

static int hook_sums_exchanged(void *, double *, int) { return 0; }  // (launch_eval has exchanged them)

static P2pArgs p2p_args(const lom_map *m)
{
    P2pArgs A;
    for (int r = 0; r < kP2pMaxRanks; r++) A.peer[r] = m->p2p ? (XWord *)m->p2p_peer[r] : nullptr;
    A.rank = m->p2p ? m->rank : 0;
    A.nranks = m->p2p ? m->nranks : 1;
    A.set_base = 0;
    A.epoch = ~0ull;
    return A;
}

void p2p_detach(lom_map *m)
{
    if (!m->p2p_local) return;
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->stream);
    for (int r = 0; r < kP2pMaxRanks; r++) {
        if (m->p2p_peer[r] && m->p2p_peer[r] != m->p2p_local) (void)hipIpcCloseMemHandle(m->p2p_peer[r]);
        m->p2p_peer[r] = nullptr;
    }
    (void)hipFree(m->p2p_local);
    m->p2p_local = nullptr;
    m->p2p = false;
}

// Single GPU, no exchange: the outer loop runs on the device.  One (k_match, k_lm) pair per outer
// iteration; the pose travels from pair to pair through AlignState in HBM, so the host enqueues
// pairs without waiting for results (chain_start / chain_continue).

// Returned by align_chained when a workgroup of k_lm gave up waiting for the others (they are not all
// resident: a caller sharing the GPU, a CU mask) or for a peer rank: the caller redoes the align
// through the host-driven loop.
constexpr int kDeviceLoopGaveUp = 100;

// k_lm's workgroups wait for each other inside the kernel, so all of them must be resident at once:
// the grid never exceeds what the occupancy query admits on this device.
// Workgroup size: 256 threads for clouds that 64 such workgroups cover with one point per lane (<= 16,384 points) or
// with TWO points per lane, both in registers for the whole solve (<= 32,768: the VLP16 scan of C2), else 512:
// the wave-level reduction is bound by the CU's f64 issue rate, and four waves -- one per SIMD -- are through it
// in half the time of eight; the final sum adds 8 partial sums instead of 16; two register points per lane are
// accumulated stage by stage so that their independent chains interleave (1.4k cycles for the two against 0.95k for
// one).  C2 (profiles/r03_*): k_lm 18.9 -> 17.8 us per launch against 512 threads with one point per lane; eight
// points per lane (C3 on 64 workgroups of 256) lose: 24.4-25.5 against 22.4 us.
// Clouds beyond what 64 workgroups of 512 cover with two points per lane (C3, C4 on one GPU) take up to 128 workgroups:
// the accumulation halves, the gather reads twice as many records (on C2-sized clouds that trade loses).
// The 256-thread shapes launch one wave more, the policy wave (k_lm): nb and the point assignment count the 256 threads.
constexpr uint32_t kLmSmallThreads = 256;
constexpr uint32_t kLmSmallLaunch = (uint32_t)lm_threads((int)kLmSmallThreads);  // the point threads and the policy wave
enum LmShape { kLmSmall = 0, kLmMid = 1, kLmBig = 2, kLmSmall2 = 3 };
static LmShape lm_shape(uint32_t n)
{
    if (n <= kMaxLmBlocks * kLmSmallThreads) return kLmSmall;
    if (n <= 2u * kMaxLmBlocks * kLmSmallThreads) return kLmSmall2;  // 256 threads, two points per lane in registers
    // (for C3's 124k points 128 workgroups of 256 threads with four points per lane in registers -- no point re-read
    // per evaluation -- measured the same as 512 threads with one: align 0.2315-0.2324 against 0.2314-0.2335 ms on one
    // box; eight per lane for C4's 248k points lose, 0.448 against 0.343 ms: AGPR spills, eight points in a row)
    return n <= 2u * kMaxLmBlocks * (uint32_t)kEvalThreads ? kLmMid : kLmBig;
}

// What belongs to a shape: its geometry and its k_lm instantiations (every instantiation has the same signature).
using LmKernel = decltype(&k_lm<(int)kLmSmallThreads>);
struct LmForm {
    uint32_t points;   // point threads of a workgroup
    uint32_t threads;  // threads of a launch
    uint32_t cap;      // most workgroups of a solve
    LmKernel single;   // the single align's kernel
    LmKernel batch;    // the batched align's
    LmKernel twice;    // the single align's with the policy run twice (LOM_DEBUG_LM_TWICE=1; kLmSmall2 only)
};
static const LmForm &lm_form(LmShape shape)
{
    constexpr int S = (int)kLmSmallThreads, E = kEvalThreads, C = (int)kMaxLmBlocks, CB = (int)kMaxLmBlocksBig;
    static const LmForm forms[4] = {
        /* kLmSmall  */ {S, kLmSmallLaunch, C, k_lm<S>, k_lm<S, C, 1, false, true>, nullptr},
        /* kLmMid    */ {E, E, C, k_lm<E>, k_lm<E, C, 1, false, true>, nullptr},
        /* kLmBig    */ {E, E, CB, k_lm<E, CB>, k_lm<E, CB, 1, false, true>, nullptr},
        /* kLmSmall2 */ {S, kLmSmallLaunch, C, k_lm<S, C, 2>, k_lm<S, C, 2, false, true>, k_lm<S, C, 2, true>},
    };
    return forms[shape];
}

// compute units a launch of this handle reaches: its partition's where it has one
static int device_cus(lom_map *m, uint32_t *out)
{
    int cus = 0;
    LOM_HIP(m, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m->device));
    *out = m->partition_cus ? m->partition_cus : (uint32_t)std::max(1, cus);
    return LOM_OK;
}

static int lm_block_limit(lom_map *m, LmShape shape, uint32_t *out)
{
    uint32_t &cached = m->lm_max_blocks[shape];
    if (!cached) {
        const LmForm &f = lm_form(shape);
        int per_cu = 0, rc;
        uint32_t cus = 0;
        LOM_HIP(m, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(f.single),
                                                                (int)f.threads, 0));
        if ((rc = device_cus(m, &cus)) != LOM_OK) return rc;
        cached = (uint32_t)std::max(1, per_cu * (int)cus);
    }
    *out = cached;
    return LOM_OK;
}

// the grid of a solve: one point per point thread up to the shape's cap, and no more than is resident at once
static int lm_grid(lom_map *m, uint32_t n, LmShape shape, uint32_t *nb)
{
    const LmForm &f = lm_form(shape);
    uint32_t limit = 0;
    const int rc = lm_block_limit(m, shape, &limit);
    if (rc != LOM_OK) return rc;
    *nb = std::min(std::min(std::max(1u, (n + f.points - 1) / f.points), f.cap), limit);
    return LOM_OK;
}

// The initial guess of an align as the kernels take it: the first pose (cloud_matcher.cpp:107), the searches'
// max_correspondence_distance 0.3 squared in f32 (:139, voxel_grid.h:215) and the NormalPrior's anchor, the guess's
// translation (:153).
static void guess_fields(const float gt[3], const float gq[4], float (&t)[3], float (&q)[4], double (&prior_b)[3],
                         float &max_sq)
{
    for (int a = 0; a < 3; a++) t[a] = gt[a];
    for (int a = 0; a < 4; a++) q[a] = gq[a];
    for (int a = 0; a < 3; a++) prior_b[a] = (double)gt[a];
    max_sq = sq_f32(0.3f);
}
// the single align: k_lm's argument
static void set_guess(const float gt[3], const float gq[4], LmInit &init)
{
    guess_fields(gt, gq, init.t, init.q, init.prior_b, init.max_sq);
}
// the batched align: the problem's descriptor, and the AlignState its first search takes the pose from
static void set_guess(const float gt[3], const float gq[4], BatchProblem &d, AlignState &state)
{
    guess_fields(gt, gq, d.guess_t, d.guess_q, d.prior_b, d.max_sq);
    pose_args(gt, gq, d.max_sq, state.P);
    for (int a = 0; a < 3; a++) state.pose_t[a] = gt[a];
    for (int a = 0; a < 4; a++) state.pose_q[a] = gq[a];
}

// Wait until report `want` of a chain has arrived.  kReportArrived, kReportError (a workgroup gave up: the error word,
// seen before or with the report) or a negative status recorded with set_error (the stream ended or failed without
// either); the caller advances its sequence counter in every case.  An idle stream is looked at once more for the
// report OR the error word: the batched align needs both (a problem that gave up writes no further report), and for
// the single align it is the same as looking for the report alone, since its caller tests the error word first.
constexpr int kReportArrived = 0, kReportError = 1;
static int wait_report(lom_map *m, const volatile AlignReport *rp, unsigned long long want, const char *solve)
{
    uint64_t spins = 0;
    while (rp->seq != want) {
        __builtin_ia32_pause();
        if (rp->error) break;
        if ((++spins & 0x3FFF) == 0) {
            const hipError_t e = hipStreamQuery(m->stream);
            if (e == hipSuccess) {
                if (rp->seq == want || rp->error) break;
                return set_error(m, LOM_ERR_HIP, (std::string(solve) + " ended without a report").c_str());
            } else if (e != hipErrorNotReady) {
                return set_error(m, LOM_ERR_HIP, (std::string("stream failed during the ") + solve).c_str(), e);
            }
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return rp->error ? kReportError : kReportArrived;
}

// The chain of an align: cloud_matcher.cpp:169-172 cannot stop before the fifth outer iteration (i > 3), so kPairsAhead
// pairs go out at once, then one pair per report while anything is open, at most 35.
//   launch_pair(i)        enqueues the (k_match, k_lm) pair of outer iteration i
//   poll(launched, open)  waits for the reports of pair `launched` and says how many solves are still open
// Both return LOM_OK or what the chain is to return at once; `launched` is kept for the caller's sequence counter.
// chain_start sends the first pairs, chain_continue does the rest (what a caller does between the two runs while the
// device works).
template <class Pair>
static int chain_start(int &launched, Pair &&launch_pair)
{
    int rc;
    for (launched = 0; launched < kPairsAhead; launched++)
        if ((rc = launch_pair(launched)) != LOM_OK) return rc;
    return LOM_OK;
}
template <class Pair, class Poll>
static int chain_continue(int &launched, Pair &&launch_pair, Poll &&poll)
{
    int rc;
    for (;;) {
        int open = 0;
        if ((rc = poll(launched, open)) != LOM_OK) return rc;
        if (open == 0 || launched >= 35) return LOM_OK;
        if ((rc = launch_pair(launched)) != LOM_OK) return rc;
        launched++;
    }
}

// an align's result from its final report
static void result_from_report(const volatile AlignReport *rp, bool counted, uint32_t nb, lom_align_result &r)
{
    lom_align_stats &st = r.stats;
    std::memset(&st, 0, sizeof st);
    st.outer_iterations = rp->outer_done;
    st.match_launches = rp->outer_done;
    st.lm_iterations = rp->lm_iterations;
    st.evaluations = rp->evaluations;
    st.valid_last = (int64_t)rp->valid_last;
    st.cand_total = (int64_t)rp->cand_total;
    st.occ_total = (int64_t)rp->occ_total;
    st.queries = (int64_t)rp->queries_total;
    // B(q) = 12 + 27*16 + 12*cand(q) + 12*valid(q) -- known only when the searches produced the counts
    st.algorithmic_bytes = counted ? 444.0 * rp->queries_total + 12.0 * rp->cand_total + 12.0 * rp->valid_total : 0.0;
    st.final_cost = rp->final_cost;
    st.last_step_norm = rp->last_step_norm;
    st.lm_workgroups = (int32_t)nb;
    float pq[4] = {rp->pose_q[0], rp->pose_q[1], rp->pose_q[2], rp->pose_q[3]};
    {   // cloud_matcher.cpp:175 rotation.normalize(), f32
        const float n2 = (pq[0] * pq[0] + pq[1] * pq[1]) + (pq[2] * pq[2] + pq[3] * pq[3]);
        const float nn = std::sqrt(n2);
        for (int a = 0; a < 4; a++) pq[a] = pq[a] / nn;
    }
    for (int a = 0; a < 3; a++) r.t[a] = rp->pose_t[a];
    for (int a = 0; a < 4; a++) r.q_wxyz[a] = pq[a];
}

// The event triples of a profiled align (launch_match: before, between and behind a pair), read once the stream is
// idle: k_match of the first `pairs`, k_lm of the first `lm_pairs` of them.
static void read_events(lom_map *m, int pairs, int lm_pairs, lom_align_stats &st)
{
    for (int i = 0; i < pairs; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, m->prof_events[(size_t)i * 3], m->prof_events[(size_t)i * 3 + 1]) == hipSuccess)
            st.match_kernel_ms += ms;
        if (i < lm_pairs &&
            hipEventElapsedTime(&ms, m->prof_events[(size_t)i * 3 + 1], m->prof_events[(size_t)i * 3 + 2]) == hipSuccess)
            st.lm_kernel_ms += ms;
    }
    st.profiled_launches = pairs;
}

static int align_chained(lom_map *m, const char *d_src, size_t n, size_t stride, const float guess_t[3],
                         const float guess_q[4], float out_t[3], float out_q[4], lom_align_stats *stats,
                         double *trace_out = nullptr, int trace_outer = 0)
{
    static_assert(offsetof(AlignReport, finished) == 8 && offsetof(AlignReport, outer_done) == 16 &&
                      offsetof(AlignReport, evaluations) == 24 && offsetof(AlignReport, pose_t) == 32 &&
                      offsetof(AlignReport, valid_last) == 64 && sizeof(AlignReport) <= 256,
                  "AlignReport is written as 64-bit words");
    int rc = scan_buffers(m, (uint32_t)n, false);
    if (rc != LOM_OK) return rc;
    if (!m->align_state.p) m->align_state_dirty = true;
    if ((rc = ensure(m, m->align_state, sizeof(AlignState))) != LOM_OK) return rc;
    if (m->align_state_dirty) {
        // a fresh allocation, or an align that ended in a give-up: its error flag must not be mistaken for this one's
        LOM_HIP(m, hipMemsetAsync(m->align_state.p, 0, sizeof(AlignState), m->stream));
        m->align_state_dirty = false;
    }
    if (!m->xrec.p) {
        const size_t bytes = (size_t)2 * kMaxLmBlocksBig * kRecWords * sizeof(XWord);
        if ((rc = ensure(m, m->xrec, bytes)) != LOM_OK) return rc;
        LOM_HIP(m, hipMemsetAsync(m->xrec.p, 0, bytes, m->stream));
    }
    if ((rc = eval_kernel_attrs(m)) != LOM_OK) return rc;
    ScanCtx c{m, d_src, stride, (uint32_t)n, 0};
    LmInit init;
    set_guess(guess_t, guess_q, init);
    // ranks of one node keep to 64 workgroups each: a shard is an eighth of the cloud, and ranks that share a GPU
    // (tests, rehearsals) must all be resident together
    LmShape shape = lm_shape(c.n);
    if (m->p2p && shape == kLmBig) shape = kLmMid;
    const LmForm &form = lm_form(shape);
    const LmKernel kernel = (m->opt_debug_lm_twice && form.twice) ? form.twice : form.single;
    uint32_t nb = 0;
    if ((rc = lm_grid(m, c.n, shape, &nb)) != LOM_OK) return rc;
    double *d_trace = nullptr;  // lom_debug_lm_trace: k_lm of outer iteration `trace_outer` records its evaluations
    if (trace_out) {
        if ((rc = ensure(m, m->dbg_trace, 201 * 8)) != LOM_OK) return rc;
        d_trace = (double *)m->dbg_trace.p;
        LOM_HIP(m, hipMemsetAsync(d_trace, 0, 201 * 8, m->stream));
    }
    volatile AlignReport *rp = reinterpret_cast<volatile AlignReport *>(m->h_report);
    rp->error = 0;
    const unsigned long long seq0 = m->report_seq;
    P2pArgs px = p2p_args(m);
    if (m->p2p) px.epoch = ++m->p2p_epoch;  // the same count on every rank: ranks issue the same sequence of aligns
    const int give_up_outer = m->test_give_up_outer;  // one shot
    m->test_give_up_outer = -1;
    unsigned long long *dbg = nullptr;  // LOM_OPT_DEBUG_LM_STAMPS: phase stamps of the last k_lm of the align
    if (m->opt_debug_lm) {
        if ((rc = ensure(m, m->dbg_stamps, 4096)) != LOM_OK) return rc;
        dbg = (unsigned long long *)m->dbg_stamps.p;
        LOM_HIP(m, hipMemsetAsync(dbg, 0, 40 * 8, m->stream));
    }
    // The replay fold (k_lm's tail, LOM_OPT_REPLAY_FOLD): on for the single align of one GPU -- with or without an exchange
    // attached, as long as it has one rank: nothing is exchanged then, and the align must not cost more for the
    // communicator being there.  Out of scope, and so off: ranks that exchange sums (px.nranks > 1: every rank would take
    // the same decision, but a disagreement is a hang) and the batched chains (kBatch compiles it out).  lom_debug_lm_trace runs the iteration it asks about, and so does an align with
    // LOM_OPT_TEST_GIVE_UP_AT_OUTER armed: the k_lm it names has to run to give up.  An align that carries the profiling
    // events (lom_map_set_profiling: every N-th) is a measurement of the kernels: each bracketed pair runs, so that
    // profiled_launches stays match_launches and no empty kernel enters match_kernel_ms / lm_kernel_ms.
    const unsigned long long fold_seq = (m->opt_replay_fold && px.nranks <= 1 && !trace_out && give_up_outer < 0 && !m->profiling)
                                            ? seq0 + (unsigned long long)kPairsAhead
                                            : 0ull;
    m->last_replayed = 0;
    int lm_events = 0;
    auto launch_pair = [&](int i) -> int {
        int r = launch_match(c, guess_t, guess_q, sq_f32(0.3f), false, i > 0);
        if (r != LOM_OK) return r;
        const double t_l = now_s();
        m->lm_seq += 8;  // a solve spends at most 5 evaluations
        px.set_base = (int)((m->lm_launches++ & 1ull) * 2ull);  // same launch count on every rank
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(form.threads), 0, m->stream, (const MatchRec *)m->scan_on.p, c.n,
                           (AlignState *)m->align_state.p, init, i == 0 ? 1 : 0, (const uint32_t *)d_block_counters(m),
                           c.match_blocks, (XWord *)m->xrec.p, m->lm_seq, reinterpret_cast<AlignReport *>(m->d_report),
                           seq0 + (unsigned long long)i + 1, fold_seq, m->patience_ticks, dbg, px,
                           (d_trace && i == trace_outer) ? d_trace : (double *)nullptr, i == give_up_outer ? 1 : 0,
                           (const BatchProblem *)nullptr);
        LOM_HIP(m, hipGetLastError());
        if (m->profiling && c.prof_used) {
            LOM_HIP(m, hipEventRecord(m->prof_events[(size_t)(c.prof_used - 1) * 3 + 2], m->stream));
            lm_events++;
        }
        c.launch_s += now_s() - t_l;
        return LOM_OK;
    };
    auto poll = [&](int launched, int &open) -> int {
        const double t_w = now_s();
        const unsigned long long want = seq0 + (unsigned long long)launched;
        const int w = wait_report(m, rp, want, "device solve");
        if (w != kReportArrived) m->report_seq = want;
        if (w < 0) return w;
        c.wait_s += now_s() - t_w;
        if (w == kReportError) {
            // the kernels still enqueued see the flag in AlignState and return at once
            (void)hipStreamSynchronize(m->stream);
            m->align_state_dirty = true;
            set_error(m, LOM_ERR_HIP, "device solve: a workgroup timed out waiting for the others");
            return kDeviceLoopGaveUp;
        }
        open = rp->finished ? 0 : 1;
        return LOM_OK;
    };
    int launched = 0;
    if ((rc = chain_start(launched, launch_pair)) != LOM_OK) return rc;
    // a caller that follows the align with radiusCleanup(result translation) (lidar_odometry.cpp:65-67) has said so: the
    // cleanup's scan goes out behind the pairs (an align that needs more than these finds it undone and scans later)
    if (m->spec_radius > 0.f && !m->p2p && !trace_out && !dbg) cleanup_scan_behind_align(m);
    m->spec_radius = 0.f;
    if (m->idle_hook) {  // the caller's own work for the ~0.1 ms this thread would only watch the report
        void (*fn)(void *) = m->idle_hook;
        m->idle_hook = nullptr;
        const double t_h = now_s();
        fn(m->idle_user);
        c.launch_s += now_s() - t_h;
    }
    if ((rc = chain_continue(launched, launch_pair, poll)) != LOM_OK) return rc;
    m->report_seq = seq0 + (unsigned long long)launched;
    lom_align_result res;
    result_from_report(rp, c.counted, nb, res);
    m->last_replayed = (int)rp->replayed;
    lom_align_stats &st = res.stats;
    for (int a = 0; a < 3; a++) out_t[a] = res.t[a];
    for (int a = 0; a < 4; a++) out_q[a] = res.q_wxyz[a];
    if (m->profiling && c.prof_used) {
        LOM_HIP(m, hipStreamSynchronize(m->stream));
        // kernels enqueued beyond the end of the loop return at once: only the executed iterations count -- those the
        // replay fold accounted for were not executed
        const int executed = std::min(c.prof_used, (int)rp->outer_done - (int)rp->replayed);
        read_events(m, executed, std::min(executed, lm_events), st);
        st.lm_profiled_launches = std::min(executed, lm_events);
    }
    st.host_launch_ms = c.launch_s * 1e3;
    st.host_wait_ms = c.wait_s * 1e3;
    if (stats) *stats = st;
    if (trace_out) {
        LOM_HIP(m, hipMemcpyAsync(trace_out, d_trace, 201 * 8, hipMemcpyDeviceToHost, m->stream));
        LOM_HIP(m, hipStreamSynchronize(m->stream));
    }
    if (dbg) {
        unsigned long long h[40];
        LOM_HIP(m, hipMemcpyAsync(h, dbg, sizeof h, hipMemcpyDeviceToHost, m->stream));
        LOM_HIP(m, hipStreamSynchronize(m->stream));
        fprintf(stderr, "k_lm eval 1 reduce+exchange: LDS rows %llu, publish %llu, gather %llu, final sum %llu cycles\n",
                h[33] - h[32], h[34] - h[33], h[35] - h[34], h[36] - h[35]);
        for (int ev = 0; ev < 5 && h[ev * 5]; ev++)
            fprintf(stderr, "k_lm eval %d: at %llu: accumulate %llu reduce+exchange %llu policy %llu cycles\n", ev,
                    h[ev * 5] - h[0], h[ev * 5 + 1] - h[ev * 5], h[ev * 5 + 3] - h[ev * 5 + 1],
                    h[ev * 5 + 4] - h[ev * 5 + 3]);
    }
    return LOM_OK;
}

static int align_device_paths(lom_map *m, const char *d_src, size_t n, size_t stride, const float guess_t[3],
                              const float guess_q[4], float out_t[3], float out_q[4], lom_align_stats *stats)
{
    if (n >= kMaxScanPoints) return set_error(m, LOM_ERR_ARG, "too many source points");
    {   // an insert nobody has looked at since (no lom_map_status): the search must see its points
        const int rcp = resolve_pending(m);
        if (rcp != LOM_OK) return rcp;
    }
    m->profiling = m->profile_period > 0 && (m->align_count++ % (unsigned)m->profile_period) == 0;
    bool fell_back = false;
    if (!m->comm && (!m->host_comm || m->p2p) && !m->opt_host_lm) {
        server_stop(m);
        int rc = align_chained(m, d_src, n, stride, guess_t, guess_q, out_t, out_q, stats);
        if (m->p2p) {
            // The ranks agree on the outcome of EVERY align, whatever happened on this one: a time-out that lands
            // on the last exchange of an align lets the peers that already hold all words finish with LOM_OK, and
            // a rank that gave up -- or failed for good -- must neither redo the align alone nor leave its peers
            // waiting (the host exchange pairs operations by its own counter only).  Two counts through the host
            // exchange: ranks that gave up (recoverable: everybody redoes the align over the host exchange) and
            // ranks that failed for good (nobody continues).  The deadline outlasts the device side: a rank can
            // be late by its kernels' patience for a peer rank, once per pair still enqueued at worst (the abort
            // words normally cut that to one patience), and an exchange nobody completes is ABANDONED, which
            // every late rank sees (comm.cpp) -- round 2's failure was a fixed 60 s here against 10 x 10 s there.
            const bool gave_up = rc == kDeviceLoopGaveUp, hard = rc != LOM_OK && !gave_up;
            double verdict[2] = {gave_up ? 1.0 : 0.0, hard ? 1.0 : 0.0};
            const double cross_s = (double)m->patience_ticks * 10.0 * 1e-8;
            const double deadline_s = 30.0 + 2.0 * (kPairsAhead + 1) * cross_s;
            if (host_comm_allreduce_deadline(m->host_comm, verdict, 2, deadline_s) != LOM_OK) {
                m->p2p = false;
                const std::string why = std::string("agreement after a device-to-device align failed: ") + host_comm_error(m->host_comm);
                return set_error(m, LOM_ERR_COMM, why.c_str());
            }
            if (verdict[1] != 0.0) {  // some rank cannot continue: the same for all
                m->p2p = false;
                (void)hipStreamSynchronize(m->stream);
                if (hard) return rc;
                return set_error(m, LOM_ERR_COMM, "a peer rank failed during a device-to-device align");
            }
            if (verdict[0] == 0.0) return LOM_OK;
            fprintf(stderr, "lidar_odometry_amd: device-to-device exchange given up on %d rank(s) (%s); rank %d redoes the align over the host exchange\n",
                    (int)verdict[0], gave_up ? m->last_error.c_str() : "a peer gave up", m->rank);
            (void)hipStreamSynchronize(m->stream);
            m->p2p = false;
        } else if (rc != kDeviceLoopGaveUp) {
            return rc;
        }
        // single GPU: k_lm's workgroups were not all resident within their patience (another process or
        // handle on the GPU, a CU mask): same align again through the host-driven loop, whose
        // workgroups never wait for each other
        m->last_error.clear();
        fell_back = true;
    }
    int rc = scan_buffers(m, (uint32_t)n, false);
    if (rc != LOM_OK) return rc;
    ScanCtx c{m, d_src, stride, (uint32_t)n, 0};
    lom_align_hooks hooks;
    hooks.user = &c;
    hooks.match_eval = hook_match_eval;
    hooks.eval_fixed = hook_eval_fixed;
    // the rank-ordered all-gather sits inside launch_eval.  With more than one rank the hook is there all the same, doing
    // nothing: the driver's replay fold (align_driver.cpp) is for aligns whose sums nobody exchanges
    hooks.allreduce = ((m->comm || m->host_comm) && m->nranks > 1) ? hook_sums_exchanged : nullptr;
    m->last_replayed = 0;
    lom_align_stats st;
    rc = lom_align_with_hooks(&hooks, guess_t, guess_q, out_t, out_q, &st);
    server_stop(m);
    if (!c.counted) st.algorithmic_bytes = 0.0;  // (SURVEY.md 8d's bytes need the counts: LOM_OPT_COUNT_CANDIDATES)
    if (rc != LOM_OK) {
        if (m->last_error.empty()) set_error(m, rc, "align failed");
        // ranks of one node: a rank that leaves the loop tells its peers (they would wait for its sums otherwise)
        if (m->host_comm) (void)lom_host_comm_abort((lom_host_comm *)m->host_comm);
        return rc == LOM_ERR_HOOK ? LOM_ERR_HIP : rc;
    }
    if (m->profiling && c.prof_used) {
        LOM_HIP(m, hipStreamSynchronize(m->stream));
        read_events(m, c.prof_used, 0, st);
    }
    st.host_launch_ms = c.launch_s * 1e3;
    st.host_wait_ms = c.wait_s * 1e3;
    st.host_fallback = fell_back ? 1 : 0;
    if (stats) *stats = st;
    return LOM_OK;
}

static int align_device(lom_map *m, const char *d_src, size_t n, size_t stride, const float guess_t[3],
                        const float guess_q[4], float out_t[3], float out_q[4], lom_align_stats *stats)
{
    const int rc = align_device_paths(m, d_src, n, stride, guess_t, guess_q, out_t, out_q, stats);
    // lom_map_radius_cleanup_after_align and lom_map_set_align_idle_hook arm ONE align, whichever path it took and however it ended
    m->spec_radius = 0.f;
    m->idle_hook = nullptr;
    return rc;
}

static int stage_scan(lom_map *m, const float *src, size_t n, size_t stride, const char **d_src)
{
    const size_t bytes = n ? (n - 1) * stride + 12 : 0;
    int rc = ensure(m, m->scan_src, std::max<size_t>(bytes, 16));
    if (rc != LOM_OK) return rc;
    if (bytes) LOM_HIP(m, hipMemcpyAsync(m->scan_src.p, src, bytes, hipMemcpyHostToDevice, m->stream));
    *d_src = (const char *)m->scan_src.p;
    return LOM_OK;
}

// ---------------------------------------------------------------------------
// Batched align (lom_match_align_batch / lom_match_align_multi): K (scan, guess) problems, each against a keyframe of its
// own (the batch: all against one), the K solves side by side in ONE device-resident chain on the RUNNER's stream -- per
// outer iteration one k_match launch and one k_lm launch for all problems of a round.  A problem's descriptor carries
// its keyframe's MapView; k_match reads it from there (k_lm reads records only).
//
// Grouping.  A problem runs with the k_lm variant (lm_shape) and grid (nb) the single align would give it on this handle,
//   so the workgroup -> point assignment and every reduction order are the single align's: bit-equal results.  Problems
//   are grouped by (variant, counted, temporal bound) -- the last two are template parameters of k_match and come from
//   the problem's map -- in order of first appearance; a group runs as one or more rounds.  Grids may differ within a
//   round: the launch is sized for the largest, and a problem's descriptor names its own (streams of similar clouds
//   differ by a workgroup or two; one round per grid made K streams K rounds).
// Rounds.  k_lm's workgroups wait for each other, so a round's whole grid must be resident at once: problems per round =
//   floor(CUs x blocks per CU / the group's largest nb), CUs of the context's partition where it has one.  Blocks per CU: the occupancy query
//   for the batch kernel, capped at 2 (the query over-reports only where SGPRs bind, from 7 blocks of 256 threads per CU
//   up -- MI355X "Residency and cooperative launch" -- far above the cap).  LOM_OPT_TEST_BATCH_ROUND_MAX caps it further.
// Chain.  kPairsAhead pairs go out at once, then one pair per round of reports while any problem of the round is
//   unfinished (a finished problem's later launches return at once, as the single align's do), at most 35.
// Give-up.  A problem whose k_lm gave up (its error word) is redone alone through the single align on its own map; the
//   others keep their device results.  LOM_OPT_TEST_GIVE_UP_AT_OUTER (one shot per map) goes to the map's first problem,
//   which opens a round of its group: the kernel applies the test to problem 0 of a launch.
// Isolation.  Own states, records, counters, exchange sets and reports: the single align's align_state, scan_on, xrec
//   and report, and the radius cleanup's scratch, are not touched.
// ---------------------------------------------------------------------------
struct BatchItem {
    lom_map *map;  // the keyframe it searches
    const char *src;
    size_t stride;
    uint32_t n;
    float gt[3], gq[4];
    int give_up_outer;  // LOM_OPT_TEST_GIVE_UP_AT_OUTER taken from its map (-1: none)
};

constexpr uint32_t kBatchBlocksPerCuCap = 2;

static int lm_batch_per_cu(lom_map *m, LmShape shape, uint32_t *out)
{
    uint32_t &cached = m->lm_batch_per_cu[shape];
    if (!cached) {
        int per_cu = 0;
        const LmForm &f = lm_form(shape);
        LOM_HIP(m, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(f.batch),
                                                                (int)f.threads, 0));
        cached = (uint32_t)std::max(1, std::min(per_cu, (int)kBatchBlocksPerCuCap));
    }
    *out = cached;
    return LOM_OK;
}

static inline size_t round_up256(size_t b) { return (b + 255) & ~size_t(255); }

// all problems through the device-resident chain; gave_up[i]: problem i's solve gave up (to be redone)
static int align_batch_chained(lom_map *m, const BatchItem *it, int count, lom_align_result *out, std::vector<char> &gave_up,
                               double &launch_s, double &wait_s)
{
    static_assert(sizeof(AlignReport) <= 256, "one report slot");
    const uint32_t part = m->stream == m->own_stream ? m->partition_cus : 0u;
    std::vector<LmShape> shape(count);
    std::vector<uint32_t> nb(count), mb(count);
    for (int i = 0; i < count; i++) {
        const uint32_t n = it[i].n;
        shape[i] = lm_shape(n);
        const int rc = lm_grid(m, n, shape[i], &nb[i]);
        if (rc != LOM_OK) return rc;
        mb[i] = n ? match_grid(n, part) : 0u;
    }
    // groups by (variant, counted, temporal) in order of first appearance, cut into rounds; `order` lists the problems round
    // by round
    struct Round {
        int first, size;  // range of `order`
        LmShape shape;
        uint32_t nb;  // the largest solve grid of its problems: the launch's x dimension
        bool counted, temporal;
        int give_up_outer;  // of its problem 0
    };
    auto counted = [&](int i) { return it[i].map->opt_count; };
    auto temporal = [&](int i) { return !it[i].map->opt_no_temporal; };
    std::vector<int> order;
    std::vector<Round> rounds;
    {
        std::vector<char> taken(count, 0);
        uint32_t cus = 0;
        int rc = device_cus(m, &cus);
        if (rc != LOM_OK) return rc;
        for (int i = 0; i < count; i++) {
            if (taken[i]) continue;
            uint32_t per_cu = 0;
            if ((rc = lm_batch_per_cu(m, shape[i], &per_cu)) != LOM_OK) return rc;
            std::vector<int> members;
            uint32_t nb_max = 0;
            for (int k = i; k < count; k++)
                if (!taken[k] && shape[k] == shape[i] && counted(k) == counted(i) && temporal(k) == temporal(i)) {
                    taken[k] = 1;
                    members.push_back(k);
                    nb_max = std::max(nb_max, nb[k]);
                }
            // (a round's launch is sized for its largest grid: residency is counted with the group's largest)
            int per_round = (int)std::max(1u, cus * per_cu / nb_max);
            if (m->test_batch_round_max > 0) per_round = std::min(per_round, m->test_batch_round_max);
            // a problem that carries a give-up test opens a round (the kernel applies it to problem 0 of a launch)
            for (size_t a = 0; a < members.size();) {
                size_t size = 1;
                while (a + size < members.size() && size < (size_t)per_round && it[members[a + size]].give_up_outer < 0) size++;
                uint32_t grid = 0;
                for (size_t k = 0; k < size; k++) grid = std::max(grid, nb[members[a + k]]);
                rounds.push_back(Round{(int)order.size(), (int)size, shape[i], grid, counted(i), temporal(i),
                                       it[members[a]].give_up_outer});
                for (size_t k = 0; k < size; k++) order.push_back(members[a + k]);
                a += size;
            }
        }
    }
    int max_slots = 0;
    for (const Round &r : rounds) max_slots = std::max(max_slots, r.size);
    // buffers: records and k_match counters per problem, exchange sets per round slot, states + descriptors per problem
    std::vector<size_t> off_rec(count), off_cnt(count);
    size_t rec_bytes = 0, cnt_bytes = 0;
    for (int i = 0; i < count; i++) {
        off_rec[i] = rec_bytes;
        rec_bytes += round_up256((size_t)std::max(it[i].n, 1u) * sizeof(MatchRec));
        off_cnt[i] = cnt_bytes;
        cnt_bytes += round_up256((size_t)std::max(mb[i], 1u) * 16);
    }
    const size_t xset_bytes = (size_t)2 * kMaxLmBlocksBig * kRecWords * sizeof(XWord);
    const size_t states_bytes = round_up256((size_t)count * sizeof(AlignState));
    const size_t dev_bytes = states_bytes + (size_t)count * sizeof(BatchProblem);
    int rc;
    if ((rc = ensure(m, m->batch_rec, rec_bytes)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->batch_cnt, cnt_bytes)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->batch_dev, dev_bytes)) != LOM_OK) return rc;
    {
        void *before = m->batch_xrec.p;
        if ((rc = ensure(m, m->batch_xrec, (size_t)max_slots * xset_bytes)) != LOM_OK) return rc;
        if (m->batch_xrec.p != before)  // fresh sets: no word may carry a sequence number of this call
            LOM_HIP(m, hipMemsetAsync(m->batch_xrec.p, 0, m->batch_xrec.bytes, m->stream));
    }
    if (m->h_batch_bytes < dev_bytes) {
        LOM_HIP(m, hipStreamSynchronize(m->stream));
        if (m->h_batch) LOM_HIP(m, hipHostFree(m->h_batch));
        m->h_batch = nullptr;
        m->h_batch_bytes = 0;
        const size_t bytes = std::max(dev_bytes, (size_t)4096);
        hipError_t e = hipHostMalloc(&m->h_batch, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return set_error(m, LOM_ERR_OOM, "hipHostMalloc(batch staging)", e);
        m->h_batch_bytes = bytes;
    }
    if (m->batch_report_slots < (size_t)count) {
        LOM_HIP(m, hipStreamSynchronize(m->stream));
        if (m->h_batch_report) LOM_HIP(m, hipHostFree(m->h_batch_report));
        m->h_batch_report = m->d_batch_report = nullptr;
        m->batch_report_slots = 0;
        const size_t slots = std::max((size_t)count, (size_t)16);
        hipError_t e = hipHostMalloc(&m->h_batch_report, slots * 256, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&m->d_batch_report, m->h_batch_report, 0);
        if (e != hipSuccess) return set_error(m, LOM_ERR_OOM, "hipHostMalloc(batch reports)", e);
        std::memset(m->h_batch_report, 0, slots * 256);
        m->batch_report_slots = slots;
    }
    // states (the guess as the first search's pose) and descriptors, in `order`, one copy to the device
    AlignState *h_states = reinterpret_cast<AlignState *>(m->h_batch);
    BatchProblem *h_desc = reinterpret_cast<BatchProblem *>((char *)m->h_batch + states_bytes);
    AlignState *d_states = reinterpret_cast<AlignState *>(m->batch_dev.p);
    const BatchProblem *d_desc = reinterpret_cast<const BatchProblem *>((char *)m->batch_dev.p + states_bytes);
    for (const Round &r : rounds)
        for (int k = 0; k < r.size; k++) {
            const int j = r.first + k, i = order[j];
            AlignState &st = h_states[j];
            std::memset(&st, 0, sizeof st);
            BatchProblem &d = h_desc[j];
            std::memset(&d, 0, sizeof d);
            d.map = view_of(it[i].map);
            d.src = it[i].src;
            d.stride = it[i].stride;
            d.rec = reinterpret_cast<MatchRec *>((char *)m->batch_rec.p + off_rec[i]);
            d.block_counters = reinterpret_cast<uint32_t *>((char *)m->batch_cnt.p + off_cnt[i]);
            d.state = d_states + j;
            d.report = reinterpret_cast<AlignReport *>((char *)m->d_batch_report + (size_t)j * 256);
            d.xrec = (char *)m->batch_xrec.p + (size_t)k * xset_bytes;
            d.n = it[i].n;
            d.match_blocks = mb[i];
            d.lm_blocks = nb[i];
            set_guess(it[i].gt, it[i].gq, d, st);
            volatile AlignReport *rp = reinterpret_cast<volatile AlignReport *>((char *)m->h_batch_report + (size_t)j * 256);
            rp->error = 0;
        }
    LOM_HIP(m, hipMemcpyAsync(m->batch_dev.p, m->h_batch, dev_bytes, hipMemcpyHostToDevice, m->stream));
    P2pArgs px = p2p_args(m);
    for (size_t ri = 0; ri < rounds.size(); ri++) {
        const Round &R = rounds[ri];
        uint32_t mb_max = 0;
        for (int k = 0; k < R.size; k++) mb_max = std::max(mb_max, mb[order[R.first + k]]);
        const BatchProblem *desc = d_desc + R.first;
        const LmForm &form = lm_form(R.shape);
        const unsigned long long seq0 = m->batch_report_seq;
        auto launch_pair = [&](int i) -> int {
            const double t_l = now_s();
            if (mb_max) {
                const bool prev = i > 0 && R.temporal;  // (the first search of a scan: no previous records)
                PoseArgs P;
                std::memset(&P, 0, sizeof P);
                hipLaunchKernelGGL(match_kernel(true, prev, R.counted, true), dim3(mb_max, R.size), dim3(kMatchThreads), 0,
                                   m->stream, MapView{}, (const char *)nullptr, (size_t)0, 0u, P, (int32_t *)nullptr,
                                   (MatchRec *)nullptr, (QStat *)nullptr, (uint32_t *)nullptr, (unsigned long long *)nullptr,
                                   (const AlignState *)nullptr, desc);
                LOM_HIP(m, hipGetLastError());
            }
            m->batch_lm_seq += 8;  // a solve spends at most 5 evaluations
            LmInit init;
            std::memset(&init, 0, sizeof init);
            const int give_up = i == R.give_up_outer ? 1 : 0;
            hipLaunchKernelGGL(form.batch, dim3(R.nb, R.size), dim3(form.threads), 0, m->stream, (const MatchRec *)nullptr, 0u,
                               (AlignState *)nullptr, init, i == 0 ? 1 : 0, (const uint32_t *)nullptr, 0u, (XWord *)nullptr,
                               m->batch_lm_seq, (AlignReport *)nullptr, seq0 + (unsigned long long)i + 1, 0ull, m->patience_ticks,
                               (unsigned long long *)nullptr, px, (double *)nullptr, give_up, desc);
            LOM_HIP(m, hipGetLastError());
            launch_s += now_s() - t_l;
            return LOM_OK;
        };
        std::vector<char> done(R.size, 0);
        bool any_gave_up = false;
        auto poll = [&](int launched, int &open) -> int {
            const double t_w = now_s();
            const unsigned long long want = seq0 + (unsigned long long)launched;
            for (int k = 0; k < R.size; k++) {
                if (done[k]) continue;
                const int j = R.first + k, i = order[j];
                volatile AlignReport *rp = reinterpret_cast<volatile AlignReport *>((char *)m->h_batch_report + (size_t)j * 256);
                const int w = wait_report(m, rp, want, "batched device solve");
                if (w < 0) {
                    m->batch_report_seq = want;
                    return w;
                }
                if (w == kReportError) {  // its later launches see the flag in its AlignState and return at once
                    gave_up[i] = 1;
                    out[i].round = (int32_t)ri;
                    any_gave_up = true;
                    done[k] = 1;
                } else if (rp->finished) {
                    result_from_report(rp, R.counted, nb[i], out[i]);
                    out[i].round = (int32_t)ri;
                    done[k] = 1;
                } else {
                    open++;
                }
            }
            wait_s += now_s() - t_w;
            return LOM_OK;
        };
        int launched = 0;
        if ((rc = chain_start(launched, launch_pair)) != LOM_OK) return rc;
        if ((rc = chain_continue(launched, launch_pair, poll)) != LOM_OK) return rc;
        m->batch_report_seq = seq0 + (unsigned long long)launched;
        if (any_gave_up) LOM_HIP(m, hipStreamSynchronize(m->stream));
    }
    return LOM_OK;
}

// The problems of one call, whichever entry point: `runner` carries the chain (stream, batch buffers), it[i].map is the
// keyframe problem i searches.  Arguments are checked by the caller.
static int align_multi(lom_map *m, BatchItem *it, int count, lom_align_result *out, int *best, bool device_input)
{
    if (count == 0) {
        if (best) *best = -1;
        return LOM_OK;
    }
    for (int i = 0; i < count; i++)
        if ((it[i].n && !it[i].src) || !scan_args_ok(it[i].n, it[i].stride)) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    m->last_error.clear();
    double launch_s = 0.0, wait_s = 0.0;
    // the handles involved, runner first, each once
    std::vector<lom_map *> maps{m};
    for (int i = 0; i < count; i++)
        if (std::find(maps.begin(), maps.end(), it[i].map) == maps.end()) maps.push_back(it[i].map);
    auto problem_error = [&](int i, int rc) {
        lom_map *pm = it[i].map;
        if (pm == m) return rc;
        const std::string why = "problem " + std::to_string(i) + ": " + pm->last_error;
        return set_error(m, rc, why.c_str());
    };
    // every map settled before anything is launched (an insert nobody has looked at yet: the search must see its points)
    for (size_t k = 0; k < maps.size(); k++) {
        lom_map *pm = maps[k];
        const bool searched = k > 0 || std::any_of(it, it + count, [&](const BatchItem &b) { return b.map == m; });
        if (!searched) continue;
        const int rcp = resolve_pending(pm);
        if (rcp != LOM_OK) {
            for (int i = 0; i < count; i++)
                if (it[i].map == pm) return problem_error(i, rcp);
        }
    }
    // stream order in: what is enqueued on a problem map's stream (a _nowait insert, a cleanup) comes first
    for (size_t k = 1; k < maps.size(); k++) {
        lom_map *pm = maps[k];
        if (pm->stream == m->stream) continue;
        if (!pm->multi_ev) LOM_HIP(m, hipEventCreateWithFlags(&pm->multi_ev, hipEventDisableTiming));
        LOM_HIP(m, hipEventRecord(pm->multi_ev, pm->stream));
        LOM_HIP(m, hipStreamWaitEvent(m->stream, pm->multi_ev, 0));
    }
    int rc;
    if (!device_input) {
        // host scans staged into one device buffer up front (a cloud shared by several problems once)
        std::vector<size_t> off((size_t)count, 0);
        std::vector<char> first((size_t)count, 1);
        size_t total = 0;
        for (int i = 0; i < count; i++) {
            int same = -1;
            for (int k = 0; k < i && same < 0; k++)
                if (it[k].src == it[i].src && it[k].n == it[i].n && it[k].stride == it[i].stride) same = k;
            if (same >= 0) {
                off[i] = off[same];
                first[i] = 0;
                continue;
            }
            off[i] = total;
            if (it[i].n) total += round_up256((it[i].n - 1) * it[i].stride + 12);
        }
        if ((rc = ensure(m, m->batch_src, std::max<size_t>(total, 256))) != LOM_OK) return rc;
        const double t_l = now_s();
        for (int i = 0; i < count; i++) {
            const char *host = it[i].src;
            it[i].src = (const char *)m->batch_src.p + off[i];
            if (first[i] && it[i].n)
                LOM_HIP(m, hipMemcpyAsync((char *)m->batch_src.p + off[i], host, (it[i].n - 1) * it[i].stride + 12,
                                          hipMemcpyHostToDevice, m->stream));
        }
        launch_s += now_s() - t_l;
    }
    // the single align's one-shot arms (a radius cleanup behind the next align, an idle hook) are the NEXT single align's,
    // on every handle involved: nothing below takes or runs them
    struct Arms {
        float spec;
        void (*hook)(void *);
        void *user;
    };
    std::vector<Arms> arms(maps.size());
    for (size_t k = 0; k < maps.size(); k++) {
        arms[k] = Arms{maps[k]->spec_radius, maps[k]->idle_hook, maps[k]->idle_user};
        maps[k]->spec_radius = 0.f;
        maps[k]->idle_hook = nullptr;
    }
    // device-resident chain: problems whose map is a plain single-GPU one (no LOM_OPT_HOST_LM, no exchange), on a runner
    // without an exchange; the others go through their map's own single align, one after another
    const bool runner_plain = !m->comm && !m->host_comm;
    std::vector<char> redo((size_t)count, 0), chained((size_t)count, 0);
    std::vector<int> idx;
    for (int i = 0; i < count; i++) {
        lom_map *pm = it[i].map;
        chained[i] = runner_plain && !pm->comm && !pm->host_comm && !pm->opt_host_lm;
        it[i].give_up_outer = -1;
        if (!chained[i]) {
            redo[i] = 1;
            continue;
        }
        if (pm->test_give_up_outer >= 0) {  // one shot: this map's first problem
            it[i].give_up_outer = pm->test_give_up_outer;
            pm->test_give_up_outer = -1;
        }
        idx.push_back(i);
    }
    rc = LOM_OK;
    if (!idx.empty()) {
        for (lom_map *pm : maps) server_stop(pm);
        std::vector<BatchItem> sub(idx.size());
        std::vector<lom_align_result> res(idx.size());
        std::vector<char> gave(idx.size(), 0);
        for (size_t k = 0; k < idx.size(); k++) sub[k] = it[idx[k]];
        rc = align_batch_chained(m, sub.data(), (int)sub.size(), res.data(), gave, launch_s, wait_s);
        for (size_t k = 0; rc == LOM_OK && k < idx.size(); k++) {
            out[idx[k]] = res[k];
            redo[idx[k]] = gave[k];
        }
    }
    // the redos and host-driven problems run on their maps' streams: the staged scans and the chain come first
    bool ordered = false;
    for (int i = 0; rc == LOM_OK && i < count; i++) {
        if (!redo[i]) continue;
        lom_map *pm = it[i].map;
        if (pm->stream != m->stream && !ordered) {
            LOM_HIP(m, hipStreamSynchronize(m->stream));
            ordered = true;
        }
        pm->last_error.clear();
        if (!chained[i]) out[i].round = -1;
        rc = align_device_paths(pm, it[i].src, it[i].n, it[i].stride, it[i].gt, it[i].gq, out[i].t, out[i].q_wxyz,
                                &out[i].stats);
        pm->spec_radius = 0.f;
        pm->idle_hook = nullptr;
        if (rc != LOM_OK) {
            rc = problem_error(i, rc);
            break;
        }
        if (chained[i]) out[i].stats.host_fallback = 1;
        launch_s += out[i].stats.host_launch_ms * 1e-3;
        wait_s += out[i].stats.host_wait_ms * 1e-3;
    }
    for (size_t k = 0; k < maps.size(); k++) {
        maps[k]->spec_radius = arms[k].spec;
        maps[k]->idle_hook = arms[k].hook;
        maps[k]->idle_user = arms[k].user;
    }
    // stream order out: the chain's trailing launches (finished problems' launches may still be queued) come before
    // whatever is enqueued next on a problem map -- an insert, a cleanup
    if (maps.size() > 1) {
        if (!m->multi_ev) LOM_HIP(m, hipEventCreateWithFlags(&m->multi_ev, hipEventDisableTiming));
        LOM_HIP(m, hipEventRecord(m->multi_ev, m->stream));
        for (size_t k = 1; k < maps.size(); k++)
            if (maps[k]->stream != m->stream) LOM_HIP(m, hipStreamWaitEvent(maps[k]->stream, m->multi_ev, 0));
    }
    if (rc != LOM_OK) return rc;
    for (int i = 0; i < count; i++) {
        lom_align_stats &st = out[i].stats;
        st.match_kernel_ms = 0.0;
        st.profiled_launches = 0;
        st.lm_kernel_ms = 0.0;
        st.lm_profiled_launches = 0;
        st.host_launch_ms = launch_s * 1e3;
        st.host_wait_ms = wait_s * 1e3;
    }
    if (best) *best = lom_align_batch_best(out, count);
    return LOM_OK;
}

// P: lom_align_problem or lom_align_multi_problem (a count beyond kMaxScanPoints is kept as that: align_multi refuses it)
template <class P>
static BatchItem batch_item(lom_map *map, const P &p)
{
    BatchItem b;
    b.map = map;
    b.src = (const char *)p.xyz;
    b.stride = p.stride_bytes;
    b.n = (uint32_t)std::min<size_t>(p.n, kMaxScanPoints);
    for (int a = 0; a < 3; a++) b.gt[a] = p.guess_t[a];
    for (int a = 0; a < 4; a++) b.gq[a] = p.guess_q_wxyz[a];
    b.give_up_outer = -1;
    return b;
}

static int align_batch(lom_map *m, const lom_align_problem *p, int count, lom_align_result *out, int *best, bool device_input)
{
    std::vector<BatchItem> it((size_t)std::max(count, 0));
    for (int i = 0; i < count; i++) it[i] = batch_item(m, p[i]);
    return align_multi(m, it.data(), count, out, best, device_input);
}

static int align_multi_entry(lom_map *m, const lom_align_multi_problem *p, int count, lom_align_result *out, int *best,
                             bool device_input)
{
    if (!m || count < 0 || (count > 0 && (!p || !out))) return LOM_ERR_ARG;
    for (int i = 0; i < count; i++)
        if (!p[i].map || p[i].map->device != m->device) return LOM_ERR_ARG;  // (handle fields only: no device call)
    std::vector<BatchItem> it((size_t)count);
    for (int i = 0; i < count; i++) it[i] = batch_item(p[i].map, p[i]);
    return align_multi(m, it.data(), count, out, best, device_input);
}

}  // namespace lom

using namespace lom;

extern "C" {

// one search (or two: first at the pose (t0, q0), then at (t, q) with the first one's records as the temporal bound)
static int64_t find_pairs_core(lom_map *m, const float *src, size_t n, size_t stride, const float *t0, const float *q0,
                               const float t[3], const float q[4], float max_sq, lom_correspondence *out)
{
    if (!m || (n && (!src || !out)) || !t || !q || !scan_args_ok(n, stride)) return LOM_ERR_ARG;
    if (n == 0) return 0;
    LOM_HIP(m, hipSetDevice(m->device));
    const char *d_src = nullptr;
    int rc = resolve_pending(m);
    if (rc != LOM_OK) return rc;
    if ((rc = stage_scan(m, src, n, stride, &d_src)) != LOM_OK) return rc;
    if ((rc = scan_buffers(m, (uint32_t)n, true)) != LOM_OK) return rc;
    ScanCtx c{m, d_src, stride, (uint32_t)n, 0};
    if (t0 && q0 && (rc = launch_match(c, t0, q0, max_sq, true)) != LOM_OK) return rc;
    if ((rc = launch_match(c, t, q, max_sq, true)) != LOM_OK) return rc;
    std::vector<int32_t> idx(n);
    std::vector<MatchRec> on(n);
    std::vector<QStat> st(n);
    LOM_HIP(m, hipMemcpyAsync(idx.data(), m->scan_idx.p, n * 4, hipMemcpyDeviceToHost, m->stream));
    LOM_HIP(m, hipMemcpyAsync(on.data(), m->scan_on.p, n * sizeof(MatchRec), hipMemcpyDeviceToHost, m->stream));
    LOM_HIP(m, hipMemcpyAsync(st.data(), m->scan_stats.p, n * sizeof(QStat), hipMemcpyDeviceToHost, m->stream));
    LOM_HIP(m, hipStreamSynchronize(m->stream));
    // index = voxel_creation_index * max_points + in_voxel_index, the creation index counting the voxels the map HOLDS: where
    // a radius cleanup has left erased voxels' slabs in place (k_cleanup_mark) the slab number runs ahead of it
    std::vector<uint32_t> dense;
    const lom_map *mp = m->parent ? m->parent : m;
    const uint32_t n_dead = mp->n_dead, dead_below = mp->dead_below;
    if (n_dead) {
        std::vector<uint32_t> cnt(dead_below);
        LOM_HIP(m, hipMemcpy(cnt.data(), mp->slabs.count, (size_t)dead_below * 4, hipMemcpyDeviceToHost));
        dense.resize(dead_below);
        uint32_t live = 0;
        for (uint32_t s = 0; s < dead_below; s++) {
            dense[s] = live;
            live += cnt[s] != 0u;
        }
    }
    const uint32_t K = mp->K;
    int64_t valid = 0;
    for (size_t i = 0; i < n; i++) {
        lom_correspondence &o = out[i];
        o.index = idx[i];
        if (n_dead && idx[i] >= 0) {
            const uint32_t slab = (uint32_t)idx[i] / K, j = (uint32_t)idx[i] % K;
            o.index = (int64_t)(slab < dead_below ? dense[slab] : slab - n_dead) * K + j;
        }
        o.origin[0] = on[i].ox;
        o.origin[1] = on[i].oy;
        o.origin[2] = on[i].oz;
        o.normal[0] = on[i].nx;
        o.normal[1] = on[i].ny;
        o.normal[2] = on[i].nz;
        o.sq_dist = st[i].sq_dist;
        o.n_cand = c.counted ? st[i].n_cand : 0u;  // the reference-algorithm counts, or nothing (LOM_OPT_COUNT_CANDIDATES)
        o.n_occ = c.counted ? st[i].n_occ : 0u;
        valid += idx[i] >= 0;
    }
    return valid;
}

int64_t lom_match_find_pairs(lom_map *m, const float *src, size_t n, size_t stride, const float t[3],
                             const float q[4], float max_dist, lom_correspondence *out)
{
    return find_pairs_core(m, src, n, stride, nullptr, nullptr, t, q, sq_f32(max_dist), out);
}

int64_t lom_match_find_pairs_sq(lom_map *m, const float *src, size_t n, size_t stride, const float t[3],
                                const float q[4], double max_dist_sq, lom_correspondence *out)
{
    return find_pairs_core(m, src, n, stride, nullptr, nullptr, t, q, threshold_f32(max_dist_sq), out);
}

int64_t lom_debug_find_pairs_after(lom_map *m, const float *src, size_t n, size_t stride, const float t_prev[3],
                                   const float q_prev[4], const float t[3], const float q[4], float max_dist,
                                   lom_correspondence *out)
{
    if (!t_prev || !q_prev) return LOM_ERR_ARG;
    return find_pairs_core(m, src, n, stride, t_prev, q_prev, t, q, sq_f32(max_dist), out);
}

int lom_comm_attach_p2p(lom_map *m, lom_host_comm *hc)
{
    if (!m || !hc) return LOM_ERR_ARG;
    if (m->comm) return set_error(m, LOM_ERR_STATE, "an RCCL communicator is already attached");
    LOM_HIP(m, hipSetDevice(m->device));
    int rank = 0, nranks = 1;
    if (host_comm_rank(hc, &rank, &nranks) != LOM_OK) return LOM_ERR_ARG;
    if (nranks > kP2pMaxRanks) return set_error(m, LOM_ERR_ARG, "device-to-device exchange: at most 8 ranks");
    p2p_detach(m);
    server_stop(m);
    // From here on every step is collective: a rank that fails locally still takes part in the
    // exchanges below, so that all ranks reach the same verdict.
    const size_t bytes = kP2pBufferBytes;  // four exchange sets + one abort word per rank
    m->p2p_epoch = 0;
    m->lm_launches = 0;  // the set pairs alternate with this count: the same on every rank from here on
    int ok = 1;
    struct Blob {
        hipIpcMemHandle_t handle;
        int ok;
    } mine, all[kP2pMaxRanks];
    std::memset(&mine, 0, sizeof mine);
    static_assert(sizeof(Blob) <= 256, "fits one host-exchange slot");
    // fine-grained (coherent across agents) device memory; plain device memory if that is refused --
    // the self-test below decides whether the exchange works on this machine
    if (hipExtMallocWithFlags(&m->p2p_local, bytes, hipDeviceMallocFinegrained) != hipSuccess) {
        (void)hipGetLastError();
        if (hipMalloc(&m->p2p_local, bytes) != hipSuccess) {
            m->p2p_local = nullptr;
            ok = 0;
        }
    }
    if (ok && (hipMemsetAsync(m->p2p_local, 0, bytes, m->stream) != hipSuccess ||
               hipStreamSynchronize(m->stream) != hipSuccess))
        ok = 0;
    if (ok && nranks > 1 && hipIpcGetMemHandle(&mine.handle, m->p2p_local) != hipSuccess) ok = 0;
    mine.ok = ok;
    if (lom_host_comm_allgather(hc, &mine, sizeof mine, all) != LOM_OK) {
        p2p_detach(m);
        return set_error(m, LOM_ERR_COMM, "device-to-device exchange: handle exchange failed");
    }
    for (int r = 0; r < nranks; r++) ok = ok && all[r].ok;
    if (ok) {
        for (int r = 0; r < nranks && ok; r++) {
            if (r == rank) {
                m->p2p_peer[r] = m->p2p_local;
            } else if (hipIpcOpenMemHandle(&m->p2p_peer[r], all[r].handle, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
                m->p2p_peer[r] = nullptr;
                ok = 0;
            }
        }
    }
    // barrier: every rank has its mappings before anybody stores through them
    double sync[1] = {0.0};
    if (lom_host_comm_allreduce(hc, sync, 1) != LOM_OK) ok = 0;
    // sequence numbers: one epoch per attach, identical on all ranks (the host exchange has done the
    // same number of operations on every rank) and above every number this handle has used
    unsigned long long hseq = 0;
    (void)host_comm_rank(hc, &rank, &nranks, &hseq);
    m->lm_seq = std::max(m->lm_seq, hseq << 32);
    m->rank = rank;
    m->nranks = nranks;
    // self-test: 200 exchanges of known values through the mappings
    uint32_t res[2] = {1u, 1u};
    if (ok && scan_buffers(m, 1, false) != LOM_OK) ok = 0;
    if (ok) {
        m->p2p = true;
        const P2pArgs A = p2p_args(m);
        m->p2p = false;
        hipLaunchKernelGGL(k_p2p_selftest, dim3(1), dim3(64), 0, m->stream, A, m->lm_seq, 200,
                           m->patience_ticks, (uint32_t *)m->results.p);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(res, (uint32_t *)m->results.p, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
            hipStreamSynchronize(m->stream) != hipSuccess)
            ok = 0;
        else if (res[0] != 0 || res[1] != 0)
            ok = 0;
    }
    m->lm_seq += 256;
    double verdict[1] = {ok ? 0.0 : 1.0};
    if (lom_host_comm_allreduce(hc, verdict, 1) != LOM_OK) verdict[0] = 1.0;
    if (verdict[0] != 0.0) {
        p2p_detach(m);
        m->rank = 0;
        m->nranks = 1;
        return set_error(m, LOM_ERR_COMM, "device-to-device exchange failed its self-test on some rank");
    }
    m->host_comm = hc;  // rank / nranks bookkeeping as with the host exchange; the caller keeps ownership
    m->p2p = true;
    return LOM_OK;
}

int lom_profile_match(lom_map *m, const float *d_src, size_t n, size_t stride, const float t[3], const float q[4],
                      float max_dist, int reps, double *avg_us_out, double *bytes_out, double *requested_bytes_out,
                      double *pair_avg_us_out)
{
    if (!m || !d_src || !n || !t || !q || reps < 1 || !avg_us_out || !scan_args_ok(n, stride)) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    int rc = scan_buffers(m, (uint32_t)n, false);
    if (rc != LOM_OK) return rc;
    ScanCtx c{m, (const char *)d_src, stride, (uint32_t)n, 0};
    const bool was = m->profiling;
    m->profiling = false;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    LOM_HIP(m, hipEventCreate(&e0));
    LOM_HIP(m, hipEventCreate(&e1));
    // warm-up; it also leaves the records the launches behind it take their temporal bound from: the train is what the
    // searches of outer iterations >= 2 of an align run (LOM_OPT_NO_TEMPORAL_BOUND: what the first one runs)
    rc = launch_match(c, t, q, sq_f32(max_dist), false);
    if (rc == LOM_OK) rc = hipEventRecord(e0, m->stream) == hipSuccess ? LOM_OK : LOM_ERR_HIP;
    for (int i = 0; rc == LOM_OK && i < reps; i++) rc = launch_match(c, t, q, sq_f32(max_dist), false);
    if (rc == LOM_OK) rc = hipEventRecord(e1, m->stream) == hipSuccess ? LOM_OK : LOM_ERR_HIP;
    // the same launches with one event pair EACH (what the sampled in-loop measurement of lom_match_align* does):
    // the difference to the train above is what an event pair adds to a single short kernel
    double pair_ms = 0.0;
    if (rc == LOM_OK && pair_avg_us_out) {
        m->profiling = true;
        c.prof_used = 0;
        const int pr = std::min(reps, 128);
        for (int i = 0; rc == LOM_OK && i < pr; i++) rc = launch_match(c, t, q, sq_f32(max_dist), false);
        m->profiling = false;
        if (rc == LOM_OK && hipStreamSynchronize(m->stream) != hipSuccess) rc = LOM_ERR_HIP;
        for (int i = 0; rc == LOM_OK && i < c.prof_used; i++) {
            float ms1 = 0.f;
            if (hipEventElapsedTime(&ms1, m->prof_events[(size_t)i * 3], m->prof_events[(size_t)i * 3 + 1]) == hipSuccess)
                pair_ms += ms1;
        }
        *pair_avg_us_out = c.prof_used ? pair_ms * 1e3 / c.prof_used : 0.0;
        c.prof_used = 0;
    }
    // what the timed launches asked the memory system for: one more launch of the same form that tallies, per query, the
    // rows it read and the slots it looked up (with the counts every query looks up 27 and the rows are the per-workgroup
    // tally of the launch)
    double scanned = 0.0, probed = 0.0;
    const bool train_counted = c.counted;
    if (rc == LOM_OK && requested_bytes_out) {
        if (train_counted) {
            std::vector<uint32_t> bc((size_t)c.match_blocks * 4);
            if (hipMemcpyAsync(bc.data(), d_block_counters(m), bc.size() * 4, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
                hipStreamSynchronize(m->stream) != hipSuccess)
                rc = LOM_ERR_HIP;
            for (uint32_t b = 0; rc == LOM_OK && b < c.match_blocks; b++) scanned += bc[(size_t)b * 4 + 3];
        } else {
            std::vector<QStat> qs(n);
            if ((rc = scan_buffers(m, (uint32_t)n, true)) == LOM_OK) rc = launch_match(c, t, q, sq_f32(max_dist), true);
            if (rc == LOM_OK && (hipMemcpyAsync(qs.data(), m->scan_stats.p, n * sizeof(QStat), hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
                                 hipStreamSynchronize(m->stream) != hipSuccess))
                rc = LOM_ERR_HIP;
            for (size_t i = 0; rc == LOM_OK && i < n; i++) {
                scanned += qs[i].n_cand;
                probed += qs[i].n_occ;
            }
        }
    }
    // the algorithmic bytes need the reference-algorithm counts: one more launch that produces them
    double sums[LOM_NSUMS];
    const double qd[4] = {q[0], q[1], q[2], q[3]}, td[3] = {t[0], t[1], t[2]};
    if (rc == LOM_OK) rc = launch_match(c, t, q, sq_f32(max_dist), false, false, 1);
    if (rc == LOM_OK) rc = launch_eval(c, qd, td, true, sums);  // folds the counters of that launch
    server_stop(m);
    if (rc == LOM_OK && hipStreamSynchronize(m->stream) != hipSuccess) rc = LOM_ERR_HIP;
    float ms = 0.f;
    if (rc == LOM_OK && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = LOM_ERR_HIP;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    m->profiling = was;
    if (rc != LOM_OK) return set_error(m, rc, "lom_profile_match failed");
    *avg_us_out = (double)ms * 1e3 / reps;
    if (bytes_out) *bytes_out = 444.0 * sums[31] + 12.0 * sums[29] + 12.0 * sums[28];
    if (requested_bytes_out) {
        // source point + slots looked up + rows of the scanned voxels + winner's normal + 52 B of output per query (+ 16 B
        // of the previous record where the temporal bound is in use)
        const double nq = sums[31];
        const double slots = train_counted ? 27.0 * nq : probed;
        const double prev_b = (c.have_prev && !m->opt_no_temporal) ? 16.0 * nq : 0.0;
        *requested_bytes_out = 12.0 * nq + 16.0 * slots + 12.0 * scanned + 12.0 * sums[28] + 52.0 * nq + prev_b;
    }
    return LOM_OK;
}

int lom_map_set_align_idle_hook(lom_map *m, void (*fn)(void *user), void *user)
{
    if (!m) return LOM_ERR_ARG;
    m->idle_hook = fn;
    m->idle_user = user;
    return LOM_OK;
}

int lom_match_align_device(lom_map *m, const float *d_src, size_t n, size_t stride, const float guess_t[3],
                           const float guess_q[4], float out_t[3], float out_q[4], lom_align_stats *stats)
{
    if (!m || (n && !d_src) || !guess_t || !guess_q || !out_t || !out_q || !stride_ok(stride)) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    m->last_error.clear();
    return align_device(m, (const char *)d_src, n, stride, guess_t, guess_q, out_t, out_q, stats);
}

// parity entry: one search at the f32 pose, then ONE evaluation of the reduced normal equations at (q, t)
// through the host-driven path's kernels (k_match + k_eval_server: accumulate_point, LDS reduction,
// record per workgroup, workgroup-ordered host sum)
int lom_debug_eval_sums(lom_map *m, const float *src, size_t n, size_t stride, const float pose_t[3],
                        const float pose_q[4], const double q[4], const double t[3], double out[LOM_NSUMS])
{
    if (!m || (n && !src) || !pose_t || !pose_q || !q || !t || !out || !scan_args_ok(n, stride)) return LOM_ERR_ARG;
    if (m->comm || m->host_comm) return set_error(m, LOM_ERR_STATE, "not with an attached exchange");
    LOM_HIP(m, hipSetDevice(m->device));
    m->last_error.clear();
    const char *d_src = nullptr;
    int rc = stage_scan(m, src, n, stride, &d_src);
    if (rc != LOM_OK) return rc;
    if ((rc = scan_buffers(m, (uint32_t)n, false)) != LOM_OK) return rc;
    ScanCtx c{m, d_src, stride, (uint32_t)n, 0};
    const bool was = m->profiling;
    m->profiling = false;
    rc = launch_match(c, pose_t, pose_q, sq_f32(0.3f), false);  // cloud_matcher.cpp:139
    if (rc == LOM_OK) rc = launch_eval(c, q, t, true, out);
    server_stop(m);
    m->profiling = was;
    if (rc == LOM_OK && hipStreamSynchronize(m->stream) != hipSuccess) rc = LOM_ERR_HIP;
    return rc;
}

// ---------------------------------------------------------------------------
// Quality report (lom_match_quality* / lom_scan_quality*): one search at the f32 pose as given, k_quality at that pose
// widened to f64, k_quality_sum into pinned host memory, ONE wait; the host math is lom_quality_from_sums (quality.cpp).
// Isolation as the batched align: buffers of its own (lom_map::qual_*), nothing of the single align's state, of an armed
// cleanup scan or idle hook, or of the map-maintenance scratch is read or written; neither call_seq nor mutations move.
// The grid is k_eval's (eval_grid): a short, latency-bound kernel behind a k_match of a few microseconds.
// ---------------------------------------------------------------------------
static int quality_core(lom_map *m, const float *src, bool device_input, size_t n, size_t stride, const float t[3],
                        const float q[4], float max_dist, float min_eig_t, float min_eig_r, lom_quality_report *out,
                        float *residual_out)
{
    if (!m || (n && !src) || !t || !q || !out || !scan_args_ok(n, stride)) return LOM_ERR_ARG;
    if (n == 0) {
        const double zero[LOM_NQSUMS] = {};
        return lom_quality_from_sums(zero, 0, min_eig_t, min_eig_r, out);
    }
    LOM_HIP(m, hipSetDevice(m->device));
    m->last_error.clear();
    int rc = resolve_pending(m);  // an insert nobody has looked at since: the search must see its points
    if (rc != LOM_OK) return rc;
    const uint32_t nn = (uint32_t)n;
    const uint32_t mb = match_grid(nn, m->stream == m->own_stream ? m->partition_cus : 0u), nb = eval_grid(nn);
    if ((rc = ensure(m, m->qual_idx, n * 4)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qual_rec, n * sizeof(MatchRec))) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qual_cnt, (size_t)kMaxMatchBlocks * 16)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qual_part, (size_t)kMaxEvalBlocks * kQualSums * 8)) != LOM_OK) return rc;
    if (!m->h_qual) {
        hipError_t e = hipHostMalloc((void **)&m->h_qual, LOM_NQSUMS * 8, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&m->d_qual, m->h_qual, 0);
        if (e != hipSuccess) return set_error(m, LOM_ERR_OOM, "hipHostMalloc(quality sums)", e);
    }
    const char *d_src = (const char *)src;
    float *d_res = residual_out;
    if (!device_input) {
        const size_t bytes = (n - 1) * stride + 12;
        if ((rc = ensure(m, m->qual_src, bytes)) != LOM_OK) return rc;
        LOM_HIP(m, hipMemcpyAsync(m->qual_src.p, src, bytes, hipMemcpyHostToDevice, m->stream));
        d_src = (const char *)m->qual_src.p;
        if (residual_out) {
            if ((rc = ensure(m, m->qual_res, n * 4)) != LOM_OK) return rc;
            d_res = (float *)m->qual_res.p;
        }
    }
    PoseArgs P;
    pose_args(t, q, sq_f32(max_dist), P);
    EvalArgs E;
    for (int a = 0; a < 4; a++) E.q[a] = (double)q[a];
    for (int a = 0; a < 3; a++) E.t[a] = (double)t[a];
    hipLaunchKernelGGL(match_kernel(false, false, m->opt_count, false), dim3(mb), dim3(kMatchThreads), 0, m->stream,
                       view_of(m), d_src, stride, nn, P, (int32_t *)m->qual_idx.p, (MatchRec *)m->qual_rec.p,
                       (QStat *)nullptr, (uint32_t *)m->qual_cnt.p, (unsigned long long *)nullptr,
                       (const AlignState *)nullptr, (const BatchProblem *)nullptr);
    hipLaunchKernelGGL(k_quality, dim3(nb), dim3(kEvalThreads), 0, m->stream, (const MatchRec *)m->qual_rec.p, nn, E,
                       (double *)m->qual_part.p, d_res);
    hipLaunchKernelGGL(k_quality_sum, dim3(1), dim3(64), 0, m->stream, (const double *)m->qual_part.p, nb, m->d_qual);
    LOM_HIP(m, hipGetLastError());
    if (!device_input && residual_out)
        LOM_HIP(m, hipMemcpyAsync(residual_out, d_res, n * 4, hipMemcpyDeviceToHost, m->stream));
    LOM_HIP(m, hipStreamSynchronize(m->stream));
    double sums[LOM_NQSUMS];
    std::memcpy(sums, m->h_qual, sizeof sums);
    return lom_quality_from_sums(sums, (int64_t)n, min_eig_t, min_eig_r, out);
}

int lom_match_quality(lom_map *m, const float *src, size_t n, size_t stride, const float t[3], const float q[4],
                      float max_dist, float min_eig_t, float min_eig_r, lom_quality_report *out, float *residual_out)
{
    return quality_core(m, src, false, n, stride, t, q, max_dist, min_eig_t, min_eig_r, out, residual_out);
}

int lom_match_quality_device(lom_map *m, const float *d_src, size_t n, size_t stride, const float t[3],
                             const float q[4], float max_dist, float min_eig_t, float min_eig_r,
                             lom_quality_report *out, float *d_residual_out)
{
    return quality_core(m, d_src, true, n, stride, t, q, max_dist, min_eig_t, min_eig_r, out, d_residual_out);
}

// ---------------------------------------------------------------------------
// Batched quality report (lom_match_quality_batch* / lom_scan_quality_batch*): K (scan, pose) problems against this
// keyframe, three launches per ROUND -- the batch form of k_match (blockIdx.y = the problem; its pose comes from a
// per-problem AlignState block the host fills: the chained batch instantiation the batched align's first search uses, as
// it is), k_quality_batch, k_quality_batch_sum -- every round enqueued before the host waits, once.
// Same answers whatever the batch: a problem searches and evaluates with the grids the single report gives it
//   (match_grid / eval_grid of its n), so its totals depend on the problem alone -- see k_quality.hpp.
// Rounds.  A round's records (48 B per point), workgroup records and k_match counters fit kQualBatchBudgetBytes (a
//   problem larger than that runs alone); problems go to rounds in the caller's order; the round buffers are reused by
//   the next round, which the stream orders behind this one.  What grows with K is small: a pose block and two
//   descriptors (about 0.6 KB) and LOM_NQSUMS totals per problem.  LOM_OPT_TEST_QUALITY_ROUND_MAX caps a round's problems too.
//   64 MiB: a quarter of the 256 MiB last-level cache, so what a round's search writes is still on the chip when its
//   evaluation reads it; 46 problems of a 28,800-point scan or 700 of a 1,900-point one -- several times the
//   workgroups the device has compute units for -- so that more per round would buy nothing.
// Clouds.  The host entries upload every distinct (pointer, n, stride) once, before the first round.
// Isolation.  lom_map::qualb_*: nothing of the single align, the single report, an armed cleanup scan or idle hook, or the
//   map-maintenance scratch is read or written; neither call_seq nor mutations move.
// ---------------------------------------------------------------------------
constexpr size_t kQualBatchBudgetBytes = (size_t)64 << 20;
constexpr int kQualBatchRoundCap = 32768;  // problems per round at most (blockIdx.y)

static int quality_batch_args_ok(const lom_map *m, const lom_quality_problem *p, int count, const void *out)
{
    if (!m || count < 0) return 0;
    if (count > 0 && (!p || !out)) return 0;
    for (int i = 0; i < count; i++)
        if ((p[i].n && !p[i].xyz) || !scan_args_ok(p[i].n, p[i].stride_bytes)) return 0;
    return 1;
}

// sums_out: count * LOM_NQSUMS doubles.  Arguments are checked by the caller.
static int quality_batch_core(lom_map *m, const lom_quality_problem *p, int count, bool device_input, float max_dist,
                              double *sums_out)
{
    std::vector<int> live;  // the problems with points, in the caller's order
    for (int i = 0; i < count; i++)
        if (p[i].n) live.push_back(i);
    if (live.empty()) {
        if (count) std::memset(sums_out, 0, (size_t)count * LOM_NQSUMS * 8);
        return LOM_OK;
    }
    LOM_HIP(m, hipSetDevice(m->device));
    m->last_error.clear();
    int rc = resolve_pending(m);  // an insert nobody has looked at since: the search must see its points
    if (rc != LOM_OK) return rc;
    const int L = (int)live.size();
    const uint32_t part_cus = m->stream == m->own_stream ? m->partition_cus : 0u;
    // host clouds: every distinct (pointer, n, stride) once
    std::vector<const char *> d_src(L);
    if (device_input) {
        for (int j = 0; j < L; j++) d_src[j] = (const char *)p[live[j]].xyz;
    } else {
        struct Cloud {
            const float *xyz;
            size_t n, stride, off;
        };
        std::vector<Cloud> clouds;
        std::vector<int> cloud_of(L);
        size_t src_bytes = 0;
        for (int j = 0; j < L; j++) {
            const lom_quality_problem &q = p[live[j]];
            size_t c = 0;
            // (the pose-lattice case hits its cloud at once: the newest is looked at first)
            for (c = clouds.size(); c-- > 0;)
                if (clouds[c].xyz == q.xyz && clouds[c].n == q.n && clouds[c].stride == q.stride_bytes) break;
            if (c == (size_t)-1) {
                c = clouds.size();
                clouds.push_back(Cloud{q.xyz, q.n, q.stride_bytes, src_bytes});
                src_bytes += round_up256((q.n - 1) * q.stride_bytes + 12);
            }
            cloud_of[j] = (int)c;
        }
        if ((rc = ensure(m, m->qualb_src, src_bytes)) != LOM_OK) return rc;
        for (const Cloud &c : clouds)
            LOM_HIP(m, hipMemcpyAsync((char *)m->qualb_src.p + c.off, c.xyz, (c.n - 1) * c.stride + 12,
                                      hipMemcpyHostToDevice, m->stream));
        for (int j = 0; j < L; j++) d_src[j] = (const char *)m->qualb_src.p + clouds[cloud_of[j]].off;
    }
    // rounds, and where a problem's records, counters and workgroup records lie in its round's buffers
    struct Round {
        int first, size;
        uint32_t mb, nb;  // the launches' x extent: the largest search / evaluation grid of its problems
    };
    std::vector<Round> rounds;
    std::vector<uint32_t> mb(L), nb(L);
    std::vector<size_t> off_rec(L), off_cnt(L), off_part(L);
    size_t rec_bytes = 0, cnt_bytes = 0, part_bytes = 0;
    {
        const int cap = m->test_quality_round_max > 0 ? std::min(m->test_quality_round_max, kQualBatchRoundCap) : kQualBatchRoundCap;
        size_t r_rec = 0, r_cnt = 0, r_part = 0;
        for (int j = 0; j < L; j++) {
            const uint32_t n = (uint32_t)p[live[j]].n;
            mb[j] = match_grid(n, part_cus);
            nb[j] = eval_grid(n);
            const size_t b_rec = round_up256((size_t)n * sizeof(MatchRec)), b_cnt = round_up256((size_t)mb[j] * 16),
                         b_part = round_up256((size_t)nb[j] * kQualSums * 8);
            const bool open = !rounds.empty() && rounds.back().size < cap &&
                              r_rec + r_cnt + r_part + b_rec + b_cnt + b_part <= kQualBatchBudgetBytes;
            if (!open) {
                rounds.push_back(Round{j, 0, 0u, 0u});
                r_rec = r_cnt = r_part = 0;
            }
            Round &R = rounds.back();
            R.size++;
            R.mb = std::max(R.mb, mb[j]);
            R.nb = std::max(R.nb, nb[j]);
            off_rec[j] = r_rec;
            off_cnt[j] = r_cnt;
            off_part[j] = r_part;
            r_rec += b_rec;
            r_cnt += b_cnt;
            r_part += b_part;
            rec_bytes = std::max(rec_bytes, r_rec);
            cnt_bytes = std::max(cnt_bytes, r_cnt);
            part_bytes = std::max(part_bytes, r_part);
        }
    }
    const size_t states_bytes = round_up256((size_t)L * sizeof(AlignState));
    const size_t match_desc_bytes = round_up256((size_t)L * sizeof(BatchProblem));
    const size_t dev_bytes = states_bytes + match_desc_bytes + round_up256((size_t)L * sizeof(QualBatchProblem));
    const size_t sums_bytes = (size_t)L * LOM_NQSUMS * 8;
    if ((rc = ensure(m, m->qualb_rec, rec_bytes)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qualb_cnt, cnt_bytes)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qualb_part, part_bytes)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qualb_dev, dev_bytes)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qualb_sums, sums_bytes)) != LOM_OK) return rc;
    if (m->h_qualb_bytes < dev_bytes + sums_bytes) {
        LOM_HIP(m, hipStreamSynchronize(m->stream));  // (the uploads above do not read it)
        if (m->h_qualb) LOM_HIP(m, hipHostFree(m->h_qualb));
        m->h_qualb = nullptr;
        m->h_qualb_bytes = 0;
        const size_t bytes = std::max(dev_bytes + sums_bytes, (size_t)65536);
        hipError_t e = hipHostMalloc(&m->h_qualb, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return set_error(m, LOM_ERR_OOM, "hipHostMalloc(quality batch staging)", e);
        m->h_qualb_bytes = bytes;
    }
    // per problem: the pose block the search reads, the search's descriptor, the evaluation's descriptor
    AlignState *h_states = reinterpret_cast<AlignState *>(m->h_qualb);
    BatchProblem *h_match = reinterpret_cast<BatchProblem *>((char *)m->h_qualb + states_bytes);
    QualBatchProblem *h_eval = reinterpret_cast<QualBatchProblem *>((char *)m->h_qualb + states_bytes + match_desc_bytes);
    double *h_sums = reinterpret_cast<double *>((char *)m->h_qualb + dev_bytes);
    AlignState *d_states = reinterpret_cast<AlignState *>(m->qualb_dev.p);
    const BatchProblem *d_match = reinterpret_cast<const BatchProblem *>((char *)m->qualb_dev.p + states_bytes);
    const QualBatchProblem *d_eval =
        reinterpret_cast<const QualBatchProblem *>((char *)m->qualb_dev.p + states_bytes + match_desc_bytes);
    const MapView view = view_of(m);
    const float max_sq = sq_f32(max_dist);
    for (int j = 0; j < L; j++) {
        const lom_quality_problem &q = p[live[j]];
        AlignState &st = h_states[j];
        std::memset(&st, 0, sizeof st);  // (finished = error = 0: the search runs)
        pose_args(q.t, q.q_wxyz, max_sq, st.P);
        BatchProblem &d = h_match[j];
        std::memset(&d, 0, sizeof d);
        d.map = view;
        d.src = d_src[j];
        d.stride = q.stride_bytes;
        d.rec = reinterpret_cast<MatchRec *>((char *)m->qualb_rec.p + off_rec[j]);
        d.block_counters = reinterpret_cast<uint32_t *>((char *)m->qualb_cnt.p + off_cnt[j]);
        d.state = d_states + j;
        d.n = (uint32_t)q.n;
        d.match_blocks = mb[j];
        QualBatchProblem &e = h_eval[j];
        std::memset(&e, 0, sizeof e);
        e.rec = d.rec;
        e.part = reinterpret_cast<double *>((char *)m->qualb_part.p + off_part[j]);
        e.out = (double *)m->qualb_sums.p + (size_t)j * LOM_NQSUMS;
        e.n = d.n;
        e.grid = nb[j];
        for (int a = 0; a < 4; a++) e.E.q[a] = (double)q.q_wxyz[a];
        for (int a = 0; a < 3; a++) e.E.t[a] = (double)q.t[a];
    }
    LOM_HIP(m, hipMemcpyAsync(m->qualb_dev.p, m->h_qualb, dev_bytes, hipMemcpyHostToDevice, m->stream));
    PoseArgs P0;
    std::memset(&P0, 0, sizeof P0);
    for (const Round &R : rounds) {
        hipLaunchKernelGGL(match_kernel(true, false, m->opt_count, true), dim3(R.mb, R.size), dim3(kMatchThreads), 0, m->stream,
                           MapView{}, (const char *)nullptr, (size_t)0, 0u, P0, (int32_t *)nullptr, (MatchRec *)nullptr,
                           (QStat *)nullptr, (uint32_t *)nullptr, (unsigned long long *)nullptr, (const AlignState *)nullptr,
                           d_match + R.first);
        hipLaunchKernelGGL(k_quality_batch, dim3(R.nb, R.size), dim3(kEvalThreads), 0, m->stream, d_eval + R.first);
        hipLaunchKernelGGL(k_quality_batch_sum, dim3(R.size), dim3(64), 0, m->stream, d_eval + R.first);
        LOM_HIP(m, hipGetLastError());
    }
    LOM_HIP(m, hipMemcpyAsync(h_sums, m->qualb_sums.p, sums_bytes, hipMemcpyDeviceToHost, m->stream));
    LOM_HIP(m, hipStreamSynchronize(m->stream));
    std::memset(sums_out, 0, (size_t)count * LOM_NQSUMS * 8);
    for (int j = 0; j < L; j++) std::memcpy(sums_out + (size_t)live[j] * LOM_NQSUMS, h_sums + (size_t)j * LOM_NQSUMS, LOM_NQSUMS * 8);
    return LOM_OK;
}

static int quality_batch_reports(lom_map *m, const lom_quality_problem *p, int count, bool device_input, float max_dist,
                                 float min_eig_t, float min_eig_r, lom_quality_report *out, int *best)
{
    if (!quality_batch_args_ok(m, p, count, out)) return LOM_ERR_ARG;
    std::vector<double> sums((size_t)count * LOM_NQSUMS);
    int rc = quality_batch_core(m, p, count, device_input, max_dist, sums.data());
    if (rc != LOM_OK) return rc;
    for (int i = 0; i < count; i++)
        if ((rc = lom_quality_from_sums(sums.data() + (size_t)i * LOM_NQSUMS, (int64_t)p[i].n, min_eig_t, min_eig_r, out + i)) != LOM_OK)
            return rc;
    if (best) *best = lom_quality_batch_best(out, count);
    return LOM_OK;
}

int lom_match_quality_batch_sums(lom_map *m, const lom_quality_problem *p, int count, float max_dist, double *sums_out)
{
    if (!quality_batch_args_ok(m, p, count, sums_out)) return LOM_ERR_ARG;
    return quality_batch_core(m, p, count, false, max_dist, sums_out);
}

int lom_match_quality_batch_sums_device(lom_map *m, const lom_quality_problem *p, int count, float max_dist,
                                        double *sums_out)
{
    if (!quality_batch_args_ok(m, p, count, sums_out)) return LOM_ERR_ARG;
    return quality_batch_core(m, p, count, true, max_dist, sums_out);
}

int lom_match_quality_batch(lom_map *m, const lom_quality_problem *p, int count, float max_dist, float min_eig_t,
                            float min_eig_r, lom_quality_report *out, int *best)
{
    return quality_batch_reports(m, p, count, false, max_dist, min_eig_t, min_eig_r, out, best);
}

int lom_match_quality_batch_device(lom_map *m, const lom_quality_problem *p, int count, float max_dist, float min_eig_t,
                                   float min_eig_r, lom_quality_report *out, int *best)
{
    return quality_batch_reports(m, p, count, true, max_dist, min_eig_t, min_eig_r, out, best);
}

// outer iterations of the last device-resident align on this handle that the replay fold accounted for instead of running
int lom_debug_replayed_iterations(lom_map *m) { return m ? m->last_replayed : LOM_ERR_ARG; }

// parity entry: a whole align on the device-resident path (k_match / k_lm chain) that also returns what
// k_lm's policy saw in outer iteration `outer_index`: for every evaluation of that solve the point
// x = [q, t] it was made at and the 32 totals after the in-kernel reduction and exchange
int lom_debug_lm_trace(lom_map *m, const float *src, size_t n, size_t stride, const float guess_t[3],
                       const float guess_q[4], int outer_index, double *trace_out, int *n_evals_out, float out_t[3],
                       float out_q[4], lom_align_stats *stats)
{
    if (!m || (n && !src) || !guess_t || !guess_q || !trace_out || !n_evals_out || !out_t || !out_q ||
        !scan_args_ok(n, stride) || outer_index < 0 || outer_index >= 35)
        return LOM_ERR_ARG;
    if (m->comm || m->host_comm) return set_error(m, LOM_ERR_STATE, "not with an attached exchange");
    LOM_HIP(m, hipSetDevice(m->device));
    m->last_error.clear();
    const char *d_src = nullptr;
    int rc = stage_scan(m, src, n, stride, &d_src);
    if (rc != LOM_OK) return rc;
    server_stop(m);
    m->profiling = false;
    double raw[201];
    rc = align_chained(m, d_src, n, stride, guess_t, guess_q, out_t, out_q, stats, raw, outer_index);
    if (rc == kDeviceLoopGaveUp) return LOM_ERR_HIP;
    if (rc != LOM_OK) return rc;
    const int ne = (int)raw[200];
    *n_evals_out = ne;
    for (int e = 0; e < ne && e < 5; e++) std::memcpy(trace_out + (size_t)e * 40, raw + (size_t)e * 40, 40 * sizeof(double));
    return LOM_OK;
}

// parity entry: one form of the LM policy on given sums (no map: the policy sees nothing else).  form 0 is lm_core.hpp on
// the host; forms 1-3 are lm_wave.hpp's on one wave (k_policy_probe.hpp), all solves of the call in one launch.
int lom_debug_lm_policy(int form, int n_solves, const int *n_evals, const double *x0, const double *prior_b,
                        const double *sums, int *action_out, double *point_out, int *recorded_out,
                        int *evaluations_out, double *last_step_norm_out, double *cost_out)
{
    if (form < 0 || form > 3 || n_solves < 1 || n_solves > 4096 || !n_evals || !x0 || !prior_b || !sums || !action_out ||
        !point_out || !recorded_out || !evaluations_out || !last_step_norm_out || !cost_out)
        return LOM_ERR_ARG;
    for (int s = 0; s < n_solves; s++)
        if (n_evals[s] < 1 || n_evals[s] > kProbeMaxEvals) return LOM_ERR_ARG;
    const size_t ns = (size_t)n_solves, slots = ns * kProbeMaxEvals;
    for (size_t i = 0; i < slots; i++) action_out[i] = -1;
    std::memset(point_out, 0, slots * 7 * sizeof(double));
    if (form == 0) {
        for (size_t s = 0; s < ns; s++) {
            LmState S;
            for (int e = 0; e < n_evals[s]; e++) {
                const size_t slot = s * kProbeMaxEvals + (size_t)e;
                const int a = e == 0 ? lm_begin(S, sums + slot * 32, x0 + s * 7, prior_b + s * 3) : lm_feed(S, sums + slot * 32);
                action_out[slot] = a;
                std::memcpy(point_out + slot * 7, a == LM_EVAL ? S.cand : S.x, 7 * sizeof(double));
                if (a != LM_EVAL) break;
            }
            recorded_out[s] = S.recorded;
            evaluations_out[s] = S.evaluations;
            last_step_norm_out[s] = S.last_step_norm;
            cost_out[s] = S.cost;
        }
        return LOM_OK;
    }
    // one device buffer: the inputs, then the outputs, each 8-byte aligned
    const size_t o_x0 = 0, o_pb = o_x0 + ns * 7 * 8, o_sums = o_pb + ns * 3 * 8, o_point = o_sums + slots * 32 * 8,
                 o_lsn = o_point + slots * 7 * 8, o_cost = o_lsn + ns * 8, o_ne = o_cost + ns * 8, o_act = o_ne + ns * 4,
                 o_rec = o_act + slots * 4, o_ev = o_rec + ns * 4, total = o_ev + ns * 4;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) return LOM_ERR_HIP;  // forms 1-3 need a GPU
    char *d = nullptr;
    if (hipMalloc((void **)&d, total) != hipSuccess) return LOM_ERR_OOM;
    hipError_t e = hipMemset(d, 0, total);
    if (e == hipSuccess) e = hipMemset(d + o_act, 0xFF, slots * 4);
    if (e == hipSuccess) e = hipMemcpy(d + o_x0, x0, ns * 7 * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + o_pb, prior_b, ns * 3 * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + o_sums, sums, slots * 32 * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + o_ne, n_evals, ns * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        PolicyProbeArgs p;
        p.n_solves = n_solves;
        p.n_evals = (const int *)(d + o_ne);
        p.x0 = (const double *)(d + o_x0);
        p.prior_b = (const double *)(d + o_pb);
        p.sums = (const double *)(d + o_sums);
        p.action = (int *)(d + o_act);
        p.point = (double *)(d + o_point);
        p.recorded = (int *)(d + o_rec);
        p.evaluations = (int *)(d + o_ev);
        p.last_step_norm = (double *)(d + o_lsn);
        p.cost = (double *)(d + o_cost);
        if (form == 1)
            hipLaunchKernelGGL(k_policy_probe<1>, dim3(1), dim3(64), 0, 0, p);
        else if (form == 2)
            hipLaunchKernelGGL(k_policy_probe<2>, dim3(1), dim3(64), 0, 0, p);
        else
            hipLaunchKernelGGL(k_policy_probe<3>, dim3(1), dim3(64), 0, 0, p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(action_out, d + o_act, slots * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(point_out, d + o_point, slots * 7 * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(recorded_out, d + o_rec, ns * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(evaluations_out, d + o_ev, ns * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(last_step_norm_out, d + o_lsn, ns * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(cost_out, d + o_cost, ns * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? LOM_OK : LOM_ERR_HIP;
}

// diagnostic: per-workgroup phase stamps of one correspondence launch (shader clock ticks)
int lom_debug_match_stamps(lom_map *m, const float *d_src, size_t n, size_t stride, const float t[3],
                           const float q[4], float max_dist, unsigned long long *stamps_out, size_t cap_blocks,
                           uint32_t *n_blocks_out)
{
    if (!m || !d_src || !n || !t || !q || !stamps_out || !n_blocks_out) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    int rc = scan_buffers(m, (uint32_t)n, false);
    if (rc != LOM_OK) return rc;
    server_stop(m);
    const uint32_t nb = match_grid((uint32_t)n);
    if (nb > cap_blocks) return LOM_ERR_ARG;
    unsigned long long *d_st = nullptr;
    LOM_HIP(m, hipMalloc(&d_st, (size_t)nb * 64));
    PoseArgs P;
    pose_args(t, q, sq_f32(max_dist), P);
    for (int rep = 0; rep < 3; rep++)  // the last launch's stamps are kept (warm caches, like an align)
        hipLaunchKernelGGL((k_match<kMatchG, kMatchRows, kMatchMinWaves, true>), dim3(nb), dim3(kMatchThreads), 0, m->stream, view_of(m),
                           (const char *)d_src, stride, (uint32_t)n, P, (int32_t *)m->scan_idx.p,
                           (MatchRec *)m->scan_on.p, (QStat *)nullptr, d_block_counters(m), d_st);
    hipError_t e = hipMemcpyAsync(stamps_out, d_st, (size_t)nb * 64, hipMemcpyDeviceToHost, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    (void)hipFree(d_st);
    if (e != hipSuccess) return set_error(m, LOM_ERR_HIP, "stamp readback", e);
    *n_blocks_out = nb;
    return LOM_OK;
}

int lom_match_align_repeat(lom_map *m, const float *d_src, size_t n, size_t stride, const float guess_t[3],
                           const float guess_q[4], int reps, float out_t[3], float out_q[4],
                           lom_align_stats *total)
{
    if (!m || (n && !d_src) || !guess_t || !guess_q || !out_t || !out_q || reps < 1 || !stride_ok(stride))
        return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    m->last_error.clear();
    lom_align_stats acc;
    std::memset(&acc, 0, sizeof acc);
    for (int r = 0; r < reps; r++) {
        lom_align_stats st;
        const int rc = align_device(m, (const char *)d_src, n, stride, guess_t, guess_q, out_t, out_q, &st);
        if (rc != LOM_OK) return rc;
        acc.outer_iterations += st.outer_iterations;
        acc.lm_iterations += st.lm_iterations;
        acc.evaluations += st.evaluations;
        acc.match_launches += st.match_launches;
        acc.queries += st.queries;
        acc.valid_last = st.valid_last;
        acc.cand_total += st.cand_total;
        acc.occ_total += st.occ_total;
        acc.final_cost = st.final_cost;
        acc.last_step_norm = st.last_step_norm;
        acc.match_kernel_ms += st.match_kernel_ms;
        acc.algorithmic_bytes += st.algorithmic_bytes;
        acc.host_launch_ms += st.host_launch_ms;
        acc.host_wait_ms += st.host_wait_ms;
        acc.profiled_launches += st.profiled_launches;
        acc.host_fallback += st.host_fallback;
        acc.lm_kernel_ms += st.lm_kernel_ms;
        acc.lm_profiled_launches += st.lm_profiled_launches;
        acc.lm_workgroups = st.lm_workgroups;
    }
    if (total) *total = acc;
    return LOM_OK;
}

int lom_align_batch_best(const lom_align_result *r, int count)
{
    if (!r || count <= 0) return -1;
    int best = 0;
    for (int i = 1; i < count; i++) {
        const lom_align_stats &a = r[i].stats, &b = r[best].stats;
        if (a.valid_last > b.valid_last || (a.valid_last == b.valid_last && a.final_cost < b.final_cost)) best = i;
    }
    return best;
}

int lom_match_align_batch(lom_map *m, const lom_align_problem *p, int count, lom_align_result *out, int *best)
{
    if (!m || count < 0 || (count > 0 && (!p || !out))) return LOM_ERR_ARG;
    return align_batch(m, p, count, out, best, false);
}

int lom_match_align_batch_device(lom_map *m, const lom_align_problem *p, int count, lom_align_result *out, int *best)
{
    if (!m || count < 0 || (count > 0 && (!p || !out))) return LOM_ERR_ARG;
    return align_batch(m, p, count, out, best, true);
}

int lom_match_align_multi(lom_map *runner, const lom_align_multi_problem *p, int count, lom_align_result *out, int *best)
{
    return align_multi_entry(runner, p, count, out, best, false);
}

int lom_match_align_multi_device(lom_map *runner, const lom_align_multi_problem *p, int count, lom_align_result *out,
                                 int *best)
{
    return align_multi_entry(runner, p, count, out, best, true);
}

int lom_match_align(lom_map *m, const float *src, size_t n, size_t stride, const float guess_t[3],
                    const float guess_q[4], float out_t[3], float out_q[4], lom_align_stats *stats)
{
    if (!m || (n && !src) || !guess_t || !guess_q || !out_t || !out_q || !stride_ok(stride)) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    m->last_error.clear();
    const char *d_src = nullptr;
    int rc = stage_scan(m, src, n, stride, &d_src);
    if (rc != LOM_OK) return rc;
    return align_device(m, d_src, n, stride, guess_t, guess_q, out_t, out_q, stats);
}

}  // extern "C"
