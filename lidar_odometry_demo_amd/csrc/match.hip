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
// and launches them: the kernel tables and one typed launcher per kernel form (match_launch.hpp), the single search, the
// host-driven evaluation, the device-to-device attach, the profiling and debug probes.  The aligns and the quality reports
// built on the launchers are host code of their own: align.hip, align_batch.hip, quality_report.hip.
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
#include "lom_internal.hpp"
#include "match_launch.hpp"
#include "pose_math.hpp"

namespace lom {

// max_sq: the f32 threshold the f32 squared distances are compared with (strictly below).  findMatchingPairs forms it
// as max_dist * max_dist in f32 (voxel_grid.h:215); getCorrespondence takes a double (:164), see threshold_f32()
void pose_args(const float t[3], const float q[4], float max_sq, PoseArgs &P)
{
    float R[9];
    rotation_matrix(q, R);  // voxel_grid.h:212 transform.rotationMatrix().cast<double>()
    for (int i = 0; i < 9; i++) P.R[i] = (double)R[i];
    for (int i = 0; i < 3; i++) P.t[i] = (double)t[i];
    P.max_sq = max_sq;
}

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

int scan_buffers(lom_map *m, uint32_t n, bool want_stats)
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

static uint32_t *d_block_counters(lom_map *m) { return (uint32_t *)(m->results.as<char>() + 1024); }
static double *d_sums(lom_map *m) { return m->results.as<double>(); }

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

// The launchers: what a form does not read is filled here and nowhere else.
void launch_k_match(lom_map *m, bool prev, bool count, uint32_t blocks, const char *d_src, size_t stride, uint32_t n,
                    const PoseArgs &P, int32_t *out_idx, MatchRec *out_rec, QStat *out_stat, uint32_t *block_counters,
                    const AlignState *state)
{
    hipLaunchKernelGGL(match_kernel(state != nullptr, prev, count, false), dim3(blocks), dim3(kMatchThreads), 0, m->stream,
                       view_of(m), d_src, stride, n, P, out_idx, out_rec, out_stat, block_counters,
                       (unsigned long long *)nullptr, state, (const BatchProblem *)nullptr);
}

void launch_k_match_batch(lom_map *m, bool prev, bool count, dim3 grid, const BatchProblem *desc)
{
    PoseArgs P;
    std::memset(&P, 0, sizeof P);
    hipLaunchKernelGGL(match_kernel(true, prev, count, true), grid, dim3(kMatchThreads), 0, m->stream, MapView{},
                       (const char *)nullptr, (size_t)0, 0u, P, (int32_t *)nullptr, (MatchRec *)nullptr, (QStat *)nullptr,
                       (uint32_t *)nullptr, (unsigned long long *)nullptr, (const AlignState *)nullptr, desc);
}

// the instantiation that stamps its phases (lom_debug_match_stamps)
static void launch_k_match_stamps(lom_map *m, uint32_t blocks, const char *d_src, size_t stride, uint32_t n,
                                  const PoseArgs &P, unsigned long long *d_stamps)
{
    hipLaunchKernelGGL((k_match<kMatchG, kMatchRows, kMatchMinWaves, true>), dim3(blocks), dim3(kMatchThreads), 0, m->stream,
                       view_of(m), d_src, stride, n, P, m->scan_idx.as<int32_t>(), m->scan_on.as<MatchRec>(), (QStat *)nullptr,
                       d_block_counters(m), d_stamps);
}

void launch_k_quality(lom_map *m, uint32_t blocks, const MatchRec *rec, uint32_t n, const EvalArgs &E, double *part,
                      float *residual_out, double *out)
{
    hipLaunchKernelGGL(k_quality, dim3(blocks), dim3(kEvalThreads), 0, m->stream, rec, n, E, part, residual_out);
    hipLaunchKernelGGL(k_quality_sum, dim3(1), dim3(64), 0, m->stream, (const double *)part, blocks, out);
}

void launch_k_quality_batch(lom_map *m, uint32_t blocks, uint32_t problems, const QualBatchProblem *desc)
{
    hipLaunchKernelGGL(k_quality_batch, dim3(blocks, problems), dim3(kEvalThreads), 0, m->stream, desc);
    hipLaunchKernelGGL(k_quality_batch_sum, dim3(problems), dim3(64), 0, m->stream, desc);
}

void fill_search(BatchProblem &d, AlignState &state, const MapView &map, const char *src, size_t stride, uint32_t n,
                 uint32_t match_blocks, MatchRec *rec, uint32_t *block_counters, AlignState *d_state, const float t[3],
                 const float q[4], float max_sq)
{
    std::memset(&state, 0, sizeof state);
    pose_args(t, q, max_sq, state.P);
    std::memset(&d, 0, sizeof d);
    d.map = map;
    d.src = src;
    d.stride = stride;
    d.rec = rec;
    d.block_counters = block_counters;
    d.state = d_state;
    d.n = n;
    d.match_blocks = match_blocks;
}

int launch_match(ScanCtx &c, const float t[3], const float q[4], float max_sq, bool stats, bool chained, int count_mode)
{
    lom_map *m = c.m;
    PoseArgs P;
    std::memset(&P, 0, sizeof P);
    if (!chained) pose_args(t, q, max_sq, P);
    c.match_blocks = c.n ? match_grid(c.n, launch_partition(m)) : 0;
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
        QStat *st = (stats && !chained) ? m->scan_stats.as<QStat>() : nullptr;
        // (a chained launch always follows a search of the same scan: launch_pair's first pair is not chained)
        const bool prev = (chained || c.have_prev) && !m->opt_no_temporal;
        const bool count = count_mode < 0 ? m->opt_count : count_mode != 0;
        const AlignState *as = chained ? m->align_state.as<const AlignState>() : nullptr;
        launch_k_match(m, prev, count, c.match_blocks, c.d_src, c.stride, c.n, P, m->scan_idx.as<int32_t>(),
                       m->scan_on.as<MatchRec>(), st, d_block_counters(m), as);
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

int eval_kernel_attrs(lom_map *m)
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
void server_stop(lom_map *m)
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
                    return fail(m, LOM_ERR_HIP, "stream failed while waiting for an evaluation", e);
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
                               m->scan_on.as<const MatchRec>(), c.n, E, (const uint32_t *)d_block_counters(m),
                               fresh_match ? c.match_blocks : 0u, m->partials.as<double>(), seq);
        }
        hipLaunchKernelGGL(k_sum_records, dim3(1), dim3(64), 0, m->stream, m->partials.as<const double>(), nb, c.n,
                           d_sums(m));
        LOM_HIP(m, hipGetLastError());
        c.launch_s += now_s() - t_launch;
        const double t_wait = now_s();
        rc = ensure(m, m->gather, (size_t)m->nranks * LOM_NSUMS * 8);
        if (rc != LOM_OK) return rc;
        rc = comm_allgather_sums(m, d_sums(m), m->gather.as<double>(), LOM_NSUMS);
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
                                   m->scan_on.as<const MatchRec>(), c.n, E, (const uint32_t *)d_block_counters(m),
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
            if (attempt >= 3) return fail(m, LOM_ERR_HIP, "evaluation server did not answer");
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

lom_align_hooks eval_hooks(ScanCtx &c)
{
    lom_map *m = c.m;
    lom_align_hooks hooks;
    hooks.user = &c;
    hooks.match_eval = hook_match_eval;
    hooks.eval_fixed = hook_eval_fixed;
    // the rank-ordered all-gather sits inside launch_eval.  With more than one rank the hook is there all the same, doing
    // nothing: the driver's replay fold (align_driver.cpp) is for aligns whose sums nobody exchanges
    hooks.allreduce = ((m->comm || m->host_comm) && m->nranks > 1) ? hook_sums_exchanged : nullptr;
    return hooks;
}

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

// What belongs to a shape: its geometry and its k_lm instantiations (every instantiation has the same signature).
using LmKernel = decltype(&k_lm<(int)kLmSmallThreads>);
struct LmForm {
    LmKernel single;  // the single align's kernel
    LmKernel batch;   // the batched align's
    LmKernel twice;   // the single align's with the policy run twice (LOM_DEBUG_LM_TWICE=1; kLmSmall2 only)
};
static const LmForm &lm_form(LmShape shape)
{
    constexpr int S = (int)kLmSmallThreads, E = kEvalThreads, C = (int)kMaxLmBlocks, CB = (int)kMaxLmBlocksBig;
    static_assert(kLmSmallLaunch == (uint32_t)lm_threads(S) && lm_threads(E) == E, "kLmGeometry's launch sizes");
    static_assert(sizeof(XWord) * 2 * kMaxLmBlocksBig * kRecWords == kExchangeSetBytes, "a solve's exchange sets");
    static const LmForm forms[4] = {
        /* kLmSmall  */ {k_lm<S>, k_lm<S, C, 1, false, true>, nullptr},
        /* kLmMid    */ {k_lm<E>, k_lm<E, C, 1, false, true>, nullptr},
        /* kLmBig    */ {k_lm<E, CB>, k_lm<E, CB, 1, false, true>, nullptr},
        /* kLmSmall2 */ {k_lm<S, C, 2>, k_lm<S, C, 2, false, true>, k_lm<S, C, 2, true>},
    };
    return forms[shape];
}

int lm_blocks_per_cu(lom_map *m, LmShape shape, bool batch, int *per_cu)
{
    const LmForm &f = lm_form(shape);
    LOM_HIP(m, hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, reinterpret_cast<const void *>(batch ? f.batch : f.single),
                                                            (int)kLmGeometry[shape].threads, 0));
    return LOM_OK;
}

void launch_k_lm(lom_map *m, LmShape shape, uint32_t blocks, uint32_t n, const LmInit &init, bool first_outer,
                 uint32_t match_blocks, unsigned long long report_seq, unsigned long long fold_report_seq,
                 unsigned long long *dbg_stamps, int p2p_set_base, unsigned long long p2p_epoch, double *dbg_trace,
                 bool give_up)
{
    const LmForm &form = lm_form(shape);
    const LmKernel kernel = (m->opt_debug_lm_twice && form.twice) ? form.twice : form.single;
    P2pArgs px = p2p_args(m);
    px.set_base = p2p_set_base;
    px.epoch = p2p_epoch;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kLmGeometry[shape].threads), 0, m->stream, m->scan_on.as<const MatchRec>(), n,
                       m->align_state.as<AlignState>(), init, first_outer ? 1 : 0, (const uint32_t *)d_block_counters(m),
                       match_blocks, m->xrec.as<XWord>(), m->lm_seq, reinterpret_cast<AlignReport *>(m->d_report), report_seq,
                       fold_report_seq, m->patience_ticks, dbg_stamps, px, dbg_trace, give_up ? 1 : 0,
                       (const BatchProblem *)nullptr);
}

void launch_k_lm_batch(lom_map *m, LmShape shape, dim3 grid, unsigned long long seq_base, unsigned long long report_seq,
                       bool first_outer, bool give_up, const BatchProblem *desc)
{
    LmInit init;
    std::memset(&init, 0, sizeof init);
    hipLaunchKernelGGL(lm_form(shape).batch, grid, dim3(kLmGeometry[shape].threads), 0, m->stream, (const MatchRec *)nullptr, 0u,
                       (AlignState *)nullptr, init, first_outer ? 1 : 0, (const uint32_t *)nullptr, 0u, (XWord *)nullptr,
                       seq_base, (AlignReport *)nullptr, report_seq, 0ull, m->patience_ticks, (unsigned long long *)nullptr,
                       p2p_args(m), (double *)nullptr, give_up ? 1 : 0, desc);
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
    if ((rc = upload_scan(m, m->scan_src, src, n, stride, &d_src)) != LOM_OK) return rc;
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
    if (m->comm) return fail(m, LOM_ERR_STATE, "an RCCL communicator is already attached");
    LOM_HIP(m, hipSetDevice(m->device));
    int rank = 0, nranks = 1;
    if (host_comm_rank(hc, &rank, &nranks) != LOM_OK) return LOM_ERR_ARG;
    if (nranks > kP2pMaxRanks) return fail(m, LOM_ERR_ARG, "device-to-device exchange: at most 8 ranks");
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
        return fail(m, LOM_ERR_COMM, "device-to-device exchange: handle exchange failed");
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
                           m->patience_ticks, m->results.as<uint32_t>());
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(res, m->results.as<uint32_t>(), 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
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
        return fail(m, LOM_ERR_COMM, "device-to-device exchange failed its self-test on some rank");
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
    if (rc != LOM_OK) return fail(m, rc, "lom_profile_match failed");
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

// parity entry: one search at the f32 pose, then ONE evaluation of the reduced normal equations at (q, t)
// through the host-driven path's kernels (k_match + k_eval_server: accumulate_point, LDS reduction,
// record per workgroup, workgroup-ordered host sum)
int lom_debug_eval_sums(lom_map *m, const float *src, size_t n, size_t stride, const float pose_t[3],
                        const float pose_q[4], const double q[4], const double t[3], double out[LOM_NSUMS])
{
    if (!m || (n && !src) || !pose_t || !pose_q || !q || !t || !out || !scan_args_ok(n, stride)) return LOM_ERR_ARG;
    if (m->comm || m->host_comm) return fail(m, LOM_ERR_STATE, "not with an attached exchange");
    LOM_HIP(m, hipSetDevice(m->device));
    m->error.clear();
    const char *d_src = nullptr;
    int rc = upload_scan(m, m->scan_src, src, n, stride, &d_src);
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
    DeviceBuf buf;
    if (alloc(buf, total) != hipSuccess) return LOM_ERR_OOM;
    char *d = buf.as<char>();
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
    DeviceBuf st;
    LOM_HIP(m, alloc(st, (size_t)nb * 64));
    unsigned long long *d_st = st.as<unsigned long long>();
    PoseArgs P;
    pose_args(t, q, sq_f32(max_dist), P);
    for (int rep = 0; rep < 3; rep++)  // the last launch's stamps are kept (warm caches, like an align)
        launch_k_match_stamps(m, nb, (const char *)d_src, stride, (uint32_t)n, P, d_st);
    hipError_t e = hipMemcpyAsync(stamps_out, d_st, (size_t)nb * 64, hipMemcpyDeviceToHost, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    if (e != hipSuccess) return fail(m, LOM_ERR_HIP, "stamp readback", e);
    *n_blocks_out = nb;
    return LOM_OK;
}

}  // extern "C"
