// The device-resident single align: the chain of (k_match, k_lm) pairs, its report protocol, the ways an align can go
// (device-resident, device-to-device between ranks, host-driven) and the lom_match_align* entry points.  Host code only:
// the kernels are launched through match.hip's typed launchers (match_launch.hpp).
//
// Built with -ffp-contract=off (see voxel_map.hip).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lom_internal.hpp"
#include "match_launch.hpp"

namespace lom {

// Single GPU, no exchange: the outer loop runs on the device.  One (k_match, k_lm) pair per outer
// iteration; the pose travels from pair to pair through AlignState in HBM, so the host enqueues
// pairs without waiting for results (chain_start / chain_continue).

// compute units a launch of this handle reaches: its partition's where it has one
int device_cus(lom_map *m, uint32_t *out)
{
    int cus = 0;
    LOM_HIP(m, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m->device));
    *out = m->partition_cus ? m->partition_cus : (uint32_t)std::max(1, cus);
    return LOM_OK;
}

// k_lm's workgroups wait for each other inside the kernel, so all of them must be resident at once:
// the grid never exceeds what the occupancy query admits on this device (the shapes and their grids: match_plan.cpp).
static int lm_block_limit(lom_map *m, LmShape shape, uint32_t *out)
{
    uint32_t &cached = m->lm_max_blocks[shape];
    if (!cached) {
        int per_cu = 0, rc;
        uint32_t cus = 0;
        if ((rc = lm_blocks_per_cu(m, shape, false, &per_cu)) != LOM_OK) return rc;
        if ((rc = device_cus(m, &cus)) != LOM_OK) return rc;
        cached = (uint32_t)std::max(1, per_cu * (int)cus);
    }
    *out = cached;
    return LOM_OK;
}

// the grid of a solve: one point per point thread up to the shape's cap, and no more than is resident at once
int lm_grid(lom_map *m, uint32_t n, LmShape shape, uint32_t *nb)
{
    uint32_t limit = 0;
    const int rc = lm_block_limit(m, shape, &limit);
    if (rc != LOM_OK) return rc;
    *nb = lm_blocks(n, shape, limit);
    return LOM_OK;
}

// the single align: k_lm's argument
static void set_guess(const float gt[3], const float gq[4], LmInit &init)
{
    guess_fields(gt, gq, init.t, init.q, init.prior_b, init.max_sq);
}

// Wait until report `want` of a chain has arrived.  kReportArrived, kReportError (a workgroup gave up: the error word,
// seen before or with the report) or a negative status recorded with fail (the stream ended or failed without
// either); the caller advances its sequence counter in every case.  An idle stream is looked at once more for the
// report OR the error word: the batched align needs both (a problem that gave up writes no further report), and for
// the single align it is the same as looking for the report alone, since its caller tests the error word first.
int wait_report(lom_map *m, const volatile AlignReport *rp, unsigned long long want, const char *solve)
{
    uint64_t spins = 0;
    while (rp->seq != want) {
        __builtin_ia32_pause();
        if (rp->error) break;
        if ((++spins & 0x3FFF) == 0) {
            const hipError_t e = hipStreamQuery(m->stream);
            if (e == hipSuccess) {
                if (rp->seq == want || rp->error) break;
                return fail(m, LOM_ERR_HIP, (std::string(solve) + " ended without a report").c_str());
            } else if (e != hipErrorNotReady) {
                return fail(m, LOM_ERR_HIP, (std::string("stream failed during the ") + solve).c_str(), e);
            }
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return rp->error ? kReportError : kReportArrived;
}

// an align's result from its final report
void result_from_report(const volatile AlignReport *rp, bool counted, uint32_t nb, lom_align_result &r)
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
        if ((rc = ensure(m, m->xrec, kExchangeSetBytes)) != LOM_OK) return rc;
        LOM_HIP(m, hipMemsetAsync(m->xrec.p, 0, kExchangeSetBytes, m->stream));
    }
    if ((rc = eval_kernel_attrs(m)) != LOM_OK) return rc;
    ScanCtx c{m, d_src, stride, (uint32_t)n, 0};
    LmInit init;
    set_guess(guess_t, guess_q, init);
    // ranks of one node keep to 64 workgroups each: a shard is an eighth of the cloud, and ranks that share a GPU
    // (tests, rehearsals) must all be resident together
    LmShape shape = lm_shape(c.n);
    if (m->p2p && shape == kLmBig) shape = kLmMid;
    uint32_t nb = 0;
    if ((rc = lm_grid(m, c.n, shape, &nb)) != LOM_OK) return rc;
    double *d_trace = nullptr;  // lom_debug_lm_trace: k_lm of outer iteration `trace_outer` records its evaluations
    if (trace_out) {
        if ((rc = ensure(m, m->dbg_trace, 201 * 8)) != LOM_OK) return rc;
        d_trace = m->dbg_trace.as<double>();
        LOM_HIP(m, hipMemsetAsync(d_trace, 0, 201 * 8, m->stream));
    }
    volatile AlignReport *rp = reinterpret_cast<volatile AlignReport *>(m->h_report);
    rp->error = 0;
    const unsigned long long seq0 = m->report_seq;
    const int nranks = m->p2p ? m->nranks : 1;
    // the same count on every rank: ranks issue the same sequence of aligns
    const unsigned long long epoch = m->p2p ? ++m->p2p_epoch : ~0ull;
    const int give_up_outer = m->test_give_up_outer;  // one shot
    m->test_give_up_outer = -1;
    unsigned long long *dbg = nullptr;  // LOM_OPT_DEBUG_LM_STAMPS: phase stamps of the last k_lm of the align
    if (m->opt_debug_lm) {
        if ((rc = ensure(m, m->dbg_stamps, 4096)) != LOM_OK) return rc;
        dbg = m->dbg_stamps.as<unsigned long long>();
        LOM_HIP(m, hipMemsetAsync(dbg, 0, 40 * 8, m->stream));
    }
    // The replay fold (k_lm's tail, LOM_OPT_REPLAY_FOLD): on for the single align of one GPU -- with or without an exchange
    // attached, as long as it has one rank: nothing is exchanged then, and the align must not cost more for the
    // communicator being there.  Out of scope, and so off: ranks that exchange sums (nranks > 1: every rank would take
    // the same decision, but a disagreement is a hang) and the batched chains (kBatch compiles it out).  lom_debug_lm_trace runs the iteration it asks about, and so does an align with
    // LOM_OPT_TEST_GIVE_UP_AT_OUTER armed: the k_lm it names has to run to give up.  An align that carries the profiling
    // events (lom_map_set_profiling: every N-th) is a measurement of the kernels: each bracketed pair runs, so that
    // profiled_launches stays match_launches and no empty kernel enters match_kernel_ms / lm_kernel_ms.
    const unsigned long long fold_seq = (m->opt_replay_fold && nranks <= 1 && !trace_out && give_up_outer < 0 && !m->profiling)
                                            ? seq0 + (unsigned long long)kPairsAhead
                                            : 0ull;
    m->last_replayed = 0;
    int lm_events = 0;
    auto launch_pair = [&](int i) -> int {
        int r = launch_match(c, guess_t, guess_q, sq_f32(0.3f), false, i > 0);
        if (r != LOM_OK) return r;
        const double t_l = now_s();
        m->lm_seq += 8;  // a solve spends at most 5 evaluations
        const int set_base = (int)((m->lm_launches++ & 1ull) * 2ull);  // same launch count on every rank
        launch_k_lm(m, shape, nb, c.n, init, i == 0, c.match_blocks, seq0 + (unsigned long long)i + 1, fold_seq, dbg, set_base,
                    epoch, (d_trace && i == trace_outer) ? d_trace : nullptr, i == give_up_outer);
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
            fail(m, LOM_ERR_HIP, "device solve: a workgroup timed out waiting for the others");
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


int align_device_paths(lom_map *m, const char *d_src, size_t n, size_t stride, const float guess_t[3],
                              const float guess_q[4], float out_t[3], float out_q[4], lom_align_stats *stats)
{
    if (n >= kMaxScanPoints) return fail(m, LOM_ERR_ARG, "too many source points");
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
                return fail(m, LOM_ERR_COMM, why.c_str());
            }
            if (verdict[1] != 0.0) {  // some rank cannot continue: the same for all
                m->p2p = false;
                (void)hipStreamSynchronize(m->stream);
                if (hard) return rc;
                return fail(m, LOM_ERR_COMM, "a peer rank failed during a device-to-device align");
            }
            if (verdict[0] == 0.0) return LOM_OK;
            fprintf(stderr, "lidar_odometry_amd: device-to-device exchange given up on %d rank(s) (%s); rank %d redoes the align over the host exchange\n",
                    (int)verdict[0], gave_up ? m->error.c_str() : "a peer gave up", m->rank);
            (void)hipStreamSynchronize(m->stream);
            m->p2p = false;
        } else if (rc != kDeviceLoopGaveUp) {
            return rc;
        }
        // single GPU: k_lm's workgroups were not all resident within their patience (another process or
        // handle on the GPU, a CU mask): same align again through the host-driven loop, whose
        // workgroups never wait for each other
        m->error.clear();
        fell_back = true;
    }
    int rc = scan_buffers(m, (uint32_t)n, false);
    if (rc != LOM_OK) return rc;
    ScanCtx c{m, d_src, stride, (uint32_t)n, 0};
    const lom_align_hooks hooks = eval_hooks(c);
    m->last_replayed = 0;
    lom_align_stats st;
    rc = lom_align_with_hooks(&hooks, guess_t, guess_q, out_t, out_q, &st);
    server_stop(m);
    if (!c.counted) st.algorithmic_bytes = 0.0;  // (SURVEY.md 8d's bytes need the counts: LOM_OPT_COUNT_CANDIDATES)
    if (rc != LOM_OK) {
        if (m->error.empty()) fail(m, rc, "align failed");
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

}  // namespace lom

using namespace lom;

extern "C" {

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
    m->error.clear();
    return align_device(m, (const char *)d_src, n, stride, guess_t, guess_q, out_t, out_q, stats);
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
    if (m->comm || m->host_comm) return fail(m, LOM_ERR_STATE, "not with an attached exchange");
    LOM_HIP(m, hipSetDevice(m->device));
    m->error.clear();
    const char *d_src = nullptr;
    int rc = upload_scan(m, m->scan_src, src, n, stride, &d_src);
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

int lom_match_align_repeat(lom_map *m, const float *d_src, size_t n, size_t stride, const float guess_t[3],
                           const float guess_q[4], int reps, float out_t[3], float out_q[4],
                           lom_align_stats *total)
{
    if (!m || (n && !d_src) || !guess_t || !guess_q || !out_t || !out_q || reps < 1 || !stride_ok(stride))
        return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    m->error.clear();
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

int lom_match_align(lom_map *m, const float *src, size_t n, size_t stride, const float guess_t[3],
                    const float guess_q[4], float out_t[3], float out_q[4], lom_align_stats *stats)
{
    if (!m || (n && !src) || !guess_t || !guess_q || !out_t || !out_q || !stride_ok(stride)) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    m->error.clear();
    const char *d_src = nullptr;
    int rc = upload_scan(m, m->scan_src, src, n, stride, &d_src);
    if (rc != LOM_OK) return rc;
    return align_device(m, d_src, n, stride, guess_t, guess_q, out_t, out_q, stats);
}

}  // extern "C"
