// The batched and the multi-map align (lom_match_align_batch* / lom_match_align_multi*): K solves side by side in one
// device-resident chain.  Host code only: the kernels are launched through match.hip's typed launchers
// (match_launch.hpp); the chain protocol is align.hip's.
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
//   floor(CUs x blocks per CU / the group's largest nb), CUs of the context's partition where it has one
//   (plan_align_rounds, match_plan.cpp: plain C++, tested on the CPU).  Blocks per CU: the occupancy query
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
    uint32_t &cached = m->batch.per_cu[shape];
    if (!cached) {
        int per_cu = 0;
        const int rc = lm_blocks_per_cu(m, shape, true, &per_cu);
        if (rc != LOM_OK) return rc;
        cached = (uint32_t)std::max(1, std::min(per_cu, (int)kBatchBlocksPerCuCap));
    }
    *out = cached;
    return LOM_OK;
}

// the solve's view of a problem's guess, on top of fill_search: the descriptor's fields k_lm reads when `first`, and the
// f32 pose in its AlignState
static void set_guess(const float gt[3], const float gq[4], BatchProblem &d, AlignState &state)
{
    guess_fields(gt, gq, d.guess_t, d.guess_q, d.prior_b, d.max_sq);
    for (int a = 0; a < 3; a++) state.pose_t[a] = gt[a];
    for (int a = 0; a < 4; a++) state.pose_q[a] = gq[a];
}

// all problems through the device-resident chain; gave_up[i]: problem i's solve gave up (to be redone)
static int align_batch_chained(lom_map *m, const BatchItem *it, int count, lom_align_result *out, std::vector<char> &gave_up,
                               double &launch_s, double &wait_s)
{
    static_assert(sizeof(AlignReport) <= 256, "one report slot");
    const uint32_t part = launch_partition(m);
    std::vector<AlignPlanProblem> prob(count);
    std::vector<uint32_t> mb(count);
    for (int i = 0; i < count; i++) {
        const uint32_t n = it[i].n;
        prob[i] = AlignPlanProblem{n, 0u, it[i].map->opt_count, !it[i].map->opt_no_temporal, it[i].give_up_outer};
        const int rc = lm_grid(m, n, lm_shape(n), &prob[i].nb);
        if (rc != LOM_OK) return rc;
        mb[i] = n ? match_grid(n, part) : 0u;
    }
    // what the plan needs from the device: its compute units, k_lm's blocks per CU of the shapes that occur
    uint32_t cus = 0, per_cu[4] = {};
    int rc = device_cus(m, &cus);
    if (rc != LOM_OK) return rc;
    for (int i = 0; i < count; i++) {
        const LmShape shape = lm_shape(it[i].n);
        if (!per_cu[shape] && (rc = lm_batch_per_cu(m, shape, &per_cu[shape])) != LOM_OK) return rc;
    }
    AlignPlan plan;
    plan_align_rounds(prob.data(), count, cus, per_cu, m->batch.test_round_max, plan);
    const std::vector<int> &order = plan.order;
    const std::vector<AlignRound> &rounds = plan.rounds;
    int max_slots = 0;
    for (const AlignRound &r : rounds) max_slots = std::max(max_slots, r.size);
    // buffers: records and k_match counters per problem, exchange sets per round slot, states + descriptors per problem
    std::vector<size_t> off_rec(count), off_cnt(count);
    BlockLayout rec, cnt, dev;  // dev: the states, then the descriptors (the staging block is its copy)
    for (int i = 0; i < count; i++) {
        off_rec[i] = rec.take((size_t)std::max(it[i].n, 1u) * sizeof(MatchRec));
        off_cnt[i] = cnt.take((size_t)std::max(mb[i], 1u) * kMatchCounterBytes);
    }
    dev.take((size_t)count * sizeof(AlignState));
    const size_t off_desc = dev.take((size_t)count * sizeof(BatchProblem)), dev_bytes = dev.end;
    if ((rc = ensure(m, m->batch.rec, rec.next)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->batch.cnt, cnt.next)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->batch.dev, dev_bytes)) != LOM_OK) return rc;
    {
        void *before = m->batch.xrec.p;
        if ((rc = ensure(m, m->batch.xrec, (size_t)max_slots * kExchangeSetBytes)) != LOM_OK) return rc;
        if (m->batch.xrec.p != before)  // fresh sets: no word may carry a sequence number of this call
            LOM_HIP(m, hipMemsetAsync(m->batch.xrec.p, 0, m->batch.xrec.bytes, m->stream));
    }
    if ((rc = ensure_pinned(m, m->batch.stage, dev_bytes, std::max(dev_bytes, (size_t)4096), hipHostMallocDefault,
                            "hipHostMalloc(batch staging)")) != LOM_OK)
        return rc;
    {
        bool fresh = false;
        const size_t slots = std::max((size_t)count, (size_t)16);
        if ((rc = ensure_pinned(m, m->batch.reports, (size_t)count * 256, slots * 256, hipHostMallocMapped | hipHostMallocCoherent,
                                "hipHostMalloc(batch reports)", &fresh)) != LOM_OK)
            return rc;
        if (fresh) std::memset(m->batch.reports.h, 0, m->batch.reports.bytes);
    }
    // states (the guess as the first search's pose) and descriptors, in `order`, one copy to the device
    AlignState *h_states = reinterpret_cast<AlignState *>(m->batch.stage.h);
    BatchProblem *h_desc = reinterpret_cast<BatchProblem *>((char *)m->batch.stage.h + off_desc);
    AlignState *d_states = reinterpret_cast<AlignState *>(m->batch.dev.p);
    const BatchProblem *d_desc = reinterpret_cast<const BatchProblem *>(m->batch.dev.as<char>() + off_desc);
    for (const AlignRound &r : rounds)
        for (int k = 0; k < r.size; k++) {
            const int j = r.first + k, i = order[j];
            AlignState &st = h_states[j];
            BatchProblem &d = h_desc[j];
            fill_search(d, st, view_of(it[i].map), it[i].src, it[i].stride, it[i].n, mb[i],
                        reinterpret_cast<MatchRec *>(m->batch.rec.as<char>() + off_rec[i]),
                        reinterpret_cast<uint32_t *>(m->batch.cnt.as<char>() + off_cnt[i]), d_states + j, it[i].gt, it[i].gq,
                        sq_f32(0.3f));  // cloud_matcher.cpp:139
            d.report = reinterpret_cast<AlignReport *>((char *)m->batch.reports.d + (size_t)j * 256);
            d.xrec = m->batch.xrec.as<char>() + (size_t)k * kExchangeSetBytes;
            d.lm_blocks = prob[i].nb;
            set_guess(it[i].gt, it[i].gq, d, st);
            volatile AlignReport *rp = reinterpret_cast<volatile AlignReport *>((char *)m->batch.reports.h + (size_t)j * 256);
            rp->error = 0;
        }
    LOM_HIP(m, hipMemcpyAsync(m->batch.dev.p, m->batch.stage.h, dev_bytes, hipMemcpyHostToDevice, m->stream));
    for (size_t ri = 0; ri < rounds.size(); ri++) {
        const AlignRound &R = rounds[ri];
        uint32_t mb_max = 0;
        for (int k = 0; k < R.size; k++) mb_max = std::max(mb_max, mb[order[R.first + k]]);
        const BatchProblem *desc = d_desc + R.first;
        const unsigned long long seq0 = m->batch.report_seq;
        auto launch_pair = [&](int i) -> int {
            const double t_l = now_s();
            if (mb_max) {
                const bool prev = i > 0 && R.temporal;  // (the first search of a scan: no previous records)
                launch_k_match_batch(m, prev, R.counted, dim3(mb_max, R.size), desc);
                LOM_HIP(m, hipGetLastError());
            }
            m->batch.lm_seq += 8;  // a solve spends at most 5 evaluations
            launch_k_lm_batch(m, R.shape, dim3(R.nb, R.size), m->batch.lm_seq, seq0 + (unsigned long long)i + 1, i == 0,
                              i == R.give_up_outer, desc);
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
                volatile AlignReport *rp = reinterpret_cast<volatile AlignReport *>((char *)m->batch.reports.h + (size_t)j * 256);
                const int w = wait_report(m, rp, want, "batched device solve");
                if (w < 0) {
                    m->batch.report_seq = want;
                    return w;
                }
                if (w == kReportError) {  // its later launches see the flag in its AlignState and return at once
                    gave_up[i] = 1;
                    out[i].round = (int32_t)ri;
                    any_gave_up = true;
                    done[k] = 1;
                } else if (rp->finished) {
                    result_from_report(rp, R.counted, prob[i].nb, out[i]);
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
        m->batch.report_seq = seq0 + (unsigned long long)launched;
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
    m->error.clear();
    double launch_s = 0.0, wait_s = 0.0;
    // the handles involved, runner first, each once
    std::vector<lom_map *> maps{m};
    for (int i = 0; i < count; i++)
        if (std::find(maps.begin(), maps.end(), it[i].map) == maps.end()) maps.push_back(it[i].map);
    auto problem_error = [&](int i, int rc) {
        lom_map *pm = it[i].map;
        if (pm == m) return rc;
        const std::string why = "problem " + std::to_string(i) + ": " + pm->error;
        return fail(m, rc, why.c_str());
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
        std::vector<HostCloud> clouds((size_t)count);
        std::vector<const char *> d_src((size_t)count);
        for (int i = 0; i < count; i++) clouds[i] = HostCloud{it[i].src, it[i].n, it[i].stride};
        const double t_l = now_s();
        if ((rc = upload_distinct(m, m->batch.src, clouds.data(), count, d_src.data())) != LOM_OK) return rc;
        for (int i = 0; i < count; i++) it[i].src = d_src[i];
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
        pm->error.clear();
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

}  // extern "C"
