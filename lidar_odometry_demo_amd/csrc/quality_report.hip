// The align quality report and its batched form (lom_match_quality* / lom_match_quality_batch*): buffers, rounds,
// descriptors and entry points.  Host code only: the kernels are launched through match.hip's typed launchers
// (match_launch.hpp); the host math is quality.cpp's.
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

using namespace lom;

extern "C" {

// ---------------------------------------------------------------------------
// Quality report (lom_match_quality* / lom_scan_quality*): one search at the f32 pose as given, k_quality at that pose
// widened to f64, k_quality_sum into pinned host memory, ONE wait; the host math is lom_quality_from_sums (quality.cpp).
// Isolation as the batched align: buffers of its own (lom_map::qual), nothing of the single align's state, of an armed
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
    m->error.clear();
    int rc = resolve_pending(m);  // an insert nobody has looked at since: the search must see its points
    if (rc != LOM_OK) return rc;
    const uint32_t nn = (uint32_t)n;
    const uint32_t mb = match_grid(nn, launch_partition(m)), nb = eval_grid(nn);
    if ((rc = ensure(m, m->qual.idx, n * 4)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qual.rec, n * sizeof(MatchRec))) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qual.cnt, (size_t)kMaxMatchBlocks * 16)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qual.part, (size_t)kMaxEvalBlocks * LOM_NQSUMS * 8)) != LOM_OK) return rc;
    if ((rc = ensure_pinned(m, m->qual.sums, LOM_NQSUMS * 8, LOM_NQSUMS * 8, hipHostMallocMapped | hipHostMallocCoherent,
                            "hipHostMalloc(quality sums)")) != LOM_OK)
        return rc;
    const char *d_src = (const char *)src;
    float *d_res = residual_out;
    if (!device_input) {
        if ((rc = upload_scan(m, m->qual.src, src, n, stride, &d_src)) != LOM_OK) return rc;
        if (residual_out) {
            if ((rc = ensure(m, m->qual.res, n * 4)) != LOM_OK) return rc;
            d_res = m->qual.res.as<float>();
        }
    }
    PoseArgs P;
    pose_args(t, q, sq_f32(max_dist), P);
    EvalArgs E;
    for (int a = 0; a < 4; a++) E.q[a] = (double)q[a];
    for (int a = 0; a < 3; a++) E.t[a] = (double)t[a];
    launch_k_match(m, false, m->opt_count, mb, d_src, stride, nn, P, m->qual.idx.as<int32_t>(), m->qual.rec.as<MatchRec>(), nullptr,
                   m->qual.cnt.as<uint32_t>());
    launch_k_quality(m, nb, m->qual.rec.as<const MatchRec>(), nn, E, m->qual.part.as<double>(), d_res, (double *)m->qual.sums.d);
    LOM_HIP(m, hipGetLastError());
    if (!device_input && residual_out)
        LOM_HIP(m, hipMemcpyAsync(residual_out, d_res, n * 4, hipMemcpyDeviceToHost, m->stream));
    LOM_HIP(m, hipStreamSynchronize(m->stream));
    double sums[LOM_NQSUMS];
    std::memcpy(sums, m->qual.sums.h, sizeof sums);
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
//   The cut and the offsets are plan_quality_rounds' (match_plan.cpp: plain C++, tested on the CPU; the budget's
//   reasons and figures are with kQualBatchBudgetBytes in match_plan.hpp).
// Clouds.  The host entries upload every distinct (pointer, n, stride) once, before the first round.
// Isolation.  lom_map::qualb: nothing of the single align, the single report, an armed cleanup scan or idle hook, or the
//   map-maintenance scratch is read or written; neither call_seq nor mutations move.
// ---------------------------------------------------------------------------
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
    m->error.clear();
    int rc = resolve_pending(m);  // an insert nobody has looked at since: the search must see its points
    if (rc != LOM_OK) return rc;
    const int L = (int)live.size();
    const uint32_t part_cus = launch_partition(m);
    // host clouds: every distinct (pointer, n, stride) once
    std::vector<const char *> d_src(L);
    if (device_input) {
        for (int j = 0; j < L; j++) d_src[j] = (const char *)p[live[j]].xyz;
    } else {
        std::vector<HostCloud> clouds(L);
        for (int j = 0; j < L; j++) clouds[j] = HostCloud{p[live[j]].xyz, p[live[j]].n, p[live[j]].stride_bytes};
        if ((rc = upload_distinct(m, m->qualb.src, clouds.data(), L, d_src.data())) != LOM_OK) return rc;
    }
    // rounds, and where a problem's records, counters and workgroup records lie in its round's buffers
    std::vector<uint32_t> n_live(L);
    for (int j = 0; j < L; j++) n_live[j] = (uint32_t)p[live[j]].n;
    QualPlan plan;
    plan_quality_rounds(n_live.data(), L, part_cus, m->qualb.test_round_max, plan);
    // per problem: the pose block the search reads, the search's descriptor, the evaluation's descriptor
    BlockLayout dev;
    dev.take((size_t)L * sizeof(AlignState));
    const size_t off_match = dev.take((size_t)L * sizeof(BatchProblem)), off_eval = dev.take((size_t)L * sizeof(QualBatchProblem));
    const size_t dev_bytes = dev.next;
    const size_t sums_bytes = (size_t)L * LOM_NQSUMS * 8;
    if ((rc = ensure(m, m->qualb.rec, plan.rec_bytes)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qualb.cnt, plan.cnt_bytes)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qualb.part, plan.part_bytes)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qualb.dev, dev_bytes)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->qualb.sums, sums_bytes)) != LOM_OK) return rc;
    // (the uploads above do not read it)
    if ((rc = ensure_pinned(m, m->qualb.stage, dev_bytes + sums_bytes, std::max(dev_bytes + sums_bytes, (size_t)65536),
                            hipHostMallocDefault, "hipHostMalloc(quality batch staging)")) != LOM_OK)
        return rc;
    AlignState *h_states = reinterpret_cast<AlignState *>(m->qualb.stage.h);
    BatchProblem *h_match = reinterpret_cast<BatchProblem *>((char *)m->qualb.stage.h + off_match);
    QualBatchProblem *h_eval = reinterpret_cast<QualBatchProblem *>((char *)m->qualb.stage.h + off_eval);
    double *h_sums = reinterpret_cast<double *>((char *)m->qualb.stage.h + dev_bytes);
    AlignState *d_states = reinterpret_cast<AlignState *>(m->qualb.dev.p);
    const BatchProblem *d_match = reinterpret_cast<const BatchProblem *>(m->qualb.dev.as<char>() + off_match);
    const QualBatchProblem *d_eval = reinterpret_cast<const QualBatchProblem *>(m->qualb.dev.as<char>() + off_eval);
    const MapView view = view_of(m);
    const float max_sq = sq_f32(max_dist);
    for (int j = 0; j < L; j++) {
        const lom_quality_problem &q = p[live[j]];
        const QualPlanProblem &at = plan.problems[j];
        BatchProblem &d = h_match[j];
        fill_search(d, h_states[j], view, d_src[j], q.stride_bytes, (uint32_t)q.n, at.mb,
                    reinterpret_cast<MatchRec *>(m->qualb.rec.as<char>() + at.off_rec),
                    reinterpret_cast<uint32_t *>(m->qualb.cnt.as<char>() + at.off_cnt), d_states + j, q.t, q.q_wxyz, max_sq);
        QualBatchProblem &e = h_eval[j];
        std::memset(&e, 0, sizeof e);
        e.rec = d.rec;
        e.part = reinterpret_cast<double *>(m->qualb.part.as<char>() + at.off_part);
        e.out = m->qualb.sums.as<double>() + (size_t)j * LOM_NQSUMS;
        e.n = d.n;
        e.grid = at.nb;
        for (int a = 0; a < 4; a++) e.E.q[a] = (double)q.q_wxyz[a];
        for (int a = 0; a < 3; a++) e.E.t[a] = (double)q.t[a];
    }
    LOM_HIP(m, hipMemcpyAsync(m->qualb.dev.p, m->qualb.stage.h, dev_bytes, hipMemcpyHostToDevice, m->stream));
    for (const QualRound &R : plan.rounds) {
        launch_k_match_batch(m, false, m->opt_count, dim3(R.mb, R.size), d_match + R.first);
        launch_k_quality_batch(m, R.nb, (uint32_t)R.size, d_eval + R.first);
        LOM_HIP(m, hipGetLastError());
    }
    LOM_HIP(m, hipMemcpyAsync(h_sums, m->qualb.sums.p, sums_bytes, hipMemcpyDeviceToHost, m->stream));
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

}  // extern "C"
