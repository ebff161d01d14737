// What the matcher's host files -- align.hip, align_batch.hip, quality_report.hip -- may call and fill: the records and
// descriptors host and kernels exchange, the typed launchers of match.hip (one per kernel form: each takes what that
// form reads and fills the parameters it does not read itself) and the pieces of the chained align that the single and
// the batched align share.  The launch geometry and everything planned from sizes alone -- grids, k_lm shapes, the
// rounds of the batched calls, block offsets -- is match_plan.hpp's, plain C++ that includes no HIP header; this header
// includes it and keeps what needs a handle or a device type.  No kernel is visible from here: a kernel of the matcher
// is named -- instantiated, launched, queried -- in match.hip alone, and this header includes no k_*.hpp (they include
// it).
#pragma once
#include <algorithm>
#include <ctime>

#include "lom_internal.hpp"
#include "match_plan.hpp"

namespace lom {

// ---- of the handle and the chain (the launch geometry: match_plan.hpp) ---------------------------------------------------
constexpr int kPairsAhead = 5;  // (k_match, k_lm) pairs enqueued before the host looks at a report
// the partition a launch of this handle is sized for: its own stream's, none on a caller's stream
static inline uint32_t launch_partition(const lom_map *m) { return m->stream == m->own_stream ? m->partition_cus : 0u; }

// ---- what host and kernels exchange ------------------------------------------------------------------------------------
// what k_match leaves behind for the evaluations of one outer iteration: source point,
// winner's stored point and normal, 48 bytes = three dwordx4 (coalesced for k_eval)
// (the winner's point and the valid flag share one dwordx4: the next outer iteration's k_match reads exactly that
// quarter back as its temporal pruning bound)
struct __attribute__((aligned(16))) MatchRec {
    float px, py, pz, nx;     // source_point_local (voxel_grid.h:226), plane_normal.x
    float ox, oy, oz, valid;  // plane_origin; valid: 0.0f = no match, else the bits kRecValid | the winner's row in the slabs
                              // (never zero, never a denormal: consumers test `!= 0.f`; the next search of the same scan
                              // reads the row back: a query whose winner has not changed leaves its record alone)
    float ny, nz, pad0, pad1;
};
static_assert(sizeof(MatchRec) == kMatchRecBytes, "three dwordx4");
struct QStat;  // k_match.hpp: the per-query debug record of lom_match_find_pairs

// Batched align (lom_match_align_batch / _multi): one problem of a round, read by the batch forms of k_match and k_lm
// from a small array in HBM (blockIdx.y = the problem's place in the round).  Everything that belongs to one problem --
// the keyframe it searches, its scan, records, search counters, solve state, exchange set and report -- hangs off its
// descriptor.
struct BatchProblem {
    MapView map;  // read by k_match only (k_lm sees the records)
    const char *src;
    size_t stride;
    MatchRec *rec;
    uint32_t *block_counters;
    AlignState *state;
    AlignReport *report;  // device view of pinned host memory
    void *xrec;           // this round slot's exchange sets (XWord)
    uint32_t n, match_blocks;
    uint32_t lm_blocks;  // the solve's grid (k_lm workgroups)
    float guess_t[3], guess_q[4];
    float max_sq;
    double prior_b[3];
};

struct LmInit {
    float t[3], q[4];   // initial guess (cloud_matcher.cpp:107), used when `first`
    double prior_b[3];  // NormalPrior anchor = the guess's translation (:153)
    float max_sq;       // max_correspondence_distance^2 of the searches (:139, voxel_grid.h:215)
};

// one problem of a round of the batched quality report (k_quality.hpp)
struct QualBatchProblem {
    const MatchRec *rec;  // the records its search left
    double *part;         // `grid` workgroup records of kQualSums doubles
    double *out;          // its kQualSums totals
    uint32_t n, grid;
    EvalArgs E;
};
static_assert(LOM_NQSUMS * sizeof(double) == kQualPartBytes, "a workgroup record of k_quality");

// ---- scans, poses ------------------------------------------------------------------------------------------------------
// (what a scan's arguments must satisfy: match_plan.hpp)
static inline float sq_f32(float max_dist) { return max_dist * max_dist; }  // voxel_grid.h:215
static inline double now_s()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
void pose_args(const float t[3], const float q[4], float max_sq, PoseArgs &P);

// The initial guess of an align as the kernels take it: the first pose (cloud_matcher.cpp:107), the searches'
// max_correspondence_distance 0.3 squared in f32 (:139, voxel_grid.h:215) and the NormalPrior's anchor, the guess's
// translation (:153).
static inline void guess_fields(const float gt[3], const float gq[4], float (&t)[3], float (&q)[4], double (&prior_b)[3],
                                float &max_sq)
{
    for (int a = 0; a < 3; a++) t[a] = gt[a];
    for (int a = 0; a < 4; a++) q[a] = gq[a];
    for (int a = 0; a < 3; a++) prior_b[a] = (double)gt[a];
    max_sq = sq_f32(0.3f);
}

// The search half of a batch problem -- the batch form of k_match reads nothing else -- and the AlignState block its pose
// comes from: both cleared (finished = error = 0: the search runs), then map, scan, outputs and the pose (t, q, max_sq).
void fill_search(BatchProblem &d, AlignState &state, const MapView &map, const char *src, size_t stride, uint32_t n,
                 uint32_t match_blocks, MatchRec *rec, uint32_t *block_counters, AlignState *d_state, const float t[3],
                 const float q[4], float max_sq);

// ---- the single search and the host-driven evaluation (match.hip) --------------------------------------------------------
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
int scan_buffers(lom_map *m, uint32_t n, bool want_stats);
// chained: the pose comes from the AlignState in HBM (t, q unused)
// count_mode: -1 = as the handle says (LOM_OPT_COUNT_CANDIDATES), 0 / 1 = without / with the reference-algorithm counts
int launch_match(ScanCtx &c, const float t[3], const float q[4], float max_sq, bool stats, bool chained = false,
                 int count_mode = -1);
void server_stop(lom_map *m);  // tell a resident evaluation server to leave (it exits within one poll of the command word)
int eval_kernel_attrs(lom_map *m);
// the hooks of the host-driven loop (lom_align_with_hooks) over one scan: a search plus an evaluation, an evaluation
lom_align_hooks eval_hooks(ScanCtx &c);

// ---- k_lm's shapes (LmShape, kLmGeometry: match_plan.hpp) ------------------------------------------------------------------
// hipOccupancyMaxActiveBlocksPerMultiprocessor of the shape's single or batch instantiation
int lm_blocks_per_cu(lom_map *m, LmShape shape, bool batch, int *per_cu);

// ---- typed launchers (match.hip) ------------------------------------------------------------------------------------------
// All enqueue on `m->stream` and leave the error check (hipGetLastError) to the caller, as the launches they replace did.
// single k_match: `state` != nullptr is the chained form (the pose comes from it, P is not read)
void launch_k_match(lom_map *m, bool prev, bool count, uint32_t blocks, const char *d_src, size_t stride, uint32_t n,
                    const PoseArgs &P, int32_t *out_idx, MatchRec *out_rec, QStat *out_stat, uint32_t *block_counters,
                    const AlignState *state = nullptr);
// batch k_match (always chained): grid = (largest search grid, problems)
void launch_k_match_batch(lom_map *m, bool prev, bool count, dim3 grid, const BatchProblem *desc);
// single k_lm on the handle's own records, state, counters, exchange sets and report; advances nothing on the handle
void launch_k_lm(lom_map *m, LmShape shape, uint32_t blocks, uint32_t n, const LmInit &init, bool first_outer,
                 uint32_t match_blocks, unsigned long long report_seq, unsigned long long fold_report_seq,
                 unsigned long long *dbg_stamps, int p2p_set_base, unsigned long long p2p_epoch, double *dbg_trace,
                 bool give_up);
// batch k_lm: grid = (largest solve grid, problems); no exchange between ranks, no debug outputs
void launch_k_lm_batch(lom_map *m, LmShape shape, dim3 grid, unsigned long long seq_base, unsigned long long report_seq,
                       bool first_outer, bool give_up, const BatchProblem *desc);
// k_quality over `n` records into `part`, then k_quality_sum of its `blocks` workgroup records into `out`
void launch_k_quality(lom_map *m, uint32_t blocks, const MatchRec *rec, uint32_t n, const EvalArgs &E, double *part,
                      float *residual_out, double *out);
// k_quality_batch on (largest evaluation grid, problems), then k_quality_batch_sum, one wave per problem
void launch_k_quality_batch(lom_map *m, uint32_t blocks, uint32_t problems, const QualBatchProblem *desc);

// ---- the chain of an align (align.hip; the batched align runs the same) ----------------------------------------------------
// Returned by align_chained when a workgroup of k_lm gave up waiting for the others (they are not all
// resident: a caller sharing the GPU, a CU mask) or for a peer rank: the caller redoes the align
// through the host-driven loop.
constexpr int kDeviceLoopGaveUp = 100;
int device_cus(lom_map *m, uint32_t *out);  // compute units a launch of this handle reaches: its partition's where it has one
int lm_grid(lom_map *m, uint32_t n, LmShape shape, uint32_t *nb);  // lm_blocks under the handle's occupancy query
constexpr int kReportArrived = 0, kReportError = 1;
int wait_report(lom_map *m, const volatile AlignReport *rp, unsigned long long want, const char *solve);
void result_from_report(const volatile AlignReport *rp, bool counted, uint32_t nb, lom_align_result &r);
int align_device_paths(lom_map *m, const char *d_src, size_t n, size_t stride, const float guess_t[3],
                       const float guess_q[4], float out_t[3], float out_q[4], lom_align_stats *stats);

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

}  // namespace lom
