// Launch planning of the matcher (match_plan.cpp), shared with match.hip, align.hip, align_batch.hip and
// quality_report.hip through match_launch.hpp.  Plain C++: nothing here needs a device, a handle or a HIP header.  The
// launch geometry of k_match, k_eval and k_lm, the grids and k_lm shapes that follow from a scan's size, the rounds of the
// batched align and of the batched quality report, and where a problem's blocks lie in a round's buffers.  What needs a
// handle -- the occupancy queries and their caches, the buffers, the launches -- stays with the callers;
// tests/cpp/test_match_plan.cpp compiles match_plan.cpp alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lom {

// ---- launch geometry ------------------------------------------------------------------------------------------------
constexpr int kMatchThreads = 256;             // 4 waves
constexpr int kMatchG = 16;                    // lanes per query: four queries per wave
constexpr int kMatchRows = 4;                  // consecutive rows of a voxel per chunk: one search and 48 bytes per lane and trip
constexpr int kMatchMinWaves = 7;              // waves per SIMD the register budget is held to (72 VGPRs)
constexpr int kEvalThreads = 512;
constexpr int kRecWords = 32;    // doubles per record
constexpr uint32_t kMaxLmBlocks = 64;    // workgroups of k_lm (one lane of a wave watches each record)
constexpr uint32_t kMaxLmBlocksBig = 128;  // ... of its variant for large clouds; also the size of an exchange set
// a solve's pair of exchange sets (k_lm.hpp: 16-byte XWords)
constexpr size_t kExchangeSetBytes = (size_t)2 * kMaxLmBlocksBig * kRecWords * 16;

constexpr uint32_t kMaxMatchBlocks = 256u * (uint32_t)kMatchMinWaves;  // one resident round: kMatchMinWaves workgroups of 4 waves per CU
constexpr uint32_t kMaxEvalBlocks = 64;  // records per launch (the host polls this many words)
uint32_t match_grid(uint32_t n, uint32_t partition_cus = 0);  // (a context on a partition of the GPU: one resident round of ITS compute units)
uint32_t eval_grid(uint32_t n);

// sizes the planners lay out (match_launch.hpp asserts them beside the types)
constexpr size_t kMatchRecBytes = 48;       // sizeof(MatchRec): what k_match leaves per point
constexpr size_t kMatchCounterBytes = 16;   // k_match's counters of one workgroup
constexpr size_t kQualPartBytes = 36 * 8;   // a workgroup record of k_quality: LOM_NQSUMS doubles

// ---- scans ------------------------------------------------------------------------------------------------------------
// a scan as the entry points take it: a stride that holds three floats and keeps them aligned, a count k_match's 32-bit
// indices cover
constexpr size_t kMaxScanPoints = 0x7FFFFFFFull;
static inline bool stride_ok(size_t stride) { return stride >= 12 && !(stride & 3); }
static inline bool scan_args_ok(size_t n, size_t stride) { return stride_ok(stride) && n < kMaxScanPoints; }
static inline size_t round_up256(size_t b) { return (b + 255) & ~size_t(255); }

// Blocks one behind the other in a buffer, each at a multiple of 256 bytes: take(size) says where the next one lies.
struct BlockLayout {
    size_t next = 0;  // where the next block begins: the buffer's size with its last block rounded up
    size_t end = 0;   // where the last block ends: the bytes in use
    size_t take(size_t size)
    {
        const size_t off = next;
        end = off + size;
        next = off + round_up256(size);
        return off;
    }
};

// ---- k_lm's shapes ------------------------------------------------------------------------------------------------------
// The 256-thread shapes launch one wave more, the policy wave (k_lm): nb and the point assignment count the 256 threads.
constexpr uint32_t kLmSmallThreads = 256;
constexpr uint32_t kLmSmallLaunch = kLmSmallThreads + 64;  // the point threads and the policy wave (lm_threads)
enum LmShape { kLmSmall = 0, kLmMid = 1, kLmBig = 2, kLmSmall2 = 3 };
struct LmGeometry {
    uint32_t points;   // point threads of a workgroup
    uint32_t threads;  // threads of a launch
    uint32_t cap;      // most workgroups of a solve
};
constexpr LmGeometry kLmGeometry[4] = {
    /* kLmSmall  */ {kLmSmallThreads, kLmSmallLaunch, kMaxLmBlocks},
    /* kLmMid    */ {(uint32_t)kEvalThreads, (uint32_t)kEvalThreads, kMaxLmBlocks},
    /* kLmBig    */ {(uint32_t)kEvalThreads, (uint32_t)kEvalThreads, kMaxLmBlocksBig},
    /* kLmSmall2 */ {kLmSmallThreads, kLmSmallLaunch, kMaxLmBlocks},
};
LmShape lm_shape(uint32_t n);
// the grid of a solve: one point per point thread up to the shape's cap, and no more than `resident_limit`, the
// workgroups of the shape that are resident at once (>= 1: align.hip's occupancy query)
uint32_t lm_blocks(uint32_t n, LmShape shape, uint32_t resident_limit);

// ---- the rounds of the batched align (align_batch.hip) ------------------------------------------------------------------
struct AlignPlanProblem {
    uint32_t n;
    uint32_t nb;  // its solve grid: lm_blocks of its n on the handle (>= 1)
    bool counted, temporal;  // k_match's template parameters, from the problem's map
    int give_up_outer;       // the give-up test it carries (-1: none)
};
struct AlignRound {
    int first, size;  // range of `order`
    LmShape shape;
    uint32_t nb;  // the largest solve grid of its problems: the launch's x dimension
    bool counted, temporal;
    int give_up_outer;  // of its problem 0
};
struct AlignPlan {
    std::vector<int> order;  // the problems round by round
    std::vector<AlignRound> rounds;
};
// Groups by (lm_shape of n, counted, temporal) in order of first appearance, a group's problems in call order, each
// group cut into rounds.  k_lm's workgroups wait for each other, so a round's whole grid must be resident at once:
// problems per round = max(1, floor(cus x per_cu[shape] / the GROUP's largest nb)) -- a round's launch is sized for its own
// largest grid, residency is counted with the group's -- and no more than round_max where that is > 0.  A problem that
// carries a give-up test opens a round: the kernel applies the test to problem 0 of a launch.
// per_cu: workgroups of the batch form of k_lm per compute unit, by shape (read for the shapes that occur).
void plan_align_rounds(const AlignPlanProblem *p, int count, uint32_t cus, const uint32_t per_cu[4], int round_max,
                       AlignPlan &out);

// ---- the rounds of the batched quality report (quality_report.hip) --------------------------------------------------------
// 64 MiB: a quarter of the 256 MiB last-level cache, so what a round's search writes is still on the chip when its
// evaluation reads it; 47 problems of a 28,800-point scan or 708 of a 1,900-point one -- several times the workgroups
// the device has compute units for -- so that more per round would buy nothing.
constexpr size_t kQualBatchBudgetBytes = (size_t)64 << 20;
constexpr int kQualBatchRoundCap = 32768;  // problems per round at most (blockIdx.y)
struct QualRound {
    int first, size;
    uint32_t mb, nb;  // the launches' x extent: the largest search / evaluation grid of its problems
};
struct QualPlanProblem {
    uint32_t mb, nb;                    // match_grid / eval_grid of its n
    size_t off_rec, off_cnt, off_part;  // its records, k_match counters and workgroup records in its round's buffers
};
struct QualPlan {
    std::vector<QualRound> rounds;
    std::vector<QualPlanProblem> problems;
    size_t rec_bytes = 0, cnt_bytes = 0, part_bytes = 0;  // the three buffers: the largest round's extents
};
// Problems go to rounds in the caller's order.  A round's records, counters and workgroup records, each block rounded up
// to 256 bytes, fit kQualBatchBudgetBytes (a problem larger than that runs alone), and it holds at most
// min(round_max where that is > 0, kQualBatchRoundCap) problems; the round buffers are reused by the next round.
void plan_quality_rounds(const uint32_t *n, int count, uint32_t partition_cus, int round_max, QualPlan &out);

}  // namespace lom
