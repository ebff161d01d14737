// Host planning of the trajectory rollouts (rollout_host.cpp), shared with rollout.hip.  Plain C++: nothing here needs a
// device or a HIP header.  The value ranges of the parameters, the states, the commands and the footprint, the footprint's
// reach, the window of the cost plane a workgroup may stage, the shapes of the launches, the score and its key, and the
// three host-only helpers.  Definitions: include/lidar_odometry_amd.h ("trajectory rollouts").
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/lidar_odometry_amd.h"
#include "plane_geometry.hpp"

namespace lom {
namespace rollout {

constexpr uint32_t kWaveLanes = 64;
constexpr uint32_t kWavesDefault = 4;        // waves of a workgroup of k_rollout_eval: 1 or 4 (LOM_ROLLOUT_OPT_TEST_WAVES)
constexpr uint32_t kThreads = 256;           // every other kernel runs workgroups of four waves
// A wave of k_rollout_eval takes these one after another.  Measured at 32, 8, 4, 2 and 1 (profiles/rollout_candidates_per_wave.json):
// each halving won, 1 by 9 % over 2 on the total -- a workgroup's 32 KiB copy of the table costs less than the waves a CU
// goes without when K / (4 * this) workgroups do not fill it several times over.
constexpr uint32_t kCandidatesPerWave = 1;
constexpr uint32_t kSegmentsMax = 8, kStepsPerSegmentMax = 128, kStepsMax = 1024;
constexpr int32_t kLethalMinLo = 1, kLethalMinHi = 100, kUnknownCostLo = -1, kUnknownCostHi = 98;
constexpr uint32_t kProgressWeightMax = 256, kCostWeightMax = 4096, kTruncationWeightMax = 1u << 20;
constexpr uint32_t kKnownFlags = LOM_ROLLOUT_KEEP_RECORDS;
constexpr size_t kMaxStates = 4096, kMaxCandidates = (size_t)1 << 20, kMaxRecords = (size_t)1 << 22;
constexpr size_t kMaxSamples = 1024;
constexpr int32_t kSampleMax = 16384;            // |fx|, |fy|, in 1/256 cell
constexpr int32_t kPositionLo = -(1 << 29), kPositionHi = (1 << 29) - 1;
constexpr uint32_t kAngles = 65536;
// the key of a pick: (s + 2^41) << 20 | (2^20 - 1 - k)
constexpr uint32_t kKeyIndexBits = 20;
constexpr uint64_t kKeyIndexMask = (1ull << kKeyIndexBits) - 1u;
constexpr int64_t kKeyBias = (int64_t)1 << 41;
// The window of the cost plane a workgroup stages in LDS: side 2 (S + reach) + 1 cells of a byte around the state's cell.
// The budget keeps a workgroup's dynamic LDS -- the reduction's 128 bytes, 32 KiB of table, up to 8 KiB of footprint and the
// window -- within the 64 KiB a launch may ask for without a per-kernel attribute, which also leaves two workgroups on a
// CU's 160 KiB: staging never halves the waves that hide the loads it does not remove.  S + reach <= 76.
constexpr uint32_t kWindowBudgetBytes = 23u << 10;
constexpr uint32_t kTableBytes = 8u * LOM_ROLLOUT_TABLE;  // (C, S) int32 pairs
constexpr uint32_t kLdsLimitBytes = 64u << 10;
static_assert(128u + kTableBytes + 8u * 1024u + ((kWindowBudgetBytes + 15u) & ~15u) <= kLdsLimitBytes, "the evaluation's dynamic LDS fits a plain launch");

// The shapes of an evaluation's launches.
struct Plan {
    uint32_t steps;            // S
    uint32_t reach;            // cells a sample lies from its pose's cell at most
    uint32_t window_side;      // 2 (S + reach) + 1, or 0: the plane is read in HBM
    uint32_t eval_threads;     // 64 * waves (the serial form: kThreads)
    uint32_t block_candidates; // candidates of a workgroup
    uint32_t blocks_x;         // workgroups per state (0: nothing to launch); blocks_y is M
    uint32_t lds_bytes;        // dynamic LDS of the evaluation
    uint32_t fill_blocks, summary_blocks;  // workgroups of kThreads lanes over the states
};

using plane::geometry_ok;  // the rule of the planning grids
bool params_ok(const lom_rollout_params *p);
bool waves_ok(int64_t waves);  // 1, 4
// m <= 4096, k <= 2^20, m * k <= 2^22, 1 <= f <= 1024
bool counts_ok(size_t m, size_t k, size_t f);
bool states_ok(const lom_rollout_state *states, size_t m);
bool footprint_ok(const int32_t *footprint, size_t f);
// max over the samples of ceil((|fx| + |fy|) / 256) + 1: a sample's cell differs from its pose's by at most this per axis
uint32_t reach(const int32_t *footprint, size_t f);
// the table of step 1's units: exactly visibility::table(4096); out: 2 * 4096 int32
void table(int32_t *out);
Plan plan(const lom_rollout_params &p, uint32_t reach_cells, size_t m, size_t k, size_t f, uint32_t waves, bool serial, bool no_lds_plane);
uint32_t blocks_for(uint64_t n);  // workgroups of kThreads lanes for n lanes (at least one)
// Step 4.  progress_weight * (P0 - end) is within 2^8 * 2^32, cost_weight * cost_sum within 2^12 * 1025 * 99 < 2^29 and
// the truncation term within 2^20 * 1025 < 2^31, so |s| < 2^41 and 1 <= s + 2^41 < 2^42: the key stays below 2^62 and is
// never 0.
int64_t score(const lom_rollout_params &p, bool have_potential, uint32_t p0, const lom_rollout_record &r);
bool admissible(const lom_rollout_params &p, bool have_potential, uint32_t p0, const lom_rollout_record &r);
uint64_t key_of(int64_t s, uint32_t k);
uint32_t key_index(uint64_t key);
int64_t key_score(uint64_t key);
// the helpers of the public header; true: done
bool footprint_rectangle(int32_t front, int32_t back, int32_t half_width, int32_t spacing, bool perimeter_only, int32_t *out, size_t cap,
                         size_t *count);
bool state_from_pose(const lom_occupancy_geometry *g, float x_m, float y_m, float yaw, lom_rollout_state *out);
bool poses(const lom_rollout_params *p, const lom_rollout_state *state, const int16_t *commands, lom_rollout_state *out);

}  // namespace rollout
}  // namespace lom
