// Host planning of the pose field (posefield_host.cpp), shared with posefield.hip.  Plain C++: nothing here needs a device
// or a HIP header.  The value ranges of the parameters, the footprint and the counts, the stencils, the tile counts, the
// launch shapes and the weight bound.  Definitions: include/lidar_odometry_amd.h ("pose field").
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/lidar_odometry_amd.h"
#include "pose_rule.hpp"

namespace lom {
namespace posefield {

constexpr uint32_t kTileX = 32, kTileY = 8;        // a tile of k_pose_relax: 32 x 8 cells, all eight headings
constexpr uint32_t kThreads = 256;                 // every kernel runs workgroups of four waves
constexpr uint32_t kMaxCost = (1u << 24) - 1;      // of turn_cost, spin_cost, reverse_cost (and of a cell)
constexpr uint32_t kMaxWeight = 7u * kMaxCost + kMaxCost;  // of a move: below 2^28
constexpr uint32_t kKnownFlags = LOM_POSE_SPIN | LOM_POSE_REVERSE;
constexpr uint32_t kMaxSamples = 1024;             // F, the rollouts' limit
constexpr int32_t kSampleMax = 16384;              // |fx|, |fy|, the rollouts' limit
constexpr uint32_t kMaxStencil = kMaxSamples;      // cells of a stencil: at most one per sample
constexpr int32_t kMaxReach = 91;                  // |dx|, |dy| of a stencil cell: 64 * sqrt 2, rounded
constexpr uint32_t kReportGroups = 64;             // workgroups of k_pose_report, at most
constexpr size_t kMaxPoints = (size_t)1 << 24;     // goals of a solve, starts of a paths call
constexpr size_t kMaxPathStates = (size_t)1 << 28; // K * cap of a paths call
constexpr size_t kMaxQueries = (size_t)1 << 30;

static_assert(kMaxWeight < (1u << 28), "a move's weight stays below 2^28");
static_assert(kPoseFlagSpin == LOM_POSE_SPIN && kPoseFlagReverse == LOM_POSE_REVERSE && kPoseHeadings == LOM_POSE_HEADINGS,
              "the header and pose_rule.hpp disagree");

// nav by the navigation field's rule; turn_cost, spin_cost, reverse_cost <= 2^24 - 1; spin_cost >= 1 under LOM_POSE_SPIN;
// known flags only
bool params_ok(const lom_posefield_params *p);
inline PoseCosts costs_of(const lom_posefield_params &p) { return PoseCosts{p.turn_cost, p.spin_cost, p.reverse_cost, p.flags}; }
// 1 <= F <= 1024 samples with |fx|, |fy| <= 16384
bool footprint_ok(const int32_t *footprint, size_t f);
// The eight stencils of a footprint that is ok: per heading the distinct cell offsets, sorted by (dy, dx), as int16
// (dx, dy) pairs -- heading h at cells[2 * first[h] ...], first[8] the total.
struct Stencils {
    std::vector<int16_t> cells;
    uint32_t first[kPoseHeadings + 1];
    uint32_t count(uint32_t h) const { return first[h + 1] - first[h]; }
};
Stencils stencils(const int32_t *footprint, size_t f);
// A re-solve's k_pose_relayer: per heading the box of the cells (x, y) with (x + dx, y + dy) inside `changed` for some cell
// (dx, dy) of that heading's stencil -- the bounding box of `changed` dilated by the mirrored stencil -- clipped to the grid
// (empty where nothing of it is inside), and `all`, the box that holds the eight (empty where all are).  `changed` is
// clipped to the grid first; an empty one gives empty boxes.
PoseBoxes relayer_boxes(const Stencils &st, const PoseBox &changed, uint32_t width, uint32_t height);

// k_pose_relax: a workgroup per tile, tiles_x x tiles_y of them; the last column and row may be cut
struct TileGrid {
    uint32_t tiles_x, tiles_y, n_tiles;
};
TileGrid tile_grid(uint32_t width, uint32_t height);
// workgroups of kThreads lanes for n lanes (at least one)
uint32_t blocks_for(size_t n);
// workgroups of k_pose_report for n cells: blocks_for(n), at most kReportGroups
uint32_t report_groups(size_t n_cells);
// the refusals of a paths call: K <= 2^24, K * cap <= 2^28, a buffer where there are states to write
bool paths_ok(const void *starts, size_t n_starts, const void *states_out, size_t cap);

}  // namespace posefield
}  // namespace lom
