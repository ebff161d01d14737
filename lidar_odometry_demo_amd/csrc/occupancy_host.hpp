// Host planning of the occupancy grid (occupancy_host.cpp), shared with occupancy.hip.  Plain C++: nothing here needs a
// device.  The scan descriptors and their checks are the assembly's (assemble_host.hpp); what is added is the value
// ranges of the geometry, the ray parameters and the rule, the step bound of the walk, the slice size the scratch budget
// admits, and the bounding boxes of a call's slices.  The origins' start cells and their range verdict
// (assemble::origin_cell) and the cut into launches are shared with the elevation grid and live there too.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "assemble_host.hpp"

namespace lom {
namespace occupancy {

constexpr uint32_t kSliceScans = 64;               // scans of one launch at most
constexpr uint32_t kMaxSide = 16384;               // cells per axis
constexpr size_t kScratchBudget = size_t(256) << 20;  // bytes of pass + hit bitmaps a handle may own
constexpr uint32_t kWindowMax = 512;               // side of the walk's LDS window in cells: 512 x 512 bits = 32 KB

inline uint32_t words_per_row(uint32_t width) { return (width + 31u) / 32u; }
// u32 words of one bitmap (a scan of a slice has two: pass and hit)
inline size_t map_words(const lom_occupancy_geometry &g) { return (size_t)g.height * words_per_row(g.width); }

// cells [x0, x1) x [y0, y1) of the grid; empty when x0 >= x1 or y0 >= y1
struct Box {
    uint32_t x0, y0, x1, y1;
    bool empty() const { return x0 >= x1 || y0 >= y1; }
};

// scans [first, first + count) of the call: one launch of k_occ_walk over the descriptors desc + first, one k_occ_fold
struct Slice : assemble::Launch {
    Box box;  // every cell a bit of the slice can fall into: origins +- max_range, clipped to the grid
};

struct Plan {
    assemble::Plan scans;        // descriptors in call order (out / blk are the assembly's and not read here)
    std::vector<int32_t> cells;  // start cell (x, y) per scan, call order
    std::vector<Slice> slices;   // in call order; a slice of empty scans only is not listed
};

bool geometry_ok(const lom_occupancy_geometry *g);
// z_lo < 0 < z_hi, margin >= 0, 0 < min_range < max_range, all finite, max_range / resolution <= 2^20
bool params_ok(const lom_occupancy_ray_params *p, float resolution);
bool rule_ok(const lom_occupancy_rule *r);
// 2 * (ceil(max_range / r) + 2): a guard, the walk ends by itself before
uint32_t max_steps(float max_range, float resolution);
// min(64, what kScratchBudget admits, at least 1), then capped by test_slice_max (0: no cap)
uint32_t slice_scans(const lom_occupancy_geometry &g, uint32_t test_slice_max);
// the cells within max_range of an origin at start cell c, two cells of slack, clipped to the grid
Box box_of(const int32_t c[2], float max_range, const lom_occupancy_geometry &g);
Box box_union(const Box &a, const Box &b);

// Ids and poses are checked as lom_map_assemble checks them (assemble::plan), then the parameters (LOM_ERR_ARG), then
// every origin's range (LOM_ERR_RANGE); the slices hold at most slice_scans(g, test_slice_max) scans.
int plan(const assemble::ScanEntry *table, size_t n_scans, const int64_t *ids, const lom_graph_pose *poses, size_t count,
         const lom_occupancy_geometry &g, const lom_occupancy_ray_params *p, uint32_t test_slice_max, Plan &out,
         std::string &why);

}  // namespace occupancy
}  // namespace lom
