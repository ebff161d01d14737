// Host planning of the navigation field (navfield_host.cpp), shared with navfield.hip.  Plain C++: nothing here needs a
// device or a HIP header.  The value ranges of the geometry and the parameters, the cell-cost table, the quantisation of
// goals and starts, the tile counts, the tiles of a re-solve's window, the plan of a shift with a re-solve and the launch
// shapes.  Definitions: include/lidar_odometry_amd.h ("navigation field").
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/lidar_odometry_amd.h"
#include "clearance_host.hpp"  // Rect: a window clipped to the grid
#include "plane_geometry.hpp"

namespace lom {
namespace navfield {

constexpr uint32_t kTile = 32;                     // a tile of k_nav_relax is 32 x 32 cells
constexpr uint32_t kThreads = 256;                 // every kernel runs workgroups of four waves
constexpr uint32_t kMaxCellCost = (1u << 24) - 1;  // of a passable cell: 7 * kMaxCellCost < 2^27 fits a u32 with room
constexpr uint32_t kMaxByteCost = 98;              // the largest cost byte that may be passable
constexpr uint32_t kKnownFlags = LOM_NAV_UNKNOWN_PASSABLE;
constexpr uint32_t kInnerCapDefault = 64;          // sweeps of a tile per launch
constexpr uint32_t kInnerCapMax = 1u << 20;
constexpr uint32_t kBatchDefault = 16;             // launches per wait
constexpr uint32_t kBatchMax = 256;
constexpr size_t kMaxPoints = (size_t)1 << 24;     // goals of a solve, starts of a paths call
constexpr size_t kMaxPathCells = (size_t)1 << 28;  // K * cap of a paths call

// k_nav_relax: a workgroup per tile, tiles_x x tiles_y of them; the last column and row may be cut
struct TileGrid {
    uint32_t tiles_x, tiles_y, n_tiles;
};

using plane::geometry_ok;  // the rule of all four planning grids
// neutral >= 1, 0 <= max_passable <= 98, neutral + 98 * factor <= 2^24 - 1, known flags only, and unknown_cost in
// 1 .. 2^24 - 1 where LOM_NAV_UNKNOWN_PASSABLE is set
bool params_ok(const lom_navfield_params *p);
// the header's step 1: the cost of a cell per cost byte (index: the byte read as unsigned), 0 = impassable
void cell_costs(const lom_navfield_params &p, uint32_t out[256]);
// a cost byte outside -1 .. 100
inline bool byte_invalid(int8_t b) { return b < -1 || b > 100; }
// The cell of a point in metres by the floor rule (f64 from the f32 values, compared before any conversion).  false: the
// point is outside the grid or not a number, and *ix = *iy = -1.
bool cell_of_metres(const lom_occupancy_geometry &g, float x, float y, int32_t *ix, int32_t *iy);
// n goals or starts of either kind as int32 (ix, iy) pairs for the device: cells are passed on as they are (the device
// refuses those outside the grid), metres go through cell_of_metres.  false: an unknown kind.
bool quantise(const lom_occupancy_geometry &g, int kind, const void *points, size_t n, int32_t *out);
TileGrid tile_grid(uint32_t width, uint32_t height);
// k_nav_diff: a workgroup per tile that holds a cell of the clipped window -- tiles [tx0, tx0 + n_tx) x [ty0, ty0 + n_ty);
// none for an empty window
struct TileRange {
    uint32_t tx0, ty0, n_tx, n_ty;
};
TileRange tile_range(const clearance::Rect &window);
// workgroups of kThreads lanes for n lanes (at least one)
uint32_t blocks_for(size_t n);
// Steps 8 and 9.  The parameters of lom_navfield_waypoints for n_starts starts: lookahead in 1 .. 65535, route_cap >= 1,
// n_starts * route_cap <= 2^28, flags 0.
constexpr uint32_t kMaxLookahead = 65535;
constexpr size_t kMaxVisiblePairs = (size_t)1 << 24;  // of a lom_navfield_visible call
constexpr uint32_t kRoutesPerGroup = 4;                // k_nav_shortcut: a wave per route
bool waypoint_params_ok(const lom_navfield_waypoint_params *p, size_t n_starts);
// ... and its output: n_starts * wp_cap <= 2^28 cells, which need a buffer where there are any
bool waypoint_output_ok(size_t n_starts, size_t wp_cap, const void *cells_out);
// workgroups of k_nav_shortcut for n routes (at least one)
uint32_t shortcut_blocks_for(size_t n_routes);
// ---- the shift with a re-solve ("Shift and re-solve") ---------------------------------------------------
// Everything of lom_navfield_shift_resolve* that needs no device, for a grid of width x height cells moved by (dx, dy).
//  - dx, dy: the shift clamped to |dx| <= width, |dy| <= height (a larger one keeps nothing, as these do), so that every
//    index of the device pass fits 32 bits.
//  - kept: the destination cells (ix, iy) whose source (ix + dx, iy + dy) lies in the grid, a box; {0, 0, 0, 0} where nothing
//    is kept.  cells_kept + cells_entered = width * height.
//  - entered[0 .. n_entered): the other cells as at most two disjoint rectangles: the whole rows outside the kept box's
//    rows, then the columns outside its columns within its rows.
//  - trailing[0 .. n_trailing): the tiles that hold a kept cell on a trailing border -- column 0 for dx > 0, column
//    width - 1 for dx < 0, row 0 for dy > 0, row height - 1 for dy < 0 -- as at most two tile ranges (a column of tiles, a
//    row of tiles; they may share a corner tile); trailing_cells counts those cells, a corner cell once.
struct ShiftPlan {
    int32_t dx, dy;
    clearance::Rect kept;
    clearance::Rect entered[2];
    uint32_t n_entered;
    uint64_t cells_kept, cells_entered;
    TileRange trailing[2];
    uint32_t n_trailing;
    uint64_t trailing_cells;
    bool moves() const { return dx != 0 || dy != 0; }
};
ShiftPlan shift_plan(uint32_t width, uint32_t height, int32_t dx, int32_t dy);
// The rows [*y0, *y1) of a host plane that lom_navfield_shift_resolve uploads, whole: every row that holds an entered cell
// or a cell of the clipped window (one run of rows: what lies between two such rows goes along).  Empty (*y0 == *y1 == 0)
// where there is neither.
void shift_upload_rows(const ShiftPlan &plan, const clearance::Rect &window, uint32_t height, uint32_t *y0, uint32_t *y1);

// More launches than any solve needs: a cell whose best route has d steps is final one launch after the next cell of
// that route is, so d + 1 launches settle it, and d is below the number of cells.  2 * cells + 64.
uint64_t launch_bound(uint32_t width, uint32_t height);

}  // namespace navfield
}  // namespace lom
