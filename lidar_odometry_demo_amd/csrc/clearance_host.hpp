// Host planning of the clearance grid (clearance_host.cpp), shared with clearance.hip.  Plain C++: nothing here needs a
// device or a HIP header.  The value ranges of the geometry and the parameters, the radius in cells and the cost table,
// the clipped and the grown rectangle of an update, and the launch shapes of its two kernels.  Definitions:
// include/lidar_odometry_amd.h ("clearance grid").
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/lidar_odometry_amd.h"
#include "plane_geometry.hpp"

namespace lom {
namespace clearance {

constexpr uint32_t kMaxRadius = 254;       // R in cells: R^2 = 64516 fits a u16 below LOM_CLEAR_FAR
constexpr uint32_t kTileCols = 64;         // a tile of k_clear_distance is one bitmap word wide ...
constexpr uint32_t kTileRowsMax = 32;      // ... and T rows high, T in 1 .. 32
constexpr uint32_t kWavesPerBlock = 4;     // both kernels run workgroups of four waves
constexpr uint32_t kKnownFlags = LOM_CLEAR_FREE_CLEARS_ELEVATION | LOM_CLEAR_UNKNOWN_IS_OBSTACLE;

inline uint32_t words_per_row(uint32_t width) { return (width + 63u) / 64u; }  // u64 words of a bitmap row

// cells [x0, x1) x [y0, y1) of the grid; empty when x0 >= x1 or y0 >= y1
struct Rect {
    uint32_t x0, y0, x1, y1;
    bool empty() const { return x0 >= x1 || y0 >= y1; }
    uint64_t cells() const { return empty() ? 0u : (uint64_t)(x1 - x0) * (y1 - y0); }
};

// k_clear_merge: a wave per bitmap word of the grown rectangle -- words [wx0, wx0 + n_wx) of rows [y0, y0 + n_rows)
struct MergeGrid {
    uint32_t wx0, n_wx, y0, n_rows;
    uint32_t blocks;  // of kWavesPerBlock waves
};

// k_clear_distance: a workgroup per tile -- word columns [wx0, wx0 + n_wx), tile rows y0 + t * tile_rows, t < n_ty, the
// last tile cut at the rectangle's y1; lds_bytes: 64 x (tile_rows + 2R)
struct TileGrid {
    uint32_t wx0, n_wx, y0, n_ty, tile_rows;
    size_t lds_bytes;
};

using plane::geometry_ok;  // the rule of all four planning grids
// floor((double)inflation_radius / (double)resolution); > kMaxRadius (also for a quotient that is no number): out of range
uint32_t radius_cells(float inflation_radius, float resolution);
// 0 <= inscribed_radius <= inflation_radius, decay >= 0, all finite, known flags only, radius_cells <= 254
bool params_ok(const lom_clearance_params *p, float resolution);
// R^2 + 1 bytes: the header's step 3, in f64
void cost_table(const lom_clearance_params &p, float resolution, uint32_t R, uint8_t *out);
// the window clipped to the grid (NULL: the whole grid)
Rect clip(const lom_clearance_window *w, const lom_occupancy_geometry &g);
// r grown by R cells on every side, clipped to the grid (an empty r stays empty)
Rect grow(const Rect &r, uint32_t R, const lom_occupancy_geometry &g);
MergeGrid merge_grid(const Rect &grown);
// tile_rows: 1 .. kTileRowsMax
TileGrid tile_grid(const Rect &r, uint32_t R, uint32_t tile_rows);

}  // namespace clearance
}  // namespace lom
