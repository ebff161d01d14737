// Host planning of the region grid (regions_host.cpp), shared with regions.hip.  Plain C++: nothing here needs a device
// or a HIP header.  The value ranges of the geometry, the parameters and the options, the word, tile and lane counts of
// the launches, the centroid rounding and the list sort.  Definitions: include/lidar_odometry_amd.h ("frontier
// regions").
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/lidar_odometry_amd.h"
#include "plane_geometry.hpp"

namespace lom {
namespace regions {

constexpr uint32_t kThreads = 256;            // every kernel runs workgroups of four waves
constexpr uint32_t kTileCols = 64;            // a tile of k_reg_label_tile: one bitmap word wide ...
constexpr uint32_t kTileRowsMax = 32;         // ... and 1, 8 or 32 rows high
constexpr uint32_t kTileRowsDefault = 8;     // the faster of 8 and 32 at 4096 x 4096 (profiles/regions_cost.json)
constexpr uint32_t kBandRows = 16;            // rows a wave of k_reg_accumulate and k_reg_centre walks down
constexpr uint32_t kScanWords = 1024;         // bitmap words per workgroup of k_reg_scan_partial
constexpr uint32_t kMaxRegionsDefault = 1u << 20;
constexpr uint64_t kMaxRegionsMax = 1ull << 26;
constexpr uint32_t kKnownFlags = LOM_REGIONS_NEIGHBOURS_8 | LOM_REGIONS_EDGE_UNKNOWN | LOM_REGIONS_CONNECT_4;
constexpr int8_t kMaxCostByte = 99;
constexpr size_t kMaxQueryPoints = (size_t)1 << 30;

// The shapes of an extract's launches.  The bitmaps are row-aligned: words_per_row u64 per row, bit ix & 63 of word
// ix >> 6.  The merge's tiles are 64 x tile_rows cells, or single cells without the tile pass.
struct Plan {
    uint32_t words_per_row, words;      // of a bitmap; words <= 2^20
    uint32_t row_blocks;                // workgroups along x of a launch with a lane per cell of a row (y is blockIdx.y)
    uint32_t bands;                     // ... and along y where a wave walks down kBandRows rows
    uint32_t tile_cols, tile_rows;      // of the merge: 64 x rows, or 1 x 1
    uint32_t tiles_x, tiles_y, n_tiles; // workgroups of k_reg_label_tile (n_tiles = 0: no tile pass)
    uint64_t row_lanes, col_lanes;      // lanes of k_reg_merge on the tile borders between rows, between columns
    uint32_t scan_blocks;               // workgroups of k_reg_scan_partial, <= 1024
};

using plane::geometry_ok;  // the rule of all four planning grids
// a known kind; lo <= hi under LOM_REGIONS_BYTES; 0 <= max_cost <= 99; min_cells >= 1; a known rank, the potential's
// only with a potential; known flags only
bool params_ok(const lom_regions_params *p, bool have_potential);
bool tile_rows_ok(int64_t rows);  // 1, 8, 32
Plan plan(uint32_t width, uint32_t height, uint32_t tile_rows, bool no_tiles);
// workgroups of kThreads lanes for n lanes (at least one)
uint32_t blocks_for(uint64_t n);
// The records an extract can fill: min(max_regions, the most regions a grid of this size can hold).  Components under
// either connectivity hold at least one cell each and no two of them touch at an edge, so ceil(cells / 2) bounds them.
uint32_t record_cap(uint64_t max_regions, uint32_t width, uint32_t height);
// floor((2 sum + cells) / (2 cells)): the mean, rounded to nearest, a half upwards.  cells >= 1.
uint32_t centroid(uint64_t sum, uint32_t cells);
// Step 5: the indices of the records with cells >= min_cells, in list order.  false: an unknown rank.
bool sort_list(const lom_regions_record *records, size_t n, uint32_t min_cells, int rank, std::vector<uint32_t> &order);

}  // namespace regions
}  // namespace lom
