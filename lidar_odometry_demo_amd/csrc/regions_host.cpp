// Host planning of lom_regions_*: value ranges, the shapes of the launches, the centroid rounding and the list sort.
// Plain C++, no HIP: regions.hip calls these, and tests/cpp/test_regions.cpp compiles this file alone.
#include "regions_host.hpp"

#include <algorithm>
#include <cmath>

namespace lom {
namespace regions {

static_assert(sizeof(lom_regions_record) == 48 && sizeof(lom_regions_params) == 20 && sizeof(lom_regions_summary) == 40,
              "the layouts the header documents");

bool params_ok(const lom_regions_params *p, bool have_potential)
{
    if (!p || (p->kind != LOM_REGIONS_BYTES && p->kind != LOM_REGIONS_FRONTIER)) return false;
    if (p->kind == LOM_REGIONS_BYTES && p->lo > p->hi) return false;
    if (p->max_cost < 0 || p->max_cost > kMaxCostByte || p->min_cells < 1u || (p->flags & ~kKnownFlags) != 0u) return false;
    if (p->rank != LOM_REGIONS_RANK_LABEL && p->rank != LOM_REGIONS_RANK_CELLS && p->rank != LOM_REGIONS_RANK_POTENTIAL) return false;
    return p->rank != LOM_REGIONS_RANK_POTENTIAL || have_potential;
}

bool tile_rows_ok(int64_t rows) { return rows == 1 || rows == 8 || rows == 32; }

Plan plan(uint32_t width, uint32_t height, uint32_t tile_rows, bool no_tiles)
{
    Plan p;
    p.words_per_row = (width + 63u) / 64u;
    p.words = p.words_per_row * height;  // at most 128 * 8192
    p.row_blocks = (p.words_per_row * 64u + kThreads - 1u) / kThreads;
    p.bands = (height + kBandRows - 1u) / kBandRows;
    p.tile_cols = no_tiles ? 1u : kTileCols, p.tile_rows = no_tiles ? 1u : tile_rows;
    p.tiles_x = (width + p.tile_cols - 1u) / p.tile_cols, p.tiles_y = (height + p.tile_rows - 1u) / p.tile_rows;
    p.n_tiles = no_tiles ? 0u : p.tiles_x * p.tiles_y;
    p.row_lanes = (uint64_t)(p.tiles_y - 1u) * width, p.col_lanes = (uint64_t)(p.tiles_x - 1u) * height;
    p.scan_blocks = (p.words + kScanWords - 1u) / kScanWords;
    return p;
}

uint32_t blocks_for(uint64_t n) { return n ? (uint32_t)((n + kThreads - 1u) / kThreads) : 1u; }

uint32_t record_cap(uint64_t max_regions, uint32_t width, uint32_t height)
{
    const uint64_t most = ((uint64_t)width * height + 1u) / 2u;
    return (uint32_t)std::min(std::min(max_regions, kMaxRegionsMax), most);
}

uint32_t centroid(uint64_t sum, uint32_t cells) { return (uint32_t)((2u * sum + cells) / (2u * (uint64_t)cells)); }

bool sort_list(const lom_regions_record *records, size_t n, uint32_t min_cells, int rank, std::vector<uint32_t> &order)
{
    order.clear();
    if (rank != LOM_REGIONS_RANK_LABEL && rank != LOM_REGIONS_RANK_CELLS && rank != LOM_REGIONS_RANK_POTENTIAL) return false;
    for (size_t i = 0; i < n; i++)
        if (records[i].cells >= min_cells) order.push_back((uint32_t)i);
    // (the records come in ascending label order, and labels differ: the order is total)
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const lom_regions_record &ra = records[a], &rb = records[b];
        if (rank == LOM_REGIONS_RANK_CELLS && ra.cells != rb.cells) return ra.cells > rb.cells;
        if (rank == LOM_REGIONS_RANK_POTENTIAL && ra.entry_potential != rb.entry_potential) return ra.entry_potential < rb.entry_potential;
        return ra.label < rb.label;
    });
    return true;
}

}  // namespace regions
}  // namespace lom
