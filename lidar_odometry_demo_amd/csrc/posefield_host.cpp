// Host planning of lom_posefield_*: value ranges, the stencils of a footprint, tile counts and launch shapes, and the two
// host-only entry points.  Plain C++, no HIP: posefield.hip calls these, and tests/cpp/test_posefield.cpp compiles this
// file with navfield_host.cpp (the parameter rule of the cell costs) and visibility_host.cpp (the table's one home) alone.
#include "posefield_host.hpp"

#include <algorithm>
#include <utility>

#include "navfield_host.hpp"
#include "visibility_host.hpp"

namespace lom {
namespace posefield {

static_assert(sizeof(lom_posefield_params) == 36 && sizeof(lom_posefield_summary) == 72 && sizeof(lom_posefield_solve_stats) == 24 &&
                  sizeof(lom_posefield_resolve_counters) == 56,
              "the layouts the header documents");
static_assert(kMaxCost == navfield::kMaxCellCost, "a layer value is a cell cost");

bool params_ok(const lom_posefield_params *p)
{
    if (!p || !navfield::params_ok(&p->nav) || (p->flags & ~kKnownFlags) != 0u) return false;
    if (p->turn_cost > kMaxCost || p->spin_cost > kMaxCost || p->reverse_cost > kMaxCost) return false;
    return !(p->flags & LOM_POSE_SPIN) || p->spin_cost >= 1u;
}

bool footprint_ok(const int32_t *footprint, size_t f)
{
    if (!footprint || f < 1u || f > kMaxSamples) return false;
    for (size_t i = 0; i < 2 * f; i++)
        if (footprint[i] < -kSampleMax || footprint[i] > kSampleMax) return false;
    return true;
}

Stencils stencils(const int32_t *footprint, size_t f)
{
    static const std::vector<int32_t> tab = [] {
        std::vector<int32_t> t(2 * 4096);
        (void)visibility::table(4096, t.data());
        return t;
    }();
    Stencils st;
    st.first[0] = 0u;
    std::vector<std::pair<int32_t, int32_t>> cells;  // (dy, dx): the sort order
    for (uint32_t h = 0; h < kPoseHeadings; h++) {
        const int32_t c = tab[2 * 512 * h], s = tab[2 * 512 * h + 1];
        cells.clear();
        for (size_t i = 0; i < f; i++) {
            int32_t dx, dy;
            pose_sample_cell(footprint[2 * i], footprint[2 * i + 1], c, s, &dx, &dy);
            cells.emplace_back(dy, dx);
        }
        std::sort(cells.begin(), cells.end());
        cells.erase(std::unique(cells.begin(), cells.end()), cells.end());
        for (const auto &cell : cells) st.cells.push_back((int16_t)cell.second), st.cells.push_back((int16_t)cell.first);
        st.first[h + 1] = st.first[h] + (uint32_t)cells.size();
    }
    return st;
}

PoseBoxes relayer_boxes(const Stencils &st, const PoseBox &changed, uint32_t width, uint32_t height)
{
    PoseBoxes b{};
    const int64_t cx0 = changed.x0, cy0 = changed.y0, cx1 = std::min(changed.x1, width), cy1 = std::min(changed.y1, height);
    if (cx0 >= cx1 || cy0 >= cy1) return b;
    int64_t ax0 = width, ay0 = height, ax1 = 0, ay1 = 0;
    for (uint32_t h = 0; h < kPoseHeadings; h++) {
        if (!st.count(h)) continue;
        int64_t lo_x = INT32_MAX, hi_x = INT32_MIN, lo_y = INT32_MAX, hi_y = INT32_MIN;  // the extents of the stencil
        for (uint32_t k = st.first[h]; k < st.first[h + 1]; k++) {
            const int64_t dx = st.cells[2 * (size_t)k], dy = st.cells[2 * (size_t)k + 1];
            lo_x = std::min(lo_x, dx), hi_x = std::max(hi_x, dx), lo_y = std::min(lo_y, dy), hi_y = std::max(hi_y, dy);
        }
        // x + dx in [cx0, cx1) for some dx in [lo_x, hi_x]: x in [cx0 - hi_x, cx1 - lo_x)
        const int64_t x0 = std::max<int64_t>(0, cx0 - hi_x), x1 = std::min<int64_t>(width, cx1 - lo_x);
        const int64_t y0 = std::max<int64_t>(0, cy0 - hi_y), y1 = std::min<int64_t>(height, cy1 - lo_y);
        if (x0 >= x1 || y0 >= y1) continue;
        b.of[h] = PoseBox{(uint32_t)x0, (uint32_t)y0, (uint32_t)x1, (uint32_t)y1};
        ax0 = std::min(ax0, x0), ay0 = std::min(ay0, y0), ax1 = std::max(ax1, x1), ay1 = std::max(ay1, y1);
    }
    if (ax0 < ax1 && ay0 < ay1) b.all = PoseBox{(uint32_t)ax0, (uint32_t)ay0, (uint32_t)ax1, (uint32_t)ay1};
    return b;
}

TileGrid tile_grid(uint32_t width, uint32_t height)
{
    TileGrid t;
    t.tiles_x = (width + kTileX - 1u) / kTileX, t.tiles_y = (height + kTileY - 1u) / kTileY;
    t.n_tiles = t.tiles_x * t.tiles_y;  // at most 256 * 1024
    return t;
}

uint32_t blocks_for(size_t n) { return n ? (uint32_t)((n + kThreads - 1u) / kThreads) : 1u; }

uint32_t report_groups(size_t n_cells) { return std::min(blocks_for(n_cells), kReportGroups); }

bool paths_ok(const void *starts, size_t n_starts, const void *states_out, size_t cap)
{
    if ((n_starts && !starts) || n_starts > kMaxPoints) return false;
    if (cap > kMaxPathStates || (cap && n_starts > kMaxPathStates / cap)) return false;
    return !(n_starts && cap && !states_out);
}

}  // namespace posefield
}  // namespace lom

extern "C" {

int lom_posefield_stencils(const int32_t *footprint, size_t n_samples, int32_t *cells_out, size_t cap, uint32_t *counts_out)
{
    using namespace lom;
    if (!counts_out || (cap && !cells_out) || !posefield::footprint_ok(footprint, n_samples)) return LOM_ERR_ARG;
    const posefield::Stencils st = posefield::stencils(footprint, n_samples);
    for (uint32_t h = 0; h < kPoseHeadings; h++) counts_out[h] = st.count(h);
    const size_t n = std::min(cap, (size_t)st.first[kPoseHeadings]);
    for (size_t i = 0; i < 2 * n; i++) cells_out[i] = st.cells[i];
    return LOM_OK;
}

uint32_t lom_posefield_heading_of_angle(uint32_t angle) { return lom::pose_heading_of_angle(angle); }

}  // extern "C"
