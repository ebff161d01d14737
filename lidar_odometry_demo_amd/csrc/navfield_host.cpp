// Host planning of lom_navfield_*: value ranges, the cell-cost table, the quantisation of goals and starts, tile counts,
// the tiles of a re-solve's window, the plan of a shift with a re-solve and launch shapes.  Plain C++, no HIP:
// navfield.hip calls these, and tests/cpp/test_navfield.cpp and tests/cpp/test_navfield_shift.cpp compile this file alone.
#include "navfield_host.hpp"

#include <algorithm>
#include <cmath>

namespace lom {
namespace navfield {

bool params_ok(const lom_navfield_params *p)
{
    if (!p || p->neutral < 1u || p->max_passable < 0 || p->max_passable > (int8_t)kMaxByteCost || (p->flags & ~kKnownFlags) != 0u)
        return false;
    // (64-bit: 98 * factor cannot wrap)
    if ((uint64_t)p->neutral + (uint64_t)kMaxByteCost * p->factor > (uint64_t)kMaxCellCost) return false;
    if ((p->flags & LOM_NAV_UNKNOWN_PASSABLE) && (p->unknown_cost < 1u || p->unknown_cost > kMaxCellCost)) return false;
    return true;
}

void cell_costs(const lom_navfield_params &p, uint32_t out[256])
{
    for (uint32_t b = 0; b < 256u; b++) out[b] = 0u;
    for (uint32_t v = 0; v <= (uint32_t)p.max_passable; v++) out[v] = p.neutral + p.factor * v;
    if (p.flags & LOM_NAV_UNKNOWN_PASSABLE) out[255] = p.unknown_cost;  // the byte -1
}

bool cell_of_metres(const lom_occupancy_geometry &g, float x, float y, int32_t *ix, int32_t *iy)
{
    const double r = (double)g.resolution;
    const double qx = std::floor(((double)x - (double)g.origin_x) / r), qy = std::floor(((double)y - (double)g.origin_y) / r);
    // (a NaN fails every comparison)
    if (qx >= 0.0 && qx < (double)g.width && qy >= 0.0 && qy < (double)g.height) {
        *ix = (int32_t)qx, *iy = (int32_t)qy;
        return true;
    }
    *ix = *iy = -1;
    return false;
}

bool quantise(const lom_occupancy_geometry &g, int kind, const void *points, size_t n, int32_t *out)
{
    if (kind == LOM_NAV_CELLS) {
        const int32_t *c = static_cast<const int32_t *>(points);
        for (size_t i = 0; i < 2 * n; i++) out[i] = c[i];
        return true;
    }
    if (kind == LOM_NAV_METRES) {
        const float *m = static_cast<const float *>(points);
        for (size_t i = 0; i < n; i++) (void)cell_of_metres(g, m[2 * i], m[2 * i + 1], out + 2 * i, out + 2 * i + 1);
        return true;
    }
    return false;
}

TileGrid tile_grid(uint32_t width, uint32_t height)
{
    TileGrid t;
    t.tiles_x = (width + kTile - 1u) / kTile, t.tiles_y = (height + kTile - 1u) / kTile;
    t.n_tiles = t.tiles_x * t.tiles_y;  // at most 256 * 256
    return t;
}

TileRange tile_range(const clearance::Rect &window)
{
    if (window.empty()) return TileRange{0u, 0u, 0u, 0u};
    const uint32_t tx0 = window.x0 / kTile, ty0 = window.y0 / kTile;
    return TileRange{tx0, ty0, (window.x1 - 1u) / kTile - tx0 + 1u, (window.y1 - 1u) / kTile - ty0 + 1u};
}

uint32_t blocks_for(size_t n) { return n ? (uint32_t)((n + kThreads - 1u) / kThreads) : 1u; }

bool waypoint_params_ok(const lom_navfield_waypoint_params *p, size_t n_starts)
{
    if (!p || p->flags != 0u || p->lookahead < 1u || p->lookahead > kMaxLookahead || p->route_cap < 1u) return false;
    return (size_t)p->route_cap <= kMaxPathCells && n_starts <= kMaxPathCells / p->route_cap;
}

bool waypoint_output_ok(size_t n_starts, size_t wp_cap, const void *cells_out)
{
    if (wp_cap > kMaxPathCells || (wp_cap && n_starts > kMaxPathCells / wp_cap)) return false;
    return !(n_starts && wp_cap && !cells_out);
}

uint32_t shortcut_blocks_for(size_t n_routes) { return n_routes ? (uint32_t)((n_routes + kRoutesPerGroup - 1u) / kRoutesPerGroup) : 1u; }

ShiftPlan shift_plan(uint32_t width, uint32_t height, int32_t dx, int32_t dy)
{
    ShiftPlan p{};
    const int64_t w = width, h = height;
    const int64_t cx = dx > w ? w : dx < -w ? -w : dx, cy = dy > h ? h : dy < -h ? -h : dy;
    p.dx = (int32_t)cx, p.dy = (int32_t)cy;
    // destination columns with a source: 0 <= ix + dx < width
    const int64_t x0 = cx < 0 ? -cx : 0, x1 = cx > 0 ? w - cx : w, y0 = cy < 0 ? -cy : 0, y1 = cy > 0 ? h - cy : h;
    if (x0 < x1 && y0 < y1) p.kept = clearance::Rect{(uint32_t)x0, (uint32_t)y0, (uint32_t)x1, (uint32_t)y1};
    p.cells_kept = p.kept.cells();
    p.cells_entered = (uint64_t)width * height - p.cells_kept;
    if (p.kept.empty()) {
        p.entered[p.n_entered++] = clearance::Rect{0u, 0u, width, height};
        return p;
    }
    // (one of the two strips per axis is empty: the kept box touches the side the content moved towards)
    if (p.kept.y0 > 0u) p.entered[p.n_entered++] = clearance::Rect{0u, 0u, width, p.kept.y0};
    if (p.kept.y1 < height) p.entered[p.n_entered++] = clearance::Rect{0u, p.kept.y1, width, height};
    if (p.kept.x0 > 0u) p.entered[p.n_entered++] = clearance::Rect{0u, p.kept.y0, p.kept.x0, p.kept.y1};
    if (p.kept.x1 < width) p.entered[p.n_entered++] = clearance::Rect{p.kept.x1, p.kept.y0, width, p.kept.y1};
    // the trailing borders: the side the content moved towards, where what lay beyond has left the grid
    if (p.dx != 0) {
        const uint32_t col = p.dx > 0 ? 0u : width - 1u;
        p.trailing[p.n_trailing++] = tile_range(clearance::Rect{col, p.kept.y0, col + 1u, p.kept.y1});
        p.trailing_cells += p.kept.y1 - p.kept.y0;
    }
    if (p.dy != 0) {
        const uint32_t row = p.dy > 0 ? 0u : height - 1u;
        p.trailing[p.n_trailing++] = tile_range(clearance::Rect{p.kept.x0, row, p.kept.x1, row + 1u});
        p.trailing_cells += p.kept.x1 - p.kept.x0 - (p.dx != 0 ? 1u : 0u);  // (the corner cell is in the column already)
    }
    return p;
}

void shift_upload_rows(const ShiftPlan &plan, const clearance::Rect &window, uint32_t height, uint32_t *y0, uint32_t *y1)
{
    uint32_t lo = height, hi = 0u;
    for (uint32_t i = 0; i < plan.n_entered; i++) lo = std::min(lo, plan.entered[i].y0), hi = std::max(hi, plan.entered[i].y1);
    if (!window.empty()) lo = std::min(lo, window.y0), hi = std::max(hi, window.y1);
    if (lo >= hi) lo = hi = 0u;
    *y0 = lo, *y1 = hi;
}

uint64_t launch_bound(uint32_t width, uint32_t height) { return 2ull * width * height + 64ull; }

}  // namespace navfield
}  // namespace lom
