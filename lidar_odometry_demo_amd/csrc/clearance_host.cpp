// Host planning of lom_clearance_*: value ranges, the radius in cells, the cost table, the rectangles of an update and the
// launch shapes of k_clear_merge and k_clear_distance.  Plain C++, no HIP: clearance.hip calls these, and
// tests/cpp/test_clearance.cpp compiles this file alone.
#include "clearance_host.hpp"

#include <algorithm>
#include <cmath>

namespace lom {
namespace clearance {

uint32_t radius_cells(float inflation_radius, float resolution)
{
    const double q = std::floor((double)inflation_radius / (double)resolution);
    return q >= 0.0 && q <= (double)kMaxRadius ? (uint32_t)q : kMaxRadius + 1u;
}

bool params_ok(const lom_clearance_params *p, float resolution)
{
    return p && std::isfinite(p->inflation_radius) && std::isfinite(p->inscribed_radius) && std::isfinite(p->decay) &&
           p->inscribed_radius >= 0.f && p->inscribed_radius <= p->inflation_radius && p->decay >= 0.f &&
           (p->flags & ~kKnownFlags) == 0u && radius_cells(p->inflation_radius, resolution) <= kMaxRadius;
}

void cost_table(const lom_clearance_params &p, float resolution, uint32_t R, uint8_t *out)
{
    const double r = (double)resolution, inscribed = (double)p.inscribed_radius, inflation = (double)p.inflation_radius;
    const double decay = (double)p.decay;
    for (uint32_t k = 0; k <= R * R; k++) {
        const double dist = std::sqrt((double)k) * r;
        if (k == 0u)
            out[k] = 100;
        else if (dist <= inscribed)
            out[k] = 99;
        else if (dist > inflation)
            out[k] = 0;
        else
            out[k] = (uint8_t)std::floor(98.0 * std::exp(-decay * (dist - inscribed)));
    }
}

Rect clip(const lom_clearance_window *w, const lom_occupancy_geometry &g)
{
    if (!w) return Rect{0u, 0u, g.width, g.height};
    // (64-bit: x0 + width cannot wrap)
    const int64_t x0 = std::max<int64_t>(w->x0, 0), y0 = std::max<int64_t>(w->y0, 0);
    const int64_t x1 = std::min<int64_t>((int64_t)w->x0 + (int64_t)w->width, g.width);
    const int64_t y1 = std::min<int64_t>((int64_t)w->y0 + (int64_t)w->height, g.height);
    if (x0 >= x1 || y0 >= y1) return Rect{0u, 0u, 0u, 0u};
    return Rect{(uint32_t)x0, (uint32_t)y0, (uint32_t)x1, (uint32_t)y1};
}

Rect grow(const Rect &r, uint32_t R, const lom_occupancy_geometry &g)
{
    if (r.empty()) return r;
    return Rect{r.x0 > R ? r.x0 - R : 0u, r.y0 > R ? r.y0 - R : 0u, std::min(r.x1 + R, g.width), std::min(r.y1 + R, g.height)};
}

MergeGrid merge_grid(const Rect &grown)
{
    MergeGrid m{0u, 0u, 0u, 0u, 0u};
    if (grown.empty()) return m;
    m.wx0 = grown.x0 / 64u, m.n_wx = (grown.x1 + 63u) / 64u - m.wx0;
    m.y0 = grown.y0, m.n_rows = grown.y1 - grown.y0;
    m.blocks = (m.n_wx * m.n_rows + kWavesPerBlock - 1u) / kWavesPerBlock;  // at most 128 * 8192 waves
    return m;
}

TileGrid tile_grid(const Rect &r, uint32_t R, uint32_t tile_rows)
{
    TileGrid t{0u, 0u, 0u, 0u, tile_rows, 0u};
    if (r.empty()) return t;
    t.wx0 = r.x0 / kTileCols, t.n_wx = (r.x1 + kTileCols - 1u) / kTileCols - t.wx0;
    t.y0 = r.y0, t.n_ty = (r.y1 - r.y0 + tile_rows - 1u) / tile_rows;
    t.lds_bytes = (size_t)kTileCols * (tile_rows + 2u * R);
    return t;
}

}  // namespace clearance
}  // namespace lom
