// The line-of-sight rule of the navigation field, written once for the host and the device (include/lidar_odometry_amd.h,
// "navigation field", steps 8 and 9): whether a cell is clear, the exact integer walk of a segment between two cells with
// the field's no-corner-cut rule, and the greedy choice of the next waypoint tested one candidate after another.
// lom_navfield_visible, both forms of k_nav_shortcut (k_navfield_waypoints.hpp) and tests/cpp/test_navfield_waypoints.cpp
// call these, as rollout_rule.hpp is shared by the rollout's two homes.  Integers throughout; no HIP header.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define LOM_NAV_LOS_HD __host__ __device__ inline
#else
#define LOM_NAV_LOS_HD inline
#endif

namespace lom {

// step 8: c is a cell cost of step 1 (0 = impassable); max_cell_cost == 0 admits every passable cell
LOM_NAV_LOS_HD bool nav_clear(uint32_t c, uint32_t max_cell_cost) { return c != 0u && (max_cell_cost == 0u || c <= max_cell_cost); }

// Step 8: whether B = (x1, y1) is visible from A = (x0, y0).  Cost: c at (x, y), a cell of the grid, by any means.  With
// i, j the steps taken along x and y, (2 i + 1) * ay against (2 j + 1) * ax says which border the segment crosses next
// (sides <= 8192: both below 2^27); equal is a lattice corner, where both step and both side cells must be clear.  While
// i == ax the comparison says y, while j == ay it says x, and a corner has i < ax and j < ay: every cell that is read lies
// in the box of A and B, so in the grid.  A itself is not read.
template <class Cost>
LOM_NAV_LOS_HD bool nav_visible(int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint32_t width, uint32_t height, uint32_t max_cell_cost,
                                const Cost &cost)
{
    if ((uint32_t)x0 >= width || (uint32_t)y0 >= height || (uint32_t)x1 >= width || (uint32_t)y1 >= height) return false;
    const int32_t dx = x1 - x0, dy = y1 - y0;
    const int32_t sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
    const uint32_t ax = (uint32_t)(dx < 0 ? -dx : dx), ay = (uint32_t)(dy < 0 ? -dy : dy);
    uint32_t i = 0u, j = 0u;
    int32_t x = x0, y = y0;
    while (i != ax || j != ay) {
        const uint32_t l = (2u * i + 1u) * ay, r = (2u * j + 1u) * ax;
        if (l < r) {
            x += sx, i++;
        } else if (l > r) {
            y += sy, j++;
        } else {
            if (!nav_clear(cost(x + sx, y), max_cell_cost) || !nav_clear(cost(x, y + sy), max_cell_cost)) return false;
            x += sx, y += sy, i++, j++;
        }
        if (!nav_clear(cost(x, y), max_cell_cost)) return false;
    }
    return true;
}

// Step 9, one anchor, the candidates one after another from the farthest: the greatest j in (a, min(a + W, n - 1)] with
// route[j] visible from route[a], a + 1 if none is (a + 1 itself needs no test).  route: n u16 (ix, iy) pairs, a < n - 1.
template <class Cost>
LOM_NAV_LOS_HD uint32_t nav_next_anchor(const uint16_t *route, uint32_t n, uint32_t a, uint32_t W, uint32_t width, uint32_t height,
                                        uint32_t max_cell_cost, const Cost &cost)
{
    const uint32_t hi = W < n - 1u - a ? a + W : n - 1u;
    const int32_t x0 = route[2 * (size_t)a], y0 = route[2 * (size_t)a + 1];
    for (uint32_t j = hi; j > a + 1u; j--)
        if (nav_visible(x0, y0, (int32_t)route[2 * (size_t)j], (int32_t)route[2 * (size_t)j + 1], width, height, max_cell_cost, cost)) return j;
    return a + 1u;
}

// Step 9 for one route of n >= 1 cells, the candidates one after another: up to wp_cap waypoints to out (u16 pairs; may be
// NULL with wp_cap 0); returns the full count.
template <class Cost>
LOM_NAV_LOS_HD uint32_t nav_waypoints_serial(const uint16_t *route, uint32_t n, uint32_t W, uint32_t width, uint32_t height,
                                             uint32_t max_cell_cost, const Cost &cost, uint16_t *out, size_t wp_cap)
{
    uint32_t count = 0u, a = 0u;
    for (;;) {
        if (count < wp_cap) out[2 * (size_t)count] = route[2 * (size_t)a], out[2 * (size_t)count + 1] = route[2 * (size_t)a + 1];
        count++;
        if (a >= n - 1u) return count;
        a = nav_next_anchor(route, n, a, W, width, height, max_cell_cost, cost);
    }
}

// the cell costs of a plane in plain memory: the byte through the table of step 1
struct NavPlaneCost {
    const int8_t *plane;
    const uint32_t *table;
    uint32_t width;
    LOM_NAV_LOS_HD uint32_t operator()(int32_t x, int32_t y) const { return table[(uint8_t)plane[(size_t)y * width + (uint32_t)x]]; }
};

}  // namespace lom
