// Navigation field, steps 8 and 9 (include/lidar_odometry_amd.h, "navigation field"): k_nav_visible,
// k_nav_shortcut and its comparison form k_nav_shortcut_serial.  The rule itself is nav_los_rule.hpp's, shared with the
// host.  Device code only; navfield.hip is the one translation unit that instantiates and launches it.  Integers
// throughout; plain vector stores only; no LDS; no workgroup ever waits for another.
#pragma once
#include "k_navfield.hpp"
#include "nav_los_rule.hpp"

namespace lom {

constexpr uint32_t kNavWave = 64;
constexpr uint32_t kNavRoutesPerGroup = kNavThreads / kNavWave;  // k_nav_shortcut: a wave per route

// the cell costs of the field's plane in HBM; 0 outside the grid (the walk never leaves it: the test costs a compare)
struct NavDeviceCost {
    const int8_t *plane;
    const uint32_t *table;
    uint32_t width, height;
    __device__ __forceinline__ uint32_t operator()(int32_t x, int32_t y) const { return nav_cost_at(plane, table, width, height, x, y); }
};

// Step 8, a lane per pair: pairs are int32 quadruples (x0, y0, x1, y1), out a byte per pair.
__global__ __launch_bounds__(kNavThreads) void k_nav_visible(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table, NavArgs a,
                                                             const int32_t *__restrict__ pairs, uint32_t n, uint32_t max_cell_cost,
                                                             uint8_t *out)
{
    const uint32_t i = blockIdx.x * kNavThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t *const q = pairs + 4 * (size_t)i;
    out[i] = nav_visible(q[0], q[1], q[2], q[3], a.width, a.height, max_cell_cost, NavDeviceCost{plane, table, a.width, a.height}) ? 1u : 0u;
}

// Step 9, a wave per route, four routes per workgroup.  routes: [K, route_cap] u16 pairs as k_nav_trace left them, read as
// one 32-bit word per cell (ix in the low half); lengths: k_nav_trace's; out: [K, wp_cap] words, zeroed by the host;
// counts[k]: the full number of waypoints.  Per anchor a the candidates (a, hi], hi = min(a + W, n - 1), go to the lanes in
// chunks of 64, the farthest chunk first: lane l of the chunk under `top` takes j = top - 63 + l, reads its cell -- 64
// consecutive words -- and walks its own segment up to the first cell that is not clear.  The ballot's highest bit is the
// greatest visible j of the chunk, and the first chunk with one ends the anchor.  a + 1 counts as visible untested (the
// rule's "a + 1 if none is"), so the chunk that holds it always ends the search.  Every value that steers the loops is the
// same in all lanes of a wave: no lane leaves before the others.
__global__ __launch_bounds__(kNavThreads) void k_nav_shortcut(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table, NavArgs g,
                                                              const uint32_t *__restrict__ routes, const uint32_t *__restrict__ lengths,
                                                              uint32_t K, uint32_t route_cap, uint32_t W, uint32_t max_cell_cost,
                                                              uint32_t *out, uint32_t wp_cap, uint32_t *counts)
{
    const uint32_t lane = threadIdx.x & (kNavWave - 1u);
    const uint32_t k = blockIdx.x * kNavRoutesPerGroup + threadIdx.x / kNavWave;
    if (k >= K) return;  // (the same k for every lane of a wave)
    const uint32_t n = min(lengths[k], route_cap);
    const uint32_t *const r = routes + (size_t)k * route_cap;
    uint32_t *const o = out + (size_t)k * wp_cap;
    const NavDeviceCost cost{plane, table, g.width, g.height};
    uint32_t count = 0u, a = 0u;
    while (n) {
        const uint32_t ra = r[a];
        if (lane == 0u && count < wp_cap) o[count] = ra;
        count++;
        if (a >= n - 1u) break;
        const int32_t x0 = (int32_t)(ra & 0xFFFFu), y0 = (int32_t)(ra >> 16);
        const uint32_t hi = min(a + W, n - 1u);  // (a < 2^28, W < 2^16)
        uint32_t next = a + 1u;
        for (uint32_t top = hi;; top -= kNavWave) {
            const int32_t j = (int32_t)(top + lane) - (int32_t)(kNavWave - 1u);
            bool vis = false;
            if (j > (int32_t)a) {
                vis = j == (int32_t)a + 1;
                if (!vis) {
                    const uint32_t rb = r[j];
                    vis = nav_visible(x0, y0, (int32_t)(rb & 0xFFFFu), (int32_t)(rb >> 16), g.width, g.height, max_cell_cost, cost);
                }
            }
            const unsigned long long m = __ballot(vis);
            if (m) {
                next = top - (uint32_t)__clzll((long long)m);  // lane 63 - clz holds j = top - clz
                break;
            }
            if (top <= a + kNavWave) break;  // (never: this chunk held a + 1)
        }
        a = next;
    }
    if (lane == 0u) counts[k] = count;
}

// The comparison form (LOM_NAV_OPT_TEST_SHORTCUT_SERIAL): a lane per route, the candidates one after another from the
// farthest.  The same bytes.
__global__ __launch_bounds__(kNavThreads) void k_nav_shortcut_serial(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table,
                                                                     NavArgs g, const uint16_t *__restrict__ routes,
                                                                     const uint32_t *__restrict__ lengths, uint32_t K, uint32_t route_cap,
                                                                     uint32_t W, uint32_t max_cell_cost, uint16_t *out, uint32_t wp_cap,
                                                                     uint32_t *counts)
{
    const uint32_t k = blockIdx.x * kNavThreads + threadIdx.x;
    if (k >= K) return;
    const uint32_t n = min(lengths[k], route_cap);
    counts[k] = n ? nav_waypoints_serial(routes + (size_t)k * route_cap * 2u, n, W, g.width, g.height, max_cell_cost,
                                         NavDeviceCost{plane, table, g.width, g.height}, out + (size_t)k * wp_cap * 2u, (size_t)wp_cap)
                  : 0u;
}

}  // namespace lom
