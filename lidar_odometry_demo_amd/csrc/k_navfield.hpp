// Navigation field (include/lidar_odometry_amd.h, "navigation field"): k_nav_fill, k_nav_seed, k_nav_relax, k_nav_report,
// k_nav_trace and k_nav_query.  Device code only; navfield.hip is the one translation unit that instantiates and launches
// it.  Integers throughout; plain vector stores and vector atomics only; no workgroup ever waits for another.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lom {

constexpr uint32_t kNavThreads = 256;              // four waves
constexpr uint32_t kNavTile = 32;                  // a tile: 32 x 32 cells, four per lane
constexpr uint32_t kNavHalo = kNavTile + 2u;       // ... staged with a one-cell halo
constexpr uint32_t kNavHaloCells = kNavHalo * kNavHalo;
constexpr uint32_t kNavUnreached = 0xFFFFFFFFu;    // LOM_NAV_UNREACHED
constexpr uint32_t kNavMax = 0xFFFFFFFEu;          // LOM_NAV_MAX
constexpr uint32_t kNavMaxCellCost = (1u << 24) - 1u;

// the summary words of a solve (zeroed per solve)
enum { NW_BLOCKED = 0, NW_REACHED = 1, NW_UNREACHED = 2, NW_INVALID = 3, NW_GOALS_USED = 4, NW_GOALS_REJECTED = 5, NW_RANGE = 6,
       NW_MAX_POTENTIAL = 7, NW_COUNT = 8 };

struct NavArgs {
    uint32_t width, height;
    uint32_t tiles_x, tiles_y;
};

// The eight steps in the fixed order E, N, W, S, NE, NW, SW, SE (+x is E, +y is N): dx + 1 and dy + 1 as two bits each.
__device__ __forceinline__ int nav_dx(uint32_t d) { return (int)((0x8246u >> (2u * d)) & 3u) - 1; }
__device__ __forceinline__ int nav_dy(uint32_t d) { return (int)((0x0A19u >> (2u * d)) & 3u) - 1; }
__device__ __forceinline__ uint32_t nav_len(uint32_t d) { return d < 4u ? 5u : 7u; }

__device__ __forceinline__ uint32_t nav_count(bool v) { return (uint32_t)__popcll(__ballot(v)); }

// the cost of cell (x, y): 0 (impassable) outside the grid
__device__ __forceinline__ uint32_t nav_cost_at(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table, uint32_t width,
                                                uint32_t height, int x, int y)
{
    if (x < 0 || y < 0 || x >= (int)width || y >= (int)height) return 0u;
    return table[(uint8_t)plane[(size_t)y * width + (uint32_t)x]];
}

// Whether the step between (x, y), which is passable, and its neighbour d is allowed: the neighbour is passable, and for
// a diagonal step so are the two cells that share an edge with both.
__device__ __forceinline__ bool nav_step_allowed(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table, uint32_t width,
                                                 uint32_t height, int x, int y, uint32_t d)
{
    const int bx = x + nav_dx(d), by = y + nav_dy(d);
    if (!nav_cost_at(plane, table, width, height, bx, by)) return false;
    return d < 4u || (nav_cost_at(plane, table, width, height, bx, y) && nav_cost_at(plane, table, width, height, x, by));
}

// Step 6, the serial walk of one lane down a field from (x, y).  From cell a the first b in the fixed order with an allowed
// step and P[b] + len * c[a] == P[a]; at the fixed point one exists, and P falls strictly, so the walk ends within n_cells
// steps.  out: `cap` u16 pairs, the first `cap` cells of the path.  Returns the full length, start and goal counted, 0 for a
// start that is not walked.  k_nav_trace and k_navset_trace (k_navset.hpp) call it.
__device__ __forceinline__ uint32_t nav_walk(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table,
                                             const uint32_t *__restrict__ field, NavArgs a, int x, int y, uint32_t cap, uint16_t *out)
{
    const uint32_t n_cells = a.width * a.height;
    uint32_t len = 0u;
    if (x >= 0 && y >= 0 && x < (int)a.width && y < (int)a.height) {
        uint32_t p = field[(size_t)y * a.width + (uint32_t)x];
        while (p != kNavUnreached) {
            if (len < cap) {
                uint16_t *const o = out + (size_t)len * 2u;
                o[0] = (uint16_t)x, o[1] = (uint16_t)y;
            }
            len++;
            if (p == 0u || len >= n_cells) break;
            const uint32_t c = nav_cost_at(plane, table, a.width, a.height, x, y);
            uint32_t next = kNavUnreached;
            for (uint32_t d = 0; d < 8u; d++) {
                if (!nav_step_allowed(plane, table, a.width, a.height, x, y, d)) continue;
                const int bx = x + nav_dx(d), by = y + nav_dy(d);
                const uint32_t pb = field[(size_t)by * a.width + (uint32_t)bx], w = nav_len(d) * c;
                if (pb <= kNavMax - w && pb + w == p) {
                    x = bx, y = by, next = pb;
                    break;
                }
            }
            p = next;  // (unreached: no step fits -- never at the fixed point; the walk ends)
        }
    }
    return len;
}

// The kernels of a lom_navfield.  A translation unit that only wants the device functions above for kernels of its own
// (navset.hip, through k_navset.hpp) defines LOM_NAV_DEVICE_FUNCTIONS_ONLY: a kernel is instantiated in one place.
#ifndef LOM_NAV_DEVICE_FUNCTIONS_ONLY

// create, clear and the start of a solve: every cell unreached, no tile marked in either mark array
__global__ __launch_bounds__(kNavThreads) void k_nav_fill(uint32_t n_cells, uint32_t n_marks, uint32_t *field, uint32_t *marks)
{
    const uint32_t i = blockIdx.x * kNavThreads + threadIdx.x;
    if (i < n_cells) field[i] = kNavUnreached;
    if (i < n_marks) marks[i] = 0u;
}

// Step 3, a lane per goal (cells; a goal given in metres was quantised on the host, (-1, -1) where it is outside): a goal
// on a passable cell of the grid becomes 0 and the tiles that read it active for the first launch.  The exchange tells
// the first of several equal goals from the others, so duplicates count once.
__global__ __launch_bounds__(kNavThreads) void k_nav_seed(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table, NavArgs a,
                                                          const int32_t *__restrict__ goals, uint32_t n, uint32_t *field,
                                                          uint32_t *marks0, uint32_t *words)
{
    const uint32_t i = blockIdx.x * kNavThreads + threadIdx.x;
    bool used = false, rejected = false;
    if (i < n) {
        const int x = goals[2 * (size_t)i], y = goals[2 * (size_t)i + 1];
        if (nav_cost_at(plane, table, a.width, a.height, x, y)) {
            if (atomicExch(field + (size_t)y * a.width + (uint32_t)x, 0u) != 0u) {
                used = true;
                // every tile that holds the goal in its interior or in its halo: the goal's 0 is a value no launch of
                // k_nav_relax writes, so no tile would mark its readers
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int nx = x + dx, ny = y + dy;
                        if (nx >= 0 && ny >= 0 && nx < (int)a.width && ny < (int)a.height)
                            marks0[((uint32_t)ny / kNavTile) * a.tiles_x + (uint32_t)nx / kNavTile] = 1u;
                    }
            }
        } else {
            rejected = true;
        }
    }
    const uint32_t n_used = nav_count(used), n_rejected = nav_count(rejected);
    if ((threadIdx.x & 63u) == 0u) {
        if (n_used) atomicAdd(words + NW_GOALS_USED, n_used);
        if (n_rejected) atomicAdd(words + NW_GOALS_REJECTED, n_rejected);
    }
}

// Step 4, one launch of the relaxation.  A workgroup owns the tile (blockIdx.x, blockIdx.y); lane t owns the four cells
// t + 256 k of it, row-major, so a wave reads two whole rows of LDS at a time and no two lanes of a group share a bank.
//
// Why any schedule gives the same bytes.  Every value a cell ever holds is 0 on a goal or P[b] + len * c[a] for a value
// P[b] some neighbour held: by induction the weight of a real route, so never below the true P, and a cell's value only
// falls.  Hence a value that is read late or stale -- in LDS while another lane rewrites it in the same sweep, or a halo
// cell that the neighbour tile rewrites in HBM during the same launch (a 32-bit word is read whole: the old value or the
// new one) -- is still an upper bound and does no harm, provided the reader runs again once the newer value is there:
// inside a tile the sweeps go on until one changes nothing, and across tiles a tile that lowered a border cell marks
// every neighbour tile that reads that cell for the next launch, whose start is behind this launch's end.  No mark is
// lost: marks for launch k + 1 go to the array that launch k does not read, and a tile clears only its own word, in the
// array it reads, after all its lanes have read it.  When a launch marks nothing, every tile's last load saw the final
// values of its halo and its last sweep changed nothing: no allowed step lowers any cell, every value is the weight of a
// real route, and with positive weights that state is unique -- the field of step 4.  Launches after it change nothing,
// so the host may run ahead.
//
// inner_cap bounds the sweeps of a launch; a tile that stops there marks itself.  all_tiles (a test switch) runs every
// tile in every launch.  *flag is set iff the launch marked a tile.
//
// nav_relax_tile (k_navset.hpp) is this body as a device function, for field blockIdx.z of a set, and the argument covers
// it as well: the fields of a set share nothing but the read-only plane and table -- each has its own P and its own mark
// words, and the one flag of a launch is only ever set.  This kernel keeps its own text: built through the shared function
// it took 40 VGPRs where profiles/navfield_kernel_resources.txt records 48, and its resources are not to move.  A change to
// one body is a change to both.
__global__ __launch_bounds__(kNavThreads) void k_nav_relax(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table, NavArgs a,
                                                           uint32_t inner_cap, uint32_t all_tiles, uint32_t *field, uint32_t *marks_cur,
                                                           uint32_t *marks_nxt, uint32_t *flag)
{
    __shared__ uint32_t s_p[kNavHaloCells];  // the potentials, with the halo
    __shared__ uint32_t s_c[kNavHaloCells];  // the cell costs, 0 = impassable or outside the grid
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_nb;                // the neighbour tiles to mark, a bit per direction
    __shared__ uint32_t s_more[3];           // "a cell fell in sweep i" at i % 3

    const uint32_t tile = blockIdx.y * a.tiles_x + blockIdx.x;
    if ((all_tiles | marks_cur[tile]) == 0u) return;  // (the same word for every lane: the whole workgroup leaves)
    const uint32_t t = threadIdx.x;
    s_tab[t] = table[t];
    if (t == 0u) s_nb = s_more[0] = s_more[1] = s_more[2] = 0u;
    __syncthreads();
    if (t == 0u) marks_cur[tile] = 0u;  // behind the barrier: every lane has read the word

    const int gx0 = (int)(blockIdx.x * kNavTile) - 1, gy0 = (int)(blockIdx.y * kNavTile) - 1;
    for (uint32_t i = t; i < kNavHaloCells; i += kNavThreads) {
        const int gx = gx0 + (int)(i % kNavHalo), gy = gy0 + (int)(i / kNavHalo);
        uint32_t p = kNavUnreached, c = 0u;
        if (gx >= 0 && gy >= 0 && gx < (int)a.width && gy < (int)a.height) {
            const size_t cell = (size_t)gy * a.width + (uint32_t)gx;
            p = field[cell];
            c = s_tab[(uint8_t)plane[cell]];
        }
        s_p[i] = p, s_c[i] = c;
    }
    __syncthreads();

    // per owned cell: its place in LDS, its cost, the steps it may take (a bit per direction), its value at the load and now
    uint32_t li[4], cost[4], steps[4], first[4], cur[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t idx = t + kNavThreads * k, x = idx & 31u, y = idx >> 5;
        li[k] = (y + 1u) * kNavHalo + x + 1u;
        cost[k] = s_c[li[k]];
        first[k] = cur[k] = s_p[li[k]];
        uint32_t m = 0u;
        if (cost[k]) {
#pragma unroll
            for (uint32_t d = 0; d < 8u; d++) {
                const int o = nav_dy(d) * (int)kNavHalo + nav_dx(d);
                bool ok = s_c[(int)li[k] + o] != 0u;
                if (d >= 4u) ok = ok && s_c[(int)li[k] + nav_dx(d)] != 0u && s_c[(int)li[k] + nav_dy(d) * (int)kNavHalo] != 0u;
                m |= ok ? 1u << d : 0u;
            }
        }
        steps[k] = m;
    }

    // the sweeps, in place: P[a] = min(P[a], min over allowed b of P[b] + len * c[a]), candidates above LOM_NAV_MAX dropped
    // Sweep i raises s_more[i % 3] in front of its barrier and reads it behind; lane 0 then lowers the word of sweep i + 2,
    // which sweep i - 1 read last (every lane is past barrier i) and sweep i + 2 writes next (behind barrier i + 1).
    uint32_t sweeps = 0u, more;
    do {
        bool changed = false;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            if (!steps[k]) continue;
            uint32_t best = cur[k];
#pragma unroll
            for (uint32_t d = 0; d < 8u; d++) {
                if (!(steps[k] >> d & 1u)) continue;
                const uint32_t pb = s_p[(int)li[k] + nav_dy(d) * (int)kNavHalo + nav_dx(d)];
                const uint32_t w = nav_len(d) * cost[k];  // < 2^27
                if (pb <= kNavMax - w) best = min(best, pb + w);  // (unreached is above kNavMax - w)
            }
            if (best < cur[k]) {
                cur[k] = best;
                s_p[li[k]] = best;
                changed = true;
            }
        }
        const uint32_t slot = sweeps % 3u;
        if (changed) s_more[slot] = 1u;
        __syncthreads();
        more = s_more[slot];
        if (t == 0u) s_more[(slot + 2u) % 3u] = 0u;
        sweeps++;
    } while (more && sweeps < inner_cap);

    // the interior that fell goes back; a border cell that fell names the neighbour tiles that read it
    uint32_t nb = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        if (cur[k] >= first[k]) continue;
        const uint32_t idx = t + kNavThreads * k, x = idx & 31u, y = idx >> 5;
        field[(size_t)(blockIdx.y * kNavTile + y) * a.width + blockIdx.x * kNavTile + x] = cur[k];
        const bool e = x == kNavTile - 1u, n = y == kNavTile - 1u, w = x == 0u, s = y == 0u;
        nb |= (e ? 1u : 0u) | (n ? 2u : 0u) | (w ? 4u : 0u) | (s ? 8u : 0u) | (e && n ? 16u : 0u) | (w && n ? 32u : 0u) |
              (w && s ? 64u : 0u) | (e && s ? 128u : 0u);
    }
    if (nb) atomicOr(&s_nb, nb);
    __syncthreads();
    if (t < 8u && (s_nb >> t & 1u)) {
        const int tx = (int)blockIdx.x + nav_dx(t), ty = (int)blockIdx.y + nav_dy(t);
        if (tx >= 0 && ty >= 0 && tx < (int)a.tiles_x && ty < (int)a.tiles_y) {
            marks_nxt[(uint32_t)ty * a.tiles_x + (uint32_t)tx] = 1u;
            *flag = 1u;
        }
    }
    if (t == 8u && more) {  // stopped at the cap: not settled yet
        marks_nxt[tile] = 1u;
        *flag = 1u;
    }
}

// Step 5 and range_exceeded, a lane per cell, at the fixed point.
__global__ __launch_bounds__(kNavThreads) void k_nav_report(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table,
                                                            const uint32_t *__restrict__ field, NavArgs a, uint32_t *words)
{
    const uint32_t i = blockIdx.x * kNavThreads + threadIdx.x;
    const bool have = i < a.width * a.height;
    bool blocked = false, reached = false, invalid = false, exceeded = false;
    uint32_t p = 0u;
    if (have) {
        const int b = plane[i];
        const uint32_t c = table[(uint8_t)b];
        invalid = b < -1 || b > 100;
        blocked = c == 0u;
        p = field[i];
        reached = p != kNavUnreached;
        // some allowed step a -> this cell with P + len * c[a] above LOM_NAV_MAX; none can be while P + 7 * 2^24 fits
        if (reached && p > kNavMax - 7u * kNavMaxCellCost) {
            const int x = (int)(i % a.width), y = (int)(i / a.width);
            for (uint32_t d = 0; d < 8u; d++) {
                if (!nav_step_allowed(plane, table, a.width, a.height, x, y, d)) continue;
                const uint32_t ca = nav_cost_at(plane, table, a.width, a.height, x + nav_dx(d), y + nav_dy(d));
                exceeded = exceeded || p > kNavMax - nav_len(d) * ca;
            }
        }
        if (!reached) p = 0u;
    }
    const uint32_t n_blocked = nav_count(blocked), n_reached = nav_count(reached), n_unreached = nav_count(have && !blocked && !reached),
                   n_invalid = nav_count(invalid);
    const bool any_exceeded = __ballot(exceeded) != 0ull;
    for (uint32_t o = 32u; o; o >>= 1) p = max(p, (uint32_t)__shfl_xor((int)p, (int)o));
    if ((threadIdx.x & 63u) == 0u) {
        if (n_blocked) atomicAdd(words + NW_BLOCKED, n_blocked);
        if (n_reached) atomicAdd(words + NW_REACHED, n_reached);
        if (n_unreached) atomicAdd(words + NW_UNREACHED, n_unreached);
        if (n_invalid) atomicAdd(words + NW_INVALID, n_invalid);
        if (any_exceeded) atomicOr(words + NW_RANGE, 1u);
        if (p) atomicMax(words + NW_MAX_POTENTIAL, p);
    }
}

// Step 6, a lane per start (cells; (-1, -1) where a start in metres is outside).  out: [K, cap] u16 pairs; lengths[k]: the
// full length.
__global__ __launch_bounds__(kNavThreads) void k_nav_trace(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table,
                                                           const uint32_t *__restrict__ field, NavArgs a,
                                                           const int32_t *__restrict__ starts, uint32_t K, uint32_t cap, uint16_t *out,
                                                           uint32_t *lengths)
{
    const uint32_t k = blockIdx.x * kNavThreads + threadIdx.x;
    if (k >= K) return;
    lengths[k] = nav_walk(plane, table, field, a, starts[2 * (size_t)k], starts[2 * (size_t)k + 1], cap, out + (size_t)k * cap * 2u);
}

// Step 7, a lane per point: the cell by the floor rule (f64 from the f32 values, compared before any conversion) and its
// P; unreached outside the grid (a NaN coordinate fails both comparisons).
__global__ __launch_bounds__(kNavThreads) void k_nav_query(const float *__restrict__ xy, uint32_t n, float resolution, float origin_x,
                                                           float origin_y, NavArgs a, const uint32_t *__restrict__ field, uint32_t *out)
{
    const uint32_t i = blockIdx.x * kNavThreads + threadIdx.x;
    if (i >= n) return;
    const double r = (double)resolution;
    const double qx = __builtin_floor(((double)xy[2 * (size_t)i] - (double)origin_x) / r);
    const double qy = __builtin_floor(((double)xy[2 * (size_t)i + 1] - (double)origin_y) / r);
    uint32_t p = kNavUnreached;
    if (qx >= 0.0 && qx < (double)a.width && qy >= 0.0 && qy < (double)a.height) p = field[(size_t)(uint32_t)qy * a.width + (uint32_t)qx];
    out[i] = p;
}

#endif  // LOM_NAV_DEVICE_FUNCTIONS_ONLY

}  // namespace lom
