// Navigation field, the re-solve after a local cost change (include/lidar_odometry_amd.h, "navigation field", "Re-solve"):
// k_nav_diff, k_nav_raise, k_nav_threshold and k_nav_reseed.  The relaxation behind them is k_nav_relax and the summary
// k_nav_report, both of k_navfield.hpp and unchanged.  Device code only; navfield.hip is the one translation unit that
// instantiates and launches it.  Integers throughout; plain vector stores and vector atomics only; no workgroup ever waits
// for another.
#pragma once
#include "k_navfield.hpp"

namespace lom {

// the words of a re-solve, behind the summary words in the same block (zeroed per re-solve)
enum { RW_CHANGED = NW_COUNT, RW_RAISED, RW_PMIN_INV, RW_TILES, RW_END };

// the clipped window [x0, x1) x [y0, y1), not empty, and the first tile that holds a cell of it
struct NavWindow {
    uint32_t x0, y0, x1, y1;
    uint32_t tx0, ty0;
};

// what a cell at (x, y) of its tile names: bit d for the neighbour tile in direction d that reads it as a halo cell
__device__ __forceinline__ uint32_t nav_border_bits(uint32_t x, uint32_t y)
{
    const bool e = x == kNavTile - 1u, n = y == kNavTile - 1u, w = x == 0u, s = y == 0u;
    return (e ? 1u : 0u) | (n ? 2u : 0u) | (w ? 4u : 0u) | (s ? 8u : 0u) | (e && n ? 16u : 0u) | (w && n ? 32u : 0u) |
           (w && s ? 64u : 0u) | (e && s ? 128u : 0u);
}

// a tile becomes a seed of the relaxation: marked once, counted once
__device__ __forceinline__ void nav_mark_seed(uint32_t *seeds, uint32_t tile, uint32_t *words)
{
    if (seeds[tile] == 0u && atomicExch(seeds + tile, 1u) == 0u) atomicAdd(words + RW_TILES, 1u);
}

// The diff, one pass over the clipped window; a workgroup per tile that holds a cell of it, lane t owns the cells
// t + 256 k of the tile.  A cell whose new byte differs from the kept one is changed: the kept plane takes the byte, and a
// cell that is now impassable reads unreached (a goal among them counts as rejected).  The tiles that hold a changed cell
// or one of its eight neighbours -- a changed cell alters its neighbours' diagonal steps through the corner rule -- are
// marked in marks_a (counted as seeds) and marks_b, either of which may be NULL.  want_pmin: the least positive P among the
// changed cells and their neighbours goes to RW_PMIN_INV, complemented so that zero means none.  A lane reads its own
// P before it writes it, and a neighbour that another lane resets at the same time gives its old value through that lane:
// the minimum does not depend on the order.
__global__ __launch_bounds__(kNavThreads) void k_nav_diff(const int8_t *__restrict__ incoming, const uint32_t *__restrict__ table, NavArgs a,
                                                          NavWindow win, uint32_t want_pmin, int8_t *kept, uint32_t *field,
                                                          uint32_t *marks_a, uint32_t *marks_b, uint32_t *words)
{
    __shared__ uint32_t s_nb;  // bit d: the neighbour tile in direction d; bit 8: this tile
    const uint32_t t = threadIdx.x;
    const uint32_t tx = win.tx0 + blockIdx.x, ty = win.ty0 + blockIdx.y;
    if (t == 0u) s_nb = 0u;
    __syncthreads();

    uint32_t n_changed = 0u, n_rejected = 0u, nb = 0u, low = 0u;  // low: the complement of the least positive P seen
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t idx = t + kNavThreads * k, x = idx & 31u, y = idx >> 5;
        const uint32_t gx = tx * kNavTile + x, gy = ty * kNavTile + y;
        if (gx < win.x0 || gx >= win.x1 || gy < win.y0 || gy >= win.y1) continue;  // (the window lies inside the grid)
        const size_t cell = (size_t)gy * a.width + gx;
        const int8_t b = incoming[cell];
        if (b == kept[cell]) continue;
        kept[cell] = b;
        n_changed++;
        nb |= 256u | nav_border_bits(x, y);
        const uint32_t p = field[cell];
        if (table[(uint8_t)b] == 0u && p != kNavUnreached) {
            n_rejected += p == 0u ? 1u : 0u;
            field[cell] = kNavUnreached;
        }
        if (want_pmin) {
            if (p != kNavUnreached && p > 0u) low = max(low, ~p);
            for (uint32_t d = 0; d < 8u; d++) {
                const int nx = (int)gx + nav_dx(d), ny = (int)gy + nav_dy(d);
                if (nx < 0 || ny < 0 || nx >= (int)a.width || ny >= (int)a.height) continue;
                const uint32_t pn = field[(size_t)ny * a.width + (uint32_t)nx];
                if (pn != kNavUnreached && pn > 0u) low = max(low, ~pn);
            }
        }
    }
    for (uint32_t o = 32u; o; o >>= 1) {
        n_changed += (uint32_t)__shfl_xor((int)n_changed, (int)o);
        n_rejected += (uint32_t)__shfl_xor((int)n_rejected, (int)o);
        low = max(low, (uint32_t)__shfl_xor((int)low, (int)o));
    }
    if ((t & 63u) == 0u) {
        if (n_changed) atomicAdd(words + RW_CHANGED, n_changed);
        if (n_rejected) atomicAdd(words + NW_GOALS_REJECTED, n_rejected);
        if (low) atomicMax(words + RW_PMIN_INV, low);
    }
    if (nb) atomicOr(&s_nb, nb);
    __syncthreads();
    if (t < 9u && (s_nb >> t & 1u)) {
        const int mx = (int)tx + (t < 8u ? nav_dx(t) : 0), my = (int)ty + (t < 8u ? nav_dy(t) : 0);
        if (mx >= 0 && my >= 0 && mx < (int)a.tiles_x && my < (int)a.tiles_y) {
            const uint32_t tile = (uint32_t)my * a.tiles_x + (uint32_t)mx;
            if (marks_a) nav_mark_seed(marks_a, tile, words);
            if (marks_b) marks_b[tile] = 1u;
        }
    }
}

// The raise phase, one launch.  Tiles, lanes, LDS, the two mark arrays and the flag are those of k_nav_relax.  A reached
// cell a with P[a] > 0 is safe iff some step a -> b is allowed under the merged plane with P[b] reached and
// P[b] + len * c[a] <= P[a]; a cell with P == 0 is safe (the diff has taken the goals that became impassable).  An unsafe
// cell is set to unreached, in place.  The tile is swept in LDS until a sweep raises nothing; what rose goes back, a
// border cell that rose names the neighbour tiles that read it, and a tile in which a cell rose becomes a seed of the
// relaxation.
//
// Why any schedule gives the same set.  A supporter b of a has P[b] <= P[a] - len * c[a] < P[a], since every weight is at
// least 5: "safe" is well-founded, and the least set of cells to raise -- the cells whose value no chain of supporters
// carries down to a goal -- is defined by it, cell by cell in increasing order of P.  A cell of that set has no supporter
// outside it, so once its supporters have risen it rises too, in whatever order.  A cell outside the set keeps a
// supporter outside the set, which is never raised, so it is never raised either: a value read late or stale -- in LDS
// while another lane raises it in the same sweep, or a halo cell that the neighbour tile raises in HBM during the same
// launch (a 32-bit word is read whole: the old value or unreached) -- can only show a supporter that is gone already and
// so delay a raise, never cause one, provided the reader runs again once the newer value is there: inside a tile the
// sweeps go on until one raises nothing, and across tiles a tile that raised a border cell marks every neighbour tile that
// reads that cell for the next launch, with the mark arrays of k_nav_relax.  When a launch marks nothing, every tile's last
// load saw the final values of its halo and its last sweep raised nothing: exactly the least set has risen.  Every value
// that is kept is the weight, or above the weight, of a real route under the merged plane (its chain of supporters), so it
// is an upper bound of the new field, and the goals are 0: the fixed point of k_nav_relax from this state is the field.
//
// inner_cap and all_tiles as in k_nav_relax.  *flag is set iff the launch marked a tile.
__global__ __launch_bounds__(kNavThreads) void k_nav_raise(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table, NavArgs a,
                                                           uint32_t inner_cap, uint32_t all_tiles, uint32_t *field, uint32_t *marks_cur,
                                                           uint32_t *marks_nxt, uint32_t *seeds, uint32_t *flag, uint32_t *words)
{
    __shared__ uint32_t s_p[kNavHaloCells];  // the potentials, with the halo
    __shared__ uint32_t s_c[kNavHaloCells];  // the cell costs, 0 = impassable or outside the grid
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_nb;                // the neighbour tiles to mark, a bit per direction
    __shared__ uint32_t s_raised;            // the cells of this tile that rose
    __shared__ uint32_t s_more[3];           // "a cell rose in sweep i" at i % 3

    const uint32_t tile = blockIdx.y * a.tiles_x + blockIdx.x;
    if ((all_tiles | marks_cur[tile]) == 0u) return;  // (the same word for every lane: the whole workgroup leaves)
    const uint32_t t = threadIdx.x;
    s_tab[t] = table[t];
    if (t == 0u) s_nb = s_raised = s_more[0] = s_more[1] = s_more[2] = 0u;
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

    // the sweeps, in place, with the three words of k_nav_relax
    uint32_t sweeps = 0u, more;
    do {
        bool changed = false;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            if (cur[k] == kNavUnreached || cur[k] == 0u) continue;
            bool safe = false;
#pragma unroll
            for (uint32_t d = 0; d < 8u; d++) {
                if (!(steps[k] >> d & 1u)) continue;
                const uint32_t pb = s_p[(int)li[k] + nav_dy(d) * (int)kNavHalo + nav_dx(d)];
                // P[b] + w <= P[a] without a sum that could wrap (unreached is above every P[a])
                safe = safe || (pb <= cur[k] && cur[k] - pb >= nav_len(d) * cost[k]);
            }
            if (!safe) {
                cur[k] = kNavUnreached;
                s_p[li[k]] = kNavUnreached;
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

    // the interior that rose goes back; a border cell that rose names the neighbour tiles that read it
    uint32_t nb = 0u, mine = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        if (cur[k] == first[k]) continue;
        const uint32_t idx = t + kNavThreads * k, x = idx & 31u, y = idx >> 5;
        field[(size_t)(blockIdx.y * kNavTile + y) * a.width + blockIdx.x * kNavTile + x] = kNavUnreached;
        nb |= nav_border_bits(x, y);
        mine++;
    }
    if (nb) atomicOr(&s_nb, nb);
    if (mine) atomicAdd(&s_raised, mine);
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
    if (t == 9u && s_raised) {
        atomicAdd(words + RW_RAISED, s_raised);
        nav_mark_seed(seeds, tile, words);
    }
}

// The threshold form's reset, a lane per cell, in place of the raise phase: every reached cell with P > 0 and P >= pmin
// reads unreached, and its tile becomes a seed.  Weights are positive, so no cell below pmin has a route through a cell
// the diff found changed, or through a neighbour of one: its value stands.
__global__ __launch_bounds__(kNavThreads) void k_nav_threshold(NavArgs a, uint32_t *field, uint32_t *seeds, uint32_t *words)
{
    const uint32_t i = blockIdx.x * kNavThreads + threadIdx.x;
    const uint32_t pmin = ~words[RW_PMIN_INV];  // unreached where the diff saw no positive P
    bool rose = false;
    if (i < a.width * a.height) {
        const uint32_t p = field[i];
        rose = p != kNavUnreached && p > 0u && p >= pmin;
        if (rose) {
            field[i] = kNavUnreached;
            nav_mark_seed(seeds, ((i / a.width) / kNavTile) * a.tiles_x + (i % a.width) / kNavTile, words);
        }
    }
    const uint32_t n = nav_count(rose);
    if ((threadIdx.x & 63u) == 0u && n) atomicAdd(words + RW_RAISED, n);
}

// The baseline form's start, a lane per cell: the goals (P == 0 on a passable cell) stay, every other cell reads
// unreached, and the tiles that read a goal become the seeds, as k_nav_seed leaves them for a full solve.
__global__ __launch_bounds__(kNavThreads) void k_nav_reseed(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table, NavArgs a,
                                                            uint32_t *field, uint32_t *seeds, uint32_t *words)
{
    const uint32_t i = blockIdx.x * kNavThreads + threadIdx.x;
    bool rose = false;
    if (i < a.width * a.height) {
        const uint32_t p = field[i];
        if (p == 0u && table[(uint8_t)plane[i]] != 0u) {
            const int x = (int)(i % a.width), y = (int)(i / a.width);
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int nx = x + dx, ny = y + dy;
                    if (nx >= 0 && ny >= 0 && nx < (int)a.width && ny < (int)a.height)
                        nav_mark_seed(seeds, ((uint32_t)ny / kNavTile) * a.tiles_x + (uint32_t)nx / kNavTile, words);
                }
        } else if (p != kNavUnreached) {
            rose = true;
            field[i] = kNavUnreached;
        }
    }
    const uint32_t n = nav_count(rose);
    if ((threadIdx.x & 63u) == 0u && n) atomicAdd(words + RW_RAISED, n);
}

}  // namespace lom
