// Navigation field, the shift with a re-solve (include/lidar_odometry_amd.h, "navigation field", "Shift and re-solve";
// DESIGN.md 7s): k_nav_shift_diff, the mover and the diff in one pass.  Behind it run k_nav_raise, the seeds, k_nav_relax
// and k_nav_report, unchanged.  Device code only; navfield.hip is the one translation unit that instantiates and launches
// it.  Integers throughout; plain vector stores and vector atomics only; no LDS beyond one word; no scratch; no workgroup
// ever waits for another.
#pragma once
#include "k_navfield_resolve.hpp"

namespace lom {

// the words of a shift with a re-solve, behind the re-solve's in the same block (zeroed per call)
enum { SW_ENTERED = RW_END, SW_GOALS_LEFT, SW_END };

// What the host plans (navfield_host.hpp, ShiftPlan): the clamped shift, the kept box [kx0, kx1) x [ky0, ky1) in
// destination cells and the clipped window [wx0, wx1) x [wy0, wy1); either may be empty (x0 >= x1).
struct NavShift {
    int32_t dx, dy;
    uint32_t kx0, ky0, kx1, ky1;
    uint32_t wx0, wy0, wx1, wy1;
};

// four u32, or four bytes, that sit at any offset: what a row moved by dx cells is against the destination's chunks
struct __attribute__((packed, aligned(4))) NavU32x4 {
    uint32_t v[4];
};
struct __attribute__((packed, aligned(1))) NavBytes4 {
    uint32_t v;
};

// One pass over the destination, a workgroup per tile; lane t owns the four cells (4 (t & 7) .. + 3, t >> 3) of it, a run
// of one row, so a wave's loads and stores of P cover eight rows of 128 consecutive bytes.  Destination cell (ix, iy) takes
// P and the kept byte of source cell (ix + dx, iy + dy) where the kept box holds it; every other cell has entered: P
// unreached and the incoming plane's byte.  A kept cell of the window takes the incoming byte too, and is changed where
// that differs from the kept one; a changed cell that is now impassable reads unreached (a goal among them counts as
// rejected).  Both go to the second block: every destination byte of both planes is written exactly once, by the lane
// that owns it, and no lane reads what another writes (the sources are the first block and the incoming plane).  The
// incoming plane is read at entered cells and at kept cells of the window, nowhere else.
//
// Stores: a run that lies in the grid with its first cell at a multiple of four cells goes out as one aligned dwordx4 of P
// and one dword of bytes (every run when the width is a multiple of four); any other run cell by cell.  Loads: a run
// whose four sources are kept loads P as one 16-byte access 4 * dx bytes off the chunk's alignment and the bytes as one
// dword at any byte offset (gfx950 takes both unaligned; profiles/navfield_shift_kernel_resources.txt has what the
// compiler emits).
//
// Counts: kept cells that changed (RW_CHANGED), entered cells (SW_ENTERED), rejected goals (NW_GOALS_REJECTED), and the
// goals that left (SW_GOALS_LEFT): the lane also reads the SOURCE cell at its own index where no destination takes that
// cell, and counts it where P == 0.
//
// Marks, as k_nav_diff leaves them: the tiles that hold a changed or an entered cell, or one of its eight neighbours,
// in marks_a (counted as seeds) and marks_b; and in marks_b alone the tiles that hold a kept cell on a trailing border --
// column 0 for dx > 0, column width - 1 for dx < 0, rows likewise -- whose supporter may have left the grid: the raise phase
// must look at them, and makes a seed of a tile itself where a cell rises.  A step between two cells of the grid never
// depends on a cell outside it, so no other kept cell lost a supporter to the move; an entered cell takes none away
// either (outside the grid was impassable).  Either array may be NULL.
__global__ __launch_bounds__(kNavThreads) void k_nav_shift_diff(const int8_t *__restrict__ incoming, const uint32_t *__restrict__ table,
                                                                NavArgs a, NavShift s, const int8_t *__restrict__ src_plane,
                                                                const uint32_t *__restrict__ src_field, int8_t *__restrict__ dst_plane,
                                                                uint32_t *__restrict__ dst_field, uint32_t *marks_a, uint32_t *marks_b,
                                                                uint32_t *words)
{
    __shared__ uint32_t s_nb;  // bit d: the neighbour tile in direction d; bit 8: this tile; bit 9: this tile, trailing border
    const uint32_t t = threadIdx.x;
    const uint32_t tx = blockIdx.x, ty = blockIdx.y;
    if (t == 0u) s_nb = 0u;
    __syncthreads();

    const uint32_t x0 = (t & 7u) * 4u, y = t >> 3;
    const uint32_t gx0 = tx * kNavTile + x0, gy = ty * kNavTile + y;
    uint32_t n_changed = 0u, n_entered = 0u, n_rejected = 0u, n_left = 0u, nb = 0u;
    if (gy < a.height && gx0 < a.width) {
        const uint32_t n_own = min(4u, a.width - gx0);
        const size_t cell0 = (size_t)gy * a.width + gx0;
        const bool row_kept = gy >= s.ky0 && gy < s.ky1;
        const bool row_win = gy >= s.wy0 && gy < s.wy1;
        const bool whole = n_own == 4u && (cell0 & 3u) == 0u;  // (the blocks are 256-byte aligned)
        uint32_t p[4], kb[4], nw[4];                           // P, the kept byte and the merged byte, as unsigned
        bool kept[4], need[4];

        // the sources
        if (n_own == 4u && row_kept && gx0 >= s.kx0 && gx0 + 4u <= s.kx1) {
            const size_t src = (size_t)((int32_t)gy + s.dy) * a.width + (size_t)((int32_t)gx0 + s.dx);
            const NavU32x4 v = *reinterpret_cast<const NavU32x4 *>(src_field + src);
            const uint32_t b4 = reinterpret_cast<const NavBytes4 *>(src_plane + src)->v;
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) p[k] = v.v[k], kb[k] = b4 >> (8u * k) & 255u, kept[k] = true;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t gx = gx0 + k;
                kept[k] = k < n_own && row_kept && gx >= s.kx0 && gx < s.kx1;
                p[k] = kNavUnreached, kb[k] = 0u;
                if (kept[k]) {
                    const size_t src = (size_t)((int32_t)gy + s.dy) * a.width + (size_t)((int32_t)gx + s.dx);
                    p[k] = src_field[src], kb[k] = (uint8_t)src_plane[src];
                }
            }
        }
        // the incoming bytes: entered cells and kept cells of the window
        bool all_need = whole;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t gx = gx0 + k;
            need[k] = k < n_own && (!kept[k] || (row_win && gx >= s.wx0 && gx < s.wx1));
            all_need = all_need && need[k];
        }
        if (all_need) {
            const uint32_t b4 = reinterpret_cast<const NavBytes4 *>(incoming + cell0)->v;  // (a caller's plane sits at any offset)
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) nw[k] = b4 >> (8u * k) & 255u;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) nw[k] = need[k] ? (uint32_t)(uint8_t)incoming[cell0 + k] : kb[k];
        }
        // the diff
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            if (k >= n_own) continue;
            const uint32_t gx = gx0 + k;
            const bool changed = kept[k] && nw[k] != kb[k];
            n_changed += changed ? 1u : 0u;
            n_entered += kept[k] ? 0u : 1u;
            if (changed || !kept[k]) nb |= 256u | nav_border_bits(x0 + k, y);
            if (changed && p[k] != kNavUnreached && table[nw[k]] == 0u) {
                n_rejected += p[k] == 0u ? 1u : 0u;
                p[k] = kNavUnreached;
            }
            if (kept[k] && ((s.dx > 0 && gx == 0u) || (s.dx < 0 && gx == a.width - 1u) || (s.dy > 0 && gy == 0u) ||
                            (s.dy < 0 && gy == a.height - 1u)))
                nb |= 512u;
            // the source cell at this index: no destination takes it iff it lies outside the kept box moved by (dx, dy)
            const int32_t bx = (int32_t)gx - s.dx, by = (int32_t)gy - s.dy;
            const bool stays = bx >= (int32_t)s.kx0 && bx < (int32_t)s.kx1 && by >= (int32_t)s.ky0 && by < (int32_t)s.ky1;
            if (!stays && src_field[cell0 + k] == 0u) n_left++;
        }
        // the second block
        if (whole) {
            *reinterpret_cast<uint4 *>(dst_field + cell0) = make_uint4(p[0], p[1], p[2], p[3]);
            *reinterpret_cast<uint32_t *>(dst_plane + cell0) = nw[0] | nw[1] << 8 | nw[2] << 16 | nw[3] << 24;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++)
                if (k < n_own) dst_field[cell0 + k] = p[k], dst_plane[cell0 + k] = (int8_t)nw[k];
        }
    }
    for (uint32_t o = 32u; o; o >>= 1) {
        n_changed += (uint32_t)__shfl_xor((int)n_changed, (int)o);
        n_entered += (uint32_t)__shfl_xor((int)n_entered, (int)o);
        n_rejected += (uint32_t)__shfl_xor((int)n_rejected, (int)o);
        n_left += (uint32_t)__shfl_xor((int)n_left, (int)o);
    }
    if ((t & 63u) == 0u) {
        if (n_changed) atomicAdd(words + RW_CHANGED, n_changed);
        if (n_entered) atomicAdd(words + SW_ENTERED, n_entered);
        if (n_rejected) atomicAdd(words + NW_GOALS_REJECTED, n_rejected);
        if (n_left) atomicAdd(words + SW_GOALS_LEFT, n_left);
    }
    if (nb) atomicOr(&s_nb, nb);
    __syncthreads();
    const uint32_t bits = s_nb;
    if (t < 9u && (bits >> t & 1u)) {
        const int mx = (int)tx + (t < 8u ? nav_dx(t) : 0), my = (int)ty + (t < 8u ? nav_dy(t) : 0);
        if (mx >= 0 && my >= 0 && mx < (int)a.tiles_x && my < (int)a.tiles_y) {
            const uint32_t tile = (uint32_t)my * a.tiles_x + (uint32_t)mx;
            if (marks_a) nav_mark_seed(marks_a, tile, words);
            if (marks_b) marks_b[tile] = 1u;
        }
    }
    if (t == 9u && (bits >> 9 & 1u) && marks_b) marks_b[ty * a.tiles_x + tx] = 1u;
}

}  // namespace lom
