// Pose field, the re-solve after a local cost change (include/lidar_odometry_amd.h, "pose field", "Re-solve"): k_pose_diff,
// k_pose_relayer, k_pose_raise and k_pose_reseed.  The relaxation behind them is k_pose_relax and the summary k_pose_report,
// both of k_posefield.hpp and unchanged.  Device code only; posefield.hip is the one translation unit that instantiates and
// launches it.  Integers throughout; plain vector stores and vector atomics only; no workgroup ever waits for another.
#pragma once
#include "k_posefield.hpp"

namespace lom {

// the words of a re-solve, behind the summary words in the same block (zeroed per re-solve).  The least changed x and y are
// kept complemented, so that zero means none and one atomicMax serves both ends of the box.
enum { QW_CHANGED = PW_COUNT, QW_STATES, QW_RAISED, QW_TILES, QW_X0_INV, QW_Y0_INV, QW_X1, QW_Y1, QW_END };

// what a cell at (x, y) of its tile names: bit d for the neighbour tile in the direction of heading d that reads it as a halo
// cell (E, NE, N, NW, W, SW, S, SE: the order of k_pose_relax's marks)
__device__ __forceinline__ uint32_t pose_border_bits(uint32_t x, uint32_t y)
{
    const bool e = x == kPoseTileX - 1u, n = y == kPoseTileY - 1u, w = x == 0u, so = y == 0u;
    return (e ? 1u : 0u) | (e && n ? 2u : 0u) | (n ? 4u : 0u) | (w && n ? 8u : 0u) | (w ? 16u : 0u) | (w && so ? 32u : 0u) | (so ? 64u : 0u) |
           (e && so ? 128u : 0u);
}

// a tile becomes a seed of the relaxation: marked once, counted once
__device__ __forceinline__ void pose_mark_seed(uint32_t *seeds, uint32_t tile, uint32_t *words)
{
    if (seeds[tile] == 0u && atomicExch(seeds + tile, 1u) == 0u) atomicAdd(words + QW_TILES, 1u);
}

// The diff, one pass over the clipped window [win.x0, win.x1) x [win.y0, win.y1), which lies inside the grid: a lane per
// cell, a workgroup per 32 x 8 cells of the window.  A cell whose new byte differs from the kept one is changed: the kept
// plane takes the byte.  The count and the bounding box of the changed cells go to the words, one set of atomics per wave
// behind a wave reduction.  Nothing else is touched: what a changed byte does to the layers is k_pose_relayer's.
__global__ __launch_bounds__(kPoseThreads) void k_pose_diff(const int8_t *__restrict__ incoming, PoseArgs a, PoseBox win, int8_t *kept,
                                                            uint32_t *words)
{
    const uint32_t t = threadIdx.x;
    const uint32_t gx = win.x0 + blockIdx.x * kPoseTileX + (t & (kPoseTileX - 1u)), gy = win.y0 + blockIdx.y * kPoseTileY + t / kPoseTileX;
    bool changed = false;
    if (gx < win.x1 && gy < win.y1) {
        const size_t cell = (size_t)gy * a.width + gx;
        const int8_t b = incoming[cell];
        if (b != kept[cell]) {
            kept[cell] = b;
            changed = true;
        }
    }
    const uint32_t n = pose_count(changed);
    if (!n) return;  // (the same count for every lane of the wave)
    uint32_t x0i = changed ? ~gx : 0u, y0i = changed ? ~gy : 0u, x1 = changed ? gx + 1u : 0u, y1 = changed ? gy + 1u : 0u;
    for (uint32_t o = 32u; o; o >>= 1) {
        x0i = max(x0i, (uint32_t)__shfl_xor((int)x0i, (int)o)), y0i = max(y0i, (uint32_t)__shfl_xor((int)y0i, (int)o));
        x1 = max(x1, (uint32_t)__shfl_xor((int)x1, (int)o)), y1 = max(y1, (uint32_t)__shfl_xor((int)y1, (int)o));
    }
    if ((t & 63u) == 0u) {
        atomicAdd(words + QW_CHANGED, n);
        atomicMax(words + QW_X0_INV, x0i), atomicMax(words + QW_Y0_INV, y0i);
        atomicMax(words + QW_X1, x1), atomicMax(words + QW_Y1, y1);
    }
}

// The layers over what changed, one launch: heading blockIdx.y, a lane per cell of boxes.all; a lane outside its heading's
// box -- the changed box dilated by that heading's stencil and clipped to the grid, so every state whose stencil covers a
// changed cell is inside -- only takes part in the ballots.  The new layer value comes from the merged plane by
// k_pose_layers' rule, with the same staging of table and stencil (the loop exists twice: see DESIGN.md 7v).  Where it
// differs from the kept one it is written and counted; a state that is now impassable and was reached reads unreached, and
// counts as a rejected goal if its P was 0.  The tile of the cell and the neighbour tiles that read the cell as halo -- a
// changed layer alters their move conditions and the corner rule -- are marked in marks (the raise phase's first launch)
// and in seeds (counted), either of which may be NULL.  No lane reads a P or a layer that another lane writes.
__global__ __launch_bounds__(kPoseThreads) void k_pose_relayer(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table, PoseArgs a,
                                                               const uint32_t *__restrict__ stencil_cells,
                                                               const uint32_t *__restrict__ stencil_first, PoseBoxes boxes, uint32_t *layers,
                                                               uint32_t *field, uint32_t *marks, uint32_t *seeds, uint32_t *words)
{
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_st[kPoseMaxStencil];
    const uint32_t h = blockIdx.y, t = threadIdx.x;
    const uint32_t first = stencil_first[h], n = min(stencil_first[h + 1u] - first, kPoseMaxStencil);
    s_tab[t] = table[t];
    for (uint32_t k = t; k < n; k += kPoseThreads) s_st[k] = stencil_cells[first + k];
    __syncthreads();
    const uint32_t bw = boxes.all.x1 - boxes.all.x0, i = blockIdx.x * kPoseThreads + t;
    const uint32_t ux = boxes.all.x0 + i % bw, uy = boxes.all.y0 + i / bw;
    const PoseBox box = boxes.of[h];
    bool differs = false, rejected = false;
    if (uy < boxes.all.y1 && ux >= box.x0 && ux < box.x1 && uy >= box.y0 && uy < box.y1) {  // (inside the grid: the boxes are clipped)
        const int x = (int)ux, y = (int)uy;
        uint32_t best = 0u;
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t pr = s_st[k];
            const int cx = x + (int)(int16_t)(pr & 0xFFFFu), cy = y + (int)(int16_t)(pr >> 16);
            uint32_t c = 0u;
            if ((uint32_t)cx < a.width && (uint32_t)cy < a.height) c = s_tab[(uint8_t)plane[(size_t)cy * a.width + (uint32_t)cx]];
            if (!c) {
                best = 0u;
                break;
            }
            best = max(best, c);
        }
        const size_t at = (size_t)h * a.width * a.height + (size_t)uy * a.width + ux;
        if (layers[at] != best) {
            layers[at] = best;
            differs = true;
            if (best == 0u) {
                const uint32_t p = field[at];
                if (p != kPoseUnreached) {
                    field[at] = kPoseUnreached;
                    rejected = p == 0u;
                }
            }
            const uint32_t tx = ux / kPoseTileX, ty = uy / kPoseTileY;
            const uint32_t nb = 256u | pose_border_bits(ux % kPoseTileX, uy % kPoseTileY);
            for (uint32_t d = 0; d < 9u; d++) {
                if (!(nb >> d & 1u)) continue;
                const int mx = (int)tx + (d < 8u ? pose_hx(d) : 0), my = (int)ty + (d < 8u ? pose_hy(d) : 0);
                if (mx < 0 || my < 0 || mx >= (int)a.tiles_x || my >= (int)a.tiles_y) continue;
                const uint32_t tile = (uint32_t)my * a.tiles_x + (uint32_t)mx;
                if (marks) marks[tile] = 1u;
                if (seeds) pose_mark_seed(seeds, tile, words);
            }
        }
    }
    const uint32_t n_differ = pose_count(differs), n_rejected = pose_count(rejected);
    if ((t & 63u) == 0u) {
        if (n_differ) atomicAdd(words + QW_STATES, n_differ);
        if (n_rejected) atomicAdd(words + PW_GOALS_REJECTED, n_rejected);
    }
}

// The raise phase, one launch.  Tiles, lanes, LDS, the two mark arrays and the flag are those of k_pose_relax: a workgroup
// owns a tile with all eight headings, lane t the eight states of the cell (t & 31, t >> 5), P and L heading-major in LDS with
// a one-cell halo, and per state the layer value, the allowed moves, the value at the load and the value now in registers.
// A reached state a with P[a] > 0 is safe iff some move a -> b of pose_move is allowed under the new layers with P[b]
// reached and P[b] + weight <= P[a]; a state with P == 0 is safe (k_pose_relayer has taken the goal states that became
// impassable).  An unsafe state is set to unreached, in place.  The tile is swept in LDS until a sweep raises nothing; what
// rose goes back, a border cell of which any heading rose names the neighbour tiles that read it, and a tile in which a
// state rose becomes a seed of the relaxation.
//
// Why any schedule gives the same set.  A supporter b of a has P[b] <= P[a] - weight < P[a], since every weight is positive:
// a translation weighs len * s >= 5 (plus a turn or reverse cost that is not negative) and a spin weighs spin_cost >= 1, which
// the parameter rule enforces wherever spins are enabled -- a spin of weight 0 would let two headings of a cell support
// each other and carry nothing down.  So "safe" is well-founded, and the least set of states to raise -- the states whose
// value no chain of supporters carries down to a goal state -- is defined by it, state by state in increasing order of P.
// A state of that set has no supporter outside it, so once its supporters have risen it rises too, in whatever order.  A
// state outside the set keeps a supporter outside the set, which is never raised, so it is never raised either: a value
// read late or stale -- in LDS while another lane raises it in the same sweep (a lane's own eight states among them: a spin's
// target is its own cell), or a halo state that the neighbour tile raises in HBM during the same launch (a 32-bit word is
// read whole: the old value or unreached) -- can only show a supporter that is gone already and so delay a raise, never
// cause one, provided the reader runs again once the newer value is there: inside a tile the sweeps go on until one raises
// nothing, and across tiles a tile that raised any heading of a border cell marks every neighbour tile that reads that cell
// for the next launch, with the mark arrays of k_pose_relax.  Every move of a state ends in its own cell or one of the eight
// around it, so nothing beyond the halo is read.  When a launch marks nothing, every tile's last load saw the final values
// of its halo and its last sweep raised nothing: exactly the least set has risen.  Every value that is kept is the weight,
// or above the weight, of a real move sequence under the new layers (its chain of supporters), so it is an upper bound of
// the new field, and the goal states are 0: the fixed point of k_pose_relax from this state is the field.
//
// inner_cap and all_tiles as in k_pose_relax.  *flag is set iff the launch marked a tile.
__global__ __launch_bounds__(kPoseThreads) void k_pose_raise(const uint32_t *__restrict__ layers, PoseArgs a, PoseCosts pc, uint32_t inner_cap,
                                                             uint32_t all_tiles, uint32_t *field, uint32_t *marks_cur, uint32_t *marks_nxt,
                                                             uint32_t *seeds, uint32_t *flag, uint32_t *words)
{
    __shared__ uint32_t s_p[kPoseHeadings * kPoseHaloCells];  // the potentials, with the halo
    __shared__ uint32_t s_l[kPoseHeadings * kPoseHaloCells];  // the layers, 0 = impassable or outside the grid
    __shared__ uint32_t s_nb;                                 // the neighbour tiles to mark, a bit per direction
    __shared__ uint32_t s_raised;                             // the states of this tile that rose
    __shared__ uint32_t s_more[3];                            // "a state rose in sweep i" at i % 3

    const uint32_t tile = blockIdx.y * a.tiles_x + blockIdx.x;
    if ((all_tiles | marks_cur[tile]) == 0u) return;  // (the same word for every lane: the whole workgroup leaves)
    const uint32_t t = threadIdx.x;
    if (t == 0u) s_nb = s_raised = s_more[0] = s_more[1] = s_more[2] = 0u;
    __syncthreads();
    if (t == 0u) marks_cur[tile] = 0u;  // behind the barrier: every lane has read the word

    const uint32_t n_cells = a.width * a.height;
    const int gx0 = (int)(blockIdx.x * kPoseTileX) - 1, gy0 = (int)(blockIdx.y * kPoseTileY) - 1;
    for (uint32_t i = t; i < kPoseHeadings * kPoseHaloCells; i += kPoseThreads) {
        const uint32_t h = i / kPoseHaloCells, c = i % kPoseHaloCells;
        const int gx = gx0 + (int)(c % kPoseHaloX), gy = gy0 + (int)(c / kPoseHaloX);
        uint32_t p = kPoseUnreached, l = 0u;
        if (gx >= 0 && gy >= 0 && gx < (int)a.width && gy < (int)a.height) {
            const size_t at = (size_t)h * n_cells + (size_t)gy * a.width + (uint32_t)gx;
            p = field[at], l = layers[at];
        }
        s_p[i] = p, s_l[i] = l;
    }
    __syncthreads();

    // per owned state: its layer value, the moves it may take (a bit per move), its value at the load and now
    const int x = (int)(t & (kPoseTileX - 1u)), y = (int)(t / kPoseTileX);
    const uint32_t li = (uint32_t)(y + 1) * kPoseHaloX + (uint32_t)(x + 1);
    const PoseLayerTile L{s_l};
    uint32_t s[kPoseHeadings], moves[kPoseHeadings], first[kPoseHeadings], cur[kPoseHeadings];
#pragma unroll
    for (uint32_t h = 0; h < kPoseHeadings; h++) {
        s[h] = s_l[h * kPoseHaloCells + li];
        first[h] = cur[h] = s_p[h * kPoseHaloCells + li];
        uint32_t m = 0u;
        if (s[h]) {
#pragma unroll
            for (uint32_t k = 0; k < kPoseMoves; k++) {
                int tx, ty;
                uint32_t th, w;
                m |= pose_move(L, pc, x, y, h, s[h], k, &tx, &ty, &th, &w) ? 1u << k : 0u;
            }
        }
        moves[h] = m;
    }

    // the sweeps, in place, with the three words of k_pose_relax
    uint32_t sweeps = 0u, more;
    do {
        bool changed = false;
#pragma unroll
        for (uint32_t h = 0; h < kPoseHeadings; h++) {
            if (cur[h] == kPoseUnreached || cur[h] == 0u) continue;
            bool safe = false;
#pragma unroll
            for (uint32_t k = 0; k < kPoseMoves; k++) {
                if (!(moves[h] >> k & 1u)) continue;
                const int o = pose_move_sign(k) * (pose_hy(h) * (int)kPoseHaloX + pose_hx(h));
                const uint32_t pb = s_p[pose_move_heading(h, k) * kPoseHaloCells + (uint32_t)((int)li + o)];
                // P[b] + w <= P[a] without a sum that could wrap (unreached is above every P[a])
                safe = safe || (pb <= cur[h] && cur[h] - pb >= pose_move_weight(pc, h, s[h], k));
            }
            if (!safe) {
                cur[h] = kPoseUnreached;
                s_p[h * kPoseHaloCells + li] = kPoseUnreached;
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

    // the states that rose go back; a border cell of which any heading rose names the neighbour tiles that read it
    uint32_t mine = 0u;
    const size_t cell = (size_t)(blockIdx.y * kPoseTileY + (uint32_t)y) * a.width + blockIdx.x * kPoseTileX + (uint32_t)x;
#pragma unroll
    for (uint32_t h = 0; h < kPoseHeadings; h++) {
        if (cur[h] == first[h]) continue;  // (a cell of a cut tile that lies outside the grid was staged unreached: it never rises)
        field[(size_t)h * n_cells + cell] = kPoseUnreached;
        mine++;
    }
    if (mine) {
        const uint32_t nb = pose_border_bits((uint32_t)x, (uint32_t)y);
        if (nb) atomicOr(&s_nb, nb);
        atomicAdd(&s_raised, mine);
    }
    __syncthreads();
    if (t < 8u && (s_nb >> t & 1u)) {
        const int tx = (int)blockIdx.x + pose_hx(t), ty = (int)blockIdx.y + pose_hy(t);
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
        atomicAdd(words + QW_RAISED, s_raised);
        pose_mark_seed(seeds, tile, words);
    }
}

// The baseline form's start, a lane per cell with its eight states, behind k_pose_layers over the whole merged plane: the
// goal states (P == 0; k_pose_relayer has taken those that became impassable) stay, every other reached state reads
// unreached and is counted, and the tiles that read a goal state's cell become the seeds, as k_pose_seed leaves them for a
// full solve.
__global__ __launch_bounds__(kPoseThreads) void k_pose_reseed(PoseArgs a, uint32_t *field, uint32_t *seeds, uint32_t *words)
{
    const uint32_t i = blockIdx.x * kPoseThreads + threadIdx.x, n_cells = a.width * a.height;
    uint32_t rose = 0u;
    if (i < n_cells) {
        bool goal = false;
        for (uint32_t h = 0; h < kPoseHeadings; h++) {
            const uint32_t p = field[(size_t)h * n_cells + i];
            if (p == 0u) {
                goal = true;
            } else if (p != kPoseUnreached) {
                field[(size_t)h * n_cells + i] = kPoseUnreached;
                rose++;
            }
        }
        if (goal) {
            const int x = (int)(i % a.width), y = (int)(i / a.width);
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int nx = x + dx, ny = y + dy;
                    if (nx >= 0 && ny >= 0 && nx < (int)a.width && ny < (int)a.height)
                        pose_mark_seed(seeds, ((uint32_t)ny / kPoseTileY) * a.tiles_x + (uint32_t)nx / kPoseTileX, words);
                }
        }
    }
    for (uint32_t o = 32u; o; o >>= 1) rose += (uint32_t)__shfl_xor((int)rose, (int)o);
    if ((threadIdx.x & 63u) == 0u && rose) atomicAdd(words + QW_RAISED, rose);
}

}  // namespace lom
