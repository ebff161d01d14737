// Pose field (include/lidar_odometry_amd.h, "pose field"): k_pose_fill, k_pose_layers, k_pose_seed, k_pose_relax,
// k_pose_report, k_pose_trace and k_pose_query.  Device code only; posefield.hip is the one translation unit that
// instantiates and launches it.  The move rule is pose_rule.hpp's, shared with the host.  P and L are planar, [8][height]
// [width] u32.  Integers throughout; plain vector stores and vector atomics only; no workgroup ever waits for another.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pose_rule.hpp"

namespace lom {

constexpr uint32_t kPoseThreads = 256;                 // four waves
constexpr uint32_t kPoseTileX = 32, kPoseTileY = 8;    // a tile: 32 x 8 cells with all eight headings, a cell per lane
constexpr uint32_t kPoseHaloX = kPoseTileX + 2u, kPoseHaloY = kPoseTileY + 2u;  // ... staged with a one-cell halo
constexpr uint32_t kPoseHaloCells = kPoseHaloX * kPoseHaloY;                    // 340: P and L of a tile are 21.8 KB of LDS
constexpr uint32_t kPoseUnreached = 0xFFFFFFFFu;       // LOM_NAV_UNREACHED
constexpr uint32_t kPoseMax = 0xFFFFFFFEu;             // LOM_NAV_MAX
constexpr uint32_t kPoseMaxWeight = 8u * ((1u << 24) - 1u);  // no move weighs more: 7 * c + a cost
constexpr uint32_t kPoseMaxStencil = 1024;             // cells of a stencil
constexpr uint32_t kPoseNoHeading = 8;                 // floor_heading where nothing is reached

// the summary words of a solve (zeroed per solve)
enum { PW_BLOCKED = 0, PW_REACHED = 1, PW_UNREACHED = 2, PW_CELLS_REACHED = 3, PW_INVALID = 4, PW_GOALS_USED = 5, PW_GOALS_REJECTED = 6,
       PW_RANGE = 7, PW_MAX_POTENTIAL = 8, PW_COUNT = 9 };

struct PoseArgs {
    uint32_t width, height;
    uint32_t tiles_x, tiles_y;
};

__device__ __forceinline__ uint32_t pose_count(bool v) { return (uint32_t)__popcll(__ballot(v)); }

// the layers of a tile in LDS, in tile coordinates (-1 .. tile: the halo); cells outside the grid were staged as 0
struct PoseLayerTile {
    const uint32_t *s_l;
    __device__ __forceinline__ uint32_t operator()(uint32_t h, int x, int y) const
    {
        return s_l[h * kPoseHaloCells + (uint32_t)(y + 1) * kPoseHaloX + (uint32_t)(x + 1)];
    }
};

// create, clear and the start of a solve: every state unreached, no tile marked in either mark array; with `all` (create
// and clear) also every layer 0 and the floor unreached with no heading
__global__ __launch_bounds__(kPoseThreads) void k_pose_fill(uint32_t n_cells, uint32_t n_marks, uint32_t all, uint32_t *field, uint32_t *layers,
                                                            uint32_t *floor, uint8_t *floor_heading, uint32_t *marks)
{
    const uint32_t i = blockIdx.x * kPoseThreads + threadIdx.x;
    if (i < n_cells) {
        for (uint32_t h = 0; h < kPoseHeadings; h++) field[(size_t)h * n_cells + i] = kPoseUnreached;
        if (all) {
            for (uint32_t h = 0; h < kPoseHeadings; h++) layers[(size_t)h * n_cells + i] = 0u;
            floor[i] = kPoseUnreached, floor_heading[i] = (uint8_t)kPoseNoHeading;
        }
    }
    if (i < n_marks) marks[i] = 0u;
}

// Step 3, a lane per (cell, heading blockIdx.y): the plane dilated by the heading's stencil.  The heading's stencil -- (dx, dy)
// int16 pairs, a u32 each -- and the 256-entry table sit in LDS; neighbouring lanes are neighbouring cells of a row, so a
// wave reads the plane at neighbouring addresses for every stencil cell.  The plane itself is read in HBM (through L2): a
// stencil reaches up to 91 cells, so the halo of a workgroup's cells does not fit LDS in general, and staging it where it
// would fit was not shown to win (NOT MEASURED), so it is not done.  A lane stops at the first impassable stencil cell.
__global__ __launch_bounds__(kPoseThreads) void k_pose_layers(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table, PoseArgs a,
                                                              const uint32_t *__restrict__ stencil_cells,
                                                              const uint32_t *__restrict__ stencil_first, uint32_t *layers)
{
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_st[kPoseMaxStencil];
    const uint32_t h = blockIdx.y, t = threadIdx.x;
    const uint32_t first = stencil_first[h], n = min(stencil_first[h + 1u] - first, kPoseMaxStencil);
    s_tab[t] = table[t];
    for (uint32_t k = t; k < n; k += kPoseThreads) s_st[k] = stencil_cells[first + k];
    __syncthreads();
    const uint32_t n_cells = a.width * a.height, i = blockIdx.x * kPoseThreads + t;
    if (i >= n_cells) return;
    const int x = (int)(i % a.width), y = (int)(i / a.width);
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
    layers[(size_t)h * n_cells + i] = best;
}

// Step 5, a lane per goal (ix, iy, h) in k_nav_seed's manner: each named passable state becomes 0, the exchange tells the
// first of several equal goal states from the others, and the tiles that read the goal's cell become active for the first
// launch (a goal's 0 is a value no launch of k_pose_relax writes, so no tile would mark its readers).
__global__ __launch_bounds__(kPoseThreads) void k_pose_seed(const uint32_t *__restrict__ layers, PoseArgs a, const int32_t *__restrict__ goals,
                                                            uint32_t n, uint32_t *field, uint32_t *marks0, uint32_t *words)
{
    const uint32_t i = blockIdx.x * kPoseThreads + threadIdx.x;
    const uint32_t n_cells = a.width * a.height;
    uint32_t used = 0u;
    bool rejected = false;
    if (i < n) {
        const int x = goals[3 * (size_t)i], y = goals[3 * (size_t)i + 1], gh = goals[3 * (size_t)i + 2];
        bool any = false;
        if (x >= 0 && y >= 0 && x < (int)a.width && y < (int)a.height && gh >= -1 && gh < (int)kPoseHeadings) {
            const size_t cell = (size_t)y * a.width + (uint32_t)x;
            for (uint32_t h = 0; h < kPoseHeadings; h++) {
                if ((gh >= 0 && (uint32_t)gh != h) || layers[(size_t)h * n_cells + cell] == 0u) continue;
                any = true;
                if (atomicExch(field + (size_t)h * n_cells + cell, 0u) != 0u) used++;
            }
            if (any)
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int nx = x + dx, ny = y + dy;
                        if (nx >= 0 && ny >= 0 && nx < (int)a.width && ny < (int)a.height)
                            marks0[((uint32_t)ny / kPoseTileY) * a.tiles_x + (uint32_t)nx / kPoseTileX] = 1u;
                    }
        }
        rejected = !any;
    }
    const uint32_t n_rejected = pose_count(rejected);
    for (uint32_t o = 32u; o; o >>= 1) used += (uint32_t)__shfl_xor((int)used, (int)o);
    if ((threadIdx.x & 63u) == 0u) {
        if (used) atomicAdd(words + PW_GOALS_USED, used);
        if (n_rejected) atomicAdd(words + PW_GOALS_REJECTED, n_rejected);
    }
}

// Step 6, one launch of the relaxation: k_nav_relax's scheme (k_navfield.hpp) extended by the heading.  A workgroup owns
// the tile (blockIdx.x, blockIdx.y) with all eight headings; lane t owns the cell (t & 31, t >> 5) of it and keeps its eight
// states in registers: the layer value, the allowed moves (a bit per move) and the value at the load and now.  P and L of
// the tile sit in LDS, heading-major with a one-cell halo: a 32-lane half reads 32 consecutive words of one heading for any
// move, so no two of its lanes share a bank, and the eight headings of a cell lie 340 words apart, on eight different
// banks.  L is only read for the move masks; the sweeps read P alone.
//
// Why any schedule gives the same bytes.  Every move of a state (a, h) ends in a state of cell a or of one of its eight
// neighbour cells, so a tile reads nothing beyond its one-cell halo, and the navigation field's argument carries over with
// "state" for "cell".  Every value a state ever holds is 0 on a goal state or P[target] + weight for a value some target of
// one of its allowed moves held: by induction the weight of a real move sequence, so never below the true P, and a state's
// value only falls.  Hence a value that is read late or stale -- in LDS while another lane rewrites it in the same sweep, or
// a halo state that the neighbour tile rewrites in HBM during the same launch (a 32-bit word is read whole) -- is still an
// upper bound and does no harm, provided the reader runs again once the newer value is there: inside a tile the sweeps go on
// until one changes nothing, and across tiles a tile that lowered any heading of a border cell marks every neighbour tile
// that reads that cell for the next launch, whose start is behind this launch's end.  No mark is lost: marks for launch
// k + 1 go to the array that launch k does not read, and a tile clears only its own word, in the array it reads, after all
// its lanes have read it.  When a launch marks nothing, every tile's last load saw the final values of its halo and its
// last sweep changed nothing: no allowed move lowers any state, every value is the weight of a real move sequence, and with
// positive weights that state is unique -- the field of step 6.  Launches after it change nothing, so the host may run
// ahead.
//
// inner_cap bounds the sweeps of a launch; a tile that stops there marks itself.  all_tiles (a test switch) runs every tile
// in every launch.  *flag is set iff the launch marked a tile.
__global__ __launch_bounds__(kPoseThreads) void k_pose_relax(const uint32_t *__restrict__ layers, PoseArgs a, PoseCosts pc, uint32_t inner_cap,
                                                             uint32_t all_tiles, uint32_t *field, uint32_t *marks_cur, uint32_t *marks_nxt,
                                                             uint32_t *flag)
{
    __shared__ uint32_t s_p[kPoseHeadings * kPoseHaloCells];  // the potentials, with the halo
    __shared__ uint32_t s_l[kPoseHeadings * kPoseHaloCells];  // the layers, 0 = impassable or outside the grid
    __shared__ uint32_t s_nb;                                 // the neighbour tiles to mark, a bit per direction
    __shared__ uint32_t s_more[3];                            // "a state fell in sweep i" at i % 3

    const uint32_t tile = blockIdx.y * a.tiles_x + blockIdx.x;
    if ((all_tiles | marks_cur[tile]) == 0u) return;  // (the same word for every lane: the whole workgroup leaves)
    const uint32_t t = threadIdx.x;
    if (t == 0u) s_nb = s_more[0] = s_more[1] = s_more[2] = 0u;
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

    // the sweeps, in place: P[state] = min(P[state], min over allowed moves of P[target] + weight), candidates above
    // LOM_NAV_MAX dropped.  Sweep i raises s_more[i % 3] in front of its barrier and reads it behind; lane 0 then lowers the
    // word of sweep i + 2, which sweep i - 1 read last (every lane is past barrier i) and sweep i + 2 writes next.
    uint32_t sweeps = 0u, more;
    do {
        bool changed = false;
#pragma unroll
        for (uint32_t h = 0; h < kPoseHeadings; h++) {
            if (!moves[h]) continue;
            uint32_t best = cur[h];
#pragma unroll
            for (uint32_t k = 0; k < kPoseMoves; k++) {
                if (!(moves[h] >> k & 1u)) continue;
                const int o = pose_move_sign(k) * (pose_hy(h) * (int)kPoseHaloX + pose_hx(h));
                const uint32_t pb = s_p[pose_move_heading(h, k) * kPoseHaloCells + (uint32_t)((int)li + o)];
                const uint32_t w = pose_move_weight(pc, h, s[h], k);  // < 2^28
                if (pb <= kPoseMax - w) best = min(best, pb + w);     // (unreached is above kPoseMax - w)
            }
            if (best < cur[h]) {
                cur[h] = best;
                s_p[h * kPoseHaloCells + li] = best;
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

    // the states that fell go back; a border cell of which any heading fell names the neighbour tiles that read it
    bool fell = false;
    const size_t cell = (size_t)(blockIdx.y * kPoseTileY + (uint32_t)y) * a.width + blockIdx.x * kPoseTileX + (uint32_t)x;
#pragma unroll
    for (uint32_t h = 0; h < kPoseHeadings; h++) {
        if (cur[h] >= first[h]) continue;  // (a cell of a cut tile that lies outside the grid never falls: its layers are 0)
        field[(size_t)h * n_cells + cell] = cur[h];
        fell = true;
    }
    if (fell) {
        const bool e = x == (int)kPoseTileX - 1, n = y == (int)kPoseTileY - 1, w = x == 0, so = y == 0;
        // a bit per direction in the order of the headings: E, NE, N, NW, W, SW, S, SE
        const uint32_t nb = (e ? 1u : 0u) | (e && n ? 2u : 0u) | (n ? 4u : 0u) | (w && n ? 8u : 0u) | (w ? 16u : 0u) | (w && so ? 32u : 0u) |
                            (so ? 64u : 0u) | (e && so ? 128u : 0u);
        if (nb) atomicOr(&s_nb, nb);
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
}

// Whether some allowed move a -> (bx, by, any heading) has P[target] + weight above LOM_NAV_MAX: the sources of such a move
// lie in the cell and its eight neighbours.  Only called for the few cells that hold a value within a move of LOM_NAV_MAX.
__device__ __forceinline__ bool pose_range_exceeded_at(const uint32_t *__restrict__ layers, const uint32_t *__restrict__ field, PoseArgs a, PoseCosts pc,
                                                    int bx, int by)
{
    const PoseLayerCells L{layers, a.width, a.height};
    const uint32_t n_cells = a.width * a.height;
    const size_t b = (size_t)by * a.width + (uint32_t)bx;
    for (int ay = by - 1; ay <= by + 1; ay++)
        for (int ax = bx - 1; ax <= bx + 1; ax++)
            for (uint32_t h = 0; h < kPoseHeadings; h++) {
                const uint32_t s = L(h, ax, ay);
                if (!s) continue;
                for (uint32_t m = 0; m < kPoseMoves; m++) {
                    int tx, ty;
                    uint32_t th, w;
                    if (!pose_move(L, pc, ax, ay, h, s, m, &tx, &ty, &th, &w) || tx != bx || ty != by) continue;
                    const uint32_t p = field[(size_t)th * n_cells + b];
                    if (p != kPoseUnreached && p > kPoseMax - w) return true;
                }
            }
    return false;
}

// Steps 7 and 8 and range_exceeded, at the fixed point: at most 64 workgroups stride over the cells, a lane per cell with
// its eight states.  The counts of a wave come from ballots and gather in wave-uniform registers over the whole stride; a
// wave issues its atomics once, at its end.
__global__ __launch_bounds__(kPoseThreads) void k_pose_report(const int8_t *__restrict__ plane, const uint32_t *__restrict__ layers,
                                                              const uint32_t *__restrict__ field, PoseArgs a, PoseCosts pc, uint32_t *floor,
                                                              uint8_t *floor_heading, uint32_t *words)
{
    const uint32_t n_cells = a.width * a.height;
    uint32_t n_blocked = 0u, n_reached = 0u, n_unreached = 0u, n_cells_reached = 0u, n_invalid = 0u, pmax = 0u;
    bool exceeded = false;
    // (the bound is the same for every lane of a wave: every lane takes part in every ballot)
    for (uint32_t base = blockIdx.x * kPoseThreads; base < n_cells; base += gridDim.x * kPoseThreads) {
        const uint32_t i = base + threadIdx.x;
        const bool have = i < n_cells;
        uint32_t fl = kPoseUnreached, fh = kPoseNoHeading;
        bool near_max = false;
        for (uint32_t h = 0; h < kPoseHeadings; h++) {
            uint32_t l = 1u, p = kPoseUnreached;
            if (have) l = layers[(size_t)h * n_cells + i], p = field[(size_t)h * n_cells + i];
            const bool reached = p != kPoseUnreached;
            n_blocked += pose_count(l == 0u);
            n_reached += pose_count(reached);
            n_unreached += pose_count(have && l != 0u && !reached);
            if (reached) {
                pmax = max(pmax, p);
                if (p < fl) fl = p, fh = h;
                near_max = near_max || p > kPoseMax - kPoseMaxWeight;  // none can exceed while P + the heaviest move fits
            }
        }
        bool invalid = false;
        if (have) {
            const int b = plane[i];
            invalid = b < -1 || b > 100;
            floor[i] = fl, floor_heading[i] = (uint8_t)fh;
        }
        n_cells_reached += pose_count(fl != kPoseUnreached);
        n_invalid += pose_count(invalid);
        if (near_max) exceeded = exceeded || pose_range_exceeded_at(layers, field, a, pc, (int)(i % a.width), (int)(i / a.width));
    }
    const bool any_exceeded = __ballot(exceeded) != 0ull;
    for (uint32_t o = 32u; o; o >>= 1) pmax = max(pmax, (uint32_t)__shfl_xor((int)pmax, (int)o));
    if ((threadIdx.x & 63u) == 0u) {
        if (n_blocked) atomicAdd(words + PW_BLOCKED, n_blocked);
        if (n_reached) atomicAdd(words + PW_REACHED, n_reached);
        if (n_unreached) atomicAdd(words + PW_UNREACHED, n_unreached);
        if (n_cells_reached) atomicAdd(words + PW_CELLS_REACHED, n_cells_reached);
        if (n_invalid) atomicAdd(words + PW_INVALID, n_invalid);
        if (any_exceeded) atomicOr(words + PW_RANGE, 1u);
        if (pmax) atomicMax(words + PW_MAX_POTENTIAL, pmax);
    }
}

// Step 9, a lane per start (ix, iy, h): the serial walk down the field.  From a state with P > 0 the first move in the
// fixed order that is allowed and has P[target] + weight == P[state]; at the fixed point one exists, and P falls strictly, so
// the walk ends within 8 * cells states.  out: [K, cap] u16 triples; lengths[k]: the full length, 0 for a start that is not
// walked.
__global__ __launch_bounds__(kPoseThreads) void k_pose_trace(const uint32_t *__restrict__ layers, const uint32_t *__restrict__ field,
                                                             const uint8_t *__restrict__ floor_heading, PoseArgs a, PoseCosts pc,
                                                             const int32_t *__restrict__ starts, uint32_t K, uint32_t cap, uint16_t *out,
                                                             uint32_t *lengths)
{
    const uint32_t k = blockIdx.x * kPoseThreads + threadIdx.x;
    if (k >= K) return;
    const PoseLayerCells L{layers, a.width, a.height};
    const uint32_t n_cells = a.width * a.height;
    int x = starts[3 * (size_t)k], y = starts[3 * (size_t)k + 1];
    const int sh = starts[3 * (size_t)k + 2];
    uint16_t *const row = out + (size_t)k * cap * 3u;
    uint32_t len = 0u;
    if (x >= 0 && y >= 0 && x < (int)a.width && y < (int)a.height && sh >= -1 && sh < (int)kPoseHeadings) {
        uint32_t h = sh < 0 ? floor_heading[(size_t)y * a.width + (uint32_t)x] : (uint32_t)sh;
        uint32_t p = h < kPoseHeadings ? field[(size_t)h * n_cells + (size_t)y * a.width + (uint32_t)x] : kPoseUnreached;
        while (p != kPoseUnreached) {
            if (len < cap) {
                uint16_t *const o = row + (size_t)len * 3u;
                o[0] = (uint16_t)x, o[1] = (uint16_t)y, o[2] = (uint16_t)h;
            }
            len++;
            if (p == 0u || len >= kPoseHeadings * n_cells) break;
            const uint32_t s = L(h, x, y);
            uint32_t next = kPoseUnreached;
            for (uint32_t m = 0; m < kPoseMoves && s; m++) {
                int tx, ty;
                uint32_t th, w;
                if (!pose_move(L, pc, x, y, h, s, m, &tx, &ty, &th, &w)) continue;
                const uint32_t pb = field[(size_t)th * n_cells + (size_t)ty * a.width + (uint32_t)tx];
                if (pb <= kPoseMax - w && pb + w == p) {
                    x = tx, y = ty, h = th, next = pb;
                    break;
                }
            }
            p = next;  // (unreached: no move fits -- never at the fixed point; the walk ends)
        }
    }
    lengths[k] = len;
}

// Step 10, a lane per point: the cell by the floor rule (f64 from the f32 values, compared before any conversion) and P of
// the named state, the floor for heading -1; unreached outside the grid (a NaN coordinate fails both comparisons) and for
// any other heading.
__global__ __launch_bounds__(kPoseThreads) void k_pose_query(const float *__restrict__ xy, const int32_t *__restrict__ headings, uint32_t n,
                                                             float resolution, float origin_x, float origin_y, PoseArgs a,
                                                             const uint32_t *__restrict__ field, const uint32_t *__restrict__ floor, uint32_t *out)
{
    const uint32_t i = blockIdx.x * kPoseThreads + threadIdx.x;
    if (i >= n) return;
    const double r = (double)resolution;
    const double qx = __builtin_floor(((double)xy[2 * (size_t)i] - (double)origin_x) / r);
    const double qy = __builtin_floor(((double)xy[2 * (size_t)i + 1] - (double)origin_y) / r);
    const int h = headings[i];
    uint32_t p = kPoseUnreached;
    if (qx >= 0.0 && qx < (double)a.width && qy >= 0.0 && qy < (double)a.height && h >= -1 && h < (int)kPoseHeadings) {
        const size_t cell = (size_t)(uint32_t)qy * a.width + (uint32_t)qx;
        p = h < 0 ? floor[cell] : field[(size_t)h * (a.width * a.height) + cell];
    }
    out[i] = p;
}

}  // namespace lom
