// Clearance grid (include/lidar_odometry_amd.h, "clearance grid"): k_clear_merge, k_clear_distance, k_clear_query,
// k_clear_count and k_clear_fill.  Device code only; clearance.hip is the one translation unit that instantiates and
// launches it.
//
// The obstacles of a row live in a bitmap, one u64 per 64 cells, written by one wave ballot per word.  k_clear_distance
// never sees a plane of row distances: a workgroup owns a tile of 64 columns (one bitmap word) by T rows, derives the row
// distance g of its T + 2R rows straight from the bitmap words -- the nearest set bit to the left and to the right by
// count-leading / trailing-zeros -- into LDS as bytes, and takes the column minimum of g^2 + dy^2 from there.  No
// workgroup waits for another; integer atomics only; no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lom {

constexpr uint32_t kClearThreads = 256;  // four waves
constexpr uint32_t kClearFar = 65535u;   // LOM_CLEAR_FAR

// the summary words of a call (zeroed per call; u32: a grid has at most 2^26 cells)
enum { CW_LETHAL = 0, CW_INSCRIBED = 1, CW_COSTED = 2, CW_UNKNOWN = 3, CW_INVALID = 4, CW_CLEARED = 5, CW_COUNT = 6 };

struct ClearArgs {
    uint32_t width, height, wpr;  // wpr: u64 words of a bitmap row
    uint32_t x0, y0, x1, y1;      // the rectangle of the update, clipped
    uint32_t R, flags;
    uint32_t tile_rows, no_prune;
};

// the wave's index in its workgroup, as a value the compiler knows to be uniform
__device__ __forceinline__ uint32_t clear_wave() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

__device__ __forceinline__ uint32_t clear_count(bool v) { return (uint32_t)__popcll(__ballot(v)); }

// Step 1, a wave per bitmap word: words [wx0, wx0 + n_wx) of rows [gy0, gy0 + n_rows), the grown rectangle widened to
// whole words.  A lane per cell: the base byte, and the obstacle bit through the wave's ballot (a lane beyond the
// grid's width votes 0, so the bits past the last column stay clear).  invalid / cleared count inside the rectangle only.
__global__ __launch_bounds__(kClearThreads) void k_clear_merge(const int8_t *__restrict__ occ, const int8_t *__restrict__ elev,
                                                               ClearArgs a, uint32_t wx0, uint32_t n_wx, uint32_t gy0,
                                                               uint32_t n_rows, int8_t *base, unsigned long long *bitmap,
                                                               uint32_t *words)
{
    const uint32_t wave = blockIdx.x * (kClearThreads / 64u) + clear_wave(), lane = threadIdx.x & 63u;
    const bool live = wave < n_wx * n_rows;  // (uniform)
    const uint32_t row = wave / n_wx, word = wx0 + (wave - row * n_wx);
    const uint32_t x = word * 64u + lane, y = gy0 + row;
    bool obstacle = false, invalid = false, cleared = false;
    if (live && x < a.width) {
        const size_t c = (size_t)y * a.width + x;
        int o = occ ? (int)occ[c] : -1, e = elev ? (int)elev[c] : -1;
        const bool bad_o = !(o == -1 || o == 0 || o == 100), bad_e = e < -1 || e > 100;
        if (bad_o) o = -1;
        if (bad_e) e = -1;
        const bool clr = e == 100 && (a.flags & LOM_CLEAR_FREE_CLEARS_ELEVATION) && o == 0;
        if (clr) e = 0;
        const int b = (o == 100 || e == 100) ? 100 : (e >= 0 ? e : (o == 0 ? 0 : -1));
        base[c] = (int8_t)b;
        obstacle = b == 100 || (b == -1 && (a.flags & LOM_CLEAR_UNKNOWN_IS_OBSTACLE));
        const bool in_rect = x >= a.x0 && x < a.x1 && y >= a.y0 && y < a.y1;
        invalid = in_rect && (bad_o || bad_e);
        cleared = in_rect && clr;
    }
    const unsigned long long bits = __ballot(obstacle);
    const uint32_t n_invalid = clear_count(invalid), n_cleared = clear_count(cleared);
    if (live && lane == 0u) {
        bitmap[(size_t)y * a.wpr + word] = bits;
        if (n_invalid) atomicAdd(words + CW_INVALID, n_invalid);
        if (n_cleared) atomicAdd(words + CW_CLEARED, n_cleared);
    }
}

// Steps 2 and 4 for the tile (blockIdx.x: the word column wx0 + blockIdx.x; blockIdx.y: rows y0 + blockIdx.y * T, cut at
// y1).  g[s][lane], s < rows + 2R: the distance along row ty0 - R + s from column `lane` of the word to the nearest
// obstacle of that row, clipped to R + 1; R + 1 for a row outside the grid.  A wave stages whole rows, so the bitmap words
// it reads are the same for all its lanes.
__global__ __launch_bounds__(kClearThreads) void k_clear_distance(const unsigned long long *__restrict__ bitmap,
                                                                  const int8_t *__restrict__ base,
                                                                  const uint8_t *__restrict__ table, ClearArgs a, uint32_t wx0,
                                                                  uint16_t *d2_out, int8_t *cost_out, uint32_t *words)
{
    extern __shared__ uint8_t g[];
    const uint32_t wave = clear_wave(), lane = threadIdx.x & 63u;
    const uint32_t word = wx0 + blockIdx.x;
    const uint32_t ty0 = a.y0 + blockIdx.y * a.tile_rows;
    const uint32_t rows = min(a.tile_rows, a.y1 - ty0);
    const uint32_t R = a.R, S = rows + 2u * R, far_g = R + 1u;
    const uint32_t kmax = (R + 63u) / 64u;  // words to look at on either side: a bit further away is beyond R for every lane
    for (uint32_t s = wave; s < S; s += kClearThreads / 64u) {
        const int y = (int)ty0 - (int)R + (int)s;
        uint32_t gv = far_g;
        if (y >= 0 && y < (int)a.height) {
            const unsigned long long *const rowp = bitmap + (size_t)y * a.wpr;
            const unsigned long long w0 = rowp[word];
            // the first non-zero word on either side and how many words away it is (uniform)
            unsigned long long vl = 0ull, vr = 0ull;
            uint32_t kl = 0u, kr = 0u;
            for (uint32_t k = 1; k <= kmax && k <= word; k++) {
                vl = rowp[word - k];
                if (vl) {
                    kl = k;
                    break;
                }
            }
            for (uint32_t k = 1; k <= kmax && word + k < a.wpr; k++) {
                vr = rowp[word + k];
                if (vr) {
                    kr = k;
                    break;
                }
            }
            uint32_t dl = far_g, dr = far_g;
            const unsigned long long left = w0 & (~0ull >> (63u - lane));  // bits at or below the lane
            if (left)
                dl = lane - (63u - (uint32_t)__clzll((long long)left));
            else if (vl)
                dl = lane + 64u * kl - (63u - (uint32_t)__clzll((long long)vl));
            const unsigned long long right = w0 >> lane;  // bits at or above the lane
            if (right)
                dr = (uint32_t)__ffsll((long long)right) - 1u;
            else if (vr)
                dr = 64u * kr - lane + (uint32_t)__ffsll((long long)vr) - 1u;
            gv = min(min(dl, dr), far_g);
        }
        g[s * 64u + lane] = (uint8_t)gv;
    }
    __syncthreads();

    const uint32_t x = word * 64u + lane;
    const bool in_cols = x >= a.x0 && x < a.x1;
    uint32_t n_lethal = 0u, n_inscribed = 0u, n_costed = 0u, n_unknown = 0u;
    for (uint32_t r = wave; r < rows; r += kClearThreads / 64u) {
        int cost = 0;
        if (in_cols) {
            const uint32_t ly = r + R;
            uint32_t best = g[ly * 64u + lane];
            best *= best;
            // outward from the cell's own row; once dy^2 reaches the best so far no further row can improve it
            for (uint32_t dy = 1; dy <= R && (a.no_prune || dy * dy < best); dy++) {
                const uint32_t up = g[(ly - dy) * 64u + lane], down = g[(ly + dy) * 64u + lane];
                const uint32_t m = min(up, down);
                best = min(best, m * m + dy * dy);
            }
            const uint32_t d2 = best <= R * R ? best : kClearFar;
            const size_t c = (size_t)(ty0 + r) * a.width + x;
            const int b = base[c];
            const int t = d2 == kClearFar ? 0 : (int)table[d2];
            cost = d2 == 0u ? 100 : (b >= 0 ? max(b, t) : (t > 0 ? t : -1));
            d2_out[c] = (uint16_t)d2;
            cost_out[c] = (int8_t)cost;
        }
        n_lethal += clear_count(in_cols && cost == 100);
        n_inscribed += clear_count(in_cols && cost == 99);
        n_costed += clear_count(in_cols && cost >= 0 && cost < 99);
        n_unknown += clear_count(in_cols && cost < 0);
    }
    // the totals: summed over the wave by the ballots above, one atomic each per wave
    if (lane == 0u) {
        if (n_lethal) atomicAdd(words + CW_LETHAL, n_lethal);
        if (n_inscribed) atomicAdd(words + CW_INSCRIBED, n_inscribed);
        if (n_costed) atomicAdd(words + CW_COSTED, n_costed);
        if (n_unknown) atomicAdd(words + CW_UNKNOWN, n_unknown);
    }
}

// A lane per query point: the cell by the floor rule (f64 from the f32 values, compared before any conversion), step 5
// and the cost; NaN and -1 outside the grid (a NaN coordinate fails both comparisons).
__global__ __launch_bounds__(kClearThreads) void k_clear_query(const float *__restrict__ xy, uint32_t n, float resolution,
                                                               float origin_x, float origin_y, uint32_t width, uint32_t height,
                                                               const uint16_t *__restrict__ d2, const int8_t *__restrict__ cost,
                                                               float *dist_out, int8_t *cost_out)
{
    const uint32_t i = blockIdx.x * kClearThreads + threadIdx.x;
    if (i >= n) return;
    const double r = (double)resolution;
    const double qx = __builtin_floor(((double)xy[2 * (size_t)i] - (double)origin_x) / r);
    const double qy = __builtin_floor(((double)xy[2 * (size_t)i + 1] - (double)origin_y) / r);
    float dist = __builtin_nanf("");
    int8_t c = -1;
    if (qx >= 0.0 && qx < (double)width && qy >= 0.0 && qy < (double)height) {
        const size_t cell = (size_t)(uint32_t)qy * width + (uint32_t)qx;
        const uint32_t v = d2[cell];
        dist = v == kClearFar ? __builtin_inff() : (float)(__dsqrt_rn((double)v) * r);
        c = cost[cell];
    }
    if (dist_out) dist_out[i] = dist;
    if (cost_out) cost_out[i] = c;
}

// the four cost totals of the plane as it stands (lom_clearance_cost)
__global__ __launch_bounds__(kClearThreads) void k_clear_count(const int8_t *__restrict__ cost, uint32_t n_cells, uint32_t *words)
{
    const uint32_t i = blockIdx.x * kClearThreads + threadIdx.x;
    const bool have = i < n_cells;
    const int c = have ? (int)cost[i] : 0;
    const uint32_t n_lethal = clear_count(have && c == 100), n_inscribed = clear_count(have && c == 99),
                   n_costed = clear_count(have && c >= 0 && c < 99), n_unknown = clear_count(have && c < 0);
    if ((threadIdx.x & 63u) == 0u) {
        if (n_lethal) atomicAdd(words + CW_LETHAL, n_lethal);
        if (n_inscribed) atomicAdd(words + CW_INSCRIBED, n_inscribed);
        if (n_costed) atomicAdd(words + CW_COSTED, n_costed);
        if (n_unknown) atomicAdd(words + CW_UNKNOWN, n_unknown);
    }
}

// create and clear: base = -1, d2 = far, cost = -1, no obstacle bit
__global__ __launch_bounds__(kClearThreads) void k_clear_fill(uint32_t n_cells, uint32_t n_words, int8_t *base, uint16_t *d2,
                                                              int8_t *cost, unsigned long long *bitmap)
{
    const uint32_t i = blockIdx.x * kClearThreads + threadIdx.x;
    if (i < n_cells) {
        base[i] = (int8_t)-1;
        d2[i] = (uint16_t)kClearFar;
        cost[i] = (int8_t)-1;
    }
    if (i < n_words) bitmap[i] = 0ull;
}

}  // namespace lom
