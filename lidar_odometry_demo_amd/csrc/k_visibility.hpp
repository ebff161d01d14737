// Visibility grid (include/lidar_odometry_amd.h, "visibility grid"): k_vis_cast, k_vis_summary, k_vis_costs, k_vis_fill,
// k_vis_marginal, k_vis_pick and k_vis_cover.  Device code only; visibility.hip is the one translation unit that
// instantiates and launches it.  Integers throughout; plain vector stores and vector atomics only; no workgroup ever waits
// for another: what one launch needs from all workgroups of another is a launch of its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lom {

constexpr uint32_t kVisThreads = 256;          // four waves: every kernel but k_vis_cast, which runs one or four
constexpr uint32_t kVisRedWords = 32;          // the head of k_vis_cast's dynamic LDS: the workgroup's partial sums
constexpr uint32_t kVisUnreached = 0xFFFFFFFFu;
constexpr uint32_t kVisIndexBits = 20;         // a viewpoint's index
constexpr unsigned long long kVisIndexMask = (1ull << kVisIndexBits) - 1ull;
// why a beam ended (LOM_VIS_END_*)
enum { VIS_INVALID = 0, VIS_EDGE = 1, VIS_RANGE = 2, VIS_HIT = 3, VIS_UNKNOWN = 4, VIS_CORNER = 5 };
// the summary words of a cast (zeroed per cast), u64 each
enum { VW_VALID = 0, VW_UNKNOWN = 1, VW_KEY = 2, VW_COUNT = 4 };

struct VisArgs {
    uint32_t width, height;
    uint32_t beams, range, depth;
    int32_t block_min;
    uint32_t win_wpr, win_words;     // a window: 2 range + 1 rows of win_wpr words
    uint32_t keep_windows, keep_beams;
    uint32_t cov_wpr;                // the covered bitmap: u32 words per grid row
};

// the record as the header lays it out (lom_visibility_record)
struct VisRecord {
    int32_t ix, iy;
    uint32_t valid, seen, unknown, free_cells, blocked, hits;
};
static_assert(sizeof(VisRecord) == 32, "VisRecord is 32 bytes");

// an entry of a selection (lom_visibility_pick)
struct VisPick {
    uint32_t k, gain;
    long long score;
};
static_assert(sizeof(VisPick) == 16, "VisPick is 16 bytes");

__device__ __forceinline__ uint32_t vis_wave_sum(uint32_t v)
{
    for (uint32_t o = 32u; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, (int)o);
    return v;
}

__device__ __forceinline__ unsigned long long vis_wave_max(unsigned long long v)
{
    for (uint32_t o = 32u; o; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, (int)o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)o);
        const unsigned long long u = ((unsigned long long)hi << 32) | lo;
        v = u > v ? u : v;
    }
    return v;
}

// a cell inside the grid whose byte is at least block_min
__device__ __forceinline__ bool vis_blocks(const int8_t *plane, const VisArgs &a, int x, int y)
{
    return (uint32_t)x < a.width && (uint32_t)y < a.height && (int)plane[(size_t)y * a.width + (uint32_t)x] >= a.block_min;
}

// Sets `bit` of a window word: a plain look first, the atomic only where the bit is missing (most cells near the start
// are marked by many beams).  The window in HBM (LOM_VIS_OPT_TEST_NO_LDS) is looked at past this CU's L1, which the
// other waves' atomics do not refresh; a stale look would only cost a redundant atomic.
template <bool kLds>
__device__ __forceinline__ void vis_mark(uint32_t *word, uint32_t bit)
{
    if (kLds) {
        if ((*word & bit) == 0u) atomicOr(word, bit);  // (result unused: ds_or_b32)
    } else {
        if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) == 0u) atomicOr(word, bit);
    }
}

// Steps 2 to 6 for one viewpoint per workgroup, lanes over beams.  The seen bits of the disc go to a window of 2R + 1 rows
// around the start cell -- in LDS (kLds), or straight in the viewpoint's window in HBM, zeroed by the host -- and behind one
// barrier the workgroup sweeps the window word by word: the plane bytes under a word's bits are read once, classed into
// an unknown and a blocking mask, and the popcounts summed over the wave, then over the workgroup, into the record.
// Why any schedule gives the same bytes: bits are only ever set, and the set of bits set is the union over the beams,
// whatever the order; a beam reads nothing another beam writes (the plane is constant, the window is only written before
// the barrier and only read behind it); popcounts and integer sums do not depend on order; every record, beam word and
// window word is written by exactly one lane.
template <bool kLds>
__global__ __launch_bounds__(kVisThreads) void k_vis_cast(const int8_t *__restrict__ plane, const int32_t *__restrict__ table,
                                                          const int32_t *__restrict__ viewpoints, VisArgs a, VisRecord *records,
                                                          uint32_t *beams, uint32_t *windows)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t vis_lds[];
    uint32_t *const red = vis_lds, *const lwin = vis_lds + kVisRedWords;
    const uint32_t k = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
    const int x0 = viewpoints[2 * (size_t)k], y0 = viewpoints[2 * (size_t)k + 1];
    const int R = (int)a.range;
    uint32_t *const gwin = windows ? windows + (size_t)k * a.win_words : nullptr;
    uint32_t *const gbeams = a.keep_beams ? beams + (size_t)k * a.beams : nullptr;
    const bool valid = (uint32_t)x0 < a.width && (uint32_t)y0 < a.height && (int)plane[(size_t)y0 * a.width + (uint32_t)x0] < a.block_min;
    if (!valid) {  // uniform over the workgroup, before any barrier
        if (t == 0u) records[k] = VisRecord{x0, y0, 0u, 0u, 0u, 0u, 0u, 0u};
        if (gbeams)
            for (uint32_t b = t; b < a.beams; b += nt) gbeams[b] = (uint32_t)VIS_INVALID << 24;
        if (kLds && a.keep_windows)
            for (uint32_t w = t; w < a.win_words; w += nt) gwin[w] = 0u;
        return;
    }
    // the start cell is seen once; it sits at (R, R) of the window
    const uint32_t start_word = (uint32_t)R * a.win_wpr + ((uint32_t)R >> 5), start_bit = 1u << ((uint32_t)R & 31u);
    if (kLds) {
        for (uint32_t w = t; w < a.win_words; w += nt) lwin[w] = w == start_word ? start_bit : 0u;
    } else if (t == 0u) {
        atomicOr(gwin + start_word, start_bit);
    }
    __syncthreads();

    const uint32_t R2 = a.range * a.range;
    uint32_t hits = 0u;
    for (uint32_t b = t; b < a.beams; b += nt) {
        const int dx = table[2 * b], dy = table[2 * b + 1];
        const uint32_t ax = (uint32_t)(dx < 0 ? -dx : dx), ay = (uint32_t)(dy < 0 ? -dy : dy);
        const int sx = (dx > 0) - (dx < 0), sy = (dy > 0) - (dy < 0);
        uint32_t i = 0u, j = 0u, unknown = 0u, reason = VIS_RANGE;
        int x = x0, y = y0;
        // every step raises i or j, so ni^2 + nj^2 > R^2 ends the walk within 2R + 2 steps
        for (uint32_t n = 0u; n < 2u * a.range + 2u; n++) {
            const uint32_t lhs = (2u * i + 1u) * ay, rhs = (2u * j + 1u) * ax;  // below 2^24 each
            uint32_t ni = i, nj = j;
            int nx = x, ny = y;
            if (lhs <= rhs) ni++, nx += sx;
            if (lhs >= rhs) nj++, ny += sy;
            if (lhs == rhs && vis_blocks(plane, a, x + sx, y) && vis_blocks(plane, a, x, y + sy)) {
                reason = VIS_CORNER;
                break;
            }
            if ((uint32_t)nx >= a.width || (uint32_t)ny >= a.height) {
                reason = VIS_EDGE;
                break;
            }
            if (ni * ni + nj * nj > R2) {
                reason = VIS_RANGE;
                break;
            }
            const uint32_t wx = (uint32_t)(nx - x0 + R), wy = (uint32_t)(ny - y0 + R);  // 0 .. 2R each: in range
            vis_mark<kLds>((kLds ? lwin : gwin) + wy * a.win_wpr + (wx >> 5), 1u << (wx & 31u));
            i = ni, j = nj, x = nx, y = ny;
            const int v = (int)plane[(size_t)ny * a.width + (uint32_t)nx];
            if (v >= a.block_min) {
                reason = VIS_HIT;
                hits++;
                break;
            }
            if (v < 0 && ++unknown == a.depth) {  // depth 0: never equal, unknown >= 1 here
                reason = VIS_UNKNOWN;
                break;
            }
        }
        if (gbeams) gbeams[b] = (i * i + j * j) | (reason << 24);
    }
    __syncthreads();

    uint32_t seen = 0u, n_unknown = 0u, n_blocked = 0u;
    for (uint32_t w = t; w < a.win_words; w += nt) {
        const uint32_t bits = kLds ? lwin[w] : __hip_atomic_load(gwin + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t unk = 0u, blk = 0u;
        if (bits) {  // a set bit is a cell of the grid, so the row is one
            const uint32_t row = w / a.win_wpr, word = w - row * a.win_wpr;
            const int8_t *const cells = plane + (size_t)(y0 - R + (int)row) * a.width + (x0 - R + 32 * (int)word);
            for (uint32_t m = bits; m; m &= m - 1u) {
                const uint32_t c = (uint32_t)__ffs((int)m) - 1u;
                const int v = (int)cells[c];
                unk |= (v < 0 ? 1u : 0u) << c;
                blk |= (v >= a.block_min ? 1u : 0u) << c;
            }
        }
        seen += (uint32_t)__popc(bits), n_unknown += (uint32_t)__popc(unk), n_blocked += (uint32_t)__popc(blk);
        if (a.keep_windows) gwin[w] = unk;  // seen & unknown
    }
    seen = vis_wave_sum(seen), n_unknown = vis_wave_sum(n_unknown), n_blocked = vis_wave_sum(n_blocked), hits = vis_wave_sum(hits);
    if ((t & 63u) == 0u) {
        uint32_t *const r = red + 4u * (t >> 6);
        r[0] = seen, r[1] = n_unknown, r[2] = n_blocked, r[3] = hits;
    }
    __syncthreads();
    if (t == 0u) {
        for (uint32_t wave = 1u; wave < (nt >> 6); wave++)
            seen += red[4u * wave], n_unknown += red[4u * wave + 1u], n_blocked += red[4u * wave + 2u], hits += red[4u * wave + 3u];
        records[k] = VisRecord{x0, y0, 1u, seen, n_unknown, seen - n_unknown - n_blocked, n_blocked, hits};
    }
}

// Step 7 over the records: the valid viewpoints, the sum of their unknown counts, and the greatest count with the least
// index that has it as one unsigned maximum of ((unknown + 1) << 20) | (2^20 - 1 - k).  Sums and a maximum: no order.
__global__ __launch_bounds__(kVisThreads) void k_vis_summary(const VisRecord *records, uint32_t n, unsigned long long *words)
{
    const uint32_t k = blockIdx.x * kVisThreads + threadIdx.x;
    uint32_t valid = 0u, unknown = 0u;
    unsigned long long key = 0ull;
    if (k < n && records[k].valid) {
        valid = 1u, unknown = records[k].unknown;
        key = ((unsigned long long)(unknown + 1u) << kVisIndexBits) | (kVisIndexMask - k);
    }
    valid = vis_wave_sum(valid), unknown = vis_wave_sum(unknown), key = vis_wave_max(key);
    if ((threadIdx.x & 63u) == 0u && valid) {
        atomicAdd(words + VW_VALID, (unsigned long long)valid);
        atomicAdd(words + VW_UNKNOWN, (unsigned long long)unknown);
        atomicMax(words + VW_KEY, key);
    }
}

// the travel costs of a selection read from a navigation field's potential at the viewpoints' cells
__global__ __launch_bounds__(kVisThreads) void k_vis_costs(const int32_t *viewpoints, uint32_t n, uint32_t width, uint32_t height,
                                                           const uint32_t *potential, uint32_t *cost)
{
    const uint32_t k = blockIdx.x * kVisThreads + threadIdx.x;
    if (k >= n) return;
    const int x = viewpoints[2 * (size_t)k], y = viewpoints[2 * (size_t)k + 1];
    cost[k] = (uint32_t)x < width && (uint32_t)y < height ? potential[(size_t)y * width + (uint32_t)x] : kVisUnreached;
}

// the covered bitmap and the picked flags of a new selection
__global__ __launch_bounds__(kVisThreads) void k_vis_fill(uint32_t *covered, uint32_t covered_words, uint32_t *picked, uint32_t n)
{
    const uint32_t i = blockIdx.x * kVisThreads + threadIdx.x;
    if (i < covered_words) covered[i] = 0u;
    if (i < n) picked[i] = 0u;
}

// The 32 covered bits under a window word: window columns are offset from the bitmap's word borders by (x0 - R) mod 32,
// so a window word meets two of its words; words outside the grid read 0.
__device__ __forceinline__ uint32_t vis_covered_under(const uint32_t *row, uint32_t cov_wpr, int col0)
{
    const int wi = col0 >> 5;  // floor: col0 may be negative
    const uint32_t s = (uint32_t)col0 & 31u;
    const uint32_t lo = (uint32_t)wi < cov_wpr ? row[wi] : 0u;
    const uint32_t hi = s && (uint32_t)(wi + 1) < cov_wpr ? row[wi + 1] : 0u;
    return s ? (lo >> s) | (hi << (32u - s)) : lo;
}

// A selection round, first of three launches: g_k = |W_k \ C| per viewpoint, a workgroup each.  A round behind an ended
// selection (the previous round's key is 0) returns at once.
__global__ __launch_bounds__(kVisThreads) void k_vis_marginal(uint32_t round, const unsigned long long *keys, const VisRecord *records,
                                                              const uint32_t *windows, const uint32_t *covered, const uint32_t *picked,
                                                              VisArgs a, uint32_t *gain)
{
    __shared__ uint32_t part[kVisThreads / 64u];
    if (round && keys[round - 1u] == 0ull) return;
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    const VisRecord r = records[k];
    if (!r.valid || picked[k]) {  // uniform over the workgroup
        if (t == 0u) gain[k] = 0u;
        return;
    }
    const uint32_t *const win = windows + (size_t)k * a.win_words;
    const int R = (int)a.range;
    uint32_t g = 0u;
    for (uint32_t w = t; w < a.win_words; w += kVisThreads) {
        const uint32_t bits = win[w];
        if (!bits) continue;
        const uint32_t row = w / a.win_wpr, word = w - row * a.win_wpr;
        const uint32_t gy = (uint32_t)(r.iy - R + (int)row);
        if (gy >= a.height) continue;  // (a set bit is a cell of the grid)
        g += (uint32_t)__popc(bits & ~vis_covered_under(covered + (size_t)gy * a.cov_wpr, a.cov_wpr, r.ix - R + 32 * (int)word));
    }
    g = vis_wave_sum(g);
    if ((t & 63u) == 0u) part[t >> 6] = g;
    __syncthreads();
    if (t == 0u) gain[k] = part[0] + part[1] + part[2] + part[3];
}

// ... second: the winner, one unsigned 64-bit maximum of (s + 2^32) << 20 | (2^20 - 1 - k) over the viewpoints that are
// valid, not picked, not excluded by their cost and gain at least min_gain: the greatest score, ties to the least index.
// -(2^32 - 1) <= s <= 2^30, so the key is below 2^53 and never 0: 0 says that the selection has ended.
__global__ __launch_bounds__(kVisThreads) void k_vis_pick(uint32_t round, unsigned long long *keys, const VisRecord *records, uint32_t n,
                                                          const uint32_t *picked, const uint32_t *gain, const uint32_t *cost,
                                                          uint32_t gain_weight, uint32_t cost_shift, uint32_t min_gain)
{
    if (round && keys[round - 1u] == 0ull) return;
    const uint32_t k = blockIdx.x * kVisThreads + threadIdx.x;
    unsigned long long key = 0ull;
    if (k < n && records[k].valid && !picked[k]) {
        const uint32_t c = cost ? cost[k] : 0u, g = gain[k];
        if (!(cost && c == kVisUnreached) && g >= min_gain) {
            const long long s = (long long)g * (long long)gain_weight - (long long)(c >> cost_shift);
            key = ((unsigned long long)(s + (1ll << 32)) << kVisIndexBits) | (kVisIndexMask - k);
        }
    }
    key = vis_wave_max(key);
    if ((threadIdx.x & 63u) == 0u && key) atomicMax(keys + round, key);
}

// ... third: the winner's entry, its picked flag, and C |= W_winner, a lane per window word; the winner is read from the
// round's key in HBM, so the host never waits between rounds.
__global__ __launch_bounds__(kVisThreads) void k_vis_cover(uint32_t round, const unsigned long long *keys, const VisRecord *records,
                                                           const uint32_t *windows, uint32_t *covered, uint32_t *picked, const uint32_t *gain,
                                                           VisArgs a, VisPick *picks)
{
    const unsigned long long key = keys[round];
    if (key == 0ull) return;
    const uint32_t k = (uint32_t)(kVisIndexMask - (key & kVisIndexMask));
    const uint32_t w = blockIdx.x * kVisThreads + threadIdx.x;
    if (w == 0u) {
        picks[round] = VisPick{k, gain[k], (long long)(key >> kVisIndexBits) - (1ll << 32)};
        picked[k] = 1u;
    }
    if (w >= a.win_words) return;
    const uint32_t bits = windows[(size_t)k * a.win_words + w];
    if (!bits) return;
    const int R = (int)a.range;
    const uint32_t row = w / a.win_wpr, word = w - row * a.win_wpr;
    const uint32_t gy = (uint32_t)(records[k].iy - R + (int)row);
    if (gy >= a.height) return;  // (a set bit is a cell of the grid)
    const int col0 = records[k].ix - R + 32 * (int)word, wi = col0 >> 5;
    const uint32_t s = (uint32_t)col0 & 31u;
    uint32_t *const crow = covered + (size_t)gy * a.cov_wpr;
    const uint32_t lo = bits << s, hi = s ? bits >> (32u - s) : 0u;
    if (lo && (uint32_t)wi < a.cov_wpr) atomicOr(crow + wi, lo);
    if (hi && (uint32_t)(wi + 1) < a.cov_wpr) atomicOr(crow + wi + 1, hi);
}

}  // namespace lom
