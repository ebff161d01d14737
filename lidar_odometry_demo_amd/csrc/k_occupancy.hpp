// Occupancy grid (include/lidar_odometry_amd.h, "occupancy grid"): k_occ_walk, k_occ_fold and k_occ_classify.  Device code
// only; occupancy.hip is the one translation unit that instantiates and launches it.  The scan descriptor and its
// constant-address-space read are the assembly's (k_asm_scan.hpp), the transform is the one every posed-scan kernel
// uses (k_posed_point.hpp).
//
// A launch of k_occ_walk holds a slice of up to 64 scans: blockIdx.y names the scan and its two bitmaps, pass and hit, of
// height x ceil(width / 32) u32 each.  Bits are only ever set, so a lane that goes to global memory first looks with a
// plain load and skips the atomic where the bit is there already -- a stale look costs an atomic, never a vote.  The hot
// loop's bits go to an LDS window around the scan's origin cell instead and are flushed once per workgroup.  k_occ_fold
// turns the bitmaps of a slice into the counts and puts them back to zero.  No workgroup waits for another; no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "k_asm_scan.hpp"
#include "k_posed_point.hpp"

namespace lom {

constexpr uint32_t kOccThreads = 256;  // k_occ_fold and k_occ_classify: a thread per cell

// the status words of a call (zeroed per call): three u64 counters, 8-byte aligned for their atomics
enum {
    OW_WALKED = 0,   // u64 (two words): rays walked
    OW_VISITED = 2,  // u64: cells visited, over all rays
    OW_MARKED = 4,   // u64: endpoints that are hits
    OW_COUNT = 6
};
// of a classification: cells free / occupied / unknown (u32: a grid has at most 2^28 cells)
enum { OC_FREE = 0, OC_OCCUPIED = 1, OC_UNKNOWN = 2, OC_COUNT = 4 };

struct OccArgs {
    float resolution, origin_x, origin_y;
    uint32_t width, height, wpr;  // wpr: u32 words of a bitmap row
    float z_lo, z_hi, margin, min_range, max_range;
    uint32_t max_steps;  // occupancy::max_steps: a guard, the walk ends by itself before
    uint32_t window;     // side of the LDS window in cells (a multiple of 32; 0: none); the launch passes window^2 / 8 bytes
    uint32_t stride;     // floats per input record (3: an archive)
};

// sets `bit` of *word; the plain load first (see above)
__device__ __forceinline__ void occ_mark(uint32_t *word, uint32_t bit)
{
    if ((*word & bit) == 0u) atomicOr(word, bit);
}

// t_a of the header's step 5: the plane rule, recomputed from the cell -- never incremented
__device__ __forceinline__ double occ_t(int c, int s, double r, double O2, double D)
{
    if (D == 0.0) return __builtin_inf();
    const int b = s > 0 ? c + 1 : c;
    return ((double)b * r - O2) / D;
}

// The hot path: a lane per ray of its scan.  The point (12 bytes of a record) is transformed by posed_point
// (k_posed_point.hpp) and never stored.  cell: the scan's start cells (x, y per scan, the host's verdict).
// bitmaps: [scan of the slice][pass, hit][row][word].
__global__ __launch_bounds__(kAsmThreads) void k_occ_walk(const AsmScan *scans, const int32_t *cell, const float *__restrict__ xyz,
                                                          OccArgs a, uint32_t *bitmaps, uint32_t *words)
{
    extern __shared__ uint32_t win[];
    const ConstAsm d = (ConstAsm)(scans + blockIdx.y);
    const uint32_t n = d->n, first = blockIdx.x * kAsmThreads;
    if (first >= n) return;  // a surplus workgroup (uniform: before any barrier)
    const size_t map_words = (size_t)a.height * a.wpr;
    uint32_t *const pass = bitmaps + (size_t)blockIdx.y * 2 * map_words;
    uint32_t *const hit = pass + map_words;
    const int c0x = cell[2 * blockIdx.y], c0y = cell[2 * blockIdx.y + 1];
    // the window: `window` cells a side, centred on the start cell, its first column a multiple of 32 (floor)
    const int W = (int)a.window, wrow = W >> 5;
    const int wx0 = (c0x - (W >> 1)) & ~31, wy0 = c0y - (W >> 1);
    const uint32_t win_words = (uint32_t)(W * wrow);
    for (uint32_t w = threadIdx.x; w < win_words; w += kAsmThreads) win[w] = 0u;
    if (W) __syncthreads();

    const uint32_t i = first + threadIdx.x;
    uint32_t visited = 0;
    bool walk = false, is_hit = false;
    if (i < n) {
        const size_t s = ((size_t)d->src + i) * a.stride;
        float px, py, pz;
        posed_point(d, xyz + s, px, py, pz);
        const double r = (double)a.resolution, Gx = (double)a.origin_x, Gy = (double)a.origin_y;
        const double Ox = (double)(float)d->t[0], Oy = (double)(float)d->t[1], Oz = (double)(float)d->t[2];
        const double O2x = Ox - Gx, O2y = Oy - Gy;
        const double Dx = (double)px - Ox, Dy = (double)py - Oy, Dz = (double)pz - Oz;
        const double L = __dsqrt_rn(Dx * Dx + (Dy * Dy + Dz * Dz));
        const double t_band = Dz > 0.0 ? (double)a.z_hi / Dz : (Dz < 0.0 ? (double)a.z_lo / Dz : __builtin_inf());
        const double reach = (L < (double)a.max_range ? L : (double)a.max_range) - (double)a.margin;
        const double q = reach / L;
        const double t_end = q < t_band ? q : t_band;
        const bool far_enough = L >= (double)a.min_range;
        walk = far_enough && t_end > 0.0;
        // the hit: the endpoint's cell by the floor rule, compared in f64 before any conversion
        const double hx = __builtin_floor(((double)px - Gx) / r), hy = __builtin_floor(((double)py - Gy) / r);
        is_hit = far_enough && L <= (double)a.max_range && (double)a.z_lo <= Dz && Dz <= (double)a.z_hi && hx >= 0.0 &&
                 hx < (double)a.width && hy >= 0.0 && hy < (double)a.height;
        if (is_hit) {
            const uint32_t ix = (uint32_t)hx, iy = (uint32_t)hy;
            occ_mark(hit + (size_t)iy * a.wpr + (ix >> 5), 1u << (ix & 31u));
        }
        if (walk) {
            int cx = c0x, cy = c0y;
            const int sx = Dx > 0.0 ? 1 : -1, sy = Dy > 0.0 ? 1 : -1;
            double tx = occ_t(cx, sx, r, O2x, Dx), ty = occ_t(cy, sy, r, O2y, Dy);
            for (uint32_t step = 0; step < a.max_steps; step++) {
                visited++;
                if ((uint32_t)cx < a.width && (uint32_t)cy < a.height) {
                    const uint32_t bit = 1u << ((uint32_t)cx & 31u);
                    const uint32_t lx = (uint32_t)(cx - wx0), ly = (uint32_t)(cy - wy0);
                    if (lx < (uint32_t)W && ly < (uint32_t)W)
                        atomicOr(win + ly * (uint32_t)wrow + (lx >> 5), bit);  // (result unused: ds_or_b32)
                    else
                        occ_mark(pass + (size_t)cy * a.wpr + ((uint32_t)cx >> 5), bit);
                }
                const bool ax = tx <= ty;  // ties: x before y
                if (!((ax ? tx : ty) <= t_end)) break;
                if (ax) {
                    cx += sx;
                    tx = occ_t(cx, sx, r, O2x, Dx);
                } else {
                    cy += sy;
                    ty = occ_t(cy, sy, r, O2y, Dy);
                }
            }
        }
    }
    // the window's non-zero words: consecutive lanes flush consecutive words of a bitmap row, so a wave's atomics cover
    // contiguous bytes.  (A non-zero word holds bits of cells in the grid only, so its row and word are the grid's.)
    if (W) {
        __syncthreads();
        for (uint32_t w = threadIdx.x; w < win_words; w += kAsmThreads) {
            const uint32_t v = win[w];
            if (v) {
                const uint32_t ly = w / (uint32_t)wrow, lw = w - ly * (uint32_t)wrow;
                const uint32_t gy = (uint32_t)(wy0 + (int)ly), gw = (uint32_t)((wx0 >> 5) + (int)lw);
                uint32_t *const g = pass + (size_t)gy * a.wpr + gw;
                if ((*g & v) != v) atomicOr(g, v);
            }
        }
    }
    // the totals: summed over the wave first, one 64-bit atomic each per wave (integer sums: no order in the result)
    const unsigned long long walked_wave = (unsigned long long)__popcll(__ballot(walk));
    const unsigned long long marked_wave = (unsigned long long)__popcll(__ballot(is_hit));
    uint32_t v = visited;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63u) == 0u) {
        if (walked_wave) atomicAdd(reinterpret_cast<unsigned long long *>(words + OW_WALKED), walked_wave);
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(words + OW_VISITED), (unsigned long long)v);
        if (marked_wave) atomicAdd(reinterpret_cast<unsigned long long *>(words + OW_MARKED), marked_wave);
    }
}

// Once per slice, a thread per cell of the slice's bounding box (word columns [wx0, wx1), rows [y0, y1)): over the S scans
// seen += hit bit, free += pass & ~hit bit -- a cell has one owner, plain read-modify-writes -- and the bitmap words of
// the box go back to zero.  The 32 cells of a word are 32 consecutive threads of one workgroup; the word's first thread
// zeroes it behind the barrier, when all 32 have read it.
__global__ __launch_bounds__(kOccThreads) void k_occ_fold(uint32_t *bitmaps, uint32_t n_scans, uint32_t width, uint32_t height,
                                                          uint32_t wpr, uint32_t wx0, uint32_t wx1, uint32_t y0, uint32_t y1,
                                                          uint32_t *free_votes, uint32_t *seen_votes)
{
    const uint32_t box_w = (wx1 - wx0) * 32u;
    const uint32_t t = blockIdx.x * kOccThreads + threadIdx.x;
    const uint32_t row = t / box_w, col = t - row * box_w;
    const bool valid = row < y1 - y0;
    const uint32_t x = wx0 * 32u + col, y = y0 + row;
    const size_t map_words = (size_t)height * wpr, w = (size_t)y * wpr + (x >> 5);
    unsigned long long nz_pass = 0ull, nz_hit = 0ull;
    if (valid) {
        uint32_t f = 0u, s = 0u;
        const uint32_t b = x & 31u;
        for (uint32_t k = 0; k < n_scans; k++) {
            const uint32_t p = bitmaps[(size_t)(2 * k) * map_words + w], h = bitmaps[(size_t)(2 * k + 1) * map_words + w];
            s += (h >> b) & 1u;
            f += ((p & ~h) >> b) & 1u;
            nz_pass |= (unsigned long long)(p != 0u) << k;
            nz_hit |= (unsigned long long)(h != 0u) << k;
        }
        if (x < width) {
            const size_t c = (size_t)y * width + x;
            if (s) seen_votes[c] += s;
            if (f) free_votes[c] += f;
        }
    }
    __syncthreads();
    if (valid && (x & 31u) == 0u) {
        for (uint32_t k = 0; k < n_scans; k++) {
            if ((nz_pass >> k) & 1ull) bitmaps[(size_t)(2 * k) * map_words + w] = 0u;
            if ((nz_hit >> k) & 1ull) bitmaps[(size_t)(2 * k + 1) * map_words + w] = 0u;
        }
    }
}

// The header's step 7, a thread per cell, and the three totals (summed over the wave first).
__global__ __launch_bounds__(kOccThreads) void k_occ_classify(const uint32_t *__restrict__ free_votes,
                                                              const uint32_t *__restrict__ seen_votes, uint32_t n_cells,
                                                              uint32_t min_free_scans, uint32_t free_per_seen,
                                                              uint32_t min_seen_scans, int8_t *out, uint32_t *totals)
{
    const uint32_t c = blockIdx.x * kOccThreads + threadIdx.x;
    bool is_free = false, is_occ = false, is_unknown = false;
    if (c < n_cells) {
        const uint32_t f = free_votes[c], s = seen_votes[c];
        is_free = f >= min_free_scans && (unsigned long long)f >= (unsigned long long)free_per_seen * (unsigned long long)s;
        is_occ = !is_free && s >= min_seen_scans;
        is_unknown = !is_free && !is_occ;
        out[c] = is_free ? (int8_t)0 : (is_occ ? (int8_t)100 : (int8_t)-1);
    }
    const uint32_t nf = (uint32_t)__popcll(__ballot(is_free)), no = (uint32_t)__popcll(__ballot(is_occ)),
                   nu = (uint32_t)__popcll(__ballot(is_unknown));
    if ((threadIdx.x & 63u) == 0u) {
        if (nf) atomicAdd(totals + OC_FREE, nf);
        if (no) atomicAdd(totals + OC_OCCUPIED, no);
        if (nu) atomicAdd(totals + OC_UNKNOWN, nu);
    }
}

}  // namespace lom
