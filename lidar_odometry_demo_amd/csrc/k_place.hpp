// Place recognition (include/lidar_odometry_amd.h, "place recognition"): the kernels.  Launched by
// place.hip alone.  wave64 throughout, no MFMA, no workgroup waits for another, vector atomics only.
//
//   k_place_bin     points -> R x S accumulation words (max of v = z - z_floor per polar cell, as u32 bits)
//   k_place_finish  accumulation words (or an uploaded raw descriptor) -> raw descriptor, unit columns, column mask;
//                   puts the accumulation words back to rest
//   k_place_query   one query x a tile of entries -> {distance, shift} per pair; a wave's lanes are the shifts
//   k_place_topk    per query, the k smallest (distance bits, id)
//
// Database layout.  Raw descriptors are [id][R][S] f32.  Unit columns are stored for k_place_query: groups of
// kPlaceGroup = 8 consecutive ids, [id / 8][S][R][id % 8] f32, so that the eight entries' values of one (column, ring)
// are one 32-byte scalar load and a column's R rings follow each other.  Masks are [id] u64, bit j = column j non-zero.
#pragma once
#include <cmath>

#include "lom_internal.hpp"

namespace lom {

constexpr int kPlaceMaxDim = 64;                    // rings, sectors: a lane is a column (finish) or a shift (query)
constexpr int kPlaceGroup = 8;                      // entries whose unit columns are interleaved
constexpr int kPlaceQueryWaves = 4;                 // waves of a k_place_query workgroup
constexpr int kPlaceTile = 64;                      // entries per k_place_query workgroup
constexpr int kPlaceBinThreads = 256;
constexpr int kPlaceTopkThreads = 1024;
constexpr uint32_t kPlaceNoCell = 0xFFFFFFFFu;

struct PlacePair {  // k_place_query's output per (query, entry)
    float distance;
    uint32_t shift;
};

struct PlaceShape {
    uint32_t R, S;
    double ring_width;    // (double)max_range / R
    double sector_width;  // 2 pi / S
    float z_floor;
};

// cell of a point: the header's definition, f64 from the f32 values; kPlaceNoCell for a point beyond the last ring
__device__ __forceinline__ uint32_t place_cell(const PlaceShape sh, float x, float y)
{
    const double dx = (double)x, dy = (double)y;
    const double rho = sqrt(dx * dx + dy * dy);
    const double fr = floor(rho / sh.ring_width);
    if (!(fr < (double)sh.R)) return kPlaceNoCell;
    double phi = atan2(dy, dx);
    if (phi < 0.0) phi += 6.283185307179586476925286766559;
    uint32_t sector = (uint32_t)floor(phi / sh.sector_width);
    if (sector >= sh.S) sector = 0;  // phi + 2 pi rounded to 2 pi itself: the angle 0
    return (uint32_t)fr * sh.S + sector;
}

// One thread per point, grid-stride.  The workgroup's table lives in LDS; its non-zero cells are merged into the
// accumulation words in HBM, which are all zero between calls (k_place_finish puts them back).  err[0] |= 1 on a
// non-finite coordinate.
__global__ __launch_bounds__(kPlaceBinThreads) void k_place_bin(const char *__restrict__ xyz, size_t stride, uint32_t n,
                                                                PlaceShape sh, uint32_t *__restrict__ acc,
                                                                uint32_t *__restrict__ err)
{
    __shared__ uint32_t s_cell[kPlaceMaxDim * kPlaceMaxDim];  // 16 KB
    const uint32_t cells = sh.R * sh.S;
    for (uint32_t c = threadIdx.x; c < cells; c += kPlaceBinThreads) s_cell[c] = 0u;
    __syncthreads();
    bool bad = false;
    for (uint32_t i = blockIdx.x * kPlaceBinThreads + threadIdx.x; i < n; i += gridDim.x * kPlaceBinThreads) {
        const float *p = reinterpret_cast<const float *>(xyz + (size_t)i * stride);
        const float x = p[0], y = p[1], z = p[2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
            bad = true;
            continue;
        }
        const float v = z - sh.z_floor;
        if (!(v > 0.f)) continue;
        const uint32_t cell = place_cell(sh, x, y);
        if (cell < cells) atomicMax(&s_cell[cell], __float_as_uint(v));  // v > 0: the bits order like the values
    }
    if (bad) atomicOr(err, 1u);
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < cells; c += kPlaceBinThreads) {
        const uint32_t v = s_cell[c];
        if (v) atomicMax(&acc[c], v);
    }
}

// where a descriptor's unit columns go: element (ring r, column j)
__device__ __forceinline__ size_t place_unit_index(uint32_t R, uint32_t S, bool grouped, uint64_t slot, uint32_t r, uint32_t j)
{
    if (!grouped) return (size_t)slot * R * S + (size_t)r * S + j;
    return ((size_t)(slot / kPlaceGroup) * S * R + (size_t)j * R + r) * kPlaceGroup + (size_t)(slot % kPlaceGroup);
}

// One wave per descriptor (blockIdx.x), lane j = column j.  src: R x S words per descriptor (f32 bits >= 0), either the
// accumulation words (zero_src = 1: they go back to rest here, and err[0] moves to err[1] for the host to read) or
// uploaded raw descriptors.  Norms in f64; a zero column stays zero and clears its mask bit.
__global__ __launch_bounds__(64) void k_place_finish(uint32_t *__restrict__ src, uint32_t R, uint32_t S, int zero_src,
                                                     float *__restrict__ dst_raw, float *__restrict__ dst_unit,
                                                     unsigned long long *__restrict__ dst_mask, uint64_t first_slot,
                                                     int grouped, uint32_t *__restrict__ err)
{
    const uint32_t j = threadIdx.x;
    const uint64_t slot = first_slot + blockIdx.x;
    uint32_t *s = src + (size_t)blockIdx.x * R * S;
    double sq = 0.0;
    if (j < S)
        for (uint32_t r = 0; r < R; r++) {
            const double v = (double)__uint_as_float(s[r * S + j]);
            sq += v * v;
        }
    const double norm = sqrt(sq);
    const unsigned long long m = __ballot(j < S && sq > 0.0);
    if (j < S)
        for (uint32_t r = 0; r < R; r++) {
            const uint32_t bits = s[r * S + j];
            const float v = __uint_as_float(bits);
            if (dst_raw) dst_raw[(size_t)slot * R * S + (size_t)r * S + j] = v;
            dst_unit[place_unit_index(R, S, grouped != 0, slot, r, j)] = sq > 0.0 ? (float)((double)v / norm) : 0.f;
            if (zero_src && bits) s[r * S + j] = 0u;
        }
    if (j == 0) {
        dst_mask[slot] = m;
        if (zero_src) {
            err[1] = err[0];
            err[0] = 0u;
        }
    }
}

template <int kCtrl>
__device__ __forceinline__ unsigned long long place_dpp_u64(unsigned long long v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, kCtrl, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), kCtrl, 0xF, 0xF, true);
    return ((unsigned long long)hi << 32) | lo;
}
// minimum over the wave (every lane takes part; a lane that must not carries ~0): DPP inside the rows of 16, the four
// row results by readlane.  The result is uniform.
__device__ __forceinline__ unsigned long long place_wave_min(unsigned long long v)
{
    unsigned long long o;
    o = place_dpp_u64<0xB1>(v), v = o < v ? o : v;   // quad_perm [1,0,3,2]
    o = place_dpp_u64<0x4E>(v), v = o < v ? o : v;   // quad_perm [2,3,0,1]
    o = place_dpp_u64<0x141>(v), v = o < v ? o : v;  // row_half_mirror
    o = place_dpp_u64<0x140>(v), v = o < v ? o : v;  // row_mirror
    unsigned long long best = ~0ull;
#pragma unroll
    for (int row = 0; row < 4; row++) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, row * 16);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), row * 16);
        const unsigned long long r = ((unsigned long long)hi << 32) | lo;
        best = r < best ? r : best;
    }
    return best;
}

// The hot path.  Workgroup = (tile of kPlaceTile entries, query blockIdx.y); the query's unit columns sit in LDS as
// [R][2S] (columns twice), so lane s reads column j' - s of the query against column j' of the entry at address
// (r * 2S + j' + S) - s: no modulo, consecutive banks.  A wave takes E entries of one group per LDS read; the entries'
// values are uniform over the wave (scalar loads).  Order of every sum: for each entry column j' = 0 .. S-1 a chain
// dot = fma(q, c, dot) over r = 0 .. R-1 from 0, then sum += dot -- fixed by (R, S) alone, so the bits of a pair's
// (distance, shift) depend on the two descriptors only.  Zero columns are zero vectors, so the columns outside V add 0.
template <int E>
__global__ __launch_bounds__(kPlaceQueryWaves * 64) void k_place_query(
    const float *__restrict__ unit, const unsigned long long *__restrict__ mask, const float *__restrict__ q_unit,
    const unsigned long long *__restrict__ q_mask, uint32_t R, uint32_t S, uint64_t id_begin, uint64_t id_end,
    PlacePair *__restrict__ out, float *__restrict__ all_dist)
{
    static_assert(E == 1 || E == 2 || E == 4 || E == 8, "E divides the group");
    extern __shared__ float s_q[];  // [R][2S]
    const uint32_t S2 = 2u * S;
    const float *qu = q_unit + (size_t)blockIdx.y * R * S;
    for (uint32_t i = threadIdx.x; i < R * S2; i += kPlaceQueryWaves * 64) {
        const uint32_t r = i / S2, c = i % S2;
        s_q[i] = qu[r * S + (c >= S ? c - S : c)];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t s = lane < S ? lane : 0u;  // lanes s >= S compute shift 0 again and stay out of the minimum
    const unsigned long long mq = q_mask[blockIdx.y];
    const unsigned long long smask = S == 64u ? ~0ull : ((1ull << S) - 1ull);
    const uint64_t n_range = id_end - id_begin;
    // tiles start at a multiple of the group size below id_begin, so that a group is never split
    const uint64_t first = id_begin / kPlaceGroup * kPlaceGroup + (uint64_t)blockIdx.x * kPlaceTile;
    constexpr uint32_t kParts = kPlaceTile / E;  // E-entry parts of the tile, dealt to the waves in turn
    const float *lq = s_q + S - s;
    for (uint32_t part = wave; part < kParts; part += kPlaceQueryWaves) {
        const uint64_t id0 = first + (uint64_t)part * E;
        if (id0 >= id_end) break;
        if (id0 + E <= id_begin) continue;
        const float *c = unit + (size_t)(id0 / kPlaceGroup) * S * R * kPlaceGroup + (size_t)(id0 % kPlaceGroup);
        float sum[E];
#pragma unroll
        for (int e = 0; e < E; e++) sum[e] = 0.f;
        for (uint32_t jc = 0; jc < S; jc++) {
            float dot[E];
#pragma unroll
            for (int e = 0; e < E; e++) dot[e] = 0.f;
            const float *cj = c + (size_t)jc * R * kPlaceGroup;
            const float *qj = lq + jc;
#pragma unroll 4
            for (uint32_t r = 0; r < R; r++) {
                const float qv = qj[r * S2];
#pragma unroll
                for (int e = 0; e < E; e++) dot[e] = __builtin_fmaf(qv, cj[r * kPlaceGroup + e], dot[e]);
            }
#pragma unroll
            for (int e = 0; e < E; e++) sum[e] += dot[e];
        }
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint64_t id = id0 + e;
            if (id >= id_end) break;  // uniform
            if (id < id_begin) continue;
            const unsigned long long mc = mask[id];
            // column j of the query meets column (j + s) mod S of the entry
            const unsigned long long rot = s ? (((mc >> s) | (mc << (S - s))) & smask) : mc;
            const int cnt = __popcll(mq & rot);
            float d = 1.f;
            if (cnt) d = fmaxf(1.f - __fdiv_rn(sum[e], (float)cnt), 0.f);  // >= 0: the bits order like the values
            const unsigned long long key = lane < S ? (((unsigned long long)__float_as_uint(d) << 8) | s) : ~0ull;
            const unsigned long long best = place_wave_min(key);
            if (lane == 0) {
                const size_t o = (size_t)blockIdx.y * n_range + (size_t)(id - id_begin);
                PlacePair p;
                p.distance = __uint_as_float((uint32_t)(best >> 8));
                p.shift = (uint32_t)(best & 0xFFu);
                out[o] = p;
                if (all_dist) all_dist[o] = p.distance;
            }
        }
    }
}

struct PlaceMatch {  // lom_place_match
    long long id;
    float distance;
    uint32_t shift;
};

// One workgroup per query: k rounds, each the minimum of (distance bits << 32 | index) over the row among the keys
// above the previous round's.  N k compares: nothing beside the query.
__global__ __launch_bounds__(kPlaceTopkThreads) void k_place_topk(const PlacePair *__restrict__ pairs, uint32_t n_range,
                                                                  uint64_t id_begin, int k, PlaceMatch *__restrict__ out)
{
    __shared__ unsigned long long s_min[kPlaceTopkThreads / 64];
    __shared__ unsigned long long s_last;
    const PlacePair *row = pairs + (size_t)blockIdx.x * n_range;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long last = 0ull;
    bool have_last = false;
    for (int round = 0; round < k; round++) {
        unsigned long long best = ~0ull;
        for (uint32_t i = threadIdx.x; i < n_range; i += kPlaceTopkThreads) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(row[i].distance) << 32) | i;
            if ((!have_last || key > last) && key < best) best = key;
        }
        best = place_wave_min(best);
        if (lane == 0) s_min[wave] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long b = ~0ull;
            for (int w = 0; w < kPlaceTopkThreads / 64; w++) b = s_min[w] < b ? s_min[w] : b;
            s_last = b;
            PlaceMatch m;
            if (b != ~0ull) {
                const uint32_t i = (uint32_t)b;
                m.id = (long long)(id_begin + i);
                m.distance = __uint_as_float((uint32_t)(b >> 32));
                m.shift = row[i].shift;
            } else {  // fewer than k entries searched
                m.id = -1;
                m.distance = __uint_as_float(0x7F800000u);
                m.shift = 0u;
            }
            out[(size_t)blockIdx.x * k + round] = m;
        }
        __syncthreads();
        last = s_last;
        have_last = true;
        if (last == ~0ull) {  // uniform: the rest are empty slots
            if (threadIdx.x == 0)
                for (int t = round + 1; t < k; t++) {
                    PlaceMatch m;
                    m.id = -1, m.distance = __uint_as_float(0x7F800000u), m.shift = 0u;
                    out[(size_t)blockIdx.x * k + t] = m;
                }
            break;
        }
    }
}

}  // namespace lom
