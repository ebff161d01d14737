// Ray carving (include/lidar_odometry_amd.h, "ray carving"): k_carve_hits, k_carve_walk and k_carve_flag.  Device code
// only; map_carve.hip is the one translation unit that instantiates and launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grid_scan.hpp"
#include "k_carve_cell.hpp"
#include "lom_internal.hpp"

namespace lom {

// the carve's own status words (scratch slot S_CARVE_WORDS, zeroed per call): the host reads them in one read-back
enum {
    CW_ERROR = 0,      // a non-finite / out-of-range endpoint, or a walk that left the index range
    CW_CROSSED = 1,    // live voxels some ray crossed
    CW_PROTECTED = 2,  // live voxels crossed often enough to go that a hit keeps
    // (word 3 is unused: the two 64-bit counters start at an even word, 8-byte aligned for their atomics)
    CW_WALKED = 4,     // u64 (two words): rays walked
    CW_VISITED = 6,    // u64: cells visited, over all rays
    CW_COUNT = 8
};

struct CarveArgs {
    float o[3];        // origin, map frame
    float voxel_size;
    float margin, min_range, max_range;
    uint32_t max_steps;  // 3 * (ceil(max_range / V) + 2): a guard, the walk ends by itself before
};

// (carve_find_slab, carve_plane, carve_t: k_carve_cell.hpp)

// A thread per endpoint: the voxel that contains it (the insert's index rule) is protected.  Plain stores: every
// writer stores the same 1.
__global__ __launch_bounds__(kThreads) void k_carve_hits(const char *xyz, size_t stride, uint32_t n, float voxel_size,
                                                         const Slot *table, uint32_t mask, uint32_t shift, uint32_t n_vox,
                                                         uint32_t *hit, uint32_t *words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = reinterpret_cast<const float *>(xyz + (size_t)i * stride);
    int ix, iy, iz;
    const bool okx = voxel_index(p[0], voxel_size, ix), oky = voxel_index(p[1], voxel_size, iy),
               okz = voxel_index(p[2], voxel_size, iz);
    if (!(okx && oky && okz)) {
        words[CW_ERROR] = 1u;
        return;
    }
    const uint32_t slab = carve_find_slab(table, mask, shift, pack_key(ix, iy, iz));
    if (slab < n_vox) hit[slab] = 1u;
}

// The hot path: a lane per ray.  All f64 from the f32 inputs, no contraction (the tree is built with -ffp-contract=off);
// state in registers, the axis picked with selects; a table probe per visited cell, cross[slab]++ where a voxel lives.
__global__ __launch_bounds__(kThreads) void k_carve_walk(const char *xyz, size_t stride, uint32_t n, CarveArgs a,
                                                         const Slot *table, uint32_t mask, uint32_t shift, uint32_t n_vox,
                                                         uint32_t *cross, uint32_t *words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t visited = 0;
    bool walk = false, range_error = false;
    if (i < n) {
        const float *p = reinterpret_cast<const float *>(xyz + (size_t)i * stride);
        const float px = p[0], py = p[1], pz = p[2];
        int e;
        // (an endpoint out of range fails the call in k_carve_hits; its ray is not walked)
        const bool ok = voxel_index(px, a.voxel_size, e) && voxel_index(py, a.voxel_size, e) && voxel_index(pz, a.voxel_size, e);
        const double V = (double)a.voxel_size;
        const double Ox = (double)a.o[0], Oy = (double)a.o[1], Oz = (double)a.o[2];
        const double Dx = (double)px - Ox, Dy = (double)py - Oy, Dz = (double)pz - Oz;
        const double L = __dsqrt_rn(Dx * Dx + (Dy * Dy + Dz * Dz));
        const double reach = L < (double)a.max_range ? L : (double)a.max_range;
        const double t_end = (reach - (double)a.margin) / L;
        walk = ok && L >= (double)a.min_range && t_end > 0.0;
        if (walk) {
            int cx = (int)(Ox / V), cy = (int)(Oy / V), cz = (int)(Oz / V);
            const int sx = Dx > 0.0 ? 1 : -1, sy = Dy > 0.0 ? 1 : -1, sz = Dz > 0.0 ? 1 : -1;
            double tx = carve_t(cx, sx, V, Ox, Dx), ty = carve_t(cy, sy, V, Oy, Dy), tz = carve_t(cz, sz, V, Oz, Dz);
            for (uint32_t step = 0; step < a.max_steps; step++) {
                visited++;
                const uint32_t slab = carve_find_slab(table, mask, shift, pack_key(cx, cy, cz));
                if (slab < n_vox) atomicAdd(&cross[slab], 1u);
                const bool ax = tx <= ty && tx <= tz;  // ties: x before y before z
                const bool ay = !ax && ty <= tz;
                const double t_min = ax ? tx : (ay ? ty : tz);
                if (!(t_min <= t_end)) break;
                const int c = (ax ? cx : (ay ? cy : cz)) + (ax ? sx : (ay ? sy : sz));
                if (c <= -kIdxBias || c >= kIdxBias) {
                    range_error = true;
                    break;
                }
                const double t = carve_t(c, ax ? sx : (ay ? sy : sz), V, ax ? Ox : (ay ? Oy : Oz), ax ? Dx : (ay ? Dy : Dz));
                cx = ax ? c : cx;
                cy = ay ? c : cy;
                cz = (ax || ay) ? cz : c;
                tx = ax ? t : tx;
                ty = ay ? t : ty;
                tz = (ax || ay) ? tz : t;
            }
        }
    }
    if (range_error) words[CW_ERROR] = 1u;
    // the two totals: summed over the wave first, one 64-bit atomic each per wave (integer sums: no order in the result)
    const unsigned long long walked_wave = (unsigned long long)__popcll(__ballot(walk));
    uint32_t v = visited;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63u) == 0u) {
        if (walked_wave) atomicAdd(reinterpret_cast<unsigned long long *>(words + CW_WALKED), walked_wave);
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(words + CW_VISITED), (unsigned long long)v);
    }
}

// the decision per slab: keep[] for the scan and the erase back end that radiusCleanup uses, and the two voxel counts
__global__ __launch_bounds__(kThreads) void k_carve_flag(const uint32_t *cross, const uint32_t *hit, const uint32_t *slab_count,
                                                         uint32_t n_vox, uint32_t min_crossings, uint32_t *keep, uint32_t *words)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    bool crossed = false, saved = false;
    if (s < n_vox) {
        const bool live = slab_count[s] != 0u;  // (an empty slab: erased before -- not kept, not counted)
        const uint32_t c = cross[s];
        const bool h = hit[s] != 0u;
        const bool often = c >= min_crossings;
        keep[s] = (live && !(often && !h)) ? 1u : 0u;
        crossed = live && c != 0u;
        saved = live && often && h;
    }
    const uint32_t nc = (uint32_t)__popcll(__ballot(crossed)), np = (uint32_t)__popcll(__ballot(saved));
    if ((threadIdx.x & 63u) == 0u) {
        if (nc) atomicAdd(words + CW_CROSSED, nc);
        if (np) atomicAdd(words + CW_PROTECTED, np);
    }
}

}  // namespace lom
