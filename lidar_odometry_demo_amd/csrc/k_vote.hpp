// Scan votes (include/lidar_odometry_amd.h, "scan votes"): k_vote_walk, k_vote_fold and k_vote_flag.  Device code only;
// vote.hip is the one translation unit that instantiates and launches it.  The table probe, the plane rule and t_a are
// the carve's (k_carve_cell.hpp), the scan descriptor and its constant-address-space read the assembly's (k_asm_scan.hpp).
//
// A launch of k_vote_walk holds a slice of up to 64 scans: blockIdx.y names the scan and its bit in the two 64-bit masks
// a slab has, hitmask and crossmask.  Bits are only ever set, so a lane first looks with a plain load and skips the
// atomic where its scan's bit is there already -- a stale look costs an atomic, never a vote.  k_vote_fold turns the
// masks of a slice into the counts and puts the masks back to zero.  No workgroup waits for another; no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grid_scan.hpp"
#include "k_asm_scan.hpp"
#include "k_carve_cell.hpp"
#include "k_posed_point.hpp"
#include "lom_internal.hpp"

namespace lom {

// the votes' own status words (zeroed per call): the host reads them in one read-back
enum {
    VW_ERROR = 0,      // a non-finite / out-of-range endpoint, or a walk that left the index range
    VW_FREE = 1,       // live voxels with free >= 1
    VW_PROTECTED = 2,  // live voxels with free >= min_free_scans that the ratio kept
    // (word 3 is unused: the two 64-bit counters start at an even word, 8-byte aligned for their atomics)
    VW_WALKED = 4,     // u64 (two words): rays walked
    VW_VISITED = 6,    // u64: cells visited, over all rays
    VW_COUNT = 8
};

struct VoteArgs {
    float voxel_size;
    float margin, min_range, max_range, clearance;
    uint32_t max_steps;  // vote::max_steps: a guard, the walk ends by itself before
};

// sets `bit` of *mask; the plain load first (see above)
__device__ __forceinline__ void vote_mark(unsigned long long *mask, unsigned long long bit)
{
    if ((*mask & bit) == 0ull) atomicOr(mask, bit);
}

// The hot path: a lane per ray of its scan.  The archive point and normal (24 bytes) are transformed as k_asm_transform
// does -- posed_point (k_posed_point.hpp), the normal likewise without t -- and never stored; the endpoint's voxel gets the scan's bit in hitmask, every live
// voxel the walk visits gets it in crossmask.  The walk is k_carve_walk's but for t_end (the header's step 4).
__global__ __launch_bounds__(kAsmThreads) void k_vote_walk(const AsmScan *scans, const float *__restrict__ xyz,
                                                           const float *__restrict__ nrm, VoteArgs a, const Slot *table,
                                                           uint32_t mask, uint32_t shift, uint32_t n_vox,
                                                           unsigned long long *hitmask, unsigned long long *crossmask,
                                                           uint32_t *words)
{
    const ConstAsm d = (ConstAsm)(scans + blockIdx.y);
    const uint32_t n = d->n, first = blockIdx.x * kAsmThreads;
    if (first >= n) return;
    const unsigned long long bit = 1ull << blockIdx.y;
    const uint32_t i = first + threadIdx.x;
    uint32_t visited = 0;
    bool walk = false, range_error = false;
    if (i < n) {
        const size_t s = ((size_t)d->src + i) * 3;
        float px, py, pz;
        posed_point(d, xyz + s, px, py, pz);
        const double n0 = nrm[s], n1 = nrm[s + 1], n2 = nrm[s + 2];
        const float nx = (float)(d->R[0] * n0 + (d->R[1] * n1 + d->R[2] * n2));
        const float ny = (float)(d->R[3] * n0 + (d->R[4] * n1 + d->R[5] * n2));
        const float nz = (float)(d->R[6] * n0 + (d->R[7] * n1 + d->R[8] * n2));
        int ix, iy, iz;
        const bool okx = voxel_index(px, a.voxel_size, ix), oky = voxel_index(py, a.voxel_size, iy),
                   okz = voxel_index(pz, a.voxel_size, iz);
        const bool ok = okx && oky && okz;
        range_error = !ok;
        if (ok) {
            const uint32_t slab = carve_find_slab(table, mask, shift, pack_key(ix, iy, iz));
            if (slab < n_vox) vote_mark(hitmask + slab, bit);
        }
        const double V = (double)a.voxel_size;
        // (the origin's range verdict is the host's: vote::origin_ok)
        const double Ox = (double)(float)d->t[0], Oy = (double)(float)d->t[1], Oz = (double)(float)d->t[2];
        const double Dx = (double)px - Ox, Dy = (double)py - Oy, Dz = (double)pz - Oz;
        const double L = __dsqrt_rn(Dx * Dx + (Dy * Dy + Dz * Dz));
        const double c = __builtin_fabs((double)nx * Dx + ((double)ny * Dy + (double)nz * Dz)) / L;
        const double reach = (L < (double)a.max_range ? L : (double)a.max_range) - (double)a.margin;
        const double plane = a.clearance > 0.f ? L - (double)a.clearance / c : reach;
        const double t_end = (plane < reach ? plane : reach) / L;
        walk = ok && L >= (double)a.min_range && t_end > 0.0;
        if (walk) {
            int cx = (int)(Ox / V), cy = (int)(Oy / V), cz = (int)(Oz / V);
            const int sx = Dx > 0.0 ? 1 : -1, sy = Dy > 0.0 ? 1 : -1, sz = Dz > 0.0 ? 1 : -1;
            double tx = carve_t(cx, sx, V, Ox, Dx), ty = carve_t(cy, sy, V, Oy, Dy), tz = carve_t(cz, sz, V, Oz, Dz);
            for (uint32_t step = 0; step < a.max_steps; step++) {
                visited++;
                const uint32_t slab = carve_find_slab(table, mask, shift, pack_key(cx, cy, cz));
                if (slab < n_vox) vote_mark(crossmask + slab, bit);
                const bool ax = tx <= ty && tx <= tz;  // ties: x before y before z
                const bool ay = !ax && ty <= tz;
                const double t_min = ax ? tx : (ay ? ty : tz);
                if (!(t_min <= t_end)) break;
                const int cn = (ax ? cx : (ay ? cy : cz)) + (ax ? sx : (ay ? sy : sz));
                if (cn <= -kIdxBias || cn >= kIdxBias) {
                    range_error = true;
                    break;
                }
                const double t = carve_t(cn, ax ? sx : (ay ? sy : sz), V, ax ? Ox : (ay ? Oy : Oz), ax ? Dx : (ay ? Dy : Dz));
                cx = ax ? cn : cx;
                cy = ay ? cn : cy;
                cz = (ax || ay) ? cz : cn;
                tx = ax ? t : tx;
                ty = ay ? t : ty;
                tz = (ax || ay) ? tz : t;
            }
        }
    }
    if (range_error) words[VW_ERROR] = 1u;
    // the two totals: summed over the wave first, one 64-bit atomic each per wave (integer sums: no order in the result)
    const unsigned long long walked_wave = (unsigned long long)__popcll(__ballot(walk));
    uint32_t v = visited;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63u) == 0u) {
        if (walked_wave) atomicAdd(reinterpret_cast<unsigned long long *>(words + VW_WALKED), walked_wave);
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(words + VW_VISITED), (unsigned long long)v);
    }
}

// Once per slice, a thread per slab: the scans of the slice that saw the voxel, and those that saw through it and did
// not see it; the masks go back to rest.
__global__ __launch_bounds__(kThreads) void k_vote_fold(unsigned long long *hitmask, unsigned long long *crossmask, uint32_t n_vox,
                                                        uint32_t *free_votes, uint32_t *seen_votes)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_vox) return;
    const unsigned long long h = hitmask[s], c = crossmask[s];
    if (h) {
        seen_votes[s] += (uint32_t)__popcll(h);
        hitmask[s] = 0ull;
    }
    if (c) {
        const uint32_t f = (uint32_t)__popcll(c & ~h);
        if (f) free_votes[s] += f;
        crossmask[s] = 0ull;
    }
}

// The decision per slab: keep[] for the scan and the erase back end that the carve and radiusCleanup use, and the two
// voxel counts; free / seen go back to rest.
__global__ __launch_bounds__(kThreads) void k_vote_flag(uint32_t *free_votes, uint32_t *seen_votes, const uint32_t *slab_count,
                                                        uint32_t n_vox, uint32_t min_free_scans, uint32_t free_per_seen,
                                                        uint32_t *keep, uint32_t *words)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    bool any_free = false, saved = false;
    if (s < n_vox) {
        const bool live = slab_count[s] != 0u;  // (an empty slab: erased before -- not kept, not counted)
        const uint32_t f = free_votes[s], sn = seen_votes[s];
        const bool enough = f >= min_free_scans;
        const bool ratio = (unsigned long long)f >= (unsigned long long)free_per_seen * (unsigned long long)sn;
        keep[s] = (live && !(enough && ratio)) ? 1u : 0u;
        any_free = live && f != 0u;
        saved = live && enough && !ratio;
        if (f) free_votes[s] = 0u;
        if (sn) seen_votes[s] = 0u;
    }
    const uint32_t nf = (uint32_t)__popcll(__ballot(any_free)), np = (uint32_t)__popcll(__ballot(saved));
    if ((threadIdx.x & 63u) == 0u) {
        if (nf) atomicAdd(words + VW_FREE, nf);
        if (np) atomicAdd(words + VW_PROTECTED, np);
    }
}

}  // namespace lom
