// Map assembly (lom_map_assemble): k_asm_transform, k_asm_offsets, k_asm_compact.  Device code only; archive.hip is the one
// translation unit that instantiates and launches it.  Definitions: include/lidar_odometry_amd.h ("scan archive and map
// assembly"); DESIGN.md 7h.
//
// A launch is a grid (workgroups of the largest scan, scans): blockIdx.y names the scan, whose descriptor is read through
// the constant address space (scalar loads, like kernel arguments); a scan's surplus workgroups leave at once.  One point
// per thread: lane i of a wave reads and writes the 12 bytes at base + 12 i, so a wave covers 768 contiguous bytes per
// array -- whole 128-byte lines but for the two ends; 16-byte accesses would need a 16-aligned base, which a 12-byte point
// at an arbitrary scan offset does not have.  No floating-point atomics, no waiting for another workgroup, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "assemble_host.hpp"
#include "k_asm_scan.hpp"
#include "k_posed_point.hpp"

namespace lom {

// (AsmScan, kAsmThreads, ConstAsm: k_asm_scan.hpp)
constexpr uint32_t kAsmWaves = kAsmThreads / 64;
constexpr uint32_t kAsmOffsetThreads = 1024;

// the predicate of k_cleanup_flag on a point: f32, strict -- a point at exactly the radius stays (and so does a NaN, for
// the insert to refuse)
__device__ inline bool asm_culled(float x, float y, float z, float cx, float cy, float cz, float r2)
{
    const float dx = x - cx, dy = y - cy, dz = z - cz;
    const float d2 = dx * dx + (dy * dy + dz * dz);
    return d2 > r2;
}

// lanes below this one whose bit is set
__device__ inline uint32_t asm_rank(unsigned long long ballot)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// The point at the scan's pose (posed_point, k_posed_point.hpp: f64, one rounding at the end) and the normal likewise
// without t, written at the scan's place in the concatenated cloud.  kCull: the workgroup's
// count of points inside the radius goes to counts[scan's row + blockIdx.x].
template <bool kCull>
__global__ __launch_bounds__(kAsmThreads) void k_asm_transform(const AsmScan *scans, const float *__restrict__ xyz,
                                                               const float *__restrict__ nrm, float *__restrict__ out_xyz,
                                                               float *__restrict__ out_nrm, float cx, float cy, float cz,
                                                               float r2, uint32_t *__restrict__ counts)
{
    const ConstAsm d = (ConstAsm)(scans + blockIdx.y);
    const uint32_t n = d->n, first = blockIdx.x * kAsmThreads;
    if (first >= n) return;
    const uint32_t i = first + threadIdx.x;
    bool keep = false;
    if (i < n) {
        const size_t s = ((size_t)d->src + i) * 3, o = ((size_t)d->out + i) * 3;
        float x, y, z;
        posed_point(d, xyz + s, x, y, z);
        const double n0 = nrm[s], n1 = nrm[s + 1], n2 = nrm[s + 2];
        out_xyz[o] = x, out_xyz[o + 1] = y, out_xyz[o + 2] = z;
        out_nrm[o] = (float)(d->R[0] * n0 + (d->R[1] * n1 + d->R[2] * n2));
        out_nrm[o + 1] = (float)(d->R[3] * n0 + (d->R[4] * n1 + d->R[5] * n2));
        out_nrm[o + 2] = (float)(d->R[6] * n0 + (d->R[7] * n1 + d->R[8] * n2));
        if (kCull) keep = !asm_culled(x, y, z, cx, cy, cz, r2);
    }
    if (kCull) {
        __shared__ uint32_t wave_kept[kAsmWaves];
        const unsigned long long b = __ballot(keep);
        if ((threadIdx.x & 63u) == 0u) wave_kept[threadIdx.x >> 6] = (uint32_t)__popcll(b);
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t sum = 0;
            for (uint32_t w = 0; w < kAsmWaves; w++) sum += wave_kept[w];
            counts[d->blk + blockIdx.x] = sum;
        }
    }
}

// offsets[k] = counts[0] + ... + counts[k - 1] for k = 0 .. count (offsets[count]: the kept total).  One workgroup walks
// the matrix in (scan, block) order, kAsmOffsetThreads entries at a time: a shuffle scan inside each wave, the waves'
// totals through LDS, the carry in a register.  Integers: the tree is fixed and exact.
__global__ __launch_bounds__(kAsmOffsetThreads) void k_asm_offsets(const uint32_t *__restrict__ counts, uint32_t count,
                                                                   uint32_t *__restrict__ offsets)
{
    constexpr uint32_t kWaves = kAsmOffsetThreads / 64;
    __shared__ uint32_t wave_total[kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < count; base += kAsmOffsetThreads) {
        const uint32_t k = base + threadIdx.x;
        const uint32_t v = k < count ? counts[k] : 0u;
        uint32_t incl = v;
        for (uint32_t step = 1; step < 64; step <<= 1) {
            const uint32_t up = __shfl_up(incl, step, 64);
            if (lane >= step) incl += up;
        }
        if (lane == 63u) wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < kWaves; w++) {
            const uint32_t t = wave_total[w];
            if (w < wave) before += t;
            all += t;
        }
        if (k < count) offsets[k] = carry + before + (incl - v);
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[count] = carry;
}

// The kept points of the staged, transformed cloud to their places: workgroup (scan, block) starts at its prefix and
// ranks its points by wave ballot and popcount, so the order of the concatenation is kept and nobody waits for anybody.
// It reads the staged points (24 bytes per point, the same as the archive's) and not the archive again: the predicate
// is defined on the rounded f32 result, which the staging buffer holds, and the f64 transform is not paid twice.
__global__ __launch_bounds__(kAsmThreads) void k_asm_compact(const AsmScan *scans, const float *__restrict__ in_xyz,
                                                             const float *__restrict__ in_nrm, float cx, float cy, float cz,
                                                             float r2, const uint32_t *__restrict__ offsets,
                                                             float *__restrict__ out_xyz, float *__restrict__ out_nrm)
{
    const ConstAsm d = (ConstAsm)(scans + blockIdx.y);
    const uint32_t n = d->n, first = blockIdx.x * kAsmThreads;
    if (first >= n) return;
    __shared__ uint32_t wave_kept[kAsmWaves];
    const uint32_t i = first + threadIdx.x, wave = threadIdx.x >> 6;
    float x = 0.f, y = 0.f, z = 0.f;
    size_t s = 0;
    bool keep = false;
    if (i < n) {
        s = ((size_t)d->out + i) * 3;
        x = in_xyz[s], y = in_xyz[s + 1], z = in_xyz[s + 2];
        keep = !asm_culled(x, y, z, cx, cy, cz, r2);
    }
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63u) == 0u) wave_kept[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!keep) return;
    uint32_t at = offsets[d->blk + blockIdx.x] + asm_rank(b);
    for (uint32_t w = 0; w < kAsmWaves; w++)
        if (w < wave) at += wave_kept[w];
    const size_t o = (size_t)at * 3;
    out_xyz[o] = x, out_xyz[o + 1] = y, out_xyz[o + 2] = z;
    out_nrm[o] = in_nrm[s], out_nrm[o + 1] = in_nrm[s + 1], out_nrm[o + 2] = in_nrm[s + 2];
}

}  // namespace lom
