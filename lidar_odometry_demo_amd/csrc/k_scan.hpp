// Generic exclusive prefix scan in global memory (the multi-launch fallback of the map's single-pass kernels): k_scan_tile,
// k_scan_add and the host recursion scan_exclusive.  Device code only; voxel_map.hip is the one translation unit
// that instantiates and launches it -- the other map files scan through its scan_u32 / scan_u64 (map_internal.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grid_scan.hpp"
#include "lom_internal.hpp"

namespace lom {

// ---------------------------------------------------------------------------
// exclusive prefix scan of uint32 (tile = 256 threads x 8 items)
// ---------------------------------------------------------------------------
constexpr int kScanItems = 8;
constexpr int kScanTile = kThreads * kScanItems;

template <typename T>
__global__ __launch_bounds__(kThreads) void k_scan_tile(const T *__restrict__ in, T *__restrict__ out,
                                                        T *__restrict__ tile_sums, uint32_t n)
{
    __shared__ T s_wave[kThreads / 64];
    const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    T v[kScanItems];
    T sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        v[k] = (base + k < n) ? in[base + k] : T(0);
        sum += v[k];
    }
    // inclusive scan of per-thread sums inside the wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    T wave_off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) {
        if (w < wave) wave_off += s_wave[w];
        total += s_wave[w];
    }
    T run = wave_off + inc - sum;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

template <typename T>
__global__ void k_scan_add(T *__restrict__ out, const T *__restrict__ tile_prefix, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] += tile_prefix[i / kScanTile];
}

// out[i] = sum in[0..i), *d_total = sum of all.  tmp must hold scan_tmp_words(n) elements of T.
// T = uint64 scans two packed uint32 quantities at once (no carry while the low sum < 2^32).
template <typename T>
static int scan_exclusive(lom_map *m, const T *in, T *out, uint32_t n, T *d_total, T *tmp)
{
    const uint32_t nt = (n + kScanTile - 1) / kScanTile;
    if (nt <= 1) {
        hipLaunchKernelGGL(k_scan_tile<T>, dim3(1), dim3(kThreads), 0, m->stream, in, out, d_total, n);
        LOM_HIP(m, hipGetLastError());
        return LOM_OK;
    }
    T *sums = tmp, *prefix = tmp + nt;
    hipLaunchKernelGGL(k_scan_tile<T>, dim3(nt), dim3(kThreads), 0, m->stream, in, out, sums, n);
    LOM_HIP(m, hipGetLastError());
    int rc = scan_exclusive<T>(m, sums, prefix, nt, d_total, tmp + 2 * (size_t)nt);
    if (rc != LOM_OK) return rc;
    hipLaunchKernelGGL(k_scan_add<T>, dim3(blocks_for(n)), dim3(kThreads), 0, m->stream, out, prefix, n);
    LOM_HIP(m, hipGetLastError());
    return LOM_OK;
}

}  // namespace lom
