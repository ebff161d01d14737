// The fused down-sampler (k_ds_*), the export (k_export_*) and k_transform.  Device code only; map_cloud.hip is the one translation unit
// that instantiates and launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grid_scan.hpp"
#include "lom_internal.hpp"
#include "table_device.hpp"

namespace lom {

// ---------------------------------------------------------------------------
// fused down-sampler: VoxelGrid(voxel, 1).addCloud(cloud) followed by getCloud() /
// getCloudWithoutNormals() (the reference's idiom, lidar_odometry.cpp:37-38,42,46-47,50) keeps
// the FIRST point of every voxel in input order and returns them in order of first appearance.
// That is: claim a slot per voxel, take the minimum input index per slot, keep the points whose
// index is that minimum, compact them by a scan over the input.  No payload slabs are touched.
// ---------------------------------------------------------------------------
// n_dev (optional): the number of input points when only the device knows it (n is then its upper bound)
__global__ void k_ds_claim(Slot *table, uint32_t mask, uint32_t shift, const char *xyz, size_t stride, uint32_t n,
                           const uint32_t *n_dev, float vs, uint32_t *pt_slot, uint32_t *head, uint32_t seq, uint32_t *bad)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (n_dev) n = min(n, *n_dev);
    if (i >= n) return;
    const float *p = point_at(xyz, i, stride);
    int ix = 0, iy = 0, iz = 0;
    if (!voxel_index(p[0], vs, ix) || !voxel_index(p[1], vs, iy) || !voxel_index(p[2], vs, iz)) {
        __hip_atomic_store(bad, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // out of range / not finite: the call fails
        pt_slot[i] = 0xFFFFFFFFu;
        return;
    }
    const uint32_t h = claim_slot(table, mask, shift, pack_key(ix, iy, iz));
    pt_slot[i] = h;
    atomicMin(&head[h], i);
}

__global__ void k_ds_flag(uint32_t n, const uint32_t *pt_slot, const uint32_t *head, uint32_t *flag)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint32_t h = pt_slot[i];
        flag[i] = (h != 0xFFFFFFFFu && head[h] == i) ? 1u : 0u;
    }
}

__global__ void k_ds_write(uint32_t n, const uint32_t *flag, const uint32_t *rank, const char *xyz, const char *nrm,
                           size_t stride, float *out_xyz, float *out_nrm, Slot *table, const uint32_t *pt_slot,
                           uint32_t *head)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    {  // the workspace goes back to rest: the kept point frees its voxel's slot and head word
        const uint32_t h = pt_slot[i];
        Slot e;
        e.key = kEmptyKey;
        e.count = 0;
        e.slab = kNoSlab;
        table[h] = e;
        head[h] = 0xFFFFFFFFu;
    }
    const size_t d = (size_t)rank[i] * 3;
    const float *p = point_at(xyz, i, stride);
    out_xyz[d] = p[0];
    out_xyz[d + 1] = p[1];
    out_xyz[d + 2] = p[2];
    if (out_nrm) {
        if (nrm) {
            const float *q = point_at(nrm, i, stride);
            out_nrm[d] = q[0];
            out_nrm[d + 1] = q[1];
            out_nrm[d + 2] = q[2];
        } else {
            out_nrm[d] = out_nrm[d + 1] = out_nrm[d + 2] = 0.f;
        }
    }
}

// ---------------------------------------------------------------------------
// Single-pass variants for per-frame sizes (n <= kOnePassMax): one element per thread, at most 256
// workgroups of 256, all resident at once.  What used to be {flag kernel, 1-3 scan launches, consumer
// kernel} is one kernel: block-local scan, then every workgroup publishes its total as a tagged 8-byte
// word {call sequence number, value} (one store; no reset between calls, the sequence number tells
// fresh from stale) and adds up the totals of the workgroups before it -- <= 255 words, one per
// thread, fixed order, so the prefix is deterministic.  Every wait is bounded (s_memrealtime); a
// workgroup that gives up writes the call's sequence number into the error word and carries on
// with a zero prefix: the host sees the error at its next read-back.
//
// Per-slot scratch (batch count, earliest input index, down-sampler head) is kept "at rest" between
// calls -- zero / 0xFFFFFFFF everywhere -- by the one thread per voxel that consumed it, so no call
// pays a memset proportional to the table capacity.
// ---------------------------------------------------------------------------
// ---- down-sampler, two kernels ------------------------------------------------------------------
// k_ds_claim (above) leaves pt_slot[] and head[]; this kernel keeps the first point of every voxel in
// order of first appearance and puts the workspace back to rest: the head point of a voxel frees its
// table slot and its head word, so neither a table re-initialisation nor a memset follows.
template <int kItems>  // consecutive points per thread: 1 up to 65536 points, 4 up to 262144
__global__ __launch_bounds__(kThreads) void k_ds_emit(Slot *table, uint32_t n, const uint32_t *n_dev,
                                                      const uint32_t *__restrict__ pt_slot, uint32_t *head, const char *xyz,
                                                      const char *nrm, size_t stride, float *out_xyz, float *out_nrm,
                                                      Granule *agg, uint32_t seq, uint32_t *words, uint32_t test_fail_from)
{
    __shared__ unsigned long long s_w[8];
    const uint32_t base = (blockIdx.x * kThreads + threadIdx.x) * kItems;
    if (n_dev) n = min(n, *n_dev);
    uint32_t h[kItems];
    bool keep[kItems];
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const uint32_t i = base + k;
        h[k] = kInvalidSlot;
        keep[k] = false;
        if (i < n) {
            h[k] = pt_slot[i];
            keep[k] = h[k] != kInvalidSlot && head[h[k]] == i;
        }
        mine += keep[k] ? 1u : 0u;
    }
    unsigned long long total;
    const unsigned long long excl = block_scan64(mine, s_w, total);
    bool gave_up;
    const unsigned long long before = grid_prefix64(total, agg, seq, words + MW_GRID, s_w, gave_up, test_fail_from);
    uint32_t at = (uint32_t)(before + excl);
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        if (!keep[k]) continue;
        const uint32_t i = base + k;
        const size_t d = (size_t)at * 3;
        at++;
        if (!gave_up) {  // without a prefix there is no place to write to; the workspace still goes back to rest below
            const float *p = point_at(xyz, i, stride);
            out_xyz[d] = p[0];
            out_xyz[d + 1] = p[1];
            out_xyz[d + 2] = p[2];
            if (out_nrm) {
                if (nrm) {
                    const float *q = point_at(nrm, i, stride);
                    out_nrm[d] = q[0];
                    out_nrm[d + 1] = q[1];
                    out_nrm[d + 2] = q[2];
                } else {
                    out_nrm[d] = out_nrm[d + 1] = out_nrm[d + 2] = 0.f;
                }
            }
        }
        Slot e;
        e.key = kEmptyKey;
        e.count = 0;
        e.slab = kNoSlab;
        table[h[k]] = e;
        head[h[k]] = 0xFFFFFFFFu;
    }
    // voxels kept; a grid that gave up reports none (whoever consumes the count on the device finds an empty cloud)
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) words[MW_COUNT] = gave_up ? 0u : (uint32_t)(before + total);
}

// ---------------------------------------------------------------------------
// export kernels
// ---------------------------------------------------------------------------
__global__ void k_export_counts(const uint32_t *slab_count, uint32_t n_vox, int mode, uint32_t *out)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_vox) out[s] = (mode == LOM_EXPORT_FIRST_PER_VOXEL) ? (slab_count[s] ? 1u : 0u) : slab_count[s];  // (empty slab: erased voxel)
}

__global__ void k_export_write(const uint32_t *off, const uint32_t *slab_count, uint32_t n_vox, uint32_t K,
                               int mode, const float *pts, const float *nrm, float *out_xyz, float *out_nrm)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n_vox * K) return;
    const uint32_t s = (uint32_t)(idx / K), j = (uint32_t)(idx % K);
    const uint32_t c = (mode == LOM_EXPORT_FIRST_PER_VOXEL) ? (slab_count[s] ? 1u : 0u) : slab_count[s];
    if (j >= c) return;
    const size_t a = ((size_t)s * K + j) * 3, b = ((size_t)off[s] + j) * 3;
    out_xyz[b] = pts[a];
    out_xyz[b + 1] = pts[a + 1];
    out_xyz[b + 2] = pts[a + 2];
    if (out_nrm) {
        out_nrm[b] = nrm[a];
        out_nrm[b + 1] = nrm[a + 1];
        out_nrm[b + 2] = nrm[a + 2];
    }
}

// CloudTransformer::transform / transformWithNormals (utils/cloud_transform.h:43-97) on the device:
// the same f32 expressions as lom_transform_points, R and t prepared on the host
struct RigidArgs {
    float R[9], t[3];
};
__global__ void k_transform(const char *xyz, const char *nrm, size_t stride, uint32_t n, RigidArgs A, float *out_xyz,
                            float *out_nrm)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = point_at(xyz, i, stride);
    const float p0 = p[0], p1 = p[1], p2 = p[2];
    float *o = out_xyz + (size_t)i * 3;
    o[0] = (A.R[0] * p0 + (A.R[1] * p1 + A.R[2] * p2)) + A.t[0];
    o[1] = (A.R[3] * p0 + (A.R[4] * p1 + A.R[5] * p2)) + A.t[1];
    o[2] = (A.R[6] * p0 + (A.R[7] * p1 + A.R[8] * p2)) + A.t[2];
    if (nrm && out_nrm) {
        const float *q = point_at(nrm, i, stride);
        const float n0 = q[0], n1 = q[1], n2 = q[2];
        float *no = out_nrm + (size_t)i * 3;
        no[0] = A.R[0] * n0 + (A.R[1] * n1 + A.R[2] * n2);
        no[1] = A.R[3] * n0 + (A.R[4] * n1 + A.R[5] * n2);
        no[2] = A.R[6] * n0 + (A.R[7] * n1 + A.R[8] * n2);
    }
}

}  // namespace lom
