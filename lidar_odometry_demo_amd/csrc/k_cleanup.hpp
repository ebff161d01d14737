// radiusCleanup: k_cleanup_flag / mark / scan and k_compact.  Device code only; map_erase.hip is the one translation unit
// that instantiates and launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grid_scan.hpp"
#include "lom_internal.hpp"

namespace lom {

// ---------------------------------------------------------------------------
// cleanup kernels
// ---------------------------------------------------------------------------
// voxel_grid.h:238-241: erase iff (getOrigin() - point).squaredNorm() > radius_sq (f32, strict)
// (a slab with no points is a voxel an earlier cleanup erased -- k_cleanup_mark --: not kept, not counted)
__global__ void k_cleanup_flag(const float *pts, const uint32_t *slab_count, uint32_t K, uint32_t n_vox, float cx, float cy,
                               float cz, float r2, uint32_t *keep)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_vox) return;
    const float *o = pts + (size_t)s * K * 3;  // voxel_with_planes.h:32-35 front()
    const float dx = o[0] - cx, dy = o[1] - cy, dz = o[2] - cz;
    const float d2 = dx * dx + (dy * dy + dz * dz);
    keep[s] = (slab_count[s] == 0u || d2 > r2) ? 0u : 1u;
}

// voxel_grid.h:240 erase(it), without moving anybody: the erased voxel's slab keeps its place in the creation order with no
// points in it, and its key stays in the table as a claimed slot without a voxel (slab == kNoSlab, count 0 -- what a
// range error leaves behind, too): a search finds no candidates there, an insert finds "it == end()" (voxel_grid.h:83)
// and creates the voxel anew at the end of the creation order, exactly as after an erase.  Exports skip empty slabs.
// The holes are closed (k_compact, table rebuilt) once they are a quarter of the slabs.
__global__ void k_cleanup_mark(Slot *table, uint32_t mask, uint32_t shift, const uint32_t *__restrict__ keep, uint32_t n_vox,
                               const unsigned long long *__restrict__ slab_key, uint32_t *slab_count)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_vox || keep[s] || slab_count[s] == 0u) return;
    const unsigned long long key = slab_key[s];
    uint32_t h = hash_key(key, shift) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++) {  // (the key is there: its voxel was live)
        const unsigned long long seen = table[h].key;
        if (seen == key) {
            table[h].count = 0u;
            table[h].slab = kNoSlab;
            break;
        }
        if (seen == kEmptyKey) break;
        h = (h + 1) & mask;
    }
    slab_count[s] = 0u;
}

// the same flags and their exclusive scan in one kernel (kItems consecutive voxels per thread, <= 256
// workgroups): keep[], newid[] and the number of voxels kept (words[MW_COUNT])
// `from`: the scan was enqueued behind an align on the same stream (lom_map_radius_cleanup_after_align) and takes its
// centre from the pose that align ended with -- lidar_odometry.cpp:65-67: current_transform_ = result, then
// radiusCleanup(current_transform_.translation, ...).  An align that has not ended there (more outer iterations to
// come, a give-up) leaves words[MW_SPEC_SEQ] = 0 and the scan undone; otherwise it is seq and words[MW_SPEC_CX..CZ] = the bits of
// the centre used: the host takes the result only for exactly the centre it would have passed.  keep[] / newid[] are
// scratch either way.
template <int kItems>
__global__ __launch_bounds__(kThreads) void k_cleanup_scan(const float *pts, const uint32_t *slab_count, uint32_t K,
                                                           uint32_t n_vox, float cx, float cy,
                                                           float cz, float r2, uint32_t *keep, uint32_t *newid,
                                                           Granule *agg, uint32_t seq, uint32_t *words, uint32_t test_fail_from,
                                                           const AlignState *from = nullptr)
{
    __shared__ unsigned long long s_w[8];
    if (from) {  // (uniform over the grid: the align's kernels are through)
        typedef const __attribute__((address_space(4))) AlignState *ConstState;
        ConstState cs = (ConstState)(from);
        const int usable = cs->finished && !cs->error;
        cx = cs->pose_t[0];
        cy = cs->pose_t[1];
        cz = cs->pose_t[2];
        if (!usable) {
            if (blockIdx.x == 0 && threadIdx.x == 0) words[MW_SPEC_SEQ] = 0u;
            return;
        }
    }
    const uint32_t base = (blockIdx.x * kThreads + threadIdx.x) * kItems;
    uint32_t f[kItems], mine = 0;
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const uint32_t s = base + k;
        f[k] = 0;
        if (s < n_vox) {
            const float *o = pts + (size_t)s * K * 3;  // voxel_with_planes.h:32-35 front()
            const float dx = o[0] - cx, dy = o[1] - cy, dz = o[2] - cz;
            const float d2 = dx * dx + (dy * dy + dz * dz);
            f[k] = (slab_count[s] == 0u || d2 > r2) ? 0u : 1u;  // voxel_grid.h:238-241 (an empty slab: erased before)
        }
        mine += f[k];
    }
    unsigned long long total;
    const unsigned long long excl = block_scan64(mine, s_w, total);
    bool gave_up;
    const unsigned long long before = grid_prefix64(total, agg, seq, words + MW_GRID, s_w, gave_up, test_fail_from);
    uint32_t run = (uint32_t)(before + excl);
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const uint32_t s = base + k;
        if (s < n_vox && !gave_up) {  // keep[] / newid[] are scratch: the host redoes a scan that gave up
            keep[s] = f[k];
            newid[s] = run;
        }
        run += f[k];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        words[MW_COUNT] = (uint32_t)(before + total);
        if (from) {
            words[MW_SPEC_CX] = __float_as_uint(cx);
            words[MW_SPEC_CY] = __float_as_uint(cy);
            words[MW_SPEC_CZ] = __float_as_uint(cz);
            words[MW_SPEC_SEQ] = seq;
        }
    }
}

__global__ void k_compact(const uint32_t *keep, const uint32_t *newid, uint32_t n_vox, uint32_t K,
                          const unsigned long long *key_in, const uint32_t *cnt_in, const float *pts_in,
                          const float *nrm_in, unsigned long long *key_out, uint32_t *cnt_out, float *pts_out,
                          float *nrm_out, uint32_t *n_vox_dev, uint32_t n_keep)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0) *n_vox_dev = n_keep;  // the device-side voxel counter follows the compaction
    if (idx >= (size_t)n_vox * K) return;
    const uint32_t s = (uint32_t)(idx / K), j = (uint32_t)(idx % K);
    if (!keep[s]) return;
    const uint32_t d = newid[s];
    const uint32_t c = cnt_in[s];
    if (j == 0) {
        key_out[d] = key_in[s];
        cnt_out[d] = c;
    }
    if (j < c) {
        const size_t a = ((size_t)s * K + j) * 3, b = ((size_t)d * K + j) * 3;
        pts_out[b] = pts_in[a];
        pts_out[b + 1] = pts_in[a + 1];
        pts_out[b + 2] = pts_in[a + 2];
        nrm_out[b] = nrm_in[a];
        nrm_out[b + 1] = nrm_in[a + 1];
        nrm_out[b + 2] = nrm_in[a + 2];
    }
}

}  // namespace lom
