// The streaming insert (batches up to kOnePassMax points, and the fallback of everything else): k_ins_claim2 /
// assign2 / scatter2 / place2, and k_ins_heads / k_ins_assign of its multi-launch form.  Device code only; map_insert.hip is the one translation unit
// that instantiates and launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grid_scan.hpp"
#include "lom_internal.hpp"
#include "table_device.hpp"

namespace lom {

// ---------------------------------------------------------------------------
// insert kernels
// ---------------------------------------------------------------------------
// per point: low word = 1 if it is the first point of a voxel seen for the first time (creation
// order = order of first appearance, voxel_grid.h:83-87), high word = size of the voxel's bucket
// if the point is the bucket's head.  One 64-bit exclusive scan then yields the new voxel's slab
// rank and the bucket's offset in the scratch list -- no same-address atomics.
__global__ void k_ins_heads(const Slot *table, uint32_t n, const uint32_t *pt_slot, const uint32_t *bkt_cnt,
                            const uint32_t *bkt_head, unsigned long long *flag64, uint32_t seq, const uint32_t *words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = pt_slot[i];
    unsigned long long f = 0;
    if (words[MW_RANGE] != seq && h != 0xFFFFFFFFu && bkt_head[h] == i) {
        f = (unsigned long long)bkt_cnt[h] << 32;
        if (table[h].slab == kNoSlab) f |= 1ull;  // voxel_grid.h:83 it == end()
    }
    flag64[i] = f;
}

__global__ void k_ins_assign(Slot *table, uint32_t n, const uint32_t *pt_slot, const uint32_t *bkt_head,
                             const unsigned long long *flag64, const unsigned long long *scan64,
                             const uint32_t *n_vox_dev, unsigned long long *slab_key, uint32_t *bkt_off,
                             uint32_t *bkt_old, uint32_t seq, const uint32_t *words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || words[MW_RANGE] == seq) return;
    const uint32_t h = pt_slot[i];
    if (h == 0xFFFFFFFFu || bkt_head[h] != i) return;
    const uint32_t n_vox_before = *n_vox_dev;  // device-side voxel counter (bumped by k_ins_place2)
    const unsigned long long sc = scan64[i];
    bkt_off[h] = (uint32_t)(sc >> 32);
    bkt_old[h] = (flag64[i] & 1ull) ? 0u : table[h].count;
    if (flag64[i] & 1ull) {
        const uint32_t slab = n_vox_before + (uint32_t)sc;
        table[h].slab = slab;
        slab_key[slab] = table[h].key;
    }
}

// ---- insert, four kernels ----------------------------------------------------------------------
// 1. k_ins_claim2   slot per point (CAS), arrival position in the voxel's bucket, earliest input index;
//                   range check folded in (a call with a bad point inserts nothing: the later kernels
//                   see the call's sequence number in the error word and only put the scratch to rest)
// 2. k_ins_assign2  one 64-bit scan: creation order of the new voxels (low word) and bucket offsets
//                   (high word); the head point of a voxel assigns slab, offset and the old count
// 3. k_ins_scatter2 bucket lists; every point takes a private copy of its bucket's size and offset
// 4. k_ins_place2   rank by input index inside the voxel (= insertion order, voxel_grid.h:86-90), store
//                   the first K - count; the head point publishes the new count and resets the scratch
__global__ __launch_bounds__(kThreads) void k_ins_claim2(Slot *table, uint32_t mask, uint32_t shift, const char *xyz,
                                                         size_t stride, uint32_t n, float vs, uint32_t *pt_slot,
                                                         uint32_t *pt_pos, uint32_t *bkt_cnt, uint32_t *bkt_head,
                                                         uint32_t seq, uint32_t *words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = point_at(xyz, i, stride);
    int ix = 0, iy = 0, iz = 0;
    if (!voxel_index(p[0], vs, ix) || !voxel_index(p[1], vs, iy) || !voxel_index(p[2], vs, iz)) {
        pt_slot[i] = kInvalidSlot;
        __hip_atomic_store(words + MW_RANGE, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // LOM_ERR_RANGE for this call
        return;
    }
    const uint32_t h = claim_slot(table, mask, shift, pack_key(ix, iy, iz));
    pt_slot[i] = h;
    pt_pos[i] = atomicAdd(&bkt_cnt[h], 1u);  // arbitrary order; fixed up by rank in k_ins_place2
    atomicMin(&bkt_head[h], i);              // earliest input index touching the voxel
}

__global__ __launch_bounds__(kThreads) void k_ins_assign2(Slot *table, uint32_t n, const uint32_t *__restrict__ pt_slot,
                                                          const uint32_t *__restrict__ bkt_cnt,
                                                          const uint32_t *__restrict__ bkt_head, uint32_t *bkt_off,
                                                          uint32_t *bkt_old, const uint32_t *n_vox_dev,
                                                          unsigned long long *slab_key, Granule *agg, uint32_t seq,
                                                          uint32_t *words, uint32_t test_fail_from)
{
    __shared__ unsigned long long s_w[8];
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const bool failed = words[MW_RANGE] == seq;  // a point of this call was out of range: nothing is inserted
    uint32_t h = kInvalidSlot;
    bool is_head = false, is_new = false;
    uint32_t old_count = 0, m = 0;
    if (i < n && !failed) {
        h = pt_slot[i];
        is_head = bkt_head[h] == i;
        if (is_head) {
            const Slot s = table[h];
            is_new = s.slab == kNoSlab;  // voxel_grid.h:83 it == end()
            old_count = is_new ? 0u : s.count;
            m = bkt_cnt[h];
        }
    }
    unsigned long long total;
    const unsigned long long v = ((unsigned long long)m << 32) | (is_new ? 1ull : 0ull);
    const unsigned long long excl = block_scan64(v, s_w, total);
    bool gave_up;
    const unsigned long long before = grid_prefix64(total, agg, seq, words + MW_GRID, s_w, gave_up, test_fail_from);
    // A workgroup without a prefix assigns nothing; what the others assigned before the give-up is taken back by
    // k_ins_place2 (slab ids at or beyond the voxel counter, which such a call does not advance).
    if (is_head && !gave_up) {
        const unsigned long long at = before + excl;
        bkt_off[h] = (uint32_t)(at >> 32);
        bkt_old[h] = old_count;
        if (is_new) {
            const uint32_t slab = *n_vox_dev + (uint32_t)at;  // creation order = order of first appearance
            table[h].slab = slab;
            slab_key[slab] = table[h].key;
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 && !gave_up) words[MW_NEW_VOX] = (uint32_t)(before + total);  // new voxels of this call
}

__global__ __launch_bounds__(kThreads) void k_ins_scatter2(uint32_t n, const uint32_t *__restrict__ pt_slot,
                                                           const uint32_t *__restrict__ pt_pos,
                                                           const uint32_t *__restrict__ bkt_off,
                                                           const uint32_t *__restrict__ bkt_cnt, uint32_t *items,
                                                           uint32_t *pt_off, uint32_t *pt_m, uint32_t seq,
                                                           const uint32_t *words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || words[MW_RANGE] == seq || words[MW_GRID] == seq) return;  // a call that failed (range / grid give-up) inserts nothing
    const uint32_t h = pt_slot[i];
    const uint32_t off = bkt_off[h];
    items[off + pt_pos[i]] = i;
    pt_off[i] = off;
    pt_m[i] = bkt_cnt[h];
}

__global__ __launch_bounds__(kThreads) void k_ins_place2(Slot *table, uint32_t n, const uint32_t *__restrict__ pt_slot,
                                                         const uint32_t *__restrict__ pt_off,
                                                         const uint32_t *__restrict__ pt_m, uint32_t *bkt_cnt,
                                                         uint32_t *bkt_head, const uint32_t *__restrict__ bkt_old,
                                                         const uint32_t *__restrict__ items, const char *xyz,
                                                         const char *nrm, size_t stride, uint32_t K, uint32_t cap_points,
                                                         float *pts, float *nrm_out, uint32_t *slab_count,
                                                         uint32_t *n_vox_dev, uint32_t seq, const uint32_t *words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = pt_slot[i];
    if (h == kInvalidSlot) return;
    const bool is_head = bkt_head[h] == i;  // only this thread resets the word, and only after this read
    if (words[MW_GRID] == seq) {
        // the scan of k_ins_assign2 gave up part-way: take back the slab ids the workgroups before the give-up
        // handed to NEW voxels (at or beyond the voxel counter, which this call does not advance), so that the
        // table is what it was before the call -- apart from claimed keys without a voxel, as after a range error
        if (is_head) {
            const uint32_t slab = table[h].slab;
            if (slab != kNoSlab && slab >= *n_vox_dev) table[h].slab = kNoSlab;
        }
    } else if (words[MW_RANGE] != seq) {
        const uint32_t old = bkt_old[h];
        const uint32_t slab = table[h].slab;
        const uint32_t m = pt_m[i];
        // voxel_grid.h:86,89-90: a voxel takes points while size() < max_points_ (cap_points; the row stride K is at least
        // that, and a voxel filled under a larger max_points_ keeps what it holds)
        const uint32_t room = cap_points > old ? cap_points - old : 0u;
        if (room) {
            const uint32_t *it = items + pt_off[i];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < m && rank < room; j++) rank += it[j] < i;
            if (rank < room) {  // voxel_grid.h:86,89-90: append while size() < max_points_, in input order
                const size_t dst = ((size_t)slab * K + old + rank) * 3;
                const Point3 pv = load3(point_at(xyz, i, stride));
                Point3 nv = {0.f, 0.f, 0.f};  // voxel_grid.h:103,107: no normals -> (0, 0, 0)
                if (nrm) nv = load3(point_at(nrm, i, stride));
                store3(pts + dst, pv);
                store3(nrm_out + dst, nv);
            }
        }
        if (is_head) {
            const uint32_t nc = old + (m < room ? m : room);
            table[h].count = nc;
            slab_count[slab] = nc;
        }
        if (i == 0) *n_vox_dev += words[MW_NEW_VOX];  // point 0 is always the head of its voxel's bucket... and exists once
    }
    if (is_head) {  // scratch back to rest
        bkt_cnt[h] = 0u;
        bkt_head[h] = 0xFFFFFFFFu;
    }
}

}  // namespace lom
