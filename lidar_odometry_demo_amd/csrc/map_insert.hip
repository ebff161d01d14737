// The voxel map's insert (voxel_grid.h:77-110, addCloud / addCloudWithoutNormals): the single-pass path for per-frame
// batches, its multi-launch form (the redo of a call whose in-kernel scan gave up, and everything the other two do not
// take), and the bulk path for batches above kOnePassMax points.  This file is the one translation unit that
// instantiates and launches the kernels of k_insert.hpp and k_bulk_insert.hpp; table, slabs, status words and the
// pending / redo protocol are voxel_map.hip (map_internal.hpp).
//
// Built with -ffp-contract=off (see voxel_map.hip).
#include <algorithm>
#include <mutex>

#include "grid_scan.hpp"
#include "k_bulk_insert.hpp"
#include "k_insert.hpp"
#include "lom_internal.hpp"
#include "map_internal.hpp"

namespace lom {

// Table size after a bulk insert: 16..32 slots per voxel (LOM_TABLE_SLOTS_PER_VOXEL at create).  The search's probe
// phase pays for every collision with a dependent round trip, and a longer table costs nothing but memory: k_match on
// C2 / C3 / C4 with 4 slots per voxel (rounds 1-2) 7.5 / 25.1 / 43.2 us, 8: 7.5 / 24.0 / 41.1, 16: 7.2 / 23.9 / 40.7,
// 32: 7.2 / 23.8 / 40.6, 64: 7.2 / 23.4 / 40.8 (same box, tools/ab_match.py).
static int shrink_after_bulk(lom_map *m)
{
    if ((uint64_t)m->cap < 16ull * std::max<uint32_t>(m->min_cap, 1u)) return LOM_OK;
    int rc = refresh_nvox(m);
    if (rc != LOM_OK) return rc;
    const uint32_t target = std::max(m->min_cap, next_pow2((uint64_t)m->table_slots_per_voxel * m->n_vox));
    return m->cap > target ? rehash(m, target) : LOM_OK;
}

struct BulkShape {
    uint32_t n_parts, part_shift, part_max, ppt, n_blk, n_words;
};

static BulkShape bulk_shape(uint32_t N, uint32_t cap, uint32_t ppt_override = 0)
{
    BulkShape b;
    // ~128 points per partition (the 512-point shape of k_bi_group: 20 KB of LDS, eight workgroups per CU) while the
    // partitions number at most kBiMaxParts; beyond 2 M points the partitions grow and the 1024-point shape takes over
    uint32_t np = 64;
    while (np < kBiMaxParts && (uint64_t)np * 128 < N) np <<= 1;
    b.n_parts = std::min(np, cap);
    b.part_shift = (uint32_t)__builtin_ctz(cap) - (uint32_t)__builtin_ctz(b.n_parts);
    b.part_max = (uint64_t)b.n_parts * 128 >= N ? 512u : kBiPartMax;
    b.ppt = N <= (1u << 20) ? 4u : 8u;
    if (ppt_override == 2 || ppt_override == 4 || ppt_override == 8) b.ppt = ppt_override;
    b.n_blk = (N + b.ppt * kBiThreads - 1) / (b.ppt * kBiThreads);
    b.n_words = (N + 31) / 32;
    return b;
}

static int bulk_scratch(lom_map *m, uint32_t N, const BulkShape &b)
{
    int rc;
    for (int s : {S_PT_OFF, S_PT_M, S_ENT_ROW})
        if ((rc = ensure(m, m->scr[s], (size_t)N * 4)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->scr[S_PT_SLOT], (size_t)N * sizeof(uint2))) != LOM_OK) return rc;
    if ((rc = ensure(m, m->scr[S_PT_POS], (size_t)N * sizeof(uint4))) != LOM_OK) return rc;
    drop_cleanup_behind_align(m);  // (the bitmap goes where its keep / newid are)
    if ((rc = ensure(m, m->scr[S_FLAG], (size_t)b.n_words * 4)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->scr[S_RANK], (size_t)b.n_words * 4)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->scr[S_HIST], (size_t)b.n_parts * b.n_blk * 4)) != LOM_OK) return rc;
    // partition sizes and starts, then the bitmap's tiles: totals, prefixes, and the counter of finished tiles (at rest: 0)
    const size_t tiles = (b.n_words + kBiTileWords - 1) / kBiTileWords;
    const bool fresh = m->scr[S_PART].bytes < (size_t)(2 * kBiMaxParts + 1 + 2 * 256 + 1) * 4;
    if ((rc = ensure(m, m->scr[S_PART], (size_t)(2 * kBiMaxParts + 1 + 2 * 256 + 1) * 4)) != LOM_OK) return rc;
    if (fresh) LOM_HIP(m, hipMemsetAsync(m->scr[S_PART].p, 0, m->scr[S_PART].bytes, m->stream));
    return tiles <= 256 ? LOM_OK : fail(m, LOM_ERR_ARG, "bulk insert: too many points");
}

// The instantiations of the bulk insert's templated kernels (every instantiation of a family has the same signature):
// k_bi_claim / k_bi_scatter by points per thread, k_bi_group by the points a partition may hold.
struct BulkPptForm {
    uint32_t ppt;
    decltype(&k_bi_claim<2>) claim;
    decltype(&k_bi_scatter<2>) scatter;
};
static const BulkPptForm kBulkPptForms[] = {
    {2, k_bi_claim<2>, k_bi_scatter<2>}, {4, k_bi_claim<4>, k_bi_scatter<4>}, {8, k_bi_claim<8>, k_bi_scatter<8>}};

static const BulkPptForm &bulk_ppt_form(uint32_t ppt)
{
    for (const BulkPptForm &f : kBulkPptForms)
        if (f.ppt == ppt) return f;
    return kBulkPptForms[2];
}

static decltype(&k_bi_group<512>) bulk_group_kernel(uint32_t part_max)
{
    return part_max == 512 ? k_bi_group<512> : k_bi_group<kBiPartMax>;
}

// batches above kOnePassMax points (see the kernels): everything is enqueued, nothing waits; the verdict -- range error,
// or a partition beyond k_bi_group's LDS, which sends the call to the four-kernel path -- is read with the call's status
static int add_points_bulk(lom_map *m, const char *d_xyz, const char *d_nrm, uint32_t N, size_t stride, uint64_t worst,
                           bool validated_on_host, bool sync_status, bool allow_shrink)
{
    int rc;
    const BulkShape b = bulk_shape(N, m->cap, m->bulk_ppt);
    if ((rc = bulk_scratch(m, N, b)) != LOM_OK) return rc;
    if (worst > m->slabs.cap && (rc = ensure_slabs(m, worst + worst / 2)) != LOM_OK) return rc;
    uint2 *pt_info = m->scr[S_PT_SLOT].as<uint2>();
    uint32_t *flag_bits = m->scr[S_FLAG].as<uint32_t>(), *word_prefix = m->scr[S_RANK].as<uint32_t>();
    uint4 *part_rec = m->scr[S_PT_POS].as<uint4>();
    uint32_t *ent_idx = m->scr[S_PT_OFF].as<uint32_t>(), *ent_w = m->scr[S_PT_M].as<uint32_t>();
    uint32_t *ent_row = m->scr[S_ENT_ROW].as<uint32_t>();
    uint32_t *hist = m->scr[S_HIST].as<uint32_t>();
    uint32_t *part_total = m->scr[S_PART].as<uint32_t>(), *part_start = part_total + kBiMaxParts;
    uint32_t *tile_total = part_start + kBiMaxParts + 1, *tile_prefix = tile_total + 256, *tiles_done = tile_prefix + 256;
    const uint32_t n_tiles = (b.n_words + kBiTileWords - 1) / kBiTileWords;
    uint32_t *words = d_words(m), *n_vox_dev = d_word(m, MW_NVOX);
    const uint32_t seq = ++m->call_seq;
    m->mutations++;
    const MapView v = view_of(m);
    const uint32_t part_max = m->test_bulk_part_max ? std::min<uint32_t>(m->test_bulk_part_max, b.part_max) : b.part_max;
    const size_t lds = (size_t)b.n_parts * 4;
    if (lds + 256 > 65536) {  // the histograms of 16,384 partitions fill the 64 KB a launch gets without asking
        static std::once_flag once;
        std::call_once(once, [] {
            const int want = (int)kBiMaxParts * 4;
            for (const BulkPptForm &f : kBulkPptForms) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(f.claim), hipFuncAttributeMaxDynamicSharedMemorySize, want);
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(f.scatter), hipFuncAttributeMaxDynamicSharedMemorySize, want);
            }
        });
    }
    const dim3 gb(b.n_blk), tb(kBiThreads);
    const BulkPptForm &form = bulk_ppt_form(b.ppt);
    hipLaunchKernelGGL(form.claim, gb, tb, lds, m->stream, m->d_table, v.mask, v.shift, d_xyz, stride, N, m->voxel_size,
                       pt_info, flag_bits, hist, b.n_parts, b.part_shift, n_vox_dev, seq, words);
    hipLaunchKernelGGL(k_bi_colscan, dim3((b.n_parts + 63) / 64), dim3(kBiThreads), 0, m->stream, hist, b.n_parts, b.n_blk,
                       part_total, part_max, seq, words);
    hipLaunchKernelGGL(form.scatter, gb, tb, lds, m->stream, N, pt_info, hist, b.n_parts, b.part_shift, part_total,
                       part_start, part_rec, seq, words);
    hipLaunchKernelGGL(bulk_group_kernel(b.part_max), dim3(b.n_parts), dim3(kThreads), 0, m->stream, m->d_table, part_start,
                       part_rec, m->max_points, flag_bits, ent_idx, ent_w, ent_row, seq, words);
    hipLaunchKernelGGL(k_bi_flagscan, dim3(n_tiles), dim3(kThreads), 0, m->stream, flag_bits, b.n_words, word_prefix,
                       tile_total, tile_prefix, tiles_done, words + MW_BULK_SCAN, seq, words);
    hipLaunchKernelGGL(k_bi_place, dim3(blocks_for(N)), dim3(kThreads), 0, m->stream, m->d_table, N, ent_idx, ent_w, ent_row,
                       flag_bits, word_prefix, tile_prefix, words + MW_BULK_SCAN, d_xyz, d_nrm, stride, m->K, m->slabs.pts,
                       m->slabs.nrm, m->slabs.key, m->slabs.count, n_vox_dev, seq, words);
    LOM_HIP(m, hipGetLastError());
    set_pending(m, d_xyz, d_nrm, N, stride, seq);  // (a partition too large: redone with the four-kernel path)
    note_insert_enqueued(m, worst);
    if (sync_status && (rc = map_status(m)) != LOM_OK) return rc;
    return allow_shrink ? shrink_after_bulk(m) : LOM_OK;
}

int add_points_device(lom_map *m, const char *d_xyz, const char *d_nrm, size_t n, size_t stride,
                      bool validated_on_host, bool sync_status, bool allow_shrink, bool multi_launch)
{
    if (m->parent) return fail(m, LOM_ERR_STATE, "a scan context has no map of its own");
    if (n == 0) return LOM_OK;
    if (n >= 0x7FFFFFFFull) return fail(m, LOM_ERR_ARG, "too many points in one call");
    const uint32_t N = (uint32_t)n;
    int rc;
    if ((rc = resolve_pending(m)) != LOM_OK) return rc;  // inserts apply in call order
    // 1. table capacity for the worst case (every point a new voxel); shrunk afterwards
    uint64_t worst = (uint64_t)m->n_vox_ub + N;
    if ((uint64_t)m->cap < 2 * worst) {
        if ((rc = refresh_nvox(m)) != LOM_OK) return rc;
        worst = (uint64_t)m->n_vox + N;
        if ((uint64_t)m->cap < 2 * worst && (rc = rehash(m, next_pow2(4 * worst))) != LOM_OK) return rc;
    }
    // 2. scratch
    const bool one_pass = N <= kOnePassMax && !multi_launch;
    if (N > kOnePassMax && N <= kBiMaxPoints && !multi_launch && !m->opt_no_bulk)
        return add_points_bulk(m, d_xyz, d_nrm, N, stride, worst, validated_on_host, sync_status, allow_shrink);
    uint32_t *pt_slot, *pt_pos, *pt_off, *pt_m, *items, *boff, *bold;
    unsigned long long *flag64 = nullptr, *scan64 = nullptr, *scan_tmp = nullptr;  // the multi-launch form's
    if ((rc = scratch(m, S_PT_SLOT, N, &pt_slot)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_PT_POS, N, &pt_pos)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_PT_OFF, N, &pt_off)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_PT_M, N, &pt_m)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_ITEMS, N, &items)) != LOM_OK) return rc;
    if ((rc = ensure_rest(m, m->scr[S_BKT_CNT], (size_t)m->cap * 4, 0)) != LOM_OK) return rc;
    if ((rc = ensure_rest(m, m->scr[S_BKT_HEAD], (size_t)m->cap * 4, 0xFF)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_BKT_OFF, m->cap, &boff)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_BKT_OLD, m->cap, &bold)) != LOM_OK) return rc;
    if (!one_pass && (rc = scan_temps(m, N, N, &flag64, &scan64, &scan_tmp)) != LOM_OK) return rc;
    uint32_t *bcnt = m->scr[S_BKT_CNT].as<uint32_t>(), *bhead = m->scr[S_BKT_HEAD].as<uint32_t>();
    uint32_t *words = d_words(m), *n_vox_dev = d_word(m, MW_NVOX);
    const uint32_t seq = ++m->call_seq;
    m->mutations++;
    const MapView v = view_of(m);
    const dim3 g(blocks_for(N)), b(kThreads);
    hipLaunchKernelGGL(k_ins_claim2, g, b, 0, m->stream, m->d_table, v.mask, v.shift, d_xyz, stride, N, m->voxel_size,
                       pt_slot, pt_pos, bcnt, bhead, seq, words);
    LOM_HIP(m, hipGetLastError());
    // Nothing below depends on a host decision: the slabs are grown for the worst case up front (memory is
    // not the constraint on a 288 GB device; the voxel counter lives on the device), so the call only
    // enqueues.  The exact voxel count is read back by whoever needs it (refresh_nvox).
    if (worst > m->slabs.cap && (rc = ensure_slabs(m, worst + worst / 2)) != LOM_OK) return rc;
    if (!one_pass) {
        // large batches: flags, one 64-bit scan (1-3 launches), assignment
        hipLaunchKernelGGL(k_ins_heads, g, b, 0, m->stream, m->d_table, N, pt_slot, bcnt, bhead, flag64, seq, words);
        LOM_HIP(m, hipGetLastError());
        unsigned long long *d_total64 = reinterpret_cast<unsigned long long *>(d_word(m, MW_TOTAL64));
        if ((rc = scan_u64(m, flag64, scan64, N, d_total64, scan_tmp)) != LOM_OK) return rc;
        hipLaunchKernelGGL(k_ins_assign, g, b, 0, m->stream, m->d_table, N, pt_slot, bhead, flag64, scan64, n_vox_dev,
                           m->slabs.key, boff, bold, seq, words);
    } else {
        hipLaunchKernelGGL(k_ins_assign2, g, b, 0, m->stream, m->d_table, N, pt_slot, bcnt, bhead, boff, bold, n_vox_dev,
                           m->slabs.key, d_agg(m), seq, words, take_test_fail_from(m));
        set_pending(m, d_xyz, d_nrm, n, stride, seq);  // (its scan gave up: redone with the multi-launch scan)
    }
    hipLaunchKernelGGL(k_ins_scatter2, g, b, 0, m->stream, N, pt_slot, pt_pos, boff, bcnt, items, pt_off, pt_m, seq, words);
    hipLaunchKernelGGL(k_ins_place2, g, b, 0, m->stream, m->d_table, N, pt_slot, pt_off, pt_m, bcnt, bhead, bold, items,
                       d_xyz, d_nrm, stride, m->K, m->max_points, m->slabs.pts, m->slabs.nrm, m->slabs.count, n_vox_dev, seq, words);
    LOM_HIP(m, hipGetLastError());
    note_insert_enqueued(m, worst);
    if (sync_status && (!validated_on_host || multi_launch)) {
        if ((rc = map_status(m)) != LOM_OK) return rc;
    }
    if (allow_shrink && N > kOnePassMax && (rc = shrink_after_bulk(m)) != LOM_OK) return rc;
    return LOM_OK;
}

}  // namespace lom

using namespace lom;

extern "C" {

int lom_map_add_points_device(lom_map *m, const float *d_xyz, const float *d_nrm, size_t n, size_t stride)
{
    if (!m || (n && !d_xyz) || stride < 12 || (stride & 3)) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    return add_points_device(m, (const char *)d_xyz, (const char *)d_nrm, n, stride, false, true);
}

int lom_map_add_points_device_nowait(lom_map *m, const float *d_xyz, const float *d_nrm, size_t n, size_t stride)
{
    if (!m || (n && !d_xyz) || stride < 12 || (stride & 3)) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    return add_points_device(m, (const char *)d_xyz, (const char *)d_nrm, n, stride, false, false);
}

int lom_profile_insert(lom_map *m, const float *d_xyz, const float *d_nrm, size_t n, size_t stride, double *total_us_out)
{
    if (!m || !d_xyz || !n || !total_us_out || stride < 12 || (stride & 3)) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    // capacity and scratch first, so that the bracket holds the insert's kernels only
    int rc = refresh_nvox(m);
    if (rc != LOM_OK) return rc;
    const uint64_t worst = (uint64_t)m->n_vox + n;
    if ((uint64_t)m->cap < 2 * worst && (rc = rehash(m, next_pow2(4 * worst))) != LOM_OK) return rc;
    if (worst > m->slabs.cap && (rc = ensure_slabs(m, worst + worst / 2)) != LOM_OK) return rc;
    if (n > kOnePassMax && n <= kBiMaxPoints && !m->opt_no_bulk &&
        (rc = bulk_scratch(m, (uint32_t)n, bulk_shape((uint32_t)n, m->cap, m->bulk_ppt))) != LOM_OK)
        return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    LOM_HIP(m, hipEventCreate(&e0));
    LOM_HIP(m, hipEventCreate(&e1));
    LOM_HIP(m, hipStreamSynchronize(m->stream));
    hipError_t e = hipEventRecord(e0, m->stream);
    rc = add_points_device(m, (const char *)d_xyz, (const char *)d_nrm, n, stride, false, false, false);
    if (e == hipSuccess) e = hipEventRecord(e1, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc != LOM_OK) return rc;
    if (e != hipSuccess) return fail(m, LOM_ERR_HIP, "lom_profile_insert", e);
    *total_us_out = (double)ms * 1e3;
    if ((rc = map_status(m)) != LOM_OK) return rc;
    // what lom_map_add_points_device does after a bulk insert: ~16 slots per voxel
    const uint32_t target = std::max(m->min_cap, next_pow2((uint64_t)m->table_slots_per_voxel * m->n_vox));
    if (m->cap > target) return rehash(m, target);
    return LOM_OK;
}

int lom_map_add_points(lom_map *m, const float *xyz, const float *nrm, size_t n, size_t stride)
{
    if (!m || (n && !xyz) || stride < 12 || (stride & 3)) return LOM_ERR_ARG;
    if (n == 0) return LOM_OK;
    LOM_HIP(m, hipSetDevice(m->device));
    // the points are in host memory: range-check them here (same f32 division and bounds as the
    // device's voxel_index) instead of paying a kernel and a synchronisation
    {
        const float vs = m->voxel_size;
        bool bad = false;
        for (size_t i = 0; i < n; i++) {
            const float *p = reinterpret_cast<const float *>(reinterpret_cast<const char *>(xyz) + i * stride);
            const float fx = p[0] / vs, fy = p[1] / vs, fz = p[2] / vs;
            bad |= !(fx > -kIdxLimit && fx < kIdxLimit) || !(fy > -kIdxLimit && fy < kIdxLimit) ||
                   !(fz > -kIdxLimit && fz < kIdxLimit);
        }
        if (bad) return fail(m, LOM_ERR_RANGE, "coordinate / voxel_size out of range or not finite");
    }
    const char *dx = nullptr, *dn = nullptr;
    int rc = resolve_pending(m);  // before the staging buffers (a pending insert's input) are overwritten
    if (rc != LOM_OK) return rc;
    if ((rc = stage_host_points(m, xyz, nrm, n, stride, &dx, &dn)) != LOM_OK) return rc;
    // the caller's buffer has been copied into the pinned bounce buffer: no need to wait for the GPU
    return add_points_device(m, dx, dn, n, stride, true, false);
}

}  // extern "C"
