// Clouds in and out of a map handle: the fused down-samplers (VoxelGrid(voxel, 1).addCloud + getCloud, the reference's
// idiom), the export (voxel_grid.h:112-162, getCloud / getCloudWithoutNormals / getSparseCloudWithoutNormals), upload
// and rigid transform.  This file is the one translation unit that instantiates and launches the kernels of
// k_downsample_export.hpp; scans, host staging and the word read-backs are voxel_map.hip's (map_internal.hpp).
//
// Built with -ffp-contract=off (see voxel_map.hip).
#include <algorithm>

#include "grid_scan.hpp"
#include "k_downsample_export.hpp"
#include "lom_internal.hpp"
#include "map_internal.hpp"
#include "pose_math.hpp"

namespace lom {

// shared body of the down-samplers: device input, results left in the workspace's scratch
// (S_ITEMS: xyz, S_PT_POS: normals), voxel count in MW_COUNT, range flag in MW_RANGE.
// wait: read the count (*n_out) and the verdict back (one synchronisation); otherwise the call only enqueues and
// the count stays on the device (d_word(m, MW_COUNT)) for the kernels that consume the result.
static int downsample_core(lom_map *m, float voxel_size, const char *dx, const char *dn, uint32_t N, size_t stride,
                           bool want_normals, bool wait, uint32_t *n_out, const uint32_t *n_dev = nullptr,
                           bool multi_launch = false)
{
    int rc;
    if ((uint64_t)m->cap < 2ull * N) {
        if ((rc = rehash(m, next_pow2(4ull * N))) != LOM_OK) return rc;
    }
    const bool one_pass = N <= 4 * kOnePassMax && !multi_launch;
    uint32_t *pt_slot, *head;
    float *oxyz, *onrm;
    if ((rc = scratch(m, S_PT_SLOT, N, &pt_slot)) != LOM_OK) return rc;
    if ((rc = ensure_rest(m, m->scr[S_DS_HEAD], (size_t)m->cap * 4, 0xFF)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_ITEMS, (size_t)N * 3, &oxyz)) != LOM_OK) return rc;   // compacted xyz
    if ((rc = scratch(m, S_PT_POS, (size_t)N * 3, &onrm)) != LOM_OK) return rc;  // compacted normals
    head = m->scr[S_DS_HEAD].as<uint32_t>();
    if (!want_normals) onrm = nullptr;
    const uint32_t seq = ++m->call_seq;
    const MapView v = view_of(m);
    const dim3 g(blocks_for(N)), b(kThreads);
    if (n_dev && !one_pass) return fail(m, LOM_ERR_ARG, "device-side point count: at most 262144 points");
    hipLaunchKernelGGL(k_ds_claim, g, b, 0, m->stream, m->d_table, v.mask, v.shift, dx, stride, N, n_dev, voxel_size,
                       pt_slot, head, seq, d_word(m, MW_RANGE));
    if (one_pass) {
        const uint32_t items = N <= kOnePassMax ? 1u : 4u;  // consecutive points per thread
        hipLaunchKernelGGL(items == 1 ? k_ds_emit<1> : k_ds_emit<4>, dim3(blocks_for((N + items - 1) / items)), b, 0, m->stream,
                           m->d_table, N, n_dev, pt_slot, head, dx, dn, stride, oxyz, onrm, d_agg(m), seq, d_words(m),
                           take_test_fail_from(m));
        LOM_HIP(m, hipGetLastError());
    } else {
        uint32_t *flag, *rank, *scan_tmp;
        if ((rc = scan_temps(m, N, N, &flag, &rank, &scan_tmp)) != LOM_OK) return rc;
        hipLaunchKernelGGL(k_ds_flag, g, b, 0, m->stream, N, pt_slot, head, flag);
        LOM_HIP(m, hipGetLastError());
        if ((rc = scan_u32(m, flag, rank, N, d_word(m, MW_COUNT), scan_tmp)) != LOM_OK) return rc;
        // the kept point of every voxel also frees its table slot and head word: the workspace is at rest again
        hipLaunchKernelGGL(k_ds_write, g, b, 0, m->stream, N, flag, rank, dx, dn, stride, oxyz, onrm, m->d_table, pt_slot,
                           head);
        LOM_HIP(m, hipGetLastError());
    }
    if (!wait) return LOM_OK;
    WordsRead r;
    if ((rc = read_words(m, MW_COUNT, MW_GRID, &r)) != LOM_OK) return rc;  // voxels, range error, (voxel counter), grid give-up
    m->status_seq = seq;
    if (r[MW_GRID] == seq) {
        // the in-kernel scan gave up: every kept point has still put its slot and head word back to rest, so the
        // workspace is empty again; same call through the flag / scan / write kernels, which wait for nobody
        if (n_dev) return fail(m, LOM_ERR_HIP, "a workgroup timed out waiting for the others of its grid");
        m->grid_redos++;
        return downsample_core(m, voxel_size, dx, dn, N, stride, want_normals, true, n_out, nullptr, true);
    }
    if (r[MW_RANGE] == seq) return fail(m, LOM_ERR_RANGE, "coordinate / voxel_size out of range or not finite");
    *n_out = r[MW_COUNT];
    return LOM_OK;
}

}  // namespace lom

using namespace lom;

extern "C" {

int64_t lom_voxel_downsample(lom_map *ws, float voxel_size, const float *xyz, const float *nrm, size_t n,
                             size_t stride, float *xyz_out, float *nrm_out, size_t cap)
{
    lom_map *m = ws;
    if (!m || !(voxel_size > 0.f) || (n && !xyz) || stride < 12 || (stride & 3) || (n && !xyz_out)) return LOM_ERR_ARG;
    if (n >= 0x7FFFFFFFull) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    int rc = lom_map_clear(m, voxel_size);  // the workspace grid ends up cleared, like a fresh VoxelGrid(voxel, 1)
    if (rc != LOM_OK || n == 0) return rc;
    const char *dx = nullptr, *dn = nullptr;
    if ((rc = stage_host_points(m, xyz, nrm, n, stride, &dx, &dn)) != LOM_OK) return rc;
    // the range rule of addCloud is checked by the claim kernel (flag read back with the count)
    uint32_t found = 0;
    if ((rc = downsample_core(m, voxel_size, dx, dn, (uint32_t)n, stride, nrm_out != nullptr, true, &found)) != LOM_OK) return rc;
    const size_t total = found;
    const size_t take = std::min(total, cap);
    if (take) {
        LOM_HIP(m, hipMemcpyAsync(xyz_out, m->scr[S_ITEMS].p, take * 12, hipMemcpyDeviceToHost, m->stream));
        if (nrm_out)
            LOM_HIP(m, hipMemcpyAsync(nrm_out, m->scr[S_PT_POS].p, take * 12, hipMemcpyDeviceToHost, m->stream));
        LOM_HIP(m, hipStreamSynchronize(m->stream));
    }
    return (int64_t)total;
}

int64_t lom_voxel_downsample_device(lom_map *ws, float voxel_size, const float *d_xyz, const float *d_nrm, size_t n,
                                    size_t stride, const float **d_xyz_out, const float **d_nrm_out)
{
    lom_map *m = ws;
    if (!m || !(voxel_size > 0.f) || (n && !d_xyz) || stride < 12 || (stride & 3) || !d_xyz_out) return LOM_ERR_ARG;
    if (n >= 0x7FFFFFFFull) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    *d_xyz_out = nullptr;
    if (d_nrm_out) *d_nrm_out = nullptr;
    int rc = lom_map_clear(m, voxel_size);
    if (rc != LOM_OK || n == 0) return rc;
    uint32_t found = 0;
    if ((rc = downsample_core(m, voxel_size, (const char *)d_xyz, (const char *)d_nrm, (uint32_t)n, stride,
                              d_nrm_out != nullptr, true, &found)) != LOM_OK)
        return rc;
    *d_xyz_out = m->scr[S_ITEMS].as<const float>();
    if (d_nrm_out) *d_nrm_out = m->scr[S_PT_POS].as<const float>();
    return (int64_t)found;
}

int lom_voxel_downsample_device_nowait(lom_map *ws, float voxel_size, const float *d_xyz, const float *d_nrm,
                                       size_t n_bound, const uint32_t *d_n, size_t stride, const float **d_xyz_out,
                                       const float **d_nrm_out, const uint32_t **d_count_out)
{
    lom_map *m = ws;
    if (!m || !(voxel_size > 0.f) || (n_bound && !d_xyz) || stride < 12 || (stride & 3) || !d_xyz_out || !d_count_out)
        return LOM_ERR_ARG;
    if (n_bound >= 0x7FFFFFFFull) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    *d_xyz_out = nullptr;
    if (d_nrm_out) *d_nrm_out = nullptr;
    int rc = lom_map_clear(m, voxel_size);
    if (rc != LOM_OK) return rc;
    *d_count_out = d_word(m, MW_COUNT);
    if (n_bound == 0) {
        LOM_HIP(m, hipMemsetAsync(d_word(m, MW_COUNT), 0, 4, m->stream));
        return LOM_OK;
    }
    if ((rc = downsample_core(m, voxel_size, (const char *)d_xyz, (const char *)d_nrm, (uint32_t)n_bound, stride,
                              d_nrm_out != nullptr, false, nullptr, d_n)) != LOM_OK)
        return rc;
    *d_xyz_out = m->scr[S_ITEMS].as<const float>();
    if (d_nrm_out) *d_nrm_out = m->scr[S_PT_POS].as<const float>();
    return LOM_OK;
}

int lom_upload_points(lom_map *m, const float *xyz, const float *nrm, size_t n, size_t stride, const float **d_xyz_out,
                      const float **d_nrm_out)
{
    if (!m || (n && !xyz) || stride < 12 || (stride & 3) || !d_xyz_out) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    *d_xyz_out = nullptr;
    if (d_nrm_out) *d_nrm_out = nullptr;
    if (n == 0) return LOM_OK;
    const char *dx = nullptr, *dn = nullptr;
    int rc = resolve_pending(m);
    if (rc != LOM_OK) return rc;
    if ((rc = stage_host_points(m, xyz, nrm, n, stride, &dx, &dn)) != LOM_OK) return rc;
    *d_xyz_out = (const float *)dx;
    if (d_nrm_out) *d_nrm_out = (const float *)dn;
    return LOM_OK;
}

int lom_transform_points_device(lom_map *m, const lom_pose *pose, const float *d_xyz, const float *d_nrm, size_t n,
                                size_t stride, const float **d_xyz_out, const float **d_nrm_out)
{
    if (!m || !pose || (n && !d_xyz) || stride < 12 || (stride & 3) || !d_xyz_out) return LOM_ERR_ARG;
    if (n >= 0x7FFFFFFFull) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    *d_xyz_out = nullptr;
    if (d_nrm_out) *d_nrm_out = nullptr;
    if (n == 0) return LOM_OK;
    int rc;
    if ((rc = resolve_pending(m)) != LOM_OK) return rc;
    const bool with_n = d_nrm && d_nrm_out;
    if ((rc = ensure(m, m->scr[S_IN_XYZ], n * 12)) != LOM_OK) return rc;
    if (with_n && (rc = ensure(m, m->scr[S_IN_NRM], n * 12)) != LOM_OK) return rc;
    RigidArgs A;
    rotation_matrix(pose->q, A.R);
    for (int i = 0; i < 3; i++) A.t[i] = pose->t[i];
    hipLaunchKernelGGL(k_transform, dim3(blocks_for((uint32_t)n)), dim3(kThreads), 0, m->stream, (const char *)d_xyz,
                       (const char *)d_nrm, stride, (uint32_t)n, A, m->scr[S_IN_XYZ].as<float>(),
                       with_n ? m->scr[S_IN_NRM].as<float>() : (float *)nullptr);
    LOM_HIP(m, hipGetLastError());
    *d_xyz_out = m->scr[S_IN_XYZ].as<const float>();
    if (with_n) *d_nrm_out = m->scr[S_IN_NRM].as<const float>();
    return LOM_OK;
}

int64_t lom_map_export(lom_map *m, int mode, float *xyz_out, float *nrm_out, size_t cap)
{
    if (!m || mode < 0 || mode > 2) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    int rc;
    if ((rc = refresh_nvox(m)) != LOM_OK) return rc;
    if (m->n_vox == 0) return 0;
    const uint32_t nv = m->n_vox;
    // (counts and offsets go where a cleanup scan behind an align leaves keep / newid: scan_temps drops such a scan, and
    // the radius cleanup that follows an export or a pointCount runs its own)
    uint32_t *cnt, *off, *scan_tmp;
    if ((rc = scan_temps(m, nv, nv, &cnt, &off, &scan_tmp)) != LOM_OK) return rc;
    hipLaunchKernelGGL(k_export_counts, dim3(blocks_for(nv)), dim3(kThreads), 0, m->stream, m->slabs.count, nv, mode, cnt);
    LOM_HIP(m, hipGetLastError());
    if ((rc = scan_u32(m, cnt, off, nv, d_word(m, MW_COUNT), scan_tmp)) != LOM_OK) return rc;
    WordsRead r;
    if ((rc = read_words(m, MW_COUNT, MW_COUNT, &r)) != LOM_OK) return rc;
    const size_t total = r[MW_COUNT];
    if (!xyz_out || cap == 0) return (int64_t)total;
    const bool want_n = nrm_out && mode == LOM_EXPORT_FULL;
    if ((rc = ensure(m, m->scr[S_IN_XYZ], total * 12)) != LOM_OK) return rc;
    if (want_n && (rc = ensure(m, m->scr[S_IN_NRM], total * 12)) != LOM_OK) return rc;
    const size_t work = (size_t)nv * m->K;
    hipLaunchKernelGGL(k_export_write, dim3(blocks_for(work)), dim3(kThreads), 0, m->stream, off, m->slabs.count, nv,
                       m->K, mode, m->slabs.pts, m->slabs.nrm, m->scr[S_IN_XYZ].as<float>(),
                       want_n ? m->scr[S_IN_NRM].as<float>() : (float *)nullptr);
    LOM_HIP(m, hipGetLastError());
    const size_t take = std::min(total, cap);
    LOM_HIP(m, hipMemcpyAsync(xyz_out, m->scr[S_IN_XYZ].p, take * 12, hipMemcpyDeviceToHost, m->stream));
    if (want_n) LOM_HIP(m, hipMemcpyAsync(nrm_out, m->scr[S_IN_NRM].p, take * 12, hipMemcpyDeviceToHost, m->stream));
    LOM_HIP(m, hipStreamSynchronize(m->stream));
    return (int64_t)total;
}

int64_t lom_map_point_count(const lom_map *cm)
{
    // the stored points are exactly what the full export would return
    return lom_map_export(const_cast<lom_map *>(cm), LOM_EXPORT_FULL_NO_NORMALS, nullptr, nullptr, 0);
}

}  // extern "C"
