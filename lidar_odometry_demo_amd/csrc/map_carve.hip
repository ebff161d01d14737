// Ray carving (lidar_odometry_amd.h, "ray carving"): voxels that enough rays of a scan pass through, and no endpoint
// falls into, are erased.  This file is the one translation unit that instantiates and launches the kernels of
// k_carve.hpp; the erase itself is map_erase.hip's (erase_begin / erase_rank / erase_finish), host staging and the word
// read-back are voxel_map.hip's (map_internal.hpp).
//
// Built with -ffp-contract=off (see voxel_map.hip).
#include <algorithm>
#include <cmath>
#include <vector>

#include "grid_scan.hpp"
#include "k_carve.hpp"
#include "lom_internal.hpp"
#include "map_internal.hpp"
#include "pose_math.hpp"

namespace lom {

// arguments first, then the state: nothing here touches HIP
static int carve_args(const lom_map *m, const float *origin, const float *xyz, size_t n, size_t stride, const lom_carve_params *p)
{
    if (!carve_params_ok(p)) return LOM_ERR_ARG;
    if (!m || !origin || (n && !xyz) || stride < 12 || (stride & 3) || n >= 0x7FFFFFFFull) return LOM_ERR_ARG;
    return LOM_OK;
}

// hits and walk of one call over the map's `nv` slabs (settled by the caller): cross[] / hit[] / the carve's words are
// left on the device.  The origin's range verdict is the host's (the array is the host's in every entry point).
static int carve_count(lom_map *m, uint32_t nv, const float origin[3], const char *d_xyz, uint32_t n, size_t stride,
                       const lom_carve_params &p)
{
    const float vs = m->voxel_size;
    for (int a = 0; a < 3; a++) {
        const float f = origin[a] / vs;
        if (!(f > -kIdxLimit && f < kIdxLimit))
            return fail(m, LOM_ERR_RANGE, "carve: origin / voxel_size out of range or not finite");
    }
    int rc;
    uint32_t *cross, *hit, *words;
    const size_t room = std::max<size_t>((size_t)nv * 2, 64);  // (twice: a growing keyframe; never nothing: an empty map)
    if ((rc = scratch(m, S_CARVE_CROSS, room, &cross)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_CARVE_HIT, room, &hit)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_CARVE_WORDS, (size_t)CW_COUNT, &words)) != LOM_OK) return rc;
    if (nv) {
        LOM_HIP(m, hipMemsetAsync(cross, 0, (size_t)nv * 4, m->stream));
        LOM_HIP(m, hipMemsetAsync(hit, 0, (size_t)nv * 4, m->stream));
    }
    LOM_HIP(m, hipMemsetAsync(words, 0, (size_t)CW_COUNT * 4, m->stream));
    CarveArgs a;
    for (int k = 0; k < 3; k++) a.o[k] = origin[k];
    a.voxel_size = vs;
    a.margin = p.margin;
    a.min_range = p.min_range;
    a.max_range = p.max_range;
    // (no ray is longer than the index range: 2^21 cells per axis)
    const double cells = std::min(std::ceil((double)p.max_range / (double)vs), 2097152.0);
    a.max_steps = 3u * ((uint32_t)cells + 2u);
    const MapView v = view_of(m);
    hipLaunchKernelGGL(k_carve_hits, dim3(blocks_for(n)), dim3(kThreads), 0, m->stream, d_xyz, stride, n, vs, v.table, v.mask,
                       v.shift, nv, hit, words);
    hipLaunchKernelGGL(k_carve_walk, dim3(blocks_for(n)), dim3(kThreads), 0, m->stream, d_xyz, stride, n, a, v.table, v.mask,
                       v.shift, nv, cross, words);
    LOM_HIP(m, hipGetLastError());
    return LOM_OK;
}

static int carve_rays(lom_map *m, const float origin[3], const float *xyz, size_t n, size_t stride, const lom_carve_params *p,
                      lom_carve_stats *stats, bool on_host)
{
    int rc = carve_args(m, origin, xyz, n, stride, p);
    if (rc != LOM_OK) return rc;
    if (m->parent) return fail(m, LOM_ERR_ARG, "a scan context cannot change its keyframe");
    if (stats) *stats = lom_carve_stats();
    if (n == 0) return LOM_OK;
    LOM_HIP(m, hipSetDevice(m->device));
    if ((rc = map_settle_nvox(m)) != LOM_OK) return rc;  // (settles a pending insert first: before the staging buffers are reused)
    const uint32_t nv = m->n_vox;  // (an empty map: hits and walk run all the same, for the range verdict and the stats)
    const char *d_xyz = (const char *)xyz, *d_none = nullptr;
    if (on_host && (rc = stage_host_points(m, xyz, nullptr, n, stride, &d_xyz, &d_none)) != LOM_OK) return rc;
    uint32_t *keep = nullptr;
    if ((rc = erase_begin(m, &keep)) != LOM_OK) return rc;
    if ((rc = carve_count(m, nv, origin, d_xyz, (uint32_t)n, stride, *p)) != LOM_OK) return rc;
    uint32_t *cross = m->scr[S_CARVE_CROSS].as<uint32_t>(), *hit = m->scr[S_CARVE_HIT].as<uint32_t>(),
             *words = m->scr[S_CARVE_WORDS].as<uint32_t>();
    const uint32_t *d_kept = d_word(m, MW_COUNT);  // (what erase_rank says, too; an empty map: read, not used)
    if (nv) {
        hipLaunchKernelGGL(k_carve_flag, dim3(blocks_for(nv)), dim3(kThreads), 0, m->stream, cross, hit, m->slabs.count, nv,
                           p->min_crossings, keep, words);
        LOM_HIP(m, hipGetLastError());
        if ((rc = erase_rank(m, &d_kept)) != LOM_OK) return rc;
    }
    // the one read-back: error word and stats with the kept count, before anything is erased
    const uint32_t *ptrs[CW_COUNT + 1];
    for (int i = 0; i < CW_COUNT; i++) ptrs[i] = words + i;
    ptrs[CW_COUNT] = d_kept;
    uint32_t got[CW_COUNT + 1];
    if ((rc = gather_words(m, ptrs, CW_COUNT + 1, got)) != LOM_OK) return rc;
    if (got[CW_ERROR]) return fail(m, LOM_ERR_RANGE, "carve: coordinate / voxel_size out of range or not finite");
    const uint32_t n_keep = nv ? got[CW_COUNT] : 0u, n_live = nv - m->n_dead;
    if (stats) {
        stats->rays_walked = (uint64_t)got[CW_WALKED] | ((uint64_t)got[CW_WALKED + 1] << 32);
        stats->rays_skipped = n - stats->rays_walked;
        stats->cells_visited = (uint64_t)got[CW_VISITED] | ((uint64_t)got[CW_VISITED + 1] << 32);
        stats->voxels_crossed = got[CW_CROSSED];
        stats->voxels_protected = got[CW_PROTECTED];
        stats->voxels_erased = n_live - n_keep;
    }
    return nv ? erase_finish(m, n_keep) : LOM_OK;
}

}  // namespace lom

using namespace lom;

extern "C" {

int lom_map_carve_rays(lom_map *m, const float origin[3], const float *xyz, size_t n, size_t stride, const lom_carve_params *p,
                       lom_carve_stats *stats)
{
    return carve_rays(m, origin, xyz, n, stride, p, stats, true);
}

int lom_map_carve_rays_device(lom_map *m, const float origin[3], const float *d_xyz, size_t n, size_t stride,
                              const lom_carve_params *p, lom_carve_stats *stats)
{
    return carve_rays(m, origin, d_xyz, n, stride, p, stats, false);
}

int64_t lom_map_carve_counts(lom_map *m, const float origin[3], const float *xyz, size_t n, size_t stride,
                             const lom_carve_params *p, uint32_t *cross_out, uint8_t *hit_out, size_t cap)
{
    int rc = carve_args(m, origin, xyz, n, stride, p);
    if (rc != LOM_OK) return rc;
    if (m->parent) return fail(m, LOM_ERR_ARG, "carve counts are the map's, not a scan context's");
    LOM_HIP(m, hipSetDevice(m->device));
    if ((rc = map_settle_nvox(m)) != LOM_OK) return rc;
    const uint32_t nv = m->n_vox;  // (an empty map: the kernels run all the same, for the range verdict)
    std::vector<uint32_t> cross(nv, 0u), hit(nv, 0u), count(nv), words(CW_COUNT, 0u);
    if (n) {
        const char *d_xyz = nullptr, *d_none = nullptr;
        if ((rc = stage_host_points(m, xyz, nullptr, n, stride, &d_xyz, &d_none)) != LOM_OK) return rc;
        if ((rc = carve_count(m, nv, origin, d_xyz, (uint32_t)n, stride, *p)) != LOM_OK) return rc;
        if (nv) {
            LOM_HIP(m, hipMemcpyAsync(cross.data(), m->scr[S_CARVE_CROSS].p, (size_t)nv * 4, hipMemcpyDeviceToHost, m->stream));
            LOM_HIP(m, hipMemcpyAsync(hit.data(), m->scr[S_CARVE_HIT].p, (size_t)nv * 4, hipMemcpyDeviceToHost, m->stream));
        }
        LOM_HIP(m, hipMemcpyAsync(words.data(), m->scr[S_CARVE_WORDS].p, (size_t)CW_COUNT * 4, hipMemcpyDeviceToHost, m->stream));
    }
    if (nv) LOM_HIP(m, hipMemcpyAsync(count.data(), m->slabs.count, (size_t)nv * 4, hipMemcpyDeviceToHost, m->stream));
    LOM_HIP(m, hipStreamSynchronize(m->stream));
    if (words[CW_ERROR]) return fail(m, LOM_ERR_RANGE, "carve: coordinate / voxel_size out of range or not finite");
    size_t live = 0;
    for (uint32_t s = 0; s < nv; s++) {
        if (!count[s]) continue;  // (the export skips empty slabs)
        if (live < cap) {
            if (cross_out) cross_out[live] = cross[s];
            if (hit_out) hit_out[live] = hit[s] ? 1 : 0;
        }
        live++;
    }
    return (int64_t)live;
}

}  // extern "C"
