// Scan votes: every archived scan at its pose votes on the voxels of an assembled map -- seen, or seen through -- and a
// rule on the two counts erases what moved.  Definitions: include/lidar_odometry_amd.h ("scan votes"); kernels:
// k_vote.hpp; host planning (parameter ranges, slices, step bound): vote_host.cpp; DESIGN.md 7i.
// New code beside the map path: the erase is the carve's (erase_begin / erase_rank / erase_finish of map_erase.hip), the
// descriptors are the assembly's, and no default path launches any of this.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "archive_internal.hpp"
#include "k_vote.hpp"
#include "lom_internal.hpp"
#include "vote_host.hpp"

using namespace lom;

namespace {

// grow-only and at rest: a fresh block is zeroed once, in stream order before its first use
int ensure_zero(lom_map *m, DeviceBuf &b, size_t bytes)
{
    if (bytes <= b.bytes) return LOM_OK;
    const int rc = ensure(m, b, bytes);
    if (rc != LOM_OK) return rc;
    LOM_HIP(m, hipMemsetAsync(b.p, 0, b.bytes, m->stream));
    return LOM_OK;
}

// who may call: the arguments that need no plan (the plan's own refusals follow in count_votes)
int refuse(lom_map *m, lom_archive *a)
{
    if (m->parent) return fail(m, LOM_ERR_ARG, "scan votes: a scan context has no map of its own");
    if (m->device != a->device) return fail(m, LOM_ERR_ARG, "scan votes: the map and the archive live on different devices");
    return LOM_OK;
}

// Plan, descriptors and every slice's walk and fold over the map's m->n_vox slabs (settled by the caller): free / seen
// and the status words are left on the device.  *launched: something was enqueued (there is a ray).  The archive's lock
// is held by the caller.
int count_votes(lom_map *m, lom_archive *a, const vote::Plan &plan, const lom_vote_params &p, bool *launched)
{
    *launched = false;
    const std::vector<assemble::AsmScan> &scans = plan.scans.scans;
    for (size_t k = 0; k < scans.size(); k++)
        if (!vote::origin_ok(scans[k], m->voxel_size))
            return fail(m, LOM_ERR_RANGE, ("scan votes: origin of scan " + std::to_string(k) +
                                           " of the call / voxel_size out of range or not finite").c_str());
    if (plan.slices.empty()) return LOM_OK;
    int rc;
    VoteBufs &b = m->vote;
    const uint32_t nv = m->n_vox;
    const size_t room = std::max<size_t>((size_t)nv * 2, 64);  // (twice: a growing keyframe; never nothing: an empty map)
    if ((rc = ensure_zero(m, b.hitmask, room * 8)) != LOM_OK) return rc;
    if ((rc = ensure_zero(m, b.crossmask, room * 8)) != LOM_OK) return rc;
    if ((rc = ensure_zero(m, b.free_votes, room * 4)) != LOM_OK) return rc;
    if ((rc = ensure_zero(m, b.seen_votes, room * 4)) != LOM_OK) return rc;
    if ((rc = ensure(m, b.words, (size_t)VW_COUNT * 4)) != LOM_OK) return rc;
    const size_t desc_bytes = scans.size() * sizeof(assemble::AsmScan);
    if ((rc = ensure(m, b.desc, desc_bytes)) != LOM_OK) return rc;
    // the archive's clouds are complete when its stream is (an add waits for its own copy; this orders the rest)
    LOM_HIP(m, hipEventRecord(a->ready_ev, a->stream));
    LOM_HIP(m, hipStreamWaitEvent(m->stream, a->ready_ev, 0));
    LOM_HIP(m, hipMemsetAsync(b.words.p, 0, (size_t)VW_COUNT * 4, m->stream));
    // (the plan outlives the copy: every caller waits for the stream before it returns)
    LOM_HIP(m, hipMemcpyAsync(b.desc.p, scans.data(), desc_bytes, hipMemcpyHostToDevice, m->stream));
    VoteArgs va;
    va.voxel_size = m->voxel_size;
    va.margin = p.margin;
    va.min_range = p.min_range;
    va.max_range = p.max_range;
    va.clearance = p.clearance;
    va.max_steps = vote::max_steps(p.max_range, m->voxel_size);
    const MapView v = view_of(m);
    for (const vote::Slice &s : plan.slices) {
        hipLaunchKernelGGL(k_vote_walk, dim3(s.grid_x, s.count), dim3(kAsmThreads), 0, m->stream,
                           b.desc.as<const AsmScan>() + s.first, a->d_xyz(), a->d_nrm(), va, v.table, v.mask, v.shift, nv,
                           b.hitmask.as<unsigned long long>(), b.crossmask.as<unsigned long long>(), b.words.as<uint32_t>());
        if (nv)
            hipLaunchKernelGGL(k_vote_fold, dim3(blocks_for(nv)), dim3(kThreads), 0, m->stream,
                               b.hitmask.as<unsigned long long>(), b.crossmask.as<unsigned long long>(), nv,
                               b.free_votes.as<uint32_t>(), b.seen_votes.as<uint32_t>());
        LOM_HIP(m, hipGetLastError());
    }
    *launched = true;
    return LOM_OK;
}

int make_plan(lom_map *m, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses, size_t count,
              const lom_vote_params *p, vote::Plan &plan)
{
    std::string why;
    const int rc = vote::plan(a->table.data(), a->table.size(), ids, poses, count, p, m->vote.test_slice_max, plan, why);
    return rc == LOM_OK ? LOM_OK : fail(m, rc, ("scan votes: " + why).c_str());
}

}  // namespace

extern "C" {

int lom_map_carve_scans(lom_map *m, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses, size_t count,
                        const lom_vote_params *p, lom_vote_stats *stats)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (!m || !a) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(a->lock);
    int rc = refuse(m, a);
    if (rc != LOM_OK) return rc;
    vote::Plan plan;
    if ((rc = make_plan(m, a, ids, poses, count, p, plan)) != LOM_OK) return rc;
    lom_vote_stats st;
    std::memset(&st, 0, sizeof st);
    st.scans = count;
    st.rays_skipped = plan.scans.points_in;
    if (plan.slices.empty()) {  // not one ray: only the origins' verdict is left
        for (const assemble::AsmScan &d : plan.scans.scans)
            if (!vote::origin_ok(d, m->voxel_size)) return fail(m, LOM_ERR_RANGE, "scan votes: an origin / voxel_size out of range or not finite");
        if (stats) *stats = st;
        return LOM_OK;
    }
    LOM_HIP(m, hipSetDevice(m->device));
    if ((rc = map_settle_nvox(m)) != LOM_OK) return rc;  // (an empty map: the walk runs all the same, for the range verdict and the stats)
    const uint32_t nv = m->n_vox;
    uint32_t *keep = nullptr;
    if ((rc = erase_begin(m, &keep)) != LOM_OK) return rc;
    bool launched = false;
    if ((rc = count_votes(m, a, plan, *p, &launched)) != LOM_OK) return rc;
    uint32_t *words = m->vote.words.as<uint32_t>();
    const uint32_t *d_kept = nullptr;
    if (nv) {
        // (runs whatever the error word says: it is what puts free / seen back to rest)
        hipLaunchKernelGGL(k_vote_flag, dim3(blocks_for(nv)), dim3(kThreads), 0, m->stream, m->vote.free_votes.as<uint32_t>(),
                           m->vote.seen_votes.as<uint32_t>(), m->slabs.count, nv, p->min_free_scans, p->free_per_seen, keep, words);
        LOM_HIP(m, hipGetLastError());
        if ((rc = erase_rank(m, &d_kept)) != LOM_OK) return rc;
    }
    // the one read-back: error word and stats with the kept count, before anything is erased
    const uint32_t *ptrs[VW_COUNT + 1];
    for (int i = 0; i < VW_COUNT; i++) ptrs[i] = words + i;
    ptrs[VW_COUNT] = d_kept;
    uint32_t got[VW_COUNT + 1] = {0};
    if ((rc = gather_words(m, ptrs, nv ? VW_COUNT + 1 : VW_COUNT, got)) != LOM_OK) return rc;
    if (got[VW_ERROR]) return fail(m, LOM_ERR_RANGE, "scan votes: coordinate / voxel_size out of range or not finite");
    const uint32_t n_keep = nv ? got[VW_COUNT] : 0u, n_live = nv - m->n_dead;
    st.rays_walked = (uint64_t)got[VW_WALKED] | ((uint64_t)got[VW_WALKED + 1] << 32);
    st.rays_skipped = plan.scans.points_in - st.rays_walked;
    st.cells_visited = (uint64_t)got[VW_VISITED] | ((uint64_t)got[VW_VISITED + 1] << 32);
    st.voxels_free = got[VW_FREE];
    st.voxels_protected = got[VW_PROTECTED];
    st.voxels_erased = n_live - n_keep;
    if (nv && (rc = erase_finish(m, n_keep)) != LOM_OK) return rc;
    if (stats) *stats = st;
    return LOM_OK;
}

int64_t lom_map_scan_votes(lom_map *m, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses, size_t count,
                           const lom_vote_params *p, uint32_t *free_out, uint32_t *seen_out, size_t cap)
{
    if (!m || !a) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(a->lock);
    int rc = refuse(m, a);
    if (rc != LOM_OK) return rc;
    vote::Plan plan;
    if ((rc = make_plan(m, a, ids, poses, count, p, plan)) != LOM_OK) return rc;
    LOM_HIP(m, hipSetDevice(m->device));
    if ((rc = map_settle_nvox(m)) != LOM_OK) return rc;
    const uint32_t nv = m->n_vox;
    bool launched = false;
    if ((rc = count_votes(m, a, plan, *p, &launched)) != LOM_OK) return rc;
    std::vector<uint32_t> free_votes(nv, 0u), seen_votes(nv, 0u), slab_count(nv), words(VW_COUNT, 0u);
    if (launched) {
        VoteBufs &b = m->vote;
        if (nv) {
            LOM_HIP(m, hipMemcpyAsync(free_votes.data(), b.free_votes.p, (size_t)nv * 4, hipMemcpyDeviceToHost, m->stream));
            LOM_HIP(m, hipMemcpyAsync(seen_votes.data(), b.seen_votes.p, (size_t)nv * 4, hipMemcpyDeviceToHost, m->stream));
            // back to rest
            LOM_HIP(m, hipMemsetAsync(b.free_votes.p, 0, (size_t)nv * 4, m->stream));
            LOM_HIP(m, hipMemsetAsync(b.seen_votes.p, 0, (size_t)nv * 4, m->stream));
        }
        LOM_HIP(m, hipMemcpyAsync(words.data(), b.words.p, (size_t)VW_COUNT * 4, hipMemcpyDeviceToHost, m->stream));
    }
    if (nv) LOM_HIP(m, hipMemcpyAsync(slab_count.data(), m->slabs.count, (size_t)nv * 4, hipMemcpyDeviceToHost, m->stream));
    LOM_HIP(m, hipStreamSynchronize(m->stream));
    if (words[VW_ERROR]) return fail(m, LOM_ERR_RANGE, "scan votes: coordinate / voxel_size out of range or not finite");
    size_t live = 0;
    for (uint32_t s = 0; s < nv; s++) {
        if (!slab_count[s]) continue;  // (the export skips empty slabs)
        if (live < cap) {
            if (free_out) free_out[live] = free_votes[s];
            if (seen_out) seen_out[live] = seen_votes[s];
        }
        live++;
    }
    return (int64_t)live;
}

}  // extern "C"
