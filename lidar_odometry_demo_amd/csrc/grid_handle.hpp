// The handle of a dense 2-D grid that integrates posed scans, written once for lom_occupancy (occupancy.hip) and
// lom_elevation (elevation.hip): the buffers of a call, what create and destroy do for both, the packed upload of a host
// cloud, the staging and the read-back of a call, the host part of a shift by whole cells (grid_handle.hip) and the
// integrate entry points (templates below).  A family keeps its geometry, its own buffers and options, its kernels and
// their launches.  Nothing here launches a kernel.
#pragma once
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "archive_internal.hpp"
#include "plane_geometry.hpp"

namespace lom {

// The grid owns its stream and every buffer below, and what the family adds.
struct GridHandle : DeviceHandle {
    DeviceBuf desc, words;         // descriptors of a call; the status words (16 u32)
    DeviceBuf cloud;               // a host cloud on its way in, packed
    PinnedBuf h_words;             // the status words on their way out
    hipEvent_t done_ev = nullptr;  // recorded behind a call's kernels, for the archive's stream to wait on
    uint32_t plan_cap = 0;         // a test's cap on the scans of one launch (0: the family's own)
    virtual ~GridHandle() = default;  // grid_destroy deletes through GridHandle *; never through DeviceHandle * (not virtual)
};

// a 64-bit counter of the status words: words[w] is its low half
inline uint64_t u64_of(const uint32_t *words, int w) { return (uint64_t)words[w] | ((uint64_t)words[w + 1] << 32); }

// The common part of a create, on a fresh handle that knows its device: the stream, done_ev, the pinned and the device
// words.  A failure's text goes to the family's create slot: LOM_ERR_HIP `setup_text`, or LOM_ERR_OOM `oom_text`.
int grid_setup(GridHandle *g, std::string &slot, const char *setup_text, const char *oom_text);
void grid_destroy(GridHandle *g);  // NULL: nothing
int grid_wait_event(GridHandle *g, void *hip_event);
// n records of stride_bytes in host memory into g->cloud, packed to 12 bytes each, on the grid's stream
int grid_upload_packed(GridHandle *g, const float *xyz, size_t n, size_t stride_bytes);
// the descriptors into g->desc and n_words status words put to zero, on the grid's stream (the descriptors outlive the
// copy: the call waits for the stream before it returns)
int grid_stage(GridHandle *g, const std::vector<assemble::AsmScan> &scans, uint32_t n_words);
// n_words status words into h_words, then the stream is waited for; record_done: done_ev is recorded behind the copy
int grid_read_words(GridHandle *g, uint32_t n_words, bool record_done);
// a per-cell int8 result for the caller: n bytes of `cells` to `out`, n_words summary words into h_words, then the wait
int grid_copy_out(GridHandle *g, int8_t *out, const DeviceBuf &cells, size_t n, uint32_t n_words);

// ---- the shift by whole cells (include/lidar_odometry_amd.h, "grid shift") --------------------------------------------
// What a family's shift does around its one launch (grid_shift.hpp): ask grid_shift_plan; keeps false: its own clear, else
// grid_shift_shadow for each block it moves, the launch from the block into its shadow, grid_shift_wait, and only then
// the swap of block and shadow and the new geometry -- so a call that fails anywhere leaves the grid as it was.  The
// shadows are allocated at the first shift that keeps something and stay: a grid that never shifts pays nothing.
struct GridShift {
    lom_occupancy_geometry geo;  // the geometry afterwards (plane_geometry.hpp: the rule)
    int32_t dx, dy;              // clamped to |dx| <= width, |dy| <= height: what the kernels take
    bool keeps;                  // some cell of the grid stays in it
};
// LOM_ERR_RANGE and "<name>: shift: ..." where the rule refuses; `geo`: the grid's own, an elevation grid's without z_ref
int grid_shift_plan(GridHandle *g, const char *name, const lom_occupancy_geometry &geo, int32_t dx, int32_t dy, GridShift &out);
// exactly `bytes` in `shadow`, once; LOM_ERR_OOM and `oom_text`
int grid_shift_shadow(GridHandle *g, DeviceBuf &shadow, size_t bytes, const char *oom_text);
int grid_shift_wait(GridHandle *g);  // the call returns with its work done

// ---- the integrate entry points -------------------------------------------------------------------------------------
// G, the family's handle, derives from GridHandle and brings: geo; Plan (has `scans`, an assemble::Plan); kName, the head
// of every error text; kPlan, the family's planner; run(plan, xyz, stride_floats, p, stats): grid_stage, every kernel of
// the call, grid_read_words (with done_ev) and the stats from the words.

// A planned call on the device.  xyz: device memory, records of stride_floats, complete when ready_event is (NULL: now);
// a: the archive that holds it, or NULL.
template <class G, class P, class S>
int grid_run(G *g, const typename G::Plan &plan, lom_archive *a, void *ready_event, const float *xyz, uint32_t stride_floats,
             const P *p, S *stats)
{
    S st;
    std::memset(&st, 0, sizeof st);
    st.scans = plan.scans.scans.size();
    if (plan.scans.points_in) {  // (empty scans only: nothing is launched)
        LOM_HIP(g, hipSetDevice(g->device));
        // the archive's clouds are complete when its stream is (an add waits for its own copy; this orders the rest)
        if (a) LOM_HIP(g, hipEventRecord(a->ready_ev, a->stream));
        if (ready_event) LOM_HIP(g, hipStreamWaitEvent(g->stream, (hipEvent_t)ready_event, 0));
        if (const int rc = g->run(plan, xyz, stride_floats, *p, st); rc != LOM_OK) return rc;
        // and what the archive does next comes behind this call's reads
        if (a) LOM_HIP(g, hipStreamWaitEvent(a->stream, g->done_ev, 0));
    }
    if (stats) *stats = st;
    return LOM_OK;
}

template <class G, class P, class S>
int grid_integrate(G *g, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses, size_t count, const P *p, S *stats)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (!g || !a) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(a->lock);
    const std::string name = G::kName;
    if (g->device != a->device) return fail(g, LOM_ERR_ARG, (name + ": the grid and the archive live on different devices").c_str());
    typename G::Plan plan;
    std::string why;
    const int rc = G::kPlan(a->table.data(), a->table.size(), ids, poses, count, g->geo, p, g->plan_cap, plan, why);
    if (rc != LOM_OK) return fail(g, rc, (name + ": " + why).c_str());
    return grid_run(g, plan, a, a->ready_ev, a->d_xyz(), 3, p, stats);
}

// One scan that is not in an archive -- a table of one entry, id 0 -- from host memory (on_host: every refusal comes
// before the upload) or from device memory, complete when the event is.
template <class G, class P, class S>
int grid_integrate_cloud(G *g, const float *xyz, bool on_host, size_t n, size_t stride_bytes, const lom_graph_pose *pose,
                         const P *p, void *hip_event_or_null, S *stats)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (!g) return LOM_ERR_ARG;
    const std::string name = G::kName;
    if ((n && !xyz) || !pose || stride_bytes < 12 || (stride_bytes & 3))
        return fail(g, LOM_ERR_ARG, (name + ": a cloud, a pose and a stride >= 12 that is a multiple of 4").c_str());
    if (n > assemble::kAsmMaxPoints) return fail(g, LOM_ERR_ARG, (name + ": more than 2^31 - 2 points in one cloud").c_str());
    const assemble::ScanEntry e{0, (uint32_t)n};
    const int64_t id = 0;
    typename G::Plan plan;
    std::string why;
    int rc = G::kPlan(&e, 1, &id, pose, 1, g->geo, p, g->plan_cap, plan, why);
    if (rc != LOM_OK) return fail(g, rc, (name + ": " + why).c_str());
    if (!on_host) return grid_run(g, plan, nullptr, hip_event_or_null, xyz, (uint32_t)(stride_bytes / 4), p, stats);
    if ((rc = grid_upload_packed(g, xyz, n, stride_bytes)) != LOM_OK) return rc;
    return grid_run(g, plan, nullptr, nullptr, g->cloud.template as<const float>(), 3, p, stats);
}

}  // namespace lom
