// LidarOdometry::processCloud, lidar_odometry.cpp:22-77, ROS-free: the stages before the align on the device (or on the
// host, csrc/host_stages.cpp), the align, the divergence guard and the keyframe update, for one frame
// (lom_odometry_process_cloud), a sequence of frames, or one frame of each of several streams
// (lom_odometry_process_batch).  Everything that touches the voxel maps or the matcher goes through the C ABI.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "odometry_internal.hpp"
#include "pose_math.hpp"
#include "stage_words.hpp"

namespace lom {
namespace {

// front end and down-samplers take frames of up to ~170k points (their in-kernel scans cover 262144 cells /
// points); larger ones go through the host stages
constexpr size_t kMaxDeviceFrame = 170000;

// what a stage function says beside a LOM_* status (LOM_OK is 0, errors are negative)
enum StageStep : int {
    kHostStages = 1,  // the device stages hand the frame back: it takes the host stages
    kFrameDone = 2    // frame_stages: the frame initialised the keyframe, there is no align
};

struct FrameInputs {  // what the stages before the align leave in HBM for it and for the keyframe update
    const float *d_down = nullptr, *d_down_n = nullptr;  // keyframe_downsampler.getCloud()            :37-38,42,69
    const float *d_match = nullptr;                      // matching_downsampler.getCloudWithoutNormals() :46-47,50
    int64_t nd = 0, nm = 0;
    // device stages: the update cloud's size and verdict are still on their way (a read-back is enqueued on this
    // workspace); collect_update() waits for them.  Returns LOM_OK / LOM_ERR_RANGE / LOM_ERR_HIP.
    lom_map *pending_update = nullptr;
    uint32_t pending_seq = 0;
    // the front end's filtered cloud (input of both down-samplers), for the redo of an update down-sampling whose
    // in-kernel scan gave up
    const float *d_fx = nullptr, *d_fn = nullptr;
    int64_t nf = 0;
    static constexpr int kScanGaveUp = 2;
    int collect_update(const char **error_out)
    {
        if (!pending_update) return LOM_OK;
        lom_map *m = pending_update;
        pending_update = nullptr;
        uint32_t w[3] = {0, 0, 0};
        const int rc = lom_map_read_device_words_end(m, w);
        if (rc != LOM_OK) {
            if (error_out) *error_out = lom_last_error(m);
            return rc;
        }
        if (w[2] == pending_seq) return kScanGaveUp;  // nothing written, workspace at rest: the caller redoes it
        if (w[1] == pending_seq) {
            if (error_out) *error_out = kVoxelRangeError;
            return LOM_ERR_RANGE;
        }
        nd = w[0];
        return LOM_OK;
    }
    // the frame will not use its update cloud: no read-back stays pending on the workspace
    void drain_update() { (void)collect_update(nullptr); }
};

// Every exit of a frame that has failed after its stages went out: the pending read-back is drained here, before the
// failure is returned.  The error text is the handle's `m`, else `text`, else what the callee has already set.
int fail_frame(lom_odometry *o, FrameInputs &in, int rc, lom_map *m, const char *text = nullptr)
{
    in.drain_update();
    if (m) return fail_map(o, rc, m);
    if (text) o->error = text;
    return rc;
}

// the frame into the front end's pinned buffer by the worker pool (one pass over ~1 MB)
void copy_to_stage(lom_odometry *o, lom_point_xyzirt *stage, const lom_point_xyzirt *pts, size_t n)
{
    run_parts(o->pool.get(), n, [&](size_t b, size_t e, unsigned) {
        std::memcpy(static_cast<void *>(stage + b), pts + b, (e - b) * sizeof(lom_point_xyzirt));
    }, 8192);
}

// :37-38 and :46-47 from a filtered cloud in HBM, each call waiting for its own verdict: the update cloud in `update_ws`
// and, if wanted, the matching cloud
int downsample_now(lom_odometry *o, FrameInputs &in, lom_map *update_ws, const float *d_fx, const float *d_fn, size_t nf,
                   bool want_match)
{
    in.nd = lom_voxel_downsample_device(update_ws, o->cfg.keyframe_update_voxel_size, d_fx, d_fn, nf, 12, &in.d_down,
                                        &in.d_down_n);
    if (in.nd < 0) return fail_map(o, (int)in.nd, update_ws);
    if (want_match) {
        in.nm = lom_voxel_downsample_device(o->matching_ds, o->cfg.keyframe_matching_voxel_size, d_fx, nullptr, nf, 12,
                                            &in.d_match, nullptr);
        if (in.nm < 0) return fail_map(o, (int)in.nm, o->matching_ds);
    }
    return LOM_OK;
}

// :25-47 on the host (worker pool), then one upload: the path of frames the device front end hands back
int stages_on_host(lom_odometry *o, const lom_point_xyzirt *pts, size_t n, const lom_pose &rel_inv, const lom_pose &ident,
                   lom_odometry_frame_stats &cur, FrameInputs &in, StageTimer &tm)
{
    const size_t cap = n ? n : 1;
    o->normalized.resize(cap);
    o->deskewed.resize(cap);
    for (auto *v : {&o->planar, &o->planar_n, &o->filtered, &o->filtered_n}) v->resize(cap * 3);
    time_normalize(pts, n, o->normalized.data(), o->pool.get());                                      // :25
    transform_non_rigid(o->normalized.data(), n, rel_inv, ident, o->deskewed.data(), o->pool.get());  // :30
    o->temp_points = n;  // :31 temp_cloud_ = deskewed_input_cloud
    o->temp_on_device = false;
    tm.lap("norm+deskew");
    size_t nu = 0;
    const size_t np = classify(o->deskewed.data(), n, o->planar.data(), o->planar_n.data(), &nu, nullptr,
                               o->classify_scratch, o->pool.get());  // :33
    const size_t nf = range_filter(o->planar.data(), o->planar_n.data(), np, o->cfg.lidar_min_range,
                                   o->cfg.lidar_max_range, o->filtered.data(), o->filtered_n.data(), o->pool.get());  // :35
    cur.planar_points = (int64_t)np;
    cur.filtered_points = (int64_t)nf;
    tm.lap("classify+filter");
    int rc;
    // the previous frame's keyframe update ran beside the host stages above; it must be through before this
    // frame touches a handle.  Its failure is reported here, by the call after the one it belongs to; this
    // frame is then not processed and poses / keyframe stay as they were.
    if ((rc = o->settle()) != LOM_OK) return rc;
    const float *d_fx = nullptr, *d_fn = nullptr;
    if ((rc = lom_upload_points(o->update_ds, o->filtered.data(), o->filtered_n.data(), nf, 12, &d_fx, &d_fn)) != LOM_OK)
        return fail_map(o, rc, o->update_ds);
    if ((rc = downsample_now(o, in, o->update_ds, d_fx, d_fn, nf, o->keyframe_has_voxels)) != LOM_OK) return rc;
    tm.lap("down-samplers");
    return LOM_OK;
}

// what the enqueue half of the device stages hands to the finish half
struct DeviceStages {
    lom_map *reader = nullptr;  // the workspace whose read-back the finish half waits for
    bool has_keyframe = false;
    uint32_t seq_u = 0, seq_m = 0;
    const float *d_fx = nullptr, *d_fn = nullptr;
};

// :25-47 on the device: the frame stays in HBM from its upload to its pose.  Front end (4 kernels), both
// down-samplers (2 kernels each) fed with device-side counts, then ONE look at the host for the sizes the
// align and the keyframe update are launched with.  Two halves around that look: stages_device_enqueue puts everything
// on the streams and the read-back behind it, stages_device_finish waits for it, settles the previous frame's keyframe
// update and takes the verdicts (lom_odometry_process_batch enqueues the stages of all its streams before it finishes
// any).  Both return kHostStages when the front end hands the frame back.
int stages_device_enqueue(lom_odometry *o, const lom_point_xyzirt *pts, size_t n, const lom_pose &rel_inv,
                          const lom_pose &ident, FrameInputs &in, StageTimer &tm, DeviceStages &ds)
{
    int rc;
    const bool neighbourhood = o->classifier == LOM_CLASSIFIER_NEIGHBOURHOOD;
    if (n > kMaxDeviceFrame) {
        if (!neighbourhood) return kHostStages;
        o->error = "frame too large for the device front end (the neighbourhood classifier has no host version)";
        return LOM_ERR_ARG;
    }
    // the frame goes into the front end's pinned buffer, then to HBM -- unless it went there while the previous frame's
    // align ran (lom_odometry_hint_next)
    const bool staged = o->ahead_pts != nullptr && o->ahead_pts == pts && o->ahead_n == n;
    o->ahead_pts = nullptr;
    lom_point_xyzirt *stage = nullptr;
    if ((rc = lom_frontend_stage(o->frontend, n, &stage)) != LOM_OK) {
        o->error = lom_frontend_last_error(o->frontend);
        return rc;
    }
    if (staged && stage == o->ahead_stage) {
        o->frames_sent_ahead++;
    } else {
        copy_to_stage(o, stage, pts, n);
    }
    if ((rc = lom_frontend_process(o->frontend, stage, n, &rel_inv, &ident, o->cfg.lidar_min_range, o->cfg.lidar_max_range)) !=
        LOM_OK) {
        if (rc == LOM_ERR_ARG && !neighbourhood) return kHostStages;  // a frame beyond the front end's size limit
        o->error = lom_frontend_last_error(o->frontend);
        return rc;
    }
    o->temp_points = n;  // :31 temp_cloud_ = deskewed_input_cloud (fetched from HBM on demand)
    o->temp_on_device = true;
    tm.lap("front end enq.");
    const float *d_fx = nullptr, *d_fn = nullptr;
    const uint32_t *d_fe = nullptr, *d_nd = nullptr, *d_nm = nullptr;
    uint32_t bound = 0;
    lom_frontend_results(o->frontend, &d_fx, &d_fn, &d_fe, &bound);
    // front end and down-samplers share a stream of their own: all of this runs beside the previous frame's
    // keyframe update (whose input is the OTHER update workspace).  Only the matching cloud is on the way to the
    // align; the keyframe-update cloud is enqueued behind the read-back the align waits for, runs beside the
    // align's first kernels, and its count and verdict are collected after the align (pending_update).
    const uint32_t *ptrs[kStageWords];
    uint32_t seq_u = 0, seq_m = 0;
    const uint32_t *u_range = nullptr, *u_grid = nullptr, *m_range = nullptr, *m_grid = nullptr;
    ptrs[kWordPlanar] = d_fe;
    ptrs[kWordFiltered] = d_fe + 1;
    ptrs[kWordFeRedoHost] = d_fe + 4;  // (sequence number of the frame)
    ptrs[kWordFeGrid] = d_fe + 5;
    ptrs[kWordFeRange] = d_fe + 6;
    const int k = neighbourhood ? kStageWords : kWordFeRange;  // (the last word is the neighbourhood classifier's)
    auto update_downsample = [&]() -> int {
        const int r = lom_voxel_downsample_device_nowait(o->update_ds, o->cfg.keyframe_update_voxel_size, d_fx, d_fn, bound,
                                                         d_fe + 1, 12, &in.d_down, &in.d_down_n, &d_nd);
        if (r != LOM_OK) return fail_map(o, r, o->update_ds);
        lom_map_status_words(o->update_ds, &u_range, &u_grid, &seq_u);
        return LOM_OK;
    };
    lom_map *reader = o->update_ds;
    const bool has_keyframe = o->keyframe_has_voxels.load();  // one look; possibly a stale `true` (see the member)
    if (has_keyframe) {
        if ((rc = lom_voxel_downsample_device_nowait(o->matching_ds, o->cfg.keyframe_matching_voxel_size, d_fx, nullptr, bound,
                                                     d_fe + 1, 12, &in.d_match, nullptr, &d_nm)) != LOM_OK)
            return fail_map(o, rc, o->matching_ds);
        lom_map_status_words(o->matching_ds, &m_range, &m_grid, &seq_m);
        ptrs[kWordDsCount] = d_nm;
        ptrs[kWordDsRange] = m_range;
        ptrs[kWordDsGrid] = m_grid;
        reader = o->matching_ds;
        if ((rc = lom_map_read_device_words_begin(reader, ptrs, k)) != LOM_OK) return fail_map(o, rc, reader);
        if ((rc = update_downsample()) != LOM_OK) return rc;
        const uint32_t *late[3] = {d_nd, u_range, u_grid};
        if ((rc = lom_map_read_device_words_begin(o->update_ds, late, 3)) != LOM_OK) return fail_map(o, rc, o->update_ds);
        in.pending_update = o->update_ds;
        in.pending_seq = seq_u;
    } else {  // first frame: the keyframe is initialised from the update cloud, there is no align
        if ((rc = update_downsample()) != LOM_OK) return rc;
        ptrs[kWordDsCount] = d_nd;
        ptrs[kWordDsRange] = u_range;
        ptrs[kWordDsGrid] = u_grid;
        if ((rc = lom_map_read_device_words_begin(reader, ptrs, k)) != LOM_OK) return fail_map(o, rc, reader);
    }
    ds = DeviceStages{reader, has_keyframe, seq_u, seq_m, d_fx, d_fn};
    return LOM_OK;
}

int stages_device_finish(lom_odometry *o, lom_odometry_frame_stats &cur, FrameInputs &in, StageTimer &tm,
                         const DeviceStages &ds)
{
    int rc;
    uint32_t got[kStageWords] = {0};
    // the one wait before the align: counts and verdicts of what it needs
    if ((rc = lom_map_read_device_words_end(ds.reader, got)) != LOM_OK) return fail_map(o, rc, ds.reader);
    tm.lap("stages (device)");
    // the previous frame's keyframe update must be through before this frame touches the keyframe handle.  Its
    // failure is reported here, by the call after the one it belongs to; poses / keyframe stay as they were.
    if ((rc = o->settle()) != LOM_OK) return fail_frame(o, in, rc, nullptr);  // (settle has set the text)
    tm.lap("settle");
    const StageVerdict v =
        decode_stage_words(got, ds.has_keyframe, o->classifier == LOM_CLASSIFIER_NEIGHBOURHOOD, lom_frontend_sequence(o->frontend),
                           ds.has_keyframe ? ds.seq_m : ds.seq_u, o->test_force_host_redo);
    if (v.count_redo) o->grid_redos++;
    in.d_fx = ds.d_fx;
    in.d_fn = ds.d_fn;
    switch (v.action) {
    case StageVerdict::kFailRange: return fail_frame(o, in, LOM_ERR_RANGE, nullptr, v.error);
    case StageVerdict::kRedoHost: in.drain_update(); return kHostStages;
    case StageVerdict::kRedoDevice: {
        // a scan that gave up -- the front end's or a down-sampler's -- has written nothing: the front end redoes its
        // stage with kernels that wait for nobody (lom_frontend_wait), and both down-samplers run again from its
        // result, each waiting for its own verdict
        in.drain_update();
        uint32_t counts[4] = {got[kWordPlanar], got[kWordFiltered], 0, 0};
        if (v.wait_front_end && (rc = lom_frontend_wait(o->frontend, counts)) != LOM_OK) {
            o->error = lom_frontend_last_error(o->frontend);
            return rc;
        }
        cur.planar_points = counts[0];
        cur.filtered_points = counts[1];
        in.nf = counts[1];
        return downsample_now(o, in, o->update_ds, ds.d_fx, ds.d_fn, (size_t)in.nf, ds.has_keyframe);
    }
    case StageVerdict::kProceed: break;
    }
    cur.planar_points = v.planar;
    cur.filtered_points = v.filtered;
    in.nf = v.filtered;
    if (ds.has_keyframe) {
        in.nm = v.matching;
    } else {
        in.nd = v.update;
    }
    return LOM_OK;
}

// the update cloud's size and verdict; a down-sampling whose in-kernel scan gave up is redone here from the
// filtered cloud still in HBM (lom_voxel_downsample_device waits for its own verdict and falls back to the
// multi-launch scan by itself).  A failure leaves its text in o->error.
int collect_or_redo_update(lom_odometry *o, FrameInputs &in)
{
    lom_map *ws = in.pending_update;
    const char *why = nullptr;
    const int rc = in.collect_update(&why);
    if (rc == FrameInputs::kScanGaveUp) {
        o->grid_redos++;
        return downsample_now(o, in, ws, in.d_fx, in.d_fn, (size_t)in.nf, false);
    }
    if (rc != LOM_OK) o->error = why ? why : "keyframe-update down-sampling failed";
    return rc;
}

// lom_map_set_align_idle_hook: runs on the caller's thread while the align's kernels work -- the hinted next frame goes
// into the front end's pinned buffer (the current frame's copy there has long been read by the device).  Host work only:
// the frame's first kernel (upload + statistics) sent ahead as well was measured and is not (a
// second queue's kernel is not started while the align's queue holds packets, and a copy-engine upload made frames slower)
void send_next_frame_ahead(void *user)
{
    lom_odometry *o = static_cast<lom_odometry *>(user);
    const lom_point_xyzirt *pts = o->hint_now;
    const size_t n = o->hint_n;
    o->hint_now = nullptr;
    if (!pts || !n || n > kMaxDeviceFrame || !o->frontend) return;
    StageTimer tm(o->debug_timing);  // ("ahead ..." line: inside the align's lap)
    lom_point_xyzirt *stage = nullptr;
    if (lom_frontend_stage(o->frontend, n, &stage) != LOM_OK) return;
    copy_to_stage(o, stage, pts, n);
    tm.lap("ahead copy");
    o->ahead_pts = pts;
    o->ahead_n = n;
    o->ahead_stage = stage;
}

// ---- processCloud in phases: lom_odometry_process_cloud runs them back to back, lom_odometry_process_batch runs each
// phase for all its streams, with ONE align (lom_match_align_multi) for all streams that align
struct Frame {
    lom_odometry_frame_stats cur{};  // becomes o->last when the frame is through
    StageTimer tm;
    lom_pose relative, rel_inv, ident, guess, previous_next;
    FrameInputs in;
    DeviceStages ds;
    int enq = kHostStages;  // stages_device_enqueue's status
    explicit Frame(bool timing) : tm(timing) {}
};

// a hint is for the call that follows it, what was sent ahead for the call after that: neither outlives its call
struct DropHints {
    lom_odometry *o = nullptr;
    const lom_point_xyzirt *sent_before = nullptr;
    void arm(lom_odometry *od)
    {
        o = od;
        o->hint_now = o->hint_pts;
        o->hint_pts = nullptr;
        sent_before = o->ahead_pts;
    }
    ~DropHints()
    {
        if (!o) return;
        o->hint_now = nullptr;
        if (o->ahead_pts == sent_before) o->ahead_pts = nullptr;  // (this call did not use it: the front end drops it)
    }
};

// :27-28 and the device stages' enqueue half
void frame_enqueue(lom_odometry *o, Frame &f, const lom_point_xyzirt *pts, size_t n)
{
    lom_pose_relative_to(&o->previous, &o->current, &f.relative);  // :27
    // :28 previous_transform_ = current_transform_ -- committed where the frame succeeds (the
    // reference has no error channel; here a frame that fails must leave the state as it found it,
    // or the next frame's constant-velocity guess and deskew would start from a zero motion)
    f.previous_next = o->current;
    lom::pose_inverse(f.relative, f.rel_inv);
    lom_pose_identity(&f.ident);
    o->parity ^= 1;
    o->update_ds = o->update_ds2[o->parity];
    f.enq = o->frontend ? stages_device_enqueue(o, pts, n, f.rel_inv, f.ident, f.in, f.tm, f.ds) : kHostStages;
}

// the stages' finish (or the host stages), then :40-44 or :51: LOM_OK = the frame aligns next (f.guess, f.in.d_match),
// kFrameDone = it initialised the keyframe, else the frame's failure
int frame_stages(lom_odometry *o, Frame &f, const lom_point_xyzirt *pts, size_t n)
{
    int rc = f.enq;
    if (rc == LOM_OK) rc = stages_device_finish(o, f.cur, f.in, f.tm, f.ds);
    if (rc == kHostStages) {
        f.in = FrameInputs();
        rc = stages_on_host(o, pts, n, f.rel_inv, f.ident, f.cur, f.in, f.tm);
        f.cur.host_stages = 1;
    }
    if (rc != LOM_OK) return rc;
    // :40 keyframe_.size() == 0 -- known on the host: the keyframe is empty until a frame has put voxels
    // into it (nd > 0 points always create at least one), and stays non-empty unless a cleanup empties it
    if (!o->keyframe_has_voxels) {  // :40-44 init keyframe
        // (if the stages ran on a stale "has voxels" -- the previous update emptied the keyframe meanwhile -- the
        // update cloud's count is still on its way)
        if ((rc = collect_or_redo_update(o, f.in)) != LOM_OK) return rc;
        if ((rc = lom_map_add_points_device(o->keyframe, f.in.d_down, f.in.d_down_n, (size_t)f.in.nd, 12)) != LOM_OK)
            return fail_map(o, rc, o->keyframe);
        o->arch_xyz = f.in.d_down, o->arch_nrm = f.in.d_down_n, o->arch_n = (size_t)f.in.nd, o->have_upd = true;
        f.cur.initialised_keyframe = 1;
        f.cur.update_points = f.in.nd;
        f.cur.keyframe_voxels = lom_map_size(o->keyframe);
        o->keyframe_has_voxels = f.cur.keyframe_voxels > 0;
        o->last = f.cur;
        o->previous = f.previous_next;  // :28
        return kFrameDone;
    }
    f.cur.matching_points = f.in.nm;
    lom_pose_compose(&o->current, &f.relative, &f.guess);  // :51
    return LOM_OK;
}

// LOM_OPT_QUALITY_REPORT: the report of the pose the align has just returned (before the divergence guard may replace
// it), over the matching cloud still in HBM, at the align's own 0.3 m gate (cloud_matcher.cpp:139), against the keyframe
// as the align saw it (its update comes later, in frame_commit)
int frame_quality(lom_odometry *o, const Frame &f, const lom_pose &result)
{
    const int rc = lom_match_quality_device(o->keyframe, f.in.d_match, (size_t)f.in.nm, 12, result.t, result.q, 0.3f,
                                            o->quality_min_eig_t, o->quality_min_eig_r, &o->quality, nullptr);
    o->have_quality = rc == LOM_OK;
    return rc;
}

// keyframe update (:67-70) with the update cloud `d_down` at `pose`: on the helper thread when there is one, so a
// failure leaves its text in o->deferred_error
int keyframe_update(lom_odometry *o, const lom_pose &pose, const float *d_down, const float *d_down_n, size_t n,
                    double t_submit)
{
    auto bad = [o](int rc, lom_map *m) {
        o->deferred_error = lom_last_error(m);
        return rc;
    };
    StageTimer ut(o->debug_timing);  // (the helper thread's own laps: "upd ..." lines)
    if (o->debug_timing) std::fprintf(stderr, "  %-14s %8.1f us\n", "upd hand-off", (ut.t0 - t_submit) * 1e6);
    int rc;
    // :69 first: the rigid transform of the update cloud reads neither the map nor what the cleanup leaves, and its
    // launch fills the time the cleanup spends waiting for its scan (enqueued behind the align) to report
    const float *d_upd = nullptr, *d_upd_n = nullptr;
    if ((rc = lom_transform_points_device(o->keyframe, &pose, d_down, d_down_n, n, 12, &d_upd, &d_upd_n)) != LOM_OK)
        return bad(rc, o->keyframe);
    if ((rc = lom_map_radius_cleanup(o->keyframe, pose.t, o->cfg.keyframe_cleanup_range)) != LOM_OK)  // :67
        return bad(rc, o->keyframe);
    ut.lap("upd cleanup");
    if (o->carve_on) {  // lom_odometry_set_carve: free space along this frame's rays, before its points go in
        if ((rc = lom_map_carve_rays_device(o->keyframe, pose.t, d_upd, n, 12, &o->carve, &o->carve_stats)) != LOM_OK)
            return bad(rc, o->keyframe);
        o->have_carve_stats = true;
        ut.lap("upd carve");
    }
    if ((rc = lom_map_add_points_device_nowait(o->keyframe, d_upd, d_upd_n, n, 12)) != LOM_OK)  // :70
        return bad(rc, o->keyframe);
    ut.lap("upd enqueue");
    // one look at the host per update: the deferred verdict of the insert and the voxel count
    if ((rc = lom_map_status(o->keyframe)) != LOM_OK) return bad(rc, o->keyframe);
    ut.lap("upd status");
    o->last.keyframe_voxels = lom_map_size(o->keyframe);
    o->keyframe_has_voxels = o->last.keyframe_voxels > 0;
    return LOM_OK;
}

// after the align (:49-51): the update cloud's verdict, :53-63, :65 and the keyframe update (:67-70)
int frame_commit(lom_odometry *o, Frame &f, const lom_align_stats &ast, lom_pose result)
{
    lom_odometry_frame_stats &cur = f.cur;
    FrameInputs &in = f.in;
    StageTimer &tm = f.tm;
    int rc;
    // the update cloud was down-sampled beside the align: its size and verdict (long since on the host)
    if ((rc = collect_or_redo_update(o, in)) != LOM_OK) return rc;
    cur.update_points = in.nd;
    cur.outer_iterations = ast.outer_iterations;
    cur.queries = ast.queries;
    o->queries_total += ast.queries;
    cur.queries_total = o->queries_total;
    tm.lap("align");
    {  // :53-63 divergence guard
        float ang[3];
        delta_euler_deg(result.q, o->current.q, ang);
        const float thr = o->cfg.angular_divergence_threshold;
        bool ok = true;
        for (int a = 0; a < 3; a++) ok = ok && (std::fabs(ang[a]) < thr || std::fabs(ang[a]) > 180 - thr);
        if (!ok) {
            result = f.guess;  // :61
            cur.unstable_rotation = 1;
        }
    }
    o->previous = f.previous_next;                                                                // :28
    o->current = result;                                                                          // :65
    o->last = cur;
    // keyframe update (:67-70): same calls in the same order, on the helper thread when there is one
    const lom_pose pose_now = o->current;
    const size_t n_down = (size_t)in.nd;
    const float *d_down = in.d_down, *d_down_n = in.d_down_n;
    o->arch_xyz = d_down, o->arch_nrm = d_down_n, o->arch_n = n_down, o->have_upd = true;
    const double t_submit = o->debug_timing ? StageTimer::now() : 0.0;
    auto update = [=]() -> int { return keyframe_update(o, pose_now, d_down, d_down_n, n_down, t_submit); };
    if (o->deferred) {
        o->deferred->submit(update);
    } else if ((rc = update()) != LOM_OK) {
        o->error = o->deferred_error;
        return rc;
    }
    tm.lap("keyframe update");
    tm.total();
    return LOM_OK;
}

}  // namespace
}  // namespace lom

using namespace lom;

extern "C" {

int lom_odometry_hint_next(lom_odometry *o, const lom_point_xyzirt *pts, size_t n)
{
    if (!o || (!pts && n)) return LOM_ERR_ARG;
    o->hint_pts = (o->no_send_ahead || !n) ? nullptr : pts;
    o->hint_n = n;
    return LOM_OK;
}

int lom_odometry_process_cloud(lom_odometry *o, const lom_point_xyzirt *pts, size_t n)
{
    if (!o || (!pts && n)) return LOM_ERR_ARG;
    try {
        Frame f(o->debug_timing);
        DropHints drop_hints;
        drop_hints.arm(o);
        frame_enqueue(o, f, pts, n);
        int rc = frame_stages(o, f, pts, n);
        if (rc == kFrameDone) return LOM_OK;
        if (rc != LOM_OK) return rc;
        lom_align_stats ast;
        lom_pose result;
        // :65-67: the keyframe update below starts with radiusCleanup(current_transform_.translation): its scan may run
        // right behind the align, on the align's own result
        if (!o->no_cleanup_behind_align) (void)lom_map_radius_cleanup_after_align(o->keyframe, o->cfg.keyframe_cleanup_range);
        // ... and the frame the caller has announced (lom_odometry_hint_next) is sent ahead while this thread would only
        // watch the align's report
        if (o->hint_now && o->frontend && o->temp_on_device) (void)lom_map_set_align_idle_hook(o->keyframe, send_next_frame_ahead, o);
        if ((rc = lom_match_align_device(o->keyframe, f.in.d_match, (size_t)f.in.nm, 12, f.guess.t, f.guess.q, result.t,
                                         result.q, &ast)) != LOM_OK)  // :49-51
            return fail_frame(o, f.in, rc, o->keyframe);
        if (o->quality_on && (rc = frame_quality(o, f, result)) != LOM_OK) return fail_frame(o, f.in, rc, o->keyframe);
        return frame_commit(o, f, ast, result);
    } catch (const std::bad_alloc &) {
        o->error = "host allocation failed";
        return LOM_ERR_OOM;
    }
}

int lom_odometry_process_batch(lom_odometry *const *o, const lom_point_xyzirt *const *frames, const size_t *n, int count,
                               int *status_out)
{
    if (count < 0 || (count > 0 && (!o || !frames || !n))) return LOM_ERR_ARG;
    for (int i = 0; i < count; i++) {
        if (!o[i] || (!frames[i] && n[i]) || o[i]->device != o[0]->device) return LOM_ERR_ARG;
        for (int j = 0; j < i; j++)
            if (o[j] == o[i]) return LOM_ERR_ARG;
    }
    std::vector<int> st((size_t)count, LOM_OK);
    try {
        std::vector<std::unique_ptr<Frame>> f((size_t)count);
        std::vector<DropHints> drop_hints((size_t)count);  // (no hint is followed: the batch arms no idle hook)
        // every stream's stages go out before any is waited for: the K front ends overlap on the device
        for (int i = 0; i < count; i++) {
            f[i].reset(new Frame(o[i]->debug_timing));
            drop_hints[i].arm(o[i]);
            frame_enqueue(o[i], *f[i], frames[i], n[i]);
        }
        std::vector<int> aligning;
        for (int i = 0; i < count; i++) {
            const int rc = frame_stages(o[i], *f[i], frames[i], n[i]);
            if (rc == LOM_OK) aligning.push_back(i);
            else if (rc != kFrameDone) st[i] = rc;
        }
        // one align for all streams that align, on the first one's keyframe stream; no cleanup scan behind it
        if (!aligning.empty()) {
            const size_t k = aligning.size();
            std::vector<lom_align_multi_problem> p(k);
            std::vector<lom_align_result> res(k);
            for (size_t a = 0; a < k; a++) {
                const Frame &fr = *f[aligning[a]];
                p[a].map = o[aligning[a]]->keyframe;
                p[a].xyz = fr.in.d_match;
                p[a].n = (size_t)fr.in.nm;
                p[a].stride_bytes = 12;
                std::memcpy(p[a].guess_t, fr.guess.t, sizeof p[a].guess_t);
                std::memcpy(p[a].guess_q_wxyz, fr.guess.q, sizeof p[a].guess_q_wxyz);
            }
            lom_map *runner = o[aligning[0]]->keyframe;
            const int rc = lom_match_align_multi_device(runner, p.data(), (int)k, res.data(), nullptr);  // :49-51
            for (size_t a = 0; a < k; a++) {
                const int i = aligning[a];
                if (rc != LOM_OK) {
                    st[i] = fail_frame(o[i], f[i]->in, rc, runner);
                    continue;
                }
                lom_pose result;
                std::memcpy(result.t, res[a].t, sizeof result.t);
                std::memcpy(result.q, res[a].q_wxyz, sizeof result.q);
                if (o[i]->quality_on) {  // per stream, one after another
                    const int rq = frame_quality(o[i], *f[i], result);
                    if (rq != LOM_OK) {
                        st[i] = fail_frame(o[i], f[i]->in, rq, o[i]->keyframe);
                        continue;
                    }
                }
                st[i] = frame_commit(o[i], *f[i], res[a].stats, result);
            }
        }
    } catch (const std::bad_alloc &) {
        for (int i = 0; i < count; i++)
            if (st[i] == LOM_OK) {
                o[i]->error = "host allocation failed";
                st[i] = LOM_ERR_OOM;
            }
    }
    int rc = LOM_OK;
    for (int i = 0; i < count; i++) {
        if (status_out) status_out[i] = st[i];
        if (rc == LOM_OK) rc = st[i];
    }
    return rc;
}

int lom_odometry_process_sequence(lom_odometry *o, const lom_point_xyzirt *const *frames, const size_t *n, size_t count,
                                  size_t *done)
{
    if (done) *done = 0;
    if (!o || (count && (!frames || !n))) return LOM_ERR_ARG;
    for (size_t i = 0; i < count; i++) {
        if (i + 1 < count) (void)lom_odometry_hint_next(o, frames[i + 1], n[i + 1]);
        const int rc = lom_odometry_process_cloud(o, frames[i], n[i]);
        if (rc != LOM_OK) return rc;
        if (done) *done = i + 1;
    }
    return LOM_OK;
}

}  // extern "C"
