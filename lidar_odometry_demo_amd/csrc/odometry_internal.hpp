// The odometry handle as its two translation units see it: odometry.cpp (create, destroy, accessors) and
// odometry_frame.cpp (processCloud).
#pragma once
#include <atomic>
#include <memory>
#include <string>
#include <vector>

#include "../../include/lidar_odometry_amd.h"
#include "host_stages.hpp"
#include "host_threads.hpp"

// ---- LidarOdometry (src/lidar_odometry.{h,cpp}) ---------------------------------------------
struct lom_odometry {
    lom_odometry_params cfg;
    int device = 0;
    lom_map *keyframe = nullptr;       // keyframe_           lidar_odometry.h:82
    // keyframe_downsampler lidar_odometry.cpp:37: two workspaces, alternating per frame -- its output feeds the
    // keyframe update of the frame, which runs on the keyframe's stream beside the NEXT frame's stages
    lom_map *update_ds2[2] = {nullptr, nullptr};
    lom_map *update_ds = nullptr;      // the one of the current frame
    int parity = 0;
    lom_map *matching_ds = nullptr;    // matching_downsampler lidar_odometry.cpp:46 (reused per frame)
    lom_pose previous, current;        // lidar_odometry.h:84-85
    lom_odometry_frame_stats last{};
    std::vector<lom_point_xyzirt> normalized, deskewed;
    lom_frontend *frontend = nullptr;  // :25-35 on the device (csrc/frontend.hip); LOM_HOST_FRONTEND=1 keeps them on the host
    bool temp_on_device = false;       // temp_cloud_ lives in the front end's HBM buffer
    // keyframe_.size() != 0 (lidar_odometry.cpp:40), tracked on the host.  Atomic: the deferred keyframe update of
    // frame k writes it on the helper thread while frame k+1's stages read it.  A stale `true` is harmless -- the
    // frame prepares a matching cloud it does not use, and the init branch collects the update cloud's count --
    // and it never goes from false to true on the helper thread.
    std::atomic<bool> keyframe_has_voxels{false};
    bool test_force_host_redo = false;  // LOM_OPT_TEST_FORCE_HOST_REDO
    int classifier = LOM_CLASSIFIER_RINGS;  // lom_odometry_set_classifier; the neighbourhood classifier has no host version
    bool debug_timing = false;          // LOM_DEBUG_TIMING=1 at create / LOM_OPT_DEBUG_TIMING
    bool no_cleanup_behind_align = false;  // LOM_NO_CLEANUP_BEHIND_ALIGN=1 at create: the cleanup's scan waits for the host (A/B)
    bool no_send_ahead = false;            // LOM_NO_SEND_AHEAD=1 at create: hints are ignored (A/B)
    // lom_odometry_hint_next: the frame the caller will bring next; `ahead_*`: what the align's idle time has sent ahead
    const lom_point_xyzirt *hint_pts = nullptr, *hint_now = nullptr;  // (hint_now: the hint the running processCloud may use)
    size_t hint_n = 0;
    const lom_point_xyzirt *ahead_pts = nullptr;
    const lom_point_xyzirt *ahead_stage = nullptr;  // where in pinned memory it went
    size_t ahead_n = 0;
    uint64_t frames_sent_ahead = 0;
    int64_t grid_redos = 0;             // frames sent to the host stages because an in-kernel scan gave up
    size_t temp_points = 0;  // temp_cloud_ (lidar_odometry.h:73-77) = the first temp_points records of `deskewed`
    lom::ClassifyScratch classify_scratch;
    std::vector<float> planar, planar_n, filtered, filtered_n, down, down_n, match, upd, upd_n;
    std::string error;
    std::unique_ptr<lom::Pool> pool;  // host workers for the per-point stages (std::execution::par in the reference)
    int64_t queries_total = 0;
    std::unique_ptr<Deferred> deferred;  // keyframe update of the previous frame
    // LOM_OPT_QUALITY_REPORT: every frame that aligns is followed by lom_match_quality_device on its matching cloud at
    // the pose the align returned; lom_odometry_get_quality hands out the last one
    bool quality_on = false, have_quality = false;
    float quality_min_eig_t = 0.f, quality_min_eig_r = 0.f;
    lom_quality_report quality{};
    // lom_odometry_set_carve: the keyframe update carves along the update cloud's rays before it inserts them.  Read and
    // written by the update (the helper thread, when there is one); the setter and the getter settle first.
    bool carve_on = false, have_carve_stats = false;
    lom_carve_params carve{};
    lom_carve_stats carve_stats{};
    // lom_odometry_set_rebuild_votes: lom_odometry_rebuild_keyframe votes the movers out of the keyframe it assembled
    bool votes_on = false, have_vote_stats = false;
    lom_vote_params votes{};
    lom_vote_stats vote_stats{};
    std::string deferred_error;
    // lom_odometry_archive_scan: where the last frame left its update cloud in HBM (one of the update workspaces; packed
    // points and normals).  Written where a frame succeeds, host values only.
    const float *arch_xyz = nullptr, *arch_nrm = nullptr;
    size_t arch_n = 0;
    bool have_upd = false;
    // finish the previous frame's keyframe update; its failure is this call's failure
    int settle()
    {
        if (!deferred) return LOM_OK;
        const int rc = deferred->join();
        if (rc != LOM_OK) error = deferred_error;
        return rc;
    }
};

namespace lom {

inline int fail_map(lom_odometry *o, int rc, lom_map *m)
{
    o->error = lom_last_error(m);
    return rc;
}

}  // namespace lom
