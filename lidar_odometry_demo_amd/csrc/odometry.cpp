// LidarOdometry (reference src/lidar_odometry.{h,cpp}) without processCloud: create, destroy, accessors and setters.
// The frame itself is csrc/odometry_frame.cpp; everything that touches the voxel maps or the matcher goes through the
// C ABI, i.e. the GPU.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>

#include "odometry_internal.hpp"
#include "pose_math.hpp"
#include "vote_host.hpp"

using namespace lom;

// the last frame's deskewed cloud as lom_odometry_place_descriptor reads it: the front end's copy in HBM (*event: its done
// event) or the host copy of a host-stage frame (*event NULL); records of sizeof(lom_point_xyzirt) bytes
static int deskewed_cloud(lom_odometry *o, const float **pts, size_t *n, void **event)
{
    *n = o->temp_points;
    *event = nullptr;
    if (!o->temp_on_device) {
        *pts = reinterpret_cast<const float *>(o->deskewed.data());
        return LOM_OK;
    }
    const lom_point_xyzirt *d = nullptr;
    uint32_t nd = 0;
    const int rc = lom_frontend_deskewed(o->frontend, &d, &nd);
    if (rc != LOM_OK) return rc;
    *pts = reinterpret_cast<const float *>(d);
    *n = nd;
    *event = lom_frontend_done_event(o->frontend);
    return LOM_OK;
}

// that cloud at the current pose into a 2-D grid of family G (csrc/occupancy.hip, csrc/elevation.hip), through the
// family's device-cloud or host-cloud integrate; reads only
template <class G, class P, class S, class DeviceOf, class LastError, class FromDevice, class FromHost>
static int grid_scan(lom_odometry *o, G *g, const P *p, S *stats, DeviceOf device_of, LastError last_error, FromDevice from_device,
                     FromHost from_host)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (!o || !g || device_of(g) != o->device) return LOM_ERR_ARG;
    if (o->temp_points == 0) return LOM_ERR_STATE;  // no frame yet
    const float *pts = nullptr;
    size_t n = 0;
    void *event = nullptr;
    int rc = deskewed_cloud(o, &pts, &n, &event);
    if (rc != LOM_OK) return rc;
    lom_graph_pose pose;
    if ((rc = lom_graph_pose_from_f32(&o->current, &pose)) != LOM_OK) return rc;
    const size_t stride = sizeof(lom_point_xyzirt);
    rc = o->temp_on_device ? from_device(g, pts, n, stride, &pose, p, event, stats) : from_host(g, pts, n, stride, &pose, p, stats);
    if (rc != LOM_OK) o->error = last_error(g);
    return rc;
}

extern "C" {

void lom_odometry_default_params(lom_odometry_params *p)
{
    // lidar_odometry.h:36-48 and config/params.yaml
    p->lidar_min_range = 4.0f;
    p->lidar_max_range = 80.0f;
    p->keyframe_voxel_size = 0.2f;
    p->keyframe_max_points_cnt = 20;
    p->keyframe_matching_voxel_size = 0.3f;
    p->keyframe_update_voxel_size = 0.1f;
    p->keyframe_cleanup_range = 80.0f;
    p->angular_divergence_threshold = 5.0f;
}

int lom_odometry_create(const lom_odometry_params *params, int device, lom_odometry **out)
{
    if (!params || !out) return LOM_ERR_ARG;
    *out = nullptr;
    lom_odometry *o = new (std::nothrow) lom_odometry();
    if (!o) return LOM_ERR_OOM;
    o->cfg = *params;
    o->device = device;
    o->debug_timing = getenv("LOM_DEBUG_TIMING") != nullptr;
    o->no_cleanup_behind_align = getenv("LOM_NO_CLEANUP_BEHIND_ALIGN") != nullptr;
    o->no_send_ahead = getenv("LOM_NO_SEND_AHEAD") != nullptr;
    {
        unsigned hw = std::thread::hardware_concurrency();
        if (const char *e = getenv("LOM_HOST_THREADS")) hw = (unsigned)std::max(1, atoi(e));
        o->pool.reset(new Pool(std::max(1u, std::min(hw, 16u))));
    }
    if (!getenv("LOM_SYNC_KEYFRAME_UPDATE")) o->deferred.reset(new Deferred());
    lom_pose_identity(&o->current);  // lidar_odometry.cpp:15-17
    o->previous = o->current;
    int rc = lom_map_create(params->keyframe_voxel_size, params->keyframe_max_points_cnt, 1 << 16, device,
                            &o->keyframe);  // :18-19
    if (rc == LOM_OK) rc = lom_map_create(params->keyframe_update_voxel_size, 1, 1 << 15, device, &o->update_ds2[0]);
    if (rc == LOM_OK) rc = lom_map_create(params->keyframe_update_voxel_size, 1, 1 << 15, device, &o->update_ds2[1]);
    o->update_ds = o->update_ds2[0];
    if (rc == LOM_OK) rc = lom_map_create(params->keyframe_matching_voxel_size, 1, 1 << 14, device, &o->matching_ds);
    // Two streams: the keyframe's (align, keyframe update) and the front end's (upload, front-end kernels, both
    // down-samplers).  The stages of frame k+1 run beside the keyframe update of frame k; the host reads the
    // stage results back (a synchronisation with the front end's stream) before it launches the align.
    if (rc == LOM_OK && !getenv("LOM_HOST_FRONTEND")) rc = lom_frontend_create(device, nullptr, &o->frontend);
    void *stage_stream = o->frontend ? lom_frontend_stream(o->frontend) : (o->keyframe ? lom_map_get_stream(o->keyframe) : nullptr);
    for (lom_map *h : {o->update_ds2[0], o->update_ds2[1], o->matching_ds})
        if (rc == LOM_OK) rc = lom_map_set_stream(h, stage_stream);
    if (rc != LOM_OK) {
        lom_odometry_destroy(o);
        return rc;
    }
    *out = o;
    return LOM_OK;
}

void lom_odometry_destroy(lom_odometry *o)
{
    if (!o) return;
    (void)o->settle();
    o->deferred.reset();
    // the down-samplers run on the front end's stream (or the keyframe's): they go before the owner of that stream
    lom_map_destroy(o->update_ds2[0]);
    lom_map_destroy(o->update_ds2[1]);
    lom_map_destroy(o->matching_ds);
    lom_frontend_destroy(o->frontend);
    lom_map_destroy(o->keyframe);
    delete o;
}

const char *lom_odometry_last_error(const lom_odometry *o) { return o ? o->error.c_str() : ""; }
lom_map *lom_odometry_keyframe(lom_odometry *o)
{
    if (!o) return nullptr;
    (void)o->settle();
    return o->keyframe;
}

int lom_odometry_get_pose(const lom_odometry *o, lom_pose *out)
{
    if (!o || !out) return LOM_ERR_ARG;
    *out = o->current;  // lidar_odometry.cpp:87-89
    return LOM_OK;
}

// getTempCloud(), lidar_odometry.h:73-75: the deskewed input cloud of the last processCloud (:31)
int64_t lom_odometry_get_temp_cloud(const lom_odometry *o, lom_point_xyzirt *out, size_t cap)
{
    if (!o || (cap && !out)) return LOM_ERR_ARG;
    const size_t n = o->temp_points;
    if (o->temp_on_device) return lom_frontend_fetch(o->frontend, 0, out, nullptr, cap);
    if (out && cap) std::memcpy(static_cast<void *>(out), o->deskewed.data(), std::min(n, cap) * sizeof(lom_point_xyzirt));
    return (int64_t)n;
}

// the place descriptor of that cloud (csrc/place.hip): from the front end's copy in HBM, behind its done event, or from
// the host copy of a host-stage frame; reads only
int lom_odometry_place_descriptor(lom_odometry *o, lom_place_db *db, int add, float *desc_out, int64_t *id_out)
{
    if (!o || !db || (!add && !desc_out) || lom_place_db_device(db) != o->device) return LOM_ERR_ARG;
    if (o->temp_points == 0) return LOM_ERR_STATE;  // no frame yet
    const size_t stride = sizeof(lom_point_xyzirt);
    const float *pts = nullptr;
    size_t n = o->temp_points;
    if (o->temp_on_device) {
        const lom_point_xyzirt *d = nullptr;
        uint32_t nd = 0;
        int rc = lom_frontend_deskewed(o->frontend, &d, &nd);
        if (rc == LOM_OK) rc = lom_place_db_wait_event(db, lom_frontend_done_event(o->frontend));
        if (rc != LOM_OK) return rc;
        pts = reinterpret_cast<const float *>(d);
        n = nd;
    } else {
        pts = reinterpret_cast<const float *>(o->deskewed.data());
    }
    if (!add) return o->temp_on_device ? lom_place_describe_device(db, pts, n, stride, desc_out) : lom_place_describe(db, pts, n, stride, desc_out);
    const int64_t id = o->temp_on_device ? lom_place_db_add_cloud_device(db, pts, n, stride) : lom_place_db_add_cloud(db, pts, n, stride);
    if (id < 0) return (int)id;
    if (id_out) *id_out = id;
    return desc_out ? lom_place_db_get(db, id, desc_out) : LOM_OK;
}

// The last frame's update cloud into a scan archive (csrc/archive.hip), device to device.  The cloud's kernels are
// through when the frame returns (the frame has collected its count and verdict), the helper thread only reads it, and
// the call returns after its copy: the next frame's down-sampler, which writes the OTHER workspace and this one a frame
// later, cannot touch what is read here.  Settling first keeps the keyframe's error channel in one place.
int lom_odometry_archive_scan(lom_odometry *o, lom_archive *a, int64_t *id_out)
{
    if (!o || !a || !id_out || lom_archive_device(a) != o->device) return LOM_ERR_ARG;
    if (!o->have_upd) return LOM_ERR_STATE;  // no frame yet
    const int rc = o->settle();
    if (rc != LOM_OK) return rc;
    const int64_t id = lom_archive_add_device(a, o->arch_xyz, o->arch_nrm, o->arch_n, 12, nullptr);
    if (id < 0) {
        o->error = lom_archive_last_error(a);
        return (int)id;
    }
    *id_out = id;
    return LOM_OK;
}

// that cloud, every point of it and no normals, into a scan archive (csrc/archive.hip); reads only
int lom_odometry_archive_deskewed(lom_odometry *o, lom_archive *a, int64_t *id_out)
{
    if (!o || !a || !id_out || lom_archive_device(a) != o->device) return LOM_ERR_ARG;
    if (o->temp_points == 0) return LOM_ERR_STATE;  // no frame yet
    const float *pts = nullptr;
    size_t n = 0;
    void *event = nullptr;
    const int rc = deskewed_cloud(o, &pts, &n, &event);
    if (rc != LOM_OK) return rc;
    const size_t stride = sizeof(lom_point_xyzirt);
    const int64_t id = o->temp_on_device ? lom_archive_add_points_device(a, pts, n, stride, event) : lom_archive_add_points(a, pts, n, stride);
    if (id < 0) {
        o->error = lom_archive_last_error(a);
        return (int)id;
    }
    *id_out = id;
    return LOM_OK;
}

int lom_odometry_occupancy_scan(lom_odometry *o, lom_occupancy *g, const lom_occupancy_ray_params *p, lom_occupancy_stats *stats)
{
    return grid_scan(o, g, p, stats, lom_occupancy_device, lom_occupancy_last_error, lom_occupancy_integrate_cloud_device,
                     lom_occupancy_integrate_cloud);
}

int lom_odometry_elevation_scan(lom_odometry *o, lom_elevation *g, const lom_elevation_point_params *p, lom_elevation_stats *stats)
{
    return grid_scan(o, g, p, stats, lom_elevation_device, lom_elevation_last_error, lom_elevation_integrate_cloud_device,
                     lom_elevation_integrate_cloud);
}

// the keyframe again from archived scans at corrected poses: the steps of the header, in its order
int lom_odometry_rebuild_keyframe(lom_odometry *o, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses,
                                  size_t count, const lom_pose *new_current, lom_assemble_stats *stats)
{
    if (!o || !a || !new_current || (count && (!ids || !poses)) || lom_archive_device(a) != o->device) return LOM_ERR_ARG;
    int rc = o->settle();  // 1.
    if (rc != LOM_OK) return rc;
    if (!o->keyframe_has_voxels) return LOM_ERR_STATE;
    (void)lom_map_radius_cleanup_after_align(o->keyframe, 0.f);  // 2. (disarms)
    o->hint_pts = nullptr;
    o->hint_n = 0;
    if ((rc = lom_map_clear(o->keyframe, o->cfg.keyframe_voxel_size)) != LOM_OK) {  // 3.
        o->error = lom_last_error(o->keyframe);
        return rc;
    }
    o->keyframe_has_voxels = false;
    o->last.keyframe_voxels = 0;
    lom_assemble_params prm;
    for (int i = 0; i < 3; i++) prm.centre[i] = new_current->t[i];
    prm.radius = o->cfg.keyframe_cleanup_range;
    lom_assemble_stats st;
    if ((rc = lom_map_assemble(o->keyframe, a, ids, poses, count, &prm, &st)) != LOM_OK) {  // 4.
        o->error = lom_archive_last_error(a);
        if (stats) std::memset(stats, 0, sizeof *stats);
        return rc;
    }
    if (o->votes_on) {  // lom_odometry_set_rebuild_votes: the scans vote on what they have just built
        lom_vote_stats vs;
        if ((rc = lom_map_carve_scans(o->keyframe, a, ids, poses, count, &o->votes, &vs)) != LOM_OK) {
            o->error = lom_last_error(o->keyframe);
            (void)lom_map_clear(o->keyframe, o->cfg.keyframe_voxel_size);  // as after a failed assembly: left cleared
            if (stats) std::memset(stats, 0, sizeof *stats);
            return rc;
        }
        o->vote_stats = vs;
        o->have_vote_stats = true;
        st.voxels_after -= (int64_t)vs.voxels_erased;
        const int64_t stored = lom_map_point_count(o->keyframe);
        if (stored >= 0) st.points_stored_after = stored;
    }
    o->last.keyframe_voxels = st.voxels_after;
    o->keyframe_has_voxels = st.voxels_after > 0;
    lom_pose inv, corr, prev;  // 5.
    lom_pose_inverse(&o->current, &inv);
    lom_pose_compose(new_current, &inv, &corr);
    lom_pose_compose(&corr, &o->previous, &prev);
    o->previous = prev;
    o->current = *new_current;
    if (stats) *stats = st;
    return LOM_OK;
}

// test hook: overwrite previous_transform_ / current_transform_ (lidar_odometry.h:84-85); together with
// clear + add on lom_odometry_keyframe() this lets a test put the pipeline into a given state before a frame
int lom_odometry_debug_set_state(lom_odometry *o, const lom_pose *previous, const lom_pose *current)
{
    if (!o || !previous || !current) return LOM_ERR_ARG;
    const int rc = o->settle();
    o->previous = *previous;
    o->current = *current;
    o->keyframe_has_voxels = lom_map_size(o->keyframe) > 0;  // the test may have replaced the keyframe
    return rc;
}

int lom_odometry_set_option(lom_odometry *o, int option, int64_t value)
{
    if (!o) return LOM_ERR_ARG;
    int rc = o->settle();
    if (rc != LOM_OK) return rc;
    switch (option) {
    case LOM_OPT_TEST_FORCE_HOST_REDO:
        if (value != 0 && o->classifier == LOM_CLASSIFIER_NEIGHBOURHOOD) return LOM_ERR_STATE;  // no host stages to redo with
        o->test_force_host_redo = value != 0;
        return LOM_OK;
    case LOM_OPT_DEBUG_TIMING: o->debug_timing = value != 0; return lom_map_set_option(o->keyframe, option, value);
    case LOM_OPT_QUALITY_REPORT:
        o->quality_on = value != 0;
        o->have_quality = false;
        return LOM_OK;
    case LOM_OPT_TEST_GRID_GIVE_UP:  // the front end's scan of the next frame
        return o->frontend ? lom_frontend_set_option(o->frontend, option, value) : LOM_ERR_STATE;
    case LOM_OPT_TEST_GRID_GIVE_UP_MATCHING_DS: return lom_map_set_option(o->matching_ds, LOM_OPT_TEST_GRID_GIVE_UP, value);
    case LOM_OPT_TEST_GRID_GIVE_UP_UPDATE_DS:  // the workspace of the NEXT frame
        return lom_map_set_option(o->update_ds2[o->parity ^ 1], LOM_OPT_TEST_GRID_GIVE_UP, value);
    case LOM_OPT_TEST_GRID_GIVE_UP_KEYFRAME: return lom_map_set_option(o->keyframe, LOM_OPT_TEST_GRID_GIVE_UP, value);
    default: return lom_map_set_option(o->keyframe, option, value);  // the align's switches live on the keyframe handle
    }
}

int64_t lom_odometry_debug_counter(const lom_odometry *o, int which)
{
    if (!o) return LOM_ERR_ARG;
    if (which == LOM_COUNTER_GRID_REDOS) {
        int64_t v = o->grid_redos;
        for (lom_map *m : {o->keyframe, o->update_ds2[0], o->update_ds2[1], o->matching_ds}) v += lom_map_debug_counter(m, which);
        if (o->frontend) v += lom_frontend_debug_counter(o->frontend, which);
        return v;
    }
    if (which == LOM_COUNTER_FRAMES_SENT_AHEAD) return (int64_t)o->frames_sent_ahead;
    if (which == LOM_COUNTER_CLEANUPS_BEHIND_ALIGN) {
        const int rc = const_cast<lom_odometry *>(o)->settle();
        return rc != LOM_OK ? rc : lom_map_debug_counter(o->keyframe, which);
    }
    return LOM_ERR_ARG;
}

int lom_odometry_set_classifier(lom_odometry *o, int kind, const lom_neighbourhood_params *p)
{
    // the arguments first, then the state
    if (kind != LOM_CLASSIFIER_RINGS && kind != LOM_CLASSIFIER_NEIGHBOURHOOD) return LOM_ERR_ARG;
    if (kind == LOM_CLASSIFIER_NEIGHBOURHOOD && !lom::neighbourhood_params_ok(p)) return LOM_ERR_ARG;
    if (!o) return LOM_ERR_ARG;
    int rc = o->settle();
    if (rc != LOM_OK) return rc;
    if (kind == LOM_CLASSIFIER_NEIGHBOURHOOD && (!o->frontend || o->test_force_host_redo)) return LOM_ERR_STATE;
    if (o->frontend && (rc = lom_frontend_set_classifier(o->frontend, kind, p)) != LOM_OK) {
        o->error = lom_frontend_last_error(o->frontend);
        return rc;
    }
    o->classifier = kind;
    return LOM_OK;
}

int lom_odometry_set_carve(lom_odometry *o, const lom_carve_params *p)
{
    // the arguments first, then the state
    if (p && !lom::carve_params_ok(p)) return LOM_ERR_ARG;
    if (!o) return LOM_ERR_ARG;
    const int rc = o->settle();  // (the previous frame's update may still be reading the old setting)
    if (rc != LOM_OK) return rc;
    o->carve_on = p != nullptr;
    if (p) o->carve = *p;
    return LOM_OK;
}

int lom_odometry_get_carve_stats(const lom_odometry *o, lom_carve_stats *out)
{
    if (!o || !out) return LOM_ERR_ARG;
    const int rc = const_cast<lom_odometry *>(o)->settle();  // the last carve belongs to the last frame's update
    if (rc != LOM_OK) return rc;
    if (!o->have_carve_stats) return LOM_ERR_STATE;
    *out = o->carve_stats;
    return LOM_OK;
}

int lom_odometry_set_rebuild_votes(lom_odometry *o, const lom_vote_params *p)
{
    // the arguments first, then the state
    if (p && !lom::vote::params_ok(p)) return LOM_ERR_ARG;
    if (!o) return LOM_ERR_ARG;
    o->votes_on = p != nullptr;
    if (p) o->votes = *p;
    return LOM_OK;
}

int lom_odometry_get_rebuild_vote_stats(const lom_odometry *o, lom_vote_stats *out)
{
    if (!o || !out) return LOM_ERR_ARG;
    if (!o->have_vote_stats) return LOM_ERR_STATE;
    *out = o->vote_stats;
    return LOM_OK;
}

int lom_odometry_set_quality_thresholds(lom_odometry *o, float min_eig_t, float min_eig_r)
{
    if (!o) return LOM_ERR_ARG;
    o->quality_min_eig_t = min_eig_t;
    o->quality_min_eig_r = min_eig_r;
    return LOM_OK;
}

int lom_odometry_get_quality(const lom_odometry *o, lom_quality_report *out)
{
    if (!o || !out) return LOM_ERR_ARG;
    if (!o->quality_on || !o->have_quality) return LOM_ERR_STATE;  // option off, or no frame has aligned yet
    *out = o->quality;
    return LOM_OK;
}

int lom_odometry_get_stats(const lom_odometry *o, lom_odometry_frame_stats *out)
{
    if (!o || !out) return LOM_ERR_ARG;
    const int rc = const_cast<lom_odometry *>(o)->settle();  // keyframe_voxels comes from the keyframe update
    *out = o->last;
    return rc;
}

}  // extern "C"
