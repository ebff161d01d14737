// lidar_odometry_amd.hpp -- header-only C++ mirror of the reference's hot-path
// classes over the C ABI of lidar_odometry_amd.h.
//
// Same class and method names, argument meaning and return shapes as
//   Pose3D        reference src/pose_3d.h:10-59
//   VoxelGrid     reference src/voxel_grid.h:17-257
//   CloudMatcher  reference src/cloud_matcher.h:13-17
//   CloudTransformer, CloudClassifier, utils::pointTimeNormalize, utils::rangeFilter  reference src/utils/*.h
//   LidarOdometry reference src/lidar_odometry.h:20-85
// so that reference src/lidar_odometry.cpp compiles against it with a type
// alias or two.  No Eigen / PCL / Ceres / robin_map needed:
// the point structs below have the memory layout of pcl::PointXYZ (16 bytes)
// and pcl::PointNormal (48 bytes, normal at byte 16), and any cloud type whose
// `.points` is a contiguous array of such structs can be passed as is.
//
// Errors: the reference has no error channel; here a failing call throws
// lom::Error (status code + lom_last_error text).  Without a gfx950 device the
// VoxelGrid constructor throws -- there is no CPU fallback.
#pragma once
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "lidar_odometry_amd.h"

namespace lom {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

struct Vector3f {
    float v[3] = {0.f, 0.f, 0.f};
    Vector3f() = default;
    Vector3f(float x, float y, float z) : v{x, y, z} {}
    float x() const { return v[0]; }
    float y() const { return v[1]; }
    float z() const { return v[2]; }
    float operator()(int i) const { return v[i]; }
    float norm() const { return std::sqrt(v[0] * v[0] + (v[1] * v[1] + v[2] * v[2])); }
};

struct Quaternionf {
    float q[4] = {1.f, 0.f, 0.f, 0.f};  // w, x, y, z
    Quaternionf() = default;
    Quaternionf(float w, float x, float y, float z) : q{w, x, y, z} {}
    float w() const { return q[0]; }
    float x() const { return q[1]; }
    float y() const { return q[2]; }
    float z() const { return q[3]; }
    float dot(const Quaternionf &o) const { return q[0] * o.q[0] + q[1] * o.q[1] + q[2] * o.q[2] + q[3] * o.q[3]; }
    static Quaternionf Identity() { return {}; }
};

// pcl::PointXYZ layout (16 bytes)
struct alignas(16) PointXYZ {
    float x = 0.f, y = 0.f, z = 0.f, pad = 1.f;
    PointXYZ() = default;
    PointXYZ(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};
// pcl::PointNormal layout (48 bytes): xyz+pad, normal+pad, curvature+pad
struct alignas(16) PointNormal {
    float x = 0.f, y = 0.f, z = 0.f, pad0 = 1.f;
    float normal_x = 0.f, normal_y = 0.f, normal_z = 0.f, pad1 = 0.f;
    float curvature = 0.f, pad2[3] = {0.f, 0.f, 0.f};
    PointNormal() = default;
    PointNormal(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};
static_assert(sizeof(PointXYZ) == 16 && sizeof(PointNormal) == 48, "PCL layouts");

template <typename PointT>
struct PointCloud {
    std::vector<PointT> points;
    using Ptr = std::shared_ptr<PointCloud<PointT>>;
    size_t size() const { return points.size(); }
    const PointT &at(size_t i) const { return points.at(i); }
};

// ---- Pose3D (src/pose_3d.h) ---------------------------------------------------
class Pose3D {
public:
    Vector3f translation;
    Quaternionf rotation;

    Pose3D() = default;
    Pose3D(const Vector3f &t, const Quaternionf &q) : translation(t), rotation(q) {}

    Pose3D relativeTo(const Pose3D &target) const
    {
        lom_pose a = c(), b = target.c(), o;
        lom_pose_relative_to(&a, &b, &o);
        return from(o);
    }
    Pose3D compose(const Pose3D &another) const
    {
        lom_pose a = c(), b = another.c(), o;
        lom_pose_compose(&a, &b, &o);
        return from(o);
    }
    Pose3D inverse() const
    {
        lom_pose a = c(), o;
        lom_pose_inverse(&a, &o);
        return from(o);
    }
    // row-major 3x3
    void rotationMatrix(float R[9]) const
    {
        lom_pose a = c();
        lom_pose_rotation_matrix(&a, R);
    }

    lom_pose c() const
    {
        lom_pose p;
        for (int i = 0; i < 3; i++) p.t[i] = translation.v[i];
        for (int i = 0; i < 4; i++) p.q[i] = rotation.q[i];
        return p;
    }
    static Pose3D from(const lom_pose &p)
    {
        return {Vector3f(p.t[0], p.t[1], p.t[2]), Quaternionf(p.q[0], p.q[1], p.q[2], p.q[3])};
    }
};

// ---- VoxelGrid (src/voxel_grid.h) -----------------------------------------------
class ScanArchive;  // below, behind PoseGraph

class VoxelGrid {
public:
    struct Correspondence {  // voxel_grid.h:40-46 (f64 like the reference)
        double source_point_local[3] = {0, 0, 0};
        double plane_origin[3] = {0, 0, 0};
        double plane_normal[3] = {0, 0, 0};
        bool valid = false;
    };

    VoxelGrid() : VoxelGrid(0.5f, 10) {}  // voxel_grid.h:253-254 defaults
    VoxelGrid(float voxel_size, size_t max_points, int device = 0)
    {
        const int rc = lom_map_create(voxel_size, max_points, 0, device, &h_);
        if (rc != LOM_OK) throw Error(rc, std::string("lom_map_create: ") + lom_last_error(nullptr));
    }
    ~VoxelGrid()
    {
        for (lom_scan *s : scans_) lom_scan_destroy(s);  // contexts go before their map
        lom_map_destroy(h_);
    }
    VoxelGrid(const VoxelGrid &) = delete;
    VoxelGrid &operator=(const VoxelGrid &) = delete;
    VoxelGrid(VoxelGrid &&o) noexcept : h_(o.h_), id_(o.id_), scans_(std::move(o.scans_))
    {
        o.h_ = nullptr;
        o.scans_.clear();
    }

    // The const members of the reference (getCorrespondence, findMatchingPairs, and CloudMatcher::align, which takes
    // `const VoxelGrid&`) may be called from several threads at once.  A map handle is single-caller, so every thread
    // gets a scan context of its own for this grid (lom_scan_create: stream, per-scan buffers, solve state), created
    // on its first such call and owned by the grid.  As in the reference, nobody may change the grid meanwhile.
    lom_scan *scan_context() const
    {
        thread_local std::unordered_map<uint64_t, lom_scan *> mine;  // this thread's contexts, by grid id
        auto it = mine.find(id_);
        if (it != mine.end()) return it->second;
        lom_scan *s = nullptr;
        const int rc = lom_scan_create(h_, &s);
        if (rc != LOM_OK) throw Error(rc, lom_last_error(h_));
        {
            std::lock_guard<std::mutex> lock(scans_mutex_);
            scans_.push_back(s);
        }
        mine.emplace(id_, s);
        return s;
    }

    void setMaxPoints(size_t max_points) { check(lom_map_set_max_points(h_, max_points)); }
    void setVoxelSize(float voxel_size) { check(lom_map_clear(h_, voxel_size)); }

    void addCloud(const PointCloud<PointNormal> &cloud)
    {
        if (cloud.points.empty()) return;
        const PointNormal *p = cloud.points.data();
        check(lom_map_add_points(h_, &p->x, &p->normal_x, cloud.points.size(), sizeof(PointNormal)));
    }
    void addCloudWithoutNormals(const PointCloud<PointXYZ> &cloud)
    {
        if (cloud.points.empty()) return;
        check(lom_map_add_points(h_, &cloud.points.data()->x, nullptr, cloud.points.size(), sizeof(PointXYZ)));
    }

    PointCloud<PointNormal>::Ptr getCloud() const
    {
        auto out = std::make_shared<PointCloud<PointNormal>>();
        std::vector<float> xyz, nrm;
        const size_t n = fetch(LOM_EXPORT_FULL, xyz, &nrm);
        out->points.resize(n);
        for (size_t i = 0; i < n; i++) {
            PointNormal &p = out->points[i];
            p.x = xyz[3 * i], p.y = xyz[3 * i + 1], p.z = xyz[3 * i + 2];
            p.normal_x = nrm[3 * i], p.normal_y = nrm[3 * i + 1], p.normal_z = nrm[3 * i + 2];
        }
        return out;
    }
    PointCloud<PointXYZ>::Ptr getCloudWithoutNormals() const { return xyz_cloud(LOM_EXPORT_FULL_NO_NORMALS); }
    PointCloud<PointXYZ>::Ptr getSparseCloudWithoutNormals() const { return xyz_cloud(LOM_EXPORT_FIRST_PER_VOXEL); }

    // voxel_grid.h:164-204, query already in the map frame
    Correspondence getCorrespondence(const Vector3f &query, double max_correspondence_distance_sq) const
    {
        PointCloud<PointXYZ> one;
        one.points.emplace_back(query.x(), query.y(), query.z());
        auto v = findAll(one, Pose3D(), 0.f, &max_correspondence_distance_sq);  // the squared threshold as it is (:164)
        Correspondence c = v[0];
        for (double &d : c.source_point_local) d = 0.0;  // the reference leaves it unset here
        return c;
    }

    // voxel_grid.h:206-234: valid correspondences only, in source order (the reference's
    // order under its mutex is unspecified)
    std::vector<Correspondence> findMatchingPairs(const PointCloud<PointXYZ> &cloud, const Pose3D &transform,
                                                  float max_correspondence_distance) const
    {
        std::vector<Correspondence> all = findAll(cloud, transform, max_correspondence_distance), out;
        out.reserve(all.size());
        for (const auto &c : all)
            if (c.valid) out.push_back(c);
        return out;
    }

    void radiusCleanup(const Vector3f &point, float radius) { check(lom_map_radius_cleanup(h_, point.v, radius)); }
    // not in the reference: the scans `ids` of the archive at the f64 `poses`, in call order, as one addCloud of their
    // concatenation (lom_map_assemble); params: nullptr keeps everything, else only the points within radius of centre
    inline lom_assemble_stats assemble(ScanArchive &archive, const std::vector<int64_t> &ids,
                                       const std::vector<lom_graph_pose> &poses, const lom_assemble_params *params = nullptr);
    // not in the reference: says that the next align on this grid is followed by radiusCleanup(<its result translation>,
    // radius), as lidar_odometry.cpp:65-67 does -- the cleanup's scan then runs right behind the align (results never differ)
    void radiusCleanupAfterAlign(float radius) { check(lom_map_radius_cleanup_after_align(h_, radius)); }
    // not in the reference: ray carving ("ray carving" in lidar_odometry_amd.h) -- erase the voxels that at least
    // params.min_crossings rays origin -> cloud[i] of this call pass through and no cloud[i] falls into
    lom_carve_stats carveRays(const Vector3f &origin, const PointCloud<PointXYZ> &cloud, const lom_carve_params &params)
    {
        lom_carve_stats st{};
        check(lom_map_carve_rays(h_, origin.v, cloud.points.empty() ? nullptr : &cloud.points.data()->x, cloud.points.size(),
                                 sizeof(PointXYZ), &params, &st));
        return st;
    }
    // not in the reference: scan votes ("scan votes" in lidar_odometry_amd.h) -- the scans `ids` of the archive at the
    // f64 `poses` vote on this map's voxels, seen or seen through, and the voxels the rule of `params` condemns are erased
    inline lom_vote_stats carveScans(ScanArchive &archive, const std::vector<int64_t> &ids,
                                     const std::vector<lom_graph_pose> &poses, const lom_vote_params &params);
    // ... erases nothing: free / seen per live voxel in the export's order
    inline void scanVotes(ScanArchive &archive, const std::vector<int64_t> &ids, const std::vector<lom_graph_pose> &poses,
                          const lom_vote_params &params, std::vector<uint32_t> &free_out, std::vector<uint32_t> &seen_out);

    size_t size() const
    {
        const int64_t n = lom_map_size(h_);
        if (n < 0) throw Error((int)n, "lom_map_size");
        return (size_t)n;
    }

    lom_map *handle() const { return h_; }

private:
    void check(int rc) const
    {
        if (rc < 0) throw Error(rc, lom_last_error(h_));
    }
    size_t fetch(int mode, std::vector<float> &xyz, std::vector<float> *nrm) const
    {
        const int64_t n = lom_map_export(h_, mode, nullptr, nullptr, 0);
        if (n < 0) throw Error((int)n, lom_last_error(h_));
        xyz.resize((size_t)n * 3);
        if (nrm) nrm->resize((size_t)n * 3);
        if (n) {
            const int64_t m = lom_map_export(h_, mode, xyz.data(), nrm ? nrm->data() : nullptr, (size_t)n);
            if (m < 0) throw Error((int)m, lom_last_error(h_));
        }
        return (size_t)n;
    }
    PointCloud<PointXYZ>::Ptr xyz_cloud(int mode) const
    {
        auto out = std::make_shared<PointCloud<PointXYZ>>();
        std::vector<float> xyz;
        const size_t n = fetch(mode, xyz, nullptr);
        out->points.resize(n);
        for (size_t i = 0; i < n; i++) out->points[i] = PointXYZ(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
        return out;
    }
    std::vector<Correspondence> findAll(const PointCloud<PointXYZ> &cloud, const Pose3D &transform, float max_dist,
                                        const double *max_dist_sq = nullptr) const
    {
        std::vector<lom_correspondence> raw(cloud.points.size());
        std::vector<Correspondence> out(cloud.points.size());
        if (cloud.points.empty()) return out;
        const lom_pose p = transform.c();
        lom_scan *ctx = scan_context();
        const int64_t rc = max_dist_sq ? lom_scan_find_pairs_sq(ctx, &cloud.points.data()->x, cloud.points.size(),
                                                                sizeof(PointXYZ), p.t, p.q, *max_dist_sq, raw.data())
                                       : lom_scan_find_pairs(ctx, &cloud.points.data()->x, cloud.points.size(),
                                                             sizeof(PointXYZ), p.t, p.q, max_dist, raw.data());
        if (rc < 0) throw Error((int)rc, lom_scan_last_error(ctx));
        for (size_t i = 0; i < raw.size(); i++) {
            Correspondence &c = out[i];
            c.valid = raw[i].index >= 0;
            c.source_point_local[0] = cloud.points[i].x;
            c.source_point_local[1] = cloud.points[i].y;
            c.source_point_local[2] = cloud.points[i].z;
            for (int a = 0; a < 3; a++) {
                c.plane_origin[a] = raw[i].origin[a];
                c.plane_normal[a] = raw[i].normal[a];
            }
        }
        return out;
    }

    static uint64_t next_id()
    {
        static std::atomic<uint64_t> n{1};
        return n.fetch_add(1);
    }
    lom_map *h_ = nullptr;
    uint64_t id_ = next_id();  // never reused: a thread's cached context of a destroyed grid is never looked up again
    mutable std::mutex scans_mutex_;
    mutable std::vector<lom_scan *> scans_;
};

// lom_quality_report as it is: counts, fit, information (rotation first, half-angle tangent), block spectra, and the
// 6x6 covariance in nav_msgs order (row-major; zeros with covariance_valid == 0 where the geometry is degenerate)
using QualityReport = lom_quality_report;

// lom_pose_lattice: the poses of a lattice around `centre` -- per axis 2 * floor(half_extent / step) + 1 nodes (one where
// the step is <= 0 or the extent below it), translation offsets in the world frame, yaw about world Z from the left;
// order: yaw outermost, then x, y, and z innermost, each ascending
inline std::vector<Pose3D> poseLattice(const Pose3D &centre, const Vector3f &half_extent_xyz, const Vector3f &step_xyz,
                                       float half_extent_yaw_rad = 0.f, float step_yaw_rad = 0.f)
{
    const lom_pose c = centre.c();
    const int n = lom_pose_lattice(&c, half_extent_xyz.v, step_xyz.v, half_extent_yaw_rad, step_yaw_rad, nullptr, 0);
    if (n < 0) throw Error(n, "poseLattice: non-finite input or too many nodes");
    std::vector<lom_pose> raw((size_t)n);
    lom_pose_lattice(&c, half_extent_xyz.v, step_xyz.v, half_extent_yaw_rad, step_yaw_rad, raw.data(), n);
    std::vector<Pose3D> out;
    out.reserve(raw.size());
    for (const lom_pose &p : raw) out.push_back(Pose3D::from(p));
    return out;
}

// ---- CloudMatcher (src/cloud_matcher.h) --------------------------------------------
class CloudMatcher {
public:
    // How good is `pose` (what align() returned, a loop-closure candidate) for this cloud against this keyframe:
    // lom_scan_quality on the calling thread's scan context.  residuals_or_null: resized to the cloud, the signed
    // point-to-plane residual per point, NaN where it has no correspondence.
    QualityReport quality(const VoxelGrid &keyframe, const PointCloud<PointXYZ> &cloud, const Pose3D &pose,
                          float max_correspondence_distance = 0.3f, float min_eig_t = 0.f, float min_eig_r = 0.f,
                          std::vector<float> *residuals_or_null = nullptr) const
    {
        const lom_pose g = pose.c();
        const float *src = cloud.points.empty() ? nullptr : &cloud.points.data()->x;
        if (residuals_or_null) residuals_or_null->resize(cloud.points.size());
        float *res = residuals_or_null && !cloud.points.empty() ? residuals_or_null->data() : nullptr;
        QualityReport out;
        lom_scan *ctx = keyframe.scan_context();
        const int rc = lom_scan_quality(ctx, src, cloud.points.size(), sizeof(PointXYZ), g.t, g.q,
                                        max_correspondence_distance, min_eig_t, min_eig_r, &out, res);
        if (rc != LOM_OK) throw Error(rc, lom_scan_last_error(ctx));
        return out;
    }
    // K candidates scored in one call (lom_scan_quality_batch on the calling thread's scan context): report i is what
    // quality(keyframe, *clouds[i], poses[i]) describes; the best candidate's index (most valid correspondences, then
    // lowest cost) in `best`, -1 for none.  A cloud that appears several times is uploaded once.
    std::vector<QualityReport> qualityBatch(const VoxelGrid &keyframe, const std::vector<const PointCloud<PointXYZ> *> &clouds,
                                            const std::vector<Pose3D> &poses, float max_correspondence_distance = 0.3f,
                                            float min_eig_t = 0.f, float min_eig_r = 0.f)
    {
        if (clouds.size() != poses.size()) throw Error(LOM_ERR_ARG, "qualityBatch: one pose per cloud");
        std::vector<lom_quality_problem> p(clouds.size());
        for (size_t i = 0; i < clouds.size(); i++) {
            if (!clouds[i]) throw Error(LOM_ERR_ARG, "qualityBatch: null cloud");
            const lom_pose g = poses[i].c();
            p[i].xyz = clouds[i]->points.empty() ? nullptr : &clouds[i]->points.data()->x;
            p[i].n = clouds[i]->points.size();
            p[i].stride_bytes = sizeof(PointXYZ);
            for (int a = 0; a < 3; a++) p[i].t[a] = g.t[a];
            for (int a = 0; a < 4; a++) p[i].q_wxyz[a] = g.q[a];
        }
        std::vector<QualityReport> out(p.size());
        lom_scan *ctx = keyframe.scan_context();
        const int rc = lom_scan_quality_batch(ctx, p.data(), (int)p.size(), max_correspondence_distance, min_eig_t, min_eig_r,
                                              out.data(), &best);
        if (rc != LOM_OK) throw Error(rc, lom_scan_last_error(ctx));
        return out;
    }
    // one cloud at many poses: the pose-lattice case (see poseLattice)
    std::vector<QualityReport> qualityBatch(const VoxelGrid &keyframe, const PointCloud<PointXYZ> &cloud,
                                            const std::vector<Pose3D> &poses, float max_correspondence_distance = 0.3f,
                                            float min_eig_t = 0.f, float min_eig_r = 0.f)
    {
        return qualityBatch(keyframe, std::vector<const PointCloud<PointXYZ> *>(poses.size(), &cloud), poses,
                            max_correspondence_distance, min_eig_t, min_eig_r);
    }
    // lom_quality_batch_best: the most valid, then the lower cost, then the lower index; -1 for none
    static int bestQuality(const std::vector<QualityReport> &reports)
    {
        return lom_quality_batch_best(reports.data(), (int)reports.size());
    }
    Pose3D align(const VoxelGrid &keyframe, const PointCloud<PointXYZ> &planar_cloud, const Pose3D &position_guess)
    {
        const lom_pose g = position_guess.c();
        lom_pose o;
        const float *src = planar_cloud.points.empty() ? nullptr : &planar_cloud.points.data()->x;
        // stateless like the reference's (lidar_odometry.cpp:49 constructs one per frame): the solve state lives in the
        // calling thread's scan context of this keyframe, so several threads may align against one grid at a time
        lom_scan *ctx = keyframe.scan_context();
        const int rc = lom_scan_align(ctx, src, planar_cloud.points.size(), sizeof(PointXYZ), g.t, g.q, o.t, o.q, &last_stats);
        if (rc != LOM_OK) throw Error(rc, lom_scan_last_error(ctx));
        return Pose3D::from(o);
    }
    // K (cloud, guess) problems against one keyframe in one call (lom_scan_align_batch): the poses align() would return
    // for each, bit for bit; per-problem stats in batch_stats, the best problem's index in best (-1 for none)
    std::vector<Pose3D> alignBatch(const VoxelGrid &keyframe, const std::vector<const PointCloud<PointXYZ> *> &clouds,
                                   const std::vector<Pose3D> &guesses)
    {
        if (clouds.size() != guesses.size()) throw Error(LOM_ERR_ARG, "alignBatch: one guess per cloud");
        std::vector<lom_align_problem> p(clouds.size());
        for (size_t i = 0; i < clouds.size(); i++) {
            if (!clouds[i]) throw Error(LOM_ERR_ARG, "alignBatch: null cloud");
            const lom_pose g = guesses[i].c();
            p[i].xyz = clouds[i]->points.empty() ? nullptr : &clouds[i]->points.data()->x;
            p[i].n = clouds[i]->points.size();
            p[i].stride_bytes = sizeof(PointXYZ);
            for (int a = 0; a < 3; a++) p[i].guess_t[a] = g.t[a];
            for (int a = 0; a < 4; a++) p[i].guess_q_wxyz[a] = g.q[a];
        }
        std::vector<lom_align_result> r(p.size());
        lom_scan *ctx = keyframe.scan_context();
        const int rc = lom_scan_align_batch(ctx, p.data(), (int)p.size(), r.data(), &best);
        if (rc != LOM_OK) throw Error(rc, lom_scan_last_error(ctx));
        std::vector<Pose3D> out;
        batch_stats.clear();
        for (const lom_align_result &x : r) {
            lom_pose o;
            for (int a = 0; a < 3; a++) o.t[a] = x.t[a];
            for (int a = 0; a < 4; a++) o.q[a] = x.q_wxyz[a];
            out.push_back(Pose3D::from(o));
            batch_stats.push_back(x.stats);
        }
        return out;
    }
    // K (cloud, guess) problems, problem i against *keyframes[i], in one call (lom_match_align_multi, keyframes[0] carries
    // the device chain): the poses align(*keyframes[i], ...) would return, bit for bit; stats and best as alignBatch's
    std::vector<Pose3D> alignMulti(const std::vector<const VoxelGrid *> &keyframes,
                                   const std::vector<const PointCloud<PointXYZ> *> &clouds, const std::vector<Pose3D> &guesses)
    {
        if (clouds.size() != guesses.size() || clouds.size() != keyframes.size())
            throw Error(LOM_ERR_ARG, "alignMulti: one keyframe and one guess per cloud");
        std::vector<lom_align_multi_problem> p(clouds.size());
        for (size_t i = 0; i < clouds.size(); i++) {
            if (!clouds[i] || !keyframes[i]) throw Error(LOM_ERR_ARG, "alignMulti: null cloud or keyframe");
            const lom_pose g = guesses[i].c();
            p[i].map = keyframes[i]->handle();
            p[i].xyz = clouds[i]->points.empty() ? nullptr : &clouds[i]->points.data()->x;
            p[i].n = clouds[i]->points.size();
            p[i].stride_bytes = sizeof(PointXYZ);
            for (int a = 0; a < 3; a++) p[i].guess_t[a] = g.t[a];
            for (int a = 0; a < 4; a++) p[i].guess_q_wxyz[a] = g.q[a];
        }
        std::vector<lom_align_result> r(p.size());
        batch_stats.clear();
        if (p.empty()) {
            best = -1;
            return {};
        }
        lom_map *runner = keyframes[0]->handle();
        const int rc = lom_match_align_multi(runner, p.data(), (int)p.size(), r.data(), &best);
        if (rc != LOM_OK) throw Error(rc, lom_last_error(runner));
        std::vector<Pose3D> out;
        for (const lom_align_result &x : r) {
            lom_pose o;
            for (int a = 0; a < 3; a++) o.t[a] = x.t[a];
            for (int a = 0; a < 4; a++) o.q[a] = x.q_wxyz[a];
            out.push_back(Pose3D::from(o));
            batch_stats.push_back(x.stats);
        }
        return out;
    }
    lom_align_stats last_stats{};
    std::vector<lom_align_stats> batch_stats;
    int best = -1;
};

// ---- CloudTransformer::transform / transformWithNormals (src/utils/cloud_transform.h:43-97)
struct CloudTransformer {
    static PointCloud<PointXYZ>::Ptr transform(const PointCloud<PointXYZ> &input, const Pose3D &pose)
    {
        auto out = std::make_shared<PointCloud<PointXYZ>>();
        out->points = input.points;
        if (input.points.empty()) return out;
        const lom_pose p = pose.c();
        lom_transform_points(&p, &input.points.data()->x, nullptr, input.points.size(), sizeof(PointXYZ),
                             &out->points.data()->x, nullptr, sizeof(PointXYZ));
        return out;
    }
    // transformNonRigid (cloud_transform.h:15-40): the deskew, on the host (lom::LidarOdometry runs it on the device)
    static PointCloud<lom_point_xyzirt>::Ptr transformNonRigid(const PointCloud<lom_point_xyzirt> &input,
                                                              const Pose3D &start_pose, const Pose3D &end_pose)
    {
        auto out = std::make_shared<PointCloud<lom_point_xyzirt>>();
        out->points.resize(input.points.size());
        const lom_pose s = start_pose.c(), e = end_pose.c();
        lom_transform_non_rigid(input.points.data(), input.points.size(), &s, &e, out->points.data());
        return out;
    }
    static PointCloud<PointNormal>::Ptr transformWithNormals(const PointCloud<PointNormal> &input, const Pose3D &pose)
    {
        auto out = std::make_shared<PointCloud<PointNormal>>();
        out->points = input.points;
        if (input.points.empty()) return out;
        const lom_pose p = pose.c();
        lom_transform_points(&p, &input.points.data()->x, &input.points.data()->normal_x, input.points.size(),
                             sizeof(PointNormal), &out->points.data()->x, &out->points.data()->normal_x,
                             sizeof(PointNormal));
        return out;
    }
};

// ---- the stages processCloud runs before the align (src/lidar_odometry.cpp:25-35), host functions of the library
// with the reference's names: a caller that keeps the reference's own orchestration but not PCL uses these;
// lom::LidarOdometry below runs the same stages on the device.
using PointXYZIRT = lom_point_xyzirt;  // lidar_point::PointXYZIRT (src/lidar_point_type.h:13-31), same 32-byte layout

namespace utils {
// utils::pointTimeNormalize (src/utils/point_time_normalize.h:15-39)
inline PointCloud<PointXYZIRT>::Ptr pointTimeNormalize(const PointCloud<PointXYZIRT> &input)
{
    auto out = std::make_shared<PointCloud<PointXYZIRT>>();
    out->points.resize(input.points.size());
    lom_point_time_normalize(input.points.data(), input.points.size(), out->points.data());
    return out;
}
// utils::rangeFilter (src/utils/range_filter.h:13-28) for the two point types the reference's data flow holds
inline PointCloud<PointNormal>::Ptr rangeFilter(const PointCloud<PointNormal> &input, float min_range, float max_range)
{
    const size_t n = input.points.size();
    std::vector<float> xyz(3 * n + 3), nrm(3 * n + 3), fx(3 * n + 3), fn(3 * n + 3);
    for (size_t i = 0; i < n; i++) {
        const PointNormal &p = input.points[i];
        xyz[3 * i] = p.x, xyz[3 * i + 1] = p.y, xyz[3 * i + 2] = p.z;
        nrm[3 * i] = p.normal_x, nrm[3 * i + 1] = p.normal_y, nrm[3 * i + 2] = p.normal_z;
    }
    const size_t m = lom_range_filter(xyz.data(), nrm.data(), n, min_range, max_range, fx.data(), fn.data());
    auto out = std::make_shared<PointCloud<PointNormal>>();
    out->points.resize(m);
    for (size_t i = 0; i < m; i++) {
        PointNormal &p = out->points[i];
        p.x = fx[3 * i], p.y = fx[3 * i + 1], p.z = fx[3 * i + 2];
        p.normal_x = fn[3 * i], p.normal_y = fn[3 * i + 1], p.normal_z = fn[3 * i + 2];
    }
    return out;
}
inline PointCloud<PointXYZ>::Ptr rangeFilter(const PointCloud<PointXYZ> &input, float min_range, float max_range)
{
    const size_t n = input.points.size();
    std::vector<float> xyz(3 * n + 3), fx(3 * n + 3);
    for (size_t i = 0; i < n; i++) xyz[3 * i] = input.points[i].x, xyz[3 * i + 1] = input.points[i].y, xyz[3 * i + 2] = input.points[i].z;
    const size_t m = lom_range_filter(xyz.data(), nullptr, n, min_range, max_range, fx.data(), nullptr);
    auto out = std::make_shared<PointCloud<PointXYZ>>();
    out->points.reserve(m);
    for (size_t i = 0; i < m; i++) out->points.emplace_back(fx[3 * i], fx[3 * i + 1], fx[3 * i + 2]);
    return out;
}
}  // namespace utils

// CloudClassifier::classify (src/utils/cloud_classifier.h:19-168): {planar points with normals, unclassified points}.
// The second cloud is returned with the reference's SIZE only (default points): its one caller drops it
// (src/lidar_odometry.cpp:33), and the library does not build it.
struct CloudClassifier {
    static std::pair<PointCloud<PointNormal>::Ptr, PointCloud<PointXYZIRT>::Ptr> classify(const PointCloud<PointXYZIRT> &input)
    {
        const size_t n = input.points.size();
        std::vector<float> xyz(3 * n + 3), nrm(3 * n + 3);
        size_t unclassified = 0;
        const size_t m = lom_cloud_classify(input.points.data(), n, xyz.data(), nrm.data(), &unclassified, nullptr);
        auto planar = std::make_shared<PointCloud<PointNormal>>();
        planar->points.resize(m);
        for (size_t i = 0; i < m; i++) {
            PointNormal &p = planar->points[i];
            p.x = xyz[3 * i], p.y = xyz[3 * i + 1], p.z = xyz[3 * i + 2];
            p.normal_x = nrm[3 * i], p.normal_y = nrm[3 * i + 1], p.normal_z = nrm[3 * i + 2];
        }
        auto rest = std::make_shared<PointCloud<PointXYZIRT>>();
        rest->points.resize(unclassified);
        return {planar, rest};
    }
};

// ---- handle owners (not in the reference) ---------------------------------------------------------------------
// The base of every class below that owns one handle of a family of the C ABI with lom_<family>_destroy and
// lom_<family>_last_error (VoxelGrid and LidarOdometry own more than that and stay on their own): the pointer, no copies,
// handle(), the destroy, and check(), which throws with the handle's last error.  A constructor that throws leaves h_ null
// for this destructor, and every lom_<family>_destroy returns at once for a null handle, so nobody tests h_.  The
// destructor runs after the derived class's members are gone and reads none of them.
template <typename H, auto Destroy, auto LastError>
class Handle {
public:
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    H *handle() const { return h_; }

protected:
    Handle() = default;
    ~Handle() { Destroy(h_); }
    void created(int rc) const  // a constructor's, with what lom_<family>_create returned
    {
        if (rc != LOM_OK) throw Error(rc, LastError(nullptr));
    }
    int64_t check(int64_t rc) const
    {
        if (rc < 0) throw Error((int)rc, LastError(h_));
        return rc;
    }
    H *h_ = nullptr;
};

// ... and of the seven grids, by the ten entry points every grid family has: construction from a geometry G and a
// device, geometry(), the cell count, clear(), shift(), setOption(), device(), stream() (a hipStream_t) and waitEvent()
// (the grid's stream waits for a hipEvent_t before what is enqueued next)
template <typename H, typename G, auto Create, auto Destroy, auto LastError, auto GetGeometry, auto Clear, auto Shift, auto SetOption, auto Device,
          auto Stream, auto WaitEvent>
class GridHandle : public Handle<H, Destroy, LastError> {
public:
    G geometry() const
    {
        G g;
        this->check(GetGeometry(this->h_, &g));
        return g;
    }
    void clear() { this->check(Clear(this->h_)); }
    // the window moves by (dx, dy) whole cells ("grid shift"): an occupancy or elevation grid keeps what still overlaps and
    // clears what enters; a planning grid is left as its clear() leaves it
    void shift(int32_t dx, int32_t dy) { this->check(Shift(this->h_, dx, dy)); }
    void setOption(int option, int64_t value) { this->check(SetOption(this->h_, option, value)); }
    int device() const { return Device(this->h_); }
    void *stream() const { return Stream(this->h_); }
    void waitEvent(void *hip_event) { this->check(WaitEvent(this->h_, hip_event)); }

protected:
    // (extra: what a family's create takes between the device and the handle -- a NavFieldSet's max_fields)
    template <typename... Extra>
    GridHandle(const G &geometry, int device, Extra... extra)
    {
        this->created(Create(&geometry, device, extra..., &this->h_));
    }
    size_t cellCount() const
    {
        const G g = geometry();
        return (size_t)g.width * g.height;
    }
};

// ---- classifier for frames without rings (not in the reference; lom_classify_neighbourhood) ----------------------
using NeighbourhoodParams = lom_neighbourhood_params;  // {radius, index_cap, min_neighbours, max_variation, min_spread}

// the per-frame front end on the device (lom_frontend_*): here as the owner of the neighbourhood classifier's workspace
class FrontEnd : public Handle<lom_frontend, lom_frontend_destroy, lom_frontend_last_error> {
public:
    explicit FrontEnd(int device = 0)
    {
        const int rc = lom_frontend_create(device, nullptr, &h_);
        if (rc != LOM_OK) throw Error(rc, "lom_frontend_create");
    }
    // LOM_CLASSIFIER_RINGS (params ignored) or LOM_CLASSIFIER_NEIGHBOURHOOD for the following lom_frontend_process calls
    void setClassifier(int kind, const NeighbourhoodParams *params = nullptr) { check(lom_frontend_set_classifier(h_, kind, params)); }
};

// the stage alone: the planar points of `input` in input order, with normals; `details` (optional): one record per input point
inline PointCloud<PointNormal>::Ptr classifyNeighbourhood(FrontEnd &fe, const PointCloud<lom_point_xyzirt> &input,
                                                          const NeighbourhoodParams &params,
                                                          std::vector<lom_neighbourhood_detail> *details = nullptr)
{
    const size_t n = input.points.size();
    std::vector<float> xyz(3 * n + 3), nrm(3 * n + 3);
    if (details) details->resize(n);
    const int64_t m = lom_classify_neighbourhood(fe.handle(), input.points.data(), n, &params, xyz.data(), nrm.data(),
                                                 details ? details->data() : nullptr);
    if (m < 0) throw Error((int)m, lom_frontend_last_error(fe.handle()));
    auto planar = std::make_shared<PointCloud<PointNormal>>();
    planar->points.resize((size_t)m);
    for (size_t i = 0; i < (size_t)m; i++) {
        PointNormal &p = planar->points[i];
        p.x = xyz[3 * i], p.y = xyz[3 * i + 1], p.z = xyz[3 * i + 2];
        p.normal_x = nrm[3 * i], p.normal_y = nrm[3 * i + 1], p.normal_z = nrm[3 * i + 2];
    }
    return planar;
}

// ---- place recognition (lom_place_*; not in the reference) --------------------------------------------
// Scan descriptors (a polar height image in the style of Scan Context) and a database of them in HBM: which earlier
// place a scan belongs to, and the yaw of a pose guess against it.  Definitions: lidar_odometry_amd.h.
using PlaceParams = lom_place_params;  // {rings, sectors, max_range, z_floor}; there are no defaults
using PlaceMatch = lom_place_match;    // {id, distance, shift}

class PlaceDatabase : public Handle<lom_place_db, lom_place_db_destroy, lom_place_db_last_error> {
public:
    explicit PlaceDatabase(const PlaceParams &params, size_t capacity_hint = 0, int device = 0) : params_(params)
    {
        created(lom_place_db_create(&params, device, capacity_hint, &h_));
    }
    const PlaceParams &params() const { return params_; }
    size_t cells() const { return (size_t)params_.rings * params_.sectors; }
    size_t size() const { return (size_t)check(lom_place_db_size(h_)); }
    void clear() { check(lom_place_db_clear(h_)); }

    // the raw rings x sectors descriptor (ring-major) of a cloud; any point type that starts with x, y, z
    template <typename PointT>
    std::vector<float> describe(const PointCloud<PointT> &cloud) const
    {
        std::vector<float> out(cells());
        check(lom_place_describe(h_, reinterpret_cast<const float *>(cloud.points.data()), cloud.points.size(), sizeof(PointT),
                                 out.data()));
        return out;
    }
    int64_t add(const std::vector<float> &descriptor)
    {
        if (descriptor.size() != cells()) throw Error(LOM_ERR_ARG, "PlaceDatabase::add: rings * sectors values");
        return check(lom_place_db_add(h_, descriptor.data()));
    }
    template <typename PointT>
    int64_t addCloud(const PointCloud<PointT> &cloud)  // describe + add, the descriptor stays in HBM
    {
        return check(lom_place_db_add_cloud(h_, reinterpret_cast<const float *>(cloud.points.data()), cloud.points.size(),
                                            sizeof(PointT)));
    }
    std::vector<float> get(int64_t id) const
    {
        std::vector<float> out(cells());
        check(lom_place_db_get(h_, id, out.data()));
        return out;
    }
    // q descriptors (q * rings * sectors values) against the entries [id_begin, id_end) (id_end < 0: all): q * k matches,
    // the nearest first; all_dist_or_null: resized to q * (id_end - id_begin) distances
    std::vector<PlaceMatch> query(const std::vector<float> &descriptors, int k, int64_t id_begin = 0, int64_t id_end = -1,
                                  std::vector<float> *all_dist_or_null = nullptr) const
    {
        if (descriptors.empty() || descriptors.size() % cells()) throw Error(LOM_ERR_ARG, "PlaceDatabase::query: whole descriptors");
        const int q = (int)(descriptors.size() / cells());
        if (id_end < 0) id_end = (int64_t)size();
        if (k < 1 || k > 64 || id_begin < 0 || id_begin > id_end) throw Error(LOM_ERR_ARG, "PlaceDatabase::query: k or id range");
        std::vector<PlaceMatch> out((size_t)q * (size_t)k);
        if (all_dist_or_null) all_dist_or_null->resize((size_t)q * (size_t)(id_end - id_begin));
        check(lom_place_db_query(h_, descriptors.data(), q, id_begin, id_end, k, out.data(),
                                 all_dist_or_null ? all_dist_or_null->data() : nullptr));
        return out;
    }
    // psi = ((S - shift) mod S) 2 pi / S: the rotation about z that takes the entry's cloud onto the query's; the query
    // sensor's rotation in the entry's frame is Rz(-psi)
    static double shiftYaw(const PlaceParams &params, uint32_t shift)
    {
        const double yaw = lom_place_shift_yaw(&params, shift);
        if (yaw != yaw) throw Error(LOM_ERR_ARG, "PlaceDatabase::shiftYaw: invalid parameters");
        return yaw;
    }
    double shiftYaw(uint32_t shift) const { return shiftYaw(params_, shift); }

private:
    PlaceParams params_;
};

// ---- pose graph (lom_graph_*; not in the reference) --------------------------------------------------------
// Keyframe poses and the relative poses measured between them, in HBM, optimised on the device: the stage behind
// PlaceDatabase::query, poseLattice / qualityBatch and align.  Definitions: lidar_odometry_amd.h ("pose graph").
using GraphPose = lom_graph_pose;      // {t[3], q_wxyz[4]}, f64
using GraphParams = lom_graph_params;  // {lambda0, gtol, xtol, pcg_rtol, max_outer, max_pcg}; there are no defaults
using GraphStats = lom_graph_stats;

class PoseGraph : public Handle<lom_graph, lom_graph_destroy, lom_graph_last_error> {
public:
    explicit PoseGraph(size_t node_hint = 0, size_t edge_hint = 0, int device = 0)
    {
        created(lom_graph_create(device, node_hint, edge_hint, &h_));
    }
    void clear() { check(lom_graph_clear(h_)); }
    size_t nodeCount() const { return (size_t)check(lom_graph_node_count(h_)); }
    size_t edgeCount() const { return (size_t)check(lom_graph_edge_count(h_)); }

    static GraphPose fromPose3D(const Pose3D &pose)
    {
        const lom_pose p = pose.c();
        GraphPose out;
        lom_graph_pose_from_f32(&p, &out);
        return out;
    }
    static Pose3D toPose3D(const GraphPose &pose)
    {
        lom_pose p;
        lom_graph_pose_to_f32(&pose, &p);
        return Pose3D::from(p);
    }
    // Omega of an edge (rotation in radians, then translation; row-major 6x6) from the quality report of the align that
    // measured it; withPrior: the align's translation prior, which the report leaves out
    static std::vector<double> informationFromQuality(const QualityReport &report, bool withPrior)
    {
        std::vector<double> out(36);
        const int rc = lom_graph_information_from_quality(&report, withPrior ? 1 : 0, out.data());
        if (rc != LOM_OK) throw Error(rc, "PoseGraph::informationFromQuality: a report with fewer than 7 correspondences");
        return out;
    }

    int64_t addNode(const GraphPose &pose, bool fixed) { return check(lom_graph_add_node(h_, &pose, fixed ? 1 : 0)); }
    int64_t addNode(const Pose3D &pose, bool fixed) { return addNode(fromPose3D(pose), fixed); }
    // the measured pose of node j in node i's frame, its 6x6 information, the Huber width (0: none)
    int64_t addEdge(int64_t i, int64_t j, const GraphPose &measurement, const std::vector<double> &info, double delta)
    {
        if (info.size() != 36) throw Error(LOM_ERR_ARG, "PoseGraph::addEdge: 36 values of information");
        return check(lom_graph_add_edge(h_, i, j, &measurement, info.data(), delta));
    }
    int64_t addEdge(int64_t i, int64_t j, const Pose3D &measurement, const std::vector<double> &info, double delta)
    {
        return addEdge(i, j, fromPose3D(measurement), info, delta);
    }
    int64_t addEdge(int64_t i, int64_t j, const Pose3D &measurement, const QualityReport &report, bool withPrior, double delta)
    {
        return addEdge(i, j, fromPose3D(measurement), informationFromQuality(report, withPrior), delta);
    }
    void setPose(int64_t id, const GraphPose &pose) { check(lom_graph_set_pose(h_, id, &pose)); }
    void setFixed(int64_t id, bool fixed) { check(lom_graph_set_fixed(h_, id, fixed ? 1 : 0)); }
    GraphStats optimize(const GraphParams &params)
    {
        GraphStats st;
        check(lom_graph_optimize(h_, &params, &st));
        return st;
    }
    std::vector<GraphPose> poses() const
    {
        std::vector<GraphPose> out(nodeCount());
        check(lom_graph_get_poses(h_, 0, (int64_t)out.size(), out.data()));
        return out;
    }
    // s = e^T Omega e of every edge at the current poses
    std::vector<double> chi2() const
    {
        std::vector<double> out(edgeCount());
        check(lom_graph_edge_chi2(h_, 0, (int64_t)out.size(), out.data()));
        return out;
    }
};

// ---- scan archive and map assembly (lom_archive_*, lom_map_assemble; not in the reference) -------------------
// Clouds with normals kept in HBM in their own sensor frame; VoxelGrid::assemble puts any of them, at f64 poses, into a
// map in one call: the stage behind PoseGraph::optimize.  Definitions: lidar_odometry_amd.h ("scan archive and map assembly").
using AssembleParams = lom_assemble_params;  // {centre[3], radius}; radius <= 0 keeps everything
using AssembleStats = lom_assemble_stats;

class ScanArchive : public Handle<lom_archive, lom_archive_destroy, lom_archive_last_error> {
public:
    explicit ScanArchive(size_t point_hint = 0, size_t scan_hint = 0, int device = 0)
    {
        created(lom_archive_create(device, point_hint, scan_hint, &h_));
    }
    void clear() { check(lom_archive_clear(h_)); }
    size_t size() const { return (size_t)check(lom_archive_scan_count(h_)); }
    size_t pointCount() const { return (size_t)check(lom_archive_point_count(h_)); }
    size_t scanSize(int64_t id) const { return (size_t)check(lom_archive_scan_size(h_, id)); }
    // a new scan; returns its id
    int64_t add(const PointCloud<PointNormal> &cloud)
    {
        const PointNormal *p = cloud.points.data();
        const bool none = cloud.points.empty();
        return check(lom_archive_add(h_, none ? nullptr : &p->x, none ? nullptr : &p->normal_x, cloud.points.size(),
                                     sizeof(PointNormal)));
    }
    // a new scan without normals (zeros are stored): what an occupancy grid reads
    int64_t addPoints(const PointCloud<PointXYZ> &cloud)
    {
        const bool none = cloud.points.empty();
        return check(lom_archive_add_points(h_, none ? nullptr : &cloud.points.data()->x, cloud.points.size(), sizeof(PointXYZ)));
    }
    PointCloud<PointNormal>::Ptr get(int64_t id) const
    {
        const size_t n = scanSize(id);
        std::vector<float> xyz(n * 3 + 3), nrm(n * 3 + 3);
        check(lom_archive_get(h_, id, xyz.data(), nrm.data(), n));
        auto out = std::make_shared<PointCloud<PointNormal>>();
        out->points.resize(n);
        for (size_t i = 0; i < n; i++) {
            PointNormal &q = out->points[i];
            q.x = xyz[3 * i], q.y = xyz[3 * i + 1], q.z = xyz[3 * i + 2];
            q.normal_x = nrm[3 * i], q.normal_y = nrm[3 * i + 1], q.normal_z = nrm[3 * i + 2];
        }
        return out;
    }
    // the row-major R the assembly uses for a pose (lom_graph_pose_rotation_matrix)
    static std::vector<double> rotationMatrix(const lom_graph_pose &pose)
    {
        std::vector<double> R(9);
        const int rc = lom_graph_pose_rotation_matrix(&pose, R.data());
        if (rc != LOM_OK) throw Error(rc, "ScanArchive::rotationMatrix: a non-finite value or a zero quaternion");
        return R;
    }
};

inline lom_assemble_stats VoxelGrid::assemble(ScanArchive &archive, const std::vector<int64_t> &ids,
                                              const std::vector<lom_graph_pose> &poses, const lom_assemble_params *params)
{
    if (ids.size() != poses.size()) throw Error(LOM_ERR_ARG, "VoxelGrid::assemble: one pose per id");
    lom_assemble_stats st;
    const int rc = lom_map_assemble(h_, archive.handle(), ids.data(), poses.data(), ids.size(), params, &st);
    if (rc != LOM_OK) throw Error(rc, lom_archive_last_error(archive.handle()));
    return st;
}

using VoteParams = lom_vote_params;  // {margin, min_range, max_range, clearance, min_free_scans, free_per_seen}
using VoteStats = lom_vote_stats;

inline lom_vote_stats VoxelGrid::carveScans(ScanArchive &archive, const std::vector<int64_t> &ids,
                                            const std::vector<lom_graph_pose> &poses, const lom_vote_params &params)
{
    if (ids.size() != poses.size()) throw Error(LOM_ERR_ARG, "VoxelGrid::carveScans: one pose per id");
    lom_vote_stats st;
    check(lom_map_carve_scans(h_, archive.handle(), ids.data(), poses.data(), ids.size(), &params, &st));
    return st;
}

inline void VoxelGrid::scanVotes(ScanArchive &archive, const std::vector<int64_t> &ids,
                                 const std::vector<lom_graph_pose> &poses, const lom_vote_params &params,
                                 std::vector<uint32_t> &free_out, std::vector<uint32_t> &seen_out)
{
    if (ids.size() != poses.size()) throw Error(LOM_ERR_ARG, "VoxelGrid::scanVotes: one pose per id");
    const size_t nv = size();
    free_out.assign(nv, 0u);
    seen_out.assign(nv, 0u);
    const int64_t got = lom_map_scan_votes(h_, archive.handle(), ids.data(), poses.data(), ids.size(), &params,
                                           free_out.data(), seen_out.data(), nv);
    if (got < 0) throw Error((int)got, lom_last_error(h_));
    if ((size_t)got != nv) throw Error(LOM_ERR_STATE, "VoxelGrid::scanVotes: voxel count changed");
}

// ---- OccupancyGrid (not in the reference) --------------------------------------------
// A dense 2-D grid of free / seen scan counts on the device: posed scans vote once per cell, and classify() gives the int8
// values of nav_msgs/OccupancyGrid (0 free, 100 occupied, -1 unknown), row-major with y as the row.  Definitions:
// lidar_odometry_amd.h ("occupancy grid").
using OccupancyGeometry = lom_occupancy_geometry;    // {resolution, origin_x, origin_y, width, height}
using OccupancyRayParams = lom_occupancy_ray_params;  // {z_lo, z_hi, margin, min_range, max_range}
using OccupancyRule = lom_occupancy_rule;            // {min_free_scans, free_per_seen, min_seen_scans}
using OccupancyStats = lom_occupancy_stats;
using OccupancySummary = lom_occupancy_summary;

class OccupancyGrid
    : public GridHandle<lom_occupancy, lom_occupancy_geometry, lom_occupancy_create, lom_occupancy_destroy, lom_occupancy_last_error,
                        lom_occupancy_get_geometry, lom_occupancy_clear, lom_occupancy_shift, lom_occupancy_set_option, lom_occupancy_device,
                        lom_occupancy_stream, lom_occupancy_wait_event> {
public:
    explicit OccupancyGrid(const lom_occupancy_geometry &geometry, int device = 0) : GridHandle(geometry, device) {}
    size_t cells() const { return cellCount(); }
    // the scans `ids` of the archive at `poses` vote
    lom_occupancy_stats integrate(ScanArchive &archive, const std::vector<int64_t> &ids, const std::vector<lom_graph_pose> &poses,
                                  const lom_occupancy_ray_params &params)
    {
        if (ids.size() != poses.size()) throw Error(LOM_ERR_ARG, "OccupancyGrid::integrate: one pose per id");
        lom_occupancy_stats st;
        check(lom_occupancy_integrate(h_, archive.handle(), ids.data(), poses.data(), ids.size(), &params, &st));
        return st;
    }
    // one scan that is not in an archive
    lom_occupancy_stats integrateCloud(const PointCloud<PointXYZ> &cloud, const lom_graph_pose &pose,
                                       const lom_occupancy_ray_params &params)
    {
        lom_occupancy_stats st;
        const bool none = cloud.points.empty();
        check(lom_occupancy_integrate_cloud(h_, none ? nullptr : &cloud.points.data()->x, cloud.points.size(), sizeof(PointXYZ),
                                            &pose, &params, &st));
        return st;
    }
    void counts(std::vector<uint32_t> &free_out, std::vector<uint32_t> &seen_out) const
    {
        const size_t n = cells();
        free_out.assign(n, 0u);
        seen_out.assign(n, 0u);
        check(lom_occupancy_counts(h_, free_out.data(), seen_out.data(), n));
    }
    std::vector<int8_t> classify(const lom_occupancy_rule &rule, lom_occupancy_summary *summary_or_null = nullptr)
    {
        std::vector<int8_t> out(cells());
        check(lom_occupancy_classify(h_, &rule, out.data(), out.size(), summary_or_null));
        return out;
    }
};

// ---- ElevationGrid (not in the reference) ---------------------------------------------
// A dense 2-D grid of integer height accumulators on the device: every point of a posed scan that is an occupancy hit
// adds its quantised height to its cell; layers() derives ground height, slope, roughness and step, cost() the int8
// values of a costmap (-1 unknown, 0 .. 99, 100 lethal), row-major with y as the row.  Definitions:
// lidar_odometry_amd.h ("elevation grid").
using ElevationGeometry = lom_elevation_geometry;        // {resolution, origin_x, origin_y, width, height, z_ref}
using ElevationPointParams = lom_elevation_point_params;  // {z_lo, z_hi, min_range, max_range}
using ElevationLayerParams = lom_elevation_layer_params;  // {min_points, window}
using ElevationCostParams = lom_elevation_cost_params;    // {max_slope, max_step, max_rough, max_span}
using ElevationStats = lom_elevation_stats;
using ElevationSummary = lom_elevation_summary;

class ElevationGrid
    : public GridHandle<lom_elevation, lom_elevation_geometry, lom_elevation_create, lom_elevation_destroy, lom_elevation_last_error,
                        lom_elevation_get_geometry, lom_elevation_clear, lom_elevation_shift, lom_elevation_set_option, lom_elevation_device,
                        lom_elevation_stream, lom_elevation_wait_event> {
public:
    struct Cells {  // the accumulators, in quanta of 2^-8 m relative to z_ref
        std::vector<uint32_t> count;
        std::vector<int32_t> zmin, zmax;
        std::vector<int64_t> sum;
    };
    struct Layers {  // NaN where a cell is invalid
        std::vector<float> min, max, mean, slope, rough, step;
    };

    explicit ElevationGrid(const lom_elevation_geometry &geometry, int device = 0) : GridHandle(geometry, device) {}
    size_t size() const { return cellCount(); }
    // the scans `ids` of the archive at `poses`
    lom_elevation_stats integrate(ScanArchive &archive, const std::vector<int64_t> &ids, const std::vector<lom_graph_pose> &poses,
                                  const lom_elevation_point_params &params)
    {
        if (ids.size() != poses.size()) throw Error(LOM_ERR_ARG, "ElevationGrid::integrate: one pose per id");
        lom_elevation_stats st;
        check(lom_elevation_integrate(h_, archive.handle(), ids.data(), poses.data(), ids.size(), &params, &st));
        return st;
    }
    // one scan that is not in an archive
    lom_elevation_stats integrateCloud(const PointCloud<PointXYZ> &cloud, const lom_graph_pose &pose,
                                       const lom_elevation_point_params &params)
    {
        lom_elevation_stats st;
        const bool none = cloud.points.empty();
        check(lom_elevation_integrate_cloud(h_, none ? nullptr : &cloud.points.data()->x, cloud.points.size(), sizeof(PointXYZ),
                                            &pose, &params, &st));
        return st;
    }
    Cells cells() const
    {
        const size_t n = size();
        Cells c;
        c.count.assign(n, 0u), c.zmin.assign(n, 0), c.zmax.assign(n, 0), c.sum.assign(n, 0);
        check(lom_elevation_cells(h_, c.count.data(), c.zmin.data(), c.zmax.data(), c.sum.data(), n));
        return c;
    }
    Layers layers(const lom_elevation_layer_params &lp)
    {
        const size_t n = size();
        Layers l;
        for (std::vector<float> *v : {&l.min, &l.max, &l.mean, &l.slope, &l.rough, &l.step}) v->assign(n, 0.f);
        check(lom_elevation_layers(h_, &lp, l.min.data(), l.max.data(), l.mean.data(), l.slope.data(), l.rough.data(),
                                   l.step.data(), n));
        return l;
    }
    std::vector<int8_t> cost(const lom_elevation_layer_params &lp, const lom_elevation_cost_params &cp,
                             lom_elevation_summary *summary_or_null = nullptr)
    {
        std::vector<int8_t> out(size());
        check(lom_elevation_cost(h_, &lp, &cp, out.data(), out.size(), summary_or_null));
        return out;
    }
};

// ---- ClearanceGrid (not in the reference) ---------------------------------------------
// Obstacle distance and inflated cost on the device: update() merges an occupancy and an elevation plane (int8,
// row-major with y as the row, either may be NULL), computes the exact truncated squared distance to the nearest obstacle
// (u16, cells) and the int8 cost of a costmap (-1 unknown, 0 .. 98, 99 inscribed, 100 lethal).  Definitions:
// lidar_odometry_amd.h ("clearance grid").
using ClearanceParams = lom_clearance_params;    // {inflation_radius, inscribed_radius, decay, flags}
using ClearanceWindow = lom_clearance_window;    // {x0, y0, width, height}
using ClearanceSummary = lom_clearance_summary;

inline ClearanceParams clearanceParams(float inflation_radius, float inscribed_radius, float decay, uint32_t flags = 0)
{
    return ClearanceParams{inflation_radius, inscribed_radius, decay, flags};
}

class ClearanceGrid
    : public GridHandle<lom_clearance, lom_occupancy_geometry, lom_clearance_create, lom_clearance_destroy, lom_clearance_last_error,
                        lom_clearance_get_geometry, lom_clearance_clear, lom_clearance_shift, lom_clearance_set_option, lom_clearance_device,
                        lom_clearance_stream, lom_clearance_wait_event> {
public:
    struct Query {  // NaN and -1 for a point outside the grid
        std::vector<float> distance;
        std::vector<int8_t> cost;
    };

    explicit ClearanceGrid(const lom_occupancy_geometry &geometry, int device = 0) : GridHandle(geometry, device) {}
    size_t size() const { return cellCount(); }
    // host planes of size() cells each; either may be NULL
    lom_clearance_summary update(const int8_t *occ_or_null, const int8_t *elev_or_null, const lom_clearance_params &params,
                                 const lom_clearance_window *window_or_null = nullptr)
    {
        lom_clearance_summary s;
        check(lom_clearance_update(h_, occ_or_null, elev_or_null, &params, window_or_null, &s));
        return s;
    }
    // the planes of the two grids, left in HBM; either may be NULL
    lom_clearance_summary updateFromGrids(OccupancyGrid *occupancy_or_null, const lom_occupancy_rule &rule,
                                          ElevationGrid *elevation_or_null, const lom_elevation_layer_params &lp,
                                          const lom_elevation_cost_params &cp, const lom_clearance_params &params,
                                          const lom_clearance_window *window_or_null = nullptr)
    {
        lom_clearance_summary s;
        check(lom_clearance_update_from_grids(h_, occupancy_or_null ? occupancy_or_null->handle() : nullptr, &rule,
                                              elevation_or_null ? elevation_or_null->handle() : nullptr, &lp, &cp, &params,
                                              window_or_null, &s));
        return s;
    }
    std::vector<int8_t> cost(lom_clearance_summary *summary_or_null = nullptr)
    {
        std::vector<int8_t> out(size());
        check(lom_clearance_cost(h_, out.data(), out.size(), summary_or_null));
        return out;
    }
    std::vector<uint16_t> distanceSq()
    {
        std::vector<uint16_t> out(size());
        check(lom_clearance_distance_sq(h_, out.data(), out.size()));
        return out;
    }
    std::vector<float> distance()
    {
        std::vector<float> out(size());
        check(lom_clearance_distance(h_, out.data(), out.size()));
        return out;
    }
    // xy: n pairs in the grid's frame
    Query query(const float *xy, size_t n)
    {
        Query q;
        q.distance.assign(n, 0.f), q.cost.assign(n, 0);
        check(lom_clearance_query(h_, xy, n, q.distance.data(), q.cost.data()));
        return q;
    }
};

// ---- NavField (not in the reference) ---------------------------------------------------
// The navigation field on the device: solve() takes an int8 cost plane (row-major with y as the row, the value range
// ClearanceGrid::cost() writes) and goals, and leaves per cell the least total cost to reach a goal (u32,
// LOM_NAV_UNREACHED where there is no route); paths() walks down it, query() reads it at points in metres.  Definitions:
// lidar_odometry_amd.h ("navigation field").
using NavFieldParams = lom_navfield_params;  // {neutral, factor, unknown_cost, max_passable, flags}
using NavFieldSummary = lom_navfield_summary;

inline NavFieldParams navfieldParams(uint32_t neutral, uint32_t factor, uint32_t unknown_cost, int8_t max_passable, uint32_t flags = 0)
{
    return NavFieldParams{neutral, factor, unknown_cost, max_passable, flags};
}

using NavFieldWaypointParams = lom_navfield_waypoint_params;  // {max_cell_cost, lookahead, route_cap, flags}

inline NavFieldWaypointParams navfieldWaypointParams(uint32_t max_cell_cost, uint32_t lookahead, uint32_t route_cap, uint32_t flags = 0)
{
    return NavFieldWaypointParams{max_cell_cost, lookahead, route_cap, flags};
}

class NavFieldSet;  // below

class NavField
    : public GridHandle<lom_navfield, lom_occupancy_geometry, lom_navfield_create, lom_navfield_destroy, lom_navfield_last_error,
                        lom_navfield_get_geometry, lom_navfield_clear, lom_navfield_shift, lom_navfield_set_option, lom_navfield_device, lom_navfield_stream,
                        lom_navfield_wait_event> {
public:
    struct Paths {  // cells: [K, cap] (ix, iy) pairs; lengths: the full length per start, 0 where none was walked
        std::vector<uint16_t> cells;
        std::vector<uint32_t> lengths;
    };
    struct Waypoints {  // cells: [K, wp_cap] (ix, iy) pairs; counts: the full number per start; lengths: the walk's full length
        std::vector<uint16_t> cells;
        std::vector<uint32_t> counts, lengths;
    };

    explicit NavField(const lom_occupancy_geometry &geometry, int device = 0) : GridHandle(geometry, device) {}
    size_t size() const { return cellCount(); }
    // a host plane of size() cells; goals: n pairs of int32 cells
    lom_navfield_summary solve(const int8_t *plane, const lom_navfield_params &params, const int32_t *goal_cells, size_t n)
    {
        lom_navfield_summary s;
        check(lom_navfield_solve(h_, plane, &params, LOM_NAV_CELLS, goal_cells, n, &s));
        return s;
    }
    // ... goals: n pairs of f32 metres
    lom_navfield_summary solveMetres(const int8_t *plane, const lom_navfield_params &params, const float *goal_xy, size_t n)
    {
        lom_navfield_summary s;
        check(lom_navfield_solve(h_, plane, &params, LOM_NAV_METRES, goal_xy, n, &s));
        return s;
    }
    // the plane a ClearanceGrid of this geometry left in HBM
    lom_navfield_summary solveFromClearance(ClearanceGrid &clearance, const lom_navfield_params &params, int goal_kind,
                                            const void *goals, size_t n)
    {
        lom_navfield_summary s;
        check(lom_navfield_solve_from_clearance(h_, clearance.handle(), &params, goal_kind, goals, n, &s));
        return s;
    }
    // the re-solve: the window's cells (NULL: the whole grid) of a host plane of size() cells, for the goals the last solve used
    lom_navfield_summary resolve(const int8_t *plane, const lom_clearance_window *window = nullptr)
    {
        lom_navfield_summary s;
        check(lom_navfield_resolve(h_, plane, window, &s));
        return s;
    }
    // ... of the plane a ClearanceGrid of this geometry left in HBM
    lom_navfield_summary resolveFromClearance(ClearanceGrid &clearance, const lom_clearance_window *window = nullptr)
    {
        lom_navfield_summary s;
        check(lom_navfield_resolve_from_clearance(h_, clearance.handle(), window, &s));
        return s;
    }
    lom_navfield_resolve_counters resolveStats() const
    {
        lom_navfield_resolve_counters s;
        check(lom_navfield_resolve_stats(h_, &s));
        return s;
    }
    // the shift with a re-solve: the geometry moves by (dx, dy) cells, the field moves with the world, the entered cells and
    // the window's cells (NULL: the whole grid) take the bytes of a host plane of size() cells in the new geometry
    lom_navfield_summary shiftResolve(int32_t dx, int32_t dy, const int8_t *plane, const lom_clearance_window *window = nullptr)
    {
        lom_navfield_summary s;
        check(lom_navfield_shift_resolve(h_, dx, dy, plane, window, &s));
        return s;
    }
    // ... of the plane a ClearanceGrid left in HBM after it was shifted by the same (dx, dy) and updated
    lom_navfield_summary shiftResolveFromClearance(int32_t dx, int32_t dy, ClearanceGrid &clearance, const lom_clearance_window *window = nullptr)
    {
        lom_navfield_summary s;
        check(lom_navfield_shift_resolve_from_clearance(h_, dx, dy, clearance.handle(), window, &s));
        return s;
    }
    lom_navfield_shift_counters shiftStats() const
    {
        lom_navfield_shift_counters s;
        check(lom_navfield_shift_stats(h_, &s));
        return s;
    }
    std::vector<uint32_t> potential()
    {
        std::vector<uint32_t> out(size());
        check(lom_navfield_potential(h_, out.data(), out.size()));
        return out;
    }
    // starts: n pairs of start_kind (LOM_NAV_CELLS: int32, LOM_NAV_METRES: f32)
    Paths paths(int start_kind, const void *starts, size_t n, size_t cap)
    {
        Paths p;
        p.cells.assign(n * cap * 2, 0), p.lengths.assign(n, 0);
        check(lom_navfield_paths(h_, start_kind, starts, n, p.cells.data(), cap, p.lengths.data()));
        return p;
    }
    // xy: n pairs in the grid's frame
    std::vector<uint32_t> query(const float *xy, size_t n)
    {
        std::vector<uint32_t> out(n);
        check(lom_navfield_query(h_, xy, n, out.data()));
        return out;
    }
    // pairs: n quadruples (x0, y0, x1, y1) of cells; a byte per pair, 1 where the second cell is in line of sight of the first
    std::vector<uint8_t> visible(const int32_t *pairs, size_t n, uint32_t max_cell_cost = 0)
    {
        std::vector<uint8_t> out(n);
        check(lom_navfield_visible(h_, pairs, n, max_cell_cost, out.data()));
        return out;
    }
    // the walks of paths(), cut to any-angle waypoints by line-of-sight shortcuts; starts as for paths()
    Waypoints waypoints(int start_kind, const void *starts, size_t n, const lom_navfield_waypoint_params &params, size_t wp_cap)
    {
        Waypoints w;
        w.cells.assign(n * wp_cap * 2, 0), w.counts.assign(n, 0), w.lengths.assign(n, 0);
        check(lom_navfield_waypoints(h_, start_kind, starts, n, &params, w.cells.data(), wp_cap, w.counts.data(), w.lengths.data()));
        return w;
    }
    // the centres of n cells (ix, iy) in the grid's frame, (x, y) pairs: origin + (i + 0.5) * resolution
    std::vector<double> waypointsMetres(const uint16_t *cells, size_t n) const
    {
        const lom_occupancy_geometry g = geometry();
        std::vector<double> xy(2 * n);
        for (size_t i = 0; i < n; i++) {
            xy[2 * i] = (double)g.origin_x + ((double)cells[2 * i] + 0.5) * (double)g.resolution;
            xy[2 * i + 1] = (double)g.origin_y + ((double)cells[2 * i + 1] + 0.5) * (double)g.resolution;
        }
        return xy;
    }
    // the length in metres of the polyline through n cells
    double polylineLength(const uint16_t *cells, size_t n) const
    {
        const double r = (double)geometry().resolution;
        double total = 0.0;
        for (size_t i = 1; i < n; i++) {
            const double dx = (double)cells[2 * i] - (double)cells[2 * i - 2], dy = (double)cells[2 * i + 1] - (double)cells[2 * i - 1];
            total += std::sqrt(dx * dx + dy * dy);
        }
        return total * r;
    }
    lom_navfield_solve_stats stats() const
    {
        lom_navfield_solve_stats s;
        check(lom_navfield_stats(h_, &s));
        return s;
    }
    // this field becomes what solve() of the plane, parameters and goals of field i of a set of this geometry would have left
    inline lom_navfield_summary adopt(NavFieldSet &set, size_t i);
};

inline std::vector<uint32_t> navfieldCellCosts(const lom_navfield_params &params)
{
    std::vector<uint32_t> out(256);
    const int rc = lom_navfield_cell_costs(&params, out.data());
    if (rc != LOM_OK) throw Error(rc, "navigation field cell costs: bad parameters");
    return out;
}

// ---- NavFieldSet (not in the reference) ------------------------------------------------
// N navigation fields over one cost plane, solved side by side in one call: field i and its summary are byte for byte what
// NavField::solve() gives for the goals [goal_offsets[i], goal_offsets[i + 1]) of one goal array.  gather() reads every
// field at points (with the goals as the points: the travel-cost matrix, which need not be symmetric -- a step pays for
// the cell it leaves), nearest() partitions the grid by nearest goal, paths() walks down a named field, NavField::adopt()
// makes one field a NavField.  Definitions: lidar_odometry_amd.h ("navigation field set").
class NavFieldSet
    : public GridHandle<lom_navset, lom_occupancy_geometry, lom_navset_create, lom_navset_destroy, lom_navset_last_error, lom_navset_get_geometry,
                        lom_navset_clear, lom_navset_shift, lom_navset_set_option, lom_navset_device, lom_navset_stream, lom_navset_wait_event> {
public:
    struct Nearest {  // owner: LOM_NAVSET_NO_OWNER where no field reaches the cell; cells_owned: per field
        std::vector<uint16_t> owner;
        std::vector<uint32_t> potential;
        std::vector<uint64_t> cells_owned;
    };

    NavFieldSet(const lom_occupancy_geometry &geometry, size_t max_fields, int device = 0) : GridHandle(geometry, device, max_fields) {}
    size_t size() const { return cellCount(); }
    size_t fieldCount() const { return lom_navset_field_count(h_); }
    // a host plane of size() cells; goals: goal_offsets[n_fields] pairs of goal_kind; goal_offsets: n_fields + 1 values
    std::vector<lom_navfield_summary> solve(const int8_t *plane, const lom_navfield_params &params, int goal_kind, const void *goals,
                                            const uint32_t *goal_offsets, size_t n_fields)
    {
        std::vector<lom_navfield_summary> s(n_fields);
        check(lom_navset_solve(h_, plane, &params, goal_kind, goals, goal_offsets, n_fields, s.data()));
        return s;
    }
    // ... a plane in HBM that is complete when hip_event is (NULL: now)
    std::vector<lom_navfield_summary> solveDevice(const int8_t *d_plane, void *hip_event, const lom_navfield_params &params, int goal_kind,
                                                  const void *goals, const uint32_t *goal_offsets, size_t n_fields)
    {
        std::vector<lom_navfield_summary> s(n_fields);
        check(lom_navset_solve_device(h_, d_plane, hip_event, &params, goal_kind, goals, goal_offsets, n_fields, s.data()));
        return s;
    }
    // ... the plane a ClearanceGrid of this geometry left in HBM
    std::vector<lom_navfield_summary> solveFromClearance(ClearanceGrid &clearance, const lom_navfield_params &params, int goal_kind,
                                                         const void *goals, const uint32_t *goal_offsets, size_t n_fields)
    {
        std::vector<lom_navfield_summary> s(n_fields);
        check(lom_navset_solve_from_clearance(h_, clearance.handle(), &params, goal_kind, goals, goal_offsets, n_fields, s.data()));
        return s;
    }
    std::vector<uint32_t> potential(size_t i)
    {
        std::vector<uint32_t> out(size());
        check(lom_navset_potential(h_, i, out.data(), out.size()));
        return out;
    }
    // [fieldCount(), n]: P of every field at n points of point_kind
    std::vector<uint32_t> gather(int point_kind, const void *points, size_t n)
    {
        std::vector<uint32_t> out(fieldCount() * n);
        check(lom_navset_gather(h_, point_kind, points, n, out.data()));
        return out;
    }
    Nearest nearest()
    {
        Nearest r;
        r.owner.resize(size()), r.potential.resize(size()), r.cells_owned.assign(fieldCount(), 0);
        check(lom_navset_nearest(h_, r.owner.data(), r.potential.data(), r.cells_owned.data()));
        return r;
    }
    // NavField::paths()' walk, start k down field field_of_start[k]
    NavField::Paths paths(const int32_t *field_of_start, int start_kind, const void *starts, size_t n, size_t cap)
    {
        NavField::Paths p;
        p.cells.assign(n * cap * 2, 0), p.lengths.assign(n, 0);
        check(lom_navset_paths(h_, field_of_start, start_kind, starts, n, p.cells.data(), cap, p.lengths.data()));
        return p;
    }
    lom_navset_solve_stats stats() const
    {
        lom_navset_solve_stats s;
        check(lom_navset_stats(h_, &s));
        return s;
    }
};

inline lom_navfield_summary NavField::adopt(NavFieldSet &set, size_t i)
{
    lom_navfield_summary s;
    check(lom_navfield_adopt(h_, set.handle(), i, &s));
    return s;
}

// ---- PoseField (not in the reference) --------------------------------------------------
// The cost-to-go over cell and heading under a robot's footprint: solve() takes an int8 cost plane, a footprint (F pairs
// of int32 fx, fy in 1/256 cell, robot frame) and goals (n triples of int32 ix, iy, h; h = -1: every passable heading of
// the cell); heading h of 0 .. 7 points along E, NE, N, NW, W, SW, S, SE.  floor() is the least over the headings, in
// NavField::potential()'s form.  Definitions: lidar_odometry_amd.h ("pose field").
using PoseFieldParams = lom_posefield_params;  // {nav, turn_cost, spin_cost, reverse_cost, flags}
using PoseFieldSummary = lom_posefield_summary;

inline PoseFieldParams posefieldParams(const lom_navfield_params &nav, uint32_t turn_cost, uint32_t spin_cost, uint32_t reverse_cost,
                                       uint32_t flags = 0)
{
    return PoseFieldParams{nav, turn_cost, spin_cost, reverse_cost, flags};
}
// the heading 0 .. 7 of an angle in 1/65536 turn; needs no device
inline uint32_t posefieldHeadingOfAngle(uint32_t angle) { return lom_posefield_heading_of_angle(angle); }
// the eight stencils of a footprint, (dx, dy) pairs per heading, sorted by (dy, dx); needs no device
inline std::vector<std::vector<int32_t>> posefieldStencils(const int32_t *footprint, size_t n_samples)
{
    uint32_t counts[LOM_POSE_HEADINGS] = {};
    if (lom_posefield_stencils(footprint, n_samples, nullptr, 0, counts) != LOM_OK) throw Error(LOM_ERR_ARG, "lom_posefield_stencils");
    size_t total = 0;
    for (uint32_t c : counts) total += c;
    std::vector<int32_t> cells(2 * total);
    (void)lom_posefield_stencils(footprint, n_samples, cells.data(), total, counts);
    std::vector<std::vector<int32_t>> out(LOM_POSE_HEADINGS);
    size_t at = 0;
    for (size_t h = 0; h < LOM_POSE_HEADINGS; at += 2 * (size_t)counts[h], h++) out[h].assign(cells.begin() + at, cells.begin() + at + 2 * (size_t)counts[h]);
    return out;
}

class PoseField
    : public GridHandle<lom_posefield, lom_occupancy_geometry, lom_posefield_create, lom_posefield_destroy, lom_posefield_last_error,
                        lom_posefield_get_geometry, lom_posefield_clear, lom_posefield_shift, lom_posefield_set_option, lom_posefield_device,
                        lom_posefield_stream, lom_posefield_wait_event> {
public:
    struct Paths {  // states: [K, cap] (ix, iy, h) triples; lengths: the full length per start, 0 where none was walked
        std::vector<uint16_t> states;
        std::vector<uint32_t> lengths;
    };
    struct Floor {  // heading: the least heading that attains the floor, 8 where none is reached
        std::vector<uint32_t> floor;
        std::vector<uint8_t> heading;
    };

    explicit PoseField(const lom_occupancy_geometry &geometry, int device = 0) : GridHandle(geometry, device) {}
    size_t size() const { return cellCount(); }
    // a host plane of size() cells
    PoseFieldSummary solve(const int8_t *plane, const PoseFieldParams &params, const int32_t *footprint, size_t n_samples,
                           const int32_t *goals, size_t n_goals)
    {
        PoseFieldSummary s;
        check(lom_posefield_solve(h_, plane, &params, footprint, n_samples, goals, n_goals, &s));
        return s;
    }
    // ... a plane in HBM that is complete when hip_event is (NULL: now)
    PoseFieldSummary solveDevice(const int8_t *d_plane, void *hip_event, const PoseFieldParams &params, const int32_t *footprint,
                                 size_t n_samples, const int32_t *goals, size_t n_goals)
    {
        PoseFieldSummary s;
        check(lom_posefield_solve_device(h_, d_plane, hip_event, &params, footprint, n_samples, goals, n_goals, &s));
        return s;
    }
    // ... the plane a ClearanceGrid of this geometry left in HBM
    PoseFieldSummary solveFromClearance(ClearanceGrid &clearance, const PoseFieldParams &params, const int32_t *footprint, size_t n_samples,
                                        const int32_t *goals, size_t n_goals)
    {
        PoseFieldSummary s;
        check(lom_posefield_solve_from_clearance(h_, clearance.handle(), &params, footprint, n_samples, goals, n_goals, &s));
        return s;
    }
    // Re-solve: the field of the kept plane with the cells of `window` (NULL: the whole grid) taken from `plane`, for the
    // footprint, parameters and goal states of the last solve
    PoseFieldSummary resolve(const int8_t *plane, const lom_clearance_window *window = nullptr)
    {
        PoseFieldSummary s;
        check(lom_posefield_resolve(h_, plane, window, &s));
        return s;
    }
    PoseFieldSummary resolveDevice(const int8_t *d_plane, void *hip_event, const lom_clearance_window *window = nullptr)
    {
        PoseFieldSummary s;
        check(lom_posefield_resolve_device(h_, d_plane, hip_event, window, &s));
        return s;
    }
    PoseFieldSummary resolveFromClearance(ClearanceGrid &clearance, const lom_clearance_window *window = nullptr)
    {
        PoseFieldSummary s;
        check(lom_posefield_resolve_from_clearance(h_, clearance.handle(), window, &s));
        return s;
    }
    lom_posefield_resolve_counters resolveStats() const
    {
        lom_posefield_resolve_counters s;
        check(lom_posefield_resolve_stats(h_, &s));
        return s;
    }
    std::vector<uint32_t> potential()  // [8][height][width]
    {
        std::vector<uint32_t> out(size() * LOM_POSE_HEADINGS);
        check(lom_posefield_potential(h_, out.data(), out.size()));
        return out;
    }
    std::vector<uint32_t> layers()  // [8][height][width]
    {
        std::vector<uint32_t> out(size() * LOM_POSE_HEADINGS);
        check(lom_posefield_layers(h_, out.data(), out.size()));
        return out;
    }
    Floor floor()
    {
        Floor f;
        f.floor.resize(size()), f.heading.resize(size());
        check(lom_posefield_floor(h_, f.floor.data(), f.heading.data(), f.floor.size()));
        return f;
    }
    // the floor in HBM, a potential plane for RolloutGrid's device form; valid until the next solve(), clear() or shift()
    const uint32_t *floorDevice()
    {
        const uint32_t *d = nullptr;
        check(lom_posefield_floor_device(h_, &d, nullptr));
        return d;
    }
    // starts: n triples (ix, iy, h), h = -1 for the floor's heading
    Paths paths(const int32_t *starts, size_t n, size_t cap)
    {
        Paths p;
        p.states.assign(n * cap * 3, 0), p.lengths.assign(n, 0);
        check(lom_posefield_paths(h_, starts, n, p.states.data(), cap, p.lengths.data()));
        return p;
    }
    // xy: n pairs in the grid's frame; headings: n values, -1 for the floor
    std::vector<uint32_t> query(const float *xy, const int32_t *headings, size_t n)
    {
        std::vector<uint32_t> out(n);
        check(lom_posefield_query(h_, xy, headings, n, out.data()));
        return out;
    }
    lom_posefield_solve_stats stats() const
    {
        lom_posefield_solve_stats s;
        check(lom_posefield_stats(h_, &s));
        return s;
    }
};

// ---- RegionGrid (not in the reference) -------------------------------------------------
// Connected regions of a grid plane on the device: extract() takes an int8 plane (row-major with y as the row, what
// OccupancyGrid::classify() writes), optionally a cost plane and a NavField potential, labels the regions of the
// frontier cells (or of a byte range) and leaves a record per region and a ranked list; goals() gives the list's centre
// or entry cells in the form NavField::solve() takes.  Definitions: lidar_odometry_amd.h ("frontier regions").
using RegionsParams = lom_regions_params;  // {kind, lo, hi, max_cost, min_cells, rank, flags}
using RegionsSummary = lom_regions_summary;
using RegionsRecord = lom_regions_record;

inline RegionsParams regionsParams(int32_t kind, int8_t lo, int8_t hi, int8_t max_cost, uint32_t min_cells, int32_t rank, uint32_t flags = 0)
{
    return RegionsParams{kind, lo, hi, max_cost, min_cells, rank, flags};
}

class RegionGrid
    : public GridHandle<lom_regions, lom_occupancy_geometry, lom_regions_create, lom_regions_destroy, lom_regions_last_error,
                        lom_regions_get_geometry, lom_regions_clear, lom_regions_shift, lom_regions_set_option, lom_regions_device, lom_regions_stream,
                        lom_regions_wait_event> {
public:
    explicit RegionGrid(const lom_occupancy_geometry &geometry, int device = 0) : GridHandle(geometry, device) {}
    size_t size() const { return cellCount(); }
    // host planes of size() cells; cost and potential may be NULL
    lom_regions_summary extract(const int8_t *plane, const lom_regions_params &params, const int8_t *cost = nullptr,
                                const uint32_t *potential = nullptr)
    {
        lom_regions_summary s;
        check(lom_regions_extract(h_, plane, cost, potential, &params, &s));
        return s;
    }
    // the planes an OccupancyGrid, a ClearanceGrid (or NULL) and a NavField (or NULL) of this geometry left in HBM
    lom_regions_summary extractFromGrids(OccupancyGrid &occupancy, const lom_occupancy_rule &rule, ClearanceGrid *clearance,
                                         NavField *navfield, const lom_regions_params &params)
    {
        lom_regions_summary s;
        check(lom_regions_extract_from_grids(h_, occupancy.handle(), &rule, clearance ? clearance->handle() : nullptr,
                                             navfield ? navfield->handle() : nullptr, &params, &s));
        return s;
    }
    std::vector<uint32_t> labels()
    {
        std::vector<uint32_t> out(size());
        check(lom_regions_labels(h_, out.data(), out.size()));
        return out;
    }
    // the list of the last extract, in rank order
    std::vector<lom_regions_record> list()
    {
        size_t n = 0;
        check(lom_regions_list(h_, nullptr, 0, &n));
        std::vector<lom_regions_record> out(n);
        check(lom_regions_list(h_, out.data(), out.size(), nullptr));
        return out;
    }
    // (ix, iy) pairs of the list's centre cells (LOM_REGIONS_GOAL_CENTRE) or entry cells (LOM_REGIONS_GOAL_ENTRY)
    std::vector<int32_t> goals(int which = LOM_REGIONS_GOAL_CENTRE)
    {
        size_t n = 0;
        check(lom_regions_goals(h_, which, nullptr, 0, &n));
        std::vector<int32_t> out(2 * n);
        check(lom_regions_goals(h_, which, out.data(), n, nullptr));
        return out;
    }
    // xy: n pairs in the grid's frame
    std::vector<uint32_t> query(const float *xy, size_t n)
    {
        std::vector<uint32_t> out(n);
        check(lom_regions_query(h_, xy, n, out.data()));
        return out;
    }
    lom_regions_extract_stats stats() const
    {
        lom_regions_extract_stats s;
        check(lom_regions_stats(h_, &s));
        return s;
    }
};

// ---- VisibilityGrid (not in the reference) ----------------------------------------------
// Rays cast over a grid plane from many viewpoints at once: cast() takes an int8 plane (row-major with y as the row, what
// OccupancyGrid::classify() or ClearanceGrid::cost() writes) and int32 (ix, iy) viewpoints, what RegionGrid::goals()
// returns, and leaves a record per viewpoint; beams() gives the simulated scans, windows() the unknown cells each
// viewpoint sees, select() the greedy next-best views.  Definitions: lidar_odometry_amd.h ("visibility grid").
using VisibilityParams = lom_visibility_params;  // {beams, range_cells, block_min, unknown_depth, flags}
using VisibilitySummary = lom_visibility_summary;
using VisibilityRecord = lom_visibility_record;
using VisibilitySelectParams = lom_visibility_select_params;  // {n, gain_weight, cost_shift, min_gain}
using VisibilityPick = lom_visibility_pick;

inline VisibilityParams visibilityParams(uint32_t beams, uint32_t range_cells, int32_t block_min = 100, uint32_t unknown_depth = 0, uint32_t flags = 0)
{
    return VisibilityParams{beams, range_cells, block_min, unknown_depth, flags};
}

inline std::vector<int32_t> visibilityTable(uint32_t beams)
{
    std::vector<int32_t> out(2 * (size_t)(beams <= 8192 ? beams : 0));
    const int rc = lom_visibility_table(beams, out.data());
    if (rc != LOM_OK) throw Error(rc, "visibility table: 4 <= beams <= 8192");
    return out;
}

class VisibilityGrid
    : public GridHandle<lom_visibility, lom_occupancy_geometry, lom_visibility_create, lom_visibility_destroy, lom_visibility_last_error,
                        lom_visibility_get_geometry, lom_visibility_clear, lom_visibility_shift, lom_visibility_set_option, lom_visibility_device,
                        lom_visibility_stream, lom_visibility_wait_event> {
public:
    explicit VisibilityGrid(const lom_occupancy_geometry &geometry, int device = 0) : GridHandle(geometry, device) {}
    size_t size() const { return cellCount(); }
    // a host plane of size() cells; viewpoints: k (ix, iy) pairs
    lom_visibility_summary cast(const int8_t *plane, const int32_t *viewpoints, size_t k, const lom_visibility_params &params)
    {
        lom_visibility_summary s;
        check(lom_visibility_cast(h_, plane, viewpoints, k, &params, &s));
        beams_ = params.beams;
        return s;
    }
    // a plane in HBM, complete when hip_event is (NULL: now)
    lom_visibility_summary castDevice(const int8_t *d_plane, void *hip_event, const int32_t *viewpoints, size_t k,
                                      const lom_visibility_params &params)
    {
        lom_visibility_summary s;
        check(lom_visibility_cast_device(h_, d_plane, hip_event, viewpoints, k, &params, &s));
        beams_ = params.beams;
        return s;
    }
    // the plane an OccupancyGrid of this geometry classifies by `rule`, in HBM
    lom_visibility_summary castFromOccupancy(OccupancyGrid &occupancy, const lom_occupancy_rule &rule, const int32_t *viewpoints, size_t k,
                                             const lom_visibility_params &params)
    {
        lom_visibility_summary s;
        check(lom_visibility_cast_from_occupancy(h_, occupancy.handle(), &rule, viewpoints, k, &params, &s));
        beams_ = params.beams;
        return s;
    }
    std::vector<lom_visibility_record> records()
    {
        size_t n = 0;
        check(lom_visibility_records(h_, nullptr, 0, &n));
        std::vector<lom_visibility_record> out(n);
        check(lom_visibility_records(h_, out.data(), out.size(), nullptr));
        return out;
    }
    // K * B words under LOM_VIS_KEEP_BEAMS: d2 in the low 24 bits, the end reason in the high 8
    std::vector<uint32_t> beams()
    {
        size_t n = 0;
        check(lom_visibility_records(h_, nullptr, 0, &n));
        std::vector<uint32_t> out(n * beams_);
        check(lom_visibility_beams(h_, out.data(), out.size()));
        return out;
    }
    // the K windows under LOM_VIS_KEEP_WINDOWS, read back; *words_per_window: the words of each
    std::vector<uint32_t> windows(size_t *words_per_window = nullptr)
    {
        size_t n = 0, words = 0;
        check(lom_visibility_records(h_, nullptr, 0, &n));
        check(lom_visibility_windows(h_, nullptr, 0, &words));
        std::vector<uint32_t> out(n * words);
        check(lom_visibility_windows(h_, out.data(), out.size(), nullptr));
        if (words_per_window) *words_per_window = words;
        return out;
    }
    const uint32_t *windowsDevice(size_t *words_per_window = nullptr)
    {
        const uint32_t *d = nullptr;
        check(lom_visibility_windows_device(h_, &d, words_per_window));
        return d;
    }
    // cost: K u32 or NULL
    std::vector<lom_visibility_pick> select(const lom_visibility_select_params &s, const uint32_t *cost = nullptr)
    {
        std::vector<lom_visibility_pick> out(s.n ? s.n : 1);
        size_t n = 0;
        check(lom_visibility_select(h_, &s, cost, out.data(), &n));
        out.resize(n);
        return out;
    }
    std::vector<lom_visibility_pick> selectFromNavfield(NavField &navfield, const lom_visibility_select_params &s)
    {
        std::vector<lom_visibility_pick> out(s.n ? s.n : 1);
        size_t n = 0;
        check(lom_visibility_select_from_navfield(h_, navfield.handle(), &s, out.data(), &n));
        out.resize(n);
        return out;
    }
    lom_visibility_call_stats stats() const
    {
        lom_visibility_call_stats s;
        check(lom_visibility_stats(h_, &s));
        return s;
    }

private:
    uint32_t beams_ = 0;
};

// ---- RolloutGrid (not in the reference) --------------------------------------------------
// Candidate command sequences rolled out from many start states at once: evaluate() tests the footprint at every pose
// against a cost plane and picks, per state, the candidate with the best score; records() gives the record per state and
// candidate.  Definitions: lidar_odometry_amd.h ("trajectory rollouts").
using RolloutParams = lom_rollout_params;  // {segments, steps_per_segment, lethal_min, unknown_cost, min_steps, progress_weight, cost_weight, truncation_weight, flags}
using RolloutState = lom_rollout_state;    // {x, y, a}
using RolloutRecord = lom_rollout_record;
using RolloutPick = lom_rollout_pick;
using RolloutSummary = lom_rollout_summary;

inline RolloutParams rolloutParams(uint32_t segments, uint32_t steps_per_segment, int32_t lethal_min = 100, int32_t unknown_cost = -1,
                                   uint32_t min_steps = 0, uint32_t progress_weight = 1, uint32_t cost_weight = 1,
                                   uint32_t truncation_weight = 0, uint32_t flags = 0)
{
    return RolloutParams{segments, steps_per_segment, lethal_min, unknown_cost, min_steps, progress_weight, cost_weight, truncation_weight, flags};
}

// (fx, fy) pairs in 1/256 cell
inline std::vector<int32_t> rolloutFootprintRectangle(int32_t front, int32_t back, int32_t half_width, int32_t spacing, bool perimeter_only = false)
{
    size_t n = 0;
    int rc = lom_rollout_footprint_rectangle(front, back, half_width, spacing, perimeter_only, nullptr, 0, &n);
    std::vector<int32_t> out(2 * n);
    if (rc == LOM_OK) rc = lom_rollout_footprint_rectangle(front, back, half_width, spacing, perimeter_only, out.data(), n, &n);
    if (rc != LOM_OK) throw Error(rc, "rollout footprint: 0 <= front, back, half_width <= 16384, spacing >= 1, at most 1024 samples");
    return out;
}

inline RolloutState rolloutStateFromPose(const lom_occupancy_geometry &geometry, float x_m, float y_m, float yaw)
{
    RolloutState s;
    const int rc = lom_rollout_state_from_pose(&geometry, x_m, y_m, yaw, &s);
    if (rc != LOM_OK) throw Error(rc, "rollout state: a valid geometry, a finite pose, -2^29 <= x, y < 2^29 in Q15 cells");
    return s;
}

// the S + 1 poses of one candidate; commands: params.segments (v, w) pairs
inline std::vector<RolloutState> rolloutPoses(const RolloutParams &params, const RolloutState &state, const int16_t *commands)
{
    const uint64_t steps = (uint64_t)params.segments * params.steps_per_segment;
    std::vector<RolloutState> out(steps <= 1024 ? (size_t)steps + 1 : 1);
    const int rc = lom_rollout_poses(&params, &state, commands, out.data());
    if (rc != LOM_OK) throw Error(rc, "rollout poses: valid parameters, a valid state, `segments` commands");
    return out;
}

class RolloutGrid
    : public GridHandle<lom_rollout, lom_occupancy_geometry, lom_rollout_create, lom_rollout_destroy, lom_rollout_last_error,
                        lom_rollout_get_geometry, lom_rollout_clear, lom_rollout_shift, lom_rollout_set_option, lom_rollout_device, lom_rollout_stream,
                        lom_rollout_wait_event> {
public:
    struct Result {
        std::vector<lom_rollout_pick> picks;  // one per state
        lom_rollout_summary summary;
    };
    explicit RolloutGrid(const lom_occupancy_geometry &geometry, int device = 0) : GridHandle(geometry, device) {}
    size_t size() const { return cellCount(); }
    // host planes of size() cells (potential may be NULL); commands: k * params.segments (v, w) pairs; footprint: f (fx, fy) pairs
    Result evaluate(const int8_t *cost_plane, const uint32_t *potential, const lom_rollout_state *states, size_t m, const int16_t *commands,
                    size_t k, const int32_t *footprint, size_t f, const lom_rollout_params &params)
    {
        Result r{std::vector<lom_rollout_pick>(m), {}};
        check(lom_rollout_evaluate(h_, cost_plane, potential, states, m, commands, k, footprint, f, &params, r.picks.data(), &r.summary));
        return r;
    }
    // planes in HBM, each complete when its event is (NULL: now)
    Result evaluateDevice(const int8_t *d_cost_plane, void *cost_event, const uint32_t *d_potential, void *potential_event,
                          const lom_rollout_state *states, size_t m, const int16_t *commands, size_t k, const int32_t *footprint, size_t f,
                          const lom_rollout_params &params)
    {
        Result r{std::vector<lom_rollout_pick>(m), {}};
        check(lom_rollout_evaluate_device(h_, d_cost_plane, cost_event, d_potential, potential_event, states, m, commands, k, footprint, f, &params,
                                          r.picks.data(), &r.summary));
        return r;
    }
    // the cost of a ClearanceGrid and the potential of a NavField (or none) of this geometry, read in HBM
    Result evaluateFromGrids(ClearanceGrid &clearance, NavField *navfield, const lom_rollout_state *states, size_t m, const int16_t *commands,
                             size_t k, const int32_t *footprint, size_t f, const lom_rollout_params &params)
    {
        Result r{std::vector<lom_rollout_pick>(m), {}};
        check(lom_rollout_evaluate_from_grids(h_, clearance.handle(), navfield ? navfield->handle() : nullptr, states, m, commands, k, footprint, f,
                                              &params, r.picks.data(), &r.summary));
        return r;
    }
    std::vector<lom_rollout_record> records()
    {
        size_t n = 0;
        check(lom_rollout_records(h_, nullptr, 0, &n));
        std::vector<lom_rollout_record> out(n);
        check(lom_rollout_records(h_, out.data(), out.size(), nullptr));
        return out;
    }
    lom_rollout_call_stats stats() const
    {
        lom_rollout_call_stats s;
        check(lom_rollout_stats(h_, &s));
        return s;
    }
};

// ---- grid shift (not in the reference): the rule by which every grid's shift(dx, dy) moves its geometry -----
// origin' = (float)((double)origin + (double)d * (double)resolution); needs no device
inline lom_occupancy_geometry gridShiftGeometry(const lom_occupancy_geometry &geometry, int32_t dx, int32_t dy)
{
    lom_occupancy_geometry out;
    const int rc = lom_grid_shift_geometry(&geometry, dx, dy, &out);
    if (rc != LOM_OK) throw Error(rc, "grid shift: a valid geometry and an origin that stays finite");
    return out;
}

struct GridShiftCells {
    int32_t dx, dy;
};
// the shift, in multiples of quantum_cells, that brings a robot at (x, y) metres back towards the middle once its cell
// leaves [margin_cells, n - margin_cells) on an axis; {0, 0} while it is inside; needs no device
inline GridShiftCells gridFollow(const lom_occupancy_geometry &geometry, double x, double y, uint32_t margin_cells, uint32_t quantum_cells)
{
    GridShiftCells s{0, 0};
    const int rc = lom_grid_follow(&geometry, x, y, margin_cells, quantum_cells, &s.dx, &s.dy);
    if (rc != LOM_OK)
        throw Error(rc, "grid follow: a valid geometry, a finite position, quantum >= 1, margin + quantum <= side / 2, a position within 2^40 cells");
    return s;
}

// ---- LidarOdometry (src/lidar_odometry.h:20-85) --------------------------------------
// For callers that do not keep the reference's own orchestration: processCloud, getCurrentPose and the
// two key-frame exporters over lom_odometry_*.  lidar_point::PointXYZIRT (src/lidar_point_type.h:13-31)
// has the layout of lom_point_xyzirt, so a PCL cloud's points can be passed as they are.
class LidarOdometry {
public:
    struct Params {  // lidar_odometry.h:23-48, defaults of GetROSDeclaration()
        float lidar_min_range = 4.0f;
        float lidar_max_range = 80.0f;
        float keyframe_voxel_size = 0.2f;
        size_t keyframe_max_points_cnt = 20;
        float keyframe_matching_voxel_size = 0.3f;
        float keyframe_update_voxel_size = 0.1f;
        float keyframe_cleanup_range = 80.0f;
        float angular_divergence_threshold = 5.0f;
    };
    using CloudType = PointCloud<lom_point_xyzirt>;

    explicit LidarOdometry(const Params &config, int device = 0)
    {
        lom_odometry_params p;
        p.lidar_min_range = config.lidar_min_range;
        p.lidar_max_range = config.lidar_max_range;
        p.keyframe_voxel_size = config.keyframe_voxel_size;
        p.keyframe_max_points_cnt = (uint32_t)config.keyframe_max_points_cnt;
        p.keyframe_matching_voxel_size = config.keyframe_matching_voxel_size;
        p.keyframe_update_voxel_size = config.keyframe_update_voxel_size;
        p.keyframe_cleanup_range = config.keyframe_cleanup_range;
        p.angular_divergence_threshold = config.angular_divergence_threshold;
        const int rc = lom_odometry_create(&p, device, &h_);
        if (rc != LOM_OK) throw Error(rc, lom_last_error(nullptr));
    }
    ~LidarOdometry() { lom_odometry_destroy(h_); }
    LidarOdometry(const LidarOdometry &) = delete;
    LidarOdometry &operator=(const LidarOdometry &) = delete;

    void processCloud(const CloudType &input_cloud)  // lidar_odometry.cpp:22-77
    {
        const int rc = lom_odometry_process_cloud(h_, input_cloud.points.data(), input_cloud.points.size());
        if (rc != LOM_OK) throw Error(rc, lom_odometry_last_error(h_));
    }
    // not in the reference: one frame for each of several distinct odometries on one device (lom_odometry_process_batch),
    // for each exactly what processCloud would do; returns the per-stream statuses (LOM_OK where the stream advanced) and
    // throws only where the call was refused before any stream moved
    static std::vector<int> processBatch(const std::vector<LidarOdometry *> &odometries,
                                         const std::vector<const CloudType *> &clouds)
    {
        if (odometries.size() != clouds.size()) throw Error(LOM_ERR_ARG, "processBatch: one cloud per odometry");
        std::vector<lom_odometry *> h(odometries.size());
        std::vector<const lom_point_xyzirt *> f(clouds.size());
        std::vector<size_t> n(clouds.size());
        for (size_t i = 0; i < clouds.size(); i++) {
            if (!odometries[i] || !clouds[i]) throw Error(LOM_ERR_ARG, "processBatch: null odometry or cloud");
            h[i] = odometries[i]->h_;
            f[i] = clouds[i]->points.data();
            n[i] = clouds[i]->points.size();
        }
        std::vector<int> st(h.size(), 1);  // (1: not written -- the call was refused)
        const int rc = lom_odometry_process_batch(h.data(), f.data(), n.data(), (int)h.size(), st.data());
        if (rc != LOM_OK && !st.empty() && st[0] == 1) throw Error(rc, "lom_odometry_process_batch");
        return st;
    }
    // not in the reference: the cloud that will come after the next processCloud, for callers that hold it already; it must
    // stay unchanged until it has been processed (it is copied to pinned memory while that processCloud's align runs)
    void hintNextCloud(const CloudType &next_cloud)
    {
        const int rc = lom_odometry_hint_next(h_, next_cloud.points.data(), next_cloud.points.size());
        if (rc != LOM_OK) throw Error(rc, lom_odometry_last_error(h_));
    }
    // the classifier of the following frames: LOM_CLASSIFIER_RINGS (the reference's, the default) or
    // LOM_CLASSIFIER_NEIGHBOURHOOD for clouds without rings (params required)
    void setClassifier(int kind, const NeighbourhoodParams *params = nullptr)
    {
        const int rc = lom_odometry_set_classifier(h_, kind, params);
        if (rc != LOM_OK) throw Error(rc, lom_odometry_last_error(h_));
    }
    // ray carving in the keyframe update (lom_odometry_set_carve): nullptr, the default, launches nothing
    void setCarve(const lom_carve_params *params)
    {
        const int rc = lom_odometry_set_carve(h_, params);
        if (rc != LOM_OK) throw Error(rc, lom_odometry_last_error(h_));
    }
    // the last keyframe update's carve; false while none has run
    bool carveStats(lom_carve_stats &out) const
    {
        const int rc = lom_odometry_get_carve_stats(h_, &out);
        if (rc != LOM_OK && rc != LOM_ERR_STATE) throw Error(rc, lom_odometry_last_error(h_));
        return rc == LOM_OK;
    }
    // scan votes in rebuildKeyframe (lom_odometry_set_rebuild_votes): nullptr, the default, changes nothing
    void setRebuildVotes(const lom_vote_params *params)
    {
        const int rc = lom_odometry_set_rebuild_votes(h_, params);
        if (rc != LOM_OK) throw Error(rc, "lom_odometry_set_rebuild_votes");
    }
    // the last rebuild's votes; false while none has run
    bool rebuildVoteStats(lom_vote_stats &out) const
    {
        const int rc = lom_odometry_get_rebuild_vote_stats(h_, &out);
        if (rc != LOM_OK && rc != LOM_ERR_STATE) throw Error(rc, "lom_odometry_get_rebuild_vote_stats");
        return rc == LOM_OK;
    }
    // LOM_OPT_QUALITY_REPORT: every frame that aligns also gets a quality report at the pose the align returned
    void setQualityReport(bool on, float min_eig_t = 0.f, float min_eig_r = 0.f)
    {
        int rc = lom_odometry_set_quality_thresholds(h_, min_eig_t, min_eig_r);
        if (rc == LOM_OK) rc = lom_odometry_set_option(h_, LOM_OPT_QUALITY_REPORT, on ? 1 : 0);
        if (rc != LOM_OK) throw Error(rc, lom_odometry_last_error(h_));
    }
    // the last aligned frame's report; throws Error(LOM_ERR_STATE) before the first one or with the option off
    QualityReport getQuality() const
    {
        QualityReport out;
        const int rc = lom_odometry_get_quality(h_, &out);
        if (rc != LOM_OK) throw Error(rc, "no quality report: the option is off or no frame has aligned yet");
        return out;
    }
    // not in the reference: the place descriptor of the last frame's deskewed cloud (getTempCloud) through `db`; with
    // id_out the descriptor also becomes a new entry of db.  Throws Error(LOM_ERR_STATE) before the first frame.
    std::vector<float> placeDescriptor(PlaceDatabase &db, int64_t *id_out = nullptr) const
    {
        std::vector<float> out(db.cells());
        const int rc = lom_odometry_place_descriptor(h_, db.handle(), id_out ? 1 : 0, out.data(), id_out);
        if (rc != LOM_OK) throw Error(rc, rc == LOM_ERR_STATE ? "no frame yet" : lom_place_db_last_error(db.handle()));
        return out;
    }
    // not in the reference: the last frame's update cloud becomes a new scan of the archive; returns its id.  Throws
    // Error(LOM_ERR_STATE) before the first frame.
    int64_t archiveScan(ScanArchive &archive)
    {
        int64_t id = -1;
        const int rc = lom_odometry_archive_scan(h_, archive.handle(), &id);
        if (rc != LOM_OK) throw Error(rc, rc == LOM_ERR_STATE ? "no frame yet" : lom_odometry_last_error(h_));
        return id;
    }
    // not in the reference: the last frame's deskewed cloud, every point and no normals, becomes a new scan of the archive;
    // returns its id.  Throws Error(LOM_ERR_STATE) before the first frame.
    int64_t archiveDeskewed(ScanArchive &archive)
    {
        int64_t id = -1;
        const int rc = lom_odometry_archive_deskewed(h_, archive.handle(), &id);
        if (rc != LOM_OK) throw Error(rc, rc == LOM_ERR_STATE ? "no frame yet" : lom_odometry_last_error(h_));
        return id;
    }
    // not in the reference: that cloud at the current pose votes on an occupancy grid (lom_odometry_occupancy_scan)
    lom_occupancy_stats occupancyScan(OccupancyGrid &grid, const lom_occupancy_ray_params &params)
    {
        lom_occupancy_stats st;
        const int rc = lom_odometry_occupancy_scan(h_, grid.handle(), &params, &st);
        if (rc != LOM_OK) throw Error(rc, rc == LOM_ERR_STATE ? "no frame yet" : lom_occupancy_last_error(grid.handle()));
        return st;
    }
    // not in the reference: that cloud at the current pose into an elevation grid (lom_odometry_elevation_scan)
    lom_elevation_stats elevationScan(ElevationGrid &grid, const lom_elevation_point_params &params)
    {
        lom_elevation_stats st;
        const int rc = lom_odometry_elevation_scan(h_, grid.handle(), &params, &st);
        if (rc != LOM_OK) throw Error(rc, rc == LOM_ERR_STATE ? "no frame yet" : lom_elevation_last_error(grid.handle()));
        return st;
    }
    // not in the reference: go on after a loop closure -- the keyframe again from the archive's scans `ids` at `poses`,
    // culled at keyframe_cleanup_range around new_current, which becomes the current pose (lom_odometry_rebuild_keyframe)
    lom_assemble_stats rebuildKeyframe(ScanArchive &archive, const std::vector<int64_t> &ids,
                                       const std::vector<lom_graph_pose> &poses, const Pose3D &new_current)
    {
        if (ids.size() != poses.size()) throw Error(LOM_ERR_ARG, "rebuildKeyframe: one pose per id");
        const lom_pose p = new_current.c();
        lom_assemble_stats st;
        const int rc = lom_odometry_rebuild_keyframe(h_, archive.handle(), ids.data(), poses.data(), ids.size(), &p, &st);
        if (rc != LOM_OK) throw Error(rc, rc == LOM_ERR_STATE ? "no keyframe yet" : lom_odometry_last_error(h_));
        return st;
    }
    Pose3D getCurrentPose() const  // :87-89
    {
        lom_pose p;
        lom_odometry_get_pose(h_, &p);
        return Pose3D::from(p);
    }
    PointCloud<PointXYZ>::Ptr getKeyFrameCloud() const { return export_(LOM_EXPORT_FIRST_PER_VOXEL); }      // :79-81
    PointCloud<PointXYZ>::Ptr getFullKeyFrameCloud() const { return export_(LOM_EXPORT_FULL_NO_NORMALS); }  // :83-85
    // lidar_odometry.h:73-75; null before the first frame, like the reference's unset shared_ptr
    CloudType::Ptr getTempCloud() const
    {
        const int64_t n = lom_odometry_get_temp_cloud(h_, nullptr, 0);
        if (n < 0) throw Error((int)n, lom_odometry_last_error(h_));
        if (n == 0) return nullptr;
        auto out = std::make_shared<CloudType>();
        out->points.resize((size_t)n);
        lom_odometry_get_temp_cloud(h_, out->points.data(), (size_t)n);
        return out;
    }
    lom_odometry_frame_stats lastFrameStats() const
    {
        lom_odometry_frame_stats s;
        lom_odometry_get_stats(h_, &s);
        return s;
    }

private:
    PointCloud<PointXYZ>::Ptr export_(int mode) const
    {
        lom_map *kf = lom_odometry_keyframe(h_);
        auto out = std::make_shared<PointCloud<PointXYZ>>();
        const int64_t n = lom_map_export(kf, mode, nullptr, nullptr, 0);
        if (n < 0) throw Error((int)n, lom_last_error(kf));
        std::vector<float> xyz((size_t)n * 3 + 3);
        const int64_t m = lom_map_export(kf, mode, xyz.data(), nullptr, (size_t)n);
        if (m < 0) throw Error((int)m, lom_last_error(kf));
        out->points.resize((size_t)n);
        for (size_t i = 0; i < (size_t)n; i++) {
            out->points[i].x = xyz[3 * i];
            out->points[i].y = xyz[3 * i + 1];
            out->points[i].z = xyz[3 * i + 2];
        }
        return out;
    }
    lom_odometry *h_ = nullptr;
};

}  // namespace lom
