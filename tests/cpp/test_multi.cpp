// CloudMatcher::alignMulti and LidarOdometry::processBatch of the header-only mirror (include/lidar_odometry_amd.hpp):
// problems against three different keyframes in ONE call against the single aligns on each keyframe, and two odometries
// stepped together against the same frames through processCloud on fresh handles -- bit for bit.  Built and run by
// tests/test_odometry_batch_gpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "check.hpp"
#include "lidar_odometry_amd.hpp"

using namespace lom;

static Quaternionf angleAxis(float angle, float ax, float ay, float az)
{
    const float ha = 0.5f * angle, s = std::sin(ha);
    return {std::cos(ha), s * ax, s * ay, s * az};
}

static bool same_bits(const Pose3D &a, const Pose3D &b)
{
    return std::memcmp(a.translation.v, b.translation.v, sizeof a.translation.v) == 0 &&
           std::memcmp(a.rotation.q, b.rotation.q, sizeof a.rotation.q) == 0;
}

// one 16-ring sweep from (px, py, 0) inside the box room [-lx, lx] x [-ly, ly] x [-2, 6]: ring-ordered, 900 azimuths
static LidarOdometry::CloudType room_scan(float px, float py, float lx, float ly)
{
    LidarOdometry::CloudType c;
    const float pi = 3.14159265358979f;
    for (int r = 0; r < 16; r++) {
        const float el = (-15.f + 2.f * (float)r) * pi / 180.f;
        for (int k = 0; k < 900; k++) {
            const float az = 2.f * pi * (float)k / 900.f;
            const float d[3] = {std::cos(el) * std::cos(az), std::cos(el) * std::sin(az), std::sin(el)};
            const float p[3] = {px, py, 0.f};
            const float lo[3] = {-lx, -ly, -2.f}, hi[3] = {lx, ly, 6.f};
            float t = 1e30f;
            for (int a = 0; a < 3; a++) {
                if (d[a] > 1e-6f) t = std::fmin(t, (hi[a] - p[a]) / d[a]);
                if (d[a] < -1e-6f) t = std::fmin(t, (lo[a] - p[a]) / d[a]);
            }
            lom_point_xyzirt q;
            std::memset(&q, 0, sizeof q);
            q.x = t * d[0];
            q.y = t * d[1];
            q.z = t * d[2];
            q.intensity = 1.f;
            q.ring = (uint16_t)r;
            q.time = 0.1f * (float)k / 900.f;
            c.points.push_back(q);
        }
    }
    return c;
}

int main()
{
    try {
        // ---- alignMulti: three keyframes that differ in voxel size and points per voxel ----
        auto full = std::make_shared<PointCloud<PointNormal>>();
        PointCloud<PointXYZ> full_xyz;
        uint32_t lcg = 777u;
        auto rnd = [&lcg]() {
            lcg = lcg * 1664525u + 1013904223u;
            return (float)((lcg >> 8) / 16777216.0);
        };
        for (int w = 0; w < 3; w++)
            for (int k = 0; k < 40000; k++) {
                const float u = 1.f + 25.f * rnd(), v = 1.f + 25.f * rnd();
                PointNormal p = w == 0 ? PointNormal(u, v, 1.f) : (w == 1 ? PointNormal(u, 1.f, v) : PointNormal(1.f, u, v));
                p.normal_x = w == 2 ? 1.f : 0.f, p.normal_y = w == 1 ? 1.f : 0.f, p.normal_z = w == 0 ? 1.f : 0.f;
                full->points.push_back(p);
                full_xyz.points.emplace_back(p.x, p.y, p.z);
            }
        VoxelGrid k0(0.25, 20), k1(0.5, 1), k2(1.0, 64);
        for (VoxelGrid *k : {&k0, &k1, &k2}) k->addCloud(*full);
        VoxelGrid voxel_filter(0.5, 1);
        voxel_filter.addCloudWithoutNormals(full_xyz);
        auto sub = voxel_filter.getCloudWithoutNormals();
        const float d = 3.14159265358979f / 180.f;
        const std::vector<Pose3D> truths{
            Pose3D({0.0f, 0.0f, 0.1f}, Quaternionf::Identity()),
            Pose3D({0.1f, 0.1f, 0.1f}, Quaternionf::Identity()),
            Pose3D({-0.1f, 0.0f, 0.0f}, angleAxis(-1.0f * d, 0, 0, 1)),
            Pose3D({0.1f, -0.1f, 0.f}, Quaternionf::Identity()),
        };
        const std::vector<const VoxelGrid *> keyframes{&k0, &k1, &k2, &k0};
        std::vector<PointCloud<PointXYZ>::Ptr> clouds;
        std::vector<const PointCloud<PointXYZ> *> ptrs;
        std::vector<Pose3D> guesses;
        for (const auto &g : truths) {
            clouds.push_back(CloudTransformer::transform(*sub, g.inverse()));
            ptrs.push_back(clouds.back().get());
            guesses.push_back(Pose3D());
        }
        CloudMatcher multi, single;
        const std::vector<Pose3D> got = multi.alignMulti(keyframes, ptrs, guesses);
        CHECK(got.size() == truths.size() && multi.batch_stats.size() == truths.size());
        for (size_t i = 0; i < truths.size() && i < got.size(); i++) {
            const Pose3D want = single.align(*keyframes[i], *clouds[i], Pose3D());
            CHECK(same_bits(got[i], want));
            const lom_align_stats &a = multi.batch_stats[i], &b = single.last_stats;
            CHECK(a.outer_iterations == b.outer_iterations && a.lm_iterations == b.lm_iterations);
            CHECK(a.evaluations == b.evaluations && a.queries == b.queries && a.valid_last == b.valid_last);
            CHECK(std::memcmp(&a.final_cost, &b.final_cost, 8) == 0 && std::memcmp(&a.last_step_norm, &b.last_step_norm, 8) == 0);
            CHECK(a.host_fallback == 0 && a.lm_workgroups == b.lm_workgroups);
        }
        CHECK(multi.alignMulti({}, {}, {}).empty() && multi.best == -1);

        // ---- processBatch: two streams in two rooms against the same frames through processCloud ----
        LidarOdometry::Params prm;
        LidarOdometry a(prm), b(prm), sa(prm), sb(prm);
        const std::vector<LidarOdometry *> both{&a, &b};
        bool ok = true;
        for (int f = 0; f < 6; f++) {
            const LidarOdometry::CloudType fa = room_scan(0.15f * (float)f, 0.f, 30.f, 20.f);
            const LidarOdometry::CloudType fb = room_scan(0.f, 0.1f * (float)f, 25.f, 35.f);
            const std::vector<int> st = LidarOdometry::processBatch(both, {&fa, &fb});
            CHECK(st.size() == 2 && st[0] == LOM_OK && st[1] == LOM_OK);
            sa.processCloud(fa);
            sb.processCloud(fb);
            ok = ok && same_bits(a.getCurrentPose(), sa.getCurrentPose()) && same_bits(b.getCurrentPose(), sb.getCurrentPose());
            const lom_odometry_frame_stats x = a.lastFrameStats(), y = sa.lastFrameStats();
            ok = ok && x.matching_points == y.matching_points && x.queries == y.queries &&
                 x.outer_iterations == y.outer_iterations && x.keyframe_voxels == y.keyframe_voxels;
        }
        CHECK(ok);
        CHECK(a.getKeyFrameCloud()->points.size() == sa.getKeyFrameCloud()->points.size());
        // the same odometry twice is refused before anything moves
        const LidarOdometry::CloudType fa = room_scan(1.f, 0.f, 30.f, 20.f);
        bool threw = false;
        try {
            (void)LidarOdometry::processBatch({&a, &a}, {&fa, &fa});
        } catch (const lom::Error &e) {
            threw = e.code == LOM_ERR_ARG;
        }
        CHECK(threw);
        CHECK(same_bits(a.getCurrentPose(), sa.getCurrentPose()));
    } catch (const lom::Error &e) {
        std::printf("lom::Error %d: %s\n", e.code, e.what());
        return 2;
    }
    return check_done();
}
