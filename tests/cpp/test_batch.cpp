// CloudMatcher::alignBatch of the header-only mirror (include/lidar_odometry_amd.hpp): the seven guesses of the
// reference's MatchingTest (test/test.cpp:226-262) on a synthetic corner scene, handed over in ONE call, against the
// same seven align() calls -- bit for bit, counters included.  Built and run by tests/test_align_batch_gpu.py.
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

int main()
{
    try {
        auto full = std::make_shared<PointCloud<PointNormal>>();
        PointCloud<PointXYZ> full_xyz;
        uint32_t lcg = 12345u;
        auto rnd = [&lcg]() {
            lcg = lcg * 1664525u + 1013904223u;
            return (float)((lcg >> 8) / 16777216.0);
        };
        for (int w = 0; w < 3; w++)
            for (int k = 0; k < 60000; k++) {
                const float u = 1.f + 25.f * rnd(), v = 1.f + 25.f * rnd();
                PointNormal p = w == 0 ? PointNormal(u, v, 1.f) : (w == 1 ? PointNormal(u, 1.f, v) : PointNormal(1.f, u, v));
                p.normal_x = w == 2 ? 1.f : 0.f, p.normal_y = w == 1 ? 1.f : 0.f, p.normal_z = w == 0 ? 1.f : 0.f;
                full->points.push_back(p);
                full_xyz.points.emplace_back(p.x, p.y, p.z);
            }
        VoxelGrid keyframe(0.25, 20);
        keyframe.addCloud(*full);
        VoxelGrid voxel_filter(0.5, 1);
        voxel_filter.addCloudWithoutNormals(full_xyz);
        auto sub = voxel_filter.getCloudWithoutNormals();
        const float d = 3.14159265358979f / 180.f;
        const std::vector<Pose3D> guess_poses{
            Pose3D({0.0f, 0.0f, 0.0f}, Quaternionf::Identity()),
            Pose3D({0.0f, 0.0f, 0.1f}, Quaternionf::Identity()),
            Pose3D({0.1f, 0.1f, 0.1f}, Quaternionf::Identity()),
            Pose3D({-0.1f, -0.1f, -0.1f}, Quaternionf::Identity()),
            Pose3D({0.1f, -0.1f, 0.f}, Quaternionf::Identity()),
            Pose3D({0.0f, 0.0f, 0.0f}, angleAxis(-1.0f * d, 0, 0, 1)),
            Pose3D({-0.2f, 0.0f, 0.0f}, angleAxis(2.0f * d, 0, 0, 1)),
        };
        std::vector<PointCloud<PointXYZ>::Ptr> clouds;
        std::vector<const PointCloud<PointXYZ> *> ptrs;
        std::vector<Pose3D> guesses;
        for (const auto &g : guess_poses) {
            clouds.push_back(CloudTransformer::transform(*sub, g.inverse()));
            ptrs.push_back(clouds.back().get());
            guesses.push_back(Pose3D());
        }
        CloudMatcher batch, single;
        const std::vector<Pose3D> got = batch.alignBatch(keyframe, ptrs, guesses);
        CHECK(got.size() == guess_poses.size() && batch.batch_stats.size() == guess_poses.size());
        std::vector<lom_align_stats> singles;
        for (size_t i = 0; i < guess_poses.size() && i < got.size(); i++) {
            const Pose3D want = single.align(keyframe, *clouds[i], Pose3D());
            singles.push_back(single.last_stats);
            CHECK(same_bits(got[i], want));
            const lom_align_stats &a = batch.batch_stats[i], &b = single.last_stats;
            CHECK(a.outer_iterations == b.outer_iterations && a.lm_iterations == b.lm_iterations);
            CHECK(a.evaluations == b.evaluations && a.queries == b.queries && a.valid_last == b.valid_last);
            CHECK(std::memcmp(&a.final_cost, &b.final_cost, 8) == 0 && std::memcmp(&a.last_step_norm, &b.last_step_norm, 8) == 0);
            CHECK(a.host_fallback == 0 && a.lm_workgroups == b.lm_workgroups);
            CHECK(got[i].relativeTo(guess_poses[i]).translation.norm() < 0.05);  // test.cpp:261
        }
        std::vector<lom_align_result> r(singles.size());
        for (size_t i = 0; i < singles.size(); i++) r[i].stats = singles[i];
        CHECK(batch.best == lom_align_batch_best(r.data(), (int)r.size()));
        // nothing to do is not an error
        CHECK(batch.alignBatch(keyframe, {}, {}).empty() && batch.best == -1);
    } catch (const lom::Error &e) {
        std::printf("lom::Error %d: %s\n", e.code, e.what());
        return 2;
    }
    return check_done();
}
