// lom::QualityReport, CloudMatcher::quality and LidarOdometry::setQualityReport / getQuality of the header-only mirror
// (include/lidar_odometry_amd.hpp) against the C ABI: the layout of lom_quality_report, a corner scene (three planes:
// every direction constrained) and a corridor-like scene (two of them: one direction free), the odometry's option on and
// off.  Built and run by tests/test_quality_cpp.py.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "check.hpp"
#include "lidar_odometry_amd.hpp"

using namespace lom;

static_assert(sizeof(lom_quality_report) == 920 && offsetof(lom_quality_report, overlap) == 24 &&
                  offsetof(lom_quality_report, sum_w) == 80 && offsetof(lom_quality_report, information) == 88 &&
                  offsetof(lom_quality_report, gradient) == 376 && offsetof(lom_quality_report, eig_t) == 424 &&
                  offsetof(lom_quality_report, eigvec_t) == 448 && offsetof(lom_quality_report, eig_r) == 520 &&
                  offsetof(lom_quality_report, eigvec_r) == 544 && offsetof(lom_quality_report, covariance) == 616 &&
                  offsetof(lom_quality_report, degenerate_t) == 904 && offsetof(lom_quality_report, covariance_valid) == 912,
              "lom_quality_report: the layout the Python binding and tests/quality_ref.py state");
static_assert(LOM_ABI_VERSION == 2 && LOM_OPT_QUALITY_REPORT == 8 && LOM_NQSUMS == 36, "ABI constants");

static bool same_bits(const Pose3D &a, const Pose3D &b)
{
    return std::memcmp(a.translation.v, b.translation.v, sizeof a.translation.v) == 0 &&
           std::memcmp(a.rotation.q, b.rotation.q, sizeof a.rotation.q) == 0;
}

// one 16-ring sweep from (px, 0, 0) inside the box room [-30, 30] x [-20, 20] x [-2, 6]
static LidarOdometry::CloudType room_scan(float px)
{
    LidarOdometry::CloudType c;
    const float pi = 3.14159265358979f;
    for (int r = 0; r < 16; r++) {
        const float el = (-15.f + 2.f * (float)r) * pi / 180.f;
        for (int k = 0; k < 900; k++) {
            const float az = 2.f * pi * (float)k / 900.f;
            const float d[3] = {std::cos(el) * std::cos(az), std::cos(el) * std::sin(az), std::sin(el)};
            const float p[3] = {px, 0.f, 0.f};
            const float lo[3] = {-30.f, -20.f, -2.f}, hi[3] = {30.f, 20.f, 6.f};
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
        // planes z = 1, y = 1 and (the corner only) x = 1, exact axis normals
        uint32_t lcg = 4242u;
        auto rnd = [&lcg]() {
            lcg = lcg * 1664525u + 1013904223u;
            return (float)((lcg >> 8) / 16777216.0);
        };
        for (int planes = 3; planes >= 2; planes--) {
            auto full = std::make_shared<PointCloud<PointNormal>>();
            PointCloud<PointXYZ> scan;
            for (int w = 0; w < planes; w++)
                for (int k = 0; k < 20000; k++) {
                    const float u = 1.f + 20.f * rnd(), v = 1.f + 20.f * rnd();
                    PointNormal p = w == 0 ? PointNormal(u, v, 1.f) : (w == 1 ? PointNormal(u, 1.f, v) : PointNormal(1.f, u, v));
                    p.normal_x = w == 2 ? 1.f : 0.f, p.normal_y = w == 1 ? 1.f : 0.f, p.normal_z = w == 0 ? 1.f : 0.f;
                    full->points.push_back(p);
                    if (k % 4 == 0) scan.points.emplace_back(p.x, p.y, p.z);
                }
            VoxelGrid keyframe(0.5, 20);
            keyframe.addCloud(*full);
            CloudMatcher m;
            const Pose3D pose({0.02f, -0.03f, 0.05f}, Quaternionf::Identity());
            std::vector<float> res;
            const QualityReport q = m.quality(keyframe, scan, pose, 0.3f, 0.01f, 0.01f, &res);
            // the same bytes from the C entry on the map handle, and again from the mirror
            lom_quality_report c;
            const lom_pose g = pose.c();
            CHECK(lom_match_quality(keyframe.handle(), &scan.points.data()->x, scan.points.size(), sizeof(PointXYZ), g.t, g.q,
                                     0.3f, 0.01f, 0.01f, &c, nullptr) == LOM_OK);
            CHECK(std::memcmp(&c, &q, sizeof q) == 0);
            const QualityReport again = m.quality(keyframe, scan, pose, 0.3f, 0.01f, 0.01f);
            CHECK(std::memcmp(&again, &q, sizeof q) == 0);
            CHECK(q.queries == (int64_t)scan.points.size() && q.valid > q.queries / 2);
            CHECK(q.inliers <= q.valid && q.inliers > q.valid / 10 * 9);
            CHECK(res.size() == scan.points.size());
            int64_t finite = 0;
            double sum2 = 0.0;
            for (float r : res)
                if (!std::isnan(r)) {
                    finite++;
                    sum2 += (double)r * (double)r;
                }
            CHECK(finite == q.valid);
            CHECK(std::fabs(std::sqrt(sum2 / (double)q.valid) - q.rmse) < 1e-6 * q.rmse);
            CHECK(q.rmse > 0.015 && q.rmse < 0.06);  // offsets 0.05 (z), 0.03 (y), 0.02 (x) from the planes
            CHECK(q.max_abs_residual >= 0.0499 && q.max_abs_residual < 0.3001);  // |r| <= the distance to the winner < the gate
            for (int a = 0; a < 6; a++)
                for (int b = 0; b < 6; b++) CHECK(q.information[a * 6 + b] == q.information[b * 6 + a]);
            CHECK(std::fabs(q.eig_t[0] + q.eig_t[1] + q.eig_t[2] - 1.0) < 1e-9);
            if (planes == 3) {
                CHECK(q.degenerate_t == 0 && q.degenerate_r == 0 && q.covariance_valid == 1);
                CHECK(q.eig_t[0] > 0.2);
                for (int a = 0; a < 6; a++) CHECK(q.covariance[a * 6 + a] > 0.0);
            } else {  // nothing constrains x: an exact zero share along +-x, a zero pivot
                CHECK(q.eig_t[0] == 0.0 && std::fabs(q.eigvec_t[0]) == 1.0 && q.eigvec_t[1] == 0.0 && q.eigvec_t[2] == 0.0);
                CHECK(q.degenerate_t == 1 && q.covariance_valid == 0 && q.covariance[0] == 0.0);
            }
        }

        // the odometry's option: same poses on and off, a report only where it is on and a frame has aligned
        LidarOdometry::Params prm;
        LidarOdometry on(prm), off(prm);
        on.setQualityReport(true, 0.01f, 0.01f);
        bool ok = true;
        for (int f = 0; f < 5; f++) {
            const LidarOdometry::CloudType fr = room_scan(0.15f * (float)f);
            bool early = false;
            if (f == 0) {
                try {
                    (void)on.getQuality();
                } catch (const lom::Error &e) {
                    early = e.code == LOM_ERR_STATE;
                }
                CHECK(early);
            }
            on.processCloud(fr);
            off.processCloud(fr);
            ok = ok && same_bits(on.getCurrentPose(), off.getCurrentPose());
            if (f > 0) {
                const QualityReport q = on.getQuality();
                ok = ok && q.queries == on.lastFrameStats().matching_points && q.valid > 100 && q.covariance_valid == 1;
            }
            bool threw = false;
            try {
                (void)off.getQuality();
            } catch (const lom::Error &e) {
                threw = e.code == LOM_ERR_STATE;
            }
            ok = ok && threw;
        }
        CHECK(ok);
    } catch (const lom::Error &e) {
        std::printf("lom::Error %d: %s\n", e.code, e.what());
        return 2;
    }
    return check_done();
}
