// lom::poseLattice and CloudMatcher::bestQuality of the header-only mirror (include/lidar_odometry_amd.hpp) against the
// C functions lom_pose_lattice and lom_quality_batch_best: host code only, no device is touched.  Built and run by
// tests/test_quality_batch_cpp.py.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "check.hpp"
#include "lidar_odometry_amd.hpp"

using namespace lom;

static_assert(LOM_ABI_VERSION == 2 && LOM_NQSUMS == 36 && LOM_OPT_TEST_QUALITY_ROUND_MAX == 108 &&
                  LOM_OPT_TEST_BATCH_ROUND_MAX == 107,
              "ABI constants");
static_assert(sizeof(lom_quality_problem) == 56 && offsetof(lom_quality_problem, n) == 8 &&
                  offsetof(lom_quality_problem, stride_bytes) == 16 && offsetof(lom_quality_problem, t) == 24 &&
                  offsetof(lom_quality_problem, q_wxyz) == 36,
              "lom_quality_problem: the layout the Python binding states");

static void lattice_case(const Pose3D &centre, const Vector3f &half, const Vector3f &step, float half_yaw, float step_yaw,
                         int expect_nodes)
{
    const lom_pose c = centre.c();
    const int n = lom_pose_lattice(&c, half.v, step.v, half_yaw, step_yaw, nullptr, 0);
    CHECK(n == expect_nodes);
    std::vector<lom_pose> raw((size_t)(n > 0 ? n : 0));
    CHECK(lom_pose_lattice(&c, half.v, step.v, half_yaw, step_yaw, raw.data(), n) == n);
    const std::vector<Pose3D> got = poseLattice(centre, half, step, half_yaw, step_yaw);
    CHECK((int)got.size() == n);
    for (size_t i = 0; i < got.size() && i < raw.size(); i++) {
        CHECK(std::memcmp(got[i].translation.v, raw[i].t, sizeof raw[i].t) == 0);
        CHECK(std::memcmp(got[i].rotation.q, raw[i].q, sizeof raw[i].q) == 0);
    }
    if (n > 1) {  // z innermost, ascending from the negative end; the centre in the middle
        const Pose3D &mid = got[(size_t)n / 2];
        CHECK(mid.translation.v[0] == centre.translation.v[0] && mid.translation.v[1] == centre.translation.v[1] &&
               mid.translation.v[2] == centre.translation.v[2]);
        CHECK(got.front().translation.v[0] <= centre.translation.v[0] && got.back().translation.v[0] >= centre.translation.v[0]);
    }
}

int main()
{
    const Pose3D centre(Vector3f(0.02f, -0.01f, 0.f), Quaternionf(0.999998f, 0.f, 0.f, 0.002f));
    lattice_case(centre, Vector3f(0.25f, 0.25f, 0.f), Vector3f(0.25f, 0.25f, 0.f), 0.0436332f, 0.0436332f, 27);
    lattice_case(centre, Vector3f(1.f, 0.55f, 0.2f), Vector3f(0.3f, 0.25f, 0.1f), 0.2f, 0.07f, 7 * 5 * 5 * 5);
    lattice_case(centre, Vector3f(1.f, 1.f, 1.f), Vector3f(0.f, -1.f, 2.f), 1.f, 0.f, 1);
    lattice_case(Pose3D(), Vector3f(0.f, 0.f, 0.f), Vector3f(0.f, 0.f, 0.f), 0.f, 0.f, 1);
    {  // a non-finite input: the C function says LOM_ERR_ARG, the mirror throws it
        const Pose3D bad(Vector3f(NAN, 0.f, 0.f), Quaternionf());
        const lom_pose c = bad.c();
        const float h[3] = {1.f, 1.f, 1.f}, s[3] = {0.5f, 0.5f, 0.5f};
        CHECK(lom_pose_lattice(&c, h, s, 0.f, 0.f, nullptr, 0) == LOM_ERR_ARG);
        bool thrown = false;
        try {
            poseLattice(bad, Vector3f(1.f, 1.f, 1.f), Vector3f(0.5f, 0.5f, 0.5f));
        } catch (const Error &e) {
            thrown = e.code == LOM_ERR_ARG;
        }
        CHECK(thrown);
    }
    {  // best-of: the mirror is the C function
        std::vector<QualityReport> r(5);
        std::memset(r.data(), 0, r.size() * sizeof(QualityReport));
        const long long rows[5][2] = {{0, 0}, {10, 6}, {10, 8}, {10, 8}, {10, 8}};
        const double cost[5] = {0.0, 0.5, 2.0, 1.0, 1.0};
        for (int i = 0; i < 5; i++) {
            r[(size_t)i].queries = rows[i][0];
            r[(size_t)i].valid = rows[i][1];
            r[(size_t)i].cost = cost[i];
        }
        CHECK(lom_quality_batch_best(r.data(), 5) == 3);
        CHECK(CloudMatcher::bestQuality(r) == 3);
        for (int count = 0; count <= 5; count++) {
            const std::vector<QualityReport> head(r.begin(), r.begin() + count);
            CHECK(CloudMatcher::bestQuality(head) == lom_quality_batch_best(r.data(), count));
        }
        CHECK(CloudMatcher::bestQuality({}) == -1 && lom_quality_batch_best(nullptr, 3) == -1);
    }
    return check_done();
}
