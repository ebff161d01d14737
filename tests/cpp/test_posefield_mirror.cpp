// lom::PoseField of the C++ mirror (include/lidar_odometry_amd.hpp).  Without an argument the program runs what needs no
// device: the refusals that come before any device is looked at and the two host-only helpers (tests/test_posefield_cpp.py).
// With one it solves on the device and prints, for tests/test_posefield_gpu.py to compare with the Python package on the
// same plane, footprint and goals: the nine summary values on a line, the field state by state on a line, the floor cell
// by cell on a line.
#include <cstdio>
#include <vector>

#include "lidar_odometry_amd.hpp"

static std::vector<int32_t> rectangle_5x3()
{
    size_t n = 0;
    (void)lom_rollout_footprint_rectangle(512, 512, 256, 128, 0, nullptr, 0, &n);
    std::vector<int32_t> fp(2 * n);
    (void)lom_rollout_footprint_rectangle(512, 512, 256, 128, 0, fp.data(), n, &n);
    return fp;
}

static int refusals()
{
    bool threw = false;
    try {
        lom::PoseField f(lom_occupancy_geometry{0.25f, -3.f, 2.f, 0, 37});
    } catch (const lom::Error &e) {
        threw = e.code == LOM_ERR_ARG;
    }
    if (!threw) return 1;
    if (lom_posefield_device(nullptr) != LOM_ERR_ARG || lom_posefield_stream(nullptr) != nullptr || lom_posefield_clear(nullptr) != LOM_ERR_ARG) return 2;
    lom_posefield_summary sm;
    if (lom_posefield_solve(nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, &sm) != LOM_ERR_ARG || lom_posefield_shift(nullptr, 1, 1) != LOM_ERR_ARG)
        return 3;
    for (uint32_t h = 0; h < 8; h++)
        if (lom::posefieldHeadingOfAngle(8192u * h) != h || lom::posefieldHeadingOfAngle(8192u * h + 4095u) != h ||
            lom::posefieldHeadingOfAngle(8192u * h + 4096u) != ((h + 1u) & 7u))
            return 4;
    const int32_t point[2] = {0, 0};
    for (const std::vector<int32_t> &s : lom::posefieldStencils(point, 1))
        if (s != std::vector<int32_t>{0, 0}) return 5;
    const std::vector<int32_t> fp = rectangle_5x3();
    const std::vector<std::vector<int32_t>> st = lom::posefieldStencils(fp.data(), fp.size() / 2);
    if (st.size() != 8 || st[0].size() != 2 * 15 || st[2].size() != 2 * 15 || st[0][0] != -2 || st[0][1] != -1 || st[2][0] != -1 || st[2][1] != -2) return 6;
    threw = false;
    try {
        const int32_t far[2] = {16385, 0};
        (void)lom::posefieldStencils(far, 1);
    } catch (const lom::Error &e) {
        threw = e.code == LOM_ERR_ARG;
    }
    if (!threw) return 7;
    const lom::PoseFieldParams p = lom::posefieldParams(lom::navfieldParams(20, 2, 300, 80, LOM_NAV_UNKNOWN_PASSABLE), 15, 3, 100, LOM_POSE_SPIN);
    if (p.nav.neutral != 20 || p.turn_cost != 15 || p.spin_cost != 3 || p.reverse_cost != 100 || p.flags != LOM_POSE_SPIN) return 8;
    return 0;
}

static int on_the_device()
{
    const lom_occupancy_geometry geo{0.25f, -3.f, 2.f, 45, 37};
    lom::PoseField f(geo);
    const size_t n = f.size();
    std::vector<int8_t> plane(n);
    for (size_t i = 0; i < n; i++) plane[i] = (int8_t)(i % 53 == 3 ? 100 : (i % 41 == 0 ? -1 : (int)(i % 11) * 7));
    const int32_t goals[12] = {22, 18, -1, 5, 30, 2, -1, 3, 0, 22, 18, 1};
    const lom::PoseFieldParams p =
        lom::posefieldParams(lom::navfieldParams(20, 2, 300, 80, LOM_NAV_UNKNOWN_PASSABLE), 15, 3, 100, LOM_POSE_SPIN | LOM_POSE_REVERSE);
    const std::vector<int32_t> fp = rectangle_5x3();
    const lom::PoseFieldSummary s = f.solve(plane.data(), p, fp.data(), fp.size() / 2, goals, 4);
    if (s.states_blocked + s.states_reached + s.states_unreached != 8 * n || s.goals_rejected < 1 || f.stats().launches == 0) return 1;
    const std::vector<uint32_t> field = f.potential(), layers = f.layers();
    const lom::PoseField::Floor floor = f.floor();
    if (field.size() != 8 * n || layers.size() != 8 * n || floor.floor.size() != n || !f.floorDevice()) return 2;
    for (size_t c = 0; c < n; c++) {
        uint32_t least = LOM_NAV_UNREACHED;
        for (size_t h = 0; h < 8; h++) least = field[h * n + c] < least ? field[h * n + c] : least;
        if (floor.floor[c] != least || (least == LOM_NAV_UNREACHED) != (floor.heading[c] == 8)) return 3;
    }
    const int32_t starts[6] = {40, 5, -1, 22, 18, -1};
    const lom::PoseField::Paths walked = f.paths(starts, 2, 64);
    if (walked.lengths.size() != 2 || walked.lengths[0] < 2 || walked.lengths[1] != 1) return 4;
    const float xy[4] = {-3.f + 0.25f * 22.5f, 2.f + 0.25f * 18.5f, -100.f, 0.f};
    const int32_t hd[2] = {-1, 0};
    const std::vector<uint32_t> q = f.query(xy, hd, 2);
    if (q[0] != 0 || q[1] != LOM_NAV_UNREACHED) return 5;
    f.shift(2, -1);
    if (f.potential() != std::vector<uint32_t>(8 * n, LOM_NAV_UNREACHED)) return 6;
    std::printf("ALL PASSED\n");
    std::printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)s.states_blocked, (unsigned long long)s.states_reached,
                (unsigned long long)s.states_unreached, (unsigned long long)s.cells_reached, (unsigned long long)s.cells_invalid,
                (unsigned long long)s.goals_used, (unsigned long long)s.goals_rejected, (unsigned long long)s.range_exceeded,
                (unsigned long long)s.max_potential);
    for (size_t i = 0; i < 8 * n; i++) std::printf("%u%c", field[i], i + 1 == 8 * n ? '\n' : ' ');
    for (size_t i = 0; i < n; i++) std::printf("%u%c", floor.floor[i], i + 1 == n ? '\n' : ' ');
    return 0;
}

int main(int argc, char **)
{
    const int rc = argc > 1 ? on_the_device() : refusals();
    if (rc == 0 && argc <= 1) std::printf("ALL PASSED\n");
    return rc;
}
