// lom::NavField of the C++ mirror (include/lidar_odometry_amd.hpp) against what tests/test_navfield_gpu.py computes for the
// same plane and goals: prints the eight summary values on one line, then the field cell by cell on the next.
#include <cstdio>
#include <vector>

#include "lidar_odometry_amd.hpp"

int main()
{
    const lom_occupancy_geometry geo{0.25f, -3.f, 2.f, 45, 37};
    lom::NavField f(geo);
    const size_t n = f.size();
    std::vector<int8_t> plane(n);
    for (size_t i = 0; i < n; i++) plane[i] = (int8_t)(i % 7 == 3 ? 100 : (i % 5 == 0 ? -1 : (int)(i % 13) * 7));
    const int32_t goals[10] = {0, 0, 44, 36, 20, 20, -1, 3, 0, 0};
    const lom::NavFieldParams p = lom::navfieldParams(20, 2, 300, 80, LOM_NAV_UNKNOWN_PASSABLE);
    const lom_navfield_summary s = f.solve(plane.data(), p, goals, 5);
    if (s.cells_blocked + s.cells_reached + s.cells_unreached != n) return 1;
    if (s.goals_used + s.goals_rejected != 4) return 1;  // a duplicate counts once
    const std::vector<uint32_t> field = f.potential();
    if (field[0] != 0 || field[n - 1] != 0) return 2;
    // a path from a reached cell ends on a goal, and its first cell is the start
    const int32_t starts[4] = {10, 30, -1, -1};
    const lom::NavField::Paths paths = f.paths(LOM_NAV_CELLS, starts, 2, 200);
    const uint32_t len = paths.lengths[0];
    if (len < 2 || len > 200 || paths.lengths[1] != 0 || paths.cells[0] != 10 || paths.cells[1] != 30) return 3;
    const size_t last = (size_t)paths.cells[2 * (len - 1) + 1] * 45 + paths.cells[2 * (len - 1)];
    if (field[last] != 0) return 3;
    // metres: the grid's origin is cell (0, 0); a point left of it is outside
    const float xy[4] = {-3.f, 2.f, -3.1f, 2.f};
    const std::vector<uint32_t> q = f.query(xy, 2);
    if (q[0] != field[0] || q[1] != LOM_NAV_UNREACHED) return 4;
    const float goal_xy[2] = {-3.f + 0.25f * 21.5f, 2.f + 0.25f * 20.5f};
    const lom_navfield_summary sm = f.solveMetres(plane.data(), p, goal_xy, 1);
    if (sm.goals_used != 1 || f.potential()[(size_t)20 * 45 + 21] != 0) return 5;
    if (lom::navfieldCellCosts(p)[80] != 180 || lom::navfieldCellCosts(p)[81] != 0 || lom::navfieldCellCosts(p)[255] != 300) return 6;
    f.setOption(LOM_NAV_OPT_TEST_BATCH, 3);
    bool threw = false;
    try {
        f.solve(plane.data(), lom::navfieldParams(0, 2, 300, 80), goals, 5);
    } catch (const lom::Error &) {
        threw = true;
    }
    if (!threw || f.stats().launches < 1) return 7;
    std::printf("ALL PASSED\n%llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)s.cells_blocked,
                (unsigned long long)s.cells_reached, (unsigned long long)s.cells_unreached, (unsigned long long)s.cells_invalid,
                (unsigned long long)s.goals_used, (unsigned long long)s.goals_rejected, (unsigned long long)s.range_exceeded,
                (unsigned long long)s.max_potential);
    for (size_t i = 0; i < n; i++) std::printf("%u%c", field[i], i + 1 == n ? '\n' : ' ');
    return 0;
}
