// lom::NavField::shiftResolve of the C++ mirror (include/lidar_odometry_amd.hpp) against what tests/test_navfield_shift_gpu.py
// computes for the same planes, goals, shift and window: prints the eight summary values on one line, cells_changed,
// cells_raised, cells_kept, cells_entered and goals_left on the next, then the field cell by cell.
#include <cstdio>
#include <vector>

#include "lidar_odometry_amd.hpp"

int main()
{
    const lom_occupancy_geometry geo{0.25f, -3.f, 2.f, 45, 37};
    lom::NavField f(geo);
    const size_t n = f.size();
    std::vector<int8_t> kept(n), fresh(n);
    for (size_t i = 0; i < n; i++) {
        kept[i] = (int8_t)(i % 7 == 3 ? 100 : (i % 5 == 0 ? -1 : (int)(i % 13) * 7));
        fresh[i] = (int8_t)(i % 11 == 2 ? 100 : (int)(i % 9) * 5);
    }
    const int32_t goals[6] = {0, 0, 44, 36, 20, 20};
    const lom::NavFieldParams p = lom::navfieldParams(20, 2, 300, 80, LOM_NAV_UNKNOWN_PASSABLE);
    // a shift with a re-solve before any solve is refused
    bool threw = false;
    try {
        f.shiftResolve(1, 1, fresh.data());
    } catch (const lom::Error &e) {
        threw = e.code == LOM_ERR_STATE;
    }
    if (!threw) return 1;
    const lom_navfield_summary s0 = f.solve(kept.data(), p, goals, 3);
    const std::vector<uint32_t> before = f.potential();
    const lom_clearance_window window{10, 8, 30, 40};  // cut at the grid's upper edge
    const lom_navfield_summary s = f.shiftResolve(6, -5, fresh.data(), &window);
    const lom_navfield_resolve_counters st = f.resolveStats();
    const lom_navfield_shift_counters sh = f.shiftStats();
    if (s.cells_blocked + s.cells_reached + s.cells_unreached != n) return 2;
    if (s.goals_used + s.goals_rejected + sh.goals_left != s0.goals_used) return 2;
    if (sh.cells_kept != (45u - 6u) * (37u - 5u) || sh.cells_kept + sh.cells_entered != n) return 3;
    if (st.relax_launches == 0 || st.waits < 3) return 3;
    const std::vector<uint32_t> field = f.potential();
    if (field == before) return 4;
    lom_occupancy_geometry moved{}, now = f.geometry();
    if (lom_grid_shift_geometry(&geo, 6, -5, &moved) != LOM_OK || now.origin_x != moved.origin_x || now.origin_y != moved.origin_y) return 5;
    // a shift of (0, 0) over an empty window changes nothing and keeps everything
    const lom_clearance_window none{3, 3, 0, 9};
    const lom_navfield_summary same = f.shiftResolve(0, 0, kept.data(), &none);
    if (f.potential() != field || f.shiftStats().cells_kept != n || same.cells_reached != s.cells_reached) return 6;
    std::printf("ALL PASSED\n%llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)s.cells_blocked,
                (unsigned long long)s.cells_reached, (unsigned long long)s.cells_unreached, (unsigned long long)s.cells_invalid,
                (unsigned long long)s.goals_used, (unsigned long long)s.goals_rejected, (unsigned long long)s.range_exceeded,
                (unsigned long long)s.max_potential);
    std::printf("%llu %llu %llu %llu %llu\n", (unsigned long long)st.cells_changed, (unsigned long long)st.cells_raised,
                (unsigned long long)sh.cells_kept, (unsigned long long)sh.cells_entered, (unsigned long long)sh.goals_left);
    for (size_t i = 0; i < n; i++) std::printf("%u%c", field[i], i + 1 == n ? '\n' : ' ');
    return 0;
}
