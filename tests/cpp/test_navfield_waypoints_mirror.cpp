// lom::NavField::waypoints and ::visible of the C++ mirror (include/lidar_odometry_amd.hpp) against what
// tests/test_navfield_waypoints_gpu.py computes for the same plane, goals and starts: prints the counts, the lengths, the
// waypoint cells and the visibility bytes, a line each.
#include <cmath>
#include <cstdio>
#include <vector>

#include "lidar_odometry_amd.hpp"

int main()
{
    const lom_occupancy_geometry geo{0.25f, -3.f, 2.f, 45, 37};
    lom::NavField f(geo);
    const size_t n = f.size();
    std::vector<int8_t> plane(n);
    for (size_t i = 0; i < n; i++) plane[i] = (int8_t)(i % 7 == 3 ? 100 : (int)(i % 4) * 5);
    const int32_t goals[2] = {40, 30};
    const int32_t starts[10] = {0, 0, 44, 0, 40, 30, -1, 2, 2, 36};
    const size_t wp_cap = 64;
    // before a solve every cell is impassable: no start is walked, and only a cell itself is visible
    const int32_t self[8] = {3, 3, 3, 3, 3, 3, 4, 3};
    const std::vector<uint8_t> blind = f.visible(self, 2);
    if (blind[0] != 1 || blind[1] != 0) return 1;
    if (f.waypoints(LOM_NAV_CELLS, starts, 5, lom::navfieldWaypointParams(0, 64, 200), wp_cap).counts[0] != 0) return 1;
    f.solve(plane.data(), lom::navfieldParams(20, 2, 300, 80), goals, 1);
    const lom::NavField::Waypoints w = f.waypoints(LOM_NAV_CELLS, starts, 5, lom::navfieldWaypointParams(40, 64, 200), wp_cap);
    const lom::NavField::Paths paths = f.paths(LOM_NAV_CELLS, starts, 5, 200);
    for (size_t k = 0; k < 5; k++) {
        if (w.lengths[k] != paths.lengths[k] || w.counts[k] > w.lengths[k]) return 2;
        if (!w.counts[k]) continue;
        // the first and the last cell of the route
        const uint16_t *first = &w.cells[k * wp_cap * 2], *last = first + 2 * (w.counts[k] - 1), *goal = &paths.cells[(k * 200 + w.lengths[k] - 1) * 2];
        if (first[0] != paths.cells[k * 200 * 2] || first[1] != paths.cells[k * 200 * 2 + 1] || last[0] != goal[0] || last[1] != goal[1]) return 3;
        // never longer than the route, whose steps are 1 and sqrt 2 cells long
        double route = 0.0;
        for (uint32_t i = 1; i < w.lengths[k]; i++) {
            const uint16_t *c = &paths.cells[(k * 200 + i) * 2];
            route += (c[0] != c[-2] && c[1] != c[-1]) ? std::sqrt(2.0) : 1.0;
        }
        if (f.polylineLength(first, w.counts[k]) > route * 0.25 + 1e-9) return 4;
    }
    if (w.counts[2] != 1 || w.counts[3] != 0 || w.counts[0] < 2) return 5;
    const std::vector<double> xy = f.waypointsMetres(&w.cells[2 * wp_cap * 2], 1);
    if (xy[0] != -3.0 + 40.5 * 0.25 || xy[1] != 2.0 + 30.5 * 0.25) return 6;
    // a serial run leaves the same bytes; a bad lookahead is refused
    f.setOption(LOM_NAV_OPT_TEST_SHORTCUT_SERIAL, 1);
    const lom::NavField::Waypoints s = f.waypoints(LOM_NAV_CELLS, starts, 5, lom::navfieldWaypointParams(40, 64, 200), wp_cap);
    if (s.cells != w.cells || s.counts != w.counts || s.lengths != w.lengths) return 7;
    bool threw = false;
    try {
        f.waypoints(LOM_NAV_CELLS, starts, 5, lom::navfieldWaypointParams(40, 0, 200), wp_cap);
    } catch (const lom::Error &) {
        threw = true;
    }
    if (!threw) return 8;
    std::vector<int32_t> pairs;
    for (int i = 0; i < 60; i++) {
        pairs.push_back((i * 7) % 45), pairs.push_back((i * 5) % 37);
        pairs.push_back(((i * 7) % 45 + i % 5) % 45), pairs.push_back(((i * 5) % 37 + i % 3) % 37);
    }
    const std::vector<uint8_t> vis = f.visible(pairs.data(), 60, 40);
    std::printf("ALL PASSED\n");
    for (size_t k = 0; k < 5; k++) std::printf("%u%c", w.counts[k], k == 4 ? '\n' : ' ');
    for (size_t k = 0; k < 5; k++) std::printf("%u%c", w.lengths[k], k == 4 ? '\n' : ' ');
    for (size_t i = 0; i < w.cells.size(); i++) std::printf("%u%c", (unsigned)w.cells[i], i + 1 == w.cells.size() ? '\n' : ' ');
    for (size_t i = 0; i < vis.size(); i++) std::printf("%u%c", (unsigned)vis[i], i + 1 == vis.size() ? '\n' : ' ');
    return 0;
}
