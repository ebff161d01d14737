// lom::ClearanceGrid of the C++ mirror (include/lidar_odometry_amd.hpp) against what tests/test_clearance_gpu.py computes
// for the same planes with tests/clearance_ref.py: prints the six summary counts, then the sums of d2 and of the cost.
#include <cmath>
#include <cstdio>
#include <vector>

#include "lidar_odometry_amd.hpp"

int main()
{
    const lom_occupancy_geometry geo{0.25f, -3.f, 2.f, 45, 37};
    lom::ClearanceGrid g(geo);
    const size_t n = g.size();
    std::vector<int8_t> occ(n), elev(n);
    for (size_t i = 0; i < n; i++) {
        occ[i] = (int8_t)(i % 97 == 5 ? 100 : (i % 3 == 0 ? -1 : 0));
        elev[i] = (int8_t)(i % 41 == 7 ? 100 : (int)(i % 11) * 9 - 1);
    }
    const lom::ClearanceParams p = lom::clearanceParams(1.8f, 0.6f, 0.7f, LOM_CLEAR_FREE_CLEARS_ELEVATION);
    const lom_clearance_summary full = g.update(occ.data(), elev.data(), p);
    const lom_clearance_window w{-2, 30, 20, 20};
    g.clear();
    const lom_clearance_summary s = g.update(occ.data(), elev.data(), p, &w);
    if (s.cells_lethal + s.cells_inscribed + s.cells_costed + s.cells_unknown != 18u * 7u) return 1;
    if (full.cells_lethal + full.cells_inscribed + full.cells_costed + full.cells_unknown != n) return 1;
    g.update(occ.data(), nullptr, p, nullptr);
    g.update(occ.data(), elev.data(), p);
    lom_clearance_summary plane;
    const std::vector<int8_t> cost = g.cost(&plane);
    const std::vector<uint16_t> d2 = g.distanceSq();
    const std::vector<float> m = g.distance();
    unsigned long long sum_d2 = 0;
    long long sum_cost = 0;
    for (size_t i = 0; i < n; i++) {
        sum_d2 += d2[i], sum_cost += cost[i];
        if (d2[i] == LOM_CLEAR_FAR ? !std::isinf(m[i]) : m[i] != (float)(std::sqrt((double)d2[i]) * 0.25)) return 2;
    }
    if (plane.cells_lethal != full.cells_lethal || plane.cells_invalid != 0) return 3;
    const float xy[6] = {-3.f, 2.f, -3.1f, 2.f, 0.f, 5.f};
    const lom::ClearanceGrid::Query q = g.query(xy, 3);
    if (q.cost[0] != cost[0] || q.cost[1] != -1 || !std::isnan(q.distance[1]) || q.cost[2] != cost[(size_t)12 * 45 + 12]) return 4;
    g.setOption(LOM_CLEAR_OPT_TEST_TILE_ROWS, 8);
    bool threw = false;
    try {
        g.update(nullptr, nullptr, p);
    } catch (const lom::Error &) {
        threw = true;
    }
    if (!threw) return 5;
    std::printf("ALL PASSED\n%llu %llu %llu %llu %llu %llu %llu %lld\n", (unsigned long long)full.cells_lethal,
                (unsigned long long)full.cells_inscribed, (unsigned long long)full.cells_costed, (unsigned long long)full.cells_unknown,
                (unsigned long long)full.cells_invalid, (unsigned long long)full.cells_cleared, sum_d2, sum_cost);
    return 0;
}
