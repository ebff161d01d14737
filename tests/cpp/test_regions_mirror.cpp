// lom::RegionGrid of the C++ mirror (include/lidar_odometry_amd.hpp) against what tests/test_regions_gpu.py computes for the
// same planes: prints the five summary values on one line, the labels cell by cell on the next, then the list's records
// field by field and the entry goals.
#include <cstdio>
#include <vector>

#include "lidar_odometry_amd.hpp"

int main()
{
    const lom_occupancy_geometry geo{0.25f, -3.f, 2.f, 45, 37};
    lom::RegionGrid g(geo);
    const size_t n = g.size();
    if (g.labels()[0] != LOM_REGIONS_NONE || !g.list().empty()) return 1;  // after create
    std::vector<int8_t> plane(n);
    std::vector<uint32_t> pot(n);
    for (size_t i = 0; i < n; i++) {
        plane[i] = (int8_t)(i % 7 == 3 ? 100 : (i % 5 == 0 || i % 11 == 2 ? -1 : 0));
        pot[i] = i % 13 == 0 ? LOM_NAV_UNREACHED : (uint32_t)((i * 37u) % 1000u);
    }
    const lom::RegionsParams p = lom::regionsParams(LOM_REGIONS_FRONTIER, 0, 0, 99, 2, LOM_REGIONS_RANK_POTENTIAL, LOM_REGIONS_CONNECT_4);
    const lom_regions_summary s = g.extract(plane.data(), p, nullptr, pot.data());
    const std::vector<uint32_t> labels = g.labels();
    const std::vector<lom_regions_record> list = g.list();
    const std::vector<int32_t> goals = g.goals(LOM_REGIONS_GOAL_ENTRY);
    if (s.regions < 2 || s.regions_recorded != s.regions || list.size() != s.regions_listed || goals.size() != 2 * list.size()) return 2;
    for (size_t k = 0; k < list.size(); k++) {
        if (list[k].cells < 2 || labels[list[k].label] != list[k].label) return 3;
        if (goals[2 * k] != list[k].entry_x || goals[2 * k + 1] != list[k].entry_y) return 3;
        if (k && list[k - 1].entry_potential > list[k].entry_potential) return 3;
    }
    // metres: the grid's origin is cell (0, 0); a point left of it is outside
    const float xy[4] = {-3.f, 2.f, -3.1f, 2.f};
    const std::vector<uint32_t> q = g.query(xy, 2);
    if (q[0] != labels[0] || q[1] != LOM_REGIONS_NONE) return 4;
    g.setOption(LOM_REGIONS_OPT_TEST_TILE_ROWS, 8);
    bool threw = false;
    try {
        g.extract(plane.data(), lom::regionsParams(LOM_REGIONS_FRONTIER, 0, 0, 99, 0, LOM_REGIONS_RANK_LABEL));
    } catch (const lom::Error &) {
        threw = true;
    }
    if (!threw || g.stats().launches < 8 || g.labels() != labels || g.list().size() != list.size()) return 5;  // a refusal changes nothing
    std::printf("ALL PASSED\n%llu %llu %llu %llu %llu\n", (unsigned long long)s.cells_member, (unsigned long long)s.regions,
                (unsigned long long)s.regions_recorded, (unsigned long long)s.regions_listed, (unsigned long long)s.largest_cells);
    for (size_t i = 0; i < n; i++) std::printf("%u%c", labels[i], i + 1 == n ? '\n' : ' ');
    for (const lom_regions_record &r : list)
        std::printf("%u %u %llu %llu %u %u %u %u %u %u %u %u %u %u %u ", r.label, r.cells, (unsigned long long)r.sum_x, (unsigned long long)r.sum_y,
                    r.min_x, r.min_y, r.max_x, r.max_y, r.centroid_x, r.centroid_y, r.centre_x, r.centre_y, r.entry_x, r.entry_y, r.entry_potential);
    std::printf("\n");
    g.clear();
    if (g.labels()[labels.size() - 1] != LOM_REGIONS_NONE || !g.list().empty()) return 6;
    return 0;
}
