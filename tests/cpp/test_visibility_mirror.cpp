// lom::VisibilityGrid of the C++ mirror (include/lidar_odometry_amd.hpp) against what tests/test_visibility_gpu.py computes
// for the same plane and viewpoints: prints the five summary values on one line, then the records field by field, the beam
// words, the window words and the picks, a line each.
#include <cstdio>
#include <vector>

#include "lidar_odometry_amd.hpp"

int main()
{
    const lom_occupancy_geometry geo{0.25f, -3.f, 2.f, 45, 37};
    lom::VisibilityGrid g(geo);
    const size_t n = g.size();
    if (!g.records().empty() || g.stats().launches != 0) return 1;  // after create
    std::vector<int8_t> plane(n);
    for (size_t i = 0; i < n; i++) plane[i] = (int8_t)(i % 7 == 3 ? 100 : (i % 5 == 0 || i % 11 == 2 ? -1 : 0));
    std::vector<int32_t> vp;
    for (int k = 0; k < 12; k++) vp.push_back((k * 13) % 50 - 2), vp.push_back((k * 7) % 40 - 1);
    const lom::VisibilityParams p = lom::visibilityParams(90, 9, 100, 2, LOM_VIS_KEEP_WINDOWS | LOM_VIS_KEEP_BEAMS);
    const lom_visibility_summary s = g.cast(plane.data(), vp.data(), 12, p);
    const std::vector<lom_visibility_record> records = g.records();
    const std::vector<uint32_t> beams = g.beams();
    size_t words = 0;
    const std::vector<uint32_t> windows = g.windows(&words);
    if (s.viewpoints != 12 || records.size() != 12 || beams.size() != 12 * 90 || words != 19 || windows.size() != 12 * 19) return 2;
    if (g.stats().launches != 2 || g.stats().waits != 1 || !g.windowsDevice()) return 2;
    uint64_t unknown = 0;
    for (const lom_visibility_record &r : records) {
        if (r.unknown + r.free + r.blocked != r.seen || (r.valid == 0) != (r.seen == 0)) return 3;
        unknown += r.unknown;
    }
    if (unknown != s.unknown_total || records[s.unknown_argmax].unknown != s.unknown_max) return 3;
    const std::vector<int32_t> table = lom::visibilityTable(90);
    if (table.size() != 180 || table[0] != 32768 || table[1] != 0) return 4;
    std::vector<uint32_t> cost(12);
    for (uint32_t k = 0; k < 12; k++) cost[k] = (k * 5u) % 7u;
    const std::vector<lom_visibility_pick> picks = g.select(lom_visibility_select_params{4, 2, 0, 1}, cost.data());
    if (picks.empty() || g.stats().launches != 13 || g.stats().waits != 1) return 5;
    bool threw = false;
    try {
        g.cast(plane.data(), vp.data(), 12, lom::visibilityParams(3, 9));
    } catch (const lom::Error &) {
        threw = true;
    }
    if (!threw || g.beams() != beams || g.windows() != windows) return 6;  // a refusal changes nothing
    std::printf("ALL PASSED\n%llu %llu %llu %llu %llu\n", (unsigned long long)s.viewpoints, (unsigned long long)s.valid,
                (unsigned long long)s.unknown_total, (unsigned long long)s.unknown_max, (unsigned long long)s.unknown_argmax);
    for (const lom_visibility_record &r : records)
        std::printf("%d %d %u %u %u %u %u %u ", r.ix, r.iy, r.valid, r.seen, r.unknown, r.free, r.blocked, r.hits);
    std::printf("\n");
    for (size_t i = 0; i < beams.size(); i++) std::printf("%u%c", beams[i], i + 1 == beams.size() ? '\n' : ' ');
    for (size_t i = 0; i < windows.size(); i++) std::printf("%u%c", windows[i], i + 1 == windows.size() ? '\n' : ' ');
    for (const lom_visibility_pick &e : picks) std::printf("%u %u %lld ", e.k, e.gain, (long long)e.score);
    std::printf("\n");
    g.clear();
    if (!g.records().empty()) return 7;
    return 0;
}
