// lom::RolloutGrid and the rollout helpers of the C++ mirror (include/lidar_odometry_amd.hpp).  Without an argument only
// the host-only helpers run (tests/test_rollout_cpp.py: no device is touched); with "device" the grid evaluates the scene
// tests/test_rollout_gpu.py computes as well and prints the summary, the picks and the records, a line each.
#include <cstdio>
#include <cstring>
#include <vector>

#include "lidar_odometry_amd.hpp"

int main(int argc, char **argv)
{
    const lom_occupancy_geometry geo{0.25f, -3.f, 2.f, 45, 37};
    const std::vector<int32_t> fp = lom::rolloutFootprintRectangle(300, 200, 150, 100, true);
    if (fp.size() != 2 * 16 || fp[0] != -200 || fp[1] != -150 || fp[fp.size() - 2] != 300 || fp.back() != 150) return 1;
    if (lom::rolloutFootprintRectangle(300, 200, 150, 100).size() != 2 * 24) return 1;
    const lom::RolloutState s0 = lom::rolloutStateFromPose(geo, -3.f, 2.f, 0.f);
    if (s0.x != 0 || s0.y != 0 || s0.a != 0) return 2;
    const lom::RolloutParams p = lom::rolloutParams(2, 20, 100, 7, 3, 2, 1, 50, LOM_ROLLOUT_KEEP_RECORDS);
    const int16_t straight[4] = {32767, 0, 32767, 0};
    const std::vector<lom::RolloutState> poses = lom::rolloutPoses(p, lom::RolloutState{5, 6, 0}, straight);
    if (poses.size() != 41 || poses[40].x != 5 + 40 * 32767 || poses[40].y != 6 || poses[40].a != 0) return 3;
    bool threw = false;
    try {
        lom::rolloutFootprintRectangle(1, 1, 1, 0);
    } catch (const lom::Error &) {
        threw = true;
    }
    if (!threw) return 4;
    if (argc < 2 || std::strcmp(argv[1], "device") != 0) {
        std::printf("ALL PASSED\n");
        return 0;
    }

    lom::RolloutGrid g(geo);
    const size_t n = g.size();
    if (!g.records().empty() || g.stats().launches != 0) return 5;  // after create
    std::vector<int8_t> plane(n);
    for (size_t i = 0; i < n; i++) plane[i] = (int8_t)(i % 97 == 3 ? 100 : (i % 41 == 0 ? -1 : (int)(i % 13)));
    std::vector<uint32_t> potential(n);
    for (size_t i = 0; i < n; i++) potential[i] = i % 53 == 5 ? LOM_NAV_UNREACHED : (uint32_t)((i * 7) % 3000);
    std::vector<lom::RolloutState> states;
    for (int k = 0; k < 5; k++) states.push_back(lom::RolloutState{(k * 9 + 2) * 32768 + 100 * k, (k * 7 + 3) * 32768 + 5, (uint32_t)(k * 9000)});
    states.push_back(lom::RolloutState{-40000, 70000, 0});  // outside
    std::vector<int16_t> commands;
    for (int k = 0; k < 70; k++)
        for (int l = 0; l < 2; l++) commands.push_back((int16_t)((k * 911) % 30000 - 9000)), commands.push_back((int16_t)((k * 37 + l * 500) % 1200 - 600));
    const lom::RolloutGrid::Result r = g.evaluate(plane.data(), potential.data(), states.data(), states.size(), commands.data(), 70, fp.data(), fp.size() / 2, p);
    const std::vector<lom_rollout_record> records = g.records();
    if (r.picks.size() != 6 || records.size() != 6 * 70 || r.summary.states != 6 || r.summary.candidates != 420) return 6;
    if (g.stats().launches != 3 || g.stats().waits != 1) return 6;
    threw = false;
    try {
        g.evaluate(plane.data(), potential.data(), states.data(), states.size(), commands.data(), 70, fp.data(), fp.size() / 2, lom::rolloutParams(9, 20));
    } catch (const lom::Error &) {
        threw = true;
    }
    const std::vector<lom_rollout_record> again = g.records();
    if (!threw || again.size() != records.size() || std::memcmp(again.data(), records.data(), records.size() * sizeof(lom_rollout_record)) != 0) return 7;
    std::printf("ALL PASSED\n%llu %llu %llu %llu %llu\n", (unsigned long long)r.summary.states, (unsigned long long)r.summary.valid_states,
                (unsigned long long)r.summary.candidates, (unsigned long long)r.summary.admissible, (unsigned long long)r.summary.states_without_pick);
    for (const lom_rollout_pick &e : r.picks) std::printf("%u %u %lld ", e.k, e.admissible, (long long)e.score);
    std::printf("\n");
    for (const lom_rollout_record &e : records)
        std::printf("%u %u %u %u %d %d %u %u ", e.free_poses, e.reason, e.cost_sum, e.cost_max, e.end_x, e.end_y, e.end_angle, e.end_potential);
    std::printf("\n");
    g.clear();
    if (!g.records().empty()) return 8;
    return 0;
}
