// The re-solve of lom::PoseField of the C++ mirror (include/lidar_odometry_amd.hpp): the three methods compile, and what
// needs no device runs -- the refusals that come before any device is looked at (tests/test_posefield_resolve_cpp.py).
#include <cstdio>
#include <cstring>

#include "lidar_odometry_amd.hpp"

// (instantiated, never called: the methods compile against the header's prototypes)
static lom::PoseFieldSummary compiled(lom::PoseField &f, lom::ClearanceGrid &c, const int8_t *plane)
{
    const lom_clearance_window w{1, 2, 3, 4};
    (void)f.resolve(plane);
    (void)f.resolveDevice(plane, nullptr, &w);
    (void)f.resolveFromClearance(c, &w);
    (void)f.resolveStats().states_raised;
    return f.resolve(plane, &w);
}

int main()
{
    (void)&compiled;
    const int8_t plane[4] = {0, 0, 0, 0};
    lom_posefield_summary sm;
    std::memset(&sm, 0xFF, sizeof sm);
    if (lom_posefield_resolve(nullptr, plane, nullptr, &sm) != LOM_ERR_ARG || sm.states_reached != 0 || sm.max_potential != 0) return 1;
    std::memset(&sm, 0xFF, sizeof sm);
    if (lom_posefield_resolve_device(nullptr, plane, nullptr, nullptr, &sm) != LOM_ERR_ARG || sm.goals_used != 0) return 2;
    std::memset(&sm, 0xFF, sizeof sm);
    if (lom_posefield_resolve_from_clearance(nullptr, nullptr, nullptr, &sm) != LOM_ERR_ARG || sm.states_blocked != 0) return 3;
    lom_posefield_resolve_counters st;
    if (lom_posefield_resolve_stats(nullptr, &st) != LOM_ERR_ARG) return 4;
    if (sizeof(lom_posefield_resolve_counters) != 56 || LOM_POSE_OPT_TEST_RESOLVE_FORM != 4) return 5;
    std::printf("ALL PASSED\n");
    return 0;
}
