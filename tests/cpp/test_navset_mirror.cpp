// lom::NavFieldSet and lom::NavField::adopt of the C++ mirror (include/lidar_odometry_amd.hpp).  Without an argument the
// program runs what needs no device: a create is refused for max_fields of 0 and of 65536 before any device is looked at
// (tests/test_navset_cpp.py).  With one it solves three fields on the device and prints, for tests/test_navset_gpu.py to
// compare with the reference on the same plane and goals: the eight summary values of each field on a line, the 3 x 3
// gather at the goals on a line, cells_owned on a line, then each field cell by cell on a line.
#include <cstdio>
#include <vector>

#include "lidar_odometry_amd.hpp"

static int refusals()
{
    const lom_occupancy_geometry geo{0.25f, -3.f, 2.f, 45, 37};
    for (size_t bad : {(size_t)0, (size_t)65536}) {
        bool threw = false;
        try {
            lom::NavFieldSet s(geo, bad);
        } catch (const lom::Error &e) {
            threw = e.code == LOM_ERR_ARG;
        }
        if (!threw) return 1;
    }
    if (lom_navset_field_count(nullptr) != 0 || lom_navset_device(nullptr) != LOM_ERR_ARG || lom_navset_stream(nullptr) != nullptr) return 2;
    lom_navfield_summary sm;
    if (lom_navfield_adopt(nullptr, nullptr, 0, &sm) != LOM_ERR_ARG) return 3;
    return 0;
}

static int on_the_device()
{
    const lom_occupancy_geometry geo{0.25f, -3.f, 2.f, 45, 37};
    lom::NavFieldSet set(geo, 4);
    lom::NavField f(geo);
    const size_t n = set.size();
    std::vector<int8_t> plane(n);
    for (size_t i = 0; i < n; i++) plane[i] = (int8_t)(i % 7 == 3 ? 100 : (i % 5 == 0 ? -1 : (int)(i % 13) * 7));
    const int32_t goals[10] = {0, 0, 44, 36, 21, 20, 44, 36, -1, 5};  // field 0: two goals; 1: one; 2: a shared one and one outside
    const uint32_t offsets[4] = {0, 2, 3, 5};
    const lom::NavFieldParams p = lom::navfieldParams(20, 2, 300, 80, LOM_NAV_UNKNOWN_PASSABLE);
    if (set.fieldCount() != 0) return 1;
    // an adopt before any solve is refused
    bool threw = false;
    try {
        f.adopt(set, 0);
    } catch (const lom::Error &e) {
        threw = e.code == LOM_ERR_STATE;
    }
    if (!threw) return 2;
    const std::vector<lom_navfield_summary> s = set.solve(plane.data(), p, LOM_NAV_CELLS, goals, offsets, 3);
    if (set.fieldCount() != 3 || s.size() != 3 || set.stats().fields != 3 || set.stats().launches == 0) return 3;
    for (const lom_navfield_summary &m : s)
        if (m.cells_blocked + m.cells_reached + m.cells_unreached != n) return 4;
    const int32_t at[6] = {0, 0, 21, 20, 44, 36};
    const std::vector<uint32_t> matrix = set.gather(LOM_NAV_CELLS, at, 3);
    if (matrix.size() != 9 || matrix[0] != 0 || matrix[4] != 0 || matrix[8] != 0 || matrix[2] != 0) return 5;
    const lom::NavFieldSet::Nearest near = set.nearest();
    uint64_t owned = 0;
    for (uint64_t c : near.cells_owned) owned += c;
    if (owned < s[0].cells_reached) return 6;  // (the union reaches what any one field does)
    // the adopted field is the set's, and the direct solve's
    for (size_t i = 0; i < 3; i++) {
        const lom_navfield_summary a = f.adopt(set, i);
        if (f.potential() != set.potential(i) || a.cells_reached != s[i].cells_reached || a.goals_used != s[i].goals_used) return 7;
        lom::NavField direct(geo);
        const lom_navfield_summary d = direct.solve(plane.data(), p, goals + 2 * offsets[i], offsets[i + 1] - offsets[i]);
        if (direct.potential() != f.potential() || d.max_potential != a.max_potential || d.goals_rejected != a.goals_rejected) return 8;
    }
    // paths across fields, and their refusal
    const int32_t which[2] = {1, 0}, starts[4] = {44, 36, 21, 20}, bad[2] = {0, 3};
    const lom::NavField::Paths walked = set.paths(which, LOM_NAV_CELLS, starts, 2, 8);
    if (walked.lengths.size() != 2 || walked.lengths[0] < 2 || walked.lengths[1] < 2) return 9;
    threw = false;
    try {
        set.paths(bad, LOM_NAV_CELLS, starts, 2, 8);
    } catch (const lom::Error &e) {
        threw = e.code == LOM_ERR_ARG;
    }
    if (!threw) return 10;
    set.shift(2, -1);
    if (set.fieldCount() != 0) return 11;
    std::printf("ALL PASSED\n");
    for (const lom_navfield_summary &m : s)
        std::printf("%llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)m.cells_blocked, (unsigned long long)m.cells_reached,
                    (unsigned long long)m.cells_unreached, (unsigned long long)m.cells_invalid, (unsigned long long)m.goals_used,
                    (unsigned long long)m.goals_rejected, (unsigned long long)m.range_exceeded, (unsigned long long)m.max_potential);
    for (size_t i = 0; i < 9; i++) std::printf("%u%c", matrix[i], i + 1 == 9 ? '\n' : ' ');
    for (size_t i = 0; i < 3; i++) std::printf("%llu%c", (unsigned long long)near.cells_owned[i], i + 1 == 3 ? '\n' : ' ');
    lom::NavFieldSet again(geo, 3);
    again.solve(plane.data(), p, LOM_NAV_CELLS, goals, offsets, 3);
    for (size_t k = 0; k < 3; k++) {
        const std::vector<uint32_t> field = again.potential(k);
        for (size_t i = 0; i < n; i++) std::printf("%u%c", field[i], i + 1 == n ? '\n' : ' ');
    }
    return 0;
}

int main(int argc, char **)
{
    const int rc = argc > 1 ? on_the_device() : refusals();
    if (rc == 0 && argc <= 1) std::printf("ALL PASSED\n");
    return rc;
}
