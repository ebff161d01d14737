// assemble::cut_launches (csrc/assemble_host.cpp), the one loop that cuts the scans of a call into launches, and the three
// planners that use it -- vote::plan, occupancy::plan, elevation::plan -- compiled into a program of its own under
// -fsanitize=address,undefined (tests/test_launch_cut_cpp.py): caps 1, 2, 3 and each planner's default, a call of no
// scans, launches of empty scans only, the largest scan and the workgroups at 1, 256 and 257 points, and every planner's
// slices against the cutter's.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "check.hpp"
#include "elevation_host.hpp"
#include "occupancy_host.hpp"
#include "vote_host.hpp"

using namespace lom;
using assemble::Launch;

static bool same(const Launch &a, const Launch &b)
{
    return a.first == b.first && a.count == b.count && a.max_n == b.max_n && a.grid_x == b.grid_x;
}

// the definition, scan by scan: a launch is the next `per` scans; it is listed when one of them has a point
static std::vector<Launch> expected(const std::vector<uint32_t> &n, uint32_t per)
{
    std::vector<Launch> out;
    for (size_t first = 0; first < n.size(); first += per) {
        const size_t end = std::min(n.size(), first + per);
        const uint32_t max_n = *std::max_element(n.begin() + first, n.begin() + end);
        if (max_n) out.push_back(Launch{(uint32_t)first, (uint32_t)(end - first), max_n, (max_n + 255u) / 256u});
    }
    return out;
}

int main()
{
    // sizes 1, 256 and 257 (one workgroup, one full, two), empty scans between them, two empty ones side by side, one last
    const std::vector<uint32_t> sizes = {1, 0, 256, 257, 0, 0, 300, 0, 0, 0, 255, 0};
    std::vector<assemble::ScanEntry> table;
    std::vector<int64_t> ids;
    uint64_t at = 0;
    for (uint32_t n : sizes) {
        ids.push_back((int64_t)table.size());
        table.push_back({at, n});
        at += n;
    }
    const std::vector<lom_graph_pose> poses(sizes.size(), lom_graph_pose{{0, 0, 0}, {1, 0, 0, 0}});
    const lom_vote_params vp = {0.1f, 1.f, 50.f, 0.f, 1u, 1u};
    const lom_occupancy_geometry og = {0.5f, -8.f, -8.f, 32u, 32u};
    const lom_occupancy_ray_params op = {-1.f, 1.f, 0.25f, 0.5f, 20.f};
    const lom_elevation_geometry eg = {0.5f, -8.f, -8.f, 32u, 32u, 0.f};
    const lom_elevation_point_params ep = {-1.f, 1.f, 0.5f, 20.f};
    std::string why;

    for (size_t count : {sizes.size(), (size_t)6, (size_t)2, (size_t)1, (size_t)0}) {
        const std::vector<uint32_t> n(sizes.begin(), sizes.begin() + count);
        assemble::Plan scans;
        CHECK(assemble::plan(table.data(), table.size(), ids.data(), poses.data(), count, scans, why) == LOM_OK);
        for (uint32_t cap : {1u, 2u, 3u, 0u}) {  // 0: the planner's default
            // the cutter itself (its cap is never 0: the default of the votes stands in)
            const uint32_t per = cap ? cap : vote::kSliceScans;
            const std::vector<Launch> want = expected(n, per), got = assemble::cut_launches(scans, per);
            CHECK(got.size() == want.size());
            for (size_t k = 0; k < got.size() && k < want.size(); k++) CHECK(same(got[k], want[k]));
            // the three planners, each at its own cap: its slices are the definition's, and so the cutter's
            vote::Plan v;
            CHECK(vote::plan(table.data(), table.size(), ids.data(), poses.data(), count, &vp, cap, v, why) == LOM_OK);
            const std::vector<Launch> cv = assemble::cut_launches(v.scans, per);
            CHECK(v.slices.size() == want.size() && cv.size() == want.size());
            for (size_t k = 0; k < want.size() && k < v.slices.size() && k < cv.size(); k++)
                CHECK(same(v.slices[k], want[k]) && same(v.slices[k], cv[k]));
            occupancy::Plan o;
            CHECK(occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), count, og, &op, cap, o, why) == LOM_OK);
            const std::vector<Launch> co = assemble::cut_launches(o.scans, occupancy::slice_scans(og, cap));
            CHECK(occupancy::slice_scans(og, cap) == (cap ? cap : occupancy::kSliceScans) && occupancy::kSliceScans == vote::kSliceScans);
            CHECK(o.slices.size() == want.size() && co.size() == want.size());
            for (size_t k = 0; k < want.size() && k < o.slices.size() && k < co.size(); k++)
                CHECK(same(o.slices[k], want[k]) && same(o.slices[k], co[k]) && !o.slices[k].box.empty());
            elevation::Plan e;
            CHECK(elevation::plan(table.data(), table.size(), ids.data(), poses.data(), count, eg, &ep, cap, e, why) == LOM_OK);
            const uint32_t eper = cap ? cap : elevation::kScansPerLaunch;
            const std::vector<Launch> we = expected(n, eper), ce = assemble::cut_launches(e.scans, eper);
            CHECK(e.launches.size() == we.size() && ce.size() == we.size());
            for (size_t k = 0; k < we.size() && k < e.launches.size() && k < ce.size(); k++)
                CHECK(same(e.launches[k], we[k]) && same(e.launches[k], ce[k]));
        }
    }
    // the figures spelled out: cap 1 lists the five scans with points; cap 2 drops the pairs (4, 5) and (8, 9)
    assemble::Plan scans;
    CHECK(assemble::plan(table.data(), table.size(), ids.data(), poses.data(), sizes.size(), scans, why) == LOM_OK);
    const std::vector<Launch> one = assemble::cut_launches(scans, 1), two = assemble::cut_launches(scans, 2),
                              all = assemble::cut_launches(scans, 64);
    CHECK(one.size() == 5 && same(one[0], Launch{0, 1, 1, 1}) && same(one[1], Launch{2, 1, 256, 1}) &&
          same(one[2], Launch{3, 1, 257, 2}) && same(one[3], Launch{6, 1, 300, 2}) && same(one[4], Launch{10, 1, 255, 1}));
    CHECK(two.size() == 4 && same(two[0], Launch{0, 2, 1, 1}) && same(two[1], Launch{2, 2, 257, 2}) &&
          same(two[2], Launch{6, 2, 300, 2}) && same(two[3], Launch{10, 2, 255, 1}));
    CHECK(all.size() == 1 && same(all[0], Launch{0, 12, 300, 2}));
    CHECK(assemble::cut_launches(assemble::Plan(), 1).empty() && assemble::cut_launches(assemble::Plan(), 64).empty());
    return check_done();
}
