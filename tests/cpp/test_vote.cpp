// The C++ side of the scan votes, two programs from one file:
//  - -DVOTE_HOST_STANDALONE (tests/test_vote_cpp.py): csrc/vote_host.cpp and csrc/assemble_host.cpp compiled into this
//    program under -fsanitize=address,undefined: the refusals of the planner, the slices of 1, 63, 64, 65 and 129 scans
//    and of a capped slice, the descriptor offsets of the slices, the origin's verdict and the step bound;
//  - default (tests/test_vote_gpu.py, needs a device): the mirror VoxelGrid::carveScans / scanVotes against the library
//    on a small map; prints the size it leaves and the voxels erased.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "check.hpp"

#ifdef VOTE_HOST_STANDALONE
#include "vote_host.hpp"

using namespace lom::vote;
using lom::assemble::ScanEntry;

int main()
{
    const lom_graph_pose ident = {{0, 0, 0}, {1, 0, 0, 0}};
    const lom_vote_params good = {0.4f, 4.f, 60.f, 0.75f, 3u, 2u};
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    Plan plan;
    std::string why;
    // parameters
    CHECK(params_ok(&good) && !params_ok(nullptr));
    {
        lom_vote_params p = good;
        p.clearance = 0.f, p.margin = 0.f, p.free_per_seen = 0u;
        CHECK(params_ok(&p));
        for (float v : {-0.1f, nan, inf}) {
            p = good, p.margin = v;
            CHECK(!params_ok(&p));
            p = good, p.clearance = v;
            CHECK(!params_ok(&p));
        }
        for (float v : {0.f, -1.f, nan, inf, 60.f, 61.f}) {
            p = good, p.min_range = v;
            CHECK(!params_ok(&p));
        }
        for (float v : {4.f, 1.f, nan, inf}) {
            p = good, p.max_range = v;
            CHECK(!params_ok(&p));
        }
        p = good, p.min_free_scans = 0u;
        CHECK(!params_ok(&p));
        p = good, p.free_per_seen = 0xFFFFFFFFu, p.min_free_scans = 0xFFFFFFFFu;
        CHECK(params_ok(&p));
    }
    // empty input: nothing is read, nothing is launched
    CHECK(lom::vote::plan(nullptr, 0, nullptr, nullptr, 0, &good, 0, plan, why) == LOM_OK && plan.slices.empty() && plan.scans.scans.empty());
    // bad parameters, ids and poses are refused, and nothing is kept
    std::vector<ScanEntry> table = {{0, 300}, {300, 0}, {300, 40}, {340, 700}};
    {
        std::vector<int64_t> ids = {0, 3};
        std::vector<lom_graph_pose> poses(2, ident);
        lom_vote_params bad = good;
        bad.min_free_scans = 0;
        CHECK(lom::vote::plan(table.data(), table.size(), ids.data(), poses.data(), 2, &bad, 0, plan, why) == LOM_ERR_ARG);
        CHECK(plan.slices.empty() && plan.scans.scans.empty() && !why.empty());
        CHECK(lom::vote::plan(table.data(), table.size(), ids.data(), poses.data(), 2, nullptr, 0, plan, why) == LOM_ERR_ARG);
        ids[1] = 4;
        CHECK(lom::vote::plan(table.data(), table.size(), ids.data(), poses.data(), 2, &good, 0, plan, why) == LOM_ERR_ARG);
        ids[1] = -1;
        CHECK(lom::vote::plan(table.data(), table.size(), ids.data(), poses.data(), 2, &good, 0, plan, why) == LOM_ERR_ARG);
        ids[1] = 3, poses[0].q_wxyz[0] = 0.0;
        CHECK(lom::vote::plan(table.data(), table.size(), ids.data(), poses.data(), 2, &good, 0, plan, why) == LOM_ERR_ARG);
        poses[0] = ident, poses[1].t[2] = std::numeric_limits<double>::infinity();
        CHECK(lom::vote::plan(table.data(), table.size(), ids.data(), poses.data(), 2, &good, 0, plan, why) == LOM_ERR_ARG);
        CHECK(lom::vote::plan(table.data(), table.size(), nullptr, poses.data(), 2, &good, 0, plan, why) == LOM_ERR_ARG);
        CHECK(plan.slices.empty());
    }
    // slices: 1, 63, 64, 65, 129 scans at the full width, ragged sizes, every slice's largest scan and descriptor offset
    for (size_t K : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)129}) {
        std::vector<int64_t> ids(K);
        std::vector<lom_graph_pose> poses(K, ident);
        for (size_t k = 0; k < K; k++) {
            ids[k] = (int64_t)(k % table.size());
            poses[k].t[0] = (double)k;
        }
        CHECK(lom::vote::plan(table.data(), table.size(), ids.data(), poses.data(), K, &good, 0, plan, why) == LOM_OK);
        CHECK(plan.scans.scans.size() == K && plan.slices.size() == (K + 63) / 64);
        size_t next = 0;
        for (const Slice &s : plan.slices) {
            CHECK(s.first == next && s.count == (K - next < 64 ? K - next : 64) && s.count >= 1 && s.count <= kSliceScans);
            uint32_t max_n = 0;
            for (uint32_t k = 0; k < s.count; k++) {
                const lom::assemble::AsmScan &d = plan.scans.scans[s.first + k];
                CHECK(d.n == table[(size_t)ids[s.first + k]].n && d.t[0] == (double)(s.first + k));
                CHECK(d.n == 0 || d.src == table[(size_t)ids[s.first + k]].offset);
                max_n = d.n > max_n ? d.n : max_n;
            }
            CHECK(s.max_n == max_n && s.grid_x == (max_n + 255) / 256 && s.grid_x >= 1);
            next += s.count;
        }
        CHECK(next == K);
    }
    // a capped slice (LOM_OPT_TEST_VOTE_SLICE_MAX); a slice of empty scans only is not launched; a cap beyond 64 is 64
    {
        std::vector<int64_t> ids = {0, 3, 1, 1, 1, 2, 1};
        std::vector<lom_graph_pose> poses(ids.size(), ident);
        CHECK(lom::vote::plan(table.data(), table.size(), ids.data(), poses.data(), ids.size(), &good, 1, plan, why) == LOM_OK);
        CHECK(plan.slices.size() == 3 && plan.slices[0].first == 0 && plan.slices[1].first == 1 && plan.slices[2].first == 5);
        CHECK(plan.slices[1].grid_x == 3 && plan.slices[2].max_n == 40 && plan.slices[2].count == 1);
        CHECK(lom::vote::plan(table.data(), table.size(), ids.data(), poses.data(), ids.size(), &good, 3, plan, why) == LOM_OK);
        CHECK(plan.slices.size() == 2 && plan.slices[0].count == 3 && plan.slices[0].max_n == 700 && plan.slices[1].first == 3 &&
              plan.slices[1].count == 3 && plan.slices[1].max_n == 40);  // (scan 6, alone and empty, is no slice)
        CHECK(lom::vote::plan(table.data(), table.size(), ids.data(), poses.data(), ids.size(), &good, 1000, plan, why) == LOM_OK);
        CHECK(plan.slices.size() == 1 && plan.slices[0].count == 7);
        ids = {1, 1};
        CHECK(lom::vote::plan(table.data(), table.size(), ids.data(), poses.data(), 2, &good, 0, plan, why) == LOM_OK);
        CHECK(plan.slices.empty() && plan.scans.scans.size() == 2 && plan.scans.points_in == 0);
    }
    // the origin's verdict: f32 t / v inside (-2^20, 2^20)
    {
        lom::assemble::AsmScan d{};
        d.t[0] = 1.0, d.t[1] = -2.0, d.t[2] = 524287.9;
        CHECK(origin_ok(d, 0.5f));
        d.t[2] = 524288.0;
        CHECK(!origin_ok(d, 0.5f));
        d.t[2] = 0.0, d.t[1] = -524288.0;
        CHECK(!origin_ok(d, 0.5f));
        d.t[1] = 0.0, d.t[0] = 1e300;  // rounds to +inf in f32
        CHECK(!origin_ok(d, 0.5f));
    }
    // the step bound is the carve's
    CHECK(max_steps(60.f, 0.5f) == 3u * 122u && max_steps(6.f, 0.2f) == 3u * 32u && max_steps(3.4e38f, 0.5f) == 3u * 2097154u);
    return check_done();
}
#else
#include "lidar_odometry_amd.hpp"

int main()
{
    if (lom_device_count() < 1) {
        std::printf("no device\n");
        return 2;
    }
    // a block of 9 x 9 x 9 voxels, one point each; three scans of 12 rays from three origins through it
    const float V = 0.5f;
    lom::PointCloud<lom::PointNormal> map_cloud;
    for (int ix = -4; ix <= 4; ix++)
        for (int iy = -4; iy <= 4; iy++)
            for (int iz = -4; iz <= 4; iz++) {
                const auto at = [&](int c) { return (float)c * V + 0.125f * (float)((c > 0) - (c < 0)); };
                map_cloud.points.push_back(lom::PointNormal(at(ix), at(iy), at(iz)));
            }
    lom::VoxelGrid grid(V, 4);
    grid.addCloud(map_cloud);
    const size_t before = grid.size();
    CHECK(before == 729);
    lom::ScanArchive a;
    lom::PointCloud<lom::PointNormal> scan;
    for (int k = 0; k < 12; k++) {
        lom::PointNormal p(2.1f, 0.3f * (float)k - 2.0f, 0.2f * (float)k - 1.0f);
        p.normal_x = -1.f;
        scan.points.push_back(p);
    }
    CHECK(a.add(scan) == 0);
    const std::vector<int64_t> ids = {0, 0, 0};
    const std::vector<lom::GraphPose> poses = {{{0.1, 0.1, 0.1}, {1, 0, 0, 0}}, {{0.1, 0.3, 0.1}, {1, 0, 0, 0}}, {{0.1, 0.1, 0.3}, {1, 0, 0, 0}}};
    const lom::VoteParams p = {0.25f, 0.5f, 6.f, 0.3f, 2u, 1u};
    std::vector<uint32_t> free_votes, seen_votes;
    grid.scanVotes(a, ids, poses, p, free_votes, seen_votes);
    CHECK(free_votes.size() == before && seen_votes.size() == before && grid.size() == before);
    size_t want = 0;
    for (size_t i = 0; i < before; i++) want += free_votes[i] >= 2u && free_votes[i] >= seen_votes[i];
    const lom::VoteStats st = grid.carveScans(a, ids, poses, p);
    CHECK(st.scans == 3 && st.rays_walked + st.rays_skipped == 36 && st.voxels_erased == want && want > 0);
    CHECK(grid.size() == before - want);
    bool threw = false;
    try {
        grid.carveScans(a, {1}, {poses[0]}, p);
    } catch (const lom::Error &e) {
        threw = e.code == LOM_ERR_ARG;
    }
    CHECK(threw && grid.size() == before - want);
    if (check_done()) return 1;
    std::printf("%zu %u\n", grid.size(), (unsigned)st.voxels_erased);
    return 0;
}
#endif
