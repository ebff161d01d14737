// The C++ side of the occupancy grid, two programs from one file:
//  - -DOCCUPANCY_HOST_STANDALONE (tests/test_occupancy_cpp.py): csrc/occupancy_host.cpp and csrc/assemble_host.cpp compiled
//    into this program under -fsanitize=address,undefined: every refusal of the planner, the slices of 1, 63, 64, 65 and
//    129 scans and of a capped slice, bounding boxes clipped at the grid's edges and for origins outside it, the step
//    bound and the slice size the scratch budget admits;
//  - default (tests/test_occupancy_gpu.py, needs a device): the mirror lom::OccupancyGrid against the library on a small
//    grid; prints the cells it classifies free and occupied.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "check.hpp"

#ifdef OCCUPANCY_HOST_STANDALONE
#include "occupancy_host.hpp"

using namespace lom::occupancy;
using lom::assemble::ScanEntry;

int main()
{
    const lom_graph_pose ident = {{0, 0, 0}, {1, 0, 0, 0}};
    const lom_occupancy_geometry geo = {0.25f, -70.f, -15.f, 584u, 120u};
    const lom_occupancy_ray_params good = {-1.5f, 0.6f, 0.f, 2.f, 60.f};
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    Plan plan;
    std::string why;
    // geometry
    CHECK(geometry_ok(&geo) && !geometry_ok(nullptr));
    {
        lom_occupancy_geometry g = geo;
        g.width = 16384u, g.height = 1u;
        CHECK(geometry_ok(&g));
        g.width = 16385u;
        CHECK(!geometry_ok(&g));
        g = geo, g.height = 0u;
        CHECK(!geometry_ok(&g));
        g = geo, g.width = 0u;
        CHECK(!geometry_ok(&g));
        for (float bad : {0.f, -0.25f, nan, inf}) {
            g = geo, g.resolution = bad;
            CHECK(!geometry_ok(&g));
        }
        for (float bad : {nan, inf, -inf}) {
            g = geo, g.origin_x = bad;
            CHECK(!geometry_ok(&g));
            g = geo, g.origin_y = bad;
            CHECK(!geometry_ok(&g));
        }
    }
    // ray parameters
    CHECK(params_ok(&good, 0.25f) && !params_ok(nullptr, 0.25f));
    {
        lom_occupancy_ray_params p = good;
        for (float bad : {0.f, 0.1f, nan, -inf}) {
            p = good, p.z_lo = bad;
            CHECK(!params_ok(&p, 0.25f));
        }
        for (float bad : {0.f, -0.1f, nan, inf}) {
            p = good, p.z_hi = bad;
            CHECK(!params_ok(&p, 0.25f));
        }
        for (float bad : {-0.1f, nan, inf}) {
            p = good, p.margin = bad;
            CHECK(!params_ok(&p, 0.25f));
        }
        for (float bad : {0.f, -1.f, nan, 60.f, 61.f}) {
            p = good, p.min_range = bad;
            CHECK(!params_ok(&p, 0.25f));
        }
        for (float bad : {nan, inf, 2.f, 1.f}) {
            p = good, p.max_range = bad;
            CHECK(!params_ok(&p, 0.25f));
        }
        p = good, p.max_range = 1048576.f * 0.25f;  // max_range / resolution == 2^20: the last one in
        CHECK(params_ok(&p, 0.25f));
        p.max_range = 1048577.f * 0.25f;
        CHECK(!params_ok(&p, 0.25f));
        p = good, p.margin = 100.f;  // a margin beyond the range is legal: nothing is walked
        CHECK(params_ok(&p, 0.25f));
    }
    // the rule
    {
        lom_occupancy_rule r = {3u, 2u, 1u};
        CHECK(rule_ok(&r) && !rule_ok(nullptr));
        r.free_per_seen = 0u;
        CHECK(rule_ok(&r));
        r.min_free_scans = 0u;
        CHECK(!rule_ok(&r));
        r.min_free_scans = 1u, r.min_seen_scans = 0u;
        CHECK(!rule_ok(&r));
    }
    // the step bound
    CHECK(max_steps(60.f, 0.25f) == 2u * (240u + 2u));
    CHECK(max_steps(60.f, 0.1f) == 2u * (600u + 2u));
    CHECK(max_steps(0.3f, 0.25f) == 2u * (2u + 2u));
    CHECK(max_steps(262144.f, 0.25f) == 2u * (1048576u + 2u));
    // the slice size under the scratch budget
    {
        CHECK(words_per_row(584u) == 19u && words_per_row(32u) == 1u && words_per_row(33u) == 2u && map_words(geo) == 120u * 19u);
        CHECK(slice_scans(geo, 0) == 64u && slice_scans(geo, 7) == 7u && slice_scans(geo, 1) == 1u && slice_scans(geo, 64) == 64u);
        lom_occupancy_geometry big = {0.25f, 0.f, 0.f, 16384u, 16384u};  // 2 x 32 MiB per scan: four scans in 256 MiB
        CHECK(slice_scans(big, 0) == 4u && slice_scans(big, 3) == 3u && slice_scans(big, 64) == 4u);
        lom_occupancy_geometry mid = {0.25f, 0.f, 0.f, 4096u, 4096u};    // 2 x 2 MiB per scan: 64
        CHECK(slice_scans(mid, 0) == 64u);
        lom_occupancy_geometry wide = {0.25f, 0.f, 0.f, 16384u, 4096u};  // 2 x 8 MiB per scan: 16
        CHECK(slice_scans(wide, 0) == 16u);
        CHECK(kScratchBudget / (map_words(big) * 8) >= 1);  // "at least 1" never has to bind at the largest grid
    }
    // start cells: floor, not truncation; the range verdict
    {
        lom::assemble::AsmScan d = {};
        int32_t c[2] = {7, 7};
        d.t[0] = -70.0, d.t[1] = -15.0;
        CHECK(origin_cell(d, geo, c) && c[0] == 0 && c[1] == 0);
        d.t[0] = -70.01, d.t[1] = -15.26;
        CHECK(origin_cell(d, geo, c) && c[0] == -1 && c[1] == -2);
        d.t[0] = 75.99, d.t[1] = 14.99;
        CHECK(origin_cell(d, geo, c) && c[0] == 583 && c[1] == 119);
        d.t[0] = 0.25 * 1073741823.0 - 70.0 - 64.0, d.t[1] = 0.0;  // (f32 spacing here is 32: well inside 2^30 cells)
        CHECK(origin_cell(d, geo, c) && c[0] < (1 << 30));
        d.t[0] = 0.25 * 1073741824.0 + 1000.0;
        CHECK(!origin_cell(d, geo, c));
        d.t[0] = -0.25 * 1073741824.0 - 1000.0;
        CHECK(!origin_cell(d, geo, c));
        d.t[0] = 1e300;  // rounds to +inf in f32
        CHECK(!origin_cell(d, geo, c));
        d.t[0] = 0.0, d.t[1] = -1e300;
        CHECK(!origin_cell(d, geo, c));
    }
    // bounding boxes: reach = ceil(max_range / r) + 2 cells either side, clipped
    {
        int32_t c[2] = {300, 60};
        Box b = box_of(c, 10.f, geo);  // 40 + 2 cells
        CHECK(b.x0 == 258u && b.x1 == 343u && b.y0 == 18u && b.y1 == 103u && !b.empty());
        b = box_of(c, 60.f, geo);      // 242 cells: clipped in y on both sides and in x on neither
        CHECK(b.x0 == 58u && b.x1 == 543u && b.y0 == 0u && b.y1 == 120u);
        c[0] = 0, c[1] = 0;            // the grid's corner
        b = box_of(c, 10.f, geo);
        CHECK(b.x0 == 0u && b.x1 == 43u && b.y0 == 0u && b.y1 == 43u);
        c[0] = 583, c[1] = 119;
        b = box_of(c, 10.f, geo);
        CHECK(b.x0 == 541u && b.x1 == 584u && b.y0 == 77u && b.y1 == 120u);
        c[0] = -20, c[1] = 60;         // an origin outside the grid whose rays reach into it
        b = box_of(c, 10.f, geo);
        CHECK(b.x0 == 0u && b.x1 == 23u && !b.empty());
        c[0] = -50;                    // ... and one whose rays do not
        b = box_of(c, 10.f, geo);
        CHECK(b.empty());
        c[0] = 700;
        b = box_of(c, 10.f, geo);
        CHECK(b.empty() && b.x0 <= 584u && b.x1 <= 584u);
        c[0] = (1 << 30) - 1, c[1] = -(1 << 30) + 1;  // the extremes of the range: no overflow
        b = box_of(c, 262144.f, geo);
        CHECK(b.empty());
        const Box e = {0, 0, 0, 0}, x = {5, 6, 9, 8}, y = {1, 7, 6, 20};
        Box u = box_union(e, x);
        CHECK(u.x0 == 5u && u.y1 == 8u);
        u = box_union(x, e);
        CHECK(u.x0 == 5u && u.y1 == 8u);
        u = box_union(x, y);
        CHECK(u.x0 == 1u && u.y0 == 6u && u.x1 == 9u && u.y1 == 20u);
    }
    // nothing to do
    CHECK(lom::occupancy::plan(nullptr, 0, nullptr, nullptr, 0, geo, &good, 0, plan, why) == LOM_OK && plan.slices.empty() && plan.scans.scans.empty());
    // refusals: everything is checked before anything is kept
    {
        std::vector<ScanEntry> table = {{0, 10}, {10, 0}, {10, 300}};
        std::vector<int64_t> ids = {0, 2};
        std::vector<lom_graph_pose> poses = {ident, ident};
        lom_occupancy_ray_params bad = good;
        bad.z_lo = 0.f;
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), 2, geo, &bad, 0, plan, why) == LOM_ERR_ARG);
        CHECK(plan.slices.empty() && plan.scans.scans.empty() && plan.cells.empty() && !why.empty());
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), 2, geo, nullptr, 0, plan, why) == LOM_ERR_ARG);
        ids[1] = 3;
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), 2, geo, &good, 0, plan, why) == LOM_ERR_ARG);
        ids[1] = -1;
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), 2, geo, &good, 0, plan, why) == LOM_ERR_ARG);
        ids[1] = 2, poses[1].q_wxyz[0] = 0.0;
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), 2, geo, &good, 0, plan, why) == LOM_ERR_ARG);
        poses[1] = ident, poses[0].t[2] = (double)nan;
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), 2, geo, &good, 0, plan, why) == LOM_ERR_ARG);
        poses[0] = ident;
        CHECK(lom::occupancy::plan(table.data(), table.size(), nullptr, poses.data(), 2, geo, &good, 0, plan, why) == LOM_ERR_ARG);
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), nullptr, 2, geo, &good, 0, plan, why) == LOM_ERR_ARG);
        CHECK(plan.slices.empty());
        // an origin beyond 2^30 cells: LOM_ERR_RANGE, even where its scan is empty, and nothing is kept
        ids[1] = 1, poses[1].t[0] = 1e12;
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), 2, geo, &good, 0, plan, why) == LOM_ERR_RANGE);
        CHECK(plan.slices.empty() && plan.scans.scans.empty() && plan.cells.empty() && why.find("scan 1") != std::string::npos);
        poses[1].t[0] = 1e8;  // far outside the grid, inside the range: legal, with an empty box
        ids[1] = 2;
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), 2, geo, &good, 1, plan, why) == LOM_OK);
        CHECK(plan.slices.size() == 2 && !plan.slices[0].box.empty() && plan.slices[1].box.empty() && plan.cells.size() == 4);
        CHECK(plan.cells[0] == 280 && plan.cells[1] == 60);
    }
    // slices of 1, 63, 64, 65 and 129 scans
    for (size_t K : {size_t(1), size_t(63), size_t(64), size_t(65), size_t(129)}) {
        std::vector<ScanEntry> table;
        uint64_t off = 0;
        for (size_t k = 0; k < K; k++) {
            const uint32_t n = (uint32_t)(1 + (k * 37) % 600);
            table.push_back({off, n});
            off += n;
        }
        std::vector<int64_t> ids(K);
        std::vector<lom_graph_pose> poses(K, ident);
        for (size_t k = 0; k < K; k++) ids[k] = (int64_t)(K - 1 - k), poses[k].t[0] = (double)k * 0.25 - 10.0;
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), K, geo, &good, 0, plan, why) == LOM_OK);
        CHECK(plan.scans.scans.size() == K && plan.cells.size() == 2 * K && plan.slices.size() == (K + 63) / 64);
        size_t next = 0;
        for (const Slice &s : plan.slices) {
            CHECK(s.first == next && s.count == (K - next < 64 ? K - next : 64) && s.count >= 1 && s.count <= kSliceScans);
            uint32_t max_n = 0;
            Box want = {0, 0, 0, 0};
            for (uint32_t k = 0; k < s.count; k++) {
                const lom::assemble::AsmScan &d = plan.scans.scans[s.first + k];
                CHECK(d.n == table[(size_t)ids[s.first + k]].n && d.src == table[(size_t)ids[s.first + k]].offset);
                CHECK(plan.cells[2 * (s.first + k)] == 240 + (int32_t)(s.first + k) && plan.cells[2 * (s.first + k) + 1] == 60);
                max_n = d.n > max_n ? d.n : max_n;
                want = box_union(want, box_of(&plan.cells[2 * (s.first + k)], good.max_range, geo));
            }
            CHECK(s.max_n == max_n && s.grid_x == (max_n + 255) / 256 && s.grid_x >= 1);
            CHECK(s.box.x0 == want.x0 && s.box.x1 == want.x1 && s.box.y0 == want.y0 && s.box.y1 == want.y1);
            // the box holds origin +- max_range of every scan, and lies in the grid
            CHECK(s.box.x1 <= geo.width && s.box.y1 <= geo.height && s.box.y0 == 0u && s.box.y1 == 120u);
            const int32_t lo = 240 + (int32_t)s.first - 240, hi = 240 + (int32_t)(s.first + s.count - 1) + 241;  // 60 m = 240 cells
            CHECK((int32_t)s.box.x0 <= (lo < 0 ? 0 : lo) && (int32_t)s.box.x1 >= (hi > 584 ? 584 : hi));
            next += s.count;
        }
        CHECK(next == K);
    }
    // a capped slice; a slice of empty scans only is not listed, and an empty scan adds nothing to a box
    {
        std::vector<ScanEntry> table = {{0, 0}, {0, 600}, {600, 40}, {640, 0}};
        std::vector<int64_t> ids = {0, 1, 3, 3, 0, 2};
        std::vector<lom_graph_pose> poses(ids.size(), ident);
        poses[2].t[0] = 1e6;  // an empty scan far away
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), ids.size(), geo, &good, 1, plan, why) == LOM_OK);
        CHECK(plan.slices.size() == 2 && plan.slices[0].first == 1 && plan.slices[1].first == 5);
        CHECK(plan.slices[0].grid_x == 3 && plan.slices[1].max_n == 40 && plan.slices[1].count == 1);
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), ids.size(), geo, &good, 3, plan, why) == LOM_OK);
        CHECK(plan.slices.size() == 2 && plan.slices[0].count == 3 && plan.slices[0].max_n == 600 && plan.slices[1].first == 3);
        CHECK(plan.slices[0].box.x1 == 523u);  // 280 + 242 + 1: the far, empty scan is not in it
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), ids.size(), geo, &good, 64, plan, why) == LOM_OK);
        CHECK(plan.slices.size() == 1 && plan.slices[0].count == 6);
        CHECK(lom::occupancy::plan(table.data(), table.size(), ids.data(), poses.data(), 1, geo, &good, 0, plan, why) == LOM_OK);
        CHECK(plan.slices.empty() && plan.scans.scans.size() == 1 && plan.scans.points_in == 0);
    }
    return check_done();
}

#else
#include "lidar_odometry_amd.hpp"

int main()
{
    try {
        const lom::OccupancyGeometry geo = {0.5f, -4.f, -3.f, 45u, 37u};
        const lom::OccupancyRayParams prm = {-1.f, 1.f, 0.f, 0.5f, 12.f};
        const lom::OccupancyRule rule = {1u, 1u, 1u};
        lom::OccupancyGrid grid(geo);
        CHECK(grid.cells() == 45u * 37u && grid.geometry().width == 45u);
        lom::PointCloud<lom::PointXYZ> cloud;
        for (int k = 0; k < 12; k++) {
            lom::PointXYZ p;
            p.x = 6.1f, p.y = (float)(0.3 * k - 2.0), p.z = (float)(0.05 * k - 0.3);  // (f64, one rounding: as the Python side)
            cloud.points.push_back(p);
        }
        lom::ScanArchive archive;
        CHECK(archive.addPoints(cloud) == 0 && archive.scanSize(0) == 12);
        const lom_graph_pose a = {{0.1, 0.1, 0.1}, {1, 0, 0, 0}}, b = {{0.1, 0.3, 0.1}, {2, 0, 0, 0.1}};
        lom::OccupancyStats st = grid.integrate(archive, {0, 0}, {a, b}, prm);
        CHECK(st.scans == 2 && st.rays_walked + st.rays_skipped == 24 && st.rays_walked == 24 && st.endpoints_marked > 0);
        std::vector<uint32_t> free1, seen1, free2, seen2;
        grid.counts(free1, seen1);
        lom::OccupancySummary sm;
        const std::vector<int8_t> cls = grid.classify(rule, &sm);
        CHECK(cls.size() == grid.cells() && sm.cells_free + sm.cells_occupied + sm.cells_unknown == grid.cells());
        CHECK(sm.cells_free > 20 && sm.cells_occupied > 2);
        // the cloud form on the same points gives the same counts
        grid.clear();
        grid.counts(free2, seen2);
        for (uint32_t v : free2) CHECK(v == 0u);
        grid.integrateCloud(cloud, a, prm);
        grid.integrateCloud(cloud, b, prm);
        grid.counts(free2, seen2);
        CHECK(free1 == free2 && seen1 == seen2);
        bool threw = false;
        try {
            lom::OccupancyRayParams bad = prm;
            bad.z_lo = 0.f;
            grid.integrateCloud(cloud, a, bad);
        } catch (const lom::Error &) {
            threw = true;
        }
        CHECK(threw);
        if (check_done()) return 1;
        std::printf("%llu %llu\n", (unsigned long long)sm.cells_free, (unsigned long long)sm.cells_occupied);
        return 0;
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
}
#endif
