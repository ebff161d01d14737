// The C++ side of the elevation grid, two programs from one file:
//  - -DELEVATION_HOST_STANDALONE (tests/test_elevation_cpp.py): csrc/elevation_host.cpp and csrc/assemble_host.cpp compiled
//    into this program under -fsanitize=address,undefined: every value range, the origins' range verdict, every refusal of
//    the planner and its order, the launches of 1, 2, 3 and 7 scans under a cap, empty scans, an empty call;
//  - default (tests/test_elevation_gpu.py, needs a device): the mirror lom::ElevationGrid against the library on a small
//    grid; prints the cells it finds unknown, lethal and costed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "check.hpp"

#ifdef ELEVATION_HOST_STANDALONE
#include "elevation_host.hpp"

using namespace lom::elevation;
using lom::assemble::ScanEntry;

int main()
{
    const lom_graph_pose ident = {{0, 0, 0}, {1, 0, 0, 0}};
    const lom_elevation_geometry geo = {0.25f, -2.f, -6.f, 96u, 48u, 0.5f};
    const lom_elevation_point_params good = {-2.5f, 0.8f, 0.5f, 8.f};
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    Plan pl;
    std::string why;
    // geometry
    CHECK(geometry_ok(&geo) && !geometry_ok(nullptr));
    {
        lom_elevation_geometry g = geo;
        g.width = 8192u, g.height = 1u;
        CHECK(geometry_ok(&g));
        g.width = 8193u;
        CHECK(!geometry_ok(&g));
        g = geo, g.height = 8193u;
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
            g = geo, g.z_ref = bad;
            CHECK(!geometry_ok(&g));
        }
        g = geo, g.z_ref = -1.0e30f;
        CHECK(geometry_ok(&g));
    }
    // point parameters
    CHECK(point_params_ok(&good, 0.25f) && !point_params_ok(nullptr, 0.25f));
    {
        lom_elevation_point_params p = good;
        for (float bad : {0.f, 0.1f, nan, -inf}) {
            p = good, p.z_lo = bad;
            CHECK(!point_params_ok(&p, 0.25f));
        }
        for (float bad : {0.f, -0.1f, nan, inf}) {
            p = good, p.z_hi = bad;
            CHECK(!point_params_ok(&p, 0.25f));
        }
        for (float bad : {0.f, -1.f, nan, 8.f, 9.f}) {
            p = good, p.min_range = bad;
            CHECK(!point_params_ok(&p, 0.25f));
        }
        for (float bad : {0.4f, nan, inf}) {
            p = good, p.max_range = bad;
            CHECK(!point_params_ok(&p, 0.25f));
        }
        p = good, p.max_range = 262144.f;  // 2^20 cells exactly
        CHECK(point_params_ok(&p, 0.25f));
        p.max_range = 262145.f;
        CHECK(!point_params_ok(&p, 0.25f));
    }
    // layer and cost parameters
    {
        lom_elevation_layer_params l = {1u, 1u};
        CHECK(layer_params_ok(&l) && !layer_params_ok(nullptr));
        l.window = 4u;
        CHECK(layer_params_ok(&l));
        l.window = 5u;
        CHECK(!layer_params_ok(&l));
        l.window = 0u;
        CHECK(!layer_params_ok(&l));
        l.window = 2u, l.min_points = 0u;
        CHECK(!layer_params_ok(&l));
        l.min_points = 0xFFFFFFFFu;
        CHECK(layer_params_ok(&l));
        const lom_elevation_cost_params c = {0.35f, 0.25f, 0.1f, 0.5f};
        CHECK(cost_params_ok(&c) && !cost_params_ok(nullptr));
        for (int field = 0; field < 4; field++)
            for (float bad : {0.f, -1.f, nan, inf}) {
                lom_elevation_cost_params b = c;
                (field == 0 ? b.max_slope : field == 1 ? b.max_step : field == 2 ? b.max_rough : b.max_span) = bad;
                CHECK(!cost_params_ok(&b));
            }
    }
    // the origins' start cells and their verdict
    {
        lom::assemble::AsmScan d{};
        int32_t c[2] = {7, 7};
        d.t[0] = -2.0, d.t[1] = -6.0;
        CHECK(origin_cell(d, geo, c) && c[0] == 0 && c[1] == 0);
        d.t[0] = -2.0000001, d.t[1] = 5.99;  // rounds to -2 in f32; y: (5.99f + 6) / 0.25 = 47.96
        CHECK(origin_cell(d, geo, c) && c[0] == 0 && c[1] == 47);
        d.t[0] = -2.26, d.t[1] = 100.0;      // left of the origin: floor, not truncation; outside the grid is legal
        CHECK(origin_cell(d, geo, c) && c[0] == -2 && c[1] == 424);
        d.t[0] = 0.25 * 1073741824.0 * 0.99;
        CHECK(origin_cell(d, geo, c));
        d.t[0] = 0.25 * 1073741824.0 * 1.01;
        CHECK(!origin_cell(d, geo, c));
        d.t[0] = -0.25 * 1073741824.0 * 1.01;
        CHECK(!origin_cell(d, geo, c));
        d.t[0] = 0.0, d.t[1] = 1e300;        // +inf in f32
        CHECK(!origin_cell(d, geo, c));
        d.t[1] = (double)nan;
        CHECK(!origin_cell(d, geo, c));
    }
    // the planner: refusals in the definition's order, nothing kept after one
    const std::vector<ScanEntry> table = {{0, 300}, {300, 0}, {300, 257}, {557, 1}, {558, 1000}, {1558, 256}, {1814, 5}};
    {
        const int64_t ids[3] = {0, 2, 4};
        const lom_graph_pose poses[3] = {ident, ident, ident};
        CHECK(plan(table.data(), table.size(), ids, poses, 3, geo, &good, 0, pl, why) == LOM_OK);
        CHECK(pl.scans.scans.size() == 3 && pl.scans.points_in == 1557 && pl.launches.size() == 1);
        CHECK(pl.launches[0].first == 0 && pl.launches[0].count == 3 && pl.launches[0].max_n == 1000 && pl.launches[0].grid_x == 4);
        CHECK(pl.scans.scans[1].src == 300 && pl.scans.scans[1].n == 257 && pl.scans.scans[2].src == 558);
        const int64_t bad_ids[3] = {0, 7, 4};
        CHECK(plan(table.data(), table.size(), bad_ids, poses, 3, geo, &good, 0, pl, why) == LOM_ERR_ARG && !why.empty());
        CHECK(pl.scans.scans.empty() && pl.launches.empty());
        const int64_t neg_ids[1] = {-1};
        CHECK(plan(table.data(), table.size(), neg_ids, poses, 1, geo, &good, 0, pl, why) == LOM_ERR_ARG);
        lom_graph_pose bad_poses[3] = {ident, ident, ident};
        bad_poses[1].q_wxyz[0] = 0.0;
        CHECK(plan(table.data(), table.size(), ids, bad_poses, 3, geo, &good, 0, pl, why) == LOM_ERR_ARG);
        bad_poses[1] = ident, bad_poses[2].t[2] = (double)nan;
        CHECK(plan(table.data(), table.size(), ids, bad_poses, 3, geo, &good, 0, pl, why) == LOM_ERR_ARG);
        CHECK(plan(table.data(), table.size(), nullptr, poses, 3, geo, &good, 0, pl, why) == LOM_ERR_ARG);
        CHECK(plan(table.data(), table.size(), ids, nullptr, 3, geo, &good, 0, pl, why) == LOM_ERR_ARG);
        CHECK(plan(table.data(), table.size(), ids, poses, 3, geo, nullptr, 0, pl, why) == LOM_ERR_ARG);
        lom_elevation_point_params bad = good;
        bad.z_lo = 0.f;
        CHECK(plan(table.data(), table.size(), ids, poses, 3, geo, &bad, 0, pl, why) == LOM_ERR_ARG);
        CHECK(why.find("point parameters") != std::string::npos && pl.scans.scans.empty());
        // an origin out of range: LOM_ERR_RANGE, after the parameters, even for an empty scan
        lom_graph_pose far_poses[3] = {ident, ident, ident};
        far_poses[2].t[1] = -1e12;
        CHECK(plan(table.data(), table.size(), ids, far_poses, 3, geo, &good, 0, pl, why) == LOM_ERR_RANGE);
        CHECK(why.find("scan 2") != std::string::npos && pl.scans.scans.empty() && pl.launches.empty());
        CHECK(plan(table.data(), table.size(), ids, far_poses, 3, geo, &bad, 0, pl, why) == LOM_ERR_ARG);
        const int64_t empty_id[1] = {1};
        CHECK(plan(table.data(), table.size(), empty_id, far_poses + 2, 1, geo, &good, 0, pl, why) == LOM_ERR_RANGE);
        far_poses[2].t[1] = 1e7;  // far from the grid, inside the range: legal
        CHECK(plan(table.data(), table.size(), ids, far_poses, 3, geo, &good, 0, pl, why) == LOM_OK);
    }
    // launches under a cap; empty scans; an empty call
    {
        const int64_t ids[7] = {6, 1, 1, 3, 5, 1, 0};
        std::vector<lom_graph_pose> poses(7, ident);
        for (uint32_t cap : {1u, 2u, 3u, 7u, 0u}) {
            CHECK(plan(table.data(), table.size(), ids, poses.data(), 7, geo, &good, cap, pl, why) == LOM_OK);
            const uint32_t per = cap ? cap : kScansPerLaunch;
            uint64_t covered = 0;
            for (const Launch &l : pl.launches) {
                CHECK(l.first % per == 0 && l.count >= 1 && l.count <= per && l.first + l.count <= 7);
                uint32_t max_n = 0;
                for (uint32_t k = 0; k < l.count; k++) {
                    max_n = std::max(max_n, pl.scans.scans[l.first + k].n);
                    covered += pl.scans.scans[l.first + k].n;
                }
                CHECK(l.max_n == max_n && max_n > 0 && l.grid_x == (max_n + 255u) / 256u);
            }
            CHECK(covered == pl.scans.points_in && covered == 5 + 1 + 256 + 300);
            if (cap == 1u) CHECK(pl.launches.size() == 4);   // the three empty scans are launches of nothing: not listed
            if (cap == 2u) CHECK(pl.launches.size() == 4 && pl.launches[1].first == 2 && pl.launches[1].max_n == 1);
            if (cap == 3u) CHECK(pl.launches.size() == 3 && pl.launches[1].grid_x == 1 && pl.launches[2].grid_x == 2);
            if (cap == 7u || cap == 0u) CHECK(pl.launches.size() == 1 && pl.launches[0].count == 7 && pl.launches[0].grid_x == 2);
        }
        const int64_t only_empty[2] = {1, 1};
        CHECK(plan(table.data(), table.size(), only_empty, poses.data(), 2, geo, &good, 0, pl, why) == LOM_OK);
        CHECK(pl.launches.empty() && pl.scans.scans.size() == 2 && pl.scans.points_in == 0);
        CHECK(plan(table.data(), table.size(), nullptr, nullptr, 0, geo, &good, 0, pl, why) == LOM_OK);
        CHECK(pl.launches.empty() && pl.scans.scans.empty());
        CHECK(plan(nullptr, 0, nullptr, nullptr, 0, geo, nullptr, 0, pl, why) == LOM_ERR_ARG);  // the parameters count even then
    }
    return check_done();
}

#else
#include "lidar_odometry_amd.hpp"

int main()
{
    try {
        const lom::ElevationGeometry geo = {0.5f, -4.f, -3.f, 45u, 37u, 0.25f};
        const lom::ElevationPointParams prm = {-2.f, 1.f, 0.5f, 30.f};
        const lom::ElevationLayerParams lp = {1u, 2u};
        const lom::ElevationCostParams cp = {0.2f, 0.12f, 0.2f, 0.3f};
        lom::ElevationGrid grid(geo);
        CHECK(grid.size() == 45u * 37u && grid.geometry().width == 45u && grid.geometry().z_ref == 0.25f);
        lom::PointCloud<lom::PointXYZ> cloud;
        for (int k = 0; k < 400; k++) {
            lom::PointXYZ p;  // (f64, one rounding: as the Python side)
            p.x = (float)(0.37 * (k % 20) + 0.2), p.y = (float)(0.41 * (k / 20) + 0.1), p.z = (float)(0.06 * (k % 20) - 0.9 + 0.5 * ((k / 20) == 9));
            cloud.points.push_back(p);
        }
        lom::ScanArchive archive;
        CHECK(archive.addPoints(cloud) == 0 && archive.scanSize(0) == 400);
        const lom_graph_pose a = {{0.1, 0.1, 0.1}, {1, 0, 0, 0}}, b = {{0.1, 0.3, 0.1}, {2, 0, 0, 0.1}};
        lom::ElevationStats st = grid.integrate(archive, {0, 0}, {a, b}, prm);
        CHECK(st.scans == 2 && st.points == 800 && st.points_marked > 600 && st.points_out_of_height == 0 && st.cells_new > 100);
        const lom::ElevationGrid::Cells c1 = grid.cells();
        uint64_t total = 0;
        for (uint32_t v : c1.count) total += v;
        CHECK(total == st.points_marked);
        lom::ElevationSummary sm;
        const std::vector<int8_t> cost = grid.cost(lp, cp, &sm);
        CHECK(cost.size() == grid.size() && sm.cells_unknown + sm.cells_lethal + sm.cells_costed == grid.size());
        CHECK(sm.cells_costed > 20 && sm.cells_lethal > 2);
        const lom::ElevationGrid::Layers l = grid.layers(lp);
        for (size_t k = 0; k < grid.size(); k++) CHECK((c1.count[k] == 0u) == std::isnan(l.min[k]) && (cost[k] == -1) == (c1.count[k] == 0u));
        // the cloud form on the same points gives the same cells
        grid.clear();
        const lom::ElevationGrid::Cells c0 = grid.cells();
        for (size_t k = 0; k < grid.size(); k++) CHECK(c0.count[k] == 0u && c0.zmin[k] == INT32_MAX && c0.zmax[k] == INT32_MIN && c0.sum[k] == 0);
        grid.integrateCloud(cloud, a, prm);
        grid.integrateCloud(cloud, b, prm);
        const lom::ElevationGrid::Cells c2 = grid.cells();
        CHECK(c1.count == c2.count && c1.zmin == c2.zmin && c1.zmax == c2.zmax && c1.sum == c2.sum);
        bool threw = false;
        try {
            lom::ElevationPointParams bad = prm;
            bad.z_lo = 0.f;
            grid.integrateCloud(cloud, a, bad);
        } catch (const lom::Error &) {
            threw = true;
        }
        CHECK(threw);
        if (check_done()) return 1;
        std::printf("%llu %llu %llu\n", (unsigned long long)sm.cells_unknown, (unsigned long long)sm.cells_lethal,
                    (unsigned long long)sm.cells_costed);
        return 0;
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
}
#endif
