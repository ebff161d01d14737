// The C++ side of the scan archive and the map assembly, two programs from one file (tests/test_assemble_cpp.py):
//  - default: the mirror lom::ScanArchive / VoxelGrid::assemble and the host function against the library; without a
//    device the constructor's loud failure, with one a small assembly and its refusals;
//  - -DASSEMBLE_HOST_STANDALONE: csrc/assemble_host.cpp compiled into this program under -fsanitize=address,undefined: the
//    planner on empty input, a single empty scan, repeated ids, bad ids and poses, archive offsets at the 2^32 boundary
//    of the point count (the kernels index with 32 bits: refused with LOM_ERR_ARG), a call beyond 2^31 - 2 points, more
//    than 2^24 scans, and 10^5 scans.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "check.hpp"

#ifdef ASSEMBLE_HOST_STANDALONE
#include "assemble_host.hpp"

using namespace lom::assemble;

int main()
{
    Plan plan;
    std::string why;
    const lom_graph_pose ident = {{0, 0, 0}, {1, 0, 0, 0}};
    // empty input: nothing is read
    CHECK(lom::assemble::plan(nullptr, 0, nullptr, nullptr, 0, plan, why) == LOM_OK && plan.scans.empty() && plan.points_in == 0);
    // NULL arrays with a count
    std::vector<ScanEntry> table = {{0, 0}};
    int64_t id0 = 0;
    CHECK(lom::assemble::plan(table.data(), 1, nullptr, &ident, 1, plan, why) == LOM_ERR_ARG);
    CHECK(lom::assemble::plan(table.data(), 1, &id0, nullptr, 1, plan, why) == LOM_ERR_ARG);
    // a single empty scan
    CHECK(lom::assemble::plan(table.data(), 1, &id0, &ident, 1, plan, why) == LOM_OK);
    CHECK(plan.scans.size() == 1 && plan.points_in == 0 && plan.grid_x == 0 && plan.blocks == 0 && plan.scans[0].n == 0);
    // repeated ids, ragged sizes, an empty scan between them: offsets and block rows
    table = {{0, 257}, {257, 0}, {257, 64}, {321, 1000}};
    std::vector<int64_t> ids = {3, 0, 1, 0, 2};
    std::vector<lom_graph_pose> poses(ids.size(), ident);
    poses[1] = {{1, 2, 3}, {0, 0, 0, -2}};  // unnormalised, w = 0: a half turn about z
    CHECK(lom::assemble::plan(table.data(), table.size(), ids.data(), poses.data(), ids.size(), plan, why) == LOM_OK);
    CHECK(plan.points_in == 1000 + 257 + 257 + 64 && plan.max_n == 1000 && plan.grid_x == 4 && plan.blocks == 4 + 2 + 0 + 2 + 1);
    const uint32_t want_out[5] = {0, 1000, 1257, 1257, 1514}, want_blk[5] = {0, 4, 6, 6, 8}, want_src[5] = {321, 0, 0, 0, 257};
    for (int k = 0; k < 5; k++)
        CHECK(plan.scans[k].out == want_out[k] && plan.scans[k].blk == want_blk[k] && plan.scans[k].src == want_src[k]);
    CHECK(plan.scans[1].R[0] == -1.0 && plan.scans[1].R[4] == -1.0 && plan.scans[1].R[8] == 1.0 && plan.scans[1].t[2] == 3.0);
    CHECK(plan.scans[0].R[0] == 1.0 && plan.scans[0].R[1] == 0.0 && plan.scans[0].R[4] == 1.0);
    // bad ids
    for (int64_t bad : {(int64_t)-1, (int64_t)4, std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::min()}) {
        ids[2] = bad;
        CHECK(lom::assemble::plan(table.data(), table.size(), ids.data(), poses.data(), ids.size(), plan, why) == LOM_ERR_ARG);
        CHECK(plan.scans.empty() && !why.empty());
    }
    ids[2] = 1;
    // bad poses
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int field = 0; field < 7; field++)
        for (double v : {nan, inf}) {
            std::vector<lom_graph_pose> p = poses;
            (field < 3 ? p[4].t[field] : p[4].q_wxyz[field - 3]) = v;
            CHECK(lom::assemble::plan(table.data(), table.size(), ids.data(), p.data(), ids.size(), plan, why) == LOM_ERR_ARG);
        }
    {
        std::vector<lom_graph_pose> p = poses;
        p[0] = {{0, 0, 0}, {0, 0, 0, 0}};
        CHECK(lom::assemble::plan(table.data(), table.size(), ids.data(), p.data(), ids.size(), plan, why) == LOM_ERR_ARG);
        CHECK(!pose_ok(&p[0]) && !pose_ok(nullptr) && pose_ok(&ident));
    }
    // the 2^32 boundary of the archive's point count: the last scan that ends at 2^32 is taken, one point further is refused
    table = {{(1ull << 32) - 100, 100}, {(1ull << 32) - 99, 100}, {1ull << 32, 1}, {1ull << 32, 0}};
    ids = {0};
    poses.assign(1, ident);
    CHECK(lom::assemble::plan(table.data(), table.size(), ids.data(), poses.data(), 1, plan, why) == LOM_OK);
    CHECK(plan.scans[0].src == 0xFFFFFF9Cu && plan.scans[0].n == 100);
    ids = {1};
    CHECK(lom::assemble::plan(table.data(), table.size(), ids.data(), poses.data(), 1, plan, why) == LOM_ERR_ARG);
    ids = {2};
    CHECK(lom::assemble::plan(table.data(), table.size(), ids.data(), poses.data(), 1, plan, why) == LOM_ERR_ARG);
    ids = {3};  // an empty scan reads nothing, wherever it lies
    CHECK(lom::assemble::plan(table.data(), table.size(), ids.data(), poses.data(), 1, plan, why) == LOM_OK && plan.scans[0].src == 0);
    // a call beyond what one insert takes: 2^31 - 2 points pass, one more is refused
    table = {{0, 0x7FFFFFFEu}, {0, 1}};
    ids = {0};
    CHECK(lom::assemble::plan(table.data(), table.size(), ids.data(), poses.data(), 1, plan, why) == LOM_OK);
    CHECK(plan.points_in == 0x7FFFFFFEull && plan.grid_x == (0x7FFFFFFEu + 255) / 256 && plan.blocks == plan.grid_x);
    ids = {0, 1};
    poses.assign(2, ident);
    CHECK(lom::assemble::plan(table.data(), table.size(), ids.data(), poses.data(), 2, plan, why) == LOM_ERR_ARG);
    // 10^5 scans, ragged, every id twice
    const size_t K = 100000;
    table.clear();
    uint64_t at = 0;
    for (size_t k = 0; k < K / 2; k++) {
        const uint32_t n = (uint32_t)((k * 37) % 300);
        table.push_back({at, n});
        at += n;
    }
    ids.resize(K);
    poses.assign(K, ident);
    for (size_t k = 0; k < K; k++) ids[k] = (int64_t)(k % (K / 2));
    CHECK(lom::assemble::plan(table.data(), table.size(), ids.data(), poses.data(), K, plan, why) == LOM_OK);
    CHECK(plan.scans.size() == K && plan.points_in == 2 * at && plan.max_n == 299 && plan.grid_x == 2);
    uint64_t out = 0, blk = 0;
    for (size_t k = 0; k < K; k++) {
        const AsmScan &d = plan.scans[k];
        CHECK(d.out == out && d.blk == blk && d.n == table[(size_t)ids[k]].n && (d.n == 0 || d.src == table[(size_t)ids[k]].offset));
        out += d.n, blk += (d.n + kAsmThreads - 1) / kAsmThreads;
    }
    CHECK(plan.blocks == blk);
    // count overflow: refused before the arrays are read
    CHECK(lom::assemble::plan(table.data(), table.size(), ids.data(), poses.data(), kAsmMaxScans + 1, plan, why) == LOM_ERR_ARG);
    CHECK(lom::assemble::plan(table.data(), table.size(), ids.data(), poses.data(), std::numeric_limits<size_t>::max(), plan, why) == LOM_ERR_ARG);
    // the cull's parameters
    bool cull = true;
    lom_assemble_params prm = {{0, 0, 0}, 5.f};
    CHECK(cull_of(nullptr, &cull, why) == LOM_OK && !cull);
    CHECK(cull_of(&prm, &cull, why) == LOM_OK && cull);
    prm.radius = 0.f;
    CHECK(cull_of(&prm, &cull, why) == LOM_OK && !cull);
    prm.radius = -1.f;
    CHECK(cull_of(&prm, &cull, why) == LOM_OK && !cull);
    prm.radius = std::numeric_limits<float>::quiet_NaN();
    CHECK(cull_of(&prm, &cull, why) == LOM_ERR_ARG);
    prm.radius = 5.f, prm.centre[1] = std::numeric_limits<float>::infinity();
    CHECK(cull_of(&prm, &cull, why) == LOM_ERR_ARG);
    // the C ABI's host function lives in the same file
    double R[9];
    CHECK(lom_graph_pose_rotation_matrix(&ident, R) == LOM_OK && R[0] == 1.0 && R[4] == 1.0 && R[8] == 1.0 && R[1] == 0.0);
    CHECK(lom_graph_pose_rotation_matrix(nullptr, R) == LOM_ERR_ARG && lom_graph_pose_rotation_matrix(&ident, nullptr) == LOM_ERR_ARG);
    return check_done();
}
#else
#include "lidar_odometry_amd.hpp"

int main()
{
    // the host function through the mirror: a quarter turn about z, from an unnormalised quaternion
    const lom::GraphPose quarter = {{1.0, 2.0, 3.0}, {2.0, 0.0, 0.0, 2.0}};
    const std::vector<double> R = lom::ScanArchive::rotationMatrix(quarter);
    CHECK(R.size() == 9 && std::fabs(R[0]) < 1e-15 && std::fabs(R[1] + 1.0) < 1e-15 && std::fabs(R[3] - 1.0) < 1e-15 && R[8] == 1.0);
    bool threw = false;
    try {
        lom::ScanArchive::rotationMatrix(lom::GraphPose{{0, 0, 0}, {0, 0, 0, 0}});
    } catch (const lom::Error &e) {
        threw = e.code == LOM_ERR_ARG;
    }
    CHECK(threw);
    if (lom_device_count() < 1) {  // without a device the constructor fails loudly
        threw = false;
        try {
            lom::ScanArchive a;
        } catch (const lom::Error &e) {
            threw = e.code == LOM_ERR_NO_DEVICE;
        }
        CHECK(threw);
    } else {
        lom::ScanArchive a(1, 1);
        lom::PointCloud<lom::PointNormal> cloud, none;
        for (int i = 0; i < 300; i++) {
            lom::PointNormal p(0.01f * (float)i, 1.f, -2.f);
            p.normal_z = 1.f;
            cloud.points.push_back(p);
        }
        CHECK(a.add(cloud) == 0 && a.add(none) == 1 && a.add(cloud) == 2 && a.size() == 3 && a.pointCount() == 600);
        CHECK(a.scanSize(1) == 0 && a.get(2)->points.size() == 300 && a.get(2)->points[299].x == cloud.points[299].x);
        lom::VoxelGrid grid(0.5f, 10), want(0.5f, 10);
        const lom::GraphPose ident = {{0, 0, 0}, {1, 0, 0, 0}};
        const lom::AssembleStats st = grid.assemble(a, {0, 1, 2}, {ident, ident, quarter});
        CHECK(st.scans == 3 && st.points_in == 600 && st.points_kept == 600 && st.voxels_before == 0);
        CHECK(st.voxels_after == (int64_t)grid.size() && st.voxels_after > 0 && st.points_stored_after > 0);
        const lom::AssembleParams cull = {{0.f, 1.f, -2.f}, 1.f};
        const lom::AssembleStats st2 = want.assemble(a, {0}, {ident}, &cull);
        CHECK(st2.points_in == 300 && st2.points_kept == 101);  // x = 0 .. 1.00 stays: the radius itself is kept
        threw = false;
        try {
            grid.assemble(a, {3}, {ident});
        } catch (const lom::Error &e) {
            threw = e.code == LOM_ERR_ARG;
        }
        CHECK(threw && (int64_t)grid.size() == st.voxels_after);
        a.clear();
        CHECK(a.size() == 0 && a.pointCount() == 0);
    }
    return check_done();
}
#endif
