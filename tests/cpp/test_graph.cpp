// The C++ side of the pose graph, two programs from one file (tests/test_graph_cpp.py):
//  - default: the mirror lom::PoseGraph and the stateless host functions against the library, no device needed;
//  - -DGRAPH_HOST_STANDALONE: csrc/graph_host.cpp compiled into this program under -fsanitize=address,undefined: the gauge
//    check, the CSR build and the Cholesky on degenerate shapes (zero nodes, zero edges, a hub of degree 200, duplicates).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "check.hpp"

#ifdef GRAPH_HOST_STANDALONE
#include "graph_host.hpp"

using namespace lom::graph;

int main()
{
    int64_t bad = 5;
    std::vector<uint32_t> row, ent;
    // zero nodes, zero edges
    CHECK(check_gauge(0, nullptr, 0, nullptr, &bad) == LOM_OK && bad == -1);
    build_csr(0, 0, nullptr, row, ent);
    CHECK(row.size() == 1 && row[0] == 0 && ent.empty());
    // nodes without edges
    std::vector<int32_t> fixed = {1, 0, 1};
    CHECK(check_gauge(3, fixed.data(), 0, nullptr, &bad) == LOM_ERR_ARG && bad == 1);
    build_csr(3, 0, nullptr, row, ent);
    CHECK(row.size() == 4 && row[3] == 0);
    // a hub of degree 200 on node 0, duplicate edges among them, the chain 1 - 2 - ... beside it
    const int n = 201;
    std::vector<int32_t> ij;
    for (int k = 1; k < n; k++) ij.push_back(0), ij.push_back(k);
    for (int k = 1; k + 1 < n; k++) ij.push_back(k + 1), ij.push_back(k);
    for (int d = 0; d < 3; d++) ij.push_back(7), ij.push_back(0);  // duplicates, the other way round
    const int64_t m = (int64_t)ij.size() / 2;
    fixed.assign(n, 0);
    CHECK(check_gauge(n, fixed.data(), m, ij.data(), &bad) == LOM_ERR_ARG && bad == 0);
    fixed[n - 1] = 1;
    CHECK(check_gauge(n, fixed.data(), m, ij.data(), &bad) == LOM_OK && bad == -1);
    build_csr(n, m, ij.data(), row, ent);
    CHECK(row.size() == (size_t)n + 1 && row[n] == 2 * m && ent.size() == (size_t)(2 * m));
    CHECK(row[1] - row[0] == 203);
    for (int k = 0; k < n; k++)
        for (uint32_t q = row[k]; q < row[k + 1]; q++) {
            CHECK(q == row[k] || ent[q - 1] < ent[q]);  // ascending edge id (and side)
            CHECK(ij[ent[q]] == k);                     // entry = edge * 2 + side indexes the node itself
        }
    int32_t loop[2] = {3, 3}, out_of_range[2] = {0, n};
    CHECK(check_gauge(n, fixed.data(), 1, loop, &bad) == LOM_ERR_ARG && bad == -1);
    CHECK(check_gauge(n, fixed.data(), 1, out_of_range, &bad) == LOM_ERR_ARG && bad == -1);
    // Cholesky: identity, a matrix with a zero pivot, a negative one, a non-finite value, and U^T U = Omega
    double om[36] = {}, U[21];
    for (int a = 0; a < 6; a++) om[a * 6 + a] = 1.0;
    CHECK(cholesky6_upper(om, U) && U[0] == 1.0 && U[1] == 0.0 && U[20] == 1.0);
    om[35] = 0.0;
    CHECK(!cholesky6_upper(om, U));
    om[35] = -1.0;
    CHECK(!cholesky6_upper(om, U));
    om[35] = 1.0, om[7] = NAN;
    CHECK(!cholesky6_upper(om, U));
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++) om[a * 6 + b] = (a == b ? 10.0 + a : 0.0) + 1.0 / (1.0 + a + b);
    CHECK(cholesky6_upper(om, U));
    for (int a = 0; a < 6; a++)
        for (int b = a; b < 6; b++) {
            double v = 0.0;
            for (int k = 0; k <= a; k++) v += U[k * 6 - k * (k - 1) / 2 + (a - k)] * U[k * 6 - k * (k - 1) / 2 + (b - k)];
            CHECK(std::fabs(v - om[a * 6 + b]) < 1e-13);
        }
    lom_graph_params p = {1e-4, 1e-5, 1e-12, 1e-8, 10, 10};
    CHECK(params_ok(&p) && !params_ok(nullptr));
    p.gtol = 0.0;
    CHECK(!params_ok(&p));
    lom_graph_pose pose = {{0, 0, 0}, {0, 0, 0, 0}};
    CHECK(!pose_ok(&pose));
    pose.q_wxyz[2] = 2.0;
    double x[7];
    CHECK(pose_ok(&pose));
    normalised(&pose, x);
    CHECK(x[5] == 1.0 && x[3] == 0.0);
    double lambda = 1.0, nu = 2.0, rho = 0.0;
    CHECK(lom_graph_lm_policy(10.0, 11.0, 3.0, &lambda, &nu, &rho) == 0 && lambda == 2.0 && nu == 4.0 && rho < 0.0);
    return check_done();
}
#else
#include "lidar_odometry_amd.hpp"

int main()
{
    // stateless host functions through the C ABI
    int32_t fixed[3] = {1, 0, 0}, ij[4] = {0, 1, 1, 2};
    int64_t bad = 0;
    CHECK(lom_graph_check_gauge(3, fixed, 2, ij, &bad) == LOM_OK && bad == -1);
    CHECK(lom_graph_check_gauge(3, fixed, 1, ij, &bad) == LOM_ERR_ARG && bad == 2);
    double lambda = 1e-3, nu = 8.0, rho = 0.0;
    CHECK(lom_graph_lm_policy(10.0, 5.0, 10.0, &lambda, &nu, &rho) == 1 && rho == 1.0 && nu == 2.0);
    CHECK(std::fabs(lambda - 1e-3 / 3.0) < 1e-18);
    // information from a quality report: S (H + P) S
    lom::QualityReport rep{};
    rep.valid = 7;
    for (int a = 0; a < 6; a++) rep.information[a * 6 + a] = 4.0;
    rep.information[0 * 6 + 3] = rep.information[3 * 6 + 0] = 2.0;
    const std::vector<double> om = lom::PoseGraph::informationFromQuality(rep, true);
    CHECK(om.size() == 36 && om[0] == 1.0 && om[21] == 104.0 && om[3] == 1.0 && om[18] == 1.0);
    CHECK(lom::PoseGraph::informationFromQuality(rep, false)[21] == 4.0);
    rep.valid = 6;
    bool threw = false;
    try {
        lom::PoseGraph::informationFromQuality(rep, true);
    } catch (const lom::Error &e) {
        threw = e.code == LOM_ERR_ARG;
    }
    CHECK(threw);
    // f32 pose to the graph's and back
    const lom::Pose3D p32(lom::Vector3f(1.5f, -2.f, 0.25f), lom::Quaternionf(0.5f, 0.5f, 0.5f, -0.5f));
    const lom::GraphPose p64 = lom::PoseGraph::fromPose3D(p32);
    CHECK(p64.t[0] == 1.5 && p64.q_wxyz[3] == -0.5);
    const lom::Pose3D back = lom::PoseGraph::toPose3D(p64);
    CHECK(back.translation.y() == -2.f && back.rotation.z() == -0.5f);
    // without a device the constructor fails loudly; with one, the refusals that need no kernel
    if (lom_device_count() < 1) {
        threw = false;
        try {
            lom::PoseGraph g;
        } catch (const lom::Error &e) {
            threw = e.code == LOM_ERR_NO_DEVICE;
        }
        CHECK(threw);
    } else {
        lom::PoseGraph g(4, 4);
        CHECK(g.addNode(p64, true) == 0 && g.addNode(p64, false) == 1 && g.nodeCount() == 2);
        std::vector<double> eye(36, 0.0);
        for (int a = 0; a < 6; a++) eye[a * 6 + a] = 1.0;
        threw = false;
        try {
            g.addEdge(0, 2, p32, eye, 0.0);
        } catch (const lom::Error &e) {
            threw = e.code == LOM_ERR_ARG;
        }
        CHECK(threw && g.edgeCount() == 0);
        CHECK(g.addEdge(0, 1, lom::Pose3D(), eye, 0.0) == 0);
        const lom::GraphParams prm = {1e-4, 1e-9, 1e-14, 1e-8, 10, 20};
        const lom::GraphStats st = g.optimize(prm);
        CHECK(st.stop_reason == LOM_GRAPH_STOP_GRADIENT && g.poses().size() == 2 && g.chi2().size() == 1);
    }
    return check_done();
}
#endif
