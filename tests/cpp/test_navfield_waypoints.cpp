// Steps 8 and 9 of the navigation field on the host, compiled into a program of its own under -fsanitize=address,undefined
// (tests/test_navfield_waypoints_cpp.py): csrc/nav_los_rule.hpp -- the code both forms of k_nav_shortcut and k_nav_visible
// run -- on planes, pairs and routes the test wrote, its answers written back for a byte-for-byte comparison with
// tests/navfield_waypoints_ref.py; and the parameter rule and the output bounds of csrc/navfield_host.cpp.
//
// argv[1], all little-endian: u32 n_cases; per case u32 {width, height, max_cell_cost, lookahead, wp_cap, n_pairs, n_routes},
// 256 u32 of the cell-cost table, width * height plane bytes, n_pairs int32 quadruples, and per route u32 n and n u16 pairs.
// argv[2]: per case n_pairs bytes, then per route u32 count and wp_cap u16 pairs.
#include <cstdio>
#include <cstring>
#include <vector>

#include "check.hpp"
#include "nav_los_rule.hpp"
#include "navfield_host.hpp"

using namespace lom;
using namespace lom::navfield;

static lom_navfield_waypoint_params wp(uint32_t max_cell_cost, uint32_t lookahead, uint32_t route_cap, uint32_t flags = 0)
{
    return lom_navfield_waypoint_params{max_cell_cost, lookahead, route_cap, flags};
}

static void test_planning()
{
    lom_navfield_waypoint_params p = wp(0, 1, 1);
    CHECK(waypoint_params_ok(&p, 0) && waypoint_params_ok(&p, 1) && waypoint_params_ok(&p, kMaxPathCells) && !waypoint_params_ok(nullptr, 1));
    CHECK(!waypoint_params_ok(&p, kMaxPathCells + 1));
    p = wp(0xFFFFFFFFu, 65535, 1024);
    CHECK(waypoint_params_ok(&p, kMaxPathCells / 1024) && !waypoint_params_ok(&p, kMaxPathCells / 1024 + 1));
    for (uint32_t bad : {0u, 65536u, 0xFFFFFFFFu}) {
        p = wp(0, bad, 10);
        CHECK(!waypoint_params_ok(&p, 1));
    }
    p = wp(0, 64, 0);
    CHECK(!waypoint_params_ok(&p, 1) && !waypoint_params_ok(&p, 0));
    p = wp(0, 64, (1u << 28) + 1u);
    CHECK(!waypoint_params_ok(&p, 0) && !waypoint_params_ok(&p, 1));
    p = wp(0, 64, 1u << 28);
    CHECK(waypoint_params_ok(&p, 1) && !waypoint_params_ok(&p, 2));
    p = wp(0, 64, 0xFFFFFFFFu);
    CHECK(!waypoint_params_ok(&p, 1));
    for (uint32_t f : {1u, 2u, 0x80000000u}) {
        p = wp(0, 64, 10, f);
        CHECK(!waypoint_params_ok(&p, 1));
    }
    uint16_t cell[2];
    CHECK(waypoint_output_ok(0, 0, nullptr) && waypoint_output_ok(5, 0, nullptr) && waypoint_output_ok(0, 5, nullptr));
    CHECK(!waypoint_output_ok(5, 1, nullptr) && waypoint_output_ok(5, 1, cell));
    CHECK(waypoint_output_ok(1u << 14, 1u << 14, cell) && !waypoint_output_ok((1u << 14) + 1u, 1u << 14, cell));
    CHECK(waypoint_output_ok(1, kMaxPathCells, cell) && !waypoint_output_ok(1, kMaxPathCells + 1, cell) && !waypoint_output_ok(0, kMaxPathCells + 1, nullptr));
    CHECK(shortcut_blocks_for(0) == 1u && shortcut_blocks_for(1) == 1u && shortcut_blocks_for(4) == 1u && shortcut_blocks_for(5) == 2u);
    CHECK(shortcut_blocks_for(kMaxPoints) == (1u << 22));
    CHECK(nav_clear(1, 0) && !nav_clear(0, 0) && !nav_clear(0, 5) && nav_clear(5, 5) && !nav_clear(6, 5) && nav_clear(0xFFFFFFu, 0));
}

template <class T>
static bool get(std::FILE *f, T *v, size_t n)
{
    return n == 0 || std::fread(v, sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    test_planning();
    if (argc != 3) {
        std::printf("usage: %s cases.bin answers.bin\n", argv[0]);
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t n_cases = 0;
    if (!get(in, &n_cases, 1)) return 2;
    size_t n_seen = 0;
    for (uint32_t k = 0; k < n_cases; k++) {
        uint32_t head[7];
        if (!get(in, head, 7)) return 2;
        const uint32_t w = head[0], h = head[1], max_cell_cost = head[2], W = head[3], wp_cap = head[4], n_pairs = head[5], n_routes = head[6];
        // exactly sized blocks, so that a read outside the plane or a route is the sanitizer's to find
        std::vector<uint32_t> table(256);
        std::vector<int8_t> plane((size_t)w * h);
        std::vector<int32_t> pairs((size_t)4 * n_pairs);
        if (!get(in, table.data(), 256) || !get(in, plane.data(), plane.size()) || !get(in, pairs.data(), pairs.size())) return 2;
        const NavPlaneCost cost{plane.data(), table.data(), w};
        std::vector<uint8_t> vis(n_pairs);
        for (uint32_t i = 0; i < n_pairs; i++) {
            const int32_t *q = pairs.data() + 4 * (size_t)i;
            vis[i] = nav_visible(q[0], q[1], q[2], q[3], w, h, max_cell_cost, cost) ? 1 : 0;
            n_seen += vis[i];
        }
        if (!vis.empty()) std::fwrite(vis.data(), 1, vis.size(), out);
        for (uint32_t r = 0; r < n_routes; r++) {
            uint32_t n = 0;
            if (!get(in, &n, 1)) return 2;
            std::vector<uint16_t> route((size_t)2 * n), cells((size_t)2 * wp_cap, 0);
            if (!get(in, route.data(), route.size())) return 2;
            const uint32_t count = n ? nav_waypoints_serial(route.data(), n, W, w, h, max_cell_cost, cost, cells.data(), wp_cap) : 0u;
            std::fwrite(&count, 4, 1, out);
            if (!cells.empty()) std::fwrite(cells.data(), 2, cells.size(), out);
        }
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("%u cases, %zu pairs visible\n", n_cases, n_seen);
    return check_done();
}
