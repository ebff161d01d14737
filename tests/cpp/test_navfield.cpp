// The navigation field's host planning (csrc/navfield_host.cpp) compiled into a program of its own under
// -fsanitize=address,undefined (tests/test_navfield_cpp.py): value ranges, the cell-cost table, the quantisation of goals
// at cell borders and at the grid's edges, and the tile counts at 1, 32, 33 and 8192 cells.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "check.hpp"
#include "navfield_host.hpp"

using namespace lom;
using namespace lom::navfield;

static lom_occupancy_geometry geo(float r, uint32_t w, uint32_t h) { return lom_occupancy_geometry{r, -1.f, 2.f, w, h}; }
static lom_navfield_params prm(uint32_t neutral, uint32_t factor, uint32_t unknown, int max_passable, uint32_t flags = 0)
{
    return lom_navfield_params{neutral, factor, unknown, (int8_t)max_passable, flags};
}

static void test_ranges()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    lom_occupancy_geometry g = geo(0.25f, 1, 1);
    CHECK(geometry_ok(&g) && !geometry_ok(nullptr));
    g = geo(0.25f, 8192, 8192);
    CHECK(geometry_ok(&g));
    for (uint32_t bad : {0u, 8193u, 0xffffffffu}) {
        g = geo(0.25f, bad, 5);
        CHECK(!geometry_ok(&g));
        g = geo(0.25f, 5, bad);
        CHECK(!geometry_ok(&g));
    }
    for (float bad : {0.f, -1.f, nan, inf}) {
        g = geo(bad, 5, 5);
        CHECK(!geometry_ok(&g));
        g = geo(0.25f, 5, 5);
        g.origin_y = bad == 0.f || bad == -1.f ? nan : bad;
        CHECK(!geometry_ok(&g));
    }
    CHECK(!params_ok(nullptr));
    lom_navfield_params p = prm(1, 0, 0, 0);
    CHECK(params_ok(&p));
    p = prm(0, 0, 1, 98);
    CHECK(!params_ok(&p));
    for (int mp : {-128, -1, 99, 100, 127}) {
        p = prm(5, 1, 1, mp);
        CHECK(!params_ok(&p));
    }
    for (int mp : {0, 1, 98}) {
        p = prm(5, 1, 1, mp);
        CHECK(params_ok(&p));
    }
    // neutral + 98 * factor <= 2^24 - 1, without wrapping: 98 * 171196 + 7 = 2^24 - 1
    p = prm(7, 171196, 1, 98);
    CHECK(params_ok(&p));
    p = prm(8, 171196, 1, 98);
    CHECK(!params_ok(&p));
    p = prm(kMaxCellCost, 0, 1, 98);
    CHECK(params_ok(&p));
    p = prm(kMaxCellCost + 1u, 0, 1, 98);
    CHECK(!params_ok(&p));
    p = prm(1, 0xffffffffu, 1, 98);  // 98 * factor wraps a u32
    CHECK(!params_ok(&p));
    p = prm(0xffffffffu, 0xffffffffu, 1, 0);
    CHECK(!params_ok(&p));
    // unknown_cost: read under the flag only
    p = prm(5, 1, 0, 98);
    CHECK(params_ok(&p));
    p = prm(5, 1, 0xffffffffu, 98);
    CHECK(params_ok(&p));
    for (uint32_t u : {0u, kMaxCellCost + 1u, 0xffffffffu}) {
        p = prm(5, 1, u, 98, LOM_NAV_UNKNOWN_PASSABLE);
        CHECK(!params_ok(&p));
    }
    for (uint32_t u : {1u, kMaxCellCost}) {
        p = prm(5, 1, u, 98, LOM_NAV_UNKNOWN_PASSABLE);
        CHECK(params_ok(&p));
    }
    for (uint32_t f : {2u, 3u, 0x80000000u}) {
        p = prm(5, 1, 1, 98, f);
        CHECK(!params_ok(&p));
    }
    CHECK(!byte_invalid(-1) && !byte_invalid(0) && !byte_invalid(100) && byte_invalid(-2) && byte_invalid(101) && byte_invalid(-128) && byte_invalid(127));
}

static void test_table()
{
    uint32_t t[256];
    for (uint32_t flags : {0u, (uint32_t)LOM_NAV_UNKNOWN_PASSABLE}) {
        for (int mp : {0, 40, 98}) {
            const lom_navfield_params p = prm(50, 3, 400, mp, flags);
            cell_costs(p, t);
            for (int b = 0; b < 256; b++) {
                const int v = (int)(int8_t)(uint8_t)b;  // the byte as the plane holds it
                uint32_t want = 0u;
                if (v >= 0 && v <= mp) want = 50u + 3u * (uint32_t)v;
                if (v == -1 && flags) want = 400u;
                CHECK(t[b] == want);
            }
        }
    }
    const lom_navfield_params big = prm(7, 171196, kMaxCellCost, 98, LOM_NAV_UNKNOWN_PASSABLE);
    cell_costs(big, t);
    CHECK(t[0] == 7u && t[98] == kMaxCellCost && t[99] == 0u && t[100] == 0u && t[255] == kMaxCellCost && t[254] == 0u && t[128] == 0u);
    CHECK(7ull * t[98] < (1ull << 27));  // a step's weight fits a u32 with room
}

static void test_quantise()
{
    const lom_occupancy_geometry g = geo(0.25f, 45, 37);  // x in [-1, 10.25), y in [2, 11.25)
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    int32_t ix, iy;
    CHECK(cell_of_metres(g, -1.f, 2.f, &ix, &iy) && ix == 0 && iy == 0);
    CHECK(cell_of_metres(g, -0.75f, 2.25f, &ix, &iy) && ix == 1 && iy == 1);  // a border belongs to the cell above it
    CHECK(cell_of_metres(g, std::nextafter(-0.75f, -2.f), std::nextafter(2.25f, 0.f), &ix, &iy) && ix == 0 && iy == 0);
    CHECK(cell_of_metres(g, std::nextafter(10.25f, 0.f), std::nextafter(11.25f, 0.f), &ix, &iy) && ix == 44 && iy == 36);
    CHECK(!cell_of_metres(g, 10.25f, 5.f, &ix, &iy) && ix == -1 && iy == -1);
    CHECK(!cell_of_metres(g, 5.f, 11.25f, &ix, &iy) && ix == -1 && iy == -1);
    CHECK(!cell_of_metres(g, std::nextafter(-1.f, -2.f), 5.f, &ix, &iy));
    CHECK(!cell_of_metres(g, 5.f, std::nextafter(2.f, 0.f), &ix, &iy));
    for (float bad : {nan, inf, -inf, 1e30f, -1e30f}) {
        CHECK(!cell_of_metres(g, bad, 5.f, &ix, &iy) && ix == -1 && iy == -1);
        CHECK(!cell_of_metres(g, 5.f, bad, &ix, &iy) && ix == -1 && iy == -1);
    }
    // both kinds through quantise: cells pass as they are, metres by the floor rule; an unknown kind is refused
    const int32_t cells[6] = {0, 0, -5, 7, 44, 99};
    const float metres[6] = {-1.f, 2.f, nan, 5.f, 10.2f, 11.2f};
    std::vector<int32_t> out(6, 77);
    CHECK(quantise(g, LOM_NAV_CELLS, cells, 3, out.data()));
    for (int i = 0; i < 6; i++) CHECK(out[i] == cells[i]);
    CHECK(quantise(g, LOM_NAV_METRES, metres, 3, out.data()));
    CHECK(out[0] == 0 && out[1] == 0 && out[2] == -1 && out[3] == -1 && out[4] == 44 && out[5] == 36);
    CHECK(!quantise(g, 2, metres, 3, out.data()) && !quantise(g, -1, cells, 3, out.data()));
    CHECK(quantise(g, LOM_NAV_CELLS, nullptr, 0, nullptr) && quantise(g, LOM_NAV_METRES, nullptr, 0, nullptr));
    // a 1 x 1 grid and the largest one
    const lom_occupancy_geometry one = geo(2.f, 1, 1), huge = geo(0.5f, 8192, 8192);
    CHECK(cell_of_metres(one, 0.99f, 3.99f, &ix, &iy) && ix == 0 && iy == 0 && !cell_of_metres(one, 1.f, 3.f, &ix, &iy));
    CHECK(cell_of_metres(huge, std::nextafter(4095.f, 0.f), std::nextafter(4098.f, 0.f), &ix, &iy) && ix == 8191 && iy == 8191);
    CHECK(!cell_of_metres(huge, 4095.f, 3.f, &ix, &iy));
}

static void test_tiles()
{
    const struct {
        uint32_t cells, tiles;
    } cases[] = {{1, 1}, {31, 1}, {32, 1}, {33, 2}, {64, 2}, {65, 3}, {129, 5}, {8191, 256}, {8192, 256}};
    for (const auto &cx : cases)
        for (const auto &cy : cases) {
            const TileGrid t = tile_grid(cx.cells, cy.cells);
            CHECK(t.tiles_x == cx.tiles && t.tiles_y == cy.tiles && t.n_tiles == cx.tiles * cy.tiles);
            // every cell lies in exactly one tile, and the last tile is not empty
            CHECK((t.tiles_x - 1u) * kTile < cx.cells && t.tiles_x * kTile >= cx.cells);
            CHECK((t.tiles_y - 1u) * kTile < cy.cells && t.tiles_y * kTile >= cy.cells);
        }
    CHECK(blocks_for(0) == 1u && blocks_for(1) == 1u && blocks_for(256) == 1u && blocks_for(257) == 2u);
    CHECK(blocks_for((size_t)8192 * 8192) == 8192u * 8192u / 256u && blocks_for(kMaxPoints) == (1u << 16));
    CHECK(launch_bound(1, 1) == 66u && launch_bound(8192, 8192) == (1ull << 27) + 64u);
    CHECK(kInnerCapDefault >= 1u && kInnerCapDefault <= kInnerCapMax && kBatchDefault >= 1u && kBatchDefault <= kBatchMax);
}

int main()
{
    test_ranges();
    test_table();
    test_quantise();
    test_tiles();
    return check_done();
}
