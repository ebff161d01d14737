// The clearance grid's host planning (csrc/clearance_host.cpp) compiled into a program of its own under
// -fsanitize=address,undefined (tests/test_clearance_cpp.py): value ranges, R, the cost table at its three boundaries,
// rectangles clipped at every border and grown, and the launch shapes -- every cell of a rectangle lies in exactly one
// tile, every cell of the grown rectangle in exactly one merge wave -- on 1 x 1 and 8192-wide grids, at R = 0 and 254.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "check.hpp"
#include "clearance_host.hpp"

using namespace lom;
using namespace lom::clearance;

static lom_occupancy_geometry geo(float r, uint32_t w, uint32_t h) { return lom_occupancy_geometry{r, -1.f, 2.f, w, h}; }
static lom_clearance_params prm(float infl, float ins, float decay, uint32_t flags = 0) { return lom_clearance_params{infl, ins, decay, flags}; }

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
    }
    g = geo(0.25f, 5, 5);
    g.origin_x = nan;
    CHECK(!geometry_ok(&g));
    g.origin_x = 0.f, g.origin_y = -inf;
    CHECK(!geometry_ok(&g));

    CHECK(radius_cells(0.f, 0.25f) == 0 && radius_cells(0.24f, 0.25f) == 0 && radius_cells(0.25f, 0.25f) == 1);
    CHECK(radius_cells(63.5f, 0.25f) == 254 && radius_cells(63.74f, 0.25f) == 254 && radius_cells(63.75f, 0.25f) == 255);
    CHECK(radius_cells(1e30f, 0.25f) == 255 && radius_cells(inf, 0.25f) == 255 && radius_cells(nan, 0.25f) == 255);
    CHECK(radius_cells(-0.1f, 0.25f) == 255);
    lom_clearance_params p = prm(2.f, 0.5f, 1.f, 3);
    CHECK(params_ok(&p, 0.25f) && !params_ok(nullptr, 0.25f));
    p = prm(2.f, 2.f, 0.f);
    CHECK(params_ok(&p, 0.25f));
    p = prm(0.f, 0.f, 0.f);
    CHECK(params_ok(&p, 0.25f));
    const lom_clearance_params bad[] = {prm(2.f, 2.5f, 1.f), prm(2.f, -0.1f, 1.f), prm(2.f, 0.5f, -1.f), prm(nan, 0.5f, 1.f),
                                        prm(2.f, nan, 1.f),  prm(2.f, 0.5f, nan),  prm(inf, 0.5f, 1.f),  prm(2.f, 0.5f, inf),
                                        prm(63.75f, 0.5f, 1.f), prm(2.f, 0.5f, 1.f, 4), prm(-1.f, -2.f, 1.f)};
    for (const lom_clearance_params &b : bad) CHECK(!params_ok(&b, 0.25f));
}

static void test_table()
{
    // R = 254: every entry, the three boundaries, non-increasing
    const float r = 0.25f;
    const lom_clearance_params p = prm(63.5f, 3.0f, 0.1f);
    const uint32_t R = radius_cells(p.inflation_radius, r);
    CHECK(R == 254);
    std::vector<uint8_t> t((size_t)R * R + 1, 0xee);
    cost_table(p, r, R, t.data());
    CHECK(t[0] == 100 && t[1] == 99 && t[144] == 99);  // 12 cells = 3.0 m: dist <= inscribed
    CHECK(t[145] == (uint8_t)std::floor(98.0 * std::exp(-(double)0.1f * (std::sqrt(145.0) * 0.25 - 3.0))) && t[145] <= 98);
    CHECK(t[(size_t)R * R] == (uint8_t)std::floor(98.0 * std::exp(-(double)0.1f * (63.5 - 3.0))));
    for (size_t k = 1; k < t.size(); k++) CHECK(t[k] <= t[k - 1]);
    // an inflation radius between two cells: sqrt(k) r > inflation is 0 even inside R^2 (no such k here: R r <= inflation)
    const lom_clearance_params q = prm(1.1f, 1.1f, 5.f);
    const uint32_t Rq = radius_cells(q.inflation_radius, r);
    CHECK(Rq == 4);
    std::vector<uint8_t> u((size_t)Rq * Rq + 1);
    cost_table(q, r, Rq, u.data());
    CHECK(u[0] == 100);
    for (size_t k = 1; k < u.size(); k++) CHECK(u[k] == 99);  // dist <= 1.0 <= inscribed everywhere
    // a resolution that does not divide: 0.3f * 3 > 0.9f in f64?  whatever the rounding, the order of the rules decides
    const lom_clearance_params w = prm(0.9f, 0.3f, 2.f);
    const uint32_t Rw = radius_cells(w.inflation_radius, 0.3f);
    CHECK(Rw == 2 || Rw == 3);
    std::vector<uint8_t> v((size_t)Rw * Rw + 1);
    cost_table(w, 0.3f, Rw, v.data());
    for (size_t k = 1; k < v.size(); k++) {
        const double d = std::sqrt((double)k) * (double)0.3f;
        if (d <= (double)0.3f) CHECK(v[k] == 99);
        else if (d > (double)0.9f) CHECK(v[k] == 0);
        else CHECK(v[k] <= 98);
    }
    // R = 0: one entry
    uint8_t one = 0;
    cost_table(prm(0.1f, 0.05f, 1.f), r, 0, &one);
    CHECK(one == 100);
}

static void check_cover(const lom_occupancy_geometry &g, const lom_clearance_window *w, uint32_t R, uint32_t T)
{
    const Rect r = clip(w, g);
    const Rect gr = grow(r, R, g);
    if (r.empty()) {
        CHECK(gr.empty() && merge_grid(gr).blocks == 0 && tile_grid(r, R, T).n_wx == 0 && tile_grid(r, R, T).n_ty == 0);
        return;
    }
    CHECK(r.x1 <= g.width && r.y1 <= g.height && gr.x0 <= r.x0 && gr.y0 <= r.y0 && gr.x1 >= r.x1 && gr.y1 >= r.y1);
    CHECK(gr.x1 <= g.width && gr.y1 <= g.height);
    CHECK(gr.x0 == (r.x0 > R ? r.x0 - R : 0) && gr.x1 == (r.x1 + R < g.width ? r.x1 + R : g.width));
    CHECK(gr.y0 == (r.y0 > R ? r.y0 - R : 0) && gr.y1 == (r.y1 + R < g.height ? r.y1 + R : g.height));
    // tiles: every cell of the rectangle exactly once, no tile without a cell of it, every word inside the bitmap row
    const TileGrid t = tile_grid(r, R, T);
    CHECK(t.tile_rows == T && t.lds_bytes == 64u * (T + 2u * R) && t.lds_bytes <= 64u * 540u);
    CHECK(t.wx0 + t.n_wx <= words_per_row(g.width) && t.n_ty <= 65535u && t.n_wx <= 128u);
    std::vector<uint8_t> seen((size_t)(r.x1 - r.x0) * (r.y1 - r.y0), 0);
    for (uint32_t by = 0; by < t.n_ty; by++)
        for (uint32_t bx = 0; bx < t.n_wx; bx++) {
            const uint32_t ty0 = t.y0 + by * T;
            CHECK(ty0 < r.y1);
            const uint32_t rows = T < r.y1 - ty0 ? T : r.y1 - ty0;
            uint32_t cells = 0;
            for (uint32_t row = 0; row < rows; row++)
                for (uint32_t lane = 0; lane < 64; lane++) {
                    const uint32_t x = (t.wx0 + bx) * 64u + lane, y = ty0 + row;
                    if (x >= r.x0 && x < r.x1) seen[(size_t)(y - r.y0) * (r.x1 - r.x0) + (x - r.x0)]++, cells++;
                }
            CHECK(cells > 0);
        }
    for (uint8_t s : seen) CHECK(s == 1);
    // merge waves: every cell of the grown rectangle exactly once
    const MergeGrid m = merge_grid(gr);
    CHECK(m.wx0 + m.n_wx <= words_per_row(g.width) && m.y0 + m.n_rows <= g.height);
    CHECK((uint64_t)m.blocks * kWavesPerBlock >= (uint64_t)m.n_wx * m.n_rows && (uint64_t)(m.blocks - 1) * kWavesPerBlock < (uint64_t)m.n_wx * m.n_rows);
    CHECK(m.wx0 * 64u <= gr.x0 && (m.wx0 + m.n_wx) * 64u >= gr.x1 && m.y0 == gr.y0 && m.n_rows == gr.y1 - gr.y0);
    CHECK((m.wx0 + 1) * 64u > gr.x0 && (m.wx0 + m.n_wx - 1) * 64u < gr.x1);
}

static void test_rectangles()
{
    struct Case {
        uint32_t w, h;
    };
    const Case grids[] = {{1, 1}, {1, 200}, {200, 1}, {45, 37}, {63, 3}, {64, 3}, {65, 3}, {130, 67}, {257, 40}, {8192, 2}, {3, 8192}};
    const uint32_t radii[] = {0, 1, 7, 40, 254};
    for (const Case &c : grids) {
        const lom_occupancy_geometry g = geo(0.1f, c.w, c.h);
        const int W = (int)c.w, H = (int)c.h;
        const lom_clearance_window windows[] = {
            {0, 0, c.w, c.h},          {-5, -5, 7, 7},           {W - 2, H - 2, 9, 9},      {-3, H - 1, 4, 1},
            {W - 1, -1, 1, 2},         {W, 0, 3, 3},             {0, H, 3, 3},              {-9, 0, 9, c.h},
            {0, -9, c.w, 9},           {3, 3, 0, 5},             {3, 3, 5, 0},              {W / 2, H / 2, 1, 1},
            {60, 1, 10, 2},            {63, 0, 2, 40},           {-2147483647 - 1, -2147483647 - 1, 0xffffffffu, 0xffffffffu},
            {2147483647, 2147483647, 0xffffffffu, 0xffffffffu},  {-1, -1, 0xffffffffu, 0xffffffffu}};
        for (uint32_t R : radii)
            for (uint32_t T : {1u, 8u, 32u}) {
                check_cover(g, nullptr, R, T);
                for (const lom_clearance_window &w : windows) check_cover(g, &w, R, T);
            }
        const Rect full = clip(nullptr, g);
        CHECK(full.x0 == 0 && full.y0 == 0 && full.x1 == c.w && full.y1 == c.h && full.cells() == (uint64_t)c.w * c.h);
        const lom_clearance_window all = {-1, -1, 0xffffffffu, 0xffffffffu};
        const Rect a = clip(&all, g);
        CHECK(a.x0 == 0 && a.y0 == 0 && a.x1 == c.w && a.y1 == c.h);
        const lom_clearance_window off = {-2147483647 - 1, 0, 100, 100};
        CHECK(clip(&off, g).empty() && clip(&off, g).cells() == 0);
    }
    // the largest launch shapes: a full 8192 x 8192 grid at T = 1
    const lom_occupancy_geometry big = geo(0.1f, 8192, 8192);
    const Rect r = clip(nullptr, big);
    const TileGrid t = tile_grid(r, 254, 1);
    CHECK(t.n_wx == 128 && t.n_ty == 8192 && t.lds_bytes == 64u * 509u);
    const MergeGrid m = merge_grid(grow(r, 254, big));
    CHECK(m.n_wx == 128 && m.n_rows == 8192 && m.blocks == 128u * 8192u / 4u);
}

int main()
{
    test_ranges();
    test_table();
    test_rectangles();
    return check_done();
}
