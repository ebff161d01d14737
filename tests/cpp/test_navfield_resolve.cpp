// The window of a navigation field's re-solve on the host: clearance::clip (csrc/clearance_host.cpp) and
// navfield::tile_range (csrc/navfield_host.cpp) against a count of the tiles that hold a cell of the clipped window.
// Plain C++: no HIP header is on the include path.
#include <cstdio>
#include <initializer_list>

#include "check.hpp"
#include "clearance_host.hpp"
#include "navfield_host.hpp"

using namespace lom;

static void check_window(uint32_t w, uint32_t h, const lom_clearance_window *win)
{
    const lom_occupancy_geometry g{0.25f, 0.f, 0.f, w, h};
    const clearance::Rect r = clearance::clip(win, g);
    const navfield::TileRange t = navfield::tile_range(r);
    const navfield::TileGrid tiles = navfield::tile_grid(w, h);
    if (r.empty()) {
        CHECK(t.n_tx == 0 && t.n_ty == 0);
        return;
    }
    CHECK(t.tx0 + t.n_tx <= tiles.tiles_x && t.ty0 + t.n_ty <= tiles.tiles_y && t.n_tx >= 1 && t.n_ty >= 1);
    // every cell of the window lies in a tile of the range, and the first and last tile of either axis hold one
    for (uint32_t y = r.y0; y < r.y1; y++)
        for (uint32_t x = r.x0; x < r.x1; x++)
            CHECK(x / navfield::kTile >= t.tx0 && x / navfield::kTile < t.tx0 + t.n_tx && y / navfield::kTile >= t.ty0 &&
                  y / navfield::kTile < t.ty0 + t.n_ty);
    CHECK(r.x0 / navfield::kTile == t.tx0 && (r.x1 - 1) / navfield::kTile == t.tx0 + t.n_tx - 1);
    CHECK(r.y0 / navfield::kTile == t.ty0 && (r.y1 - 1) / navfield::kTile == t.ty0 + t.n_ty - 1);
}

int main()
{
    const uint32_t shapes[][2] = {{1, 1}, {1, 70}, {70, 1}, {33, 31}, {65, 33}, {129, 65}};
    for (const auto &s : shapes) {
        check_window(s[0], s[1], nullptr);
        for (int32_t x0 : {-40, -1, 0, 1, 30, 31, 32, 33, 63, 64, 128, 129, 1000})
            for (int32_t y0 : {-3, 0, 31, 32, 64, 65})
                for (uint32_t ww : {0u, 1u, 2u, 32u, 33u, 500u, 0xFFFFFFFFu})
                    for (uint32_t hh : {0u, 1u, 2u, 34u, 0xFFFFFFFFu}) {
                        const lom_clearance_window win{x0, y0, ww, hh};
                        check_window(s[0], s[1], &win);
                    }
    }
    // the 2 x 2 window across the tile corner at (31..32, 31..32) is four tiles; one cell is one
    const lom_occupancy_geometry g{0.25f, 0.f, 0.f, 129, 65};
    const lom_clearance_window corner{31, 31, 2, 2}, cell{32, 32, 1, 1}, outside{129, 0, 5, 5}, far{INT32_MIN, INT32_MIN, 7, 7};
    navfield::TileRange t = navfield::tile_range(clearance::clip(&corner, g));
    CHECK(t.tx0 == 0 && t.ty0 == 0 && t.n_tx == 2 && t.n_ty == 2);
    t = navfield::tile_range(clearance::clip(&cell, g));
    CHECK(t.tx0 == 1 && t.ty0 == 1 && t.n_tx == 1 && t.n_ty == 1);
    CHECK(navfield::tile_range(clearance::clip(&outside, g)).n_tx == 0 && navfield::tile_range(clearance::clip(&far, g)).n_ty == 0);
    t = navfield::tile_range(clearance::clip(nullptr, g));
    CHECK(t.tx0 == 0 && t.ty0 == 0 && t.n_tx == 5 && t.n_ty == 3);
    return check_done();
}
