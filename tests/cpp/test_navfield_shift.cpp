// The host plan of lom_navfield_shift_resolve* (csrc/navfield_host.cpp: shift_plan, shift_upload_rows) in a program of its
// own, with no HIP header: for every side from 1 to 40 and every shift from -(n + 1) to n + 1 on both axes (the other side
// taken from a short list), the plan against a brute-force count of kept, entered and trailing cells, cell by cell; the
// clamped shift beyond every side; the upload rows against every cell the host form reads.
#include <climits>
#include <cstdio>
#include <vector>

#include "navfield_host.hpp"

using namespace lom;

static long g_plans = 0;

static bool in_rect(const clearance::Rect &r, uint32_t x, uint32_t y) { return x >= r.x0 && x < r.x1 && y >= r.y0 && y < r.y1; }

static bool in_tiles(const navfield::TileRange &t, uint32_t tx, uint32_t ty)
{
    return tx >= t.tx0 && tx < t.tx0 + t.n_tx && ty >= t.ty0 && ty < t.ty0 + t.n_ty;
}

static int check(uint32_t w, uint32_t h, int32_t dx, int32_t dy)
{
    const navfield::ShiftPlan p = navfield::shift_plan(w, h, dx, dy);
    g_plans++;
    if (p.dx > (int32_t)w || p.dx < -(int32_t)w || p.dy > (int32_t)h || p.dy < -(int32_t)h) return 1;
    if (p.n_entered > 2u || p.n_trailing > 2u) return 2;
    if (p.moves() != (dx != 0 || dy != 0)) return 3;
    const navfield::TileGrid tg = navfield::tile_grid(w, h);
    std::vector<uint8_t> tile_has(tg.n_tiles, 0);
    uint64_t kept = 0, entered = 0, trailing = 0;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const int64_t sx = (int64_t)x + dx, sy = (int64_t)y + dy;  // the UNCLAMPED shift decides
            const bool k = sx >= 0 && sx < (int64_t)w && sy >= 0 && sy < (int64_t)h;
            if (k != in_rect(p.kept, x, y)) return 4;
            // the clamped shift gives the same source where there is one
            if (k && ((int64_t)x + p.dx != sx || (int64_t)y + p.dy != sy)) return 5;
            uint32_t n_in = 0;
            for (uint32_t i = 0; i < p.n_entered; i++) n_in += in_rect(p.entered[i], x, y) ? 1u : 0u;
            if (n_in != (k ? 0u : 1u)) return 6;  // every entered cell in exactly one rectangle, no kept cell in any
            kept += k ? 1u : 0u, entered += k ? 0u : 1u;
            const bool t = k && ((dx > 0 && x == 0u) || (dx < 0 && x == w - 1u) || (dy > 0 && y == 0u) || (dy < 0 && y == h - 1u));
            if (t) {
                trailing++;
                tile_has[(y / navfield::kTile) * tg.tiles_x + x / navfield::kTile] = 1;
            }
        }
    if (kept != p.cells_kept || entered != p.cells_entered || trailing != p.trailing_cells) return 7;
    if (p.kept.empty() && (p.kept.x0 | p.kept.y0 | p.kept.x1 | p.kept.y1) != 0u) return 8;
    for (uint32_t ty = 0; ty < tg.tiles_y; ty++)
        for (uint32_t tx = 0; tx < tg.tiles_x; tx++) {
            bool named = false;
            for (uint32_t i = 0; i < p.n_trailing; i++) named = named || in_tiles(p.trailing[i], tx, ty);
            if (named != (tile_has[ty * tg.tiles_x + tx] != 0)) return 9;  // exactly the tiles that hold a trailing cell
        }
    // the upload rows: every row with an entered cell or a cell of the window lies inside, for a few windows
    const lom_occupancy_geometry g{0.25f, 0.f, 0.f, w, h};
    const lom_clearance_window wins[4] = {{0, 0, 0, 0}, {-3, (int32_t)h / 2, 5, 2}, {(int32_t)w - 1, (int32_t)h - 1, 9, 9}, {0, 0, (int32_t)w, 1}};
    for (int i = 0; i < 5; i++) {
        const clearance::Rect r = clearance::clip(i < 4 ? &wins[i] : nullptr, g);
        uint32_t y0 = 77, y1 = 77;
        navfield::shift_upload_rows(p, r, h, &y0, &y1);
        if (y0 > y1 || y1 > h) return 10;
        bool any = false;
        for (uint32_t y = 0; y < h; y++) {
            bool read = false;
            for (uint32_t x = 0; x < w; x++) read = read || !in_rect(p.kept, x, y) || (!r.empty() && in_rect(r, x, y));
            if (read && !(y >= y0 && y < y1)) return 11;
            any = any || read;
        }
        if (!any && (y0 != 0u || y1 != 0u)) return 12;
        if (any && (y0 == y1)) return 13;
    }
    return 0;
}

int main()
{
    const uint32_t others[4] = {1, 7, 33, 40};
    for (uint32_t n = 1; n <= 40; n++)
        for (int32_t d = -(int32_t)(n + 1); d <= (int32_t)(n + 1); d++)
            for (uint32_t m : others)
                for (int32_t e : {0, 1, -1, (int32_t)m - 1, -(int32_t)m, (int32_t)m + 1}) {
                    if (const int rc = check(n, m, d, e)) {
                        std::printf("FAILED %d: %u x %u by (%d, %d)\n", rc, n, m, d, e);
                        return 1;
                    }
                    if (const int rc = check(m, n, e, d)) {
                        std::printf("FAILED %d: %u x %u by (%d, %d)\n", rc, m, n, e, d);
                        return 1;
                    }
                }
    // the full cross on the tile-bordered sides, and shifts beyond every side
    for (int32_t dx = -66; dx <= 66; dx++)
        for (int32_t dy = -34; dy <= 34; dy++)
            if (const int rc = check(65, 33, dx, dy)) {
                std::printf("FAILED %d: 65 x 33 by (%d, %d)\n", rc, dx, dy);
                return 1;
            }
    for (int32_t big : {INT_MAX, INT_MIN, INT_MAX - 1, INT_MIN + 1, 1 << 30})
        for (int32_t small : {0, 1, -1}) {
            if (check(129, 65, big, small) || check(129, 65, small, big) || check(8192, 3, big, big)) {
                std::printf("FAILED: a shift of %d\n", big);
                return 1;
            }
        }
    const navfield::ShiftPlan far = navfield::shift_plan(129, 65, INT_MIN, INT_MAX);
    if (far.dx != -129 || far.dy != 65 || far.cells_kept != 0u || far.n_entered != 1u || far.n_trailing != 0u) return 1;
    std::printf("plans: %ld\nALL PASSED\n", g_plans);
    return 0;
}
