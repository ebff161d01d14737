// The pose field's move rule (csrc/pose_rule.hpp) and host planning (csrc/posefield_host.cpp, with csrc/navfield_host.cpp
// and csrc/visibility_host.cpp) compiled into a program of its own under -fsanitize=address,undefined
// (tests/test_posefield_cpp.py): the headings, the heading of an angle, the six moves with their conditions, targets and
// weights on small layers, every refusal of the parameter and footprint checks, the stencils of a point, of rectangles and
// of the farthest sample, the tile counts and launch shapes at the test shapes and at 8192 x 8192 without overflow, the
// refusals of a paths call, and the two host-only entry points.
#include <cstdio>
#include <cstring>
#include <vector>

#include "check.hpp"
#include "posefield_host.hpp"

using namespace lom;
using namespace lom::posefield;

static void test_headings()
{
    const int hx[8] = {1, 1, 0, -1, -1, -1, 0, 1}, hy[8] = {0, 1, 1, 1, 0, -1, -1, -1};
    for (uint32_t h = 0; h < 8; h++) {
        CHECK(pose_hx(h) == hx[h] && pose_hy(h) == hy[h] && pose_len(h) == ((h & 1u) ? 7u : 5u));
        CHECK(pose_heading_of_angle(8192u * h) == h && pose_heading_of_angle(8192u * h + 4095u) == h);
        CHECK(pose_heading_of_angle(8192u * h + 4096u) == ((h + 1u) & 7u));
        CHECK(lom_posefield_heading_of_angle(8192u * h + 65536u * 3u) == h);
        CHECK(pose_move_heading(h, POSE_F) == h && pose_move_heading(h, POSE_B) == h);
        CHECK(pose_move_heading(h, POSE_FL) == ((h + 1u) & 7u) && pose_move_heading(h, POSE_SL) == ((h + 1u) & 7u));
        CHECK(pose_move_heading(h, POSE_FR) == ((h + 7u) & 7u) && pose_move_heading(h, POSE_SR) == ((h + 7u) & 7u));
    }
    CHECK(pose_heading_of_angle(65535u) == 0u && pose_heading_of_angle(0xFFFFFFFFu) == 0u && pose_heading_of_angle(61439u) == 7u);
    CHECK(pose_move_sign(POSE_F) == 1 && pose_move_sign(POSE_FL) == 1 && pose_move_sign(POSE_FR) == 1 && pose_move_sign(POSE_SL) == 0 &&
          pose_move_sign(POSE_SR) == 0 && pose_move_sign(POSE_B) == -1);
    int32_t dx, dy;
    pose_sample_cell(0, 0, 32768, 0, &dx, &dy);
    CHECK(dx == 0 && dy == 0);
    pose_sample_cell(127, -128, 32768, 0, &dx, &dy);  // half a cell less one unit stays, half a cell to the other side leaves
    CHECK(dx == 0 && dy == 0);
    pose_sample_cell(128, -129, 32768, 0, &dx, &dy);
    CHECK(dx == 1 && dy == -1);
    pose_sample_cell(16384, -16384, 23170, 23170, &dx, &dy);
    CHECK(dx == 91 && dy == 0);
}

struct Moved {
    bool ok;
    int x, y;
    uint32_t h, w;
};

static Moved moved(const std::vector<uint32_t> &layers, uint32_t width, uint32_t height, const PoseCosts &pc, int x, int y, uint32_t h, uint32_t m)
{
    const PoseLayerCells L{layers.data(), width, height};
    Moved r{false, -9, -9, 99u, 0u};
    r.ok = pose_move(L, pc, x, y, h, L(h, x, y), m, &r.x, &r.y, &r.h, &r.w);
    return r;
}

static void test_moves()
{
    const uint32_t W = 3, Hh = 3, n = W * Hh;
    std::vector<uint32_t> layers(8 * n, 10u);  // every state passable, layer value 10
    const PoseCosts all{20u, 3u, 200u, kPoseFlagSpin | kPoseFlagReverse}, none{20u, 3u, 200u, 0u};
    // from the centre, heading E
    Moved r = moved(layers, W, Hh, all, 1, 1, 0, POSE_F);
    CHECK(r.ok && r.x == 2 && r.y == 1 && r.h == 0 && r.w == 50);
    r = moved(layers, W, Hh, all, 1, 1, 0, POSE_FL);
    CHECK(r.ok && r.x == 2 && r.y == 1 && r.h == 1 && r.w == 70);
    r = moved(layers, W, Hh, all, 1, 1, 0, POSE_FR);
    CHECK(r.ok && r.x == 2 && r.y == 1 && r.h == 7 && r.w == 70);
    r = moved(layers, W, Hh, all, 1, 1, 0, POSE_SL);
    CHECK(r.ok && r.x == 1 && r.y == 1 && r.h == 1 && r.w == 3);
    r = moved(layers, W, Hh, all, 1, 1, 0, POSE_SR);
    CHECK(r.ok && r.x == 1 && r.y == 1 && r.h == 7 && r.w == 3);
    r = moved(layers, W, Hh, all, 1, 1, 0, POSE_B);
    CHECK(r.ok && r.x == 0 && r.y == 1 && r.h == 0 && r.w == 250);
    // the switches
    CHECK(!moved(layers, W, Hh, none, 1, 1, 0, POSE_SL).ok && !moved(layers, W, Hh, none, 1, 1, 0, POSE_SR).ok && !moved(layers, W, Hh, none, 1, 1, 0, POSE_B).ok);
    CHECK(moved(layers, W, Hh, none, 1, 1, 0, POSE_F).ok && moved(layers, W, Hh, none, 1, 1, 0, POSE_FL).ok);
    // a diagonal heading: length 7, and both side cells are tested in the source heading's layer
    r = moved(layers, W, Hh, all, 1, 1, 3, POSE_F);  // NW
    CHECK(r.ok && r.x == 0 && r.y == 2 && r.h == 3 && r.w == 70);
    r = moved(layers, W, Hh, all, 1, 1, 3, POSE_B);
    CHECK(r.ok && r.x == 2 && r.y == 0 && r.h == 3 && r.w == 270);
    layers[3 * n + 1 * W + 0] = 0u;  // L[NW] at (0, 1): a side cell of the step to (0, 2)
    CHECK(!moved(layers, W, Hh, all, 1, 1, 3, POSE_F).ok && !moved(layers, W, Hh, all, 1, 1, 3, POSE_FL).ok);
    CHECK(moved(layers, W, Hh, all, 1, 1, 3, POSE_B).ok);  // the other way has other side cells
    layers[3 * n + 1 * W + 0] = 10u;
    layers[2 * n + 1 * W + 0] = 0u;  // L[N] at (0, 1): another heading's layer does not matter to the side cells
    CHECK(moved(layers, W, Hh, all, 1, 1, 3, POSE_F).ok);
    layers[2 * n + 1 * W + 0] = 10u;
    // the rotation needs the new heading's layer at the target cell
    layers[4 * n + 2 * W + 0] = 0u;  // L[W] at (0, 2)
    CHECK(moved(layers, W, Hh, all, 1, 1, 3, POSE_F).ok && !moved(layers, W, Hh, all, 1, 1, 3, POSE_FL).ok && moved(layers, W, Hh, all, 1, 1, 3, POSE_FR).ok);
    layers[4 * n + 2 * W + 0] = 10u;
    layers[1 * n + 1 * W + 1] = 0u;  // L[NE] at the centre: no spin to the left from E
    CHECK(!moved(layers, W, Hh, all, 1, 1, 0, POSE_SL).ok && moved(layers, W, Hh, all, 1, 1, 0, POSE_SR).ok);
    layers[1 * n + 1 * W + 1] = 10u;
    // the grid's border: nothing leaves it
    CHECK(!moved(layers, W, Hh, all, 2, 1, 0, POSE_F).ok && !moved(layers, W, Hh, all, 0, 1, 0, POSE_B).ok && moved(layers, W, Hh, all, 2, 1, 0, POSE_SL).ok);
    CHECK(!moved(layers, W, Hh, all, 2, 2, 1, POSE_F).ok && moved(layers, W, Hh, all, 2, 2, 1, POSE_B).ok);
    // the weight bound: the greatest layer value and the greatest costs stay below 2^28
    const PoseCosts most{kMaxCost, kMaxCost, kMaxCost, kPoseFlagSpin | kPoseFlagReverse};
    for (uint32_t h = 0; h < 8; h++)
        for (uint32_t m = 0; m < kPoseMoves; m++) {
            const uint32_t w = pose_move_weight(most, h, kMaxCost, m);
            CHECK(w >= 1u && w <= kMaxWeight && w < (1u << 28));
        }
    CHECK(pose_move_weight(PoseCosts{0u, 1u, 0u, 3u}, 0, 1u, POSE_FL) == 5u && pose_move_weight(PoseCosts{0u, 1u, 0u, 3u}, 1, 1u, POSE_SL) == 1u);
}

static lom_posefield_params make(uint32_t turn, uint32_t spin, uint32_t reverse, uint32_t flags)
{
    return lom_posefield_params{lom_navfield_params{50u, 3u, 400u, 98, 0u}, turn, spin, reverse, flags};
}

static void test_params_and_footprints()
{
    lom_posefield_params p = make(0, 0, 0, 0);
    CHECK(params_ok(&p) && !params_ok(nullptr));
    p = make(kMaxCost, kMaxCost, kMaxCost, LOM_POSE_SPIN | LOM_POSE_REVERSE);
    CHECK(params_ok(&p));
    p = make(0, 0, 0, LOM_POSE_REVERSE);
    CHECK(params_ok(&p));
    p = make(0, 1, 0, LOM_POSE_SPIN);
    CHECK(params_ok(&p));
    const lom_posefield_params refused[] = {make(kMaxCost + 1u, 1, 0, 0), make(0, kMaxCost + 1u, 0, 0), make(0, 1, kMaxCost + 1u, 0),
                                            make(0, 0, 0, LOM_POSE_SPIN), make(0, 0, 0, LOM_POSE_SPIN | LOM_POSE_REVERSE), make(0, 1, 0, 4u),
                                            make(0, 1, 0, 1u << 31)};
    for (const lom_posefield_params &r : refused) CHECK(!params_ok(&r));
    p = make(0, 1, 0, 0);
    p.nav.neutral = 0;
    CHECK(!params_ok(&p));
    p = make(0, 1, 0, 0);
    p.nav.max_passable = 99;
    CHECK(!params_ok(&p));
    p = make(0, 1, 0, 0);
    p.nav.flags = 2u;
    CHECK(!params_ok(&p));
    p = make(0, 1, 0, 0);
    p.nav.flags = LOM_NAV_UNKNOWN_PASSABLE, p.nav.unknown_cost = 0;
    CHECK(!params_ok(&p));
    const PoseCosts pc = costs_of(make(1, 2, 3, 2));
    CHECK(pc.turn == 1 && pc.spin == 2 && pc.reverse == 3 && pc.flags == 2);

    const int32_t point[2] = {0, 0}, far[2] = {16384, -16384}, too_far[2] = {16385, 0}, too_low[2] = {0, -16385};
    std::vector<int32_t> many(2 * 1025, 0);
    CHECK(footprint_ok(point, 1) && footprint_ok(far, 1) && footprint_ok(many.data(), 1024));
    CHECK(!footprint_ok(nullptr, 1) && !footprint_ok(point, 0) && !footprint_ok(many.data(), 1025) && !footprint_ok(too_far, 1) && !footprint_ok(too_low, 1));
    Stencils st = stencils(point, 1);
    CHECK(st.first[8] == 8 && st.cells == std::vector<int16_t>(16, 0));
    // a 9 x 3-cell rectangle at half-cell spacing: 27 cells at the axial headings, sorted by (dy, dx)
    std::vector<int32_t> rect;
    for (int x = -1024; x <= 1024; x += 128)
        for (int y = -256; y <= 256; y += 128) rect.push_back(x), rect.push_back(y);
    st = stencils(rect.data(), rect.size() / 2);
    for (uint32_t h = 0; h < 8; h += 2) CHECK(st.count(h) == 27);
    for (uint32_t h = 1; h < 8; h += 2) CHECK(st.count(h) > 27 && st.count(h) < 60);
    CHECK(st.cells[0] == -4 && st.cells[1] == -1 && st.cells[2] == -3 && st.cells[1 + 2 * 26] == 1 && st.cells[2 * 26] == 4);
    const uint32_t n0 = st.first[2];
    CHECK(st.cells[2 * n0] == -1 && st.cells[2 * n0 + 1] == -4);  // heading N: 3 x 9
    for (uint32_t h = 0; h < 8; h++)
        for (uint32_t k = st.first[h] + 1; k < st.first[h + 1]; k++) {
            const int16_t *a = &st.cells[2 * (k - 1)], *b = &st.cells[2 * k];
            CHECK(a[1] < b[1] || (a[1] == b[1] && a[0] < b[0]));  // sorted, distinct
        }
    st = stencils(far, 1);
    CHECK(st.first[8] == 8 && st.cells[0] == 64 && st.cells[1] == -64 && st.cells[2] == kMaxReach && st.cells[3] == 0);
    for (int16_t v : st.cells) CHECK(v >= -kMaxReach && v <= kMaxReach);
    st = stencils(many.data(), 1024);
    CHECK(st.first[8] == 8);  // 1024 equal samples are one cell
    // the entry point
    uint32_t counts[8] = {};
    int32_t cells[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    CHECK(lom_posefield_stencils(rect.data(), rect.size() / 2, cells, 3, counts) == LOM_OK && counts[0] == 27 && cells[0] == -4 && cells[5] == -1 &&
          cells[6] == 9);
    CHECK(lom_posefield_stencils(rect.data(), rect.size() / 2, nullptr, 0, counts) == LOM_OK);
    CHECK(lom_posefield_stencils(rect.data(), rect.size() / 2, nullptr, 1, counts) == LOM_ERR_ARG);
    CHECK(lom_posefield_stencils(rect.data(), rect.size() / 2, cells, 3, nullptr) == LOM_ERR_ARG);
    CHECK(lom_posefield_stencils(too_far, 1, cells, 3, counts) == LOM_ERR_ARG && lom_posefield_stencils(nullptr, 1, cells, 3, counts) == LOM_ERR_ARG);
}

static void test_shapes()
{
    const uint32_t shapes[][2] = {{1, 1}, {1, 70}, {70, 1}, {31, 7}, {32, 8}, {33, 9}, {129, 65}, {4096, 4096}, {8192, 8192}};
    for (const auto &s : shapes) {
        const TileGrid t = tile_grid(s[0], s[1]);
        CHECK(t.tiles_x * kTileX >= s[0] && (t.tiles_x - 1u) * kTileX < s[0] && t.tiles_y * kTileY >= s[1] && (t.tiles_y - 1u) * kTileY < s[1]);
        CHECK(t.n_tiles == t.tiles_x * t.tiles_y);
        const size_t n = (size_t)s[0] * s[1];
        CHECK((size_t)blocks_for(n) * kThreads >= n && ((size_t)blocks_for(n) - 1u) * kThreads < n);
        CHECK(report_groups(n) >= 1u && report_groups(n) <= kReportGroups && report_groups(n) <= blocks_for(n));
        CHECK(n * kPoseHeadings < ((size_t)1 << 32));  // a state index fits 32 bits
    }
    CHECK(tile_grid(8192, 8192).n_tiles == 256u * 1024u && blocks_for(0) == 1u && report_groups(0) == 1u && report_groups(257) == 2u);
    const int32_t starts[3] = {0, 0, 0};
    uint16_t out[3];
    CHECK(paths_ok(starts, 1, out, 1) && paths_ok(nullptr, 0, nullptr, 0) && paths_ok(starts, 1, nullptr, 0));
    CHECK(!paths_ok(nullptr, 1, out, 1) && !paths_ok(starts, 1, nullptr, 1) && !paths_ok(starts, kMaxPoints + 1, out, 1));
    CHECK(!paths_ok(starts, 2, out, kMaxPathStates) && paths_ok(starts, 1, out, kMaxPathStates) && !paths_ok(starts, 1, out, kMaxPathStates + 1));
    CHECK(!paths_ok(starts, 3, out, ~(size_t)0 / 2));
}

int main()
{
    test_headings();
    test_moves();
    test_params_and_footprints();
    test_shapes();
    return check_done();
}
