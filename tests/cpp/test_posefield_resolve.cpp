// posefield::relayer_boxes (csrc/posefield_host.cpp) under -fsanitize=address,undefined (tests/test_posefield_resolve_cpp.py):
// the eight boxes of a re-solve's k_pose_relayer against a brute-force dilation, for five footprints, for changed boxes on
// every border of the grid, for boxes larger than the grid and for grids smaller than a stencil.  Plain C++: no HIP header
// is on the include path.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "check.hpp"
#include "posefield_host.hpp"

using namespace lom;

// xs = -back, -back + spacing, ... while < front, then front; ys likewise: the rectangle lattice of the tests' footprints
static std::vector<int32_t> rectangle(int front, int back, int half, int spacing)
{
    std::vector<int> xs, ys;
    for (int x = -back; x < front; x += spacing) xs.push_back(x);
    xs.push_back(front);
    for (int y = -half; y < half; y += spacing) ys.push_back(y);
    ys.push_back(half);
    std::vector<int32_t> fp;
    for (int x : xs)
        for (int y : ys) fp.push_back(x), fp.push_back(y);
    return fp;
}

static std::vector<std::vector<int32_t>> footprints()
{
    std::vector<std::vector<int32_t>> out;
    out.push_back({0, 0});                               // the point
    out.push_back(rectangle(512, 512, 256, 128));        // 5 x 3 cells
    out.push_back(rectangle(1024, 1024, 256, 128));      // 9 x 3 cells
    std::vector<int32_t> l;                              // the asymmetric L
    for (int x = -256; x <= 1024; x += 128) l.push_back(x), l.push_back(0);
    for (int y = 128; y <= 512; y += 128) l.push_back(-256), l.push_back(y);
    out.push_back(l);
    std::vector<int32_t> big;                            // 1024 samples within a 7 x 5-cell box
    uint32_t s = 12345u;
    for (int i = 0; i < 1024; i++) {
        s = s * 1664525u + 1013904223u;
        const int x = (int)((s >> 8) % 1537u) - 768;
        s = s * 1664525u + 1013904223u;
        big.push_back(x), big.push_back((int)((s >> 8) % 1025u) - 512);
    }
    out.push_back(big);
    std::vector<int32_t> off = {4096, 0, 4352, 0};      // ahead of the centre only: the stencil does not hold (0, 0)
    out.push_back(off);
    return out;
}

static void check_boxes(const posefield::Stencils &st, const PoseBox &changed, uint32_t w, uint32_t h)
{
    const PoseBoxes b = posefield::relayer_boxes(st, changed, w, h);
    const int64_t cx1 = std::min(changed.x1, w), cy1 = std::min(changed.y1, h);
    bool any = false;
    for (uint32_t hd = 0; hd < kPoseHeadings; hd++) {
        // brute force: every cell of the grid some stencil cell of which lies in the changed box
        int64_t x0 = w, y0 = h, x1 = -1, y1 = -1;       // the bounding box of the dilation, before it is clipped
        std::vector<char> hit((size_t)w * h, 0);
        for (int64_t cy = changed.y0; cy < cy1; cy++)
            for (int64_t cx = changed.x0; cx < cx1; cx++)
                for (uint32_t k = st.first[hd]; k < st.first[hd + 1]; k++) {
                    const int64_t x = cx - st.cells[2 * (size_t)k], y = cy - st.cells[2 * (size_t)k + 1];
                    x0 = std::min(x0, x), y0 = std::min(y0, y), x1 = std::max(x1, x), y1 = std::max(y1, y);
                    if (x >= 0 && y >= 0 && x < (int64_t)w && y < (int64_t)h) hit[(size_t)y * w + (size_t)x] = 1;
                }
        const PoseBox &g = b.of[hd];
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++)
                if (hit[(size_t)y * w + x]) CHECK(x >= g.x0 && x < g.x1 && y >= g.y0 && y < g.y1);
        // ... and no wider than the clipped bounding box of the dilation
        const int64_t wx0 = std::max<int64_t>(x0, 0), wy0 = std::max<int64_t>(y0, 0), wx1 = std::min<int64_t>(x1 + 1, w), wy1 = std::min<int64_t>(y1 + 1, h);
        if (wx0 < wx1 && wy0 < wy1) {
            CHECK(g.x0 == wx0 && g.y0 == wy0 && g.x1 == wx1 && g.y1 == wy1);
            CHECK(b.all.x0 <= g.x0 && b.all.y0 <= g.y0 && b.all.x1 >= g.x1 && b.all.y1 >= g.y1);
            any = true;
        } else {
            CHECK(g.empty());
        }
        CHECK(g.x1 <= w && g.y1 <= h);
    }
    CHECK(any == !b.all.empty());
    if (any) {  // the union is tight: each side is some heading's
        bool l = false, r = false, lo = false, hi = false;
        for (const PoseBox &g : b.of)
            if (!g.empty()) l |= g.x0 == b.all.x0, r |= g.x1 == b.all.x1, lo |= g.y0 == b.all.y0, hi |= g.y1 == b.all.y1;
        CHECK(l && r && lo && hi);
    }
}

int main()
{
    const uint32_t shapes[][2] = {{1, 1}, {1, 20}, {40, 1}, {31, 7}, {33, 9}, {65, 17}, {200, 190}};
    for (const std::vector<int32_t> &fp : footprints()) {
        CHECK(posefield::footprint_ok(fp.data(), fp.size() / 2));
        const posefield::Stencils st = posefield::stencils(fp.data(), fp.size() / 2);
        for (const auto &s : shapes) {
            const uint32_t w = s[0], h = s[1];
            const PoseBox boxes[] = {
                {0, 0, 1, 1}, {w - 1, 0, w, 1}, {0, h - 1, 1, h}, {w - 1, h - 1, w, h},  // the corners
                {0, 0, w, 1}, {0, h - 1, w, h}, {0, 0, 1, h}, {w - 1, 0, w, h},          // the borders
                {w / 2, h / 2, w / 2 + 1, h / 2 + 1}, {w / 3, h / 3, w / 3 + 3, h / 3 + 2},
                {0, 0, w, h}, {0, 0, w + 50, h + 70}, {w / 2, h / 2, 4 * w + 9, 3 * h + 5},  // as large as the grid, and larger
                {0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu},
            };
            for (const PoseBox &c : boxes) check_boxes(st, c, w, h);
            // an empty changed box gives empty boxes
            const PoseBoxes e = posefield::relayer_boxes(st, PoseBox{3, 3, 3, 9}, w, h);
            CHECK(e.all.empty());
            for (const PoseBox &g : e.of) CHECK(g.empty());
            const PoseBoxes o = posefield::relayer_boxes(st, PoseBox{w, 0, w + 4, h}, w, h);  // wholly outside
            CHECK(o.all.empty());
        }
    }
    // the point's boxes are the changed box itself
    const int32_t point[2] = {0, 0};
    const PoseBoxes p = posefield::relayer_boxes(posefield::stencils(point, 1), PoseBox{5, 6, 9, 8}, 65, 17);
    for (const PoseBox &g : p.of) CHECK(g.x0 == 5 && g.y0 == 6 && g.x1 == 9 && g.y1 == 8);
    CHECK(p.all.x0 == 5 && p.all.y0 == 6 && p.all.x1 == 9 && p.all.y1 == 8);
    return check_done();
}
