// The rule of the grid shift (csrc/plane_geometry.hpp) and its C ABI (csrc/grid_shift_host.cpp) compiled as host code into a
// program of its own under -fsanitize=address,undefined (tests/test_grid_shift_cpp.py), with no HIP header on its include
// path, and run over the table of cases tests/test_grid_shift_host.py walks: the shifted origins' bits and every refusal
// from a file the Python test writes, and lom_grid_follow for every side from 2 to 40, every admissible margin and quantum
// and every cell from -200 to 239 against the shifts tests/grid_shift_ref.py expects.  The C++ mirror's new members are
// compiled against, and its two rule functions are the ones that run.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

#include "check.hpp"
#include "lidar_odometry_amd.hpp"
#include "plane_geometry.hpp"

// every grid of the mirror has shift(dx, dy) (the signature is checked; nothing here needs a device)
template <class G>
constexpr bool has_shift = std::is_same_v<decltype(std::declval<G &>().shift(int32_t(0), int32_t(0))), void>;
static_assert(has_shift<lom::OccupancyGrid> && has_shift<lom::ElevationGrid> && has_shift<lom::ClearanceGrid> && has_shift<lom::NavField> &&
                  has_shift<lom::RegionGrid> && has_shift<lom::VisibilityGrid> && has_shift<lom::RolloutGrid>,
              "a grid of the mirror without shift(dx, dy)");

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

struct ShiftCase {  // as tests/test_grid_shift_cpp.py packs it
    float resolution, origin_x, origin_y;
    uint32_t width, height;
    int32_t dx, dy, status;
    float want_x, want_y;
};
static_assert(sizeof(ShiftCase) == 40, "packed by the Python test");

static void test_shift_cases(std::FILE *f)
{
    uint32_t n = 0;
    CHECK(std::fread(&n, 4, 1, f) == 1);
    std::vector<ShiftCase> cases(n);
    CHECK(std::fread(cases.data(), sizeof(ShiftCase), n, f) == n);
    int ok = 0, range = 0, arg = 0;
    for (const ShiftCase &c : cases) {
        const lom_occupancy_geometry in{c.resolution, c.origin_x, c.origin_y, c.width, c.height};
        const lom_occupancy_geometry sentinel{7.f, 8.f, 9.f, 10, 11};
        lom_occupancy_geometry out = sentinel;
        const int rc = lom_grid_shift_geometry(&in, c.dx, c.dy, &out);
        CHECK(rc == c.status);
        CHECK(rc == lom::plane::shift_geometry(&in, c.dx, c.dy, &out));
        if (rc == LOM_OK) {
            ok++;
            CHECK(same_bits(out.origin_x, c.want_x) && same_bits(out.origin_y, c.want_y));
            CHECK(same_bits(out.resolution, c.resolution) && out.width == c.width && out.height == c.height);
            const lom_occupancy_geometry m = lom::gridShiftGeometry(in, c.dx, c.dy);  // the mirror
            CHECK(std::memcmp(&m, &out, sizeof m) == 0);
            lom_occupancy_geometry self = in;  // in place
            CHECK(lom_grid_shift_geometry(&self, c.dx, c.dy, &self) == LOM_OK && std::memcmp(&self, &out, sizeof self) == 0);
        } else {
            (rc == LOM_ERR_RANGE ? range : arg)++;
            CHECK(std::memcmp(&out, &sentinel, sizeof out) == 0);  // out untouched
            bool threw = false;
            try {
                lom::gridShiftGeometry(in, c.dx, c.dy);
            } catch (const lom::Error &) {
                threw = true;
            }
            CHECK(threw);
        }
    }
    CHECK(ok > 200 && range >= 3 && arg >= 8);
    const lom_occupancy_geometry g{0.25f, -37.5f, -37.5f, 9, 9};
    lom_occupancy_geometry out;
    CHECK(lom_grid_shift_geometry(nullptr, 1, 1, &out) == LOM_ERR_ARG && lom_grid_shift_geometry(&g, 1, 1, nullptr) == LOM_ERR_ARG);
    std::printf("shift cases: %u (%d ok, %d range, %d arg)\n", n, ok, range, arg);
}

// the expected shifts: for n = 2 .. 40, every (quantum, margin) in the Python test's order, 440 int32 for q = -200 .. 239
static void test_follow_table(std::FILE *f)
{
    constexpr int kQ0 = -200, kQ = 440;
    std::vector<int32_t> want(kQ);
    size_t calls = 0;
    for (int geo = 0; geo < 2; geo++) {
        const float r = geo ? 0.1f : 0.25f, o = geo ? -12.3f : -37.5f;
        if (geo) CHECK(std::fseek(f, -(long)(2870 * kQ * 4), SEEK_CUR) == 0);  // the table again
        for (uint32_t n = 2; n <= 40; n++)
            for (uint32_t quantum = 1; quantum <= n / 2; quantum++)
                for (uint32_t margin = 0; margin + quantum <= n / 2; margin++) {
                    CHECK(std::fread(want.data(), 4, kQ, f) == (size_t)kQ);
                    const lom_occupancy_geometry g{r, o, o, n, n};
                    for (int k = 0; k < kQ; k++) {
                        // x: the centre of cell q; y: cell q' (the cells in reverse), on its lower border where that is exact
                        const int q = kQ0 + k, qy = kQ0 + kQ - 1 - k;
                        const double x = (double)o + ((double)q + 0.5) * (double)r;
                        const double y = (double)o + ((double)qy + (geo ? 0.5 : 0.0)) * (double)r;
                        const lom::GridShiftCells s = lom::gridFollow(g, x, y, margin, quantum);
                        CHECK(s.dx == want[k] && s.dy == want[kQ - 1 - k]);
                        const int ax = q - s.dx, ay = qy - s.dy;  // the robot's cell afterwards
                        CHECK(ax >= (int)margin && ax < (int)n - (int)margin && ay >= (int)margin && ay < (int)n - (int)margin);
                        CHECK(s.dx % (int)quantum == 0 && s.dy % (int)quantum == 0);
                        calls++;
                    }
                }
    }
    CHECK(calls == 2u * 2870u * 440u);
    std::printf("follow calls: %zu\n", calls);
}

static void test_follow_refusals()
{
    const lom_occupancy_geometry g{0.25f, -37.5f, -37.5f, 20, 12};
    int32_t dx = 77, dy = 77;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto call = [&](const lom_occupancy_geometry &geo, double x, double y, uint32_t margin, uint32_t quantum) {
        dx = dy = 77;
        const int rc = lom_grid_follow(&geo, x, y, margin, quantum, &dx, &dy);
        if (rc != LOM_OK) CHECK(dx == 0 && dy == 0);
        return rc;
    };
    CHECK(call(g, 0, 0, 2, 4) == LOM_OK && call(g, 0, 0, 3, 4) == LOM_ERR_ARG);
    CHECK(call(g, 0, 0, 0, 0) == LOM_ERR_ARG);
    CHECK(call(g, 0, 0, 0xFFFFFFFFu, 1) == LOM_ERR_ARG && call(g, 0, 0, 1, 0xFFFFFFFFu) == LOM_ERR_ARG);
    lom_occupancy_geometry one = g;
    one.width = 1;
    CHECK(call(one, 0, 0, 0, 1) == LOM_ERR_ARG);
    CHECK(call(g, nan, 0, 1, 1) == LOM_ERR_ARG && call(g, 0, nan, 1, 1) == LOM_ERR_ARG && call(g, inf, 0, 1, 1) == LOM_ERR_ARG &&
          call(g, 0, -inf, 1, 1) == LOM_ERR_ARG);
    lom_occupancy_geometry bad = g;
    bad.resolution = 0.f;
    CHECK(call(bad, 0, 0, 1, 1) == LOM_ERR_ARG);
    bad = g, bad.height = 16385;
    CHECK(call(bad, 0, 0, 1, 1) == LOM_ERR_ARG);
    CHECK(lom_grid_follow(nullptr, 0, 0, 1, 1, &dx, &dy) == LOM_ERR_ARG);
    dy = 5;
    CHECK(lom_grid_follow(&g, 0, 0, 1, 1, nullptr, &dy) == LOM_ERR_ARG && dy == 0);
    dx = 5;
    CHECK(lom_grid_follow(&g, 0, 0, 1, 1, &dx, nullptr) == LOM_ERR_ARG && dx == 0);
    const double far = -37.5 + (1099511627776.0 + 1.0) * 0.25;
    CHECK(call(g, far, 0, 1, 1) == LOM_ERR_RANGE && call(g, 0, -far, 1, 1) == LOM_ERR_RANGE);
    CHECK(call(g, -37.5 + 1099511627776.0 * 0.25, 0, 1, 1) == LOM_ERR_RANGE);  // |q| = 2^40 passes, |d| does not
    CHECK(call(g, 1e308, 0, 1, 1) == LOM_ERR_RANGE);
    const double edge = -37.5 + (2147483647.0 + 10.0 + 0.5) * 0.25;
    CHECK(call(g, edge, -37.0, 1, 1) == LOM_OK && dx == 2147483647 && dy == 0);
    CHECK(call(g, edge + 0.25, -37.0, 1, 1) == LOM_ERR_RANGE);
    CHECK(call(g, -37.5 + (-2147483647.0 + 10.0 + 0.5) * 0.25, -37.0, 1, 1) == LOM_OK && dx == -2147483647);
    CHECK(call(g, -37.5 + (-2147483647.0 + 9.0 + 0.5) * 0.25, -37.0, 1, 1) == LOM_ERR_RANGE);
    // towards zero: n = 20, quantum 4
    CHECK(call(g, -37.5 + (-1 + 0.5) * 0.25, -37.0, 0, 4) == LOM_OK && dx == -8);
    CHECK(call(g, -37.5 + (21 + 0.5) * 0.25, -37.0, 0, 4) == LOM_OK && dx == 8);
    bool threw = false;
    try {
        lom::gridFollow(g, far, 0, 1, 1);
    } catch (const lom::Error &e) {
        threw = e.code == LOM_ERR_RANGE;
    }
    CHECK(threw);
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    test_shift_cases(f);
    test_follow_table(f);
    std::fclose(f);
    test_follow_refusals();
    return check_done();
}
