// The navigation field set's host planning (csrc/navset_host.cpp, with csrc/navfield_host.cpp) compiled into a program of
// its own under -fsanitize=address,undefined (tests/test_navset_cpp.py): the offsets rule with every refusal, the field
// index per goal, the sizes and launch shapes at the test shapes and at 4096 x 4096 x 65535 and 8192 x 8192 x 65535 without
// overflow, the report's and the partition's workgroup counts, the refusals of gather and paths, a summary from its words.
#include <cstdio>
#include <cstring>
#include <vector>

#include "check.hpp"
#include "navset_host.hpp"

using namespace lom;
using namespace lom::navset;

static bool refused(const std::vector<uint32_t> &offsets, size_t n_fields, uint32_t max_fields, const void *goals, const char *word)
{
    size_t n_goals = 77;
    const char *why = offsets_refusal(offsets.empty() ? nullptr : offsets.data(), n_fields, max_fields, goals, &n_goals);
    return why && std::strstr(why, word) && n_goals == 0;
}

static void test_offsets()
{
    const int32_t some[2] = {0, 0};
    size_t n_goals = 77;
    CHECK(max_fields_ok(1) && max_fields_ok(65535) && !max_fields_ok(0) && !max_fields_ok(65536) && !max_fields_ok(~0ull));
    // no fields: neither offsets nor goals are read
    CHECK(offsets_refusal(nullptr, 0, 4, nullptr, &n_goals) == nullptr && n_goals == 0);
    // fields without goals, fields that share nothing, an empty field in the middle
    std::vector<uint32_t> o = {0, 0};
    CHECK(offsets_refusal(o.data(), 1, 1, nullptr, &n_goals) == nullptr && n_goals == 0);
    o = {0, 2, 2, 5};
    CHECK(offsets_refusal(o.data(), 3, 3, some, &n_goals) == nullptr && n_goals == 5);
    o = {0, 1u << 24};
    CHECK(offsets_refusal(o.data(), 1, 1, some, &n_goals) == nullptr && n_goals == (size_t)1 << 24);
    // every refusal
    CHECK(refused({0, 1, 2}, 2, 1, some, "max_fields"));
    CHECK(refused({}, 1, 4, some, "n_fields + 1"));
    CHECK(refused({1, 2}, 1, 4, some, "start at 0"));
    CHECK(refused({0, 3, 2}, 2, 4, some, "never fall"));
    CHECK(refused({0, 3, 3, 2}, 3, 4, some, "never fall"));
    CHECK(refused({0, (1u << 24) + 1u}, 1, 4, some, "2^24"));
    CHECK(refused({0, 0xFFFFFFFFu}, 1, 4, some, "2^24"));
    CHECK(refused({0, 1}, 1, 4, nullptr, "goals"));
    // the field of every goal
    o = {0, 2, 2, 5, 5};
    std::vector<uint32_t> of(5, 99);
    field_of_goals(o.data(), 4, of.data());
    CHECK(of == (std::vector<uint32_t>{0, 0, 2, 2, 2}));
    field_of_goals(o.data(), 0, of.data());
}

static void test_sizes_and_shapes()
{
    const uint32_t shapes[][2] = {{1, 1}, {1, 70}, {70, 1}, {32, 32}, {33, 31}, {65, 33}, {129, 65}};
    const uint32_t tiles[][2] = {{1, 1}, {1, 3}, {3, 1}, {1, 1}, {2, 1}, {3, 2}, {5, 3}};
    for (size_t k = 0; k < 7; k++) {
        const uint32_t w = shapes[k][0], h = shapes[k][1];
        for (uint32_t n : {1u, 2u, 5u, 17u}) {
            const Sizes z = sizes(w, h, n);
            CHECK(z.fields == (uint64_t)w * h * 4 * n && z.plane == (uint64_t)w * h);
            CHECK(z.marks == (uint64_t)2 * tiles[k][0] * tiles[k][1] * 4 * n && z.words == ((uint64_t)n * 8 + 2) * 4);
            const RelaxGrid g = relax_grid(w, h, n);
            CHECK(g.x == tiles[k][0] && g.y == tiles[k][1] && g.z == n && g.groups() == (uint64_t)tiles[k][0] * tiles[k][1] * n);
        }
        const uint64_t cells = (uint64_t)w * h;
        CHECK(report_groups(cells) == (cells + 255) / 256 && nearest_groups(cells) == (cells + 255) / 256);  // (all below the caps)
    }
    // the largest: 64-bit throughout
    Sizes z = sizes(4096, 4096, 65535);
    CHECK(z.fields == 4398046511104ull - 67108864ull && z.plane == 16777216ull && z.marks == 2ull * 16384 * 4 * 65535 && z.words == (65535ull * 8 + 2) * 4);
    RelaxGrid g = relax_grid(4096, 4096, 65535);
    CHECK(g.x == 128 && g.y == 128 && g.z == 65535 && g.groups() == 16384ull * 65535);
    z = sizes(8192, 8192, 65535);
    CHECK(z.fields == (uint64_t)8192 * 8192 * 4 * 65535 && z.fields > (1ull << 44) - (1ull << 29) && z.marks == 2ull * 65536 * 4 * 65535);
    g = relax_grid(8192, 8192, 65535);
    CHECK(g.x == 256 && g.y == 256 && g.z <= 65535 && g.groups() == 65536ull * 65535);
    // the report runs a bounded number of workgroups per field, the partition a bounded number in all
    CHECK(report_groups(1) == 1 && report_groups(256) == 1 && report_groups(257) == 2 && report_groups(64 * 256) == 64);
    CHECK(report_groups(64 * 256 + 1) == kReportGroups && report_groups(4096ull * 4096) == kReportGroups && report_groups(8192ull * 8192) == kReportGroups);
    CHECK(report_groups(0) == 1 && nearest_groups(0) == 1);
    CHECK(nearest_groups(2048 * 256) == 2048 && nearest_groups(2048 * 256 + 1) == kNearestGroups && nearest_groups(8192ull * 8192) == kNearestGroups);
}

static void test_gather_and_paths()
{
    const int32_t pts[4] = {0, 0, 1, 1};
    uint32_t out[8];
    CHECK(gather_refusal(LOM_NAV_CELLS, pts, 2, 4, out) == nullptr && gather_refusal(LOM_NAV_METRES, pts, 2, 4, out) == nullptr);
    CHECK(gather_refusal(LOM_NAV_CELLS, nullptr, 0, 4, nullptr) == nullptr);  // no points: nothing to read or write
    CHECK(gather_refusal(LOM_NAV_CELLS, pts, 2, 0, nullptr) == nullptr);     // no fields: nothing to write
    CHECK(gather_refusal(2, pts, 2, 4, out) && gather_refusal(-1, pts, 2, 4, out));
    CHECK(gather_refusal(LOM_NAV_CELLS, nullptr, 2, 4, out) && gather_refusal(LOM_NAV_CELLS, pts, 2, 4, nullptr));
    CHECK(gather_refusal(LOM_NAV_CELLS, pts, ((size_t)1 << 24) + 1, 1, out));
    CHECK(gather_refusal(LOM_NAV_CELLS, pts, (size_t)1 << 24, 16, out) == nullptr && gather_refusal(LOM_NAV_CELLS, pts, (size_t)1 << 24, 17, out));
    CHECK(gather_refusal(LOM_NAV_CELLS, pts, 4097, 65535, out));
    const int32_t which[4] = {0, 3, 1, 3};
    CHECK(path_fields_ok(which, 4, 4) && !path_fields_ok(which, 4, 3) && path_fields_ok(which, 1, 1) && !path_fields_ok(which, 1, 0));
    CHECK(path_fields_ok(nullptr, 0, 0) && !path_fields_ok(nullptr, 1, 4));
    const int32_t negative[2] = {0, -1}, huge[1] = {0x7FFFFFFF};
    CHECK(!path_fields_ok(negative, 2, 4) && !path_fields_ok(huge, 1, 65535));
}

static void test_summary()
{
    const uint32_t words[8] = {700, 0xFFFFFFF0u, 1, 3, 2, 0, 0, 0}, plane_words[2] = {250, 7};
    lom_navfield_summary s{};
    summary_of(words, plane_words, 1000, &s);
    CHECK(s.cells_blocked == 250 && s.cells_invalid == 7 && s.cells_reached == 700 && s.cells_unreached == 50);
    CHECK(s.max_potential == 0xFFFFFFF0u && s.range_exceeded == 1 && s.goals_used == 3 && s.goals_rejected == 2);
    CHECK(s.cells_blocked + s.cells_reached + s.cells_unreached == 1000);
}

int main()
{
    test_offsets();
    test_sizes_and_shapes();
    test_gather_and_paths();
    test_summary();
    return check_done();
}
