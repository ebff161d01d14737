// The region grid's host planning (csrc/regions_host.cpp) compiled into a program of its own under
// -fsanitize=address,undefined (tests/test_regions_cpp.py): the value checks, the word, tile and lane counts at widths 1,
// 63, 64, 65 and 8192, the centroid rounding at the half and the list sort with ties.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "check.hpp"
#include "regions_host.hpp"

using namespace lom;
using namespace lom::regions;

static lom_occupancy_geometry geo(float r, uint32_t w, uint32_t h) { return lom_occupancy_geometry{r, -1.f, 2.f, w, h}; }
static lom_regions_params prm(int kind, int lo, int hi, int max_cost, uint32_t min_cells, int rank, uint32_t flags = 0)
{
    return lom_regions_params{kind, (int8_t)lo, (int8_t)hi, (int8_t)max_cost, min_cells, rank, flags};
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
        g.origin_x = bad == 0.f || bad == -1.f ? nan : bad;
        CHECK(!geometry_ok(&g));
    }
    CHECK(!params_ok(nullptr, true));
    lom_regions_params p = prm(LOM_REGIONS_BYTES, 0, 0, 0, 1, LOM_REGIONS_RANK_LABEL);
    CHECK(params_ok(&p, false) && params_ok(&p, true));
    for (int kind : {-1, 2, 77}) {
        p = prm(kind, 0, 0, 0, 1, 0);
        CHECK(!params_ok(&p, true));
    }
    // lo <= hi under BYTES; neither is read under FRONTIER
    p = prm(LOM_REGIONS_BYTES, -128, 127, 99, 1, 0);
    CHECK(params_ok(&p, false));
    p = prm(LOM_REGIONS_BYTES, 5, 4, 99, 1, 0);
    CHECK(!params_ok(&p, false));
    p = prm(LOM_REGIONS_FRONTIER, 5, 4, 99, 1, 0);
    CHECK(params_ok(&p, false));
    for (int mc : {-128, -1, 100, 127}) {
        p = prm(LOM_REGIONS_FRONTIER, 0, 0, mc, 1, 0);
        CHECK(!params_ok(&p, true));
    }
    for (int mc : {0, 50, 99}) {
        p = prm(LOM_REGIONS_FRONTIER, 0, 0, mc, 1, 0);
        CHECK(params_ok(&p, true));
    }
    p = prm(LOM_REGIONS_FRONTIER, 0, 0, 99, 0, 0);
    CHECK(!params_ok(&p, true));
    p = prm(LOM_REGIONS_FRONTIER, 0, 0, 99, 0xffffffffu, 0);
    CHECK(params_ok(&p, true));
    for (int rank : {-1, 3, 100}) {
        p = prm(LOM_REGIONS_FRONTIER, 0, 0, 99, 1, rank);
        CHECK(!params_ok(&p, true));
    }
    p = prm(LOM_REGIONS_FRONTIER, 0, 0, 99, 1, LOM_REGIONS_RANK_CELLS);
    CHECK(params_ok(&p, false));
    p = prm(LOM_REGIONS_FRONTIER, 0, 0, 99, 1, LOM_REGIONS_RANK_POTENTIAL);
    CHECK(params_ok(&p, true) && !params_ok(&p, false));
    for (uint32_t f = 0; f < 8u; f++) {
        p = prm(LOM_REGIONS_FRONTIER, 0, 0, 99, 1, 0, f);
        CHECK(params_ok(&p, false));
    }
    for (uint32_t f : {8u, 9u, 0x80000000u, 0xffffffffu}) {
        p = prm(LOM_REGIONS_FRONTIER, 0, 0, 99, 1, 0, f);
        CHECK(!params_ok(&p, false));
    }
    CHECK(tile_rows_ok(1) && tile_rows_ok(8) && tile_rows_ok(32));
    for (int64_t bad : {0, -1, 2, 16, 33, 64, 1 << 20}) CHECK(!tile_rows_ok(bad));
}

static void test_plan()
{
    const struct {
        uint32_t width, words, tiles, row_blocks;
    } cases[] = {{1, 1, 1, 1}, {63, 1, 1, 1}, {64, 1, 1, 1}, {65, 2, 2, 1}, {256, 4, 4, 1}, {257, 5, 5, 2}, {8192, 128, 128, 32}};
    for (const auto &c : cases)
        for (uint32_t height : {1u, 7u, 8u, 9u, 32u, 33u, 65u, 8192u})
            for (uint32_t rows : {1u, 8u, 32u}) {
                const Plan p = plan(c.width, height, rows, false);
                CHECK(p.words_per_row == c.words && p.words == c.words * height && p.row_blocks == c.row_blocks);
                CHECK(p.row_blocks * kThreads >= p.words_per_row * 64u && (p.row_blocks - 1u) * kThreads < p.words_per_row * 64u);
                CHECK(p.tiles_x == c.tiles && p.tile_cols == 64u && p.tile_rows == rows);
                CHECK((p.bands - 1u) * kBandRows < height && p.bands * kBandRows >= height);
                // every row lies in exactly one tile row, and the last is not empty
                CHECK((p.tiles_y - 1u) * rows < height && p.tiles_y * rows >= height);
                CHECK(p.n_tiles == p.tiles_x * p.tiles_y);
                CHECK(p.row_lanes == (uint64_t)(p.tiles_y - 1u) * c.width && p.col_lanes == (uint64_t)(p.tiles_x - 1u) * height);
                CHECK(p.scan_blocks >= 1u && p.scan_blocks <= 1024u && (uint64_t)p.scan_blocks * kScanWords >= p.words &&
                      (uint64_t)(p.scan_blocks - 1u) * kScanWords < p.words);
                // without the tile pass every cell is a tile of the merge
                const Plan q = plan(c.width, height, rows, true);
                CHECK(q.n_tiles == 0u && q.tile_cols == 1u && q.tile_rows == 1u && q.tiles_x == c.width && q.tiles_y == height);
                CHECK(q.row_lanes == (uint64_t)(height - 1u) * c.width && q.col_lanes == (uint64_t)(c.width - 1u) * height);
                CHECK(q.words == p.words && q.row_blocks == p.row_blocks);
                CHECK(q.row_lanes + q.col_lanes < (1ull << 27));  // a lane index fits a u32
            }
    const Plan big = plan(8192, 8192, 32, false);
    CHECK(big.words == (1u << 20) && big.scan_blocks == 1024u && big.n_tiles == 128u * 256u);
    const Plan one = plan(1, 1, 32, false);
    CHECK(one.row_lanes == 0u && one.col_lanes == 0u && one.n_tiles == 1u);
    CHECK(blocks_for(0) == 1u && blocks_for(1) == 1u && blocks_for(256) == 1u && blocks_for(257) == 2u);
    CHECK(record_cap(kMaxRegionsDefault, 8192, 8192) == (1u << 20) && record_cap(kMaxRegionsDefault, 129, 65) == (129u * 65u + 1u) / 2u);
    CHECK(record_cap(3, 129, 65) == 3u && record_cap(1, 1, 1) == 1u && record_cap(kMaxRegionsMax, 8192, 8192) == (1u << 25));
    CHECK(record_cap(~0ull, 8192, 8192) == (1u << 25) && record_cap(5, 3, 3) == 5u && record_cap(6, 3, 3) == 5u);
}

static void test_centroid()
{
    // floor((2 sum + cells) / (2 cells)): the mean to nearest, a half upwards
    CHECK(centroid(0, 1) == 0u && centroid(8191, 1) == 8191u);
    CHECK(centroid(0, 2) == 0u && centroid(1, 2) == 1u && centroid(2, 2) == 1u && centroid(3, 2) == 2u);
    CHECK(centroid(4, 3) == 1u && centroid(5, 3) == 2u && centroid(7, 3) == 2u);  // 1.33, 1.67, 2.33
    CHECK(centroid(9, 6) == 2u && centroid(8, 6) == 1u);                           // 1.5 up, 1.33 down
    // the largest sums: a full grid's
    const uint64_t cells = 8192ull * 8192ull, sum = 8192ull * (8191ull * 8192ull / 2ull);
    CHECK(centroid(sum, (uint32_t)cells) == 4096u);  // the mean is 4095.5
    CHECK(centroid(8191ull * cells, (uint32_t)cells) == 8191u);
}

static lom_regions_record rec(uint32_t label, uint32_t cells, uint32_t entry_potential)
{
    lom_regions_record r{};
    r.label = label, r.cells = cells, r.entry_potential = entry_potential;
    return r;
}

static void test_sort()
{
    // in ascending label order, as the device leaves them
    const std::vector<lom_regions_record> r = {rec(3, 5, 900), rec(10, 9, 100), rec(11, 5, 100), rec(40, 1, 0xffffffffu),
                                               rec(41, 9, 50),  rec(90, 5, 900), rec(95, 2, 0)};
    std::vector<uint32_t> order;
    CHECK(sort_list(r.data(), r.size(), 1, LOM_REGIONS_RANK_LABEL, order) && order == (std::vector<uint32_t>{0, 1, 2, 3, 4, 5, 6}));
    CHECK(sort_list(r.data(), r.size(), 1, LOM_REGIONS_RANK_CELLS, order) && order == (std::vector<uint32_t>{1, 4, 0, 2, 5, 6, 3}));
    CHECK(sort_list(r.data(), r.size(), 1, LOM_REGIONS_RANK_POTENTIAL, order) && order == (std::vector<uint32_t>{6, 4, 1, 2, 0, 5, 3}));
    CHECK(sort_list(r.data(), r.size(), 5, LOM_REGIONS_RANK_CELLS, order) && order == (std::vector<uint32_t>{1, 4, 0, 2, 5}));
    CHECK(sort_list(r.data(), r.size(), 6, LOM_REGIONS_RANK_POTENTIAL, order) && order == (std::vector<uint32_t>{4, 1}));
    CHECK(sort_list(r.data(), r.size(), 10, LOM_REGIONS_RANK_LABEL, order) && order.empty());
    CHECK(sort_list(r.data(), 0, 1, LOM_REGIONS_RANK_CELLS, order) && order.empty());
    CHECK(sort_list(nullptr, 0, 1, LOM_REGIONS_RANK_LABEL, order) && order.empty());
    CHECK(!sort_list(r.data(), r.size(), 1, 3, order) && order.empty() && !sort_list(r.data(), r.size(), 1, -1, order));
}

int main()
{
    test_ranges();
    test_plan();
    test_centroid();
    test_sort();
    return check_done();
}
