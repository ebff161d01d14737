// The visibility grid's host planning (csrc/visibility_host.cpp) compiled into a program of its own under
// -fsanitize=address,undefined (tests/test_visibility_cpp.py): the value checks at every limit, the direction table at
// B = 4, 360 and 8192, the window sizes at R = 0, 15, 16 and 254, the launch shapes and the key's bit budget at its extremes.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "check.hpp"
#include "visibility_host.hpp"

using namespace lom;
using namespace lom::visibility;

static lom_occupancy_geometry geo(float r, uint32_t w, uint32_t h) { return lom_occupancy_geometry{r, -1.f, 2.f, w, h}; }
static lom_visibility_params prm(uint32_t beams, uint32_t range, int32_t block_min, uint32_t depth, uint32_t flags = 0)
{
    return lom_visibility_params{beams, range, block_min, depth, flags};
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
    lom_visibility_params p = prm(4, 0, 1, 0);
    CHECK(params_ok(&p));
    p = prm(8192, 254, 100, 65535, LOM_VIS_KEEP_WINDOWS | LOM_VIS_KEEP_BEAMS);
    CHECK(params_ok(&p));
    for (uint32_t beams : {0u, 3u, 8193u, 0xffffffffu}) {
        p = prm(beams, 10, 100, 0);
        CHECK(!params_ok(&p));
    }
    for (uint32_t range : {255u, 256u, 0xffffffffu}) {
        p = prm(64, range, 100, 0);
        CHECK(!params_ok(&p));
    }
    for (int32_t block_min : {0, -1, 101, 127, std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max()}) {
        p = prm(64, 10, block_min, 0);
        CHECK(!params_ok(&p));
    }
    for (uint32_t depth : {65536u, 0xffffffffu}) {
        p = prm(64, 10, 100, depth);
        CHECK(!params_ok(&p));
    }
    for (uint32_t flags : {4u, 8u, 0x80000000u, 0xffffffffu}) {
        p = prm(64, 10, 100, 0, flags);
        CHECK(!params_ok(&p));
    }
    CHECK(!select_ok(nullptr));
    lom_visibility_select_params s{1, 1, 0, 1};
    CHECK(select_ok(&s));
    s = lom_visibility_select_params{1024, 4096, 31, 0xffffffffu};
    CHECK(select_ok(&s));
    for (const lom_visibility_select_params bad : {lom_visibility_select_params{0, 1, 0, 1}, lom_visibility_select_params{1025, 1, 0, 1},
                                                   lom_visibility_select_params{1, 0, 0, 1}, lom_visibility_select_params{1, 4097, 0, 1},
                                                   lom_visibility_select_params{1, 1, 32, 1}, lom_visibility_select_params{1, 1, 0, 0}})
        CHECK(!select_ok(&bad));
    CHECK(waves_ok(1) && waves_ok(4) && !waves_ok(0) && !waves_ok(2) && !waves_ok(8) && !waves_ok(-1));
}

static void test_table()
{
    std::vector<int32_t> t(2 * 8192 + 2, 77);
    CHECK(!table(3, t.data()) && !table(8193, t.data()) && !table(0, t.data()) && !table(64, nullptr));
    CHECK(t[0] == 77);
    CHECK(table(4, t.data()));
    const int32_t four[8] = {32768, 0, 0, 32768, -32768, 0, 0, -32768};
    for (int i = 0; i < 8; i++) CHECK(t[i] == four[i]);
    CHECK(t[8] == 77);  // nothing past 2 * beams
    for (uint32_t beams : {360u, 8192u}) {
        std::fill(t.begin(), t.end(), 77);
        CHECK(table(beams, t.data()));
        CHECK(t[2 * beams] == 77 && t[0] == 32768 && t[1] == 0);
        const uint32_t q = beams / 4;
        CHECK(t[2 * q] == 0 && t[2 * q + 1] == 32768 && t[4 * q] == -32768 && t[4 * q + 1] == 0 && t[6 * q] == 0 && t[6 * q + 1] == -32768);
        for (uint32_t b = 0; b < beams; b++) {
            const int64_t dx = t[2 * b], dy = t[2 * b + 1], n2 = dx * dx + dy * dy;
            // a rounded point of the circle of radius 32768: within 1 of it
            CHECK(n2 >= (int64_t)32767 * 32767 && n2 <= (int64_t)32769 * 32769);
            // the table is symmetric under a half turn
            const uint32_t o = (b + beams / 2) % beams;
            CHECK(t[2 * o] == -dx && t[2 * o + 1] == -dy);
            // (2 i + 1) * |d| at the last step of the longest walk fits 24 bits
            CHECK((uint64_t)(2 * 255 + 1) * (uint64_t)std::max(dx < 0 ? -dx : dx, dy < 0 ? -dy : dy) < (1ull << 24));
        }
    }
    // B = 360: beam 45 is the exact diagonal, beam 30 is (cos 30, sin 30)
    CHECK(table(360, t.data()));
    CHECK(t[90] == 23170 && t[91] == 23170 && t[60] == 28378 && t[61] == 16384);
}

static void test_windows_and_shapes()
{
    Window w = window(0);
    CHECK(w.side == 1 && w.words_per_row == 1 && w.words == 1 && w.bytes == 4);
    w = window(15);
    CHECK(w.side == 31 && w.words_per_row == 1 && w.words == 31 && w.bytes == 124);
    w = window(16);
    CHECK(w.side == 33 && w.words_per_row == 2 && w.words == 66 && w.bytes == 264);
    w = window(254);
    CHECK(w.side == 509 && w.words_per_row == 16 && w.words == 8144 && w.bytes == 32576);
    CHECK(windows_bytes(0, 254) == 0 && windows_bytes(1, 0) == 4);
    CHECK(windows_bytes(kMaxViewpoints, 254) == (uint64_t)32576 << 20);  // no wrap at the greatest cast
    CHECK(windows_bytes(8241, 254) > kMaxWindowBytesDefault && windows_bytes(8240, 254) <= kMaxWindowBytesDefault);
    CHECK(blocks_for(0) == 1 && blocks_for(1) == 1 && blocks_for(256) == 1 && blocks_for(257) == 2 && blocks_for(1u << 20) == 4096);
    Plan p = plan(1, 1, 0, 4, false, 0);
    CHECK(p.cast_threads == 256 && p.lds_bytes == 128 + 16 && p.summary_blocks == 1 && p.cover_blocks == 1 && p.covered_words_per_row == 1 &&
          p.covered_words == 1 && p.fill_blocks == 1);
    p = plan(8192, 8192, 254, 1, false, kMaxViewpoints);
    CHECK(p.cast_threads == 64 && p.lds_bytes == 128 + 32576 && p.lds_bytes % 16 == 0 && p.lds_bytes <= 64 * 1024);
    CHECK(p.summary_blocks == 4096 && p.cover_blocks == 32 && p.covered_words_per_row == 256 && p.covered_words == 256u * 8192u && p.fill_blocks == 8192);
    p = plan(33, 31, 31, 4, true, 300);
    CHECK(p.lds_bytes == 128 && p.win.words == 63 * 2 && p.covered_words_per_row == 2 && p.covered_words == 62 && p.summary_blocks == 2);
    p = plan(32, 5, 40, 4, false, 1);
    CHECK(p.covered_words_per_row == 1 && p.win.words_per_row == 3 && p.lds_bytes == 128 + ((81 * 3 * 4 + 15) & ~15));
}

static void test_key()
{
    // the extremes of the score: the greatest gain at the greatest weight and no cost; no gain... (min_gain >= 1) and the dearest cost
    const uint32_t g_max = 509u * 509u;
    const int64_t s_hi = score(g_max, 4096, 0, 0), s_lo = score(1, 1, 0xFFFFFFFEu, 0);
    CHECK(s_hi == (int64_t)g_max * 4096 && s_hi <= ((int64_t)1 << 30) && s_lo == 1 - (int64_t)0xFFFFFFFEu);
    CHECK(score(10, 3, 0xFFFFFFFFu, 31) == 29 && score(10, 3, 1000, 3) == 30 - 125);
    const uint32_t k_max = (uint32_t)kMaxViewpoints - 1u;
    for (int64_t s : {s_lo, (int64_t)-1, (int64_t)0, (int64_t)1, s_hi}) {
        for (uint32_t k : {0u, 1u, k_max}) {
            const uint64_t key = key_of(s, k);
            CHECK(key != 0 && key < (1ull << 53) && key_index(key) == k && key_score(key) == s);
        }
        // a greater score wins whatever the index; at equal scores the least index wins
        CHECK(key_of(s, 0) > key_of(s, 1) && key_of(s, 1) > key_of(s, k_max));
        if (s < s_hi) CHECK(key_of(s + 1, k_max) > key_of(s, 0));
    }
    CHECK(key_of(s_lo, k_max) >= (1ull << kKeyIndexBits));  // the least key of all is above "no candidate"
}

int main()
{
    test_ranges();
    test_table();
    test_windows_and_shapes();
    test_key();
    return check_done();
}
