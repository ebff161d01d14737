// The trajectory rollouts' host planning (csrc/rollout_host.cpp) and the shared rule (csrc/rollout_rule.hpp) compiled into
// a program of its own under -fsanitize=address,undefined (tests/test_rollout_cpp.py): every refusal of the validation at
// its limits, the footprint's reach, the staged window and the launch shapes, the key's bit budget at its extremes, the
// helpers, and -- given a file of vectors written by tests/rollout_ref.py -- the rule on the host against the reference:
// the table, the poses step by step and in closed form, and the pose test.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "check.hpp"
#include "rollout_host.hpp"
#include "rollout_rule.hpp"

using namespace lom;
using namespace lom::rollout;

static lom_rollout_params prm(uint32_t L, uint32_t Tn, int32_t lethal = 100, int32_t unknown = -1, uint32_t min_steps = 0, uint32_t pw = 1,
                              uint32_t cw = 1, uint32_t tw = 0, uint32_t flags = 0)
{
    return lom_rollout_params{L, Tn, lethal, unknown, min_steps, pw, cw, tw, flags};
}

static void test_params()
{
    CHECK(!params_ok(nullptr));
    lom_rollout_params p = prm(1, 1, 1, -1, 0, 0, 0, 0, 0);
    CHECK(params_ok(&p));
    p = prm(8, 128, 100, 98, 1024, 256, 4096, 1u << 20, LOM_ROLLOUT_KEEP_RECORDS);
    CHECK(params_ok(&p));
    for (uint32_t L : {0u, 9u, 0xffffffffu}) CHECK(!params_ok(&(p = prm(L, 1))));
    for (uint32_t Tn : {0u, 129u, 0xffffffffu, 0x20000000u}) CHECK(!params_ok(&(p = prm(8, Tn))));
    for (int32_t lethal : {0, -1, 101, std::numeric_limits<int32_t>::min()}) CHECK(!params_ok(&(p = prm(1, 1, lethal))));
    for (int32_t unknown : {-2, 99, 100, std::numeric_limits<int32_t>::max()}) CHECK(!params_ok(&(p = prm(1, 1, 100, unknown))));
    CHECK(params_ok(&(p = prm(2, 5, 100, -1, 10))) && !params_ok(&(p = prm(2, 5, 100, -1, 11))));
    CHECK(!params_ok(&(p = prm(1, 1, 100, -1, 0, 257))) && !params_ok(&(p = prm(1, 1, 100, -1, 0, 1, 4097))));
    CHECK(!params_ok(&(p = prm(1, 1, 100, -1, 0, 1, 1, (1u << 20) + 1u))) && !params_ok(&(p = prm(1, 1, 100, -1, 0, 1, 1, 0, 2))));
    CHECK(waves_ok(1) && waves_ok(4) && !waves_ok(0) && !waves_ok(2) && !waves_ok(8) && !waves_ok(-1));
}

static void test_inputs()
{
    CHECK(counts_ok(0, 0, 1) && counts_ok(4096, 1024, 1024) && counts_ok(4, 1u << 20, 1) && counts_ok(0, 1u << 20, 1));
    CHECK(!counts_ok(4097, 1, 1) && !counts_ok(1, (1u << 20) + 1, 1) && !counts_ok(5, 1u << 20, 1) && !counts_ok(4096, 1025, 1));
    CHECK(!counts_ok(1, 1, 0) && !counts_ok(1, 1, 1025));
    lom_rollout_state s[2] = {{-(1 << 29), (1 << 29) - 1, 65535}, {0, 0, 0}};
    CHECK(states_ok(s, 2) && states_ok(nullptr, 0) && !states_ok(nullptr, 1));
    for (int i = 0; i < 5; i++) {
        lom_rollout_state bad[2] = {{0, 0, 0}, {0, 0, 0}};
        if (i == 0) bad[1].x = 1 << 29;
        if (i == 1) bad[1].x = -(1 << 29) - 1;
        if (i == 2) bad[1].y = 1 << 29;
        if (i == 3) bad[0].y = std::numeric_limits<int32_t>::min();
        if (i == 4) bad[1].a = 65536;
        CHECK(!states_ok(bad, 2));
    }
    const int32_t fp[6] = {16384, -16384, 0, 0, -16384, 16384};
    CHECK(footprint_ok(fp, 3) && !footprint_ok(nullptr, 1) && !footprint_ok(fp, 0) && !footprint_ok(fp, 1025));
    for (int32_t bad : {16385, -16385, std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max()}) {
        int32_t f2[4] = {0, 0, 0, bad};
        CHECK(!footprint_ok(f2, 2));
        f2[3] = 0, f2[0] = bad;
        CHECK(!footprint_ok(f2, 2));
    }
    const int32_t origin[2] = {0, 0}, one[2] = {256, 0}, diag[2] = {-257, 300};
    CHECK(reach(origin, 1) == 1 && reach(one, 1) == 2 && reach(diag, 1) == 4 && reach(fp, 3) == 129);
}

// the proof behind the window: over every table entry, a sample's cell lies within reach of its pose's cell
static void test_reach_bound(const std::vector<int32_t> &tab)
{
    const int32_t fps[][2] = {{16384, 16384}, {-16384, 16384}, {255, 0}, {256, 1}, {-300, -511}, {0, 0}, {1, -1}};
    for (const auto &f : fps) {
        const uint32_t r = reach(f, 1);
        for (uint32_t b = 0; b < kRolloutTable; b++)
            for (int32_t x : {0, 32767, -1, -32768, 12345}) {
                int32_t px, py;
                rollout_sample_at(x, -x, f[0], f[1], tab[2 * b], tab[2 * b + 1], &px, &py);
                const int32_t dx = (px >> 15) - (x >> 15), dy = (py >> 15) - (-x >> 15);
                if ((uint32_t)std::abs(dx) > r || (uint32_t)std::abs(dy) > r) {
                    CHECK(!"a sample beyond the reach");
                    return;
                }
            }
    }
}

static void test_plan()
{
    lom_rollout_params p = prm(1, 64);
    Plan pl = plan(p, 2, 3, 100, 16, 4, false, false);
    CHECK(pl.steps == 64 && pl.window_side == 133 && pl.eval_threads == 256 && pl.block_candidates == 4 && pl.blocks_x == 25);
    CHECK(pl.lds_bytes == 128 + ((133 * 133 + 15) & ~15u) + 32768 + 128 && pl.fill_blocks == 1 && pl.summary_blocks == 1);
    pl = plan(p, 2, 3, 100, 16, 1, false, true);
    CHECK(pl.window_side == 0 && pl.eval_threads == 64 && pl.block_candidates == 1 && pl.blocks_x == 100 && pl.lds_bytes == 128 + 32768 + 128);
    pl = plan(p, 2, 3, 257, 16, 4, true, false);
    CHECK(pl.window_side == 133 && pl.eval_threads == 256 && pl.block_candidates == 256 && pl.blocks_x == 2 && pl.lds_bytes == 128 + ((133 * 133 + 15) & ~15u));
    // the window at its budget: S + reach = 76 fits, 77 does not
    CHECK(plan(prm(1, 75), 1, 1, 1, 1, 4, false, false).window_side == 153 && plan(prm(1, 76), 1, 1, 1, 1, 4, false, false).window_side == 0);
    // nothing to launch without states or candidates; the largest shapes
    CHECK(plan(p, 1, 0, 5, 1, 4, false, false).blocks_x == 0 && plan(p, 1, 5, 0, 1, 4, false, false).blocks_x == 0);
    pl = plan(prm(8, 128), 129, 4, 1u << 20, 1024, 1, false, false);
    CHECK(pl.steps == 1024 && pl.window_side == 0 && pl.blocks_x == (1u << 20) && pl.lds_bytes == 128 + 32768 + 8192 && pl.lds_bytes <= kLdsLimitBytes);
    pl = plan(prm(1, 1), 75, 4096, 1024, 1024, 4, false, false);
    CHECK(pl.window_side == 153 && pl.lds_bytes <= kLdsLimitBytes && pl.fill_blocks == 16 && pl.summary_blocks == 16 && pl.blocks_x == 256);
    CHECK(blocks_for(0) == 1 && blocks_for(256) == 1 && blocks_for(257) == 2);
}

static void test_key()
{
    const lom_rollout_params hi = prm(8, 128, 100, 98, 0, 256, 4096, 1u << 20);
    lom_rollout_record best{1025, 0, 0, 0, 0, 0, 0, 0}, worst{1, 2, 1025u * 99u, 99, 0, 0, 0, 0xFFFFFFFEu};
    const int64_t s_hi = score(hi, true, 0xFFFFFFFEu, best), s_lo = score(hi, true, 0, worst);
    CHECK(s_hi == 256ll * 0xFFFFFFFEll && s_lo == -256ll * 0xFFFFFFFEll - 4096ll * 1025 * 99 - (1ll << 20) * 1024);
    CHECK(s_hi < (1ll << 41) && s_lo > -(1ll << 41));
    CHECK(key_of(s_lo, (1u << 20) - 1u) != 0 && key_of(s_hi, 0) < (1ull << 62));
    for (int64_t s : {s_lo, (int64_t)-1, (int64_t)0, (int64_t)1, s_hi})
        for (uint32_t k : {0u, 1u, (1u << 20) - 1u}) CHECK(key_score(key_of(s, k)) == s && key_index(key_of(s, k)) == k);
    CHECK(key_of(5, 3) > key_of(4, 0) && key_of(5, 3) > key_of(5, 4) && key_of(5, 3) < key_of(5, 2));
    CHECK(score(hi, false, 7, best) == 0 && admissible(hi, false, 0xFFFFFFFFu, best));
    lom_rollout_params q = prm(1, 4, 100, -1, 3);
    lom_rollout_record r{3, 2, 0, 0, 0, 0, 0, 5};
    CHECK(!admissible(q, true, 1, r));
    r.free_poses = 4;
    CHECK(admissible(q, true, 1, r) && !admissible(q, true, 0xFFFFFFFFu, r));
    r.end_potential = 0xFFFFFFFFu;
    CHECK(!admissible(q, true, 1, r) && admissible(q, false, 1, r));
}

static void test_helpers()
{
    size_t n = 7;
    CHECK(!footprint_rectangle(-1, 0, 0, 1, false, nullptr, 0, &n) && n == 0);
    CHECK(!footprint_rectangle(0, 0, 0, 0, false, nullptr, 0, &n) && !footprint_rectangle(16385, 0, 0, 1, false, nullptr, 0, &n));
    CHECK(!footprint_rectangle(0, 0, 0, 1, false, nullptr, 0, nullptr) && !footprint_rectangle(0, 0, 0, 1, false, nullptr, 1, &n));
    CHECK(!footprint_rectangle(4096, 4096, 4096, 128, false, nullptr, 0, &n));   // 65 x 65
    CHECK(footprint_rectangle(4096, 4096, 4096, 128, true, nullptr, 0, &n) && n == 256);
    CHECK(footprint_rectangle(16384, 16384, 16384, 1 << 30, false, nullptr, 0, &n) && n == 4);
    CHECK(footprint_rectangle(16384, 16384, 16384, INT32_MAX, false, nullptr, 0, &n) && n == 4);  // the counts are summed in 64 bits
    CHECK(footprint_rectangle(0, 0, 0, INT32_MAX, true, nullptr, 0, &n) && n == 1);
    int32_t out[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    CHECK(footprint_rectangle(10, 0, 3, 100, false, out, 3, &n) && n == 4 && out[0] == 0 && out[1] == -3 && out[4] == 10 && out[5] == -3 && out[6] == 9);
    const lom_occupancy_geometry g{0.1f, -5.f, 3.25f, 100, 80};
    lom_rollout_state s{};
    CHECK(state_from_pose(&g, -5.f, 3.25f, 0.f, &s) && s.x == 0 && s.y == 0 && s.a == 0);
    CHECK(state_from_pose(&g, -5.f, 3.25f, -3.14159265f, &s) && s.a == 32768);
    CHECK(!state_from_pose(&g, std::numeric_limits<float>::quiet_NaN(), 0.f, 0.f, &s) && !state_from_pose(&g, 0.f, 1e6f, 0.f, &s));
    CHECK(!state_from_pose(&g, 0.f, 0.f, std::numeric_limits<float>::infinity(), &s) && !state_from_pose(nullptr, 0.f, 0.f, 0.f, &s) &&
          !state_from_pose(&g, 0.f, 0.f, 0.f, nullptr));
    CHECK(state_from_pose(&g, 0.f, 0.f, 1.0e9f, &s) && s.a < 65536 && !state_from_pose(&g, 0.f, 0.f, 3.0e38f, &s));  // beyond llround's range
    lom_rollout_params p = prm(1, 2);
    const int16_t cmd[2] = {100, 1};
    lom_rollout_state st{0, 0, 0}, poses3[3];
    CHECK(poses(&p, &st, cmd, poses3) && poses3[2].x == 200 && poses3[2].a == 2);
    CHECK(!poses(nullptr, &st, cmd, poses3) && !poses(&p, nullptr, cmd, poses3) && !poses(&p, &st, nullptr, poses3) && !poses(&p, &st, cmd, nullptr));
    st.a = 65536;
    CHECK(!poses(&p, &st, cmd, poses3));
}

// ---- the rule against the reference's vectors -------------------------------------------------------------------------------------
static bool read_ints(std::FILE *f, std::vector<long long> &v, size_t n)
{
    v.resize(n);
    for (size_t i = 0; i < n; i++)
        if (std::fscanf(f, "%lld", &v[i]) != 1) return false;
    return true;
}

static void test_vectors(const char *path, const std::vector<int32_t> &tab)
{
    std::FILE *f = std::fopen(path, "r");
    CHECK(f != nullptr);
    if (!f) return;
    std::vector<long long> v;
    CHECK(read_ints(f, v, 1) && v[0] == kRolloutTable && read_ints(f, v, 2 * kRolloutTable));
    bool same = true;
    for (size_t i = 0; i < 2 * kRolloutTable; i++) same = same && v[i] == tab[i];
    CHECK(same);
    CHECK(read_ints(f, v, 1));
    const size_t motions = (size_t)v[0];
    size_t pose_count = 0;
    for (size_t c = 0; c < motions; c++) {
        CHECK(read_ints(f, v, 5));
        const lom_rollout_params p = prm((uint32_t)v[0], (uint32_t)v[1]);
        const lom_rollout_state st{(int32_t)v[2], (int32_t)v[3], (uint32_t)v[4]};
        const uint32_t S = p.segments * p.steps_per_segment;
        CHECK(read_ints(f, v, 2 * p.segments));
        std::vector<int16_t> cmd(v.begin(), v.end());
        std::vector<long long> want;
        CHECK(read_ints(f, want, 3 * (S + 1)));
        std::vector<lom_rollout_state> got(S + 1);
        CHECK(poses(&p, &st, cmd.data(), got.data()));
        bool steps_ok = true, closed_ok = true;
        for (uint32_t t = 0; t <= S; t++) {
            steps_ok = steps_ok && got[t].x == want[3 * t] && got[t].y == want[3 * t + 1] && got[t].a == want[3 * t + 2];
            // the closed form the kernel uses: the angle of pose t, and the step that leads to it from the angle one w back
            int32_t v_in = 0, w_in = 0;
            const int32_t sum = rollout_angle_sum(st.a, cmd.data(), p.segments, p.steps_per_segment, t, &v_in, &w_in);
            closed_ok = closed_ok && ((uint32_t)sum & kRolloutAngleMask) == want[3 * t + 2];
            if (t) {
                const uint32_t b = ((uint32_t)(sum - w_in) & kRolloutAngleMask) >> kRolloutAngleShift;
                closed_ok = closed_ok && want[3 * t] - want[3 * (t - 1)] == rollout_increment(v_in, tab[2 * b]) &&
                            want[3 * t + 1] - want[3 * (t - 1) + 1] == rollout_increment(v_in, tab[2 * b + 1]);
            }
            pose_count++;
        }
        CHECK(steps_ok);
        CHECK(closed_ok);
    }
    CHECK(read_ints(f, v, 1));
    const size_t scenes = (size_t)v[0];
    size_t tests = 0;
    for (size_t c = 0; c < scenes; c++) {
        CHECK(read_ints(f, v, 4));
        const uint32_t w = (uint32_t)v[0], h = (uint32_t)v[1];
        const int32_t lethal = (int32_t)v[2], unknown = (int32_t)v[3];
        CHECK(read_ints(f, v, (size_t)w * h));
        std::vector<int8_t> plane(v.begin(), v.end());
        CHECK(read_ints(f, v, 1));
        const uint32_t F = (uint32_t)v[0];
        CHECK(read_ints(f, v, 2 * F));
        std::vector<int32_t> fp(v.begin(), v.end());
        CHECK(read_ints(f, v, 1));
        const size_t queries = (size_t)v[0];
        bool ok = true;
        for (size_t q = 0; q < queries; q++) {
            CHECK(read_ints(f, v, 5));
            const uint32_t b = (uint32_t)v[2] >> kRolloutAngleShift;
            uint32_t cost = 77;
            const uint32_t code = rollout_pose_test((int32_t)v[0], (int32_t)v[1], tab[2 * b], tab[2 * b + 1], fp.data(), F, w, h, lethal, unknown,
                                                    RolloutPlaneCell{plane.data(), w}, &cost);
            ok = ok && code == v[3] && cost == v[4];
            tests++;
        }
        CHECK(ok);
    }
    std::fclose(f);
    std::printf("vectors: %zu poses, %zu pose tests\n", pose_count, tests);
    CHECK(pose_count > 1000 && tests > 500);
}

int main(int argc, char **argv)
{
    std::vector<int32_t> tab(2 * kRolloutTable);
    table(tab.data());
    CHECK(tab[0] == 32768 && tab[1] == 0 && tab[2 * 1024] == 0 && tab[2 * 1024 + 1] == 32768);
    test_params();
    test_inputs();
    test_reach_bound(tab);
    test_plan();
    test_key();
    test_helpers();
    if (argc > 1) test_vectors(argv[1], tab);
    return check_done();
}
