// Host driver's replay fold under the sanitizers: a stand-alone program (host code only, never loaded into Python).
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tests/cpp/test_replay_fold_host.cpp lidar_odometry_demo_amd/csrc/align_driver.cpp -o /tmp/replay_fold_host
//   /tmp/replay_fold_host
// The stub evaluator is a scan without correspondences: every sum is zero, the prior alone is solved (gradient 0 at the
// guess: the solve ends at once) and the pose stays at the guess -- so iteration 1 searches at iteration 0's pose, the
// driver folds iterations 2..4 and the reference's count, 5, is what it reports.
#include <cstdio>
#include <cstring>

#include "lidar_odometry_amd.h"

static int g_match_calls = 0, g_fixed_calls = 0;
static const double kQueries = 1000.0;

static int match_eval(void *, const float *, const float *, const double *, const double *, double *sums)
{
    g_match_calls++;
    std::memset(sums, 0, LOM_NSUMS * sizeof(double));
    sums[31] = kQueries;
    return 0;
}

static int eval_fixed(void *, const double *, const double *, double *sums)
{
    g_fixed_calls++;
    std::memset(sums, 0, LOM_NSUMS * sizeof(double));
    sums[31] = kQueries;
    return 0;
}

static int run(int fold, lom_align_stats *st, float t[3], float q[4])
{
    lom_align_hooks hooks;
    std::memset(&hooks, 0, sizeof hooks);
    hooks.match_eval = match_eval;
    hooks.eval_fixed = eval_fixed;
    const float gt[3] = {1.f, 2.f, 3.f}, gq[4] = {1.f, 0.f, 0.f, 0.f};
    g_match_calls = g_fixed_calls = 0;
    lom_debug_set_host_replay_fold(fold);
    return lom_align_with_hooks(&hooks, gt, gq, t, q, st);
}

int main()
{
    lom_align_stats off, on;
    float t0[3], q0[4], t1[3], q1[4];
    if (run(0, &off, t0, q0) != LOM_OK) return 1;
    const int calls_off = g_match_calls;
    if (run(1, &on, t1, q1) != LOM_OK) return 2;
    const int calls_on = g_match_calls;
    std::printf("outer %d / %d, searches %d / %d\n", off.outer_iterations, on.outer_iterations, calls_off, calls_on);
    if (off.outer_iterations != 5 || calls_off != 5) return 3;
    if (on.outer_iterations != 5 || calls_on != 2) return 4;
    if (std::memcmp(&off, &on, sizeof off) != 0) return 5;
    if (std::memcmp(t0, t1, sizeof t0) != 0 || std::memcmp(q0, q1, sizeof q0) != 0) return 6;
    for (int outer = 1; outer <= 35; outer++)
        if (outer + lom_debug_replay_fold_count(outer, 0.0) != (outer < 5 ? 5 : outer) ||
            outer + lom_debug_replay_fold_count(outer, 1.0) != 35)
            return 7;
    std::puts("ok");
    return 0;
}
