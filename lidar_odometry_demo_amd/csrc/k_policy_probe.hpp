// lom_debug_lm_policy: the wave forms of the LM policy (lm_wave.hpp) on GIVEN sums -- no map, no scan, no search.
// One 64-lane workgroup replays every solve of the call: per evaluation the 32 totals and, for evaluation 0, the start
// point go to LDS (where k_lm holds s_tot and s_x), the policy runs exactly as k_lm calls it (begin or feed, then
// propose when asked), and the action and the point it leaves behind are written out.  A solve's replay ends with its
// first LM_DONE; evaluations not replayed keep the caller's -1 / zeros.
//   kForm 1: lmw_*          (LmState in LDS, v_readlane broadcasts)
//   kForm 2: lmw2_*<false>  (k_lm's 512-thread shape: row state in registers, the rest in LDS)
//   kForm 3: lmw2_*<true>   (k_lm's 256-thread shape: all state in registers)
// The checker is tests/test_lm_policy_gpu.py (against tests/lm_ref.py); tools/microbench/policy.hip times the same code.
#pragma once
#include <hip/hip_runtime.h>

#include "lm_wave.hpp"

namespace lom {

constexpr int kProbeMaxEvals = 5;  // iteration 0 + max_num_iterations candidates

struct PolicyProbeArgs {
    int n_solves;
    const int *n_evals;      // [n_solves], 1..kProbeMaxEvals
    const double *x0;        // [n_solves][7]
    const double *prior_b;   // [n_solves][3]
    const double *sums;      // [n_solves][kProbeMaxEvals][32]
    int *action;             // [n_solves][kProbeMaxEvals]
    double *point;           // [n_solves][kProbeMaxEvals][7]: LM_EVAL the candidate, LM_DONE the solution
    int *recorded, *evaluations;        // [n_solves]
    double *last_step_norm, *cost;      // [n_solves]
};

template <int kForm>
__global__ __launch_bounds__(64) void k_policy_probe(PolicyProbeArgs p)
{
    __shared__ LmState s_lm;
    __shared__ LmShared s_sh;
    __shared__ double s_tot[32], s_x[7], s_done[7];
    const int lane = threadIdx.x;
    LmWave W;
    LmShared r_sh;
    for (int s = 0; s < p.n_solves; s++) {
        const double *prior_b = p.prior_b + (size_t)s * 3;
        const int ne = p.n_evals[s];
        for (int e = 0; e < ne && e < kProbeMaxEvals; e++) {
            const size_t slot = (size_t)s * kProbeMaxEvals + e;
            if (lane < 32) s_tot[lane] = p.sums[slot * 32 + lane];
            if (lane < 7 && e == 0) s_x[lane] = p.x0[(size_t)s * 7 + lane];
            __syncthreads();
            int a;
            if constexpr (kForm == 1) {
                a = e == 0 ? lmw_begin(s_lm, s_tot, s_x, prior_b, lane) : lmw_feed(s_lm, s_tot, lane);
                if (a == LM_PROPOSE) a = lmw_propose(s_lm, lane);
                if (lane < 7) {
                    s_x[lane] = s_lm.cand[lane];
                    s_done[lane] = s_lm.x[lane];
                }
            } else if constexpr (kForm == 2) {
                a = e == 0 ? lmw2_begin<false>(W, s_sh, s_tot, s_x, prior_b, lane)
                           : lmw2_feed<false>(W, s_sh, s_tot, s_x, prior_b, lane);
                if (a == LM_PROPOSE) a = lmw2_propose<false>(W, s_sh, s_x, lane);
                if (lane < 7) s_done[lane] = s_sh.x[lane];
            } else {
                a = e == 0 ? lmw2_begin<true>(W, r_sh, s_tot, s_x, prior_b, lane)
                           : lmw2_feed<true>(W, r_sh, s_tot, s_x, prior_b, lane);
                if (a == LM_PROPOSE) a = lmw2_propose<true>(W, r_sh, s_x, lane);
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < 7; i++) s_done[i] = r_sh.x[i];
                }
            }
            a = __builtin_amdgcn_readfirstlane(a);
            __syncthreads();
            if (lane < 7) p.point[slot * 7 + lane] = a == LM_EVAL ? s_x[lane] : s_done[lane];
            if (lane == 0) p.action[slot] = a;
            __syncthreads();
            if (a != LM_EVAL) break;
        }
        if (lane == 0) {
            const LmShared &S = kForm == 2 ? s_sh : r_sh;
            p.recorded[s] = kForm == 1 ? s_lm.recorded : S.recorded;
            p.evaluations[s] = kForm == 1 ? s_lm.evaluations : S.evaluations;
            p.last_step_norm[s] = kForm == 1 ? s_lm.last_step_norm : S.last_step_norm;
            p.cost[s] = kForm == 1 ? s_lm.cost : S.cost;
        }
        __syncthreads();
    }
}

}  // namespace lom
