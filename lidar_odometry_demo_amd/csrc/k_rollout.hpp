// Trajectory rollouts (include/lidar_odometry_amd.h, "trajectory rollouts"): k_rollout_fill, k_rollout_eval,
// k_rollout_eval_serial and k_rollout_summary.  Device code only; rollout.hip is the one translation unit that
// instantiates and launches it.  The rule of a step and of a pose test is rollout_rule.hpp's, shared with the host.
// Integers throughout; plain vector stores and vector atomics only; no workgroup ever waits for another: what one launch
// needs from all workgroups of another is a launch of its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rollout_rule.hpp"

namespace lom {

constexpr uint32_t kRolloutThreads = 256;      // four waves: every kernel but k_rollout_eval, which runs one or four
constexpr uint32_t kRolloutRedWords = 32;      // the head of the evaluation's dynamic LDS: the workgroup's partial results
constexpr uint32_t kRolloutUnreached = 0xFFFFFFFFu;
constexpr uint32_t kRolloutIndexBits = 20;     // a candidate's index in the key
constexpr unsigned long long kRolloutIndexMask = (1ull << kRolloutIndexBits) - 1ull;
constexpr long long kRolloutKeyBias = 1ll << 41;
// the summary words of an evaluation (zeroed by k_rollout_fill), u64 each
enum { RW_VALID = 0, RW_ADMISSIBLE = 1, RW_NO_PICK = 2, RW_COUNT = 4 };

struct RolloutArgs {
    uint32_t width, height;
    uint32_t segments, steps_per_segment, steps;  // L, Tn, S
    int32_t lethal_min, unknown_cost;
    uint32_t min_steps, progress_weight, cost_weight, truncation_weight;
    uint32_t n_candidates, n_samples;             // K, F
    uint32_t window_side, window_half;            // the staged window: side cells around the state's cell, half = S + reach
    uint32_t block_candidates;                    // candidates of a workgroup
    uint32_t keep_records;
};

// the record and the pick as the header lays them out (lom_rollout_record, lom_rollout_pick)
struct RolloutRecord {
    uint32_t free_poses, reason, cost_sum, cost_max;
    int32_t end_x, end_y;
    uint32_t end_angle, end_potential;
};
static_assert(sizeof(RolloutRecord) == 32, "RolloutRecord is 32 bytes");
struct RolloutPick {
    uint32_t k, admissible;
    long long score;
};
static_assert(sizeof(RolloutPick) == 16, "RolloutPick is 16 bytes");

__device__ __forceinline__ uint32_t rollout_wave_sum(uint32_t v)
{
    for (uint32_t o = 32u; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, (int)o);
    return v;
}

__device__ __forceinline__ uint32_t rollout_wave_max(uint32_t v)
{
    for (uint32_t o = 32u; o; o >>= 1) {
        const uint32_t u = (uint32_t)__shfl_xor((int)v, (int)o);
        v = u > v ? u : v;
    }
    return v;
}

__device__ __forceinline__ unsigned long long rollout_wave_max64(unsigned long long v)
{
    for (uint32_t o = 32u; o; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, (int)o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)o);
        const unsigned long long u = ((unsigned long long)hi << 32) | lo;
        v = u > v ? u : v;
    }
    return v;
}

// A cell through the staged window: what lies in the window is read in LDS, anything else (the host's proof says: nothing)
// in HBM, so a wrong window could cost time, never a wrong byte or a read out of bounds.
struct RolloutWindowCell {
    const int8_t *plane;
    uint32_t width;
    const int8_t *window;
    int32_t wx0, wy0;
    uint32_t side;
    __device__ __forceinline__ int8_t operator()(int32_t cx, int32_t cy) const
    {
        const uint32_t ux = (uint32_t)(cx - wx0), uy = (uint32_t)(cy - wy0);
        if (ux < side && uy < side) return window[uy * side + ux];
        return plane[(size_t)cy * width + (uint32_t)cx];
    }
};

// the window of the workgroup's state, by all of its lanes: cells outside the grid read 0 and are never asked for
__device__ __forceinline__ void rollout_stage_window(const int8_t *plane, const RolloutArgs &a, int32_t wx0, int32_t wy0, int8_t *window)
{
    const uint32_t n = a.window_side * a.window_side;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t row = i / a.window_side, col = i - row * a.window_side;
        const int32_t gx = wx0 + (int32_t)col, gy = wy0 + (int32_t)row;
        window[i] = (uint32_t)gx < a.width && (uint32_t)gy < a.height ? plane[(size_t)gy * a.width + (uint32_t)gx] : (int8_t)0;
    }
}

// Steps 3 and 4 for one candidate, by one lane: the record, and the key of its score -- 0 when it is not admissible.
__device__ __forceinline__ unsigned long long rollout_finish(const RolloutArgs &a, const uint32_t *potential, uint32_t p0, uint32_t m, uint32_t k,
                                                             uint32_t free_poses, uint32_t reason, uint32_t cost_sum, uint32_t cost_max,
                                                             int32_t end_x, int32_t end_y, uint32_t end_angle, RolloutRecord *records)
{
    const int32_t ex = end_x >> kRolloutCellShift, ey = end_y >> kRolloutCellShift;
    const uint32_t end_potential =
        potential && (uint32_t)ex < a.width && (uint32_t)ey < a.height ? potential[(size_t)ey * a.width + (uint32_t)ex] : kRolloutUnreached;
    if (a.keep_records)
        records[(size_t)m * a.n_candidates + k] = RolloutRecord{free_poses, reason, cost_sum, cost_max, end_x, end_y, end_angle, end_potential};
    if (free_poses <= a.min_steps) return 0ull;
    if (potential && (p0 == kRolloutUnreached || end_potential == kRolloutUnreached)) return 0ull;
    long long s = -(long long)a.cost_weight * (long long)cost_sum -
                  (long long)a.truncation_weight * ((long long)a.steps + 1ll - (long long)free_poses);
    if (potential) s += (long long)a.progress_weight * ((long long)p0 - (long long)end_potential);
    return ((unsigned long long)(s + kRolloutKeyBias) << kRolloutIndexBits) | (kRolloutIndexMask - k);
}

// the workgroup's best key and admissible count to the state's words: one atomic each per workgroup
__device__ __forceinline__ void rollout_reduce(uint32_t *red, unsigned long long best, uint32_t admissible, uint32_t m, unsigned long long *keys,
                                               uint32_t *counts)
{
    const uint32_t t = threadIdx.x, nw = blockDim.x >> 6;
    best = rollout_wave_max64(best), admissible = rollout_wave_sum(admissible);
    if ((t & 63u) == 0u) {
        uint32_t *const r = red + 4u * (t >> 6);
        r[0] = (uint32_t)best, r[1] = (uint32_t)(best >> 32), r[2] = admissible;
    }
    __syncthreads();
    if (t == 0u) {
        for (uint32_t w = 1u; w < nw; w++) {
            const unsigned long long u = ((unsigned long long)red[4u * w + 1u] << 32) | red[4u * w];
            best = u > best ? u : best, admissible += red[4u * w + 2u];
        }
        if (admissible) {
            atomicMax(keys + m, best);
            atomicAdd(counts + m, admissible);
        }
    }
}

// the keys and counts of the states and the summary words of a new evaluation
__global__ __launch_bounds__(kRolloutThreads) void k_rollout_fill(unsigned long long *keys, uint32_t *counts, uint32_t n, unsigned long long *words)
{
    const uint32_t i = blockIdx.x * kRolloutThreads + threadIdx.x;
    if (i < n) keys[i] = 0ull, counts[i] = 0u;
    if (i < (uint32_t)RW_COUNT) words[i] = 0ull;
}

// Steps 1 to 4, a workgroup per state (blockIdx.y) and block of candidates (blockIdx.x).  A wave takes one candidate at a
// time with a lane per pose, in chunks of 64 poses.  The pose sequence depends on no load: a pose's angle is the closed
// form of rollout_angle_sum, its position the state plus the prefix sum of the steps before it -- each lane computes the
// step that leads to its pose, a wave inclusive scan adds them, and the last lane's position carries to the next chunk.
// Every lane then tests the footprint at its pose, with the table and the footprint in LDS and the plane in HBM or, where
// the host found that the window fits (kWindow), staged in LDS; neighbouring lanes are neighbouring poses and touch
// neighbouring cells.  A 64-bit ballot of the blocked poses and its trailing zeros give t*; the costs are wave sums and
// maxima over the lanes below it; the chunks behind a blocked one are skipped.  Lane values below t* are what a serial
// walk computes, pose by pose, and nothing above t* is read, so the early exit cannot change a byte; sums, maxima and the
// key's maximum do not depend on order; every record is written by exactly one lane.
template <bool kWindow>
__global__ __launch_bounds__(kRolloutThreads) void k_rollout_eval(const int8_t *__restrict__ plane, const uint32_t *__restrict__ potential,
                                                                  const int32_t *__restrict__ table, const int32_t *__restrict__ states,
                                                                  const int16_t *__restrict__ commands, const int32_t *__restrict__ footprint,
                                                                  RolloutArgs a, RolloutRecord *records, unsigned long long *keys, uint32_t *counts)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t rollout_lds[];
    uint32_t *const red = rollout_lds;
    int32_t *const ltab = reinterpret_cast<int32_t *>(rollout_lds + kRolloutRedWords);
    int32_t *const lfoot = ltab + 2u * kRolloutTable;
    int8_t *const lwin = reinterpret_cast<int8_t *>(lfoot + 2u * a.n_samples);
    const uint32_t m = blockIdx.y, t = threadIdx.x, nt = blockDim.x, lane = t & 63u, wave = t >> 6, nw = nt >> 6;
    const int32_t x0 = states[3u * m], y0 = states[3u * m + 1u];
    const uint32_t a0 = (uint32_t)states[3u * m + 2u];
    const int32_t cx0 = x0 >> kRolloutCellShift, cy0 = y0 >> kRolloutCellShift;
    const uint32_t k_begin = blockIdx.x * a.block_candidates;
    unsigned long long best = 0ull;
    uint32_t admissible = 0u;
    if ((uint32_t)cx0 < a.width && (uint32_t)cy0 < a.height) {  // uniform over the workgroup
        for (uint32_t i = t; i < 2u * kRolloutTable; i += nt) ltab[i] = table[i];
        for (uint32_t i = t; i < 2u * a.n_samples; i += nt) lfoot[i] = footprint[i];
        if (kWindow) rollout_stage_window(plane, a, cx0 - (int32_t)a.window_half, cy0 - (int32_t)a.window_half, lwin);
        __syncthreads();
        const uint32_t p0 = potential ? potential[(size_t)cy0 * a.width + (uint32_t)cx0] : kRolloutUnreached;
        const RolloutWindowCell wcell{plane, a.width, lwin, cx0 - (int32_t)a.window_half, cy0 - (int32_t)a.window_half, a.window_side};
        const RolloutPlaneCell pcell{plane, a.width};
        for (uint32_t c = wave; c < a.block_candidates; c += nw) {
            const uint32_t k = k_begin + c;
            if (k >= a.n_candidates) break;  // uniform over the wave
            const int16_t *const cmd = commands + (size_t)k * 2u * a.segments;
            int32_t carry_x = x0, carry_y = y0;  // the last pose of the chunk before
            int32_t end_x = x0, end_y = y0;
            uint32_t end_a = a0, free_poses = a.steps + 1u, reason = ROLLOUT_OK, cost_sum = 0u, cost_max = 0u;
            for (uint32_t base = 0u; base <= a.steps; base += 64u) {
                const uint32_t tp = base + lane;
                const bool active = tp <= a.steps;
                int32_t v_in = 0, w_in = 0;
                const int32_t angle_sum = rollout_angle_sum(a0, cmd, a.segments, a.steps_per_segment, active ? tp : a.steps, &v_in, &w_in);
                const uint32_t at = (uint32_t)angle_sum & kRolloutAngleMask;
                int32_t dx = 0, dy = 0;
                if (active && tp) {  // the step that leads here starts at the angle one w back
                    const uint32_t bu = ((uint32_t)(angle_sum - w_in) & kRolloutAngleMask) >> kRolloutAngleShift;
                    dx = rollout_increment(v_in, ltab[2u * bu]), dy = rollout_increment(v_in, ltab[2u * bu + 1u]);
                }
                for (uint32_t o = 1u; o < 64u; o <<= 1) {
                    const int32_t ux = __shfl_up(dx, o), uy = __shfl_up(dy, o);
                    if (lane >= o) dx += ux, dy += uy;
                }
                const int32_t x = carry_x + dx, y = carry_y + dy;
                carry_x = __shfl(x, 63), carry_y = __shfl(y, 63);  // (lanes past S add nothing)
                const uint32_t bt = at >> kRolloutAngleShift;
                uint32_t cost = 0u;
                const uint32_t code = kWindow ? rollout_pose_test(x, y, ltab[2u * bt], ltab[2u * bt + 1u], lfoot, a.n_samples, a.width, a.height,
                                                                  a.lethal_min, a.unknown_cost, wcell, &cost)
                                              : rollout_pose_test(x, y, ltab[2u * bt], ltab[2u * bt + 1u], lfoot, a.n_samples, a.width, a.height,
                                                                  a.lethal_min, a.unknown_cost, pcell, &cost);
                const unsigned long long blocked = __ballot(active && code != ROLLOUT_OK);
                const uint32_t in_chunk = a.steps + 1u - base < 64u ? a.steps + 1u - base : 64u;
                const uint32_t n_free = blocked ? (uint32_t)__builtin_ctzll(blocked) : in_chunk;
                const uint32_t mine = lane < n_free ? cost : 0u;
                cost_sum += rollout_wave_sum(mine);
                const uint32_t chunk_max = rollout_wave_max(mine);
                cost_max = chunk_max > cost_max ? chunk_max : cost_max;
                if (n_free) end_x = __shfl(x, (int)n_free - 1), end_y = __shfl(y, (int)n_free - 1), end_a = (uint32_t)__shfl((int)at, (int)n_free - 1);
                if (blocked) {
                    free_poses = base + n_free, reason = (uint32_t)__shfl((int)code, (int)n_free);
                    break;
                }
            }
            if (lane == 0u) {
                const unsigned long long key =
                    rollout_finish(a, potential, p0, m, k, free_poses, reason, cost_sum, cost_max, end_x, end_y, end_a, records);
                if (key) best = key > best ? key : best, admissible++;
            }
        }
    } else if (a.keep_records) {
        for (uint32_t c = t; c < a.block_candidates; c += nt)
            if (k_begin + c < a.n_candidates)
                records[(size_t)m * a.n_candidates + k_begin + c] = RolloutRecord{0u, ROLLOUT_INVALID, 0u, 0u, x0, y0, a0, kRolloutUnreached};
    }
    rollout_reduce(red, best, admissible, m, keys, counts);
}

// The plain form (LOM_ROLLOUT_OPT_TEST_SERIAL): a lane per candidate steps pose by pose, with the table and the footprint
// in HBM, and stops at the first blocked pose.  It shares rollout_rule.hpp's step and pose test, and nothing of the closed
// form, the scan or the ballot above: the baseline, and an independent second implementation.
template <bool kWindow>
__global__ __launch_bounds__(kRolloutThreads) void k_rollout_eval_serial(const int8_t *__restrict__ plane, const uint32_t *__restrict__ potential,
                                                                         const int32_t *__restrict__ table, const int32_t *__restrict__ states,
                                                                         const int16_t *__restrict__ commands,
                                                                         const int32_t *__restrict__ footprint, RolloutArgs a,
                                                                         RolloutRecord *records, unsigned long long *keys, uint32_t *counts)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t rollout_lds[];
    uint32_t *const red = rollout_lds;
    int8_t *const lwin = reinterpret_cast<int8_t *>(rollout_lds + kRolloutRedWords);
    const uint32_t m = blockIdx.y, k = blockIdx.x * a.block_candidates + threadIdx.x;
    const int32_t x0 = states[3u * m], y0 = states[3u * m + 1u];
    const uint32_t a0 = (uint32_t)states[3u * m + 2u];
    const int32_t cx0 = x0 >> kRolloutCellShift, cy0 = y0 >> kRolloutCellShift;
    const bool valid = (uint32_t)cx0 < a.width && (uint32_t)cy0 < a.height;
    unsigned long long best = 0ull;
    uint32_t admissible = 0u;
    if (kWindow && valid) {  // uniform over the workgroup
        rollout_stage_window(plane, a, cx0 - (int32_t)a.window_half, cy0 - (int32_t)a.window_half, lwin);
        __syncthreads();
    }
    if (k < a.n_candidates) {
        if (valid) {
            const uint32_t p0 = potential ? potential[(size_t)cy0 * a.width + (uint32_t)cx0] : kRolloutUnreached;
            const RolloutWindowCell wcell{plane, a.width, lwin, cx0 - (int32_t)a.window_half, cy0 - (int32_t)a.window_half, a.window_side};
            const RolloutPlaneCell pcell{plane, a.width};
            const int16_t *const cmd = commands + (size_t)k * 2u * a.segments;
            int32_t x = x0, y = y0, end_x = x0, end_y = y0;
            uint32_t ang = a0, end_a = a0, free_poses = a.steps + 1u, reason = ROLLOUT_OK, cost_sum = 0u, cost_max = 0u;
            for (uint32_t tp = 0u, l = 0u, in_segment = 0u; tp <= a.steps; tp++) {
                const uint32_t b = ang >> kRolloutAngleShift;
                const int32_t tc = table[2u * b], ts = table[2u * b + 1u];
                uint32_t cost = 0u;
                const uint32_t code = kWindow ? rollout_pose_test(x, y, tc, ts, footprint, a.n_samples, a.width, a.height, a.lethal_min,
                                                                  a.unknown_cost, wcell, &cost)
                                              : rollout_pose_test(x, y, tc, ts, footprint, a.n_samples, a.width, a.height, a.lethal_min,
                                                                  a.unknown_cost, pcell, &cost);
                if (code != ROLLOUT_OK) {
                    free_poses = tp, reason = code;
                    break;
                }
                cost_sum += cost, cost_max = cost > cost_max ? cost : cost_max;
                end_x = x, end_y = y, end_a = ang;
                if (tp == a.steps) break;
                const int32_t v = cmd[2u * l], w = cmd[2u * l + 1u];
                x += rollout_increment(v, tc), y += rollout_increment(v, ts);
                ang = (uint32_t)((int32_t)ang + w) & kRolloutAngleMask;
                if (++in_segment == a.steps_per_segment) in_segment = 0u, l++;
            }
            const unsigned long long key = rollout_finish(a, potential, p0, m, k, free_poses, reason, cost_sum, cost_max, end_x, end_y, end_a, records);
            if (key) best = key, admissible = 1u;
        } else if (a.keep_records) {
            records[(size_t)m * a.n_candidates + k] = RolloutRecord{0u, ROLLOUT_INVALID, 0u, 0u, x0, y0, a0, kRolloutUnreached};
        }
    }
    rollout_reduce(red, best, admissible, m, keys, counts);
}

// Steps 4 and 5 over the states: the pick from the state's key and count, and the summary's sums.
__global__ __launch_bounds__(kRolloutThreads) void k_rollout_summary(const int32_t *states, uint32_t n, uint32_t width, uint32_t height,
                                                                     const unsigned long long *keys, const uint32_t *counts, RolloutPick *picks,
                                                                     unsigned long long *words)
{
    const uint32_t i = blockIdx.x * kRolloutThreads + threadIdx.x;
    uint32_t valid = 0u, admissible = 0u, none = 0u;
    if (i < n) {
        const int32_t cx = states[3u * i] >> kRolloutCellShift, cy = states[3u * i + 1u] >> kRolloutCellShift;
        valid = (uint32_t)cx < width && (uint32_t)cy < height ? 1u : 0u;
        const unsigned long long key = keys[i];
        admissible = counts[i], none = key ? 0u : 1u;
        picks[i] = key ? RolloutPick{(uint32_t)(kRolloutIndexMask - (key & kRolloutIndexMask)), admissible,
                                     (long long)(key >> kRolloutIndexBits) - kRolloutKeyBias}
                       : RolloutPick{0xFFFFFFFFu, 0u, 0ll};
    }
    valid = rollout_wave_sum(valid), admissible = rollout_wave_sum(admissible), none = rollout_wave_sum(none);
    if ((threadIdx.x & 63u) == 0u) {
        if (valid) atomicAdd(words + RW_VALID, (unsigned long long)valid);
        if (admissible) atomicAdd(words + RW_ADMISSIBLE, (unsigned long long)admissible);
        if (none) atomicAdd(words + RW_NO_PICK, (unsigned long long)none);
    }
}

}  // namespace lom
