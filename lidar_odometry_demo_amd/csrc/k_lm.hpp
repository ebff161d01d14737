// Device-resident solve: the exchange words, the reduce-and-exchange between workgroups and ranks, k_p2p_selftest,
// k_lm and k_sum_records (see match.hip for the overview).  Device code only; match.hip is the one translation unit
// that instantiates and launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "k_eval.hpp"
#include "k_match.hpp"
#include "lm_core.hpp"
#include "lm_wave.hpp"
#include "lom_internal.hpp"
#include "pose_math.hpp"

namespace lom {

// Exchange word of k_lm: a value and a check word = sequence number XOR the value's bits.  A reader
// accepts the pair only when check ^ bits == the sequence number it waits for, so the two 8-byte
// words need no ordering between them and no separate "record complete" flag: publishing is one
// memory round trip and reading is one more.
struct __attribute__((aligned(16))) XWord {
    unsigned long long bits, check;
};

// The pair travels as ONE 16-byte agent-coherent access each way (sc1: past this XCD's L2).  Nothing relies on the
// access being indivisible -- a reader that catches half a pair sees check ^ bits != seq and polls again -- it only
// halves the memory instructions of the exchange (two 8-byte atomics per word each way in round 2).
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void xword_store(XWord *dst, double v, unsigned long long seq)
{
    u64x2 w;
    w.x = (unsigned long long)__double_as_longlong(v);
    w.y = seq ^ w.x;
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst), "v"(w) : "memory");
}
__device__ __forceinline__ void xword_load_issue(const XWord *src, u64x2 &r)  // result valid after xword_load_wait
{
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=&v"(r) : "v"(src) : "memory");
}
template <int kN>
__device__ __forceinline__ void xword_load_wait(u64x2 (&r)[kN])
{
    static_assert(kN == 4 || kN == 8, "loads in flight per lane");
    if constexpr (kN == 4)
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3])::"memory");
    else
        asm volatile("s_waitcnt vmcnt(0)"
                     : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7])::"memory");
}

// a' + b' after v_permlane{32,16}_swap(a, b): lanes of the lower half (of the wave / of each pair of rows) end with
// a[lane] + a[partner], lanes of the upper half with b[partner] + b[lane] -- two values folded by one addition
// (lane mapping verified on the device: tools/microbench/permlane_swap.hip)
template <int kWidth>
__device__ __forceinline__ double swap_add(double a, double b)
{
    unsigned int alo = (unsigned int)__double2loint(a), ahi = (unsigned int)__double2hiint(a);
    unsigned int blo = (unsigned int)__double2loint(b), bhi = (unsigned int)__double2hiint(b);
    if constexpr (kWidth == 32) {
        const auto lo = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
        const auto hi = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
        return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
    } else {
        const auto lo = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
        return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
    }
}

// the kT / 32 partial sums of s_part added in order into s_tot[0..30] by one wave (lane = its thread's index in it)
template <int kT>
__device__ __forceinline__ void lm_final_sum(const double *s_part, double *s_tot, int lane)
{
    if (lane < 31) {
        double v = 0.0;
#pragma unroll
        for (int g = 0; g < kT / 32; g++) v += s_part[g * 32 + lane];
        s_tot[lane] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// k_lm's evaluation epilogue: workgroup reduction of the 28 per-lane sums through LDS in a fixed
// order, every row total published straight from the lane that holds it (plus the workgroup's
// slice of k_match's counters), then all workgroups' words gathered and added in workgroup order
// into s_tot[0..30] -- bitwise the same on every workgroup.  Only the first wave may read s_tot
// afterwards (no workgroup barrier behind the final sum); the caller's next __syncthreads()
// releases s_acc / s_part for the following evaluation.
//   s_acc: 32 doubles per wave;  s_part: kT doubles (kT = threads that hold points).
// kGridArg: the workgroups of the solve are `nb`, not gridDim.x (k_lm's batch form: one launch holds problems of
// different grids, sized for the largest)
// kFinalSum = false (k_lm's 256-thread shapes): the caller's policy wave adds the kT / 32 partial sums in s_part itself
// (lm_final_sum), behind the second __syncthreads() here; the kT threads of the point waves stop at that barrier.
template <int kT, int kBlocks, bool kGridArg = false, bool kFinalSum = true>
__device__ __forceinline__ void reduce_and_exchange(const double acc[28], double *s_acc, double *s_part,
                                                    const uint32_t *__restrict__ block_counters,
                                                    uint32_t n_match_blocks, XWord *set, uint32_t nb,
                                                    unsigned long long seq, unsigned long long timeout_ticks,
                                                    double *s_tot, int *s_failed, const int32_t *chain_error,
                                                    const uint4 pre, unsigned long long *dbg = nullptr)
{
#define RX_STAMP(k)                                                     \
    if (dbg && blockIdx.x == 0 && threadIdx.x == 0) {                   \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");     \
        dbg[k] = __builtin_amdgcn_s_memtime();                          \
    }
    RX_STAMP(0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    XWord *mine = set + (size_t)blockIdx.x * kRecWords;
    // Wave level, all in registers, as a reduce-scatter: v_permlane32_swap exchanges the upper half of one
    // register with the lower half of another, so ONE add folds two values at once -- the lower 32 lanes keep
    // value k, the upper 32 value k + 14 (28 -> 14 values per lane); v_permlane16_swap does the same between
    // the 16-lane rows (14 -> 7: row r now holds values k + 7 r); four DPP butterflies finish the 7 values
    // inside each row.  147 instructions instead of the 168 of a quad pre-sum plus an LDS pass over 28 x 128
    // doubles, and what goes through LDS is 28 doubles per wave.  The order of the additions is fixed.
    double s1[14];
#pragma unroll
    for (int k = 0; k < 14; k++) s1[k] = swap_add<32>(acc[k], acc[k + 14]);
    double s2[7];
#pragma unroll
    for (int k = 0; k < 7; k++) {
        double v = swap_add<16>(s1[k], s1[k + 7]);
        v += dpp_f64<kDppXor1>(v);
        v += dpp_f64<kDppXor2>(v);
        v += dpp_f64<kDppHalfMirror>(v);
        v += dpp_f64<kDppMirror>(v);
        s2[k] = v;
    }
    if ((lane & 15) == 0) {  // the first lane of row r holds the wave's totals of values 7 r .. 7 r + 6
        double *dst = s_acc + wave * 32 + 7 * (lane >> 4);
#pragma unroll
        for (int k = 0; k < 7; k++) dst[k] = s2[k];
    }
    if (wave == kT / 64 - 1) {  // the workgroup's slice of k_match's counters (first evaluation of a launch only)
        // the slice of a workgroup is at most one block per lane when k_lm runs 28 workgroups or more: the caller
        // then loaded this lane's block with the kernel's start-up loads (`pre`); counts are exact in f64, and the
        // wave sum is the permlane-swap / DPP fold of the residual sums (36 LDS-crossbar shuffles in round 2)
        double d0 = 0.0, d1 = 0.0, d2 = 0.0;
        if (n_match_blocks) {
            const uint32_t grid = kGridArg ? nb : gridDim.x;
            const uint32_t chunk = (n_match_blocks + grid - 1) / grid;
            if (chunk <= 64u) {
                uint4 r = pre;
                if constexpr (kT != 256) {  // (the 512-thread shapes have no registers to spare for the early load)
                    const uint32_t b = blockIdx.x * chunk + (uint32_t)lane;
                    r = make_uint4(0u, 0u, 0u, 0u);
                    if ((uint32_t)lane < chunk && b < n_match_blocks) r = *reinterpret_cast<const uint4 *>(block_counters + (size_t)b * 4);
                }
                d0 = (double)r.x;
                d1 = (double)r.y;
                d2 = (double)r.z;
            } else {
                const uint32_t lo = blockIdx.x * chunk;
                const uint32_t hi = min(lo + chunk, n_match_blocks);
                unsigned long long c0 = 0, c1 = 0, c2 = 0;
                for (uint32_t b = lo + lane; b < hi; b += 64) {
                    const uint4 r = *reinterpret_cast<const uint4 *>(block_counters + (size_t)b * 4);
                    c0 += r.x;
                    c1 += r.y;
                    c2 += r.z;
                }
                d0 = (double)c0;
                d1 = (double)c1;
                d2 = (double)c2;
            }
            // rows after the two swaps: 0 = d0, 1 = d2, 2 = d1, 3 = nothing; four butterflies finish each row
            double v = swap_add<16>(swap_add<32>(d0, d1), swap_add<32>(d2, 0.0));
            v += dpp_f64<kDppXor1>(v);
            v += dpp_f64<kDppXor2>(v);
            v += dpp_f64<kDppHalfMirror>(v);
            v += dpp_f64<kDppMirror>(v);
            d0 = v;
        }
        if (lane == 0 || lane == 16 || lane == 32) xword_store(mine + 28 + (lane == 0 ? 0 : (lane == 32 ? 1 : 2)), d0, seq);
    }
    __syncthreads();
    if (tid < 28) {  // the eight waves' totals, in wave order
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < kT / 64; w++) v += s_acc[w * 32 + tid];
        RX_STAMP(1);
        xword_store(mine + tid, v, seq);
    }
    RX_STAMP(2);
    // gather: thread (g = tid / 32, k = tid % 32) takes word k of workgroups kPer g .. kPer g + kPer - 1
    {
        constexpr int kPer = kBlocks / (kT / 32);
        const int k = tid & 31, g = tid >> 5;
        unsigned long long vb[kPer];
        bool ok[kPer];
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            vb[u] = 0;
            ok[u] = (k >= 31) || ((uint32_t)(g * kPer + u) >= nb);
        }
        // Let the words land before the first poll: a poll that comes too early is a wasted memory
        // round trip (and 52 workgroups x 512 lanes of them load the memory side).  Measured on C2:
        // no head start 0.1724 ms per align, s_sleep 8 / 12 / 16 / 20 / 24 -> 0.1668 / 0.1657 / 0.1645 /
        // 0.1650 / 0.1650; again after the round-2 reduction: 4 / 8 / 12 / 16 / 24 -> 0.1580 / 0.1562 / 0.1545 /
        // 0.1539 / 0.1548; round 3 (256-thread workgroups, two points per lane): 4 / 8 / 12 / 16 / 20 / 24 / 32 ->
        // 0.1349 / 0.1333 / 0.1315 / 0.1312 / 0.1325 / 0.1343 / 0.1366; at the end of round 3: 10 / 13 / 16 / 20 ->
        // 0.1355 / 0.1342 / 0.1332 / 0.1328.
        __builtin_amdgcn_s_sleep(16);
        const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
        uint32_t polls = 0;
        // a patience shorter than the head start just slept (16 x 64 cycles, > 0.4 us = 40 ticks of 10 ns) cannot be
        // met whatever the first poll finds: the wait counts as timed out -- which is what makes a 1-tick patience a
        // deterministic way to force the give-up path (tests), not a race against the other workgroups' stores
        if (timeout_ticks < 40ull) {
            *s_failed = 1;
#pragma unroll
            for (int u = 0; u < kPer; u++) ok[u] = true;
        }
        const XWord *mine_src = set + (size_t)(g * kPer) * kRecWords + k;  // (a set holds kMaxLmBlocksBig records: in bounds)
        for (; timeout_ticks >= 40ull;) {
            u64x2 r[kPer];
#pragma unroll
            for (int u = 0; u < kPer; u++) xword_load_issue(mine_src + (size_t)u * kRecWords, r[u]);
            xword_load_wait(r);
            bool all = true;
#pragma unroll
            for (int u = 0; u < kPer; u++) {
                if (!ok[u]) {
                    vb[u] = r[u].x;
                    ok[u] = (r[u].y ^ r[u].x) == seq;
                }
                all = all && ok[u];
            }
            if (all) break;
            if (__builtin_amdgcn_s_memrealtime() - t_start > timeout_ticks) {
                *s_failed = 1;  // some workgroup never published: give up (the grid drains)
                break;
            }
            // a wait that drags on: has a workgroup of this launch given up already?  Then the words this one waits
            // for will never come; it leaves now, not after its own patience.
            if ((++polls & 255u) == 0 && __hip_atomic_load(chain_error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                *s_failed = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        double part = 0.0;
#pragma unroll
        for (int u = 0; u < kPer; u++) part += __longlong_as_double((long long)vb[u]);  // absent workgroups add +0.0
        s_part[tid] = part;
    }
    RX_STAMP(3);
    __syncthreads();
    if constexpr (kFinalSum) {
        if (tid < 64) lm_final_sum<kT>(s_part, s_tot, tid);  // the first wave keeps the totals to itself
        RX_STAMP(4);
    }
#undef RX_STAMP
}

// ---------------------------------------------------------------------------
// k_lm: one whole ceres::Solve (cloud_matcher.cpp:157-158) of the single-GPU align, resident
// on the GPU.  Launched behind k_match once per outer iteration.  Every evaluation the
// Levenberg-Marquardt policy (lm_core.hpp) asks for is done by the whole grid:
//   each workgroup reduces its points to one 256-byte record and publishes it in HBM
//   (agent-coherent stores, sequence word last; two record sets alternate), waits until
//   the records of all workgroups carry the evaluation's sequence number, and adds them
//   in workgroup order -- every workgroup holds the same totals bit for bit and runs the
//   same policy step (one lane), so no decision has to be broadcast and nothing returns to
//   the host between the evaluations of a solve.
// Workgroup 0 then writes the f32 pose back (:161-167), prepares the pose of the next
// k_match in AlignState, decides convergence (:169-172) and copies the state to the report in
// pinned host memory.  Every wait is bounded (s_memrealtime); a workgroup that gives up sets
// the error flags and leaves, the others follow.
// ---------------------------------------------------------------------------
// ---- ranks of one node: the ranks' totals exchanged by the GPUs themselves -------------------
// Every rank owns a small buffer in its HBM: [4 sets][kP2pMaxRanks][32] exchange words.  Inside one
// launch the sets alternate with the sequence number (the dependency chain of a solve keeps a rank at
// most one evaluation ahead of its peers); consecutive launches alternate between the set pairs
// {0,1} and {2,3}, so the first publish of the next k_lm can never overwrite a slot a lagging peer
// still polls for the previous kernel's last evaluation (the kernels of different ranks are not
// ordered against each other).  Rank r's
// workgroup 0 stores its 32 rank totals into slot r of EVERY rank's buffer (its own directly, the
// peers' through their IPC mappings: xGMI), system-coherent stores, same {bits, seq ^ bits} words as
// inside a GPU.  Every workgroup of every rank then reads its own GPU's buffer and adds the ranks'
// words in rank order: identical bits on all workgroups of all ranks, no host in the loop.
// Behind the four sets every buffer holds one ABORT word per rank: a rank whose kernel gives up (its workgroups not
// all resident, a peer that never published) stores the number of the align it abandons -- the same number on every
// rank -- into its word in EVERY rank's buffer.  A kernel waiting for that rank's totals looks at the abort words
// whenever a wait drags on and leaves at once, instead of after its own (ten times longer) patience: without that
// word the ranks reached the host-side agreement up to 100 s apart (round 2's three-rank failure).
constexpr size_t kP2pExchangeWords = (size_t)4 * kP2pMaxRanks * kRecWords;  // XWords before the abort words
constexpr size_t kP2pBufferBytes = kP2pExchangeWords * sizeof(XWord) + kP2pMaxRanks * sizeof(unsigned long long);
struct P2pArgs {
    XWord *peer[kP2pMaxRanks];  // peer[r]: rank r's buffer as seen from this GPU (peer[rank] = local)
    int rank, nranks;
    int set_base;  // 0 or 2: consecutive launches use disjoint pairs of exchange sets (see global_exchange)
    unsigned long long epoch;  // number of this device-to-device align (>= 1; ~0: the attach self-test)
};

__device__ __forceinline__ unsigned long long *p2p_abort_words(XWord *buffer)
{
    return reinterpret_cast<unsigned long long *>(buffer + kP2pExchangeWords);
}

// this rank abandons align `epoch`: tell every rank (own buffer included)
__device__ __forceinline__ void p2p_publish_abort(const P2pArgs &A)
{
    for (int r = 0; r < A.nranks; r++)
        __hip_atomic_store(p2p_abort_words(A.peer[r]) + A.rank, A.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ void global_exchange(const P2pArgs &A, double *s_tot, unsigned long long seq,
                                                unsigned long long timeout_ticks, int *s_failed, bool publisher,
                                                int lane)
{
    const size_t set_off = (size_t)((unsigned)A.set_base + (unsigned)(seq & 1)) * kP2pMaxRanks * kRecWords;
    if (publisher && lane < kRecWords) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(s_tot[lane]);
        for (int r = 0; r < A.nranks; r++) {
            XWord *dst = A.peer[r] + set_off + (size_t)A.rank * kRecWords + lane;
            __hip_atomic_store(&dst->bits, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&dst->check, seq ^ b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    // lane (h = lane / 32, k = lane % 32) reads word k of ranks h, h + 2, h + 4, h + 6
    const XWord *local = A.peer[A.rank] + set_off;
    const int k = lane & 31, h = lane >> 5;
    unsigned long long vb[4] = {0, 0, 0, 0};
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
    const unsigned long long *aborts = p2p_abort_words(A.peer[A.rank]);
    bool failed = false;
    uint32_t polls = 0;
    for (;;) {
        bool all = true;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int r = h + 2 * u;
            if (r < A.nranks) {
                const XWord *w = local + (size_t)r * kRecWords + k;
                const unsigned long long bits = __hip_atomic_load(&w->bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                const unsigned long long chk = __hip_atomic_load(&w->check, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                vb[u] = bits;
                all = all && ((chk ^ bits) == seq);
            }
        }
        if (__ballot(!all) == 0ull) break;
        if (__builtin_amdgcn_s_memrealtime() - t_start > timeout_ticks) {
            failed = true;  // a rank never published: give up (every grid drains)
            break;
        }
        if ((++polls & 63u) == 0) {  // a wait that drags on: has a rank abandoned this align?
            unsigned long long ab = 0;
            if (lane < A.nranks) ab = __hip_atomic_load(aborts + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (__ballot(lane < A.nranks && ab == A.epoch) != 0ull) {
                failed = true;
                break;
            }
        }
        __builtin_amdgcn_s_sleep(1);
    }
    // rank order: lanes < 32 hold the even ranks, their partners (lane + 32) the odd ones
    double total = 0.0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const double mine = __longlong_as_double((long long)vb[u]);
        const double other = __shfl_xor(mine, 32, 64);
        total += (h == 0) ? mine : other;   // rank 2u     (absent ranks add +0.0)
        total += (h == 0) ? other : mine;   // rank 2u + 1
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < kRecWords) s_tot[lane] = total;
    if (failed && lane == 0) *s_failed = 1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lom_comm_attach_p2p's self-test: `rounds` exchanges of known values between all ranks
__global__ __launch_bounds__(64) void k_p2p_selftest(P2pArgs A, unsigned long long seq_base, int rounds,
                                                     unsigned long long timeout_ticks, uint32_t *result)
{
    __shared__ double s_tot[kRecWords];
    __shared__ int s_failed;
    const int lane = threadIdx.x;
    if (lane == 0) s_failed = 0;
    __syncthreads();
    uint32_t bad = 0;
    for (int i = 0; i < rounds && !s_failed; i++) {
        if (lane < kRecWords) s_tot[lane] = (double)(A.rank + 1) * 1000.0 + (double)i + 0.5 * (double)lane;
        __syncthreads();
        // the first round also absorbs the start-up skew between the ranks' processes
        global_exchange(A, s_tot, seq_base + 1 + (unsigned long long)i, i == 0 ? timeout_ticks * 100 : timeout_ticks,
                        &s_failed, true, lane);
        if (lane < kRecWords && !s_failed) {
            double want = 0.0;
            for (int r = 0; r < A.nranks; r++) want += (double)(r + 1) * 1000.0 + (double)i + 0.5 * (double)lane;
            if (s_tot[lane] != want) bad++;
        }
        __syncthreads();
    }
    for (int d = 32; d >= 1; d >>= 1) bad += __shfl_xor(bad, d, 64);
    if (lane == 0) {
        result[0] = bad;
        result[1] = (uint32_t)s_failed;
    }
}

// kRegPts: this lane's first points (first, first + step, ...) stay in registers for every evaluation of the solve
template <int kRegPts>
__device__ __forceinline__ void accumulate_all(const MatchRec *__restrict__ rec, uint32_t n, uint32_t first,
                                               uint32_t step, const float4 (&ra)[kRegPts], const float4 (&rb)[kRegPts],
                                               const float4 (&rc)[kRegPts], const double *x, double acc[28])
{
    const double q0 = x[0], q1 = x[1], q2 = x[2], q3 = x[3], t0 = x[4], t1 = x[5], t2 = x[6];
    const double qe = quat_excess(q0, q1, q2, q3);
#pragma unroll
    for (int k = 0; k < 28; k++) acc[k] = 0.0;
    // The register points go through unconditionally and stage by stage -- residuals and Jacobians of all of them, then
    // their sums -- so that the scheduler interleaves the independent chains (a wave alone on its SIMD issues a dependent
    // instruction every ~9 cycles, independent ones every ~5).  A lane without a match, or beyond the cloud, holds a zero
    // normal: every term it adds is exactly zero.
    PointTerms T[kRegPts];
#pragma unroll
    for (int p = 0; p < kRegPts; p++) point_terms(ra[p], rb[p], rc[p], q0, q1, q2, q3, qe, t0, t1, t2, T[p]);
#pragma unroll
    for (int p = 0; p < kRegPts; p++) point_accumulate(T[p], acc);
    for (uint32_t i = first + (uint32_t)kRegPts * step; i < n; i += step) {
        const float4 *r4 = reinterpret_cast<const float4 *>(rec + i);
        const float4 xa = r4[0], xb = r4[1], xc = r4[2];
        if (xb.w != 0.f) accumulate_point(xa, xb, xc, q0, q1, q2, q3, qe, t0, t1, t2, acc);
    }
}

// kPolicyTwice (LOM_DEBUG_LM_TWICE=1 at create, a measurement aid): the first wave runs every policy step twice -- the
// first time on state that is put back afterwards -- and the phase stamps time the second run: the same instructions
// on the same data, with the step's code already in the instruction cache.
// kBatch: one launch for all problems of a batched align's round (single GPU, no exchange, no debug outputs) --
// blockIdx.y selects the problem (`batch[blockIdx.y]`: records, n, guess, state, k_match's counters, exchange set,
// report, solve grid): the problem's solve runs on the single align's grid for it (`lm_blocks` workgroups; those beyond
// it in a launch sized for the round's largest leave at once); a give-up test applies to problem 0 of the launch.
// kT: the threads that hold points.  The 256-thread shapes run one wave more (lm_threads): the POLICY WAVE, which holds
// the solve's state and no points, while the four point waves hold the points and the accumulators.  Each role runs a
// loop of its own, so the compiler allocates registers for each live set on its own (one loop carried both: 256 VGPRs +
// 34-58 AGPRs and ~200 SGPR spills, one wave per SIMD); the roles meet at the three __syncthreads() of an evaluation.
// fold_report_seq (the single align; the batch form and ranks that exchange sums never fold): 0 = every outer iteration
// runs; else the replay fold is on -- see the end of the kernel -- and this is the report sequence word the host looks
// for first, that of pair kPairsAhead, which a launch that ends the align by folding before that pair writes in place of
// its own.
constexpr int lm_threads(int kT) { return kT == 256 ? kT + 64 : kT; }
template <int kT, int kBlocks = (int)kMaxLmBlocks, int kRegPts = 1, bool kPolicyTwice = false, bool kBatch = false>
__global__ __launch_bounds__(lm_threads(kT)) void k_lm(const MatchRec *__restrict__ rec, uint32_t n, AlignState *state,
                                                     LmInit init, int first_outer,
                                                     const uint32_t *__restrict__ block_counters,
                                                     uint32_t n_match_blocks, XWord *xrec,
                                                     unsigned long long seq_base, AlignReport *report,
                                                     unsigned long long report_seq,
                                                     unsigned long long fold_report_seq,
                                                     unsigned long long timeout_ticks,
                                                     unsigned long long *dbg_stamps, P2pArgs px,
                                                     double *dbg_trace, int test_give_up,
                                                     const BatchProblem *batch = nullptr)
{
    static_assert(!kBatch || !kPolicyTwice, "the batch form is a product kernel");
    if constexpr (kBatch) {
        const ConstBatch d = (ConstBatch)(batch + blockIdx.y);
        rec = d->rec;
        n = d->n;
        state = d->state;
        block_counters = d->block_counters;
        n_match_blocks = d->match_blocks;
        xrec = reinterpret_cast<XWord *>(d->xrec);
        report = d->report;
        if (blockIdx.y != 0) test_give_up = 0;
        if (blockIdx.x >= d->lm_blocks) return;  // (uniform: before any barrier)
    }
    constexpr bool kRoles = lm_threads(kT) != kT;  // a policy wave of its own (wave kT / 64)
    __shared__ double s_acc[(kT / 64) * 32];  // the point waves' totals of one evaluation
    __shared__ double s_tot[kRecWords];
    __shared__ double s_part[kT];
    __shared__ double s_x[7];
    LmWave W;  // the solve's state: per-row part in the registers of the policy wave, the rest in LDS (lm_wave.hpp)
    // the solve's uniform state: in every lane's registers in the 256-thread shapes, one copy in LDS in the 512-thread ones
    constexpr bool kRegState = kT == 256;
    __shared__ LmShared s_lm;
    LmShared r_lm;
    __shared__ int s_action, s_failed;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the wave that runs the policy (kRoles: it holds no points), and its first thread, which writes the state back
    constexpr int kPolicyWave = kRoles ? kT / 64 : 0, kOwnerTid = kPolicyWave * 64;
    const uint32_t nb = kBatch ? ((ConstBatch)(batch + blockIdx.y))->lm_blocks : gridDim.x;
    const uint32_t first = blockIdx.x * (uint32_t)kT + tid, step = nb * (uint32_t)kT;
    // start-up loads issued together (one memory round trip, not three): this lane's first point --
    // it stays in registers for every evaluation of the solve --, the pose, the chain's stop flags
    // (the records' loads are ISSUED here and waited for behind the other start-up loads: left to the compiler, the second
    // register point's loads were scheduled behind the first one's wait -- two round trips where one will do; a lane
    // beyond the cloud reads record 0 and forgets it)
    typedef float RecQuarter __attribute__((ext_vector_type(4)));
    RecQuarter raw_a[kRegPts], raw_b[kRegPts], raw_c[kRegPts];
    float4 ra[kRegPts], rb[kRegPts], rc[kRegPts];
    bool have[kRegPts];
#pragma unroll
    for (int p = 0; p < kRegPts; p++) {
        const uint32_t i = first + (uint32_t)p * step;
        have[p] = tid < kT && i < n;
        const MatchRec *at = rec + (have[p] ? i : 0u);
        asm volatile("global_load_dwordx4 %0, %3, off\n\tglobal_load_dwordx4 %1, %3, off offset:16\n\t"
                     "global_load_dwordx4 %2, %3, off offset:32"
                     : "=&v"(raw_a[p]), "=&v"(raw_b[p]), "=&v"(raw_c[p])
                     : "v"(at)
                     : "memory");
    }
    // ... and, in the last wave, this lane's block of k_match's counters (reduce_and_exchange folds them)
    // (both without a divergent branch around the load -- every lane loads, from a clamped address, and picks afterwards --:
    // the compiler waits for the loads of a divergent region where the region ends, which made these two more round
    // trips in a row behind the records')
    uint4 cnt_pre = make_uint4(0u, 0u, 0u, 0u);
    RecQuarter cnt_raw = {0.f, 0.f, 0.f, 0.f};
    bool cnt_want = false;
    if constexpr (kT == 256) {
        const uint32_t chunk = (n_match_blocks + nb - 1) / nb;
        const uint32_t b = blockIdx.x * chunk + (uint32_t)lane;
        cnt_want = wave == kT / 64 - 1 && n_match_blocks && chunk <= 64u && (uint32_t)lane < chunk && b < n_match_blocks;
        const uint32_t *at = block_counters + (size_t)(cnt_want ? b : 0u) * 4;
        asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(cnt_raw) : "v"(at) : "memory");  // (issued, like the records)
    }
    float x0;
    {
        const int k = tid < 7 ? tid : 0;
        if (first_outer) {  // (uniform)
            if constexpr (kBatch) x0 = k < 4 ? batch[blockIdx.y].guess_q[k] : batch[blockIdx.y].guess_t[k - 4];
            else x0 = k < 4 ? init.q[k] : init.t[k - 4];
        } else {
            const float *from = k < 4 ? &state->pose_q[k] : &state->pose_t[k - 4];
            x0 = *from;
        }
    }
    // the previous outer iteration's tallies, read now (scalar loads, with everything else that starts the kernel) for
    // workgroup 0's write-back at the very end: read there they were one more memory round trip on the critical path
    typedef const __attribute__((address_space(4))) AlignState *ConstState;
    struct {
        int32_t outer_done, lm_iterations, evaluations;
        double valid_total, cand_total, occ_total, queries_total;
    } prev = {0, 0, 0, 0.0, 0.0, 0.0, 0.0};
    if (!first_outer) {
        ConstState cs = (ConstState)state;
        prev.outer_done = cs->outer_done;
        prev.lm_iterations = cs->lm_iterations;
        prev.evaluations = cs->evaluations;
        prev.valid_total = cs->valid_total;
        prev.cand_total = cs->cand_total;
        prev.occ_total = cs->occ_total;
        prev.queries_total = cs->queries_total;
        if (cs->finished | cs->error) return;  // chained launch after the end
    }
    // ... and parked in LDS until then: eleven scalar registers less to carry (or spill) through the solve
    __shared__ double s_prev[4];
    __shared__ int32_t s_prev_i[3];
    if (tid == 0) {
        s_prev[0] = prev.valid_total;
        s_prev[1] = prev.cand_total;
        s_prev[2] = prev.occ_total;
        s_prev[3] = prev.queries_total;
        s_prev_i[0] = prev.outer_done;
        s_prev_i[1] = prev.lm_iterations;
        s_prev_i[2] = prev.evaluations;
    }
    // the records are needed from here on
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(cnt_raw)::"memory");
    if (cnt_want)
        cnt_pre = make_uint4(__float_as_uint(cnt_raw.x), __float_as_uint(cnt_raw.y), __float_as_uint(cnt_raw.z), __float_as_uint(cnt_raw.w));
#pragma unroll
    for (int p = 0; p < kRegPts; p++) {
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(raw_a[p]), "+v"(raw_b[p]), "+v"(raw_c[p])::"memory");
        ra[p] = have[p] ? make_float4(raw_a[p].x, raw_a[p].y, raw_a[p].z, raw_a[p].w) : make_float4(0.f, 0.f, 0.f, 0.f);
        rb[p] = have[p] ? make_float4(raw_b[p].x, raw_b[p].y, raw_b[p].z, raw_b[p].w) : make_float4(0.f, 0.f, 0.f, 0.f);
        rc[p] = have[p] ? make_float4(raw_c[p].x, raw_c[p].y, raw_c[p].z, raw_c[p].w) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // kRoles: the ranks' exchange arguments parked in LDS as well (read by the policy step only when ranks exchange)
    __shared__ P2pArgs s_px;
    if (kRoles && tid == 0) s_px = px;
    auto ranks_args = [&]() -> const P2pArgs & {
        if constexpr (kRoles) return s_px;
        else return px;
    };
    if (tid < 7) s_x[tid] = (double)x0;  // cloud_matcher.cpp:122-131
    __shared__ uint32_t s_pose0[7];  // the bits of the f32 pose this iteration searched at, for the replay fold at the end
    if (!kBatch && tid < 7) s_pose0[tid] = __float_as_uint(x0);
    if (tid == 0) s_failed = test_give_up;  // LOM_OPT_TEST_GIVE_UP_AT_OUTER: this launch behaves as if its waits had timed out
    __syncthreads();
    unsigned long long seq = seq_base;
    uint32_t counters_from = n_match_blocks;  // k_match's counters are folded by the first evaluation only
    double counters[4] = {0.0, 0.0, 0.0, 0.0};  // valid, cand, occ of the last k_match; queries (all ranks)
    int action = LM_EVAL;
    // LOM_DEBUG_LM: shader-clock stamps of workgroup 0 in the first k_lm of the align (0 start, 1 accumulated: the first
    // point lane; 3 totals known, 4 policy done: the policy wave's first lane)
#define LM_STAMP(k)                                                                                          \
    if (dbg_stamps && first_outer && blockIdx.x == 0 && tid == ((k) < 3 ? 0 : kOwnerTid) && ev < 5) {      \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                          \
        dbg_stamps[ev * 5 + (k)] = __builtin_amdgcn_s_memtime();                                             \
    }
    // the wave index as a scalar: the roles' loops are branched around, not masked (a masked branch would keep the
    // points live through the policy loop)
    const bool policy_wave = __builtin_amdgcn_readfirstlane(wave) == kPolicyWave;
    if (kRoles && !policy_wave) {
        // ---- the point waves: accumulate, reduce-scatter, publish and gather; the policy wave does the rest ----
        for (int ev = 0;; ev++) {
            double acc[28];
            LM_STAMP(0);
            accumulate_all<kRegPts>(rec, n, first, step, ra, rb, rc, s_x, acc);
            LM_STAMP(1);
            seq++;
            XWord *set = xrec + (size_t)(seq & 1) * kMaxLmBlocksBig * kRecWords;
            reduce_and_exchange<kT, kBlocks, kBatch, false>(acc, s_acc, s_part, block_counters, counters_from, set, nb, seq,
                                                            timeout_ticks, s_tot, &s_failed, &state->error, cnt_pre,
                                                            (dbg_stamps && first_outer && ev == 1) ? dbg_stamps + 32 : nullptr);
            counters_from = 0;
            __syncthreads();  // the policy step is done: s_x holds the next point, s_action what comes next
            if (s_failed || s_action != LM_EVAL) return;  // (uniform; the policy wave reports)
        }
    }
    // ---- the policy wave (kRoles), or the whole workgroup (512 threads: the first wave runs the policy) ----
    for (int ev = 0; action == LM_EVAL; ev++) {
        seq++;
        if constexpr (kRoles) {
            // the point waves' two barriers of reduce_and_exchange, then their kT / 32 partial sums, added here
            __syncthreads();
            __syncthreads();
            lm_final_sum<kT>(s_part, s_tot, lane);
            if (dbg_stamps && first_outer && ev == 1 && blockIdx.x == 0 && tid == kOwnerTid) {
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                dbg_stamps[32 + 4] = __builtin_amdgcn_s_memtime();
            }
        } else {
            double acc[28];
            LM_STAMP(0);
            accumulate_all<kRegPts>(rec, n, first, step, ra, rb, rc, s_x, acc);
            LM_STAMP(1);
            XWord *set = xrec + (size_t)(seq & 1) * kMaxLmBlocksBig * kRecWords;
            reduce_and_exchange<kT, kBlocks, kBatch>(acc, s_acc, s_part, block_counters, counters_from, set, nb, seq,
                                                     timeout_ticks, s_tot, &s_failed, &state->error, cnt_pre,
                                                     (dbg_stamps && first_outer && ev == 1) ? dbg_stamps + 32 : nullptr);
            counters_from = 0;
        }
        const bool ranks = ranks_args().nranks > 1;
        if (ranks && policy_wave && !s_failed) {
            // ranks of one node: this GPU's totals become the totals over all ranks
            if (lane == 31) s_tot[31] = (double)n;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // ten times the patience of the in-GPU waits: the peers are other processes
            global_exchange(ranks_args(), s_tot, seq, timeout_ticks * 10, &s_failed, blockIdx.x == 0, lane);
        }
        LM_STAMP(3);
        // lom_debug_lm_trace: the point and the totals of every evaluation of this solve, as the
        // policy is about to see them ([ev][40]: x[7], pad, sums[32]; [200] = evaluations recorded)
        if (dbg_trace && blockIdx.x == 0 && policy_wave && !s_failed && ev < 5) {
            if (lane < 7) dbg_trace[ev * 40 + lane] = s_x[lane];
            if (lane < 31) dbg_trace[ev * 40 + 8 + lane] = s_tot[lane];
            if (lane == 31) dbg_trace[ev * 40 + 8 + 31] = ranks ? s_tot[31] : (double)n;
            if (lane == 0) dbg_trace[200] = (double)(ev + 1);
        }
        LmWave W_keep = W;
        LmShared S_keep = r_lm;
        double x_keep = 0.0;
#pragma nounroll
        for (int rep = 0; rep < (kPolicyTwice ? 2 : 1); rep++)
        if (policy_wave && !s_failed) {
            if constexpr (kPolicyTwice) {
                if (rep == 0) {
                    if (lane < 7) x_keep = s_x[lane];
                } else {
                    W = W_keep;
                    r_lm = S_keep;
                    if (lane < 7) s_x[lane] = x_keep;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    LM_STAMP(3);
                }
            }
            // the policy wave holds the totals (s_tot) and runs the policy (lm_core.hpp's, lane-parallel and
            // register-resident: lm_wave.hpp)
            int a;
            if (ev == 0) {
                if (lane == 0) {
                    counters[0] = s_tot[28];
                    counters[1] = s_tot[29];
                    counters[2] = s_tot[30];
                    counters[3] = ranks ? s_tot[31] : (double)n;
                }
                const double *prior_b = kBatch ? batch[blockIdx.y].prior_b : init.prior_b;
                a = kRegState ? lmw2_begin<true>(W, r_lm, s_tot, s_x, prior_b, lane)
                              : lmw2_begin<false>(W, s_lm, s_tot, s_x, prior_b, lane);
            } else {
                const double *prior_b = kBatch ? batch[blockIdx.y].prior_b : init.prior_b;
                a = kRegState ? lmw2_feed<true>(W, r_lm, s_tot, s_x, prior_b, lane)
                              : lmw2_feed<false>(W, s_lm, s_tot, s_x, prior_b, lane);
            }
            // the point of the next evaluation lands in s_x
            if (a == LM_PROPOSE)
                a = kRegState ? lmw2_propose<true>(W, r_lm, s_x, lane) : lmw2_propose<false>(W, s_lm, s_x, lane);
            if (lane == 0) s_action = a;
        }
        LM_STAMP(4);
        __syncthreads();
        if (s_failed) {  // uniform over the workgroup
            if (tid == kOwnerTid) {
                __hip_atomic_store(&state->error, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (ranks_args().nranks > 1) p2p_publish_abort(ranks_args());  // the peers leave their waits for this rank at once
                __hip_atomic_store(&report->error, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            return;
        }
        action = s_action;
    }
#undef LM_STAMP
    if (blockIdx.x != 0 || tid != kOwnerTid) return;
    // ---- end of the outer iteration (workgroup 0, one lane of the policy wave) ----
    const LmShared &S = kRegState ? r_lm : s_lm;
    prev.outer_done = s_prev_i[0];
    prev.lm_iterations = s_prev_i[1];
    prev.evaluations = s_prev_i[2];
    prev.valid_total = s_prev[0];
    prev.cand_total = s_prev[1];
    prev.occ_total = s_prev[2];
    prev.queries_total = s_prev[3];
    const int outer = prev.outer_done;
    float pq[4], pt[3];
    for (int a = 0; a < 4; a++) pq[a] = (float)S.x[a];      // :161-164
    for (int a = 0; a < 3; a++) pt[a] = (float)S.x[4 + a];  // :165-167
    int finished = ((S.last_step_norm < 1e-4 && outer > 3) || outer + 1 >= 35) ? 1 : 0;  // :117, :169-172
    // Replay fold (lm_core.hpp, replay_fold_count).  The pose written back equals, bit for bit, the pose this iteration
    // searched at -- read from AlignState, where a previous k_lm derived P for k_match from exactly these seven words
    // (not so in iteration 0, whose search took a PoseArgs built on the host) --: the next iteration would write the same
    // records, add the same sums in the same order, take the same policy branches and end here again, and so on until
    // the stop rule.  Those iterations are accounted for below instead of run; the kernels already enqueued for them
    // find `finished` and return.  -0.0 against +0.0 is no equality.
    int folded = 0;
    if constexpr (!kBatch) {
        if (fold_report_seq && !first_outer && !finished && ranks_args().nranks <= 1) {
            bool same = true;
            for (int a = 0; a < 4; a++) same = same && __float_as_uint(pq[a]) == s_pose0[a];
            for (int a = 0; a < 3; a++) same = same && __float_as_uint(pt[a]) == s_pose0[4 + a];
            if (same) folded = replay_fold_count(outer + 1, S.last_step_norm);
            if (folded) finished = 1;
        }
    }
    AlignState st;
    float R[9];
    rotation_matrix(pq, R);  // voxel_grid.h:212
    for (int i = 0; i < 9; i++) st.P.R[i] = (double)R[i];
    for (int i = 0; i < 3; i++) st.P.t[i] = (double)pt[i];
    st.P.max_sq = kBatch ? batch[blockIdx.y].max_sq : init.max_sq;
    for (int a = 0; a < 3; a++) st.pose_t[a] = pt[a];
    for (int a = 0; a < 4; a++) st.pose_q[a] = pq[a];
    st.finished = finished;
    st.error = 0;
    st.outer_done = outer + 1 + folded;
    st.lm_iterations = prev.lm_iterations + S.recorded;
    st.evaluations = prev.evaluations + S.evaluations;
    st.replayed = folded;
    st.valid_last = counters[0];
    st.valid_total = prev.valid_total + counters[0];
    st.cand_total = prev.cand_total + counters[1];
    st.occ_total = prev.occ_total + counters[2];
    st.queries_total = prev.queries_total + counters[3];
    for (int r = 0; r < folded; r++) {  // each folded iteration adds what this one added, as the executed loop would have
        st.lm_iterations += S.recorded;
        st.evaluations += S.evaluations;
        st.valid_total += counters[0];
        st.cand_total += counters[1];
        st.occ_total += counters[2];
        st.queries_total += counters[3];
    }
    st.final_cost = S.cost;
    st.last_step_norm = S.last_step_norm;
    *state = st;
    // The host reads its first report after the fifth outer iteration (the stop rule cannot fire
    // earlier, and it enqueued five pairs at once): the reports of iterations 1-4 would only cost
    // this kernel a PCIe round trip each.
    // (a fold ends the align at iteration 5 or 35 of the reference's count, wherever it happens: it always reports)
    if (st.outer_done < kPairsAhead) return;
    if (folded && report_seq < fold_report_seq) report_seq = fold_report_seq;  // the word the host is waiting for
    // report: payload as system-scope stores, drained, then the sequence word
    unsigned long long *dst_w = reinterpret_cast<unsigned long long *>(report);
    auto put = [&](size_t byte_off, unsigned long long v) {
        __hip_atomic_store(dst_w + byte_off / 8, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    auto two_i = [](int lo, int hi) { return (unsigned long long)(uint32_t)lo | ((unsigned long long)(uint32_t)hi << 32); };
    auto two_f = [](float lo, float hi) {
        return (unsigned long long)__float_as_uint(lo) | ((unsigned long long)__float_as_uint(hi) << 32);
    };
    put(offsetof(AlignReport, finished), two_i(st.finished, 0));
    put(offsetof(AlignReport, outer_done), two_i(st.outer_done, st.lm_iterations));
    put(offsetof(AlignReport, evaluations), two_i(st.evaluations, st.replayed));
    put(offsetof(AlignReport, pose_t), two_f(pt[0], pt[1]));
    put(offsetof(AlignReport, pose_t) + 8, two_f(pt[2], pq[0]));
    put(offsetof(AlignReport, pose_t) + 16, two_f(pq[1], pq[2]));
    put(offsetof(AlignReport, pose_t) + 24, two_f(pq[3], 0.f));
    put(offsetof(AlignReport, valid_last), (unsigned long long)__double_as_longlong(st.valid_last));
    put(offsetof(AlignReport, valid_total), (unsigned long long)__double_as_longlong(st.valid_total));
    put(offsetof(AlignReport, cand_total), (unsigned long long)__double_as_longlong(st.cand_total));
    put(offsetof(AlignReport, occ_total), (unsigned long long)__double_as_longlong(st.occ_total));
    put(offsetof(AlignReport, queries_total), (unsigned long long)__double_as_longlong(st.queries_total));
    put(offsetof(AlignReport, final_cost), (unsigned long long)__double_as_longlong(st.final_cost));
    put(offsetof(AlignReport, last_step_norm), (unsigned long long)__double_as_longlong(st.last_step_norm));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(dst_w, report_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// multi-GPU path: fold the records of one launch in workgroup order -> LOM_NSUMS doubles in HBM
__global__ __launch_bounds__(64) void k_sum_records(const double *__restrict__ rec, uint32_t n_rec,
                                                    uint32_t n_queries, double *__restrict__ out)
{
    const int k = threadIdx.x;
    if (k >= LOM_NSUMS) return;
    double v = 0.0;
    if (k < 31) {
        uint32_t b = 0;
        for (; b + 4 <= n_rec; b += 4) {  // independent loads in flight, fixed summation order
            const double a0 = rec[(size_t)b * kRecWords + k], a1 = rec[(size_t)(b + 1) * kRecWords + k];
            const double a2 = rec[(size_t)(b + 2) * kRecWords + k], a3 = rec[(size_t)(b + 3) * kRecWords + k];
            v += a0;
            v += a1;
            v += a2;
            v += a3;
        }
        for (; b < n_rec; b++) v += rec[(size_t)b * kRecWords + k];
    } else {
        v = (double)n_queries;
    }
    out[k] = v;
}

}  // namespace lom
