// Evaluation of the robustified normal equations: point_terms / accumulate_point, k_eval and k_eval_server (see
// match.hip for the overview).  Device code only; match.hip is the one translation unit that instantiates and launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "k_match.hpp"
#include "lom_internal.hpp"

namespace lom {

// ---------------------------------------------------------------------------
// Evaluation: residual + Jacobian + robust weight + reduction.  One lane per
// source point, grid-stride; 28 f64 accumulators per lane; each workgroup
// publishes ONE 256-byte record: [0..27] its sums, [28..30] its slice of the
// counters k_match left per workgroup, [31] the evaluation's sequence number.
//
//   k_eval         one evaluation per launch; records stay in HBM (multi-GPU path:
//                  k_sum_records folds them for the RCCL all-gather).
//   k_eval_server  host-driven path, one GPU per rank.  Launched once per outer iteration behind
//                  k_match, it evaluates at the launch pose, then stays resident and
//                  serves the LM iterations: the host writes {seq, op, pose} into
//                  pinned host memory, every workgroup polls that word, evaluates,
//                  and stores its record straight into coherent pinned host memory
//                  (payload, system-scope release, sequence word).  The host polls the
//                  <= 64 sequence words and adds the records in workgroup order --
//                  bitwise reproducible; per LM iteration there is no kernel launch,
//                  no inter-workgroup hand-off, no copy and no stream synchronisation.
//                  The first point of every lane stays in registers across
//                  evaluations.  Workgroups never wait on each other, and every spin
//                  is bounded by a wall-clock timeout (s_memrealtime), so the grid
//                  always drains; the host relaunches if a server timed out.
// ---------------------------------------------------------------------------
constexpr int kAccStride = kEvalThreads + 16;  // LDS row stride (doubles): rows k, k+1 land on disjoint banks

struct EvalCmd {  // pinned host memory, written by the host only
    unsigned long long seq;  // increases with every command
    unsigned int op;         // kCmdEval / kCmdStop
    unsigned int pad;
    double q[4];
    double t[3];
};
constexpr unsigned int kCmdEval = 1, kCmdStop = 2;
constexpr int kPublishPlain = 0, kPublishHost = 1, kPublishDevice = 2;

// The f64 residual / Jacobian arithmetic below contracts a * b + c to one FMA (the library is built with
// -ffp-contract=off for the f32 index and distance expressions of the search, which must round like the reference's
// x86 build; these f64 sums are compared with the oracle's to 1e-12 of their scale, not bit for bit, and the order of
// the additions across points differs from any CPU's anyway): a third fewer instructions per point.
#pragma clang fp contract(fast)
struct PointTerms {
    double J[6], r;
};
// |q|^2 - 1 of an evaluation's quaternion (uniform: once per evaluation, every lane may compute it).  About 1e-7 at the
// start of every solve, whose quaternion is an f32 pose widened, and whatever the LM candidates drift to afterwards.
__host__ __device__ __forceinline__ double quat_excess(const double q0, const double q1, const double q2,
                                                       const double q3)
{
    return (((q0 * q0 - 1.0) + q1 * q1) + q2 * q2) + q3 * q3;
}
// cloud_matcher.cpp:54  (rot*local_point + t - plane_origin).dot(plane_normal); p, n and rp = rot*local_point (by the
// unit-quaternion formula) are kept for the Jacobian
struct PointGeom {
    double p[3], nn[3], rp[3];
};
__host__ __device__ __forceinline__ double point_residual(const float4 ra, const float4 rb, const float4 rc,
                                                          const double q0, const double q1, const double q2,
                                                          const double q3, const double t0, const double t1,
                                                          const double t2, PointGeom &G)
{
    const double p[3] = {(double)ra.x, (double)ra.y, (double)ra.z};
    const double o[3] = {(double)rb.x, (double)rb.y, (double)rb.z};
    const double nn[3] = {(double)ra.w, (double)rc.x, (double)rc.y};
    // rp = p + 2 (q0 c + u x c), c = u x p: the factor 2 rides on the last multiply-add
    const double c0 = q2 * p[2] - q3 * p[1];
    const double c1 = q3 * p[0] - q1 * p[2];
    const double c2 = q1 * p[1] - q2 * p[0];
    const double rp0 = p[0] + 2.0 * (q0 * c0 + (q2 * c2 - q3 * c1));
    const double rp1 = p[1] + 2.0 * (q0 * c1 + (q3 * c0 - q1 * c2));
    const double rp2 = p[2] + 2.0 * (q0 * c2 + (q1 * c1 - q2 * c0));
    const double e0 = rp0 + t0 - o[0], e1 = rp1 + t1 - o[1], e2 = rp2 + t2 - o[2];
    for (int a = 0; a < 3; a++) {
        G.p[a] = p[a];
        G.nn[a] = nn[a];
    }
    G.rp[0] = rp0;
    G.rp[1] = rp1;
    G.rp[2] = rp2;
    return e0 * nn[0] + (e1 * nn[1] + e2 * nn[2]);
}
// cloud_matcher.cpp:48-98 for one correspondence: residual and 1x6 tangent Jacobian.  qe = quat_excess(q).
// The rotation columns in closed form, J[0..2] = 2 (h x n) with h = rp + qe p:
//   the reference differentiates the homogeneous rotation H(q) p = |q|^2 R(q/|q|) p, which is multiplicative,
//   H(a (x) q) = H(a) H(q), and its manifold steps on the left, q <- z (x) q, with H(1 + eps e_j) = I + 2 eps [e_j]x +
//   O(eps^2): d r / d delta_j = 2 n . (e_j x H(q) p) = 2 (H(q) p x n)_j;
//   and H(q) p = rp + (|q|^2 - 1) p, because 2 u (u.p) = 2 u x (u x p) + 2 |u|^2 p.
__host__ __device__ __forceinline__ void point_terms(const float4 ra, const float4 rb, const float4 rc, const double q0,
                                                     const double q1, const double q2, const double q3, const double qe,
                                                     const double t0, const double t1, const double t2, PointTerms &T)
{
    PointGeom G;
    T.r = point_residual(ra, rb, rc, q0, q1, q2, q3, t0, t1, t2, G);
    const double *nn = G.nn;
    const double h0 = G.rp[0] + qe * G.p[0], h1 = G.rp[1] + qe * G.p[1], h2 = G.rp[2] + qe * G.p[2];
    const double c0 = h1 * nn[2] - h2 * nn[1];
    const double c1 = h2 * nn[0] - h0 * nn[2];
    const double c2 = h0 * nn[1] - h1 * nn[0];
    T.J[0] = c0 + c0;
    T.J[1] = c1 + c1;
    T.J[2] = c2 + c2;
    T.J[3] = nn[0];  // cloud_matcher.cpp:96-98
    T.J[4] = nn[1];
    T.J[5] = nn[2];
}
// The same terms the way the reference writes them (cloud_matcher.cpp:64-91 and Ceres' QuaternionManifold): four ambient
// derivatives times the 4x3 plus-Jacobian.  No kernel calls it; tests/cpp/test_point_terms.cpp holds point_terms to it.
__host__ __device__ __forceinline__ void point_terms_ambient(const float4 ra, const float4 rb, const float4 rc,
                                                             const double q0, const double q1, const double q2,
                                                             const double q3, const double t0, const double t1,
                                                             const double t2, PointTerms &T)
{
    PointGeom G;
    T.r = point_residual(ra, rb, rc, q0, q1, q2, q3, t0, t1, t2, G);
    const double *p = G.p, *nn = G.nn;
    // cloud_matcher.cpp:64-91: ambient d r / d q_i = (dR/dq_i p).n
    double v0, v1, v2, ja[4];
    v0 = 2.0 * q0 * p[0] + 2.0 * -q3 * p[1] + 2.0 * q2 * p[2];
    v1 = 2.0 * q3 * p[0] + 2.0 * q0 * p[1] + 2.0 * -q1 * p[2];
    v2 = 2.0 * -q2 * p[0] + 2.0 * q1 * p[1] + 2.0 * q0 * p[2];
    ja[0] = v0 * nn[0] + (v1 * nn[1] + v2 * nn[2]);
    v0 = 2.0 * q1 * p[0] + 2.0 * q2 * p[1] + 2.0 * q3 * p[2];
    v1 = 2.0 * q2 * p[0] + 2.0 * -q1 * p[1] + 2.0 * -q0 * p[2];
    v2 = 2.0 * q3 * p[0] + 2.0 * q0 * p[1] + 2.0 * -q1 * p[2];
    ja[1] = v0 * nn[0] + (v1 * nn[1] + v2 * nn[2]);
    v0 = 2.0 * -q2 * p[0] + 2.0 * q1 * p[1] + 2.0 * q0 * p[2];
    v1 = 2.0 * q1 * p[0] + 2.0 * q2 * p[1] + 2.0 * q3 * p[2];
    v2 = 2.0 * -q0 * p[0] + 2.0 * q3 * p[1] + 2.0 * -q2 * p[2];
    ja[2] = v0 * nn[0] + (v1 * nn[1] + v2 * nn[2]);
    v0 = 2.0 * -q3 * p[0] + 2.0 * -q0 * p[1] + 2.0 * q1 * p[2];
    v1 = 2.0 * q0 * p[0] + 2.0 * -q3 * p[1] + 2.0 * q2 * p[2];
    v2 = 2.0 * q1 * p[0] + 2.0 * q2 * p[1] + 2.0 * q3 * p[2];
    ja[3] = v0 * nn[0] + (v1 * nn[1] + v2 * nn[2]);
    // Ceres QuaternionManifold plus-Jacobian (4x3): ambient -> tangent
    T.J[0] = ja[0] * -q1 + ja[1] * q0 + ja[2] * -q3 + ja[3] * q2;
    T.J[1] = ja[0] * -q2 + ja[1] * q3 + ja[2] * q0 + ja[3] * -q1;
    T.J[2] = ja[0] * -q3 + ja[1] * -q2 + ja[2] * q1 + ja[3] * q0;
    T.J[3] = nn[0];  // cloud_matcher.cpp:96-98
    T.J[4] = nn[1];
    T.J[5] = nn[2];
}
// 1 / d to f64 rounding without the IEEE divide: an estimate and two Newton steps (lm_wave.hpp's fast_rcp).  The host
// form, for the comparison program, starts from an estimate 2^-24 off so that the steps have work to do there too.
__host__ __device__ __forceinline__ double huber_rcp(const double d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    double y = __builtin_amdgcn_rcp(d);
#else
    double y = (1.0 / d) * (1.0 + 0x1p-24);
#endif
    double e = __builtin_fma(-d, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-d, y, 1.0);
    return __builtin_fma(y, e, y);
}
// ceres::HuberLoss(0.15) (cloud_matcher.cpp:134) on s = r^2: rho = s, rho' = 1 up to s = 0.15^2; beyond it
// rho = 2 a sqrt(s) - a^2, rho' = a / sqrt(s), floored at DBL_MIN; rho'' <= 0 -> plain IRLS weight rho'.  sqrt(r r) is |r|
// to rounding, so neither a square root nor a divide nor a branch: two selects on |r| > 0.15 (strict, like s > 0.15^2:
// r = 0 and |r| = 0.15 take the quadratic side; the side not selected may hold inf or NaN, which a select drops).
struct HuberTerms {
    double rho, w;
};
__host__ __device__ __forceinline__ HuberTerms huber_terms(const double r)
{
    const double a = fabs(r);
    const bool big = a > 0.15;
    // both sides are computed before the selects: written inside them, the reciprocal stays behind a branch.
    // 2 a |r| - a^2 as a (2 |r| - a): one instruction more than 0.3 |r| - 0.0225, and two f64 constants fewer to keep in
    // scalar registers through the solve (as 0.3 |r| - 0.0225, k_lm<512,128,1> spilled six more of them)
    const double rho_big = 0.15 * (2.0 * a - 0.15), rho_small = r * r;
    const double w_big = fmax(DBL_MIN, 0.15 * huber_rcp(a));
    HuberTerms H;
    H.rho = big ? rho_big : rho_small;
    H.w = big ? w_big : 1.0;
    return H;
}
// the form it replaces, with the square root and the divide (tests/cpp/test_point_terms.cpp; no kernel calls it)
__host__ __device__ __forceinline__ HuberTerms huber_terms_sqrt(const double r)
{
    const double s = r * r;
    HuberTerms H = {s, 1.0};
    if (s > 0.15 * 0.15) {
        const double rr = sqrt(s);
        H.rho = 2.0 * 0.15 * rr - 0.15 * 0.15;
        H.w = fmax(DBL_MIN, 0.15 / rr);
    }
    return H;
}
// the robust weight, then the 28 sums
__host__ __device__ __forceinline__ void point_accumulate(const PointTerms &T, double acc[28])
{
    const double r = T.r;
    const HuberTerms H = huber_terms(r);
    const double rho0 = H.rho, w = H.w;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; a++) {
        const double wa = w * T.J[a];
#pragma unroll
        for (int b = a; b < 6; b++) acc[k++] += wa * T.J[b];
    }
#pragma unroll
    for (int a = 0; a < 6; a++) acc[21 + a] += w * T.J[a] * r;
    acc[27] += 0.5 * rho0;
}
// cloud_matcher.cpp:48-102 for one correspondence, accumulated into the 28 sums
__device__ __forceinline__ void accumulate_point(const float4 ra, const float4 rb, const float4 rc,
                                                 const double q0, const double q1, const double q2, const double q3,
                                                 const double qe, const double t0, const double t1, const double t2,
                                                 double acc[28])
{
    PointTerms T;
    point_terms(ra, rb, rc, q0, q1, q2, q3, qe, t0, t1, t2, T);
    point_accumulate(T, acc);
}
#pragma clang fp contract(off)

// Workgroup reduction of the 28 per-lane sums through LDS in a fixed order, plus the
// workgroup's slice of k_match's counters; one wave then writes the 256-byte record.
// s_acc: dynamic LDS, 28 rows of kAccStride doubles.
__device__ __forceinline__ void reduce_and_publish(const double acc[28], double *s_acc, unsigned long long *s_cnt,
                                                   const uint32_t *__restrict__ block_counters,
                                                   uint32_t n_match_blocks, double *out_rec,
                                                   unsigned long long seq, int mode)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < 28; k++) s_acc[k * kAccStride + tid] = acc[k];
    if (wave == 0 && n_match_blocks) {
        const uint32_t chunk = (n_match_blocks + gridDim.x - 1) / gridDim.x;
        const uint32_t lo = blockIdx.x * chunk;
        const uint32_t hi = min(lo + chunk, n_match_blocks);
        unsigned long long c0 = 0, c1 = 0, c2 = 0;
        for (uint32_t b = lo + lane; b < hi; b += 64) {
            const uint4 r = *reinterpret_cast<const uint4 *>(block_counters + (size_t)b * 4);
            c0 += r.x;
            c1 += r.y;
            c2 += r.z;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            c0 += __shfl_xor(c0, d, 64);
            c1 += __shfl_xor(c1, d, 64);
            c2 += __shfl_xor(c2, d, 64);
        }
        if (lane == 0) {
            s_cnt[0] = c0;
            s_cnt[1] = c1;
            s_cnt[2] = c2;
        }
    }
    __syncthreads();
    // thread (k = tid / 16, j = tid % 16) adds row k's elements j, j+16, ... in order
    const int k = tid >> 4, j = tid & 15;
    double v = 0.0;
    if (k < 28) {
        const double *row = s_acc + k * kAccStride + j;
#pragma unroll 8
        for (int i = 0; i < kEvalThreads / 16; i++) v += row[i * 16];
    }
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d, 16);
    __syncthreads();  // every read of s_acc is done: its first words become the staging row
    if (j == 0 && k < 28) s_acc[k] = v;
    __syncthreads();
    if (tid < 32) {  // one wave writes the whole 256-byte record
        double o = 0.0;
        if (tid < 28)
            o = s_acc[tid];
        else if (tid < 31)
            o = n_match_blocks ? (double)s_cnt[tid - 28] : 0.0;
        double *dst = out_rec + (size_t)blockIdx.x * kRecWords;
        if (mode == kPublishHost) {
            // payload as system-scope (write-through) stores, wait until they have left the wave,
            // then the sequence word: the same order a system-scope release gives, without its
            // L2 write-back pass (nothing this wave wrote is cached)
            if (tid < 31) __hip_atomic_store(dst + tid, o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (tid == 31)
                __hip_atomic_store(reinterpret_cast<unsigned long long *>(dst + 31), seq, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
        } else if (mode == kPublishDevice) {
            // to the other workgroups of this launch (any XCD): every store of the record
            // agent-coherent and drained before the sequence word; the readers use
            // agent-coherent loads for both
            if (tid < 31) __hip_atomic_store(dst + tid, o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (tid == 31)
                __hip_atomic_store(reinterpret_cast<unsigned long long *>(dst + 31), seq, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        } else if (tid < 31) {
            dst[tid] = o;
        }
    }
    __syncthreads();  // s_acc / s_cnt may be rewritten by the next evaluation
}

__global__ __launch_bounds__(kEvalThreads) void k_eval(const MatchRec *__restrict__ rec, uint32_t n, EvalArgs E,
                                                       const uint32_t *__restrict__ block_counters,
                                                       uint32_t n_match_blocks, double *out_rec,
                                                       unsigned long long seq)
{
    extern __shared__ __attribute__((aligned(16))) double s_acc[];
    __shared__ unsigned long long s_cnt[3];
    double acc[28];
#pragma unroll
    for (int k = 0; k < 28; k++) acc[k] = 0.0;
    const double qe = quat_excess(E.q[0], E.q[1], E.q[2], E.q[3]);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 *r4 = reinterpret_cast<const float4 *>(rec + i);
        const float4 ra = r4[0], rb = r4[1], rc = r4[2];
        if (rb.w != 0.f) accumulate_point(ra, rb, rc, E.q[0], E.q[1], E.q[2], E.q[3], qe, E.t[0], E.t[1], E.t[2], acc);
    }
    reduce_and_publish(acc, s_acc, s_cnt, block_counters, n_match_blocks, out_rec, seq, kPublishPlain);
}

__global__ __launch_bounds__(kEvalThreads) void k_eval_server(const MatchRec *__restrict__ rec, uint32_t n,
                                                              EvalArgs E0, const uint32_t *__restrict__ block_counters,
                                                              uint32_t n_match_blocks, double *out_rec,
                                                              unsigned long long seq0, const EvalCmd *cmd,
                                                              unsigned long long cmd_seen,
                                                              unsigned long long timeout_ticks)
{
    extern __shared__ __attribute__((aligned(16))) double s_acc[];
    __shared__ unsigned long long s_cnt[3];
    __shared__ EvalCmd s_cmd;
    const uint32_t first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    // this lane's first point stays in registers for every evaluation of the outer iteration
    float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra, rc = ra;
    if (first < n) {
        const float4 *r4 = reinterpret_cast<const float4 *>(rec + first);
        ra = r4[0];
        rb = r4[1];
        rc = r4[2];
    }
    double q0 = E0.q[0], q1 = E0.q[1], q2 = E0.q[2], q3 = E0.q[3], t0 = E0.t[0], t1 = E0.t[1], t2 = E0.t[2];
    unsigned long long seq = seq0;
    uint32_t counters_from = n_match_blocks;  // counters are folded by the first evaluation only
    for (;;) {
        double acc[28];
#pragma unroll
        for (int k = 0; k < 28; k++) acc[k] = 0.0;
        const double qe = quat_excess(q0, q1, q2, q3);
        if (rb.w != 0.f) accumulate_point(ra, rb, rc, q0, q1, q2, q3, qe, t0, t1, t2, acc);
        for (uint32_t i = first + step; i < n; i += step) {
            const float4 *r4 = reinterpret_cast<const float4 *>(rec + i);
            const float4 xa = r4[0], xb = r4[1], xc = r4[2];
            if (xb.w != 0.f) accumulate_point(xa, xb, xc, q0, q1, q2, q3, qe, t0, t1, t2, acc);
        }
        reduce_and_publish(acc, s_acc, s_cnt, block_counters, counters_from, out_rec, seq, kPublishHost);
        counters_from = 0;
        // wait for the next command from the host (bounded: the grid always drains).  The first
        // wave reads the 72-byte command with ONE instruction per poll (lanes 0..8, one word each,
        // relaxed system-scope loads: no cache invalidate per poll), then once more after the
        // sequence word changed -- the host wrote the payload before the sequence word.
        if (threadIdx.x < 64) {
            const int lane = threadIdx.x;
            unsigned long long *words = reinterpret_cast<unsigned long long *>(const_cast<EvalCmd *>(cmd));
            unsigned long long *my = words + (lane < 9 ? lane : 0);
            const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
            bool timed_out = false;
            for (;;) {
                const unsigned long long w = __hip_atomic_load(my, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if (__shfl(w, 0, 64) != cmd_seen) break;
                if (__builtin_amdgcn_s_memrealtime() - t_start > timeout_ticks) {
                    timed_out = true;  // host went away: leave
                    break;
                }
                __builtin_amdgcn_s_sleep(4);
            }
            const unsigned long long w = __hip_atomic_load(my, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (lane < 9) reinterpret_cast<unsigned long long *>(&s_cmd)[lane] = w;
            if (timed_out && lane == 0) s_cmd.op = kCmdStop;
        }
        __syncthreads();
        if (s_cmd.op != kCmdEval) return;  // uniform over the workgroup
        q0 = s_cmd.q[0];
        q1 = s_cmd.q[1];
        q2 = s_cmd.q[2];
        q3 = s_cmd.q[3];
        t0 = s_cmd.t[0];
        t1 = s_cmd.t[1];
        t2 = s_cmd.t[2];
        seq = s_cmd.seq;
        cmd_seen = s_cmd.seq;
        __syncthreads();  // s_cmd is rewritten by thread 0 in the next round
    }
}

}  // namespace lom
