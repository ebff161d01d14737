// Quality report of a pose: k_quality and k_quality_sum, and their K-problem forms k_quality_batch and k_quality_batch_sum
// (see quality_report.hip "quality report" and "batched quality report").  Device code only; match.hip
// is the one translation unit that instantiates and launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "k_eval.hpp"
#include "k_match.hpp"
#include "lom_internal.hpp"

namespace lom {

// ---------------------------------------------------------------------------
// One evaluation over the records a search left, at the report's pose: the align's own residual, Jacobian and 28 sums
// (point_terms / point_accumulate of k_eval.hpp) plus what a caller judges the pose by.  One lane per
// record, grid-stride; LOM_NQSUMS f64 values per lane:
//   [0..27] sum w J J^T (21), sum w J r (6), sum 0.5 rho     [28] sum w        [29] sum w r^2
//   [30] sum r^2 over valid   [31] sum r^2 over inliers      [32] sum |R p + t - o|^2
//   [33] valid records        [34] inliers (r^2 <= 0.15^2: the branch in which the Huber weight is 1)
//   [35] max |r|
// Reduction, in a fixed order throughout (the same inputs give the same bytes): inside a workgroup through LDS as
// reduce_and_publish does it, kQualRows values at a time (static LDS: 50 KB instead of 152 KB for all 36 at once);
// each workgroup leaves one record of LOM_NQSUMS doubles; k_quality_sum, one wave, adds the records in workgroup order
// and stores the totals straight into pinned host memory.  Sums add, [35] takes the maximum.
// ---------------------------------------------------------------------------
constexpr int kQualSums = LOM_NQSUMS;
constexpr int kQualMaxSlot = 35;
constexpr int kQualRows = 12;  // values per LDS pass; kQualSums = 3 passes
static_assert(kQualSums % kQualRows == 0 && kQualRows * 32 <= kEvalThreads, "one half-wave per row of a pass");

#pragma clang fp contract(fast)  // as k_eval.hpp: f64 sums compared to 1e-12 of their scale, not bit for bit
__device__ __forceinline__ void quality_point(const float4 ra, const float4 rb, const float4 rc, const EvalArgs &E,
                                              const double qe, double acc[kQualSums],
                                              float *__restrict__ residual_out, uint32_t i)
{
    if (rb.w == 0.f) {  // no correspondence
        if (residual_out) residual_out[i] = __builtin_nanf("");
        return;
    }
    const double q0 = E.q[0], q1 = E.q[1], q2 = E.q[2], q3 = E.q[3];
    PointTerms T;
    point_terms(ra, rb, rc, q0, q1, q2, q3, qe, E.t[0], E.t[1], E.t[2], T);
    point_accumulate(T, acc);
    const double r = T.r, s = r * r;
    const bool inlier = !(s > 0.15 * 0.15);
    // the weight point_accumulate applied, here still by huber_terms_sqrt's square root and divide (equal to rounding)
    double w = 1.0;
    if (!inlier) w = fmax(DBL_MIN, 0.15 / sqrt(s));
    // e = R p + t - o, the rotation as point_terms applies it
    const double p[3] = {(double)ra.x, (double)ra.y, (double)ra.z};
    double uv0 = q2 * p[2] - q3 * p[1];
    double uv1 = q3 * p[0] - q1 * p[2];
    double uv2 = q1 * p[1] - q2 * p[0];
    uv0 += uv0;
    uv1 += uv1;
    uv2 += uv2;
    const double rp0 = (p[0] + q0 * uv0) + (q2 * uv2 - q3 * uv1);
    const double rp1 = (p[1] + q0 * uv1) + (q3 * uv0 - q1 * uv2);
    const double rp2 = (p[2] + q0 * uv2) + (q1 * uv1 - q2 * uv0);
    const double e0 = rp0 + E.t[0] - (double)rb.x, e1 = rp1 + E.t[1] - (double)rb.y, e2 = rp2 + E.t[2] - (double)rb.z;
    acc[28] += w;
    acc[29] += w * s;
    acc[30] += s;
    acc[31] += inlier ? s : 0.0;
    acc[32] += e0 * e0 + (e1 * e1 + e2 * e2);
    acc[33] += 1.0;
    acc[34] += inlier ? 1.0 : 0.0;
    acc[kQualMaxSlot] = fmax(acc[kQualMaxSlot], fabs(r));
    if (residual_out) residual_out[i] = (float)r;
}
#pragma clang fp contract(off)

// k_quality's fold of a workgroup's values into its record, for the batch form (k_quality itself keeps the code it was
// verified with, statement for statement the same: inlining this function there reschedules its epilogue): half-wave
// (k = tid / 32) takes value pass * kQualRows + k -- lane j adds the lanes' entries j, j + 32, ... in order, then the 32
// partial results fold in a fixed butterfly.
__device__ __forceinline__ void quality_block_reduce(const double (&acc)[kQualSums], double *__restrict__ s_red,
                                                     double *__restrict__ out_rec, uint32_t block)
{
    const int tid = threadIdx.x, k = tid >> 5, j = tid & 31;
#pragma unroll
    for (int pass = 0; pass < kQualSums / kQualRows; pass++) {
        if (pass) __syncthreads();  // the previous pass's reads are done
#pragma unroll
        for (int a = 0; a < kQualRows; a++) s_red[a * kAccStride + tid] = acc[pass * kQualRows + a];
        __syncthreads();
        if (k < kQualRows) {
            const bool is_max = pass * kQualRows + k == kQualMaxSlot;
            const double *row = s_red + k * kAccStride + j;
            double v = 0.0;
#pragma unroll 8
            for (int i = 0; i < kEvalThreads / 32; i++) {
                const double x = row[i * 32];
                v = is_max ? fmax(v, x) : v + x;
            }
#pragma unroll
            for (int d = 16; d >= 1; d >>= 1) {
                const double x = __shfl_xor(v, d, 32);
                v = is_max ? fmax(v, x) : v + x;
            }
            if (j == 0) out_rec[(size_t)block * kQualSums + pass * kQualRows + k] = v;
        }
    }
}

// lane k < kQualSums: the workgroups' records in workgroup order -> total k
__device__ __forceinline__ void quality_sum_records(const double *__restrict__ rec, uint32_t n_rec,
                                                    double *__restrict__ out)
{
    const int k = threadIdx.x;
    if (k >= kQualSums) return;
    const bool is_max = k == kQualMaxSlot;
    double v = 0.0;
    for (uint32_t b = 0; b < n_rec; b++) {
        const double x = rec[(size_t)b * kQualSums + k];
        v = is_max ? fmax(v, x) : v + x;
    }
    out[k] = v;
}

// residual_out: n floats or nullptr.  ONE instantiation serves both: the report's bytes must not depend on whether the
// caller asked for the residuals, and two instantiations need not contract and order their f64 arithmetic alike.
__global__ __launch_bounds__(kEvalThreads) void k_quality(const MatchRec *__restrict__ rec, uint32_t n, EvalArgs E,
                                                          double *__restrict__ out_rec,
                                                          float *__restrict__ residual_out)
{
    __shared__ __attribute__((aligned(16))) double s_red[kQualRows * kAccStride];
    double acc[kQualSums];
#pragma unroll
    for (int k = 0; k < kQualSums; k++) acc[k] = 0.0;
    const double qe = quat_excess(E.q[0], E.q[1], E.q[2], E.q[3]);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 *r4 = reinterpret_cast<const float4 *>(rec + i);
        const float4 ra = r4[0], rb = r4[1], rc = r4[2];
        quality_point(ra, rb, rc, E, qe, acc, residual_out, i);
    }
    // half-wave (k = tid / 32) takes value pass * kQualRows + k: lane j adds the lanes' entries j, j + 32, ... in order,
    // then the 32 partial results fold in a fixed butterfly
    const int tid = threadIdx.x, k = tid >> 5, j = tid & 31;
#pragma unroll
    for (int pass = 0; pass < kQualSums / kQualRows; pass++) {
        if (pass) __syncthreads();  // the previous pass's reads are done
#pragma unroll
        for (int a = 0; a < kQualRows; a++) s_red[a * kAccStride + tid] = acc[pass * kQualRows + a];
        __syncthreads();
        if (k < kQualRows) {
            const bool is_max = pass * kQualRows + k == kQualMaxSlot;
            const double *row = s_red + k * kAccStride + j;
            double v = 0.0;
#pragma unroll 8
            for (int i = 0; i < kEvalThreads / 32; i++) {
                const double x = row[i * 32];
                v = is_max ? fmax(v, x) : v + x;
            }
#pragma unroll
            for (int d = 16; d >= 1; d >>= 1) {
                const double x = __shfl_xor(v, d, 32);
                v = is_max ? fmax(v, x) : v + x;
            }
            if (j == 0) out_rec[(size_t)blockIdx.x * kQualSums + pass * kQualRows + k] = v;
        }
    }
}

// one wave: the records of k_quality's workgroups in workgroup order -> the totals, in pinned host memory
__global__ __launch_bounds__(64) void k_quality_sum(const double *__restrict__ rec, uint32_t n_rec,
                                                    double *__restrict__ out)
{
    quality_sum_records(rec, n_rec, out);
}

// ---------------------------------------------------------------------------
// Batched form (lom_match_quality_batch*): K (scan, pose) problems of a round in one launch each of the search (the
// batch form of k_match, whose pose comes from a per-problem AlignState the host filled), the evaluation and the sum.
// blockIdx.y is the problem's place in the round; a problem keeps the evaluation grid the single report gives it
// (eval_grid(n) workgroups, the launch is sized for the round's largest and the others' surplus workgroups leave at
// once), so which lane sees which record and every reduction order depend on the problem's n alone: its totals do not
// depend on what else is in the batch, on the round size or on the problem's place.  No per-point residuals here.
// ---------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) QualBatchProblem *ConstQualBatch;  // scalar loads, like kernel arguments

__global__ __launch_bounds__(kEvalThreads) void k_quality_batch(const QualBatchProblem *batch)
{
    __shared__ __attribute__((aligned(16))) double s_red[kQualRows * kAccStride];
    const ConstQualBatch d = (ConstQualBatch)(batch + blockIdx.y);
    const uint32_t grid = d->grid, n = d->n;
    if (blockIdx.x >= grid) return;
    const MatchRec *__restrict__ rec = d->rec;
    EvalArgs E;
#pragma unroll
    for (int a = 0; a < 4; a++) E.q[a] = d->E.q[a];
#pragma unroll
    for (int a = 0; a < 3; a++) E.t[a] = d->E.t[a];
    double acc[kQualSums];
#pragma unroll
    for (int k = 0; k < kQualSums; k++) acc[k] = 0.0;
    const double qe = quat_excess(E.q[0], E.q[1], E.q[2], E.q[3]);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += grid * blockDim.x) {
        const float4 *r4 = reinterpret_cast<const float4 *>(rec + i);
        const float4 ra = r4[0], rb = r4[1], rc = r4[2];
        quality_point(ra, rb, rc, E, qe, acc, nullptr, i);
    }
    quality_block_reduce(acc, s_red, d->part, blockIdx.x);
}

// one wave per problem: its workgroups' records in workgroup order -> its totals in HBM (one copy per call fetches all)
__global__ __launch_bounds__(64) void k_quality_batch_sum(const QualBatchProblem *batch)
{
    const ConstQualBatch d = (ConstQualBatch)(batch + blockIdx.x);
    quality_sum_records(d->part, d->grid, d->out);
}

}  // namespace lom
