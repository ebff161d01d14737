// Pose graph kernels (definitions: include/lidar_odometry_amd.h, "pose graph"; launched by graph.hip alone).
// All f64.  An edge lane works on one edge, a node row (16 lanes) on one node; no kernel waits for another workgroup and
// none uses a floating-point atomic, so a result depends on the graph alone.
//
// Device records:  pose      [node][7]   t, q (w x y z)
//                  edge      ij [edge][2], Z [edge][7], U [edge][21] (Omega = U^T U, upper triangle row-major), delta [edge]
//                  B         [edge][2][36]  sqrt(w) U A_i, sqrt(w) U A_j, row-major 6x6
//                  c, u, e   [edge][6]
//                  node vectors (g, D, x, r, z, p, y) [node][6]; blocks (Hd, Minv) [node][36]
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lom {

constexpr int kGraphThreads = 256;
constexpr int kGraphRow = 16;                                    // lanes that share one node's incident edges
constexpr int kGraphRowsPerBlock = kGraphThreads / kGraphRow;    // nodes per workgroup of the node kernels

// scalars of one PCG solve, in HBM
struct GraphScalars {
    double rz, rz0, pAp, alpha, beta;
    int32_t done;   // 0 running, 1 converged, 2 broke down (p^T A p <= 0 or a value that is not a number)
    int32_t iters;
};

// what the host reads once per outer iteration (pinned host memory)
struct GraphReport {
    double cost, grad_max;              // at the current poses
    double cost_new, denom, step_max;   // of the step: cost at the candidate, d^T (lambda D d - g), max|d|
    int32_t pcg_iters, pcg_done;
};

enum { GRAPH_SCALAR_INIT = 0, GRAPH_SCALAR_ALPHA = 1, GRAPH_SCALAR_BETA = 2 };

__host__ __device__ constexpr int g_upper(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }  // r <= c
__host__ __device__ constexpr int g_lower(int r, int c) { return r * (r + 1) / 2 + c; }               // c <= r

__device__ inline void g_quat_mul(const double a[4], const double b[4], double o[4])
{
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

__device__ inline void g_quat_matrix(const double q[4], double R[9])
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z), R[1] = 2.0 * (x * y - w * z), R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z), R[4] = 1.0 - 2.0 * (x * x + z * z), R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y), R[7] = 2.0 * (y * z + w * x), R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// rotation vector in (-pi, pi] of a unit quaternion
__device__ inline void g_quat_log(const double q[4], double r[3])
{
    const double sgn = q[0] < 0.0 ? -1.0 : 1.0;
    const double w = sgn * q[0], x = sgn * q[1], y = sgn * q[2], z = sgn * q[3];
    const double n = sqrt(x * x + y * y + z * z);
    const double k = n < 1e-12 ? 2.0 / w : 2.0 * atan2(n, w) / n;
    r[0] = k * x, r[1] = k * y, r[2] = k * z;
}

// Jl^-1(p) = I - 0.5 [p]x + c [p]x^2
__device__ inline void g_jl_inv(const double p[3], double J[9])
{
    const double th2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    const double th = sqrt(th2);
    const double c = th < 1e-8 ? 1.0 / 12.0 : 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
    // [p]x^2 = p p^T - th^2 I
    J[0] = 1.0 + c * (p[0] * p[0] - th2), J[1] = c * p[0] * p[1] + 0.5 * p[2], J[2] = c * p[0] * p[2] - 0.5 * p[1];
    J[3] = c * p[1] * p[0] - 0.5 * p[2], J[4] = 1.0 + c * (p[1] * p[1] - th2), J[5] = c * p[1] * p[2] + 0.5 * p[0];
    J[6] = c * p[2] * p[0] + 0.5 * p[1], J[7] = c * p[2] * p[1] - 0.5 * p[0], J[8] = 1.0 + c * (p[2] * p[2] - th2);
}

// X (+) d: R <- R Exp(a), t <- t + b, the quaternion re-normalised; a fixed node keeps its bytes
__device__ inline void g_retract(const double *X, const double *d, int fixed, double out[7])
{
    if (fixed) {
#pragma unroll
        for (int a = 0; a < 7; a++) out[a] = X[a];
        return;
    }
    const double a0 = d[0], a1 = d[1], a2 = d[2];
    const double th2 = a0 * a0 + a1 * a1 + a2 * a2, th = sqrt(th2);
    const double k = th < 1e-6 ? 0.5 - th2 / 48.0 : sin(0.5 * th) / th;
    const double dq[4] = {cos(0.5 * th), k * a0, k * a1, k * a2};
    const double q[4] = {X[3], X[4], X[5], X[6]};
    double o[4];
    g_quat_mul(q, dq, o);
    const double nrm = sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
    out[0] = X[0] + d[3], out[1] = X[1] + d[4], out[2] = X[2] + d[5];
    out[3] = o[0] / nrm, out[4] = o[1] / nrm, out[5] = o[2] / nrm, out[6] = o[3] / nrm;
}

// e = [ Log(R_i^T R_j R_z^T) ; R_i^T (t_j - t_i) - t_z ]; also R_i and t_ij for the Jacobians
__device__ inline void g_edge_error(const double Xi[7], const double Xj[7], const double Z[7], double Ri[9], double tij[3],
                                    double e[6])
{
    const double qic[4] = {Xi[3], -Xi[4], -Xi[5], -Xi[6]}, qj[4] = {Xj[3], Xj[4], Xj[5], Xj[6]};
    const double qzc[4] = {Z[3], -Z[4], -Z[5], -Z[6]}, qi[4] = {Xi[3], Xi[4], Xi[5], Xi[6]};
    double a[4], qe[4];
    g_quat_mul(qic, qj, a);
    g_quat_mul(a, qzc, qe);
    g_quat_log(qe, e);
    g_quat_matrix(qi, Ri);
    const double d0 = Xj[0] - Xi[0], d1 = Xj[1] - Xi[1], d2 = Xj[2] - Xi[2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        tij[k] = Ri[k] * d0 + Ri[3 + k] * d1 + Ri[6 + k] * d2;  // column k of R_i
        e[3 + k] = tij[k] - Z[k];
    }
}

// ue = U e, s = |ue|^2 = e^T Omega e, the Huber weight and rho(s)
__device__ inline void g_edge_loss(const double U[21], const double e[6], double delta, double ue[6], double &s, double &w,
                                   double &rho)
{
    s = 0.0;
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double v = 0.0;
#pragma unroll
        for (int c = r; c < 6; c++) v += U[g_upper(r, c)] * e[c];
        ue[r] = v;
        s += v * v;
    }
    if (delta == 0.0 || s <= delta * delta) {
        w = 1.0;
        rho = s;
    } else {
        const double rs = sqrt(s);
        w = delta / rs;
        rho = 2.0 * delta * rs - delta * delta;
    }
}

__device__ inline void g_load7(const double *p, double out[7])
{
#pragma unroll
    for (int a = 0; a < 7; a++) out[a] = p[a];
}

// sw * U * A for A = [ TL 0 ; BL BR ] (3x3 blocks), into out[36]
template <bool HAS_BL>
__device__ inline void g_whiten_store(const double U[21], double sw, const double TL[9], const double BL[9],
                                      const double BR[9], double *out)
{
#pragma unroll
    for (int r = 0; r < 6; r++) {
#pragma unroll
        for (int col = 0; col < 6; col++) {
            double v = 0.0;
            if (col < 3) {
#pragma unroll
                for (int k = r; k < 6; k++) {
                    if (k < 3)
                        v += U[g_upper(r, k)] * TL[k * 3 + col];
                    else if (HAS_BL)
                        v += U[g_upper(r, k)] * BL[(k - 3) * 3 + col];
                }
            } else {
#pragma unroll
                for (int k = (r > 3 ? r : 3); k < 6; k++) v += U[g_upper(r, k)] * BR[(k - 3) * 3 + (col - 3)];
            }
            out[r * 6 + col] = sw * v;
        }
    }
}

// One lane per edge: e, s, w, the edge's cost, c = sqrt(w) U e and the two whitened Jacobian blocks.
__global__ __launch_bounds__(kGraphThreads) void k_graph_linearise(uint32_t m, const double *__restrict__ pose,
                                                                   const int32_t *__restrict__ ij,
                                                                   const double *__restrict__ Zs,
                                                                   const double *__restrict__ Us,
                                                                   const double *__restrict__ deltas, double *__restrict__ e_out,
                                                                   double *__restrict__ s_out, double *__restrict__ w_out,
                                                                   double *__restrict__ cost_out, double *__restrict__ B,
                                                                   double *__restrict__ c_out)
{
    const uint32_t ed = blockIdx.x * kGraphThreads + threadIdx.x;
    if (ed >= m) return;
    double Xi[7], Xj[7], Z[7], U[21];
    g_load7(pose + (size_t)ij[2 * ed] * 7, Xi);
    g_load7(pose + (size_t)ij[2 * ed + 1] * 7, Xj);
    g_load7(Zs + (size_t)ed * 7, Z);
#pragma unroll
    for (int k = 0; k < 21; k++) U[k] = Us[(size_t)ed * 21 + k];
    double Ri[9], tij[3], e[6], ue[6], s, w, rho;
    g_edge_error(Xi, Xj, Z, Ri, tij, e);
    g_edge_loss(U, e, deltas[ed], ue, s, w, rho);
    const double sw = sqrt(w);
#pragma unroll
    for (int r = 0; r < 6; r++) {
        e_out[(size_t)ed * 6 + r] = e[r];
        c_out[(size_t)ed * 6 + r] = sw * ue[r];
    }
    s_out[ed] = s;
    w_out[ed] = w;
    cost_out[ed] = 0.5 * rho;

    double J[9], TL[9], BL[9], BR[9];
    // A_i = [ -Jl^-1(e_r), 0 ; [t_ij]x, -R_i^T ]
    g_jl_inv(e, J);
#pragma unroll
    for (int k = 0; k < 9; k++) TL[k] = -J[k];
    BL[0] = 0.0, BL[1] = -tij[2], BL[2] = tij[1];
    BL[3] = tij[2], BL[4] = 0.0, BL[5] = -tij[0];
    BL[6] = -tij[1], BL[7] = tij[0], BL[8] = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) BR[a * 3 + b] = -Ri[b * 3 + a];
    g_whiten_store<true>(U, sw, TL, BL, BR, B + (size_t)ed * 72);
    // A_j = [ Jl^-1(-e_r) R_z, 0 ; 0, R_i^T ]
    const double me[3] = {-e[0], -e[1], -e[2]}, qz[4] = {Z[3], Z[4], Z[5], Z[6]};
    double Rz[9];
    g_jl_inv(me, J);
    g_quat_matrix(qz, Rz);
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            TL[a * 3 + b] = J[a * 3] * Rz[b] + J[a * 3 + 1] * Rz[3 + b] + J[a * 3 + 2] * Rz[6 + b];
            BR[a * 3 + b] = Ri[b * 3 + a];
        }
    g_whiten_store<false>(U, sw, TL, BL, BR, B + (size_t)ed * 72 + 36);
}

// sum over the 16 lanes of a row in lane order; every lane of the row gets the total
__device__ inline double g_row_sum(double v)
{
    double tot = __shfl(v, 0, kGraphRow);
#pragma unroll 1  // (unrolled, the 15 reads of all 27 sums of a gather are in flight at once and spill)
    for (int l = 1; l < kGraphRow; l++) tot += __shfl(v, l, kGraphRow);
    return tot;
}

// One 16-lane row per node over the CSR of its incident edges (ascending edge id): g_n = sum B^T c, the diagonal block
// H_nn = sum B^T B, D_n = diag(H_nn), Hd = H_nn + lambda D_n and Minv = Hd^-1 by Cholesky in lane 0.  The node's k-th
// incident edge goes to lane k mod 16, each lane adds its edges in ascending order, and the lanes' sums are added in lane
// order: a hub does not run in one lane, and the order is fixed.  A fixed node's outputs read 0.
__global__ __launch_bounds__(kGraphThreads) void k_graph_node_gather(uint32_t n, const int32_t *__restrict__ fixed,
                                                                     const uint32_t *__restrict__ row_ptr,
                                                                     const uint32_t *__restrict__ ent,
                                                                     const double *__restrict__ B,
                                                                     const double *__restrict__ c, double lambda,
                                                                     double *__restrict__ g, double *__restrict__ Hd,
                                                                     double *__restrict__ D, double *__restrict__ Minv)
{
    const uint32_t node = blockIdx.x * kGraphRowsPerBlock + (threadIdx.x / kGraphRow);
    const uint32_t lane = threadIdx.x % kGraphRow;
    if (node >= n) return;
    if (fixed[node]) {
        for (uint32_t k = lane; k < 36; k += kGraphRow) Hd[(size_t)node * 36 + k] = 0.0, Minv[(size_t)node * 36 + k] = 0.0;
        if (lane < 6) g[(size_t)node * 6 + lane] = 0.0, D[(size_t)node * 6 + lane] = 0.0;
        return;
    }
    double acc[27];
#pragma unroll
    for (int q = 0; q < 27; q++) acc[q] = 0.0;
    const uint32_t end = row_ptr[node + 1];
    for (uint32_t k = row_ptr[node] + lane; k < end; k += kGraphRow) {
        const uint32_t en = ent[k];
        const double *bp = B + (size_t)(en >> 1) * 72 + (en & 1u) * 36;
        const double *cp = c + (size_t)(en >> 1) * 6;
        double b[36], cv[6];
#pragma unroll
        for (int q = 0; q < 36; q++) b[q] = bp[q];
#pragma unroll
        for (int q = 0; q < 6; q++) cv[q] = cp[q];
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int b2 = a; b2 < 6; b2++) {
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < 6; r++) v += b[r * 6 + a] * b[r * 6 + b2];
                acc[g_upper(a, b2)] += v;
            }
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < 6; r++) v += b[r * 6 + a] * cv[r];
            acc[21 + a] += v;
        }
    }
#pragma unroll
    for (int q = 0; q < 27; q++) acc[q] = g_row_sum(acc[q]);
    if (lane != 0) return;
    // Hd = H_nn + lambda D_n and its inverse by Cholesky, triangles packed: L and Li = L^-1 lower, row-major
    double L[21], Li[21];
#pragma unroll
    for (int a = 0; a < 6; a++) {
        g[(size_t)node * 6 + a] = acc[21 + a];
        D[(size_t)node * 6 + a] = acc[g_upper(a, a)];
        acc[g_upper(a, a)] += lambda * acc[g_upper(a, a)];
    }
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b2 = 0; b2 < 6; b2++) Hd[(size_t)node * 36 + a * 6 + b2] = a <= b2 ? acc[g_upper(a, b2)] : acc[g_upper(b2, a)];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double d = acc[g_upper(j, j)];
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[g_lower(j, k)] * L[g_lower(j, k)];
        ok = ok && d > 0.0;
        L[g_lower(j, j)] = sqrt(d);
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = acc[g_upper(j, i)];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[g_lower(i, k)] * L[g_lower(j, k)];
            L[g_lower(i, j)] = v / L[g_lower(j, j)];
        }
    }
#pragma unroll
    for (int col = 0; col < 6; col++) {
        Li[g_lower(col, col)] = 1.0 / L[g_lower(col, col)];
#pragma unroll
        for (int i = col + 1; i < 6; i++) {
            double v = 0.0;
#pragma unroll
            for (int k = col; k < i; k++) v += L[g_lower(i, k)] * Li[g_lower(k, col)];
            Li[g_lower(i, col)] = -v / L[g_lower(i, i)];
        }
    }
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b2 = a; b2 < 6; b2++) {  // Hd^-1 = Li^T Li
            double v = 0.0;
#pragma unroll
            for (int k = b2; k < 6; k++) v += Li[g_lower(k, a)] * Li[g_lower(k, b2)];
            v = (ok && v == v) ? v : 0.0;
            Minv[(size_t)node * 36 + a * 6 + b2] = v;
            Minv[(size_t)node * 36 + b2 * 6 + a] = v;
        }
}

// Mat-vec, edge pass: u_e = B_i p_i + B_j p_j, a fixed node's p taken as zero.
__global__ __launch_bounds__(kGraphThreads) void k_graph_mv_edge(uint32_t m, const int32_t *__restrict__ ij,
                                                                 const int32_t *__restrict__ fixed,
                                                                 const double *__restrict__ B, const double *__restrict__ p,
                                                                 double *__restrict__ u, const GraphScalars *__restrict__ sc)
{
    if (sc->done) return;
    const uint32_t ed = blockIdx.x * kGraphThreads + threadIdx.x;
    if (ed >= m) return;
    const int32_t i = ij[2 * ed], j = ij[2 * ed + 1];
    const bool fi = fixed[i] != 0, fj = fixed[j] != 0;
    double pi[6], pj[6];
#pragma unroll
    for (int a = 0; a < 6; a++) {
        pi[a] = fi ? 0.0 : p[(size_t)i * 6 + a];
        pj[a] = fj ? 0.0 : p[(size_t)j * 6 + a];
    }
    const double *bp = B + (size_t)ed * 72;
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double v = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) v += bp[r * 6 + a] * pi[a];
#pragma unroll
        for (int a = 0; a < 6; a++) v += bp[36 + r * 6 + a] * pj[a];
        u[(size_t)ed * 6 + r] = v;
    }
}

// Mat-vec, node pass: y_n = sum_e B_{e,n}^T u_e + lambda D_n p_n, rows as in k_graph_node_gather, and the workgroup's
// partial of p^T y (its 16 nodes in order).
__global__ __launch_bounds__(kGraphThreads) void k_graph_mv_node(uint32_t n, const int32_t *__restrict__ fixed,
                                                                 const uint32_t *__restrict__ row_ptr,
                                                                 const uint32_t *__restrict__ ent,
                                                                 const double *__restrict__ B, const double *__restrict__ u,
                                                                 const double *__restrict__ D, double lambda,
                                                                 const double *__restrict__ p, double *__restrict__ y,
                                                                 double *__restrict__ partial,
                                                                 const GraphScalars *__restrict__ sc)
{
    __shared__ double dots[kGraphRowsPerBlock];
    if (sc->done) return;
    const uint32_t row = threadIdx.x / kGraphRow, lane = threadIdx.x % kGraphRow;
    const uint32_t node = blockIdx.x * kGraphRowsPerBlock + row;
    const bool live = node < n && !fixed[node];
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) {
        const uint32_t end = row_ptr[node + 1];
        for (uint32_t k = row_ptr[node] + lane; k < end; k += kGraphRow) {
            const uint32_t en = ent[k];
            const double *bp = B + (size_t)(en >> 1) * 72 + (en & 1u) * 36;
            const double *up = u + (size_t)(en >> 1) * 6;
            double uv[6];
#pragma unroll
            for (int r = 0; r < 6; r++) uv[r] = up[r];
#pragma unroll
            for (int a = 0; a < 6; a++) {
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < 6; r++) v += bp[r * 6 + a] * uv[r];
                acc[a] += v;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 6; a++) acc[a] = g_row_sum(acc[a]);
    if (lane == 0) {
        double dot = 0.0;
        if (node < n) {
#pragma unroll
            for (int a = 0; a < 6; a++) {
                const double pa = live ? p[(size_t)node * 6 + a] : 0.0;
                const double ya = live ? acc[a] + lambda * D[(size_t)node * 6 + a] * pa : 0.0;
                y[(size_t)node * 6 + a] = ya;
                dot += pa * ya;
            }
        }
        dots[row] = dot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int r = 0; r < kGraphRowsPerBlock; r++) tot += dots[r];
        partial[blockIdx.x] = tot;
    }
}

// fixed tree over the workgroup's 256 values
__device__ inline double g_block_sum(double v, double *lds)
{
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = kGraphThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    return lds[0];
}

// PCG start, one lane per node: x = 0, r = -g, z = Minv r, p = z, and the workgroup's partial of r^T z.
__global__ __launch_bounds__(kGraphThreads) void k_graph_cg_init(uint32_t n, const double *__restrict__ g,
                                                                 const double *__restrict__ Minv, double *__restrict__ x,
                                                                 double *__restrict__ r, double *__restrict__ z,
                                                                 double *__restrict__ p, double *__restrict__ partial)
{
    __shared__ double lds[kGraphThreads];
    const uint32_t node = blockIdx.x * kGraphThreads + threadIdx.x;
    double dot = 0.0;
    if (node < n) {
        double rv[6];
#pragma unroll
        for (int a = 0; a < 6; a++) rv[a] = -g[(size_t)node * 6 + a];
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double v = 0.0;
#pragma unroll
            for (int b = 0; b < 6; b++) v += Minv[(size_t)node * 36 + a * 6 + b] * rv[b];
            x[(size_t)node * 6 + a] = 0.0;
            r[(size_t)node * 6 + a] = rv[a];
            z[(size_t)node * 6 + a] = v;
            p[(size_t)node * 6 + a] = v;
            dot += rv[a] * v;
        }
    }
    const double tot = g_block_sum(dot, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// One workgroup finishes a dot product from the partials (thread t adds partials t, t + 256, ... in order, then the
// tree) and writes the solve's scalars.
__global__ __launch_bounds__(kGraphThreads) void k_graph_cg_scalar(int mode, uint32_t count,
                                                                   const double *__restrict__ partial, double rtol2,
                                                                   GraphScalars *__restrict__ sc)
{
    __shared__ double lds[kGraphThreads];
    if (mode != GRAPH_SCALAR_INIT && sc->done) return;
    double v = 0.0;
    for (uint32_t k = threadIdx.x; k < count; k += kGraphThreads) v += partial[k];
    const double tot = g_block_sum(v, lds);
    if (threadIdx.x != 0) return;
    if (mode == GRAPH_SCALAR_INIT) {
        sc->rz = tot, sc->rz0 = tot, sc->pAp = 0.0, sc->alpha = 0.0, sc->beta = 0.0;
        sc->iters = 0;
        sc->done = tot > 0.0 ? 0 : (tot == 0.0 ? 1 : 2);
    } else if (mode == GRAPH_SCALAR_ALPHA) {
        sc->pAp = tot;
        if (tot > 0.0)
            sc->alpha = sc->rz / tot;
        else
            sc->done = 2;
    } else {
        sc->iters += 1;
        if (tot != tot)
            sc->done = 2;
        else if (tot <= rtol2 * sc->rz0)
            sc->done = 1;
        sc->beta = tot / sc->rz;
        sc->rz = tot;
    }
}

// x += alpha p, r -= alpha y, z = Minv r, and the workgroup's partial of r^T z; one lane per node
__global__ __launch_bounds__(kGraphThreads) void k_graph_cg_update(uint32_t n, const double *__restrict__ Minv,
                                                                   const double *__restrict__ p, const double *__restrict__ y,
                                                                   double *__restrict__ x, double *__restrict__ r,
                                                                   double *__restrict__ z, double *__restrict__ partial,
                                                                   const GraphScalars *__restrict__ sc)
{
    __shared__ double lds[kGraphThreads];
    if (sc->done) return;
    const double alpha = sc->alpha;
    const uint32_t node = blockIdx.x * kGraphThreads + threadIdx.x;
    double dot = 0.0;
    if (node < n) {
        double rv[6];
#pragma unroll
        for (int a = 0; a < 6; a++) {
            x[(size_t)node * 6 + a] += alpha * p[(size_t)node * 6 + a];
            rv[a] = r[(size_t)node * 6 + a] - alpha * y[(size_t)node * 6 + a];
            r[(size_t)node * 6 + a] = rv[a];
        }
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double v = 0.0;
#pragma unroll
            for (int b = 0; b < 6; b++) v += Minv[(size_t)node * 36 + a * 6 + b] * rv[b];
            z[(size_t)node * 6 + a] = v;
            dot += rv[a] * v;
        }
    }
    const double tot = g_block_sum(dot, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// p = z + beta p, one lane per value
__global__ __launch_bounds__(kGraphThreads) void k_graph_cg_dir(uint32_t count, const double *__restrict__ z,
                                                                double *__restrict__ p, const GraphScalars *__restrict__ sc)
{
    if (sc->done) return;
    const uint32_t k = blockIdx.x * kGraphThreads + threadIdx.x;
    if (k < count) p[k] = z[k] + sc->beta * p[k];
}

// x (+) d into the candidate poses (lane k < n: node k), and the cost at the candidate (lane k < m: edge k, which
// retracts its own two nodes the same way): k_graph_linearise's cost path without the blocks.
__global__ __launch_bounds__(kGraphThreads) void k_graph_retract_cost(uint32_t n, uint32_t m, const double *__restrict__ pose,
                                                                      const int32_t *__restrict__ fixed,
                                                                      const double *__restrict__ d, double *__restrict__ cand,
                                                                      const int32_t *__restrict__ ij,
                                                                      const double *__restrict__ Zs,
                                                                      const double *__restrict__ Us,
                                                                      const double *__restrict__ deltas,
                                                                      double *__restrict__ cost_out)
{
    const uint32_t k = blockIdx.x * kGraphThreads + threadIdx.x;
    if (k < n) {
        double out[7];
        g_retract(pose + (size_t)k * 7, d + (size_t)k * 6, fixed[k], out);
#pragma unroll
        for (int a = 0; a < 7; a++) cand[(size_t)k * 7 + a] = out[a];
    }
    if (k >= m) return;
    const int32_t i = ij[2 * k], j = ij[2 * k + 1];
    double Xi[7], Xj[7], Z[7], U[21];
    g_retract(pose + (size_t)i * 7, d + (size_t)i * 6, fixed[i], Xi);
    g_retract(pose + (size_t)j * 7, d + (size_t)j * 6, fixed[j], Xj);
    g_load7(Zs + (size_t)k * 7, Z);
#pragma unroll
    for (int q = 0; q < 21; q++) U[q] = Us[(size_t)k * 21 + q];
    double Ri[9], tij[3], e[6], ue[6], s, w, rho;
    g_edge_error(Xi, Xj, Z, Ri, tij, e);
    g_edge_loss(U, e, deltas[k], ue, s, w, rho);
    cost_out[k] = 0.5 * rho;
}

// fixed tree over a wave's 64 values
__device__ inline double g_wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return __shfl(v, 0, 64);
}
__device__ inline double g_wave_max(double v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return __shfl(v, 0, 64);
}

// One wave: the scalars the host needs per outer iteration, to the pinned report.  Lane l adds values l, l + 64, ... in
// order, then the tree.  with_step == 0: cost and max|g| alone.
__global__ __launch_bounds__(64) void k_graph_report(uint32_t n, uint32_t m, const double *__restrict__ cost_e,
                                                     const double *__restrict__ cost_c, const double *__restrict__ g,
                                                     const double *__restrict__ D, const double *__restrict__ d, double lambda,
                                                     int with_step, const GraphScalars *__restrict__ sc,
                                                     GraphReport *__restrict__ report)
{
    const uint32_t lane = threadIdx.x;
    double cost = 0.0, cost_new = 0.0, denom = 0.0, gmax = 0.0, dmax = 0.0;
    for (uint32_t k = lane; k < m; k += 64) {
        cost += cost_e[k];
        if (with_step) cost_new += cost_c[k];
    }
    for (uint32_t k = lane; k < n * 6; k += 64) {
        const double gv = g[k];
        gmax = fabs(gv) > gmax ? fabs(gv) : gmax;
        if (with_step) {
            const double dv = d[k];
            denom += dv * (lambda * D[k] * dv - gv);
            dmax = fabs(dv) > dmax ? fabs(dv) : dmax;
        }
    }
    cost = g_wave_sum(cost), cost_new = g_wave_sum(cost_new), denom = g_wave_sum(denom);
    gmax = g_wave_max(gmax), dmax = g_wave_max(dmax);
    if (lane == 0) {
        report->cost = cost, report->grad_max = gmax;
        report->cost_new = cost_new, report->denom = denom, report->step_max = dmax;
        report->pcg_iters = with_step ? sc->iters : 0;
        report->pcg_done = with_step ? sc->done : 0;
    }
}

}  // namespace lom
