// Host math of the align quality report (lom_quality_from_sums): counts and fit figures, the full information matrix,
// the spectra of its translation and rotation blocks, and the pose covariance by Cholesky.  Plain C++, no HIP: the
// device part (k_quality.hpp, launched by match.hip for quality_report.hip) only produces the LOM_NQSUMS reduced values this file reads.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/lidar_odometry_amd.h"

namespace {

// Cyclic Jacobi on a symmetric 3x3 (row-major), eigenvalues ascending in w, row k of V the unit eigenvector of w[k].
// A rotation is skipped where the off-diagonal entry is exactly zero, so a matrix that is diagonal already comes back
// with its diagonal untouched (an unconstrained axis reads exactly 0.0).
void eig_sym3(const double A_in[9], double w[3], double V[9])
{
    double A[3][3], U[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};  // columns of U: eigenvectors
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) A[i][j] = A_in[i * 3 + j];
    for (int sweep = 0; sweep < 32; sweep++) {
        const double off = std::fabs(A[0][1]) + std::fabs(A[0][2]) + std::fabs(A[1][2]);
        if (off == 0.0) break;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                // Rutishauser's formulas: t = tan of the rotation angle, the smaller root
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
                const int r = 3 - p - q;  // the third index
                const double arp = A[r][p], arq = A[r][q];
                A[r][p] = A[p][r] = c * arp - s * arq;
                A[r][q] = A[q][r] = s * arp + c * arq;
                for (int k = 0; k < 3; k++) {
                    const double ukp = U[k][p], ukq = U[k][q];
                    U[k][p] = c * ukp - s * ukq;
                    U[k][q] = s * ukp + c * ukq;
                }
            }
    }
    int order[3] = {0, 1, 2};
    std::sort(order, order + 3, [&](int a, int b) { return A[a][a] < A[b][b] || (A[a][a] == A[b][b] && a < b); });
    for (int k = 0; k < 3; k++) {
        w[k] = A[order[k]][order[k]];
        for (int i = 0; i < 3; i++) V[k * 3 + i] = U[i][order[k]];
    }
}

// eigenvalues / eigenvectors of block / scale and the count of eigenvalues below `min_eig`
void block_spectrum(const double block[9], double scale, float min_eig, double w[3], double V[9], int32_t *degenerate)
{
    double B[9];
    bool finite = std::isfinite(scale);
    for (int i = 0; i < 9; i++) {
        B[i] = scale > 0.0 ? block[i] / scale : 0.0;
        finite = finite && std::isfinite(B[i]);
    }
    *degenerate = 0;
    if (!finite) {
        for (int i = 0; i < 3; i++) w[i] = NAN;
        for (int i = 0; i < 9; i++) V[i] = NAN;
        return;
    }
    eig_sym3(B, w, V);
    if (min_eig > 0.f)
        for (int i = 0; i < 3; i++) *degenerate += w[i] < (double)min_eig;
}

// inv(M) of a symmetric positive definite 6x6 by Cholesky; false where a pivot is <= 0 or anything is non-finite
bool spd_inverse6(const double M[36], double inv[36])
{
    double L[6][6] = {};
    for (int j = 0; j < 6; j++) {
        double d = M[j * 6 + j];
        for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        L[j][j] = std::sqrt(d);
        for (int i = j + 1; i < 6; i++) {
            double v = M[i * 6 + j];
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
            if (!std::isfinite(L[i][j])) return false;
        }
    }
    for (int c = 0; c < 6; c++) {  // L L^T x = e_c
        double y[6], x[6];
        for (int i = 0; i < 6; i++) {
            double v = i == c ? 1.0 : 0.0;
            for (int k = 0; k < i; k++) v -= L[i][k] * y[k];
            y[i] = v / L[i][i];
        }
        for (int i = 5; i >= 0; i--) {
            double v = y[i];
            for (int k = i + 1; k < 6; k++) v -= L[k][i] * x[k];
            x[i] = v / L[i][i];
        }
        for (int i = 0; i < 6; i++) {
            if (!std::isfinite(x[i])) return false;
            inv[i * 6 + c] = x[i];
        }
    }
    for (int i = 0; i < 6; i++)  // the two triangles agree to rounding: make them agree exactly
        for (int j = i + 1; j < 6; j++) inv[i * 6 + j] = inv[j * 6 + i] = 0.5 * (inv[i * 6 + j] + inv[j * 6 + i]);
    return true;
}

}  // namespace

extern "C" int lom_quality_from_sums(const double sums[LOM_NQSUMS], int64_t queries, float min_eig_t, float min_eig_r,
                                     lom_quality_report *out)
{
    if (!sums || !out || queries < 0) return LOM_ERR_ARG;
    lom_quality_report &r = *out;
    std::memset(&r, 0, sizeof r);
    const double valid_d = sums[33], inliers_d = sums[34];
    // (counts arrive as exact f64 integers; anything else -- NaN, negative -- reads as none)
    r.queries = queries;
    r.valid = (valid_d >= 0.0 && valid_d < 9.0e18) ? (int64_t)valid_d : 0;
    r.inliers = (inliers_d >= 0.0 && inliers_d < 9.0e18) ? (int64_t)inliers_d : 0;
    r.overlap = queries > 0 ? (double)r.valid / (double)queries : 0.0;
    r.cost = sums[27];
    r.rmse = r.valid > 0 ? std::sqrt(sums[30] / (double)r.valid) : 0.0;
    r.rmse_inliers = r.inliers > 0 ? std::sqrt(sums[31] / (double)r.inliers) : 0.0;
    r.max_abs_residual = sums[35];
    r.mean_sq_dist = r.valid > 0 ? sums[32] / (double)r.valid : 0.0;
    r.sigma2 = sums[29] / (double)std::max<int64_t>(1, r.valid - 6);
    r.sum_w = sums[28];
    int k = 0;
    for (int a = 0; a < 6; a++)
        for (int b = a; b < 6; b++) r.information[a * 6 + b] = r.information[b * 6 + a] = sums[k++];
    for (int a = 0; a < 6; a++) r.gradient[a] = sums[21 + a];

    double Htt[9], Hrr[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            Hrr[i * 3 + j] = r.information[i * 6 + j];
            Htt[i * 3 + j] = r.information[(3 + i) * 6 + 3 + j];
        }
    block_spectrum(Htt, r.sum_w, min_eig_t, r.eig_t, r.eigvec_t, &r.degenerate_t);
    block_spectrum(Hrr, 4.0 * r.sum_w, min_eig_r, r.eig_r, r.eigvec_r, &r.degenerate_r);

    // nav_msgs order: M = S P H P^T S, translation first, the half-angle tangent rescaled to radians
    if (r.valid >= 7 && std::isfinite(r.sigma2)) {
        static const int perm[6] = {3, 4, 5, 0, 1, 2};
        static const double scale[6] = {1.0, 1.0, 1.0, 0.5, 0.5, 0.5};
        double M[36], inv[36];
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) M[i * 6 + j] = scale[i] * scale[j] * r.information[perm[i] * 6 + perm[j]];
        if (spd_inverse6(M, inv)) {
            bool finite = true;
            for (int i = 0; i < 36; i++) {
                r.covariance[i] = r.sigma2 * inv[i];
                finite = finite && std::isfinite(r.covariance[i]);
            }
            r.covariance_valid = finite ? 1 : 0;
            if (!finite) std::memset(r.covariance, 0, sizeof r.covariance);
        }
    }
    return LOM_OK;
}

// the best of a batch: most valid, then lower cost, then lower index; a report of no queries ranks below any other
extern "C" int lom_quality_batch_best(const lom_quality_report *r, int count)
{
    if (!r || count <= 0) return -1;
    int best = 0;
    for (int i = 1; i < count; i++) {
        const lom_quality_report &a = r[i], &b = r[best];
        const bool a_empty = a.queries == 0, b_empty = b.queries == 0;
        if (a_empty != b_empty) {
            if (b_empty) best = i;
            continue;
        }
        if (a.valid > b.valid || (a.valid == b.valid && a.cost < b.cost)) best = i;
    }
    return best;
}

// nodes -k .. k along one axis: k = floor(half_extent / step), 0 where the step is not positive or the extent below it
static long long lattice_half_nodes(double half_extent, double step)
{
    if (!(step > 0.0) || half_extent < step) return 0;
    return (long long)std::floor(half_extent / step);
}

extern "C" int lom_pose_lattice(const lom_pose *centre, const float half_extent_xyz[3], const float step_xyz[3],
                                float half_extent_yaw_rad, float step_yaw_rad, lom_pose *out, int cap)
{
    if (!centre || !half_extent_xyz || !step_xyz) return LOM_ERR_ARG;
    bool finite = std::isfinite(half_extent_yaw_rad) && std::isfinite(step_yaw_rad);
    for (int a = 0; a < 3; a++)
        finite = finite && std::isfinite(centre->t[a]) && std::isfinite(half_extent_xyz[a]) && std::isfinite(step_xyz[a]);
    for (int a = 0; a < 4; a++) finite = finite && std::isfinite(centre->q[a]);
    if (!finite) return LOM_ERR_ARG;
    const double cw = (double)centre->q[0], cx = (double)centre->q[1], cy = (double)centre->q[2], cz = (double)centre->q[3];
    if (!(cw * cw + cx * cx + cy * cy + cz * cz > 0.0)) return LOM_ERR_ARG;  // nothing to normalise
    long long k[3];
    const long long ky = lattice_half_nodes((double)half_extent_yaw_rad, (double)step_yaw_rad);
    double total = (double)(2 * ky + 1);
    for (int a = 0; a < 3; a++) {
        k[a] = lattice_half_nodes((double)half_extent_xyz[a], (double)step_xyz[a]);
        total *= (double)(2 * k[a] + 1);
    }
    if (!(total <= 2147483647.0) || ky > (1ll << 30) || k[0] > (1ll << 30) || k[1] > (1ll << 30) || k[2] > (1ll << 30))
        return LOM_ERR_ARG;
    const int count = (int)total;
    if (!out || cap < count) return count;
    lom_pose *o = out;
    for (long long jy = -ky; jy <= ky; jy++) {
        // yaw_z(angle) = (cos(angle / 2), 0, 0, sin(angle / 2)), times the centre's quaternion from the left
        const double angle = (double)jy * (double)step_yaw_rad;
        const double w1 = std::cos(0.5 * angle), z1 = std::sin(0.5 * angle);
        double q[4] = {w1 * cw - z1 * cz, w1 * cx - z1 * cy, w1 * cy + z1 * cx, w1 * cz + z1 * cw};
        const double norm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int a = 0; a < 4; a++) q[a] /= norm;
        for (long long ix = -k[0]; ix <= k[0]; ix++)
            for (long long iy = -k[1]; iy <= k[1]; iy++)
                for (long long iz = -k[2]; iz <= k[2]; iz++, o++) {
                    o->t[0] = (float)((double)centre->t[0] + (double)ix * (double)step_xyz[0]);
                    o->t[1] = (float)((double)centre->t[1] + (double)iy * (double)step_xyz[1]);
                    o->t[2] = (float)((double)centre->t[2] + (double)iz * (double)step_xyz[2]);
                    for (int a = 0; a < 4; a++) o->q[a] = (float)q[a];
                }
    }
    return count;
}
