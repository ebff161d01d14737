// The per-point arithmetic of csrc/k_eval.hpp as a program of its own (tests/test_point_terms_cpp.py), compiled for the
// host: point_terms (closed-form rotation columns) and huber_terms (no square root, no divide, no branch) against the
// forms they replace, point_terms_ambient and huber_terms_sqrt, each measured against a long double evaluation of the
// reference's formulas (PointToPlaneErrorAnalytic::Evaluate, Ceres' QuaternionManifold plus-Jacobian, ceres::HuberLoss).
// The bar: on the same seeded inputs the new form's worst error, relative to the entry's scale, is at most twice the
// old form's.  No HIP call is made.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>

#include "check.hpp"
#include "k_eval.hpp"

using namespace lom;
typedef long double ld;

// residual and the three rotation columns of the tangent Jacobian in long double, as the reference writes them:
// Eigen's quaternion * vector for the residual, the four dR/dq_k matrices, then Ceres' 4x3 plus-Jacobian
static void reference_terms(const float p_[3], const float o_[3], const float n_[3], const double q_[4],
                            const double t_[3], ld J[3], ld &r)
{
    const ld p[3] = {p_[0], p_[1], p_[2]}, o[3] = {o_[0], o_[1], o_[2]}, n[3] = {n_[0], n_[1], n_[2]};
    const ld q0 = q_[0], q1 = q_[1], q2 = q_[2], q3 = q_[3];
    const ld uv[3] = {2 * (q2 * p[2] - q3 * p[1]), 2 * (q3 * p[0] - q1 * p[2]), 2 * (q1 * p[1] - q2 * p[0])};
    const ld rp[3] = {p[0] + q0 * uv[0] + (q2 * uv[2] - q3 * uv[1]), p[1] + q0 * uv[1] + (q3 * uv[0] - q1 * uv[2]),
                      p[2] + q0 * uv[2] + (q1 * uv[1] - q2 * uv[0])};
    r = 0;
    for (int a = 0; a < 3; a++) r += (rp[a] + (ld)t_[a] - o[a]) * n[a];
    const ld M[4][3][3] = {{{q0, -q3, q2}, {q3, q0, -q1}, {-q2, q1, q0}},
                           {{q1, q2, q3}, {q2, -q1, -q0}, {q3, q0, -q1}},
                           {{-q2, q1, q0}, {q1, q2, q3}, {-q0, q3, -q2}},
                           {{-q3, -q0, q1}, {q0, -q3, q2}, {q1, q2, q3}}};
    ld ja[4];
    for (int k = 0; k < 4; k++) {
        ja[k] = 0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) ja[k] += 2 * M[k][i][j] * p[j] * n[i];
    }
    J[0] = ja[0] * -q1 + ja[1] * q0 + ja[2] * -q3 + ja[3] * q2;
    J[1] = ja[0] * -q2 + ja[1] * q3 + ja[2] * q0 + ja[3] * -q1;
    J[2] = ja[0] * -q3 + ja[1] * -q2 + ja[2] * q1 + ja[3] * q0;
}

// ceres::HuberLoss(a = 0.15) on s = r^2: rho and rho'
static void reference_huber(double r, ld &rho, ld &w)
{
    const ld a = 0.15, b = a * a, s = (ld)r * (ld)r;  // (ceres holds a and b = a * a as doubles; 0.15 * 0.15 widened below)
    if (s > (ld)(0.15 * 0.15)) {
        const ld rr = sqrtl(s);
        rho = 2 * a * rr - b;
        w = a / rr;
        if (w < (ld)DBL_MIN) w = DBL_MIN;
    } else {
        rho = s;
        w = 1;
    }
}

struct Worst {
    double old_form = 0.0, new_form = 0.0;
    void add(ld got_old, ld got_new, ld ref, ld scale)
    {
        old_form = std::fmax(old_form, (double)(fabsl(got_old - ref) / scale));
        new_form = std::fmax(new_form, (double)(fabsl(got_new - ref) / scale));
    }
};

static void unit3(std::mt19937_64 &rng, double v[3])
{
    std::normal_distribution<double> g;
    double n2 = 0.0;
    do {
        for (int a = 0; a < 3; a++) v[a] = g(rng);
        n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    } while (n2 < 1e-6);
    for (int a = 0; a < 3; a++) v[a] /= std::sqrt(n2);
}

// the quaternion classes: |q|^2 - 1 of 0 (unit to f64 rounding), of an f32 cast (about +-6e-8), of +-1e-3
static const char *const kQuatClass[] = {"unit", "f32 cast", "+1e-3", "-1e-3"};

static void test_point_terms(int cases)
{
    std::mt19937_64 rng(20240611);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    Worst jac[4], all;
    double worst_uncorrected[4] = {0, 0, 0, 0}, worst_excess[4] = {0, 0, 0, 0}, least_excess_f32 = 1.0;
    for (int c = 0; c < cases; c++) {
        const int cls = c % 4;
        double ax[3], dir[3], nrm[3];
        unit3(rng, ax);
        unit3(rng, dir);
        unit3(rng, nrm);
        // rotations small (an align's) and large
        const double ang = (c % 8 < 4 ? 0.05 : 3.1) * (2.0 * U(rng) - 1.0);
        double q[4] = {std::cos(0.5 * ang), std::sin(0.5 * ang) * ax[0], std::sin(0.5 * ang) * ax[1], std::sin(0.5 * ang) * ax[2]};
        if (cls == 1)
            for (int a = 0; a < 4; a++) q[a] = (double)(float)q[a];
        if (cls >= 2)
            for (int a = 0; a < 4; a++) q[a] *= std::sqrt(cls == 2 ? 1.0 + 1e-3 : 1.0 - 1e-3);
        const double len = c % 16 == 15 ? 100.0 : 100.0 * U(rng);  // |p| up to 100 m
        const double t[3] = {2.0 * U(rng) - 1.0, 2.0 * U(rng) - 1.0, 2.0 * U(rng) - 1.0};
        float p[3], n[3], o[3];
        for (int a = 0; a < 3; a++) {
            p[a] = (float)(len * dir[a]);
            n[a] = (float)nrm[a];
        }
        // the plane origin puts the residual at 0, on either side of the knee, or up to 0.3 (to f32 rounding of o)
        const double targets[6] = {0.0, 0.1499, 0.1501, -0.1501, 0.3 * U(rng), -0.3 * U(rng)};
        const double want_r = targets[(c / 4) % 6];
        {
            const float zero[3] = {0.f, 0.f, 0.f};
            ld J0[3], r0;
            reference_terms(p, zero, n, q, t, J0, r0);  // r0 = (R p + t) . n
            const double back = (double)r0 - want_r;    // o = back * n gives the residual r0 - back |n|^2
            for (int a = 0; a < 3; a++) o[a] = (float)(back * nrm[a]);
        }
        const float4 ra = make_float4(p[0], p[1], p[2], n[0]), rb = make_float4(o[0], o[1], o[2], 1.f),
                     rc = make_float4(n[1], n[2], 0.f, 0.f);
        const double qe = quat_excess(q[0], q[1], q[2], q[3]);
        PointTerms Told, Tnew, Tunc;
        point_terms_ambient(ra, rb, rc, q[0], q[1], q[2], q[3], t[0], t[1], t[2], Told);
        point_terms(ra, rb, rc, q[0], q[1], q[2], q[3], qe, t[0], t[1], t[2], Tnew);
        point_terms(ra, rb, rc, q[0], q[1], q[2], q[3], 0.0, t[0], t[1], t[2], Tunc);  // without the |q|^2 - 1 term
        ld J[3], r;
        reference_terms(p, o, n, q, t, J, r);
        // the scale of a rotation column's entry: 2 |H(q) p| |n|
        const double plen = std::sqrt((double)p[0] * p[0] + (double)p[1] * p[1] + (double)p[2] * p[2]);
        const double nlen = std::sqrt((double)n[0] * n[0] + (double)n[1] * n[1] + (double)n[2] * n[2]);
        const ld scale = 2.0 * (1.0 + qe) * plen * nlen + DBL_MIN;
        for (int a = 0; a < 3; a++) {
            jac[cls].add(Told.J[a], Tnew.J[a], J[a], scale);
            all.add(Told.J[a], Tnew.J[a], J[a], scale);
            worst_uncorrected[cls] = std::fmax(worst_uncorrected[cls], (double)(fabsl((ld)Tunc.J[a] - J[a]) / scale));
            CHECK(Tnew.J[3 + a] == (double)n[a] && Told.J[3 + a] == (double)n[a]);
        }
        CHECK(Tnew.r == Told.r);  // the residual is the same code
        CHECK(fabsl((ld)Tnew.r - r) <= 64 * DBL_EPSILON * (plen + 2.0));
        CHECK(std::fabs(Tnew.r - want_r) < 1e-4);  // the placement worked (o is f32 at up to 100 m: a few 1e-6)
        worst_excess[cls] = std::fmax(worst_excess[cls], std::fabs(qe));
        if (cls == 1) least_excess_f32 = std::fmin(least_excess_f32, std::fabs(qe));
    }
    for (int cls = 0; cls < 4; cls++)
        std::printf("rotation columns, |q|^2 - 1 %-8s (up to %.1e): worst error / scale  old %.3e  new %.3e  "
                    "(new without the |q|^2 - 1 term %.3e)\n",
                    kQuatClass[cls], worst_excess[cls], jac[cls].old_form, jac[cls].new_form, worst_uncorrected[cls]);
    std::printf("point_terms rotation columns: worst error / scale  old %.3e  new %.3e\n", all.old_form, all.new_form);
    CHECK(all.new_form <= 2.0 * all.old_form);
    for (int cls = 0; cls < 4; cls++) CHECK(jac[cls].new_form <= 2.0 * jac[cls].old_form);
    CHECK(all.old_form < 1e-14);  // (the yardstick itself is sound)
    // the inputs do exercise the correction: without it the f32-cast and +-1e-3 classes miss by orders of magnitude
    CHECK(worst_excess[0] < 1e-15 && worst_excess[1] > 1e-8 && worst_excess[1] < 3e-7);
    CHECK(worst_uncorrected[1] > 100.0 * jac[1].new_form && worst_uncorrected[2] > 1e-4 && worst_uncorrected[3] > 1e-4);
    (void)least_excess_f32;
}

static void test_huber(int cases)
{
    std::mt19937_64 rng(77);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    Worst rho, w;
    auto one = [&](double r) {
        const HuberTerms Ho = huber_terms_sqrt(r), Hn = huber_terms(r);
        ld rr, ww;
        reference_huber(r, rr, ww);
        // rho's scale: its own value, and never less than the knee's b = 0.15^2 (rho is continuous there)
        rho.add(Ho.rho, Hn.rho, rr, fmaxl(rr, (ld)(0.15 * 0.15)));
        w.add(Ho.w, Hn.w, ww, ww);
        return Hn;
    };
    // the special points behave as before: r = 0 and |r| = 0.15 exactly take the quadratic side (strict >)
    for (double r : {0.0, -0.0, 0.15, -0.15, DBL_MIN, -DBL_MIN, 4.9e-324}) {
        const HuberTerms Ho = huber_terms_sqrt(r), Hn = one(r);
        CHECK(Hn.w == 1.0 && Hn.rho == r * r);
        CHECK(Hn.w == Ho.w && Hn.rho == Ho.rho);
    }
    // just either side of the knee, ulp by ulp
    double up = 0.15, down = 0.15;
    for (int i = 0; i < 64; i++) {
        up = std::nextafter(up, 1.0);
        down = std::nextafter(down, 0.0);
        for (double r : {up, -up}) {
            const HuberTerms Hn = one(r);
            CHECK(Hn.w < 1.0 + 2 * DBL_EPSILON && Hn.w > 1.0 - 200 * DBL_EPSILON);
        }
        for (double r : {down, -down}) {
            const HuberTerms Hn = one(r);
            CHECK(Hn.w == 1.0 && Hn.rho == r * r);
        }
    }
    for (int c = 0; c < cases; c++) {
        const int kind = c % 4;
        double r = kind == 0 ? 0.3 * U(rng) : kind == 1 ? 0.15 + 1e-3 * (2.0 * U(rng) - 1.0) : kind == 2 ? 0.15 * U(rng) : 0.15 + 0.15 * U(rng);
        if (c & 4) r = -r;
        one(r);
    }
    // far outliers and the floor of the weight (a residual no scan produces; the selects must still hold)
    for (double r : {1.0, 50.0, 1e6, 1e150, 1e300, DBL_MAX}) {
        const HuberTerms Ho = huber_terms_sqrt(r), Hn = huber_terms(r);
        CHECK(Hn.w >= DBL_MIN && Hn.w <= 1.0);
        if (r <= 1e150) one(r);  // (beyond, r * r overflows in the old form: rho = inf, w = DBL_MIN)
        else CHECK(Ho.w == DBL_MIN);
    }
    std::printf("huber rho: worst error / scale  old %.3e  new %.3e\n", rho.old_form, rho.new_form);
    std::printf("huber weight: worst relative error  old %.3e  new %.3e\n", w.old_form, w.new_form);
    CHECK(rho.new_form <= 2.0 * rho.old_form);
    CHECK(w.new_form <= 2.0 * w.old_form);
    CHECK(w.old_form < 4 * DBL_EPSILON && rho.old_form < 4 * DBL_EPSILON);
}

// the 28 sums of a few points through both forms: the sums the solve sees, entry by entry at the scale the parity tests
// use (sqrt(A_aa A_bb) for A, sqrt(A_aa 2 cost) for g)
static void test_sums()
{
    std::mt19937_64 rng(5);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    double acc_new[28] = {0}, acc_old[28] = {0};
    const double q[4] = {(double)0.99993f, (double)0.0031f, (double)-0.0042f, (double)0.0105f}, t[3] = {0.05, 0.03, -0.02};
    const double qe = quat_excess(q[0], q[1], q[2], q[3]);
    for (int i = 0; i < 500; i++) {
        double nrm[3];
        unit3(rng, nrm);
        const float4 ra = make_float4((float)(40 * U(rng)), (float)(40 * U(rng)), (float)(3 * U(rng)), (float)nrm[0]);
        const float4 rc = make_float4((float)nrm[1], (float)nrm[2], 0.f, 0.f);
        const float4 rb = make_float4(ra.x + (float)(0.2 * U(rng)), ra.y + (float)(0.2 * U(rng)), ra.z + (float)(0.2 * U(rng)), 1.f);
        PointTerms Tn, To;
        point_terms(ra, rb, rc, q[0], q[1], q[2], q[3], qe, t[0], t[1], t[2], Tn);
        point_terms_ambient(ra, rb, rc, q[0], q[1], q[2], q[3], t[0], t[1], t[2], To);
        point_accumulate(Tn, acc_new);
        // the old accumulation, spelled out
        const HuberTerms H = huber_terms_sqrt(To.r);
        int k = 0;
        for (int a = 0; a < 6; a++)
            for (int b = a; b < 6; b++) acc_old[k++] += H.w * To.J[a] * To.J[b];
        for (int a = 0; a < 6; a++) acc_old[21 + a] += H.w * To.J[a] * To.r;
        acc_old[27] += 0.5 * H.rho;
    }
    auto diag = [&](int a) { return acc_old[a * 6 - (a * (a - 1)) / 2]; };
    int k = 0;
    double worst = 0.0;
    for (int a = 0; a < 6; a++)
        for (int b = a; b < 6; b++, k++)
            worst = std::fmax(worst, std::fabs(acc_new[k] - acc_old[k]) / std::sqrt(diag(a) * diag(b)));
    for (int a = 0; a < 6; a++)
        worst = std::fmax(worst, std::fabs(acc_new[21 + a] - acc_old[21 + a]) / (std::sqrt(diag(a) * 2.0 * acc_old[27]) + std::fabs(acc_old[21 + a])));
    worst = std::fmax(worst, std::fabs(acc_new[27] - acc_old[27]) / acc_old[27]);
    std::printf("28 sums of 500 points, new against old: worst difference / scale %.3e\n", worst);
    CHECK(acc_old[27] > 0.0 && worst < 1e-13);
}

int main()
{
    test_point_terms(4800);
    test_huber(4000);
    test_sums();
    return check_done();
}
