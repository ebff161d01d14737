// Host restatement of the four front-end stages, ROS-free (see host_stages.hpp), and their C entries.
// In the reference these stay C++ on the host (north_star); they are restated here so the
// streaming configuration (BASELINE.json configs[4]) can run end to end without ROS2/PCL/Eigen.
// Built with -ffp-contract=off; f32 expression shapes follow the reference's.
#include "host_stages.hpp"

#include <cmath>
#include <cstring>

#include "pose_math.hpp"

namespace lom {

namespace {
constexpr double kPi = 3.14159265358979323846;
}

// ---- utils::pointTimeNormalize ---------------------------------------------------
void time_normalize(const lom_point_xyzirt *in, size_t n, lom_point_xyzirt *out, Pool *pool)
{
    // min / max of the stamps (:21, sequential in the reference; exact, so parts may be combined)
    float part_lo[64], part_hi[64];
    for (int p = 0; p < 64; p++) part_lo[p] = 3.402823466e+38f, part_hi[p] = -3.402823466e+38f;
    run_parts(pool, n, [&](size_t b, size_t e, unsigned part) {
        float l = 3.402823466e+38f, h = -3.402823466e+38f;
        for (size_t i = b; i < e; i++) {
            l = in[i].time < l ? in[i].time : l;
            h = in[i].time > h ? in[i].time : h;
        }
        part_lo[part & 63] = l;
        part_hi[part & 63] = h;
    });
    float lo = 3.402823466e+38f, hi = -3.402823466e+38f;
    for (int p = 0; p < 64; p++) {
        lo = part_lo[p] < lo ? part_lo[p] : lo;
        hi = part_hi[p] > hi ? part_hi[p] : hi;
    }
    const float range = hi - lo;  // point_time_normalize.h:27 (0/0 when all stamps are equal, as there)
    run_parts(pool, n, [&](size_t b, size_t e, unsigned) {
        for (size_t i = b; i < e; i++) {
            out[i] = in[i];
            out[i].time = (in[i].time - lo) / range;
        }
    });
}

// ---- Eigen Quaternionf::slerp (used by transformNonRigid) ------------------------------
static void slerp(const float a[4], float t, const float b[4], float out[4])
{
    const float one = 1.0f - 1.1920928955078125e-07f;
    const float d = (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
    const float ad = std::fabs(d);
    float s0, s1;
    if (ad >= one) {
        s0 = 1.0f - t;
        s1 = t;
    } else {
        const float theta = std::acos(ad);
        const float st = std::sin(theta);
        s0 = std::sin((1.0f - t) * theta) / st;
        s1 = std::sin(t * theta) / st;
    }
    if (d < 0.0f) s1 = -s1;
    for (int i = 0; i < 4; i++) out[i] = s0 * a[i] + s1 * b[i];
}

// ---- CloudTransformer::transformNonRigid ---------------------------------------------
void transform_non_rigid(const lom_point_xyzirt *in, size_t n, const lom_pose &start, const lom_pose &end,
                         lom_point_xyzirt *out, Pool *pool)
{
    run_parts(pool, n, [&](size_t pb, size_t pe, unsigned) {
    for (size_t i = pb; i < pe; i++) {
        const float t = in[i].time;
        float q[4], r[3];
        slerp(start.q, t, end.q, q);  // cloud_transform.h:27
        const float p[3] = {in[i].x, in[i].y, in[i].z};
        lom::quat_rotate<float>(q, p, r);
        const float w1 = (float)(1.0 - (double)t);  // :30
        out[i] = in[i];
        // the reference weights start.translation by time and end.translation by (1 - time)
        out[i].x = (r[0] + start.t[0] * t) + end.t[0] * w1;
        out[i].y = (r[1] + start.t[1] * t) + end.t[1] * w1;
        out[i].z = (r[2] + start.t[2] * t) + end.t[2] * w1;
    }
    });
}

// ---- utils::rangeFilter ------------------------------------------------------------
size_t range_filter(const float *xyz, const float *nrm, size_t n, float min_range, float max_range, float *xyz_out,
                    float *nrm_out, Pool *pool)
{
    const float lo = min_range * min_range, hi = max_range * max_range;
    auto keep = [&](size_t i) {
        const float *p = xyz + 3 * i;
        const float r2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
        return r2 >= lo && r2 <= hi;
    };
    // contiguous parts: count, then copy each part to its offset -- the output keeps the input order
    size_t count[65] = {};
    run_parts(pool, n, [&](size_t b, size_t e, unsigned part) {
        size_t c = 0;
        for (size_t i = b; i < e; i++) c += keep(i) ? 1 : 0;
        count[part & 63] = c;
    });
    size_t offset[65];
    offset[0] = 0;
    for (int p = 0; p < 64; p++) offset[p + 1] = offset[p] + count[p];
    run_parts(pool, n, [&](size_t b, size_t e, unsigned part) {
        size_t w = offset[part & 63];
        for (size_t i = b; i < e; i++) {
            if (!keep(i)) continue;
            std::memcpy(xyz_out + 3 * w, xyz + 3 * i, 12);
            if (nrm && nrm_out) std::memcpy(nrm_out + 3 * w, nrm + 3 * i, 12);
            w++;
        }
    });
    return offset[64];
}

// ---- CloudClassifier::classify ---------------------------------------------------------
size_t classify(const lom_point_xyzirt *in, size_t n, float *xyz_out, float *nrm_out, size_t *unclassified,
                size_t grid[2], ClassifyScratch &sc, Pool *pool)
{
    std::vector<lom_point_xyzirt> &cloud = sc.cloud;
    // organise by ring (map key is uint8_t in the reference, :23) and azimuth bin
    size_t ring_count[256] = {};
    {
        std::vector<uint32_t> &hist = sc.hist;
        const unsigned parts = pool ? pool->size() : 1u;
        hist.assign((size_t)parts * 256, 0u);
        run_parts(pool, n, [&](size_t b, size_t e, unsigned part) {
            uint32_t *h = hist.data() + (size_t)part * 256;
            for (size_t i = b; i < e; i++) h[(uint8_t)in[i].ring]++;
        });
        for (unsigned p = 0; p < parts; p++)
            for (int r = 0; r < 256; r++) ring_count[r] += hist[(size_t)p * 256 + r];
    }
    int row_of[256];
    size_t H = 0, W = 0;
    for (int r = 0; r < 256; r++) {
        row_of[r] = -1;
        if (ring_count[r]) {
            row_of[r] = (int)H++;
            W = ring_count[r] > W ? ring_count[r] : W;
        }
    }
    if (grid) grid[0] = H, grid[1] = W;
    if (unclassified) *unclassified = 0;
    const size_t total = H * W;
    if (!total) return 0;
    if (cloud.size() < total) cloud.resize(total);
    run_parts(pool, total, [&](size_t b, size_t e, unsigned) {  // empty cells are zero points (:41-46)
        std::memset(static_cast<void *>(cloud.data() + b), 0, (e - b) * sizeof(lom_point_xyzirt));
    });
    // cell of every point in parallel, then the scatter in input order (last writer wins, :52-54)
    std::vector<uint32_t> &cell = sc.cell;
    if (cell.size() < n) cell.resize(n);
    run_parts(pool, n, [&](size_t pb, size_t pe, unsigned) {
        for (size_t i = pb; i < pe; i++) {
            const lom_point_xyzirt &p = in[i];
            const float azimuth = (float)(std::atan2((double)-p.y, (double)p.x) + kPi);       // :49 (double atan2)
            const size_t idx = (size_t)std::fabs((double)(azimuth * (float)W) / (2.0 * kPi));  // :50
            cell[i] = idx < W ? (uint32_t)((size_t)row_of[(uint8_t)p.ring] * W + idx) : 0xFFFFFFFFu;
        }
    });
    // every part owns a contiguous range of cells and walks the points in input order, so the last
    // writer of a cell is the same as in the sequential loop
    run_parts(pool, total, [&](size_t cb, size_t ce, unsigned) {
        for (size_t i = 0; i < n; i++) {
            const uint32_t c = cell[i];
            if (c >= cb && c < ce) cloud[c] = in[i];
        }
    });
    // curvature over the flattened array (+-4 window crosses ring boundaries), :76-103
    const int cw = 4;
    const float intensity_max = 1000.0f;
    if (total > (size_t)(2 * cw)) {
        // each cell reads its neighbours' coordinates only and writes its own intensity
        run_parts(pool, total - 2 * (size_t)cw, [&](size_t pb, size_t pe, unsigned) {
        for (size_t i = pb + (size_t)cw; i < pe + (size_t)cw; i++) {
            lom_point_xyzirt &o = cloud[i];
            const float range = powf(o.x, 2) + powf(o.y, 2) + powf(o.z, 2);
            if ((double)range < 0.1) {
                o.intensity = intensity_max;
                continue;
            }
            float dx = (float)((double)(-o.x) * (cw * 2.0 + 1.0));
            float dy = (float)((double)(-o.y) * (cw * 2.0 + 1.0));
            float dz = (float)((double)(-o.z) * (cw * 2.0 + 1.0));
            for (int w = -cw; w <= cw; w++) {
                dx += cloud[i + w].x;
                dy += cloud[i + w].y;
                dz += cloud[i + w].z;
            }
            o.intensity = (float)(std::sqrt((double)(dx * dx + dy * dy + dz * dz)) / (double)range);
        }
        });
    }
    // normals from the previous ring, :105-165
    const int nw = 4;
    const float flat = 0.05f;
    const double flat10 = (double)flat * 10.0;
    // rays are independent: each one fills its own slice, slices are concatenated in ray order
    std::vector<float> &tmp_xyz = sc.tmp_xyz, &tmp_nrm = sc.tmp_nrm;
    if (tmp_xyz.size() < total * 3) tmp_xyz.resize(total * 3), tmp_nrm.resize(total * 3);
    std::vector<size_t> &cnt_p = sc.cnt_p, &cnt_u = sc.cnt_u;
    cnt_p.assign(H, 0);
    cnt_u.assign(H, 0);
    run_parts(pool, H - 1, [&](size_t rb, size_t re, unsigned) {
    for (size_t ray = rb + 1; ray < re + 1; ray++) {
        size_t np = 0, nu = 0;
        float *oxyz = tmp_xyz.data() + ray * W * 3, *onrm = tmp_nrm.data() + ray * W * 3;
        for (long pi = nw; pi < (long)W - nw; pi++) {
            const lom_point_xyzirt &pt = cloud[ray * W + (size_t)pi];
            if (pt.intensity < flat) {
                const lom_point_xyzirt *row = &cloud[(ray - 1) * W];
                int found = 0;
                float L[3] = {0, 0, 0}, R[3] = {0, 0, 0};
                for (long q = pi - nw; q < pi; q++)
                    if ((double)row[q].intensity < flat10) {
                        L[0] = row[q].x, L[1] = row[q].y, L[2] = row[q].z;
                        found++;
                        break;
                    }
                for (long q = pi + nw; q > pi; q--)
                    if ((double)row[q].intensity < flat10) {
                        R[0] = row[q].x, R[1] = row[q].y, R[2] = row[q].z;
                        found++;
                        break;
                    }
                if (found == 2) {
                    const float a[3] = {L[0] - pt.x, L[1] - pt.y, L[2] - pt.z};
                    const float b[3] = {R[0] - pt.x, R[1] - pt.y, R[2] - pt.z};
                    float c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
                    const float z = lom::sum3(c[0] * c[0], c[1] * c[1], c[2] * c[2]);
                    if (z > 0.f) {
                        const float s = std::sqrt(z);
                        c[0] /= s, c[1] /= s, c[2] /= s;
                    }
                    oxyz[3 * np] = pt.x, oxyz[3 * np + 1] = pt.y, oxyz[3 * np + 2] = pt.z;
                    onrm[3 * np] = c[0], onrm[3 * np + 1] = c[1], onrm[3 * np + 2] = c[2];
                    np++;
                } else {
                    nu++;
                }
            } else if (pt.intensity < intensity_max) {
                nu++;
            }
        }
        cnt_p[ray] = np;
        cnt_u[ray] = nu;
    }
    }, 2);
    size_t np = 0, nu = 0;
    std::vector<size_t> &off_p = sc.off_p;
    off_p.assign(H + 1, 0);
    for (size_t ray = 1; ray < H; ray++) {
        off_p[ray] = np;
        np += cnt_p[ray];
        nu += cnt_u[ray];
    }
    run_parts(pool, H - 1, [&](size_t rb, size_t re, unsigned) {
        for (size_t ray = rb + 1; ray < re + 1; ray++) {
            std::memcpy(xyz_out + 3 * off_p[ray], tmp_xyz.data() + ray * W * 3, cnt_p[ray] * 12);
            std::memcpy(nrm_out + 3 * off_p[ray], tmp_nrm.data() + ray * W * 3, cnt_p[ray] * 12);
        }
    }, 2);
    if (unclassified) *unclassified = nu;
    return np;
}

// Eigen eulerAngles(0,1,2) of (qa * qb^-1).toRotationMatrix(), degrees (lidar_odometry.cpp:54-55)
void delta_euler_deg(const float qa[4], const float qb[4], float out[3])
{
    lom_pose a{}, b{}, inv, prod;
    std::memcpy(a.q, qa, 16);
    std::memcpy(b.q, qb, 16);
    lom::pose_inverse(b, inv);
    lom::pose_compose(a, inv, prod);
    float m[9];
    lom::rotation_matrix(prod.q, m);
    auto M = [&m](int r, int c) { return m[r * 3 + c]; };
    float res[3];
    res[0] = std::atan2(M(1, 2), M(2, 2));
    const float c2 = std::sqrt(M(0, 0) * M(0, 0) + M(0, 1) * M(0, 1));
    if (res[0] > 0.f) {
        res[0] -= (float)kPi;
        res[1] = std::atan2(-M(0, 2), -c2);
    } else {
        res[1] = std::atan2(-M(0, 2), c2);
    }
    const float s1 = std::sin(res[0]), c1 = std::cos(res[0]);
    res[2] = std::atan2(s1 * M(2, 0) - c1 * M(1, 0), c1 * M(1, 1) - s1 * M(2, 1));
    for (int i = 0; i < 3; i++) out[i] = ((-res[i]) * 180.0f) / (float)kPi;
}

}  // namespace lom

using namespace lom;

extern "C" {

void lom_point_time_normalize(const lom_point_xyzirt *in, size_t n, lom_point_xyzirt *out) { time_normalize(in, n, out); }

void lom_transform_non_rigid(const lom_point_xyzirt *in, size_t n, const lom_pose *start, const lom_pose *end,
                             lom_point_xyzirt *out)
{
    transform_non_rigid(in, n, *start, *end, out);
}

size_t lom_range_filter(const float *xyz, const float *nrm, size_t n, float min_range, float max_range, float *xyz_out,
                        float *nrm_out)
{
    return range_filter(xyz, nrm, n, min_range, max_range, xyz_out, nrm_out);
}

size_t lom_cloud_classify(const lom_point_xyzirt *in, size_t n, float *xyz_out, float *nrm_out,
                          size_t *unclassified_out, size_t grid_out[2])
{
    ClassifyScratch scratch;
    return classify(in, n, xyz_out, nrm_out, unclassified_out, grid_out, scratch);
}

}  // extern "C"
