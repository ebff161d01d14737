// The kernels of the per-frame front end; frontend.hip alone launches them.
//
// Four kernels, no host decision in between (sizes the host does not know travel as device words):
//   k_fe_stats     min / max of the stamps, points per ring (uint8 ring id, cloud_classifier.h:23)
//   k_fe_deskew    time normalisation, per-point slerp + weighted translation, ring row + azimuth cell,
//                  "last writer wins" per cell as an atomicMax over input indices (:47-55)
//   k_fe_curv      organised cloud (zero points in empty cells) + 9-tap curvature over the FLATTENED
//                  array (:76-103; the window crosses ring boundaries, as in the reference)
//   k_fe_planar    normals from the previous ring (:105-165), range filter, and the compaction of the
//                  surviving planar points in ray-major order (one in-kernel scan, grid_scan.hpp)
//
// Bit-exactness against the host code of host_stages.cpp (= oracle/pipeline.c): every f32 / f64 operation
// below is the host's, in the host's order (-ffp-contract=off).  The three library calls are handled
// like this: acos / sin of the FRAME's rotation angle are computed once on the host (glibc); the
// per-point sin((1 - t) theta), sin(t theta) use glibc's own sinf algorithm restated below
// (exhaustively equal to libm's on this image for 0 <= x <= pi/2, tools/check_sinf.c); the double
// atan2 of the azimuth comes from the device library; the host's value lies within 2e-14 of it, and a
// point whose azimuth bin is not the same at both ends of that band raises a flag -- the frame is then
// redone by the host stages (a band of 4e-14 rad against bins of 2 pi / W: ~1e-11 per point).
#pragma once
#include <cstdint>
#include <cstring>

#include "grid_scan.hpp"
#include "lom_internal.hpp"
#include "pose_math.hpp"

namespace lom {

constexpr double kPi = 3.14159265358979323846;
constexpr int kFeItems = 4;  // cells per thread of k_fe_planar: up to 4 * 65536 cells per frame

// ---- glibc 2.35 sinf (sysdeps/ieee754/flt-32/s_sinf.c, sincosf.h: ARM optimized-routines) for
// |x| < 120: double-precision polynomial on the reduced argument, result rounded to f32 once ----------
__host__ __device__ inline float glibc_sinf(float y)
{
    const double C0 = 0x1p0, C1 = -0x1.ffffffd0c621cp-2, C2 = 0x1.55553e1068f19p-5, C3 = -0x1.6c087e89a359dp-10,
                 C4 = 0x1.99343027bf8c3p-16;
    const double S1 = -0x1.555545995a603p-3, S2 = 0x1.1107605230bc4p-7, S3 = -0x1.994eb3774cf24p-13;
    const double HPI_INV = 0x1.45F306DC9C883p+23, HPI = 0x1.921FB54442D18p0;
    uint32_t bits;
    memcpy(&bits, &y, 4);
    const uint32_t top = (bits >> 20) & 0x7ffu;
    double x = (double)y;
    if (top < 0x3F4u) {  // abstop12(y) < abstop12(pi/4)
        const double s = x * x;
        if (top < 0x398u) return y;  // |y| < 2^-12
        const double x3 = x * s;
        const double s1 = S2 + s * S3;
        const double x7 = x3 * s;
        const double ss = x + x3 * S1;
        return (float)(ss + x7 * s1);
    }
    // reduce_fast: quadrant in bits 24..31 of x * (2/pi * 2^24)
    const double r = x * HPI_INV;
    const int n = ((int32_t)r + 0x800000) >> 24;
    x = x - (double)n * HPI;
    const double sg = ((n & 3) == 1 || (n & 3) == 2) ? -1.0 : 1.0;  // sign[n & 3] = {1, -1, -1, 1}
    const double neg = (n & 2) ? -1.0 : 1.0;                         // second table: negated coefficients
    const double xs = x * sg, x2 = x * x;
    if ((n & 1) == 0) {
        const double x3 = xs * x2;
        const double s1 = neg * S2 + x2 * (neg * S3);
        const double x7 = x3 * x2;
        const double ss = xs + x3 * (neg * S1);
        return (float)(ss + x7 * s1);
    }
    const double x4 = x2 * x2;
    const double c2 = neg * C3 + x2 * (neg * C4);
    const double c1 = neg * C0 + x2 * (neg * C1);
    const double x6 = x4 * x2;
    const double c = c1 + x4 * (neg * C2);
    return (float)(c + x6 * c2);
}

// what the host prepares per frame: the two poses of transformNonRigid and the frame-level pieces of
// Eigen's Quaternionf::slerp (cloud_transform.h:27)
struct FrameConst {
    float sq[4], eq[4];  // start / end rotation
    float st[3], et[3];  // start / end translation
    float theta, sin_theta;
    int linear;  // |dot| >= 1 - eps: the coefficients are 1 - t and t
    int negate;  // dot < 0: the second coefficient changes sign
    float min_sq, max_sq;  // rangeFilter bounds, squared in f32 (range_filter.h:18-19)
};

// per-frame statistics: two sets, a frame uses set (frame & 1) and clears the other one for its successor
struct FeStats {
    uint32_t ring_count[256];
    uint32_t tmin, tmax;  // order-preserving images of the f32 stamps
    uint32_t pad[6];
};

__device__ __forceinline__ uint32_t f32_ordered(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float f32_unordered(uint32_t u)
{
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// words written for the host / the consumers:  [0] planar points  [1] filtered points  [2] H  [3] W
//   [4] fall-back flag (sequence number of the frame that must be redone on the host)  [5] grid error
//   [6] neighbourhood classifier: a point of the frame is out of range / not finite (sequence number)
constexpr int kFeWords = 8;

// `in` may be the pinned host buffer the frame was staged in (read over the host link, once): the kernel then leaves
// the frame in HBM (`keep`) for the kernels behind it -- the upload and the first pass over the frame are one pass,
// without a copy engine's start-up in front of them.
__global__ __launch_bounds__(kThreads) void k_fe_stats(const lom_point_xyzirt *__restrict__ in, uint32_t n, FeStats *mine,
                                                       FeStats *next, lom_point_xyzirt *__restrict__ keep)
{
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_min[kThreads / 64], s_max[kThreads / 64];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const lom_point_xyzirt p = in[i];
        if (keep) keep[i] = p;
        if (p.time == p.time) {  // the host's `<` / `>` scans skip NaN stamps
            const uint32_t o = f32_ordered(p.time);
            lo = o < lo ? o : lo;
            hi = o > hi ? o : hi;
        }
        atomicAdd(&s_hist[(uint8_t)p.ring], 1u);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t a = __shfl_xor(lo, d, 64), b = __shfl_xor(hi, d, 64);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        s_min[threadIdx.x >> 6] = lo;
        s_max[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (s_hist[threadIdx.x]) atomicAdd(&mine->ring_count[threadIdx.x], s_hist[threadIdx.x]);
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; w++) {
            lo = s_min[w] < lo ? s_min[w] : lo;
            hi = s_max[w] > hi ? s_max[w] : hi;
        }
        atomicMin(&mine->tmin, lo);
        atomicMax(&mine->tmax, hi);
    }
    if (blockIdx.x == 0) {  // the other set goes back to rest for the next frame
        next->ring_count[threadIdx.x] = 0;
        if (threadIdx.x == 0) {
            next->tmin = 0xFFFFFFFFu;
            next->tmax = 0u;
        }
    }
}

// rows of the organised cloud: ring ids in ascending order of the uint8 key (std::map<uint8_t, ...>,
// cloud_classifier.h:23,56-66); W = the largest ring (:33-39).  Every workgroup derives them from the
// 256 counters; thread r holds ring r.
__device__ __forceinline__ void ring_layout(const FeStats *st, uint32_t *s_row, uint32_t *s_tmp, uint32_t &H, uint32_t &W)
{
    const uint32_t cnt = st->ring_count[threadIdx.x];
    const uint32_t has = cnt ? 1u : 0u;
    // inclusive scan of `has` and max of `cnt` over the 256 threads
    uint32_t inc = has, mx = cnt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = __shfl_xor(mx, d, 64);
        mx = o > mx ? o : mx;
    }
    if (lane == 63) s_tmp[wave] = inc;
    if (lane == 0) s_tmp[4 + wave] = mx;
    __syncthreads();
    uint32_t off = 0, tot = 0, w = 0;
    for (int k = 0; k < kThreads / 64; k++) {
        if (k < wave) off += s_tmp[k];
        tot += s_tmp[k];
        w = s_tmp[4 + k] > w ? s_tmp[4 + k] : w;
    }
    s_row[threadIdx.x] = off + inc - has;
    H = tot;
    W = w;
    __syncthreads();
}

__global__ __launch_bounds__(kThreads) void k_fe_deskew(const lom_point_xyzirt *__restrict__ in, uint32_t n, FrameConst F,
                                                        const FeStats *st, lom_point_xyzirt *__restrict__ desk,
                                                        uint32_t *win, uint32_t cell_cap, uint32_t seq, uint32_t *words)
{
    __shared__ uint32_t s_row[256], s_tmp[8];
    uint32_t H, W;
    ring_layout(st, s_row, s_tmp, H, W);
    const unsigned long long total = (unsigned long long)H * W;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        words[2] = H;
        words[3] = W;
        if (total > cell_cap) __hip_atomic_store(words + 4, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const float lo = f32_unordered(st->tmin), hi = f32_unordered(st->tmax);
    const float range = hi - lo;  // point_time_normalize.h:27
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        lom_point_xyzirt p = in[i];
        const float t = (p.time - lo) / range;  // :33
        // Eigen Quaternionf::slerp(t, end) of start (cloud_transform.h:27)
        float s0, s1;
        if (F.linear) {
            s0 = 1.0f - t;
            s1 = t;
        } else {
            s0 = glibc_sinf((1.0f - t) * F.theta) / F.sin_theta;
            s1 = glibc_sinf(t * F.theta) / F.sin_theta;
        }
        if (F.negate) s1 = -s1;
        float q[4], r[3];
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = s0 * F.sq[k] + s1 * F.eq[k];
        const float v[3] = {p.x, p.y, p.z};
        quat_rotate<float>(q, v, r);
        const float w1 = (float)(1.0 - (double)t);  // :30
        // the reference weights start.translation by time and end.translation by (1 - time)
        p.x = (r[0] + F.st[0] * t) + F.et[0] * w1;
        p.y = (r[1] + F.st[1] * t) + F.et[1] * w1;
        p.z = (r[2] + F.st[2] * t) + F.et[2] * w1;
        p.time = t;
        desk[i] = p;
        // cloud_classifier.h:49-50: azimuth = atan2(-y, x) + pi (double) narrowed to f32, then the bin
        const double az_d = atan2((double)-p.y, (double)p.x) + kPi;
        const float az = (float)az_d;
        const double binf = fabs((double)(az * (float)W) / (2.0 * kPi));
        {   // could a last-bits difference between this atan2 and the host's change the cell?  The bin is a
            // monotone function of the azimuth: evaluate it at both ends of the band the host's value lies in
            const float az_lo = (float)(az_d - 2e-14), az_hi = (float)(az_d + 2e-14);
            const double b_lo = fabs((double)(az_lo * (float)W) / (2.0 * kPi)), b_hi = fabs((double)(az_hi * (float)W) / (2.0 * kPi));
            const bool in_lo = b_lo < (double)W, in_hi = b_hi < (double)W;
            if (in_lo != in_hi || (in_lo && (uint32_t)b_lo != (uint32_t)b_hi))
                __hip_atomic_store(words + 4, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (binf < (double)W && total <= cell_cap) {  // :52 approx_point_index < max_row_width
            const uint32_t idx = (uint32_t)binf;
            const uint32_t cell = s_row[(uint8_t)p.ring] * W + idx;
            atomicMax(&win[cell], i + 1u);  // the sequential loop's last writer = the largest input index
        }
    }
}

// organised cloud as {x, y, z, curvature} per cell
__global__ __launch_bounds__(kThreads) void k_fe_curv(const lom_point_xyzirt *__restrict__ desk, const uint32_t *__restrict__ win,
                                                      const uint32_t *__restrict__ words, uint32_t cell_cap,
                                                      float4 *__restrict__ org)
{
    const uint32_t total = words[2] * words[3];
    if ((unsigned long long)words[2] * words[3] > cell_cap) return;
    const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= total) return;
    auto cell_point = [&](uint32_t cc, float &x, float &y, float &z, float &inten) {
        const uint32_t j = win[cc];
        x = y = z = inten = 0.f;  // PointType(): empty cells are zero points (:45)
        if (j) {
            const lom_point_xyzirt p = desk[j - 1u];
            x = p.x, y = p.y, z = p.z, inten = p.intensity;
        }
    };
    float x, y, z, inten;
    cell_point(c, x, y, z, inten);
    const uint32_t cw = 4;
    if (c >= cw && c + cw < total) {  // :79 for (i = w; i < size - w; i++)
        const float range = x * x + y * y + z * z;  // :81 (pow(v, 2) is v * v in the reference build)
        if ((double)range < 0.1) {
            inten = 1000.0f;  // :82-85
        } else {
            float dx = (float)((double)(-x) * 9.0);  // :87-89
            float dy = (float)((double)(-y) * 9.0);
            float dz = (float)((double)(-z) * 9.0);
            for (uint32_t w = c - cw; w <= c + cw; w++) {  // :91-95, the centre included
                float ax, ay, az, ai;
                if (w == c)
                    ax = x, ay = y, az = z;
                else
                    cell_point(w, ax, ay, az, ai);
                dx += ax;
                dy += ay;
                dz += az;
            }
            inten = (float)(sqrt((double)(dx * dx + dy * dy + dz * dz)) / (double)range);  // :97
        }
    }
    org[c] = make_float4(x, y, z, inten);
}

template <int kItems>  // cells per thread: 1 while a frame's cells fit one resident grid of 65536 threads, else kFeItems
__global__ __launch_bounds__(kThreads) void k_fe_planar(const float4 *__restrict__ org, uint32_t *win, uint32_t cell_cap,
                                                        FrameConst F, float *__restrict__ out_xyz,
                                                        float *__restrict__ out_nrm, Granule *agg, uint32_t seq,
                                                        uint32_t *words, uint32_t test_fail_from)
{
    __shared__ unsigned long long s_w[8];
    const uint32_t H = words[2], W = words[3];
    const bool overflow = (unsigned long long)H * W > cell_cap;
    const uint32_t total = overflow ? 0u : H * W;
    const uint32_t base = (blockIdx.x * kThreads + threadIdx.x) * kItems;
    const float flat = 0.05f;
    const double flat10 = (double)flat * 10.0;  // :121 flatness_threshold * 10.0
    bool keep[kItems];
    float px[kItems], py[kItems], pz[kItems], nx[kItems], ny[kItems], nz[kItems];
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const uint32_t c = base + k;
        keep[k] = false;
        px[k] = py[k] = pz[k] = nx[k] = ny[k] = nz[k] = 0.f;
        if (c >= total) continue;
        win[c] = 0u;  // the cell table goes back to rest (k_fe_curv has read it)
        const uint32_t ray = c / W, col = c % W;
        if (ray < 1u || col < 4u || col + 4u >= W) continue;  // :107-108
        const float4 pt = org[c];
        if (!(pt.w < flat)) continue;  // :110
        const float4 *row = org + (size_t)(ray - 1u) * W;
        int found = 0;
        float L0 = 0.f, L1 = 0.f, L2 = 0.f, R0 = 0.f, R1 = 0.f, R2 = 0.f;
        // the eight neighbours of the previous ring, all loaded before any is looked at (a loop that stops at the first
        // hit asks for them one round trip after the other); then the reference's two scans over the loaded values
        float4 nbl[4], nbr[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            nbl[t] = row[col - 4u + (uint32_t)t];  // :116 q = col - 4 .. col - 1
            nbr[t] = row[col + 4u - (uint32_t)t];  // :125 q = col + 4 .. col + 1
        }
        bool hit = false;
#pragma unroll
        for (int t = 0; t < 4; t++) {  // :116-123 first from the left
            if (!hit && (double)nbl[t].w < flat10) {
                L0 = nbl[t].x, L1 = nbl[t].y, L2 = nbl[t].z;
                hit = true;
            }
        }
        found += hit ? 1 : 0;
        hit = false;
#pragma unroll
        for (int t = 0; t < 4; t++) {  // :125-132 first from the right
            if (!hit && (double)nbr[t].w < flat10) {
                R0 = nbr[t].x, R1 = nbr[t].y, R2 = nbr[t].z;
                hit = true;
            }
        }
        found += hit ? 1 : 0;
        if (found != 2) continue;
        const float a0 = L0 - pt.x, a1 = L1 - pt.y, a2 = L2 - pt.z;
        const float b0 = R0 - pt.x, b1 = R1 - pt.y, b2 = R2 - pt.z;
        float c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;  // :136
        const float zz = sum3(c0 * c0, c1 * c1, c2 * c2);
        if (zz > 0.f) {  // Eigen normalized()
            const float s = sqrtf(zz);
            c0 /= s, c1 /= s, c2 /= s;
        }
        mine += 1ull << 32;  // a planar point (:138-148)
        const float r2 = pt.x * pt.x + pt.y * pt.y + pt.z * pt.z;  // range_filter.h:20-22
        if (r2 >= F.min_sq && r2 <= F.max_sq) {
            keep[k] = true;
            mine += 1ull;
            px[k] = pt.x, py[k] = pt.y, pz[k] = pt.z;
            nx[k] = c0, ny[k] = c1, nz[k] = c2;
        }
    }
    unsigned long long tot;
    const unsigned long long excl = block_scan64(mine, s_w, tot);
    bool gave_up;  // no prefix: nothing is written (the cell table is at rest already); the host stages redo the frame
    const unsigned long long before = grid_prefix64(tot, agg, seq, words + 5, s_w, gave_up, test_fail_from);
    uint32_t at = (uint32_t)(before + excl);  // low word: filtered points before this thread
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        if (!keep[k] || gave_up) continue;
        float *o = out_xyz + (size_t)at * 3, *no = out_nrm + (size_t)at * 3;
        o[0] = px[k], o[1] = py[k], o[2] = pz[k];
        no[0] = nx[k], no[1] = ny[k], no[2] = nz[k];
        at++;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        // a grid that gave up hands an empty cloud on -- also when it was a workgroup in the MIDDLE that gave up and this
        // one still got its prefix (the slow predecessor published in between): part of the output was never written
        const bool hole = __hip_atomic_load(words + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == seq;
        const unsigned long long all = (gave_up || hole) ? 0ull : before + tot;
        words[0] = (uint32_t)(all >> 32);  // planar points
        words[1] = (uint32_t)all;          // after the range filter
    }
}

__global__ void k_debug_sinf(float *x, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = glibc_sinf(x[i]);
}

}  // namespace lom
