// Neighbourhood classifier of the per-frame front end: planar / not planar and a normal per point of a frame that has
// no rings.  The frame is its own spatial index -- a voxel map with voxel size = radius that
// keeps the first K points of a voxel (the map's ordinary insert), so the 27 voxels around a point's voxel hold every
// stored point within the radius.
//
//   k_nb_eval     one query per 16-lane DPP row, as in k_normals (normals.hip): 27 slot probes, the neighbours as one
//                 flattened candidate sequence, f64 moments per lane, DPP row sums.  What k_normals does next -- one
//                 lane of sixteen solves the 3x3 eigenproblem while fifteen wait, once per wave and query round -- is
//                 done differently: a row handles four queries in turn and parks their ten moments in LDS; then ONE
//                 wave solves the workgroup's 64 matrices, one per lane, with all its lanes busy (a sixteenth of the
//                 Jacobi issue slots).  All three eigenvalues come out; flag + normal go into one 16-byte record per
//                 INPUT point, the detail record on request.
//   k_nb_compact  the flagged points in input order, range filter folded in: mode 0 is ONE kernel with the in-kernel
//                 scan of grid_scan.hpp; modes 1 and 2, with k_nb_offsets between them, are the multi-launch form
//                 that waits for nobody and redoes a frame whose scan gave up.
#pragma once
#include "grid_scan.hpp"
#include "lom_internal.hpp"

namespace lom {

constexpr int kNbRow = 16;                      // lanes per query
constexpr int kNbRows = kThreads / kNbRow;      // queries in flight per workgroup
constexpr int kNbPerRow = 4;                    // queries a row handles before the workgroup solves
constexpr int kNbBatch = kNbRows * kNbPerRow;   // = 64: one matrix per lane of the solving wave
static_assert(kNbBatch == 64, "the solving wave takes one matrix per lane");
constexpr uint32_t kNbMaxBlocks = 1024;         // workgroups of the multi-launch compaction at most (kThreads points each)

struct NbArgs {
    double r2;             // radius^2, f64 product of the f32 radius widened
    double max_variation;  // thresholds: the f32 parameters widened
    double min_spread;
    uint32_t min_neighbours;
};

template <int kCtrl>
__device__ __forceinline__ double nb_dpp_f64(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), kCtrl, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), kCtrl, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double nb_row_sum(double v)  // all 16 lanes of the row end with the total
{
    v += nb_dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
    v += nb_dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
    v += nb_dpp_f64<0x141>(v);  // row_half_mirror
    v += nb_dpp_f64<0x140>(v);  // row_mirror
    return v;
}

// one Jacobi rotation in the (p, q) plane of the symmetric matrix a (upper triangle: 00 01 02 11 12 22 as scalars
// through references), accumulated into the columns p, q of V
__device__ __forceinline__ void nb_rotate(double &app, double &aqq, double &apq, double &akp, double &akq, double &v0p,
                                          double &v0q, double &v1p, double &v1q, double &v2p, double &v2q)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    // A <- G^T A G: the rotated pair is annihilated, the diagonal moves by t * apq, the third row / column mixes
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double kp = akp, kq = akq;
    akp = c * kp - s * kq;
    akq = s * kp + c * kq;
    double a, b;
    a = v0p, b = v0q, v0p = c * a - s * b, v0q = s * a + c * b;
    a = v1p, b = v1q, v1p = c * a - s * b, v1q = s * a + c * b;
    a = v2p, b = v2q, v2p = c * a - s * b, v2q = s * a + c * b;
}

// eigenvalues (ascending) of {a00 a01 a02; . a11 a12; . . a22} and the unit eigenvector of the smallest: cyclic Jacobi
// on scalars (no indexed arrays, hence no scratch)
__device__ inline void nb_eigen(double a00, double a01, double a02, double a11, double a12, double a22, double ev[3],
                                double vec[3])
{
    double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
    for (int sweep = 0; sweep < 12; sweep++) {
        const double off = fabs(a01) + fabs(a02) + fabs(a12);
        const double diag = fabs(a00) + fabs(a11) + fabs(a22);
        if (off <= 1e-18 * diag || off == 0.0) break;
        nb_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1); third index 2: a[2][0], a[2][1]
        nb_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2); third index 1: a[1][0], a[1][2]
        nb_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2); third index 0: a[0][1], a[0][2]
    }
    double e0 = a00, e1 = a11, e2 = a22;
    int i0 = 0, i1 = 1, i2 = 2;
    if (e1 < e0) {
        const double t = e0;
        e0 = e1, e1 = t;
        i0 = 1, i1 = 0;
    }
    if (e2 < e1) {
        const double t = e1;
        e1 = e2, e2 = t;
        const int ti = i1;
        i1 = i2, i2 = ti;
    }
    if (e1 < e0) {
        const double t = e0;
        e0 = e1, e1 = t;
        const int ti = i0;
        i0 = i1, i1 = ti;
    }
    (void)i2;
    ev[0] = e0, ev[1] = e1, ev[2] = e2;
    vec[0] = i0 == 0 ? v00 : (i0 == 1 ? v01 : v02);
    vec[1] = i0 == 0 ? v10 : (i0 == 1 ? v11 : v12);
    vec[2] = i0 == 0 ? v20 : (i0 == 1 ? v21 : v22);
}

// rec[i] = {normal, planar flag in the bits of w}; detail (may be null): lom_neighbourhood_detail per input point.
// idx_range / idx_grid: the index map's status words of the insert in front of this kernel (sequence number idx_seq):
// a point out of range, an in-kernel scan that gave up (idx_grid[1]: a bulk insert sent back) -- they travel on as the
// front end's own words [6] (range) and [5] (redo), so that the host looks at one place.
__global__ __launch_bounds__(kThreads) void k_nb_eval(MapView map, const lom_point_xyzirt *__restrict__ pts, uint32_t n, NbArgs P,
                                                      float4 *__restrict__ rec, lom_neighbourhood_detail *__restrict__ detail,
                                                      const uint32_t *idx_range, const uint32_t *idx_grid, uint32_t idx_seq,
                                                      uint32_t seq, uint32_t *words)
{
    __shared__ uint32_t s_pref[kNbRows][32], s_base[kNbRows][32];
    __shared__ double s_mom[10][kNbBatch];  // [moment][query of the batch]: the solving lane l reads column l
    const int gl = threadIdx.x % kNbRow, grp = threadIdx.x / kNbRow;
    if (blockIdx.x == 0 && threadIdx.x == 0 && idx_range) {
        if (*idx_range == idx_seq) __hip_atomic_store(words + 6, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (idx_grid[0] == idx_seq || idx_grid[1] == idx_seq)
            __hip_atomic_store(words + 5, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (uint32_t base = blockIdx.x * kNbBatch; base < n; base += gridDim.x * kNbBatch) {  // uniform over the workgroup
#pragma unroll 1
        for (int j = 0; j < kNbPerRow; j++) {
            const uint32_t q = base + (uint32_t)(j * kNbRows + grp);
            const bool live = q < n;  // a row past the end runs along with nothing to read (no divergence inside a wave)
            const lom_point_xyzirt *sp = pts + (live ? q : n - 1u);
            const float qx = sp->x, qy = sp->y, qz = sp->z;
            int ix = 0, iy = 0, iz = 0;
            const bool inr = live && voxel_index(qx, map.voxel_size, ix) && voxel_index(qy, map.voxel_size, iy) &&
                             voxel_index(qz, map.voxel_size, iz);
            uint32_t cnt[2] = {0, 0}, slab[2] = {0, 0};
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const int b = gl + s * kNbRow;
                const int nx = ix + b / 9 - 1, ny = iy + (b / 3) % 3 - 1, nz = iz + b % 3 - 1;
                const bool act = inr && b < 27 && nx > -kIdxBias && nx < kIdxBias && ny > -kIdxBias && ny < kIdxBias &&
                                 nz > -kIdxBias && nz < kIdxBias;
                if (act) {
                    const unsigned long long key = pack_key(nx, ny, nz);
                    uint32_t h = hash_key(key, map.shift) & map.mask;
                    for (uint32_t probe = 0; probe <= map.mask; probe++) {
                        const Slot sl = map.table[h];
                        if (sl.key == key) {
                            cnt[s] = sl.count;
                            slab[s] = sl.slab;
                            break;
                        }
                        if (sl.key == kEmptyKey) break;
                        h = (h + 1) & map.mask;
                    }
                }
            }
            // inclusive prefix of the counts in scan order over the row (two sets of 16)
            uint32_t run = 0;
#pragma unroll
            for (int s = 0; s < 2; s++) {
                uint32_t inc = cnt[s];
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) {
                    const uint32_t o = __shfl_up(inc, d, 16);
                    if (gl >= d) inc += o;
                }
                const int b = gl + s * kNbRow;
                s_pref[grp][b] = (b < 27) ? run + inc : 0xFFFFFFFFu;
                s_base[grp][b] = slab[s] * map.K - (run + inc - cnt[s]);
                run += __shfl(inc, 15, 16);
            }
            const uint32_t T = run;  // <= 27 * K
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            double m0 = 0.0, s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
            const uint32_t *pref = s_pref[grp];
            for (uint32_t c = gl; c < T; c += kNbRow) {
                uint32_t b = 0;  // smallest b with pref[b] > c
                b += (pref[b + 15] <= c) ? 16u : 0u;
                b += (pref[b + 7] <= c) ? 8u : 0u;
                b += (pref[b + 3] <= c) ? 4u : 0u;
                b += (pref[b + 1] <= c) ? 2u : 0u;
                b += (pref[b] <= c) ? 1u : 0u;
                const float *vp = map.pts + (size_t)(s_base[grp][b] + c) * 3;
                const double dx = (double)vp[0] - (double)qx, dy = (double)vp[1] - (double)qy, dz = (double)vp[2] - (double)qz;
                const double d2 = dx * dx + dy * dy + dz * dz;
                if (d2 <= P.r2) {
                    m0 += 1.0;
                    s1x += dx, s1y += dy, s1z += dz;
                    sxx += dx * dx, sxy += dx * dy, sxz += dx * dz, syy += dy * dy, syz += dy * dz, szz += dz * dz;
                }
            }
            m0 = nb_row_sum(m0);
            s1x = nb_row_sum(s1x), s1y = nb_row_sum(s1y), s1z = nb_row_sum(s1z);
            sxx = nb_row_sum(sxx), sxy = nb_row_sum(sxy), sxz = nb_row_sum(sxz);
            syy = nb_row_sum(syy), syz = nb_row_sum(syz), szz = nb_row_sum(szz);
            if (gl == 0) {
                const int col = j * kNbRows + grp;
                s_mom[0][col] = m0;
                s_mom[1][col] = s1x, s_mom[2][col] = s1y, s_mom[3][col] = s1z;
                s_mom[4][col] = sxx, s_mom[5][col] = sxy, s_mom[6][col] = sxz;
                s_mom[7][col] = syy, s_mom[8][col] = syz, s_mom[9][col] = szz;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        const uint32_t q = base + threadIdx.x;
        if (threadIdx.x < kNbBatch && q < n) {  // wave 0: one matrix per lane
            const int l = threadIdx.x;
            const double m0 = s_mom[0][l];
            double ev[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
            if (m0 >= 1.0) {
                const double mx = s_mom[1][l] / m0, my = s_mom[2][l] / m0, mz = s_mom[3][l] / m0;
                nb_eigen(s_mom[4][l] / m0 - mx * mx, s_mom[5][l] / m0 - mx * my, s_mom[6][l] / m0 - mx * mz,
                         s_mom[7][l] / m0 - my * my, s_mom[8][l] / m0 - my * mz, s_mom[9][l] / m0 - mz * mz, ev, v);
            }
            const uint32_t m = (uint32_t)m0;
            const double tr = ev[0] + ev[1] + ev[2];
            const bool planar = m >= P.min_neighbours && tr > 0.0 && ev[0] / tr <= P.max_variation && ev[1] / ev[2] >= P.min_spread;
            const lom_point_xyzirt *sp = pts + q;
            // towards the sensor origin: n . p must not be positive
            const double side = -((double)sp->x * v[0] + (double)sp->y * v[1] + (double)sp->z * v[2]);
            const double sgn = side < 0.0 ? -1.0 : 1.0;
            rec[q] = make_float4((float)(sgn * v[0]), (float)(sgn * v[1]), (float)(sgn * v[2]), __uint_as_float(planar ? 1u : 0u));
            if (detail) {
                lom_neighbourhood_detail d;
                d.neighbours = m;
                d.planar = planar ? 1 : 0;
                d.eig[0] = ev[0], d.eig[1] = ev[1], d.eig[2] = ev[2];
                detail[q] = d;
            }
        }
        __syncthreads();  // s_mom is free again
    }
}

// kMode 0: the single-pass form (in-kernel scan; a grid that gave up writes nothing and leaves the call's sequence number
// in words[5]).  kMode 1: workgroup totals into blk[].  kMode 2: write with the offsets k_nb_offsets left in blk[]; it also
// takes the give-up mark of the attempt it redoes out of words[5].
// kItems: consecutive points per thread (1 up to 65536 points, 4 beyond).  apply_range: utils::rangeFilter behind the
// classifier (range_filter.h:18-22, the arithmetic of k_fe_planar); without it the filtered count equals the planar one.
template <int kItems, int kMode>
__global__ __launch_bounds__(kThreads) void k_nb_compact(const lom_point_xyzirt *__restrict__ pts, const float4 *__restrict__ rec,
                                                         uint32_t n, float min_sq, float max_sq, int apply_range,
                                                         float *__restrict__ out_xyz, float *__restrict__ out_nrm, Granule *agg,
                                                         unsigned long long *blk, uint32_t seq, uint32_t *words,
                                                         uint32_t test_fail_from)
{
    __shared__ unsigned long long s_w[8];
    const uint32_t base = (blockIdx.x * kThreads + threadIdx.x) * kItems;
    bool keep[kItems];
    float px[kItems], py[kItems], pz[kItems];
    float4 r[kItems];
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const uint32_t i = base + k;
        keep[k] = false;
        px[k] = py[k] = pz[k] = 0.f;
        r[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i >= n) continue;
        r[k] = rec[i];
        if (__float_as_uint(r[k].w) == 0u) continue;
        mine += 1ull << 32;  // a planar point
        const lom_point_xyzirt p = pts[i];
        const float r2 = p.x * p.x + p.y * p.y + p.z * p.z;
        if (!apply_range || (r2 >= min_sq && r2 <= max_sq)) {
            keep[k] = true;
            mine += 1ull;
            px[k] = p.x, py[k] = p.y, pz[k] = p.z;
        }
    }
    unsigned long long tot;
    const unsigned long long excl = block_scan64(mine, s_w, tot);
    if (kMode == 1) {
        if (threadIdx.x == 0) blk[blockIdx.x] = tot;
        return;
    }
    bool gave_up = false;
    unsigned long long before;
    if (kMode == 0)
        before = grid_prefix64(tot, agg, seq, words + 5, s_w, gave_up, test_fail_from);
    else
        before = blk[blockIdx.x];
    uint32_t at = (uint32_t)(before + excl);  // low word: kept points before this thread
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        if (!keep[k] || gave_up) continue;
        float *o = out_xyz + (size_t)at * 3, *no = out_nrm + (size_t)at * 3;
        o[0] = px[k], o[1] = py[k], o[2] = pz[k];
        no[0] = r[k].x, no[1] = r[k].y, no[2] = r[k].z;
        at++;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        bool hole = false;  // a workgroup in the middle gave up and this one still got its prefix (see k_fe_planar)
        if (kMode == 0) hole = __hip_atomic_load(words + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == seq;
        const unsigned long long all = (gave_up || hole) ? 0ull : before + tot;
        words[0] = (uint32_t)(all >> 32);  // planar points
        words[1] = (uint32_t)all;          // after the range filter
        words[2] = 0u;                     // no organised cloud
        words[3] = 0u;
        if (kMode == 2) words[5] = 0u;
    }
}

// exclusive scan of the nb workgroup totals in place: one workgroup, a chunk of kThreads totals at a time
__global__ __launch_bounds__(kThreads) void k_nb_offsets(unsigned long long *blk, uint32_t nb)
{
    __shared__ unsigned long long s_w[8];
    unsigned long long carry = 0;
    for (uint32_t c = 0; c < nb; c += kThreads) {
        const uint32_t i = c + threadIdx.x;
        const unsigned long long v = i < nb ? blk[i] : 0ull;
        unsigned long long tot;
        const unsigned long long excl = block_scan64(v, s_w, tot);
        if (i < nb) blk[i] = carry + excl;
        carry += tot;
    }
}

}  // namespace lom
