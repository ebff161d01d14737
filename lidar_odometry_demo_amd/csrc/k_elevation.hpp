// Elevation grid (include/lidar_odometry_amd.h, "elevation grid"): k_elev_clear, k_elev_accumulate, k_elev_unpack and
// k_elev_derive.  Device code only; elevation.hip is the one translation unit that instantiates and launches it.  The
// scan descriptor and its constant-address-space read are the assembly's (k_asm_scan.hpp), the transform is the one every
// posed-scan kernel uses (k_posed_point.hpp).  The hit rule is k_occ_walk's, restated here: shared as one device function
// it changed the code of both kernels (see k_posed_point.hpp), and device code stays as it is.
//
// A cell is one aligned record of 32 bytes -- sum, count, zmin, zmax -- so its four accumulators share a sector.  All
// accumulation is integer atomics: 64-bit add, 32-bit add, signed min and max; the result does not depend on any order.
// No workgroup waits for another; no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "k_asm_scan.hpp"
#include "k_posed_point.hpp"

namespace lom {

constexpr uint32_t kElevThreads = 256;  // k_elev_clear, k_elev_unpack: a thread per cell
constexpr uint32_t kElevTileX = 32, kElevTileY = 8;  // k_elev_derive: a thread per cell of a tile
constexpr uint32_t kElevMaxR = 4;                    // the window's R at most: the tile's halo
constexpr int32_t kElevInvalid = 0x7FFFFFFF;         // in the staged tile: not a valid cell (a zmin is at most 2^19)

struct __attribute__((aligned(32))) ElevCell {
    long long sum;          // of zq
    uint32_t count;
    int32_t zmin, zmax;     // INT32_MAX / INT32_MIN while count == 0
    uint32_t pad[3];
};
static_assert(sizeof(ElevCell) == 32, "one sector per cell");

// the status words of an integrate (zeroed per call): three u64 counters, 8-byte aligned for their atomics
enum {
    EW_MARKED = 0,   // u64 (two words): points that contributed
    EW_HEIGHT = 2,   // u64: hits out of the height range
    EW_NEW = 4,      // u64: cells whose count left 0
    EW_COUNT = 6
};
// of a cost: cells unknown / lethal / costed (u32: a grid has at most 2^26 cells)
enum { EC_UNKNOWN = 0, EC_LETHAL = 1, EC_COSTED = 2, EC_COUNT = 4 };

struct ElevArgs {
    float resolution, origin_x, origin_y, z_ref;
    uint32_t width, height;
    float z_lo, z_hi, min_range, max_range;
    uint32_t stride;  // floats per input record (3: an archive)
    uint32_t merge;   // LOM_ELEV_OPT_TEST_WAVE_MERGE
};

struct ElevDeriveArgs {
    float resolution, z_ref;
    uint32_t width, height, min_points;
    int R;
    float *min_out, *max_out, *mean_out, *slope_out, *rough_out, *step_out;  // each may be NULL
    int8_t *cost_out;                                                        // NULL: no cost, no totals
    float max_slope, max_step, max_rough, max_span;
};

__global__ __launch_bounds__(kElevThreads) void k_elev_clear(ElevCell *cells, uint32_t n_cells)
{
    const uint32_t c = blockIdx.x * kElevThreads + threadIdx.x;
    if (c >= n_cells) return;
    ElevCell e;
    e.sum = 0, e.count = 0u, e.zmin = 0x7FFFFFFF, e.zmax = (int32_t)0x80000000;
    e.pad[0] = e.pad[1] = e.pad[2] = 0u;
    cells[c] = e;
}

// a cell's four updates; true: its count left 0
__device__ __forceinline__ bool elev_update(ElevCell *c, uint32_t cnt, int32_t lo, int32_t hi, long long sum)
{
    const uint32_t before = atomicAdd(&c->count, cnt);
    atomicMin(&c->zmin, lo);
    atomicMax(&c->zmax, hi);
    atomicAdd(reinterpret_cast<unsigned long long *>(&c->sum), (unsigned long long)sum);  // two's complement: a signed sum
    return before == 0u;
}

// A lane per point of its scan (blockIdx.y), all scans of a call in one launch.  The point (12 bytes of a record) is
// transformed by posed_point and never stored.  Consecutive points of a ring land
// in the same cell, so the lanes of a wave that share a cell are merged before anything goes to memory: the first
// contributing lane's cell is broadcast, its sharers are reduced across the wave (a lone lane skips the reduction) and
// retire, until none is left -- one count add, one min, one max and one 64-bit add per distinct cell per wave.
__global__ __launch_bounds__(kAsmThreads) void k_elev_accumulate(const AsmScan *scans, const float *__restrict__ xyz, ElevArgs a,
                                                                 ElevCell *cells, uint32_t *words)
{
    const ConstAsm d = (ConstAsm)(scans + blockIdx.y);
    const uint32_t n = d->n, first = blockIdx.x * kAsmThreads;
    if (first >= n) return;  // a surplus workgroup (uniform)
    const uint32_t i = first + threadIdx.x;
    bool marked = false, out_of_height = false;
    uint32_t cell = 0u;
    int32_t zq = 0;
    if (i < n) {
        const size_t s = ((size_t)d->src + i) * a.stride;
        float px, py, pz;
        posed_point(d, xyz + s, px, py, pz);
        const double r = (double)a.resolution, Gx = (double)a.origin_x, Gy = (double)a.origin_y;
        const double Ox = (double)(float)d->t[0], Oy = (double)(float)d->t[1], Oz = (double)(float)d->t[2];
        const double Dx = (double)px - Ox, Dy = (double)py - Oy, Dz = (double)pz - Oz;
        const double L = __dsqrt_rn(Dx * Dx + (Dy * Dy + Dz * Dz));
        // the endpoint's cell by the floor rule, compared in f64 before any conversion
        const double hx = __builtin_floor(((double)px - Gx) / r), hy = __builtin_floor(((double)py - Gy) / r);
        const bool hit = L >= (double)a.min_range && L <= (double)a.max_range && (double)a.z_lo <= Dz && Dz <= (double)a.z_hi &&
                         hx >= 0.0 && hx < (double)a.width && hy >= 0.0 && hy < (double)a.height;
        if (hit) {
            const double h = (double)pz - (double)a.z_ref;
            if (__builtin_fabs(h) < 2048.0) {
                marked = true;
                zq = (int32_t)__builtin_rint(h * 256.0);  // ties to even; |zq| <= 2^19
                cell = (uint32_t)hy * a.width + (uint32_t)hx;
            } else {
                out_of_height = true;
            }
        }
    }
    bool is_new = false;
    if (a.merge) {
        unsigned long long todo = __ballot(marked);
        const uint32_t lane = threadIdx.x & 63u;
        while (todo) {  // (wave-uniform: every lane runs the shuffles below)
            const int lead = __builtin_ctzll(todo);
            const uint32_t key = (uint32_t)__shfl((int)cell, lead);
            const bool mine = marked && ((todo >> lane) & 1ull) && cell == key;
            const unsigned long long group = __ballot(mine);
            int32_t lo = zq, hi = zq;
            long long sum = zq;
            if (group != (1ull << lead)) {  // more than the leader: reduce, the others contribute neutral values
                lo = mine ? zq : 0x7FFFFFFF, hi = mine ? zq : (int32_t)0x80000000, sum = mine ? (long long)zq : 0ll;
                for (int off = 32; off > 0; off >>= 1) {
                    const int32_t l2 = __shfl_xor(lo, off), h2 = __shfl_xor(hi, off);
                    const long long s2 = __shfl_xor(sum, off);
                    lo = l2 < lo ? l2 : lo, hi = h2 > hi ? h2 : hi, sum += s2;
                }
            }
            if (lane == (uint32_t)lead) is_new = elev_update(cells + key, (uint32_t)__popcll(group), lo, hi, sum);
            todo &= ~group;
        }
    } else if (marked) {
        is_new = elev_update(cells + cell, 1u, zq, zq, (long long)zq);
    }
    // the totals: summed over the wave first, one 64-bit atomic each per wave (integer sums: no order in the result)
    const unsigned long long marked_wave = (unsigned long long)__popcll(__ballot(marked));
    const unsigned long long height_wave = (unsigned long long)__popcll(__ballot(out_of_height));
    const unsigned long long new_wave = (unsigned long long)__popcll(__ballot(is_new));
    if ((threadIdx.x & 63u) == 0u) {
        if (marked_wave) atomicAdd(reinterpret_cast<unsigned long long *>(words + EW_MARKED), marked_wave);
        if (height_wave) atomicAdd(reinterpret_cast<unsigned long long *>(words + EW_HEIGHT), height_wave);
        if (new_wave) atomicAdd(reinterpret_cast<unsigned long long *>(words + EW_NEW), new_wave);
    }
}

// cells [first, first + n) of the records into four arrays of their own, for lom_elevation_cells
__global__ __launch_bounds__(kElevThreads) void k_elev_unpack(const ElevCell *__restrict__ cells, uint32_t first, uint32_t n,
                                                              uint32_t *count, int32_t *zmin, int32_t *zmax, long long *sum)
{
    const uint32_t c = blockIdx.x * kElevThreads + threadIdx.x;
    if (c >= n) return;
    const ElevCell e = cells[first + c];
    count[c] = e.count, zmin[c] = e.zmin, zmax[c] = e.zmax, sum[c] = e.sum;
}

// The derived layers and the cost, a thread per cell of a 32 x 8 tile.  The tile and a halo of R cells are staged in LDS
// as one word per cell: its zmin, or kElevInvalid where the cell is outside the grid or has fewer than min_points.  The
// nine sums of the fit are int64 in registers, Cramer's rule is int64, and the f64 solve, the residuals and the cost run
// in the lane (the header's steps 1 to 6, in its order of operations).
__global__ __launch_bounds__(kElevTileX *kElevTileY) void k_elev_derive(const ElevCell *__restrict__ cells, ElevDeriveArgs a,
                                                                        uint32_t *totals)
{
    constexpr int kPitchMax = (int)(kElevTileX + 2 * kElevMaxR), kRowsMax = (int)(kElevTileY + 2 * kElevMaxR);
    __shared__ int32_t tile[kPitchMax * kRowsMax];
    const int R = a.R, pitch = (int)kElevTileX + 2 * R, rows = (int)kElevTileY + 2 * R;
    const int x0 = (int)(blockIdx.x * kElevTileX) - R, y0 = (int)(blockIdx.y * kElevTileY) - R;
    const int tid = (int)(threadIdx.y * kElevTileX + threadIdx.x);
    for (int w = tid; w < pitch * rows; w += (int)(kElevTileX * kElevTileY)) {
        const int ly = w / pitch, lx = w - ly * pitch;
        const int gx = x0 + lx, gy = y0 + ly;
        int32_t v = kElevInvalid;
        if (gx >= 0 && gx < (int)a.width && gy >= 0 && gy < (int)a.height) {
            const ElevCell *e = cells + ((size_t)gy * a.width + (size_t)gx);
            if (e->count >= a.min_points) v = e->zmin;
        }
        tile[w] = v;
    }
    __syncthreads();
    const uint32_t cx = blockIdx.x * kElevTileX + threadIdx.x, cy = blockIdx.y * kElevTileY + threadIdx.y;
    const bool in_grid = cx < a.width && cy < a.height;
    bool unknown = false, lethal = false, costed = false;
    if (in_grid) {
        const size_t c = (size_t)cy * a.width + cx;
        const int lcx = (int)threadIdx.x + R, lcy = (int)threadIdx.y + R;
        const int32_t z0 = tile[lcy * pitch + lcx];
        const double Q = 1.0 / 256.0;
        const float nanf_ = __builtin_nanf("");
        float o_min = nanf_, o_max = nanf_, o_mean = nanf_, o_slope = nanf_, o_rough = nanf_, o_step = nanf_;
        int8_t cost = (int8_t)-1;
        if (z0 == kElevInvalid) {
            unknown = true;
        } else {
            long long n = 0, Si = 0, Sj = 0, Sii = 0, Sij = 0, Sjj = 0, Sd = 0, Sid = 0, Sjd = 0, step_q = 0;
            for (int j = -R; j <= R; j++) {
                for (int i = -R; i <= R; i++) {
                    const int32_t z = tile[(lcy + j) * pitch + (lcx + i)];
                    if (z == kElevInvalid) continue;
                    const long long dd = (long long)z - (long long)z0;
                    n += 1, Si += i, Sj += j, Sii += i * i, Sij += i * j, Sjj += j * j;
                    Sd += dd, Sid += i * dd, Sjd += j * dd;
                    if (i >= -1 && i <= 1 && j >= -1 && j <= 1 && (i != 0 || j != 0)) {
                        const long long ad = dd < 0 ? -dd : dd;
                        step_q = ad > step_q ? ad : step_q;
                    }
                }
            }
            const long long det = Sii * (Sjj * n - Sj * Sj) - Sij * (Sij * n - Sj * Si) + Si * (Sij * Sj - Sjj * Si);
            double slope = 0.0, rough = 0.0;
            if (det > 0) {
                const long long a_num = Sid * (Sjj * n - Sj * Sj) - Sij * (Sjd * n - Sj * Sd) + Si * (Sjd * Sj - Sjj * Sd);
                const long long b_num = Sii * (Sjd * n - Sj * Sd) - Sid * (Sij * n - Sj * Si) + Si * (Sij * Sd - Sjd * Si);
                const long long c_num = Sii * (Sjj * Sd - Sjd * Sj) - Sij * (Sij * Sd - Sjd * Si) + Sid * (Sij * Sj - Sjj * Si);
                const double A = (double)a_num / (double)det, B = (double)b_num / (double)det, C = (double)c_num / (double)det;
                slope = (__dsqrt_rn(A * A + B * B) * Q) / (double)a.resolution;
                double S = 0.0;
                for (int j = -R; j <= R; j++) {
                    for (int i = -R; i <= R; i++) {
                        const int32_t z = tile[(lcy + j) * pitch + (lcx + i)];
                        if (z == kElevInvalid) continue;
                        const double e = (double)((long long)z - (long long)z0) - ((A * (double)i + B * (double)j) + C);
                        S = S + e * e;
                    }
                }
                rough = __dsqrt_rn(S / (double)n) * Q;
                o_slope = (float)slope, o_rough = (float)rough;
            }
            const ElevCell e = cells[c];
            const double step = Q * (double)step_q;
            const double span = Q * (double)((long long)e.zmax - (long long)e.zmin);
            o_step = (float)step;
            o_min = (float)((double)a.z_ref + (double)e.zmin * Q);
            o_max = (float)((double)a.z_ref + (double)e.zmax * Q);
            o_mean = (float)((double)a.z_ref + ((double)e.sum * Q) / (double)e.count);
            if (a.cost_out) {
                lethal = span > (double)a.max_span || step > (double)a.max_step || (det > 0 && slope > (double)a.max_slope);
                costed = !lethal;
                if (lethal) {
                    cost = (int8_t)100;
                } else {
                    double m = step / (double)a.max_step;
                    if (det > 0) {
                        const double ms = slope / (double)a.max_slope, mr = rough / (double)a.max_rough;
                        m = ms > m ? ms : m;
                        m = mr > m ? mr : m;
                    }
                    m = m < 1.0 ? m : 1.0;
                    cost = (int8_t)(int)__builtin_floor(99.0 * m);
                }
            }
        }
        if (a.min_out) a.min_out[c] = o_min;
        if (a.max_out) a.max_out[c] = o_max;
        if (a.mean_out) a.mean_out[c] = o_mean;
        if (a.slope_out) a.slope_out[c] = o_slope;
        if (a.rough_out) a.rough_out[c] = o_rough;
        if (a.step_out) a.step_out[c] = o_step;
        if (a.cost_out) a.cost_out[c] = cost;
    }
    if (a.cost_out) {  // the three totals, summed over the wave first
        const uint32_t nu = (uint32_t)__popcll(__ballot(unknown)), nl = (uint32_t)__popcll(__ballot(lethal)),
                       nc = (uint32_t)__popcll(__ballot(costed));
        if ((tid & 63) == 0) {
            if (nu) atomicAdd(totals + EC_UNKNOWN, nu);
            if (nl) atomicAdd(totals + EC_LETHAL, nl);
            if (nc) atomicAdd(totals + EC_COSTED, nc);
        }
    }
}

}  // namespace lom
