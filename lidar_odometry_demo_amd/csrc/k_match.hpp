// Correspondence search of the scan matcher: the DPP row helpers and k_match (see match.hip for the
// overview).  Device code only; match.hip is the one translation unit that instantiates and launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "lom_internal.hpp"
#include "match_launch.hpp"  // launch geometry (kMatch*, kEvalThreads), MatchRec, BatchProblem

namespace lom {

constexpr uint32_t kRecValid = 0x40000000u;  // rows below 2^30 are told apart (a larger map still matches, it only rewrites)

// per-query debug record written by k_match for lom_match_find_pairs
struct __attribute__((aligned(8))) QStat {
    float sq_dist;
    uint32_t n_cand;
    uint32_t n_occ;
    uint32_t pad;
};

// ---------------------------------------------------------------------------
// k_match<G>: one query per group of G lanes (G = 16: four queries per wave).
//
//  1. probe    lane l takes neighbours b = l, l+G, ... < 27 in the reference's scan
//              order ix, iy, iz (voxel_grid.h:175-179): one 16-byte slot load each.
//  2. prune    a neighbour voxel whose nearest possible coordinate is provably
//              farther than max_dist cannot hold a point with d2 < max_sq
//              (voxel_grid.h:186), so its points are not read.  Exact: such points
//              never win in the reference either.  Counts stay the reference's.
//  3. flatten  the remaining voxels' points, cut into chunks of up to four consecutive
//              rows of one voxel, form one chunk sequence in scan order (inclusive prefix
//              of the chunk counts in LDS); lane l takes chunks l, l+G, ... and finds each
//              one's voxel by a 5-step binary search -- one search, one address and 48 bytes
//              in flight (three dwordx4) per four candidates.
//  4. select   private strict minimum per lane (candidates arrive in scan order),
//              then the lexicographic minimum of (sq_dist, candidate ordinal) over
//              the group == "first encountered wins" of voxel_grid.h:183-191.
// ---------------------------------------------------------------------------
// Pruning bound along one axis, once per query: squared lower bounds of |q - x| over the
// coordinates x of the neighbour voxels i-1 (gm2) and i+1 (gp2).  Coordinates with
// (int)(x / vs) == j lie in [lo_j, hi_j] (truncation: index 0 is double width), so voxel
// i+1 starts at (i >= 0 ? i+1 : i) * vs and voxel i-1 ends at (i <= 0 ? i-1 : i) * vs.
// (slack_vs = 1e-4 * vs comes from the caller as a wave-uniform value in a scalar register: left to the compiler it was
// hoisted into a vector register and, under the register budget, spilled -- and the reload's s_waitcnt vmcnt(0) then
// waited for every global load in flight, the next query's prefetch included)
__device__ __forceinline__ void axis_gaps(float q, int i, float vs, float slack_vs, float &gm2, float &gp2)
{
    const float fi = (float)i;
    const float face_p = ((i >= 0) ? fi + 1.f : fi) * vs;
    const float face_m = ((i <= 0) ? fi - 1.f : fi) * vs;
    // slack for the f32 rounding of x / vs at the voxel faces and of the distance itself
    const float slack = slack_vs + 1e-6f * fabsf(q);
    const float gp = fmaxf((face_p - q) - slack, 0.f);
    const float gm = fmaxf((q - face_m) - slack, 0.f);
    gm2 = gm * gm;
    gp2 = gp * gp;
}

// One query group == one 16-lane DPP row: shifts, butterflies and mirrors inside the row are
// VALU operand modifiers (no LDS crossbar trip, no index registers).  Lanes shifted in from
// outside the row read 0.  Every lane of a row is active wherever these are used.
template <int kCtrl>
__device__ __forceinline__ uint32_t row_dpp(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xF, 0xF, true);
}
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;
__device__ __forceinline__ uint32_t row_scan_inclusive(uint32_t v)
{
    v += row_dpp<0x111>(v);  // row_shr:1
    v += row_dpp<0x112>(v);  // row_shr:2
    v += row_dpp<0x114>(v);  // row_shr:4
    v += row_dpp<0x118>(v);  // row_shr:8
    return v;
}
__device__ __forceinline__ uint32_t row_sum(uint32_t v)
{
    v += row_dpp<kDppXor1>(v);
    v += row_dpp<kDppXor2>(v);
    v += row_dpp<kDppHalfMirror>(v);  // pairs the two quads of a half
    v += row_dpp<kDppMirror>(v);      // pairs the two halves
    return v;
}
__device__ __forceinline__ uint32_t row_min32(uint32_t v)
{
    v = min(v, row_dpp<kDppXor1>(v));
    v = min(v, row_dpp<kDppXor2>(v));
    v = min(v, row_dpp<kDppHalfMirror>(v));
    return min(v, row_dpp<kDppMirror>(v));
}
// lane kLane (0..15) of the row, to every lane of the row (ds_swizzle bit mode: and 0x10, or kLane)
template <int kLane>
__device__ __forceinline__ uint32_t row_lane(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x10 | (kLane << 5));
}
// lane 15 of the row, to every lane of the row (ds_swizzle bit mode: and 0x10, or 0x0F)
__device__ __forceinline__ uint32_t row_last(uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1F0); }

template <int kCtrl>
__device__ __forceinline__ double dpp_f64(double v)  // the value of the DPP partner lane
{
    return __hiloint2double((int)row_dpp<kCtrl>((uint32_t)__double2hiint(v)),
                            (int)row_dpp<kCtrl>((uint32_t)__double2loint(v)));
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// Two 16-byte slot loads in flight together, each ONE dwordx4 (the compiler otherwise splits a
// slot into a key load and a dependent count/slab load: two round trips per hit).
__device__ __forceinline__ void load_slots2(const Slot *a, const Slot *b, u32x4 &ra, u32x4 &rb)
{
    asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %3, off\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(ra), "=&v"(rb)
                 : "v"(a), "v"(b)
                 : "memory");
}
__device__ __forceinline__ u32x4 load_slot(const Slot *a)
{
    u32x4 r;
    asm volatile("global_load_dwordx4 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(r) : "v"(a) : "memory");
    return r;
}

typedef float f32x3 __attribute__((ext_vector_type(3)));
// Four consecutive 12-byte rows = 48 bytes from one address as three 16-byte loads in flight together.  What the
// vector L1 charges a load instruction is, per four consecutive lanes, the 128-byte lines they touch
// (tools/microbench/tcp_lines.hip): three instructions over a lane's 48 bytes cost 3/4 of what four 12-byte loads do.
// The address is a multiple of 4, not of 16 unless K % 4 == 0: global_load_dwordx4 takes that on gfx950 (the driver
// runs the memory pipeline in unaligned mode; tools/microbench/unaligned_x4.hip checks it).
__device__ __forceinline__ void load_chunk48(const float *a, f32x3 (&r)[4])
{
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f32x4 v0, v1, v2;
    asm volatile("global_load_dwordx4 %0, %3, off\n\tglobal_load_dwordx4 %1, %3, off offset:16\n\t"
                 "global_load_dwordx4 %2, %3, off offset:32\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v0), "=&v"(v1), "=&v"(v2)
                 : "v"(a)
                 : "memory");
    r[0] = f32x3{v0.x, v0.y, v0.z};
    r[1] = f32x3{v0.w, v1.x, v1.y};
    r[2] = f32x3{v1.z, v1.w, v2.x};
    r[3] = f32x3{v2.y, v2.z, v2.w};
}

// Two 12-byte loads issued back to back and waited for together (the winner's point and normal).  The loads of a
// trip are asm blocks because, left to the compiler, the first use of load 1 was scheduled ahead of the address
// computation of load 2: the "two loads in flight" of round 2 were two dependent round trips (C2 / C3 / C4: 7.9 / 29.9
// / 53.7 us; issued together 6.8 / 28.1 / 47.7 us, profiles/r03_b_*).
__device__ __forceinline__ void load_points2(const float *a, const float *b, f32x3 &ra, f32x3 &rb)
{
    asm volatile("global_load_dwordx3 %0, %2, off\n\tglobal_load_dwordx3 %1, %3, off\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(ra), "=&v"(rb)
                 : "v"(a), "v"(b)
                 : "memory");
}

// kStamp = true is a diagnostic build (lom_debug_match_stamps): thread 0 of every workgroup records
// the shader clock after each phase of its first query, every wait fully drained before a stamp.
// Its run time is not representative; the product launches kStamp = false only.
template <bool kOn>
struct Stamper {  // product build: nothing
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void first_done() {}
    __device__ __forceinline__ void flush(unsigned long long *) {}
};
template <>
struct Stamper<true> {
    unsigned long long t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool first = true;
    __device__ __forceinline__ void mark(int i)
    {
        if (!first) return;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        if (threadIdx.x == 0) t[i] = __builtin_amdgcn_s_memtime();
    }
    __device__ __forceinline__ void first_done() { first = false; }
    __device__ __forceinline__ void flush(unsigned long long *out)
    {
        if (threadIdx.x != 0) return;
        t[7] = __builtin_amdgcn_s_memtime();
        for (int i = 0; i < 8; i++) out[(size_t)blockIdx.x * 8 + i] = t[i];
    }
};
#define LOM_STAMP(i) stamper.mark(i)

typedef const __attribute__((address_space(4))) BatchProblem *ConstBatch;  // read with scalar loads, like kernel arguments

// kChained: the pose comes from the AlignState a previous k_lm left in HBM (read through the
// constant address space: scalar loads, like kernel arguments), and the launch does nothing once
// the outer loop has finished -- the host enqueues several outer iterations ahead.
// kPrev: the records of the PREVIOUS search of the same scan against the same map are still at out_rec (outer
// iterations >= 2 of an align): where the old winner still lies in the query's 27 voxels, its f32 distance at the new
// pose bounds this search's minimum from above, and a neighbour voxel whose nearest face is provably farther than that
// cannot hold the winner -- see "temporal bound" in the loop.  Exact.
// kCount: the reference-algorithm counts per query (occupied voxels among the 27, their stored points: SURVEY.md 8d's
// cand(q), the tests' n_cand / n_occ) need every one of the 27 slots.  Without them (the product's align, unless
// LOM_OPT_COUNT_CANDIDATES asks) a neighbour voxel that the bound prunes is not even looked up: its slot is neither
// hashed nor loaded -- the result cannot depend on whether a voxel exists whose points could not win.
// kBatch (chained only): one launch for all problems of a batched align's round -- blockIdx.y selects the problem
// (`batch[blockIdx.y]`: map, scan, records, counters, state), blockIdx.x runs over THAT problem's search grid (workgroups
// beyond it leave at once); per query everything is what the single align's launch does.
template <int G, int kU, int kMinWaves, bool kStamp = false, bool kChained = false, bool kPrev = kChained, bool kCount = true,
          bool kBatch = false>
__global__ __launch_bounds__(kMatchThreads, kMinWaves) void k_match(MapView map, const char *__restrict__ src, size_t stride,
                                                         uint32_t n, PoseArgs Parg, int32_t *__restrict__ out_idx,
                                                         MatchRec *__restrict__ out_rec,
                                                         QStat *__restrict__ out_stat,
                                                         uint32_t *__restrict__ block_counters,
                                                         unsigned long long *__restrict__ stamps = nullptr,
                                                         const AlignState *state = nullptr,
                                                         const BatchProblem *batch = nullptr)
{
    static_assert(G == 16 && kU == 4, "one query per 16-lane DPP row, a chunk of four rows per lane and trip");
    static_assert(!kBatch || (kChained && !kStamp), "the batch form is a chained search");
    constexpr uint32_t kRowsLog2 = 2;  // rows per chunk
    uint32_t batch_grid = 0;  // (kBatch) this problem's search grid
    if constexpr (kBatch) {
        const ConstBatch d = (ConstBatch)(batch + blockIdx.y);
        // (the `map` argument is unused)
        map.table = d->map.table;
        map.mask = d->map.mask;
        map.shift = d->map.shift;
        map.pts = d->map.pts;
        map.nrm = d->map.nrm;
        map.K = d->map.K;
        map.voxel_size = d->map.voxel_size;
        map.inv_voxel_size = d->map.inv_voxel_size;
        map.prune_slack = d->map.prune_slack;
        src = d->src;
        stride = d->stride;
        n = d->n;
        out_rec = d->rec;
        block_counters = d->block_counters;
        state = d->state;
        batch_grid = d->match_blocks;
        if (blockIdx.x >= batch_grid) return;
    }
    // the first query's source point is on its way before anything else: the chained form's pose comes through a
    // scalar-cache miss of its own, and the LDS tables below need a barrier -- one memory round trip instead of two
    // ahead of the first probe (the loop fetches the next query's point the same way, behind the current one's work)
    constexpr int kGroups0 = kMatchThreads / G;
    // (the chained form: the pointer to the state comes in with the kernel's first argument loads, not in a round trip
    // of its own between the point's load and the pose's)
    if constexpr (kChained) asm volatile("" ::"s"(state));
    const uint32_t q_first = blockIdx.x * kGroups0 + threadIdx.x / G;
    f32x3 sp_next = {0.f, 0.f, 0.f};
    // (without the counts the temporal bound decides which slots are loaded at all: the previous record travels with the
    // source point, one query ahead; with them it is only needed once the slots are back)
    constexpr bool kPrevEarly = kPrev && !kCount;
    float4 pv_next = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q_first < n) {
        sp_next = *reinterpret_cast<const f32x3 *>(src + (size_t)q_first * stride);
        if constexpr (kPrevEarly) pv_next = reinterpret_cast<const float4 *>(out_rec + q_first)[1];
    }
    struct {
        double R[9], t[3];
        float max_sq;
    } P;
    if constexpr (kChained) {
        typedef const __attribute__((address_space(4))) AlignState *ConstState;
        ConstState cs = (ConstState)(state);
        // pose and stop flags in ONE scalar round trip (the flags first and the pose behind the branch were two)
#pragma unroll
        for (int i = 0; i < 9; i++) P.R[i] = cs->P.R[i];
#pragma unroll
        for (int i = 0; i < 3; i++) P.t[i] = cs->P.t[i];
        P.max_sq = cs->P.max_sq;
        const int stop = cs->finished | cs->error;
        asm volatile("" ::"s"(P.max_sq), "s"(stop), "s"(P.R[0]), "s"(P.R[1]), "s"(P.R[2]), "s"(P.R[3]), "s"(P.R[4]), "s"(P.R[5]),
                     "s"(P.R[6]), "s"(P.R[7]), "s"(P.R[8]), "s"(P.t[0]), "s"(P.t[1]), "s"(P.t[2]));  // all loaded before the branch
        if (stop) return;
    } else {
#pragma unroll
        for (int i = 0; i < 9; i++) P.R[i] = Parg.R[i];
#pragma unroll
        for (int i = 0; i < 3; i++) P.t[i] = Parg.t[i];
        P.max_sq = Parg.max_sq;
    }
    Stamper<kStamp> stamper;
    LOM_STAMP(0);
    constexpr int kGroups = kMatchThreads / G;
    constexpr int kSets = 2;                  // neighbours b = gl (set 0) and 16 + gl (set 1) < 27
    // per neighbour b in scan order: .z inclusive prefix of the scanned CHUNKS (entries >= 27: never reached),
    // .x slab * K - 4 * exclusive prefix, so that chunk ch of the flattened sequence starts at row .x + 4 * ch,
    // .y count + 4 * exclusive prefix: .y - 4 * ch rows of the voxel remain from there
    __shared__ uint4 s_pb[kGroups][32];
    __shared__ uint32_t s_cnt[kGroups][4];
    __shared__ double s_pose[12];             // [component][R row (3), t]: what the component lanes multiply with
    __shared__ float s_gap[kGroups][12];      // per query [axis][to voxel i-1, 0, to voxel i+1]: squared pruning gaps
    const int gl = threadIdx.x % G;
    const int grp = threadIdx.x / G;
    const uint32_t groups_total = (kBatch ? batch_grid : gridDim.x) * kGroups;
    // per-group counters live in LDS (one ds_add per counter and query by the writing lane):
    // four fewer live registers keep the kernel at 64 VGPRs without spilling
    if (gl < 4) s_cnt[grp][gl] = 0u;
    if (threadIdx.x < 12) {
        const int c = threadIdx.x >> 2, k = threadIdx.x & 3;
        double v = P.t[0];
#pragma unroll
        for (int cc = 0; cc < 3; cc++)
#pragma unroll
            for (int kk = 0; kk < 4; kk++)
                if (c == cc && k == kk) v = kk < 3 ? P.R[cc * 3 + kk] : P.t[cc];
        s_pose[threadIdx.x] = v;
    }
    __syncthreads();
    // Work that is the same for the lanes of a query is split over them instead of repeated by each: lanes
    // 0, 1, 2 of a row prepare the x, y, z component (f64 transform, f32 cast, truncating index, the two
    // pruning gaps of that axis) and hand the results to the row -- values through ds_swizzle broadcasts, the
    // gap table through 12 LDS words.  Lanes 3..15 repeat component z (same instruction stream, results unused).
    const int comp = gl < 2 ? gl : 2;
    const double *my_pose = s_pose + comp * 4;
    // this lane's neighbours (scan order ix, iy, iz): key and hash of a neighbour follow from the centre's by ADDING a lane
    // constant -- pack_key is a sum of shifted fields, and the Fibonacci hash multiplies by a constant modulo 2^64, so
    // hash(key0 + d) = (key0 * phi + d * phi) >> shift.  One 64-bit multiply per query, no per-neighbour packing.
    // (the products are kept opaque: under the 72-register budget the compiler otherwise folds prod0 + dprod back into
    // (key0 + dkey) * phi -- two quarter-rate multiplies and a 64-bit mad per neighbour -- to save their four registers;
    // the three gap-table addresses of a neighbour travel as byte offsets packed into one register instead)
    constexpr unsigned long long kPhi = 0x9E3779B97F4A7C15ull;
    unsigned long long dkey[kSets], dprod[kSets];
    uint32_t gap_off[kSets];
#pragma unroll
    for (int s = 0; s < kSets; s++) {
        const int b = gl + s * G;
        const int dx = b / 9 - 1, dy = (b / 3) % 3 - 1, dz = b % 3 - 1;
        dkey[s] = (unsigned long long)(((long long)dx << 42) + ((long long)dy << 21) + (long long)dz);
        dprod[s] = dkey[s] * kPhi;
        asm volatile("" : "+v"(dprod[s]));
        const uint32_t ox = 4u * (uint32_t)(0 + (b < 27 ? dx + 1 : 1)), oy = 4u * (uint32_t)(3 + (b < 27 ? dy + 1 : 1)),
                       oz = 4u * (uint32_t)(6 + (b < 27 ? dz + 1 : 1));
        gap_off[s] = ox | (oy << 8) | (oz << 16);
    }
    const char *gap_base = reinterpret_cast<const char *>(&s_gap[grp][0]);
    if (gl < 3) s_gap[grp][gl * 3 + 1] = 0.f;  // the centre column of the gap table never changes (own group, own wave)

    const float slack_vs = map.prune_slack;  // 1e-4f * voxel_size
    for (uint32_t q = blockIdx.x * kGroups + grp; q < n; q += groups_total) {
        f32x3 sp = sp_next;
        // the previous search's {winner point, valid} of this query: not needed before the slots are back, so it is
        // asked for here (one round trip beside theirs) rather than a query ahead (four more live registers)
        float4 pv = pv_next;
        if constexpr (kPrev && !kPrevEarly) pv = reinterpret_cast<const float4 *>(out_rec + q)[1];
        if (q + groups_total < n) {
            sp_next = *reinterpret_cast<const f32x3 *>(src + (size_t)(q + groups_total) * stride);
            if constexpr (kPrevEarly) pv_next = reinterpret_cast<const float4 *>(out_rec + (q + groups_total))[1];
        }
        const double p0 = (double)sp.x, p1 = (double)sp.y, p2 = (double)sp.z;
        // voxel_grid.h:220-223: R*p + t in f64 (Eigen order a0 + (a1 + a2)), cast to f32 -- this lane's component
        const float qc = (float)((my_pose[0] * p0 + (my_pose[1] * p1 + my_pose[2] * p2)) + my_pose[3]);
        int ic = 0;
        const bool okc = voxel_index_fast(qc, map.voxel_size, map.inv_voxel_size, ic);
        float gm2, gp2;
        axis_gaps(qc, ic, map.voxel_size, slack_vs, gm2, gp2);
        if (gl < 3) {
            s_gap[grp][gl * 3 + 0] = gm2;
            s_gap[grp][gl * 3 + 2] = gp2;
        }
        const int icc = okc ? ic : (int)0x80000000;  // out of range / not finite
        // temporal bound, part 1 (this lane's axis): does the old winner's own voxel index -- the expression the insert
        // stored it under -- lie within one of the new centre's?  (lanes 3..15 repeat axis z, as above)
        uint32_t near_c = 0u;
        if constexpr (kPrev) {
            const float oc = gl == 0 ? pv.x : (gl == 1 ? pv.y : pv.z);
            int io = 0;
            const bool oko = voxel_index_fast(oc, map.voxel_size, map.inv_voxel_size, io);
            near_c = (okc && oko && (uint32_t)(io - ic + 1) <= 2u) ? 1u : 0u;
        }
        const float qx = __uint_as_float(row_lane<0>(__float_as_uint(qc)));
        const float qy = __uint_as_float(row_lane<1>(__float_as_uint(qc)));
        const float qz = __uint_as_float(row_lane<2>(__float_as_uint(qc)));
        const int ix = (int)row_lane<0>((uint32_t)icc), iy = (int)row_lane<1>((uint32_t)icc),
                  iz = (int)row_lane<2>((uint32_t)icc);
        const bool inr = ix != (int)0x80000000 && iy != (int)0x80000000 && iz != (int)0x80000000;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        LOM_STAMP(1);  // source point loaded and transformed
        // ---- temporal bound, part 2 ----
        // The winner of the previous search (same scan, same map, the pose one solve earlier) is a stored point.  If its
        // voxel index lies within one of this query's centre index on every axis it is one of this query's candidates in
        // the reference (voxel_grid.h:175-183), so its distance d_prev2 -- the very f32 expression of the candidate loop
        // -- is an upper bound of this search's minimum B.  A voxel whose nearest face is provably farther than B holds
        // only points with d2 > B (the argument of the plain bound with B in place of max_sq, same slack): they can
        // neither win nor tie, so every candidate with d2 <= B -- the old winner among them -- is scanned in the
        // reference's order and the first strict minimum is the reference's (:183-191).  An old winner outside the 27
        // voxels, or beyond max_dist, or none: the plain bound.  With kCount the counts (n_cand, n_occ) stay the slot
        // counts of all 27 voxels.
        auto temporal_bound = [&]() -> float {
            float Bv = P.max_sq;
            if constexpr (kPrev) {
                const float ex = qx - pv.x, ey = qy - pv.y, ez = qz - pv.z;
                const float d_prev2 = ex * ex + (ey * ey + ez * ez);
                const bool near = row_min32(near_c) != 0u;  // all three axes (lanes 2..15 hold axis z)
                if (near && pv.w != 0.f && d_prev2 < P.max_sq) Bv = d_prev2;  // (NaN: no bound)
            }
            return Bv;
        };
        float B = P.max_sq;
        if constexpr (!kCount) B = temporal_bound();
        // ---- probe ----
        // stored indices lie in (-2^20, 2^20): a centre at least two voxels inside has all 27 neighbours in range
        const uint32_t kInner = (uint32_t)(2 * kIdxBias - 3);
        const bool safe = (uint32_t)(ix + (kIdxBias - 2)) < kInner && (uint32_t)(iy + (kIdxBias - 2)) < kInner &&
                          (uint32_t)(iz + (kIdxBias - 2)) < kInner;
        const unsigned long long key0 = inr ? pack_key(ix, iy, iz) : 0ull;
        const unsigned long long prod0 = key0 * kPhi;
        uint32_t cnt[kSets], scan_cnt[kSets], slab[kSets];
        unsigned long long key[kSets];
        uint32_t h[kSets];
        bool act[kSets];
        float lower[kSets];
#pragma unroll
        for (int s = 0; s < kSets; s++) {
            const int b = gl + s * G;
            act[s] = inr && b < 27;
            if (act[s] && !safe) {  // the outermost index layers: neighbours beyond the range cannot exist
                const int nx = ix + (b / 9 - 1), ny = iy + ((b / 3) % 3 - 1), nz = iz + (b % 3 - 1);
                act[s] = nx > -kIdxBias && nx < kIdxBias && ny > -kIdxBias && ny < kIdxBias && nz > -kIdxBias &&
                         nz < kIdxBias;
            }
            key[s] = act[s] ? key0 + dkey[s] : 0ull;
            h[s] = act[s] ? ((uint32_t)((prod0 + dprod[s]) >> map.shift) & map.mask) : 0u;
            lower[s] = *reinterpret_cast<const float *>(gap_base + (gap_off[s] & 0xFFu)) +
                       (*reinterpret_cast<const float *>(gap_base + ((gap_off[s] >> 8) & 0xFFu)) +
                        *reinterpret_cast<const float *>(gap_base + (gap_off[s] >> 16)));
            if constexpr (!kCount) {  // a pruned neighbour is not looked up
                if (lower[s] > B * 1.0001f) {
                    act[s] = false;
                    key[s] = 0ull;
                    h[s] = 0u;
                }
            }
        }
        // both sets' first slots in flight together
        u32x4 raw[kSets];
        load_slots2(map.table + h[0], map.table + h[1], raw[0], raw[1]);
#pragma unroll
        for (int s = 0; s < kSets; s++) {
            cnt[s] = 0;
            slab[s] = 0;
            if (act[s]) {
                u32x4 r = raw[s];
                uint32_t hh = h[s];
                for (uint32_t probe = 0; probe <= map.mask; probe++) {
                    const unsigned long long k = ((unsigned long long)r.y << 32) | r.x;
                    if (k == key[s]) {
                        cnt[s] = r.z;
                        slab[s] = r.w;
                        break;
                    }
                    if (k == kEmptyKey) break;
                    hh = (hh + 1) & map.mask;
                    r = load_slot(map.table + hh);
                }
            }
        }
        LOM_STAMP(2);  // slots probed
        uint32_t probed = 0;  // (lom_profile_match's tally launch: the slots this query asked for)
        if constexpr (!kCount && !kChained)
            if (out_stat) probed = row_sum((act[0] ? 1u : 0u) + (act[1] ? 1u : 0u));
        if constexpr (kCount) B = temporal_bound();
        uint32_t w_d, w_c, best_pi0, best_c, n_cand = 0, n_occ = 0, T = 0;  // T: points actually read
        float best;
        if constexpr (kCount) {
            // the reference's counts: occupied voxels (<= 27) above bit 26, stored points (<= 27 K, K < 2^16) below: one
            // row sum for both sets
            uint32_t mine = 0;
#pragma unroll
            for (int s = 0; s < kSets; s++) mine += cnt[s] | ((cnt[s] ? 1u : 0u) << 26);
            const uint32_t tot = row_sum(mine);
            n_cand = tot & ((1u << 26) - 1u);
            n_occ = tot >> 26;
        }
        const float bound = B * 1.0001f;
#pragma unroll
        for (int s = 0; s < kSets; s++) {
            // a neighbour voxel whose nearest face is provably farther than the bound is not read
            scan_cnt[s] = (lower[s] > bound) ? 0u : cnt[s];
        }
        // ---- group-wide prefix over the scanned neighbours in scan order ----
        // best starts at max_sq: "d2 < best" then implies voxel_grid.h:186's d2 < max_sq, and NaN never wins
        best = P.max_sq;
        best_c = 0xFFFFFFFFu;
        best_pi0 = 0;
        {
            // chunks of up to four consecutive points of one voxel: nch chunks per scanned voxel
            uint32_t nch[kSets], read = 0;
#pragma unroll
            for (int s = 0; s < kSets; s++) {
                nch[s] = (scan_cnt[s] + ((1u << kRowsLog2) - 1u)) >> kRowsLog2;
                read += scan_cnt[s];
            }
            uint32_t Tc = 0;  // chunks of this query
            if (map.K <= 16380u) {
                // both sets' chunk counts in one register (16 voxels x K / 4 < 2^16 each): ONE row scan, one broadcast
#pragma unroll
                for (int s = 0; s < kSets; s += 2) {
                    const uint32_t inc = row_scan_inclusive(nch[s] | (nch[s + 1] << 16));
                    const uint32_t last = row_last(inc);
                    const uint32_t tot_a = last & 0xFFFFu, inc_a = Tc + (inc & 0xFFFFu), inc_b = Tc + tot_a + (inc >> 16);
                    const uint32_t ex_a = (inc_a - nch[s]) << kRowsLog2, ex_b = (inc_b - nch[s + 1]) << kRowsLog2;
                    const int b_a = gl + s * G, b_b = b_a + G;
                    s_pb[grp][b_a] = make_uint4(slab[s] * map.K - ex_a, scan_cnt[s] + ex_a, (b_a < 27) ? inc_a : 0xFFFFFFFFu, 0u);
                    s_pb[grp][b_b] =
                        make_uint4(slab[s + 1] * map.K - ex_b, scan_cnt[s + 1] + ex_b, (b_b < 27) ? inc_b : 0xFFFFFFFFu, 0u);
                    Tc += tot_a + (last >> 16);
                }
            } else {
#pragma unroll
                for (int s = 0; s < kSets; s++) {
                    const uint32_t inc = row_scan_inclusive(nch[s]);
                    const int b = gl + s * G;
                    const uint32_t ex = (Tc + inc - nch[s]) << kRowsLog2;
                    s_pb[grp][b] = make_uint4(slab[s] * map.K - ex, scan_cnt[s] + ex, (b < 27) ? Tc + inc : 0xFFFFFFFFu, 0u);
                    Tc += row_last(inc);
                }
            }
            // points actually read (after the exact pruning): one more row sum (an LDS atomic per lane instead cost the
            // kernel's tail 0.3 us: sixteen lanes on one word)
            if constexpr (!kChained) T += row_sum(read);  // (only lom_profile_match reads it: not computed inside an align)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            LOM_STAMP(3);  // prefix in LDS
            // Binary search of a chunk's voxel: the first two of its five levels compare with three values read once
            // per query, the last reads the entry and its successor together -- three dependent LDS round trips
            // per chunk of four candidates.
            const uint4 *pb = s_pb[grp];
            const uint32_t p7 = pb[7].z, p15 = pb[15].z, p23 = pb[23].z;
            // lane l takes chunks l, l + 16, ... of the flattened sequence; a chunk's four points are consecutive rows:
            // one address, four 12-byte loads in flight, compared in ascending order (strict minimum per lane: first
            // wins).  Rows of a chunk beyond the voxel's count are read (they exist: the slab, the next one, or the
            // padding behind the last) and not compared.
            for (uint32_t ch = gl; ch < Tc; ch += G) {
                // smallest b with prefix[b] > ch
                uint32_t b = (p15 <= ch) ? 16u : 0u;
                b += ((b ? p23 : p7) <= ch) ? 8u : 0u;
                b += (pb[b + 3].z <= ch) ? 4u : 0u;
                b += (pb[b + 1].z <= ch) ? 2u : 0u;
                const uint4 e = pb[b];
                const uint2 nx = *reinterpret_cast<const uint2 *>(&pb[b + 1]);
                const bool up = e.z <= ch;
                const uint32_t c0 = ch << 2;
                const uint32_t pi0 = (up ? nx.x : e.x) + c0;   // first row of the chunk
                const uint32_t nv = (up ? nx.y : e.y) - c0;    // rows of the voxel from there on (>= 1)
                f32x3 pt[4];
                load_chunk48(map.pts + (size_t)pi0 * 3, pt);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const f32x3 a = pt[u];
                    const float dx = qx - a.x, dy = qy - a.y, dz = qz - a.z;
                    const float d2 = dx * dx + (dy * dy + dz * dz);  // voxel_grid.h:184 f32 squaredNorm
                    if ((u == 0 || nv > (uint32_t)u) && d2 < best) {  // :186-187 strict
                        best = d2;
                        best_c = c0 + (uint32_t)u;
                        best_pi0 = pi0;
                    }
                }
            }
        }
        LOM_STAMP(4);  // candidates scanned
        // lexicographic min over the group; d2 >= 0 so its bit pattern orders like the value
        // (as two 32-bit row minima -- the distance bits, then the ordinal among the lanes that hold that distance --:
        // half the instructions of four 64-bit compare-and-select steps)
        w_d = row_min32(__float_as_uint(best));
        w_c = row_min32(__float_as_uint(best) == w_d ? best_c : 0xFFFFFFFFu);
        const bool valid = w_c != 0xFFFFFFFFu;
        LOM_STAMP(5);  // group minimum known
        // the lane that scanned the winner reads its point again together with the normal (two loads, one round
        // trip: keeping the point in registers through the candidate loop cost three selects per candidate)
        if (valid ? (best_c == w_c) : (gl == 0)) {
            int32_t idx = -1;
            const size_t pi = (size_t)best_pi0 + (best_c & 3u);
            const uint32_t mark = valid ? (kRecValid | (uint32_t)pi) : 0u;
            if (valid) idx = (int32_t)pi;
            // Outer iterations >= 2: most queries find the winner they had (the pose moves by millimetres).  Such a query's
            // record -- point, normal, mark -- is what it would write again: neither the winner's point and normal are
            // fetched (the last of the query's dependent round trips) nor anything stored.
            bool same = false;
            if constexpr (kPrev) same = __float_as_uint(pv.w) == mark && pi < (size_t)kRecValid;
            if (!same) {
                f32x3 wp = {0.f, 0.f, 0.f}, wn = {0.f, 0.f, 0.f};
                if (valid) load_points2(map.pts + pi * 3, map.nrm + pi * 3, wp, wn);  // voxel_grid.h:197-198
                float4 *rec = reinterpret_cast<float4 *>(out_rec + q);
                if constexpr (kPrev)
                    reinterpret_cast<float *>(rec)[3] = wn.x;  // the source point is there since the first search of this scan
                else
                    rec[0] = make_float4(sp.x, sp.y, sp.z, wn.x);
                rec[1] = make_float4(wp.x, wp.y, wp.z, __uint_as_float(mark));
                rec[2] = make_float4(wn.y, wn.z, 0.f, 0.f);
            }
            if constexpr (!kChained) out_idx[q] = idx;  // (only lom_match_find_pairs reads it)
            if (!kChained && out_stat) {
                QStat st;
                st.sq_dist = valid ? best : 0.f;
                // with the counts: the reference algorithm's; without: what this launch itself read (rows) and looked up
                // (slots) for the query -- lom_profile_match's "requested bytes"; lom_match_find_pairs reports zeros then
                st.n_cand = kCount ? n_cand : T;
                st.n_occ = kCount ? n_occ : probed;
                st.pad = 0;
                out_stat[q] = st;
            }
            atomicAdd(&s_cnt[grp][0], valid ? 1u : 0u);
            if constexpr (kCount) {
                atomicAdd(&s_cnt[grp][1], n_cand);
                atomicAdd(&s_cnt[grp][2], n_occ);
            }
            if constexpr (!kChained) atomicAdd(&s_cnt[grp][3], T);  // candidates actually read (after the exact pruning)
        }
        LOM_STAMP(6);  // winner's normal loaded, record stored
        stamper.first_done();
        // the LDS tables are rewritten next iteration: all reads above are complete for this wave
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    stamper.flush(stamps);
    // per-block counters, summed in fixed order by k_finish (no same-address atomics:
    // one word saturates at ~88 atomics/us, MI355X_MICROARCH.md "dequeue")
    __syncthreads();
    if (threadIdx.x < 4) {
        uint32_t v = 0;
        for (int g = 0; g < kGroups; g++) v += s_cnt[g][threadIdx.x];
        block_counters[blockIdx.x * 4 + threadIdx.x] = v;
    }
}
#undef LOM_STAMP

}  // namespace lom
