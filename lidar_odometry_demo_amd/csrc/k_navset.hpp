// Navigation field set (include/lidar_odometry_amd.h, "navigation field set"): k_navset_seed, k_navset_relax,
// k_navset_plane_count, k_navset_report, k_navset_gather, k_navset_nearest and k_navset_trace.  Device code only;
// navset.hip is the one translation unit that instantiates and launches it.  The fields are planar, [n_fields][height]
// [width] u32, over one plane and one table; the tile body, the walk and the step rules are k_navfield.hpp's.  Integers
// throughout; plain vector stores and vector atomics only; no workgroup ever waits for another.
#pragma once
#define LOM_NAV_DEVICE_FUNCTIONS_ONLY  // the constants, the step rules, nav_relax_tile and nav_walk; no kernel
#include "k_navfield.hpp"

namespace lom {

constexpr uint32_t kNavSetNoOwner = 0xFFFFu;      // LOM_NAVSET_NO_OWNER
constexpr uint32_t kNavSetReportGroups = 64;      // workgroups of k_navset_report per field, at most
constexpr uint32_t kNavSetNearestGroups = 2048;   // workgroups of k_navset_nearest, at most
constexpr uint32_t kNavSetOwnerSlots = 64;        // per-workgroup owner counts of k_navset_nearest

// the words of a field's report (zeroed per solve), and of the plane's
enum { NSW_REACHED = 0, NSW_MAX_POTENTIAL = 1, NSW_RANGE = 2, NSW_GOALS_USED = 3, NSW_GOALS_REJECTED = 4, NSW_FIELD_COUNT = 8 };
enum { NSP_BLOCKED = 0, NSP_INVALID = 1, NSP_COUNT = 2 };

// the sum of v over the workgroup, in lane 0 (s: four words of LDS, free again behind the call)
__device__ __forceinline__ uint32_t navset_group_sum(uint32_t v, uint32_t *s)
{
    for (uint32_t o = 32u; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, (int)o);
    if ((threadIdx.x & 63u) == 0u) s[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint32_t total = s[0] + s[1] + s[2] + s[3];
    __syncthreads();
    return total;
}

// One tile of one field in one launch of the relaxation: k_nav_relax's body (k_navfield.hpp, where the comment says why any
// schedule gives the same bytes and why that covers the fields of a set) on the field, marks and flag it is given.  The two
// bodies are the same text; k_nav_relax keeps its own because its resources moved when it was built through this function.
__device__ __forceinline__ void nav_relax_tile(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table, NavArgs a,
                                               uint32_t inner_cap, uint32_t all_tiles, uint32_t *field, uint32_t *marks_cur,
                                               uint32_t *marks_nxt, uint32_t *flag)
{
    __shared__ uint32_t s_p[kNavHaloCells];  // the potentials, with the halo
    __shared__ uint32_t s_c[kNavHaloCells];  // the cell costs, 0 = impassable or outside the grid
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_nb;                // the neighbour tiles to mark, a bit per direction
    __shared__ uint32_t s_more[3];           // "a cell fell in sweep i" at i % 3

    const uint32_t tile = blockIdx.y * a.tiles_x + blockIdx.x;
    if ((all_tiles | marks_cur[tile]) == 0u) return;  // (the same word for every lane: the whole workgroup leaves)
    const uint32_t t = threadIdx.x;
    s_tab[t] = table[t];
    if (t == 0u) s_nb = s_more[0] = s_more[1] = s_more[2] = 0u;
    __syncthreads();
    if (t == 0u) marks_cur[tile] = 0u;  // behind the barrier: every lane has read the word

    const int gx0 = (int)(blockIdx.x * kNavTile) - 1, gy0 = (int)(blockIdx.y * kNavTile) - 1;
    for (uint32_t i = t; i < kNavHaloCells; i += kNavThreads) {
        const int gx = gx0 + (int)(i % kNavHalo), gy = gy0 + (int)(i / kNavHalo);
        uint32_t p = kNavUnreached, c = 0u;
        if (gx >= 0 && gy >= 0 && gx < (int)a.width && gy < (int)a.height) {
            const size_t cell = (size_t)gy * a.width + (uint32_t)gx;
            p = field[cell];
            c = s_tab[(uint8_t)plane[cell]];
        }
        s_p[i] = p, s_c[i] = c;
    }
    __syncthreads();

    // per owned cell: its place in LDS, its cost, the steps it may take (a bit per direction), its value at the load and now
    uint32_t li[4], cost[4], steps[4], first[4], cur[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t idx = t + kNavThreads * k, x = idx & 31u, y = idx >> 5;
        li[k] = (y + 1u) * kNavHalo + x + 1u;
        cost[k] = s_c[li[k]];
        first[k] = cur[k] = s_p[li[k]];
        uint32_t m = 0u;
        if (cost[k]) {
#pragma unroll
            for (uint32_t d = 0; d < 8u; d++) {
                const int o = nav_dy(d) * (int)kNavHalo + nav_dx(d);
                bool ok = s_c[(int)li[k] + o] != 0u;
                if (d >= 4u) ok = ok && s_c[(int)li[k] + nav_dx(d)] != 0u && s_c[(int)li[k] + nav_dy(d) * (int)kNavHalo] != 0u;
                m |= ok ? 1u << d : 0u;
            }
        }
        steps[k] = m;
    }

    // the sweeps, in place: P[a] = min(P[a], min over allowed b of P[b] + len * c[a]), candidates above LOM_NAV_MAX dropped
    // Sweep i raises s_more[i % 3] in front of its barrier and reads it behind; lane 0 then lowers the word of sweep i + 2,
    // which sweep i - 1 read last (every lane is past barrier i) and sweep i + 2 writes next (behind barrier i + 1).
    uint32_t sweeps = 0u, more;
    do {
        bool changed = false;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            if (!steps[k]) continue;
            uint32_t best = cur[k];
#pragma unroll
            for (uint32_t d = 0; d < 8u; d++) {
                if (!(steps[k] >> d & 1u)) continue;
                const uint32_t pb = s_p[(int)li[k] + nav_dy(d) * (int)kNavHalo + nav_dx(d)];
                const uint32_t w = nav_len(d) * cost[k];  // < 2^27
                if (pb <= kNavMax - w) best = min(best, pb + w);  // (unreached is above kNavMax - w)
            }
            if (best < cur[k]) {
                cur[k] = best;
                s_p[li[k]] = best;
                changed = true;
            }
        }
        const uint32_t slot = sweeps % 3u;
        if (changed) s_more[slot] = 1u;
        __syncthreads();
        more = s_more[slot];
        if (t == 0u) s_more[(slot + 2u) % 3u] = 0u;
        sweeps++;
    } while (more && sweeps < inner_cap);

    // the interior that fell goes back; a border cell that fell names the neighbour tiles that read it
    uint32_t nb = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        if (cur[k] >= first[k]) continue;
        const uint32_t idx = t + kNavThreads * k, x = idx & 31u, y = idx >> 5;
        field[(size_t)(blockIdx.y * kNavTile + y) * a.width + blockIdx.x * kNavTile + x] = cur[k];
        const bool e = x == kNavTile - 1u, n = y == kNavTile - 1u, w = x == 0u, s = y == 0u;
        nb |= (e ? 1u : 0u) | (n ? 2u : 0u) | (w ? 4u : 0u) | (s ? 8u : 0u) | (e && n ? 16u : 0u) | (w && n ? 32u : 0u) |
              (w && s ? 64u : 0u) | (e && s ? 128u : 0u);
    }
    if (nb) atomicOr(&s_nb, nb);
    __syncthreads();
    if (t < 8u && (s_nb >> t & 1u)) {
        const int tx = (int)blockIdx.x + nav_dx(t), ty = (int)blockIdx.y + nav_dy(t);
        if (tx >= 0 && ty >= 0 && tx < (int)a.tiles_x && ty < (int)a.tiles_y) {
            marks_nxt[(uint32_t)ty * a.tiles_x + (uint32_t)tx] = 1u;
            *flag = 1u;
        }
    }
    if (t == 8u && more) {  // stopped at the cap: not settled yet
        marks_nxt[tile] = 1u;
        *flag = 1u;
    }
}

// A lane per goal of all fields (cells, as k_nav_seed takes them), field_of[i] its field: k_nav_seed's rule on that
// field's P, marks and words.  Duplicates within a field count once; two fields may hold the same goal.
__global__ __launch_bounds__(kNavThreads) void k_navset_seed(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table, NavArgs a,
                                                             const int32_t *__restrict__ goals, const uint32_t *__restrict__ field_of,
                                                             uint32_t n, uint32_t n_tiles, uint32_t *fields, uint32_t *marks0,
                                                             uint32_t *words)
{
    const uint32_t i = blockIdx.x * kNavThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t z = field_of[i];
    const int x = goals[2 * (size_t)i], y = goals[2 * (size_t)i + 1];
    uint32_t *const w = words + (size_t)z * NSW_FIELD_COUNT;
    if (!nav_cost_at(plane, table, a.width, a.height, x, y)) {
        atomicAdd(w + NSW_GOALS_REJECTED, 1u);
        return;
    }
    uint32_t *const field = fields + (size_t)z * a.width * a.height;
    if (atomicExch(field + (size_t)y * a.width + (uint32_t)x, 0u) == 0u) return;  // a duplicate
    atomicAdd(w + NSW_GOALS_USED, 1u);
    uint32_t *const marks = marks0 + (size_t)z * n_tiles;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int nx = x + dx, ny = y + dy;
            if (nx >= 0 && ny >= 0 && nx < (int)a.width && ny < (int)a.height)
                marks[((uint32_t)ny / kNavTile) * a.tiles_x + (uint32_t)nx / kNavTile] = 1u;
        }
}

// One launch of the relaxation of every field: the tile (blockIdx.x, blockIdx.y) of field blockIdx.z.  marks_cur and
// marks_nxt are [n_fields][n_tiles]; *flag is the one word of the launch, set iff a tile of any field was marked.
__global__ __launch_bounds__(kNavThreads) void k_navset_relax(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table, NavArgs a,
                                                              uint32_t inner_cap, uint32_t all_tiles, uint32_t n_tiles, uint32_t *fields,
                                                              uint32_t *marks_cur, uint32_t *marks_nxt, uint32_t *flag)
{
    const size_t z = blockIdx.z;
    nav_relax_tile(plane, table, a, inner_cap, all_tiles, fields + z * a.width * a.height, marks_cur + z * n_tiles, marks_nxt + z * n_tiles,
                   flag);
}

// cells_blocked and cells_invalid depend on the plane alone: counted once, gridDim.x workgroups striding over the cells,
// the counts in registers, one pair of atomics per workgroup.
__global__ __launch_bounds__(kNavThreads) void k_navset_plane_count(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table,
                                                                    uint32_t n_cells, uint32_t *plane_words)
{
    __shared__ uint32_t s_sum[4];
    uint32_t blocked = 0u, invalid = 0u;
    for (uint32_t i = blockIdx.x * kNavThreads + threadIdx.x; i < n_cells; i += gridDim.x * kNavThreads) {
        const int b = plane[i];
        blocked += table[(uint8_t)b] == 0u ? 1u : 0u;
        invalid += b < -1 || b > 100 ? 1u : 0u;
    }
    blocked = navset_group_sum(blocked, s_sum);
    invalid = navset_group_sum(invalid, s_sum);
    if (threadIdx.x == 0u) {
        if (blocked) atomicAdd(plane_words + NSP_BLOCKED, blocked);
        if (invalid) atomicAdd(plane_words + NSP_INVALID, invalid);
    }
}

// Step 5 of field blockIdx.y at the fixed point: gridDim.x workgroups stride over its cells, keep cells_reached, the
// greatest P and range_exceeded (k_nav_report's rule) in registers, reduce by wave and workgroup, and issue one set of
// atomics per workgroup.
__global__ __launch_bounds__(kNavThreads) void k_navset_report(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table,
                                                               const uint32_t *__restrict__ fields, NavArgs a, uint32_t *words)
{
    __shared__ uint32_t s_sum[4];
    __shared__ uint32_t s_max, s_range;
    if (threadIdx.x == 0u) s_max = s_range = 0u;
    const uint32_t n_cells = a.width * a.height;
    const uint32_t *const field = fields + (size_t)blockIdx.y * n_cells;
    uint32_t reached = 0u, pmax = 0u, exceeded = 0u;
    for (uint32_t i = blockIdx.x * kNavThreads + threadIdx.x; i < n_cells; i += gridDim.x * kNavThreads) {
        const uint32_t p = field[i];
        if (p == kNavUnreached) continue;
        reached++;
        pmax = max(pmax, p);
        if (p > kNavMax - 7u * kNavMaxCellCost) {
            const int x = (int)(i % a.width), y = (int)(i / a.width);
            for (uint32_t d = 0; d < 8u; d++) {
                if (!nav_step_allowed(plane, table, a.width, a.height, x, y, d)) continue;
                const uint32_t ca = nav_cost_at(plane, table, a.width, a.height, x + nav_dx(d), y + nav_dy(d));
                exceeded |= p > kNavMax - nav_len(d) * ca ? 1u : 0u;
            }
        }
    }
    reached = navset_group_sum(reached, s_sum);  // (its first barrier is behind lane 0's stores above)
    for (uint32_t o = 32u; o; o >>= 1) pmax = max(pmax, (uint32_t)__shfl_xor((int)pmax, (int)o));
    const bool any_exceeded = __ballot(exceeded != 0u) != 0ull;
    if ((threadIdx.x & 63u) == 0u) {
        if (pmax) atomicMax(&s_max, pmax);
        if (any_exceeded) atomicOr(&s_range, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t *const w = words + (size_t)blockIdx.y * NSW_FIELD_COUNT;
        if (reached) atomicAdd(w + NSW_REACHED, reached);
        if (s_max) atomicMax(w + NSW_MAX_POTENTIAL, s_max);
        if (s_range) atomicOr(w + NSW_RANGE, 1u);
    }
}

// A lane per (field blockIdx.y, point): P of the field at the point's cell (cells; (-1, -1) where a point in metres is
// outside), unreached outside the grid.  out: [n_fields][n].
__global__ __launch_bounds__(kNavThreads) void k_navset_gather(const uint32_t *__restrict__ fields, NavArgs a,
                                                               const int32_t *__restrict__ points, uint32_t n, uint32_t *out)
{
    const uint32_t j = blockIdx.x * kNavThreads + threadIdx.x;
    if (j >= n) return;
    const int x = points[2 * (size_t)j], y = points[2 * (size_t)j + 1];
    uint32_t p = kNavUnreached;
    if (x >= 0 && y >= 0 && x < (int)a.width && y < (int)a.height)
        p = fields[(size_t)blockIdx.y * a.width * a.height + (size_t)y * a.width + (uint32_t)x];
    out[(size_t)blockIdx.y * n + j] = p;
}

// A lane per cell over the fields: the least P and the least index that attains it; owner kNavSetNoOwner where no field
// reaches the cell.  owner_out, potential_out and owned (u64 per field, zeroed) may each be NULL.  cells_owned: a wave
// peels its owners off by ballot, one count per distinct owner; the counts gather per workgroup in kNavSetOwnerSlots words
// of LDS keyed by owner % slots (an owner that finds its slot taken by another goes to HBM at once), and the workgroup
// issues one atomic per used slot at its end.
__global__ __launch_bounds__(kNavThreads) void k_navset_nearest(const uint32_t *__restrict__ fields, uint32_t n_cells, uint32_t n_fields,
                                                                uint16_t *owner_out, uint32_t *potential_out, unsigned long long *owned)
{
    __shared__ uint32_t s_tag[kNavSetOwnerSlots], s_count[kNavSetOwnerSlots];
    if (threadIdx.x < kNavSetOwnerSlots) s_tag[threadIdx.x] = kNavSetNoOwner, s_count[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    // (every lane of a wave runs the same number of rounds: the ballots below need them all)
    const uint32_t rounds = (n_cells + gridDim.x * kNavThreads - 1u) / (gridDim.x * kNavThreads);
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t i = (r * gridDim.x + blockIdx.x) * kNavThreads + threadIdx.x;
        uint32_t best = kNavUnreached, owner = kNavSetNoOwner;
        if (i < n_cells) {
            for (uint32_t z = 0; z < n_fields; z++) {
                const uint32_t p = fields[(size_t)z * n_cells + i];
                if (p < best) best = p, owner = z;
            }
            if (owner_out) owner_out[i] = (uint16_t)owner;
            if (potential_out) potential_out[i] = best;
        }
        if (!owned) continue;
        unsigned long long left = __ballot(owner != kNavSetNoOwner);
        while (left) {
            const uint32_t first = (uint32_t)__ffsll((long long)left) - 1u;
            const uint32_t who = (uint32_t)__shfl((int)owner, (int)first);
            const unsigned long long same = __ballot(owner == who) & left;
            if (lane == first) {
                const uint32_t count = (uint32_t)__popcll(same), slot = who % kNavSetOwnerSlots;
                const uint32_t tag = atomicCAS(&s_tag[slot], kNavSetNoOwner, who);
                if (tag == kNavSetNoOwner || tag == who)
                    atomicAdd(&s_count[slot], count);
                else
                    atomicAdd(owned + who, (unsigned long long)count);
            }
            left &= ~same;
        }
    }
    if (!owned) return;
    __syncthreads();
    if (threadIdx.x < kNavSetOwnerSlots && s_count[threadIdx.x]) atomicAdd(owned + s_tag[threadIdx.x], (unsigned long long)s_count[threadIdx.x]);
}

// Step 6 on a named field, a lane per start: nav_walk down field field_of[k] (validated on the host).
__global__ __launch_bounds__(kNavThreads) void k_navset_trace(const int8_t *__restrict__ plane, const uint32_t *__restrict__ table,
                                                              const uint32_t *__restrict__ fields, NavArgs a,
                                                              const int32_t *__restrict__ starts, const int32_t *__restrict__ field_of,
                                                              uint32_t K, uint32_t cap, uint16_t *out, uint32_t *lengths)
{
    const uint32_t k = blockIdx.x * kNavThreads + threadIdx.x;
    if (k >= K) return;
    const uint32_t *const field = fields + (size_t)(uint32_t)field_of[k] * a.width * a.height;
    lengths[k] = nav_walk(plane, table, field, a, starts[2 * (size_t)k], starts[2 * (size_t)k + 1], cap, out + (size_t)k * cap * 2u);
}

}  // namespace lom
