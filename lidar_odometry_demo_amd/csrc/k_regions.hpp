// Region grid (include/lidar_odometry_amd.h, "frontier regions"): k_reg_mask, k_reg_label_tile, k_reg_merge, k_reg_flatten,
// k_reg_scan_partial, k_reg_scan_top, k_reg_number, k_reg_accumulate, k_reg_centroid, k_reg_centre, k_reg_record and
// k_reg_query.  Device code only; regions.hip is the one translation unit that instantiates and launches it.  Integers
// throughout; plain vector stores and vector atomics only; no workgroup ever waits for another: what one launch needs
// from all workgroups of another is a launch of its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lom {

constexpr uint32_t kRegThreads = 256;          // four waves
constexpr uint32_t kRegTileCols = 64;          // a tile is one bitmap word wide ...
constexpr uint32_t kRegTileRowsMax = 32;       // ... and at most 32 rows high
constexpr uint32_t kRegAccRows = 16;           // rows a wave of k_reg_accumulate and k_reg_centre walks down
constexpr uint32_t kRegScanWords = 1024;       // bitmap words per workgroup of k_reg_scan_partial: four per lane
constexpr uint32_t kRegNone = 0xFFFFFFFFu;     // LOM_REGIONS_NONE
constexpr uint32_t kRegUnreached = 0xFFFFFFFFu;
constexpr uint32_t kRegIndexBits = 26;         // a linear index
constexpr unsigned long long kRegNoKey = ~0ull;

// the summary words of an extract (zeroed per extract)
enum { RW_MEMBER = 0, RW_REGIONS = 1, RW_LISTED = 2, RW_LARGEST = 3, RW_COUNT = 4 };

struct RegArgs {
    uint32_t width, height;
    uint32_t words_per_row;  // of the row-aligned bitmaps
};

// What the accumulating kernels keep per recorded region, 64 bytes; k_reg_record packs it into a lom_regions_record.
struct RegAcc {
    uint32_t label, cells;
    unsigned long long sum_x, sum_y;
    uint32_t min_x, min_y, max_x, max_y;
    unsigned long long key_centre, key_entry;  // (d^2 << 26) | index, (P << 26) | index
    uint32_t cx, cy;
};
static_assert(sizeof(RegAcc) == 64, "RegAcc is 64 bytes");

// the record as the header lays it out (lom_regions_record), written field by field
struct RegRecord {
    uint32_t label, cells;
    unsigned long long sum_x, sum_y;
    uint16_t min_x, min_y, max_x, max_y, centroid_x, centroid_y, centre_x, centre_y, entry_x, entry_y;
    uint32_t entry_potential;
};
static_assert(sizeof(RegRecord) == 48, "RegRecord is 48 bytes");

// Which of the three cells above a member need a link of their own, a bit each (1: above left, 2: above, 4: above
// right), given the members around it: cl, cr its left and right neighbours, ul, um, ur the three above.  Members that
// are neighbours in a row are linked already (a run), so a link is left out where a link between the same two runs is
// made elsewhere: the one straight up where the pair to the left is a pair of members too (going left, the first pair of
// the two runs' overlap is linked); a diagonal one where the cell straight up, or the neighbour under the diagonal cell,
// is a member (that pair links the same runs).  Under 4-connectivity there are no diagonal links.
__device__ __forceinline__ uint32_t reg_up_links(bool cl, bool cr, bool ul, bool um, bool ur, bool conn4)
{
    uint32_t m = (um && !(cl && ul)) ? 2u : 0u;
    if (!conn4) m |= ((ul && !um && !cl) ? 1u : 0u) | ((ur && !um && !cr) ? 4u : 0u);
    return m;
}

// ---- the union-find words ---------------------------------------------------------------------------------------------
// L[i] of a member is the index of a member of i's component that is not above i; a root has L[i] == i.  The chain from
// any cell falls strictly, so it ends, at a root.
template <typename T>
__device__ __forceinline__ uint32_t reg_find(const T *L, uint32_t i)
{
    for (;;) {
        const uint32_t p = L[i];
        if (p == i) return i;
        i = p;
    }
}

// The same walk on the words in HBM, halving the path as it goes: a cell whose parent is no root is lowered to its
// grandparent -- a member of its component below it, by an atomic minimum, so the three properties below k_reg_merge
// hold -- and the walk goes on from there.  Long chains (a full row linked cell by cell without the tile pass) shrink
// with every walk over them.
__device__ __forceinline__ uint32_t reg_find_halving(uint32_t *L, uint32_t i)
{
    for (;;) {
        const uint32_t p = L[i];
        if (p == i) return i;
        const uint32_t g = L[p];
        if (g == p) return p;
        atomicMin(L + i, g);
        i = g;
    }
}

// The lock-free union of the components of a and b (LDS words, or with kHalve the words in HBM): find both roots; if they
// differ, lower the larger root's word to the smaller root with an atomic minimum; if that word was no root any more --
// another lane linked it first, to the value returned -- go on from there.
template <bool kHalve, typename T>
__device__ __forceinline__ void reg_unite(T *L, uint32_t a, uint32_t b)
{
    for (;;) {
        if constexpr (kHalve) {
            a = reg_find_halving(L, a), b = reg_find_halving(L, b);
        } else {
            a = reg_find(L, a), b = reg_find(L, b);
        }
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b, b = t;
        }
        const uint32_t old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

// Step 1, a lane per cell of a row (y = blockIdx.y), a wave per 64 aligned cells: membership, the wave's ballot as one
// word of the row-aligned bitmap, and L[i] = i for a member, LOM_REGIONS_NONE for every other cell.
__global__ __launch_bounds__(kRegThreads) void k_reg_mask(const int8_t *__restrict__ plane, const int8_t *__restrict__ cost,
                                                          const uint32_t *__restrict__ potential, RegArgs a, int kind, int lo, int hi,
                                                          int max_cost, uint32_t flags, unsigned long long *bitmap, uint32_t *L)
{
    const uint32_t x = blockIdx.x * kRegThreads + threadIdx.x, y = blockIdx.y;
    const bool have = x < a.width;
    const size_t i = (size_t)y * a.width + x;
    bool member = false;
    if (have) {
        const int v = plane[i];
        if (kind == 0) {
            member = v >= lo && v <= hi;
        } else if (v == 0) {
            const bool edge = (flags & 2u) != 0u, all8 = (flags & 1u) != 0u;
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    if ((dx == 0 && dy == 0) || (!all8 && dx != 0 && dy != 0)) continue;
                    const int nx = (int)x + dx, ny = (int)y + dy;
                    const bool inside = nx >= 0 && ny >= 0 && nx < (int)a.width && ny < (int)a.height;
                    member = member || (inside ? plane[(size_t)ny * a.width + (uint32_t)nx] == -1 : edge);
                }
        }
        if (member && cost) {
            const int c = cost[i];
            member = c >= 0 && c <= max_cost;
        }
        if (member && potential) member = potential[i] != kRegUnreached;
        L[i] = member ? (uint32_t)i : kRegNone;
    }
    const unsigned long long bits = __ballot(member);
    const uint32_t word = x >> 6;
    if ((threadIdx.x & 63u) == 0u && word < a.words_per_row) bitmap[(size_t)y * a.words_per_row + word] = bits;
}

// Step 2 inside a tile: a workgroup per tile of 64 columns by `rows` rows (1, 8 or 32), its bitmap words in LDS.  A
// member starts under the first cell of its run (count-leading-zeros on the row's word), so the runs of a row are
// flat from the start; then overlapping runs of adjacent rows are united (reg_up_links: one link per pair of runs where
// the bits show it) by the lock-free loop on LDS words, always the larger index under the smaller.  Behind a barrier every
// member reads its root and writes the root's global linear index.  Local and global indices order alike inside a tile,
// so the least local index is the least global one.
__global__ __launch_bounds__(kRegThreads) void k_reg_label_tile(const unsigned long long *__restrict__ bitmap, RegArgs a, uint32_t rows,
                                                                uint32_t conn4, uint32_t *L)
{
    __shared__ unsigned long long s_bits[kRegTileRowsMax];
    __shared__ uint32_t s_par[kRegTileRowsMax * kRegTileCols];
    const uint32_t t = threadIdx.x, y0 = blockIdx.y * rows, x0 = blockIdx.x * kRegTileCols;
    if (t < kRegTileRowsMax) s_bits[t] = (t < rows && y0 + t < a.height) ? bitmap[(size_t)(y0 + t) * a.words_per_row + blockIdx.x] : 0ull;
    __syncthreads();
    const uint32_t n = rows * kRegTileCols;
    for (uint32_t c = t; c < n; c += kRegThreads) {
        const uint32_t ly = c >> 6, lx = c & 63u;
        const unsigned long long cur = s_bits[ly];
        if (!(cur >> lx & 1ull)) continue;
        const unsigned long long gaps = ~cur & ((1ull << lx) - 1ull);  // the cells left of lx that are no members
        s_par[c] = ly * kRegTileCols + (gaps ? 64u - (uint32_t)__clzll((long long)gaps) : 0u);
    }
    __syncthreads();
    for (uint32_t c = t + kRegTileCols; c < n; c += kRegThreads) {  // (row 0 has no row above it in the tile)
        const uint32_t ly = c >> 6, lx = c & 63u;
        const unsigned long long cur = s_bits[ly], up = s_bits[ly - 1u];
        if (!(cur >> lx & 1ull)) continue;
        const bool l = lx > 0u, r = lx < 63u;
        const uint32_t links = reg_up_links(l && (cur >> (lx - 1u) & 1ull), r && (cur >> (lx + 1u) & 1ull), l && (up >> (lx - 1u) & 1ull),
                                            (up >> lx & 1ull) != 0ull, r && (up >> (lx + 1u) & 1ull), conn4 != 0u);
        if (links & 1u) reg_unite<false>(s_par, c, c - kRegTileCols - 1u);
        if (links & 2u) reg_unite<false>(s_par, c, c - kRegTileCols);
        if (links & 4u) reg_unite<false>(s_par, c, c - kRegTileCols + 1u);
    }
    __syncthreads();
    for (uint32_t c = t; c < n; c += kRegThreads) {
        const uint32_t ly = c >> 6, lx = c & 63u;
        if (!(s_bits[ly] >> lx & 1ull)) continue;
        const uint32_t root = reg_find(s_par, c);
        L[(size_t)(y0 + ly) * a.width + x0 + lx] = (y0 + (root >> 6)) * a.width + x0 + (root & 63u);
    }
}

__device__ __forceinline__ bool reg_member_at(const uint32_t *L, RegArgs a, int x, int y)
{
    return x >= 0 && y >= 0 && x < (int)a.width && y < (int)a.height && L[(size_t)y * a.width + (uint32_t)x] != kRegNone;
}

// Step 2 across tiles: the adjacencies the tile pass did not see, united in HBM by the same lock-free loop.  Tiles are
// tile_cols x tile_rows cells (1 x 1 without the tile pass: then every adjacency comes through here).  The first
// row_lanes lanes stand on the first row of a tile row, a lane per cell, and link the member there to the three cells
// above it (reg_up_links decides which links the neighbouring lanes make anyway); the other lanes stand on the first
// column of a tile column, a lane per cell, and link the member there to its left neighbour and, by the same rule, the
// two diagonal pairs that cross the border there.  A pair may be united twice; that changes nothing.
//
// Why any schedule gives the same words.  Three things hold for every member i at every moment: L[i] <= i; L[i] lies
// in i's component -- a word only ever takes the value of a root found from a cell that an adjacency joins to it; and
// L[i] only falls -- the one write is an atomic minimum.  So chains fall strictly and end, a find may read a word late or
// stale (in a cache of its own compute unit) and still walks up real ancestors, and an atomic minimum on a word that has
// meanwhile stopped being a root returns what it became, from where the loop goes on: no link is lost.  A union returns
// only once both cells hang under one root.  After the launch all adjacent members share a root, so a component has
// exactly one root, and as a root is the least word of its chain in the component, it is the component's least index --
// whatever order the lanes ran in.  Every lane's loop ends: each pass either returns or moves to a strictly smaller
// root.
__global__ __launch_bounds__(kRegThreads) void k_reg_merge(RegArgs a, uint32_t tile_cols, uint32_t tile_rows, uint32_t row_lanes,
                                                           uint32_t col_lanes, uint32_t conn4, uint32_t *L)
{
    const uint32_t j = blockIdx.x * kRegThreads + threadIdx.x;
    if (j < row_lanes) {
        const int x = (int)(j % a.width), y = (int)((j / a.width + 1u) * tile_rows);
        if (!reg_member_at(L, a, x, y)) return;
        const uint32_t i = (uint32_t)y * a.width + (uint32_t)x;
        const uint32_t links = reg_up_links(reg_member_at(L, a, x - 1, y), reg_member_at(L, a, x + 1, y), reg_member_at(L, a, x - 1, y - 1),
                                            reg_member_at(L, a, x, y - 1), reg_member_at(L, a, x + 1, y - 1), conn4 != 0u);
        if (links & 1u) reg_unite<true>(L, i, i - a.width - 1u);
        if (links & 2u) reg_unite<true>(L, i, i - a.width);
        if (links & 4u) reg_unite<true>(L, i, i - a.width + 1u);
    } else if (j - row_lanes < col_lanes) {
        const uint32_t k = j - row_lanes;
        const int y = (int)(k % a.height), x = (int)((k / a.height + 1u) * tile_cols);
        const uint32_t i = (uint32_t)y * a.width + (uint32_t)x;
        const bool me = reg_member_at(L, a, x, y), left = reg_member_at(L, a, x - 1, y);
        if (me && left) reg_unite<true>(L, i, i - 1u);
        if (conn4 || y == 0) return;
        const bool up = reg_member_at(L, a, x, y - 1), up_left = reg_member_at(L, a, x - 1, y - 1);
        // (x, y) with the cell above left; (x - 1, y) with the cell above right: reg_up_links' diagonal rule
        if (me && up_left && !up && !left) reg_unite<true>(L, i, i - a.width - 1u);
        if (left && up && !up_left && !me) reg_unite<true>(L, i - 1u, i - a.width);
    }
}

// A launch of its own behind the merge, the shape of k_reg_mask: every member's word becomes its root, the roots' ballot
// a word of the root bitmap.  A lane that reads a word another lane has already flattened reads an ancestor all the
// same, and roots do not change here.  (The members are counted in k_reg_scan_partial, from the bitmap: an atomic per
// wave on one word here took 3 ms of a 4096 x 4096 extract.)
__global__ __launch_bounds__(kRegThreads) void k_reg_flatten(RegArgs a, uint32_t *L, unsigned long long *rootbits)
{
    const uint32_t x = blockIdx.x * kRegThreads + threadIdx.x, y = blockIdx.y;
    const uint32_t i = y * a.width + x;
    bool root = false;
    if (x < a.width && L[i] != kRegNone) {
        const uint32_t r = reg_find_halving(L, i);
        root = r == i;
        if (!root) L[i] = r;
    }
    const unsigned long long roots = __ballot(root);
    const uint32_t word = x >> 6;
    if ((threadIdx.x & 63u) == 0u && word < a.words_per_row) rootbits[(size_t)y * a.words_per_row + word] = roots;
}

// Step 3, first launch: a workgroup per 1024 words of the root bitmap, four per lane.  prefix[w]: the roots in the
// workgroup's words before w; block_sums[b]: the roots in all of workgroup b's words.  The members are counted on the
// way, from the same words of the member bitmap: one addition per wave.
__global__ __launch_bounds__(kRegThreads) void k_reg_scan_partial(const unsigned long long *__restrict__ rootbits,
                                                                  const unsigned long long *__restrict__ bitmap, uint32_t n_words,
                                                                  uint32_t *prefix, uint32_t *block_sums, uint32_t *words)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t t = threadIdx.x, w0 = (blockIdx.x * kRegThreads + t) * 4u;
    uint32_t c[4], sum = 0u, members = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        c[k] = w0 + k < n_words ? (uint32_t)__popcll(rootbits[w0 + k]) : 0u;
        members += w0 + k < n_words ? (uint32_t)__popcll(bitmap[w0 + k]) : 0u;
        sum += c[k];
    }
    for (uint32_t o = 32u; o; o >>= 1) members += (uint32_t)__shfl_xor((int)members, (int)o);
    if ((t & 63u) == 0u && members) atomicAdd(words + RW_MEMBER, members);
    uint32_t incl = sum;  // the inclusive scan of a wave
    for (uint32_t o = 1u; o < 64u; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
        if ((t & 63u) >= o) incl += v;
    }
    if ((t & 63u) == 63u) s_wave[t >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - sum;
    for (uint32_t v = 0; v < (t >> 6); v++) before += s_wave[v];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        if (w0 + k < n_words) prefix[w0 + k] = before;
        before += c[k];
    }
    if (t == kRegThreads - 1u) block_sums[blockIdx.x] = before;
}

// Step 3, second launch, one workgroup: block_sums (at most 1024 of them) becomes its exclusive scan in place, and the
// total is the number of regions.
__global__ __launch_bounds__(kRegThreads) void k_reg_scan_top(uint32_t n_blocks, uint32_t *block_sums, uint32_t *words)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t t = threadIdx.x;
    uint32_t c[4], sum = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        c[k] = t * 4u + k < n_blocks ? block_sums[t * 4u + k] : 0u;
        sum += c[k];
    }
    uint32_t incl = sum;
    for (uint32_t o = 1u; o < 64u; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
        if ((t & 63u) >= o) incl += v;
    }
    if ((t & 63u) == 63u) s_wave[t >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - sum;
    for (uint32_t v = 0; v < (t >> 6); v++) before += s_wave[v];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        if (t * 4u + k < n_blocks) block_sums[t * 4u + k] = before;
        before += c[k];
    }
    if (t == kRegThreads - 1u) words[RW_REGIONS] = before;
}

// Step 3, third launch, the shape of k_reg_mask: a root's number is the count of root bits before its own.  The root
// writes it to number[i] (the members of its region read it from there) and, if it gets a record, starts the record.
__global__ __launch_bounds__(kRegThreads) void k_reg_number(RegArgs a, const unsigned long long *__restrict__ rootbits,
                                                            const uint32_t *__restrict__ prefix, const uint32_t *__restrict__ block_sums,
                                                            uint32_t cap, uint32_t *number, RegAcc *acc)
{
    const uint32_t x = blockIdx.x * kRegThreads + threadIdx.x, y = blockIdx.y, word = x >> 6;
    if (x >= a.width) return;
    const uint32_t w = y * a.words_per_row + word;
    const unsigned long long bits = rootbits[w];
    if (!(bits >> (x & 63u) & 1ull)) return;
    const uint32_t r = block_sums[w / kRegScanWords] + prefix[w] + (uint32_t)__popcll(bits & ((1ull << (x & 63u)) - 1ull));
    const uint32_t i = y * a.width + x;
    number[i] = r;
    if (r < cap) acc[r] = RegAcc{i, 0u, 0ull, 0ull, kRegNone, kRegNone, 0u, 0u, kRegNoKey, kRegNoKey, 0u, 0u};
}

// the sum of the positions of the set bits of m
__device__ __forceinline__ uint32_t reg_position_sum(unsigned long long m)
{
    return (uint32_t)__popcll(m & 0xAAAAAAAAAAAAAAAAull) + 2u * (uint32_t)__popcll(m & 0xCCCCCCCCCCCCCCCCull) +
           4u * (uint32_t)__popcll(m & 0xF0F0F0F0F0F0F0F0ull) + 8u * (uint32_t)__popcll(m & 0xFF00FF00FF00FF00ull) +
           16u * (uint32_t)__popcll(m & 0xFFFF0000FFFF0000ull) + 32u * (uint32_t)__popcll(m & 0xFFFFFFFF00000000ull);
}

// what a wave carries for the region it is in, the same in every lane
struct RegCarry {
    uint32_t r = kRegNone, n = 0u, min_x = kRegNone, min_y = kRegNone, max_x = 0u, max_y = 0u;
    unsigned long long sum_x = 0ull, sum_y = 0ull;
};

// The sums of a group go to the region's record: three additions, two minima, two maxima.  With `filter` a minimum or
// maximum is issued only where the record does not hold as good a bound already (the words only fall, or only rise, so
// a bound read late is still one): that spares the hot record most of them, at the price of waiting for four loads, so
// it is for what a wave carried down its band, not for the small groups issued row by row.
__device__ __forceinline__ void reg_flush(RegAcc *acc, RegCarry &c, bool issuer, bool filter)
{
    if (c.r != kRegNone && issuer) {
        RegAcc *const g = acc + c.r;
        atomicAdd(&g->cells, c.n), atomicAdd(&g->sum_x, c.sum_x), atomicAdd(&g->sum_y, c.sum_y);
        if (!filter || c.min_x < g->min_x) atomicMin(&g->min_x, c.min_x);
        if (!filter || c.min_y < g->min_y) atomicMin(&g->min_y, c.min_y);
        if (!filter || c.max_x > g->max_x) atomicMax(&g->max_x, c.max_x);
        if (!filter || c.max_y > g->max_y) atomicMax(&g->max_y, c.max_y);
    }
    c = RegCarry{};
}

// Step 4, counts and sums: a wave holds 64 aligned cells of a row and walks down kRegAccRows rows (blockIdx.y names the
// band).  The lanes of a wave that share a label are merged before the atomics on the region's record: their ballot
// gives the count, the least and the greatest x and the sum of x by bit operations, and y is the row's.  The wave carries
// these for one label down its band -- the first it meets while it carries none -- and issues them when a row comes
// without that label and at the end, so one large region, the hot record, gets one set of atomics per wave and band;
// the groups of other labels are issued row by row.  wave_merge == 0 (a test switch): every member lane issues its
// own.  Integer sums, minima and maxima do not depend on the order.
__global__ __launch_bounds__(kRegThreads) void k_reg_accumulate(RegArgs a, const uint32_t *__restrict__ L, const uint32_t *__restrict__ number,
                                                                uint32_t cap, uint32_t wave_merge, RegAcc *acc)
{
    const uint32_t x = blockIdx.x * kRegThreads + threadIdx.x, lane = threadIdx.x & 63u, xb = x - lane;
    const uint32_t y0 = blockIdx.y * kRegAccRows, y1 = min(y0 + kRegAccRows, a.height);
    RegCarry c;
    uint32_t c_label = kRegNone;
    for (uint32_t y = y0; y < y1; y++) {
        uint32_t label = kRegNone, r = kRegNone;
        if (x < a.width) {
            label = L[y * a.width + x];
            if (label != kRegNone) r = number[label];
        }
        const bool counted = r < cap;  // (kRegNone is not)
        if (!wave_merge) {
            if (counted) {
                RegAcc *const g = acc + r;
                atomicAdd(&g->cells, 1u), atomicAdd(&g->sum_x, (unsigned long long)x), atomicAdd(&g->sum_y, (unsigned long long)y);
                atomicMin(&g->min_x, x), atomicMin(&g->min_y, y), atomicMax(&g->max_x, x), atomicMax(&g->max_y, y);
            }
            continue;
        }
        unsigned long long todo = __ballot(counted);
        bool met = false;  // the carried label is in this row
        while (todo) {     // (wave-uniform)
            const int first = __ffsll((long long)todo) - 1;
            const uint32_t lab = (uint32_t)__shfl((int)label, first), rr = (uint32_t)__shfl((int)r, first);
            const unsigned long long m = __ballot(counted && label == lab);
            const uint32_t n = (uint32_t)__popcll(m);
            RegCarry g;
            g.r = rr, g.n = n, g.sum_x = (unsigned long long)n * xb + reg_position_sum(m), g.sum_y = (unsigned long long)n * y;
            g.min_x = xb + (uint32_t)__ffsll((long long)m) - 1u, g.max_x = xb + 63u - (uint32_t)__clzll((long long)m);
            g.min_y = g.max_y = y;
            if (c_label == kRegNone) c_label = lab, c.r = rr;
            if (lab == c_label) {
                met = true;
                c.n += g.n, c.sum_x += g.sum_x, c.sum_y += g.sum_y;
                c.min_x = min(c.min_x, g.min_x), c.max_x = max(c.max_x, g.max_x), c.min_y = min(c.min_y, y), c.max_y = max(c.max_y, y);
            } else {
                reg_flush(acc, g, (int)lane == first, false);
            }
            todo &= ~m;
        }
        if (!met && c_label != kRegNone) {
            reg_flush(acc, c, lane == 0u, true);
            c_label = kRegNone;
        }
    }
    reg_flush(acc, c, lane == 0u, true);
}

// Step 4, the centroid cell, a lane per recorded region: floor((2 sum + cells) / (2 cells)) per axis.
__global__ __launch_bounds__(kRegThreads) void k_reg_centroid(const uint32_t *__restrict__ words, uint32_t cap, RegAcc *acc)
{
    const uint32_t r = blockIdx.x * kRegThreads + threadIdx.x;
    if (r >= min(words[RW_REGIONS], cap)) return;
    RegAcc *const g = acc + r;
    const unsigned long long n = g->cells;  // >= 1: the root is a member
    g->cx = (uint32_t)((2ull * g->sum_x + n) / (2ull * n)), g->cy = (uint32_t)((2ull * g->sum_y + n) / (2ull * n));
}

// the least of a wave's 64-bit values, in every lane
__device__ __forceinline__ unsigned long long reg_wave_min(unsigned long long v)
{
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
        const unsigned long long other = (unsigned long long)hi << 32 | lo;
        v = other < v ? other : v;
    }
    return v;
}

// Step 4, the centre and the entry cell: a second pass once the centroids exist, the bands of k_reg_accumulate.  Each is
// one unsigned 64-bit minimum of (key << 26) | linear index, the key d^2 to the centroid cell (below 2^27) or P (below
// 2^32).  Where all members of a wave's row share a label the wave takes its minimum first and carries it down the band
// while the label stays; one lane issues the atomics when it changes and at the end.  Else, and with wave_merge == 0,
// every member lane issues its own.  A key that is not below what the record already holds skips the atomic: keys are
// distinct and the word only falls, so such a key cannot be the minimum.
__global__ __launch_bounds__(kRegThreads) void k_reg_centre(RegArgs a, const uint32_t *__restrict__ L, const uint32_t *__restrict__ number,
                                                            const uint32_t *__restrict__ potential, uint32_t cap, uint32_t wave_merge,
                                                            RegAcc *acc)
{
    const uint32_t x = blockIdx.x * kRegThreads + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t y0 = blockIdx.y * kRegAccRows, y1 = min(y0 + kRegAccRows, a.height);
    uint32_t c_label = kRegNone, c_r = kRegNone;  // carried, the same in every lane
    unsigned long long c_kc = kRegNoKey, c_ke = kRegNoKey;
    const auto lower = [&](uint32_t r, unsigned long long kc, unsigned long long ke) {
        RegAcc *const g = acc + r;
        if (kc < g->key_centre) atomicMin(&g->key_centre, kc);
        if (potential && ke < g->key_entry) atomicMin(&g->key_entry, ke);
    };
    const auto flush = [&]() {
        if (c_r != kRegNone && lane == 0u) lower(c_r, c_kc, c_ke);
        c_label = c_r = kRegNone, c_kc = c_ke = kRegNoKey;
    };
    for (uint32_t y = y0; y < y1; y++) {
        const uint32_t i = y * a.width + x;
        uint32_t label = kRegNone, r = kRegNone;
        if (x < a.width) {
            label = L[i];
            if (label != kRegNone) r = number[label];
        }
        const bool counted = r < cap;
        unsigned long long kc = kRegNoKey, ke = kRegNoKey;
        if (counted) {
            const int dx = (int)x - (int)acc[r].cx, dy = (int)y - (int)acc[r].cy;
            kc = (unsigned long long)(uint32_t)(dx * dx + dy * dy) << kRegIndexBits | i;
            if (potential) ke = (unsigned long long)potential[i] << kRegIndexBits | i;
        }
        const unsigned long long all = __ballot(counted);
        if (!all) continue;  // (wave-uniform)
        const int first = __ffsll((long long)all) - 1;
        const uint32_t lab = (uint32_t)__shfl((int)label, first), rr = (uint32_t)__shfl((int)r, first);
        if (wave_merge && __ballot(counted && label == lab) == all) {  // one label in the row's 64 cells
            if (lab != c_label) {
                flush();
                c_label = lab, c_r = rr;
            }
            kc = reg_wave_min(kc), ke = reg_wave_min(ke);
            c_kc = kc < c_kc ? kc : c_kc, c_ke = ke < c_ke ? ke : c_ke;
        } else {
            flush();
            if (counted) lower(r, kc, ke);
        }
    }
    flush();
}

// Step 4 and the summary, a lane per recorded region: the 48-byte record, the regions the list will hold and the largest
// count.
__global__ __launch_bounds__(kRegThreads) void k_reg_record(RegArgs a, const RegAcc *__restrict__ acc, uint32_t cap, uint32_t min_cells,
                                                            uint32_t have_potential, RegRecord *records, uint32_t *words)
{
    const uint32_t r = blockIdx.x * kRegThreads + threadIdx.x;
    bool listed = false;
    uint32_t cells = 0u;
    if (r < min(words[RW_REGIONS], cap)) {
        const RegAcc g = acc[r];
        const uint32_t centre = (uint32_t)(g.key_centre & ((1ull << kRegIndexBits) - 1ull));
        const uint32_t entry = have_potential ? (uint32_t)(g.key_entry & ((1ull << kRegIndexBits) - 1ull)) : centre;
        RegRecord o;
        o.label = g.label, o.cells = g.cells, o.sum_x = g.sum_x, o.sum_y = g.sum_y;
        o.min_x = (uint16_t)g.min_x, o.min_y = (uint16_t)g.min_y, o.max_x = (uint16_t)g.max_x, o.max_y = (uint16_t)g.max_y;
        o.centroid_x = (uint16_t)g.cx, o.centroid_y = (uint16_t)g.cy;
        o.centre_x = (uint16_t)(centre % a.width), o.centre_y = (uint16_t)(centre / a.width);
        o.entry_x = (uint16_t)(entry % a.width), o.entry_y = (uint16_t)(entry / a.width);
        o.entry_potential = have_potential ? (uint32_t)(g.key_entry >> kRegIndexBits) : kRegUnreached;
        records[r] = o;
        cells = g.cells;
        listed = cells >= min_cells;
    }
    const uint32_t n_listed = (uint32_t)__popcll(__ballot(listed));
    for (uint32_t o = 32u; o; o >>= 1) cells = max(cells, (uint32_t)__shfl_xor((int)cells, (int)o));
    if ((threadIdx.x & 63u) == 0u) {
        if (n_listed) atomicAdd(words + RW_LISTED, n_listed);
        if (cells) atomicMax(words + RW_LARGEST, cells);
    }
}

// Step 7, a lane per point: the cell by the floor rule (f64 from the f32 values, compared before any conversion) and its
// label; LOM_REGIONS_NONE outside the grid (a NaN coordinate fails both comparisons).
__global__ __launch_bounds__(kRegThreads) void k_reg_query(const float *__restrict__ xy, uint32_t n, float resolution, float origin_x,
                                                           float origin_y, RegArgs a, const uint32_t *__restrict__ L, uint32_t *out)
{
    const uint32_t i = blockIdx.x * kRegThreads + threadIdx.x;
    if (i >= n) return;
    const double r = (double)resolution;
    const double qx = __builtin_floor(((double)xy[2 * (size_t)i] - (double)origin_x) / r);
    const double qy = __builtin_floor(((double)xy[2 * (size_t)i + 1] - (double)origin_y) / r);
    uint32_t v = kRegNone;
    if (qx >= 0.0 && qx < (double)a.width && qy >= 0.0 && qy < (double)a.height) v = L[(size_t)(uint32_t)qy * a.width + (uint32_t)qx];
    out[i] = v;
}

}  // namespace lom
