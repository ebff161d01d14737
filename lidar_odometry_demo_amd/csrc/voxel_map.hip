// Device-resident voxel map: the MI355X counterpart of the reference's
// VoxelGrid container (src/voxel_grid.h:17-257) and VoxelWithPlanes payload
// (src/voxel_with_planes.h:10-36).
//
//   addCloud / addCloudWithoutNormals (:77-110)  -> lom_map_add_points[_device]
//   radiusCleanup (:236-246)                     -> lom_map_radius_cleanup
//   getCloud / getCloudWithoutNormals /
//   getSparseCloudWithoutNormals (:112-162)      -> lom_map_export
//   setVoxelSize / setMaxPoints / size (:56-66, :248-251)
//
// The reference inserts serially; a voxel keeps the first max_points points in
// call order and that order is the nearest-neighbour tie-break order.  The
// insert below is data-parallel but a pure function of the input order:
// hash slots are claimed with a 64-bit CAS (which voxel gets which slot does
// not matter), creation order comes from a prefix scan over "first point of a
// new voxel" flags, and a point's position inside its voxel is its rank among
// the batch's points of that voxel by input index -- no result depends on the
// order in which atomics land.
//
// Built with -ffp-contract=off: the f32 index and distance expressions must
// round like the reference's (plain -O3 x86-64 build, no FMA contraction).
//
// The kernels live in k_scan.hpp, k_table.hpp, k_insert.hpp, k_bulk_insert.hpp, k_cleanup.hpp, k_carve.hpp and
// k_downsample_export.hpp; this file is the one translation unit that instantiates and launches them.  Handles, scan
// contexts and options are handle.hip.  Who uses which scratch slot (scr[]) is tabulated in lom_internal.hpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "grid_scan.hpp"
#include "k_bulk_insert.hpp"
#include "k_carve.hpp"
#include "k_cleanup.hpp"
#include "k_downsample_export.hpp"
#include "k_insert.hpp"
#include "k_scan.hpp"
#include "k_table.hpp"
#include "lom_internal.hpp"
#include "pose_math.hpp"

namespace lom {

MapView view_of(const lom_map *self)
{
    const lom_map *m = self->parent ? self->parent : self;  // a scan context reads its keyframe's table and slabs
    MapView v;
    v.table = m->d_table;
    v.mask = m->cap - 1;
    v.shift = 64 - (uint32_t)__builtin_ctz(m->cap);
    v.pts = m->slabs.pts;
    v.nrm = m->slabs.nrm;
    v.K = m->K;
    v.voxel_size = m->voxel_size;
    int e = 0;
    const float inv = 1.0f / m->voxel_size;
    // power of two with a normal reciprocal: scaling by inv is exact
    v.inv_voxel_size = (std::frexp(m->voxel_size, &e) == 0.5f && std::isnormal(inv)) ? inv : 0.f;
    v.prune_slack = 1e-4f * m->voxel_size;
    return v;
}

// ---------------------------------------------------------------------------
// host-side management
// ---------------------------------------------------------------------------
static uint32_t next_pow2(uint64_t v)
{
    uint64_t p = 1024;
    while (p < v) p <<= 1;
    return (uint32_t)std::min<uint64_t>(p, 1ull << 31);
}

static int table_alloc(lom_map *m, uint32_t cap, Slot **out)
{
    Slot *t = nullptr;
    hipError_t e = hipMalloc(&t, (size_t)cap * sizeof(Slot));
    if (e != hipSuccess) return fail(m, LOM_ERR_OOM, "hipMalloc(table)", e);
    hipLaunchKernelGGL(k_table_init, dim3(blocks_for(cap)), dim3(kThreads), 0, m->stream, t, cap);
    LOM_HIP(m, hipGetLastError());
    *out = t;
    return LOM_OK;
}

// scratch words: [0..1] u64 scan total, [2] flag, [4] u32 scan total, [6] device-side voxel counter
static uint32_t *d_nvox(lom_map *m) { return m->scr[S_MISC].as<uint32_t>() + 6; }
static uint32_t *d_word(lom_map *m, int i) { return m->scr[S_MISC].as<uint32_t>() + i; }

// scratch slot `slot` grown to `count` elements of T (lom_internal.hpp: who keeps what in which slot)
template <class T>
static int scratch(lom_map *m, int slot, size_t count, T **out)
{
    const int rc = ensure(m, m->scr[slot], count * sizeof(T));
    *out = m->scr[slot].as<T>();
    return rc;
}

int read_words(lom_map *m, int first, int n);

// exact voxel count on the host (waits for pending inserts of this handle)
static int refresh_nvox(lom_map *m)
{
    int rc = resolve_pending(m);
    if (rc != LOM_OK) return rc;
    if (!m->n_vox_stale) return LOM_OK;
    rc = read_words(m, 6, 1);
    if (rc != LOM_OK) return rc;
    m->n_vox = m->h_flags[0];
    m->n_vox_ub = m->n_vox;
    m->n_vox_stale = false;
    return LOM_OK;
}

static int rehash(lom_map *m, uint32_t new_cap)
{
    m->mutations++;
    Slot *t = nullptr;
    int rc = table_alloc(m, new_cap, &t);
    if (rc != LOM_OK) return rc;
    Slot *old = m->d_table;
    m->d_table = t;
    m->cap = new_cap;
    if (m->n_vox) {
        const MapView v = view_of(m);
        hipLaunchKernelGGL(k_rebuild, dim3(blocks_for(m->n_vox)), dim3(kThreads), 0, m->stream, m->d_table,
                           v.mask, v.shift, m->slabs.key, m->slabs.count, m->n_vox);
        LOM_HIP(m, hipGetLastError());
    }
    if (old) {
        LOM_HIP(m, hipStreamSynchronize(m->stream));
        LOM_HIP(m, hipFree(old));
    }
    return LOM_OK;
}

static void slabs_free(Slabs &s)
{
    if (s.key) (void)hipFree(s.key);
    if (s.count) (void)hipFree(s.count);
    if (s.pts) (void)hipFree(s.pts);
    if (s.nrm) (void)hipFree(s.nrm);
    s = Slabs();
}

void map_free(lom_map *m)
{
    if (m->d_table) (void)hipFree(m->d_table);
    m->d_table = nullptr;
    slabs_free(m->slabs);
    slabs_free(m->alt);
}

// k_match reads a chunk of four consecutive 12-byte rows from any live row on: the rows behind the last slab exist
constexpr size_t kRowPadBytes = 64;
static int slabs_alloc(lom_map *m, uint32_t cap, Slabs &s)
{
    const size_t pb = (size_t)cap * m->K * 3 * sizeof(float);
    if (hipMalloc(&s.key, (size_t)cap * 8) != hipSuccess || hipMalloc(&s.count, (size_t)cap * 4) != hipSuccess ||
        hipMalloc(&s.pts, pb + kRowPadBytes) != hipSuccess || hipMalloc(&s.nrm, pb + kRowPadBytes) != hipSuccess) {
        (void)hipGetLastError();
        slabs_free(s);
        return fail(m, LOM_ERR_OOM, "hipMalloc(slabs)");
    }
    s.cap = cap;
    return LOM_OK;
}

static int ensure_slabs(lom_map *m, uint64_t want)
{
    if (want <= m->slabs.cap) return LOM_OK;
    if (want > 0x7FFFFFFFull / std::max<uint32_t>(1, m->K)) return fail(m, LOM_ERR_OOM, "map too large");
    uint32_t nc = std::max<uint32_t>(4096, m->slabs.cap);
    while (nc < want) nc *= 2;
    Slabs s;
    int rc = slabs_alloc(m, nc, s);
    if (rc != LOM_OK) return rc;
    const uint32_t live = std::min(std::max(m->n_vox, m->n_vox_ub), m->slabs.cap);  // upper bound of the slabs in use
    if (live) {
        const size_t pb = (size_t)live * m->K * 3 * sizeof(float);
        LOM_HIP(m, hipMemcpyAsync(s.key, m->slabs.key, (size_t)live * 8, hipMemcpyDeviceToDevice, m->stream));
        LOM_HIP(m, hipMemcpyAsync(s.count, m->slabs.count, (size_t)live * 4, hipMemcpyDeviceToDevice, m->stream));
        LOM_HIP(m, hipMemcpyAsync(s.pts, m->slabs.pts, pb, hipMemcpyDeviceToDevice, m->stream));
        LOM_HIP(m, hipMemcpyAsync(s.nrm, m->slabs.nrm, pb, hipMemcpyDeviceToDevice, m->stream));
    }
    LOM_HIP(m, hipStreamSynchronize(m->stream));
    slabs_free(m->slabs);
    m->slabs = s;
    return LOM_OK;
}

constexpr size_t kWordsOffset = 512;  // of h_report / d_report: [0, 256) AlignReport, [512, 768) these words

int gather_words_begin(lom_map *m, const uint32_t *const *ptrs, int n)
{
    m->words_pending = 0;
    if (n <= 0) return LOM_OK;
    WordPtrs w;
    for (int i = 0; i < 32; i++) w.p[i] = i < n ? ptrs[i] : nullptr;
    if (++m->words_tag == 0) m->words_tag = 1;  // the block starts zeroed: 0 is "nothing yet"
    hipLaunchKernelGGL(k_gather_words, dim3(1), dim3(64), 0, m->stream, w, n,
                       reinterpret_cast<unsigned long long *>((char *)m->d_report + kWordsOffset), m->words_tag);
    LOM_HIP(m, hipGetLastError());
    m->words_pending = n;
    return LOM_OK;
}

int gather_words_end(lom_map *m, uint32_t *out)
{
    const int n = m->words_pending;
    const uint32_t tag = m->words_tag;
    m->words_pending = 0;
    volatile unsigned long long *hw = reinterpret_cast<volatile unsigned long long *>((char *)m->h_report + kWordsOffset);
    uint64_t spins = 0;
    for (int i = 0; i < n; i++) {
        while ((uint32_t)(hw[i] >> 32) != tag) {
            __builtin_ia32_pause();
            if ((++spins & 0x3FFF) != 0) continue;
            const hipError_t e = hipStreamQuery(m->stream);
            if (e == hipSuccess) {
                if ((uint32_t)(hw[i] >> 32) == tag) break;
                return fail(m, LOM_ERR_HIP, "device words did not arrive");
            }
            if (e != hipErrorNotReady) return fail(m, LOM_ERR_HIP, "stream failed while reading device words", e);
        }
        out[i] = (uint32_t)hw[i];
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return LOM_OK;
}

int gather_words(lom_map *m, const uint32_t *const *ptrs, int n, uint32_t *out)
{
    const int rc = gather_words_begin(m, ptrs, n);
    return rc != LOM_OK ? rc : gather_words_end(m, out);
}

int read_words(lom_map *m, int first, int n)
{
    const uint32_t *ptrs[32];
    for (int i = 0; i < n; i++) ptrs[i] = d_word(m, first + i);
    return gather_words(m, ptrs, n, m->h_flags);
}

// grow-only scratch that is kept at rest (every byte == fill) between calls: a fresh allocation is
// filled once; whoever dirties a word puts it back
static int ensure_rest(lom_map *m, DeviceBuf &b, size_t bytes, int fill)
{
    if (bytes <= b.bytes) return LOM_OK;
    const int rc = ensure(m, b, bytes);
    if (rc != LOM_OK) return rc;
    LOM_HIP(m, hipMemsetAsync(b.p, fill, b.bytes, m->stream));
    return LOM_OK;
}

static Granule *d_agg(lom_map *m) { return (Granule *)(m->scr[S_MISC].as<char>() + 256); }

static int add_points_device(lom_map *m, const char *d_xyz, const char *d_nrm, size_t n, size_t stride,
                             bool validated_on_host, bool sync_status, bool allow_shrink = true, bool multi_launch = false);

// one-shot test hook (LOM_OPT_TEST_GRID_GIVE_UP): the first workgroup that gives up in the next in-kernel scan
static uint32_t take_test_fail_from(lom_map *m)
{
    const int v = m->test_grid_give_up;
    if (v >= 65536) {  // + 65536 per in-kernel scan to let pass first
        m->test_grid_give_up = v - 65536;
        return 0xFFFFFFFFu;
    }
    m->test_grid_give_up = -1;
    return v < 0 ? 0xFFFFFFFFu : (uint32_t)v;
}

// deferred verdict of the calls enqueued since the last check (waits for them): a point out of range
// (such a call inserted / returned nothing) or a workgroup that gave up waiting inside a single-pass kernel.
// A call that gave up has changed nothing (grid_scan.hpp); if it is the handle's last insert -- whose input
// buffers the caller keeps valid until this check -- it is redone here with the multi-launch scan, whose
// kernels do not wait for each other.
static int map_status(lom_map *m)
{
    // [0] range flag, [1] voxel counter, [2] grid error, [3] bulk insert sent back: sequence numbers of failed calls
    int rc = read_words(m, 5, 4);
    if (rc != LOM_OK) return rc;
    const uint32_t checked = m->status_seq;
    m->status_seq = m->call_seq;
    if (m->n_vox_stale) {
        m->n_vox = m->h_flags[1];
        m->n_vox_ub = m->n_vox;
        m->n_vox_stale = false;
    }
    const uint32_t range_seq = m->h_flags[0];
    const size_t pending = m->pending_n;
    m->pending_n = 0;  // the last single-pass / bulk insert is through, one way or the other
    // a bulk insert with a partition beyond k_bi_group's LDS wrote nothing: the four-kernel path redoes it, like a
    // single-pass insert whose scan gave up
    const uint32_t grid_seq = (pending && m->h_flags[3] == m->pending_seq) ? m->h_flags[3] : m->h_flags[2];
    if (grid_seq > checked && grid_seq != m->grid_resolved_seq) {
        if (grid_seq == m->pending_seq && pending) {
            m->grid_redos++;
            m->grid_resolved_seq = grid_seq;
            const int rc2 = add_points_device(m, m->pending_xyz, m->pending_nrm, pending, m->pending_stride, false, true, true, true);
            if (rc2 != LOM_OK) return rc2;
            if (range_seq > checked && range_seq != grid_seq)
                return fail(m, LOM_ERR_RANGE, "coordinate / voxel_size out of range or not finite");
            return LOM_OK;
        }
        return fail(m, LOM_ERR_HIP,
                         "a workgroup timed out waiting for the others of its grid; that call changed nothing, repeat it");
    }
    if (range_seq > checked) return fail(m, LOM_ERR_RANGE, "coordinate / voxel_size out of range or not finite");
    return LOM_OK;
}

// The handle's last single-pass insert has not been looked at yet (a caller that never asks for lom_map_status):
// before anything consumes or changes the map, see whether its in-kernel scan gave up, and redo it if so.
// Callers that check lom_map_status() themselves (the streaming path) never pay this read-back.
static int settle_pending_locked(lom_map *m);
int resolve_pending(lom_map *m)
{
    if (m->parent) {
        // A scan context.  The reference's calls are synchronous: an align that follows an addCloud sees its points.
        // Here the map's maintenance kernels run on the MAP's stream and a context has a stream of its own, so the
        // first call of a context after the map changed (a) settles an insert nobody has looked at yet and (b) orders
        // the context's stream behind the map's.  (Nobody changes the map while contexts are in use; several contexts
        // may arrive here together after a change, hence the lock.)
        lom_map *p = m->parent;
        if (!p->pending_n.load(std::memory_order_acquire) && m->seen_mutations == p->mutations.load(std::memory_order_acquire))
            return LOM_OK;
        std::lock_guard<std::mutex> lock(p->settle_mutex);
        if (p->pending_n) {
            const int rc = settle_pending_locked(p);
            if (rc != LOM_OK) return fail(m, rc, p->error.c_str());
        }
        const uint64_t now = p->mutations;
        if (m->seen_mutations != now) {
            if (!m->parent_ev) LOM_HIP(m, hipEventCreateWithFlags(&m->parent_ev, hipEventDisableTiming));
            LOM_HIP(m, hipEventRecord(m->parent_ev, p->stream));
            LOM_HIP(m, hipStreamWaitEvent(m->stream, m->parent_ev, 0));
            m->seen_mutations = now;
        }
        return LOM_OK;
    }
    if (!m->pending_n.load(std::memory_order_acquire)) return LOM_OK;
    // the map's own caller: contexts of this map may be settling the same insert right now
    std::lock_guard<std::mutex> lock(m->settle_mutex);
    return settle_pending_locked(m);
}

// the caller holds m->settle_mutex (m is a map, not a context)
static int settle_pending_locked(lom_map *m)
{
    if (!m->pending_n) return LOM_OK;  // somebody else settled it while this thread waited for the lock
    int rc = read_words(m, 7, 2);  // scan gave up / bulk insert sent back
    if (rc != LOM_OK) return rc;
    const size_t n = m->pending_n;
    m->pending_n = 0;
    if (m->h_flags[0] != m->pending_seq && m->h_flags[1] != m->pending_seq) return LOM_OK;
    m->grid_redos++;
    m->grid_resolved_seq = m->pending_seq;
    return add_points_device(m, m->pending_xyz, m->pending_nrm, n, m->pending_stride, false, true, true, true);
}

// lom_scan_create: a context starts from a settled keyframe.  Under the map's settle lock: the C++ mirror's worker threads
// create their contexts -- and other contexts make their first call -- together.
int settle_map(lom_map *map)
{
    std::lock_guard<std::mutex> lock(map->settle_mutex);
    const int rc = settle_pending_locked(map);
    return rc != LOM_OK ? rc : refresh_nvox(map);
}

// lom_map_create: the status words and the first table
int map_init(lom_map *m, size_t capacity_hint)
{
    m->min_cap = next_pow2(4ull * std::max<size_t>(capacity_hint, 256));
    // status / counter words (256 bytes) + the block aggregates of the single-pass kernels (256 x 2 granules)
    int rc = ensure(m, m->scr[S_MISC], 256 + 256 * 2 * sizeof(Granule));
    if (rc == LOM_OK) {
        if (hipMemsetAsync(m->scr[S_MISC].p, 0, m->scr[S_MISC].bytes, m->stream) != hipSuccess) rc = LOM_ERR_HIP;
    }
    if (rc == LOM_OK) rc = table_alloc(m, m->min_cap, &m->d_table);
    if (rc == LOM_OK) m->cap = m->min_cap;
    if (rc == LOM_OK && hipStreamSynchronize(m->stream) != hipSuccess) rc = LOM_ERR_HIP;
    return rc;
}

// Table size after a bulk insert: 16..32 slots per voxel (LOM_TABLE_SLOTS_PER_VOXEL at create).  The search's probe
// phase pays for every collision with a dependent round trip, and a longer table costs nothing but memory: k_match on
// C2 / C3 / C4 with 4 slots per voxel (rounds 1-2) 7.5 / 25.1 / 43.2 us, 8: 7.5 / 24.0 / 41.1, 16: 7.2 / 23.9 / 40.7,
// 32: 7.2 / 23.8 / 40.6, 64: 7.2 / 23.4 / 40.8 (same box, tools/ab_match.py).
static int shrink_after_bulk(lom_map *m)
{
    if ((uint64_t)m->cap < 16ull * std::max<uint32_t>(m->min_cap, 1u)) return LOM_OK;
    int rc = refresh_nvox(m);
    if (rc != LOM_OK) return rc;
    const uint32_t target = std::max(m->min_cap, next_pow2((uint64_t)m->table_slots_per_voxel * m->n_vox));
    return m->cap > target ? rehash(m, target) : LOM_OK;
}

// An insert whose verdict nobody has read yet: should its in-kernel scan have given up (single-pass) or a partition have
// been too large (bulk), lom_map_status() / whoever consumes the map next redoes it -- the caller keeps the input valid
// until then.  pending_n is what other threads read (resolve_pending's fast path): it is stored last.
static void set_pending(lom_map *m, const char *d_xyz, const char *d_nrm, size_t n, size_t stride, uint32_t seq)
{
    m->pending_xyz = d_xyz;
    m->pending_nrm = d_nrm;
    m->pending_stride = stride;
    m->pending_seq = seq;
    m->pending_n = n;
}

// the insert's kernels are enqueued: the table has keys, the voxel count is the device's to know
static void note_insert_enqueued(lom_map *m, uint64_t worst)
{
    m->table_clean = false;
    m->n_vox_ub = (uint32_t)std::min<uint64_t>(worst, 0xFFFFFFFFull);
    m->n_vox_stale = true;
}

struct BulkShape {
    uint32_t n_parts, part_shift, part_max, ppt, n_blk, n_words;
};

static BulkShape bulk_shape(uint32_t N, uint32_t cap, uint32_t ppt_override = 0)
{
    BulkShape b;
    // ~128 points per partition (the 512-point shape of k_bi_group: 20 KB of LDS, eight workgroups per CU) while the
    // partitions number at most kBiMaxParts; beyond 2 M points the partitions grow and the 1024-point shape takes over
    uint32_t np = 64;
    while (np < kBiMaxParts && (uint64_t)np * 128 < N) np <<= 1;
    b.n_parts = std::min(np, cap);
    b.part_shift = (uint32_t)__builtin_ctz(cap) - (uint32_t)__builtin_ctz(b.n_parts);
    b.part_max = (uint64_t)b.n_parts * 128 >= N ? 512u : kBiPartMax;
    b.ppt = N <= (1u << 20) ? 4u : 8u;
    if (ppt_override == 2 || ppt_override == 4 || ppt_override == 8) b.ppt = ppt_override;
    b.n_blk = (N + b.ppt * kBiThreads - 1) / (b.ppt * kBiThreads);
    b.n_words = (N + 31) / 32;
    return b;
}

static int bulk_scratch(lom_map *m, uint32_t N, const BulkShape &b)
{
    int rc;
    for (int s : {S_PT_OFF, S_PT_M, S_ENT_ROW})
        if ((rc = ensure(m, m->scr[s], (size_t)N * 4)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->scr[S_PT_SLOT], (size_t)N * sizeof(uint2))) != LOM_OK) return rc;
    if ((rc = ensure(m, m->scr[S_PT_POS], (size_t)N * sizeof(uint4))) != LOM_OK) return rc;
    if ((rc = ensure(m, m->scr[S_FLAG], (size_t)b.n_words * 4)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->scr[S_RANK], (size_t)b.n_words * 4)) != LOM_OK) return rc;
    if ((rc = ensure(m, m->scr[S_HIST], (size_t)b.n_parts * b.n_blk * 4)) != LOM_OK) return rc;
    // partition sizes and starts, then the bitmap's tiles: totals, prefixes, and the counter of finished tiles (at rest: 0)
    const size_t tiles = (b.n_words + kBiTileWords - 1) / kBiTileWords;
    const bool fresh = m->scr[S_PART].bytes < (size_t)(2 * kBiMaxParts + 1 + 2 * 256 + 1) * 4;
    if ((rc = ensure(m, m->scr[S_PART], (size_t)(2 * kBiMaxParts + 1 + 2 * 256 + 1) * 4)) != LOM_OK) return rc;
    if (fresh) LOM_HIP(m, hipMemsetAsync(m->scr[S_PART].p, 0, m->scr[S_PART].bytes, m->stream));
    return tiles <= 256 ? LOM_OK : fail(m, LOM_ERR_ARG, "bulk insert: too many points");
}

// The instantiations of the bulk insert's templated kernels (every instantiation of a family has the same signature):
// k_bi_claim / k_bi_scatter by points per thread, k_bi_group by the points a partition may hold.
struct BulkPptForm {
    uint32_t ppt;
    decltype(&k_bi_claim<2>) claim;
    decltype(&k_bi_scatter<2>) scatter;
};
static const BulkPptForm kBulkPptForms[] = {
    {2, k_bi_claim<2>, k_bi_scatter<2>}, {4, k_bi_claim<4>, k_bi_scatter<4>}, {8, k_bi_claim<8>, k_bi_scatter<8>}};

static const BulkPptForm &bulk_ppt_form(uint32_t ppt)
{
    for (const BulkPptForm &f : kBulkPptForms)
        if (f.ppt == ppt) return f;
    return kBulkPptForms[2];
}

static decltype(&k_bi_group<512>) bulk_group_kernel(uint32_t part_max)
{
    return part_max == 512 ? k_bi_group<512> : k_bi_group<kBiPartMax>;
}

// batches above kOnePassMax points (see the kernels): everything is enqueued, nothing waits; the verdict -- range error,
// or a partition beyond k_bi_group's LDS, which sends the call to the four-kernel path -- is read with the call's status
static int add_points_bulk(lom_map *m, const char *d_xyz, const char *d_nrm, uint32_t N, size_t stride, uint64_t worst,
                           bool validated_on_host, bool sync_status, bool allow_shrink)
{
    int rc;
    const BulkShape b = bulk_shape(N, m->cap, m->bulk_ppt);
    if ((rc = bulk_scratch(m, N, b)) != LOM_OK) return rc;
    if (worst > m->slabs.cap && (rc = ensure_slabs(m, worst + worst / 2)) != LOM_OK) return rc;
    uint2 *pt_info = m->scr[S_PT_SLOT].as<uint2>();
    uint32_t *flag_bits = m->scr[S_FLAG].as<uint32_t>(), *word_prefix = m->scr[S_RANK].as<uint32_t>();
    uint4 *part_rec = m->scr[S_PT_POS].as<uint4>();
    uint32_t *ent_idx = m->scr[S_PT_OFF].as<uint32_t>(), *ent_w = m->scr[S_PT_M].as<uint32_t>();
    uint32_t *ent_row = m->scr[S_ENT_ROW].as<uint32_t>();
    uint32_t *hist = m->scr[S_HIST].as<uint32_t>();
    uint32_t *part_total = m->scr[S_PART].as<uint32_t>(), *part_start = part_total + kBiMaxParts;
    uint32_t *tile_total = part_start + kBiMaxParts + 1, *tile_prefix = tile_total + 256, *tiles_done = tile_prefix + 256;
    const uint32_t n_tiles = (b.n_words + kBiTileWords - 1) / kBiTileWords;
    uint32_t *words = d_word(m, 0);
    const uint32_t seq = ++m->call_seq;
    m->mutations++;
    const MapView v = view_of(m);
    const uint32_t part_max = m->test_bulk_part_max ? std::min<uint32_t>(m->test_bulk_part_max, b.part_max) : b.part_max;
    const size_t lds = (size_t)b.n_parts * 4;
    if (lds + 256 > 65536) {  // the histograms of 16,384 partitions fill the 64 KB a launch gets without asking
        static std::once_flag once;
        std::call_once(once, [] {
            const int want = (int)kBiMaxParts * 4;
            for (const BulkPptForm &f : kBulkPptForms) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(f.claim), hipFuncAttributeMaxDynamicSharedMemorySize, want);
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(f.scatter), hipFuncAttributeMaxDynamicSharedMemorySize, want);
            }
        });
    }
    const dim3 gb(b.n_blk), tb(kBiThreads);
    const BulkPptForm &form = bulk_ppt_form(b.ppt);
    hipLaunchKernelGGL(form.claim, gb, tb, lds, m->stream, m->d_table, v.mask, v.shift, d_xyz, stride, N, m->voxel_size,
                       pt_info, flag_bits, hist, b.n_parts, b.part_shift, d_nvox(m), seq, words);
    hipLaunchKernelGGL(k_bi_colscan, dim3((b.n_parts + 63) / 64), dim3(kBiThreads), 0, m->stream, hist, b.n_parts, b.n_blk,
                       part_total, part_max, seq, words);
    hipLaunchKernelGGL(form.scatter, gb, tb, lds, m->stream, N, pt_info, hist, b.n_parts, b.part_shift, part_total,
                       part_start, part_rec, seq, words);
    hipLaunchKernelGGL(bulk_group_kernel(b.part_max), dim3(b.n_parts), dim3(kThreads), 0, m->stream, m->d_table, part_start,
                       part_rec, m->max_points, flag_bits, ent_idx, ent_w, ent_row, seq, words);
    hipLaunchKernelGGL(k_bi_flagscan, dim3(n_tiles), dim3(kThreads), 0, m->stream, flag_bits, b.n_words, word_prefix,
                       tile_total, tile_prefix, tiles_done, words + 10, seq, words);
    hipLaunchKernelGGL(k_bi_place, dim3(blocks_for(N)), dim3(kThreads), 0, m->stream, m->d_table, N, ent_idx, ent_w, ent_row,
                       flag_bits, word_prefix, tile_prefix, words + 10, d_xyz, d_nrm, stride, m->K, m->slabs.pts, m->slabs.nrm,
                       m->slabs.key, m->slabs.count, d_nvox(m), seq, words);
    LOM_HIP(m, hipGetLastError());
    set_pending(m, d_xyz, d_nrm, N, stride, seq);  // (a partition too large: redone with the four-kernel path)
    note_insert_enqueued(m, worst);
    if (sync_status && (rc = map_status(m)) != LOM_OK) return rc;
    return allow_shrink ? shrink_after_bulk(m) : LOM_OK;
}

// sync_status: wait for the insert's verdict (LOM_ERR_RANGE when a point's index is out of range; such a
// call inserts nothing).  Without it the call only enqueues; lom_map_status() reports later.
static int add_points_device(lom_map *m, const char *d_xyz, const char *d_nrm, size_t n, size_t stride,
                             bool validated_on_host, bool sync_status, bool allow_shrink, bool multi_launch)
{
    if (m->parent) return fail(m, LOM_ERR_STATE, "a scan context has no map of its own");
    if (n == 0) return LOM_OK;
    if (n >= 0x7FFFFFFFull) return fail(m, LOM_ERR_ARG, "too many points in one call");
    const uint32_t N = (uint32_t)n;
    int rc;
    if ((rc = resolve_pending(m)) != LOM_OK) return rc;  // inserts apply in call order
    // 1. table capacity for the worst case (every point a new voxel); shrunk afterwards
    uint64_t worst = (uint64_t)m->n_vox_ub + N;
    if ((uint64_t)m->cap < 2 * worst) {
        if ((rc = refresh_nvox(m)) != LOM_OK) return rc;
        worst = (uint64_t)m->n_vox + N;
        if ((uint64_t)m->cap < 2 * worst && (rc = rehash(m, next_pow2(4 * worst))) != LOM_OK) return rc;
    }
    // 2. scratch
    const bool one_pass = N <= kOnePassMax && !multi_launch;
    if (N > kOnePassMax && N <= kBiMaxPoints && !multi_launch && !m->opt_no_bulk)
        return add_points_bulk(m, d_xyz, d_nrm, N, stride, worst, validated_on_host, sync_status, allow_shrink);
    uint32_t *pt_slot, *pt_pos, *pt_off, *pt_m, *items, *boff, *bold;
    unsigned long long *flag64 = nullptr, *scan64 = nullptr, *scan_tmp = nullptr;  // the multi-launch form's
    if ((rc = scratch(m, S_PT_SLOT, N, &pt_slot)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_PT_POS, N, &pt_pos)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_PT_OFF, N, &pt_off)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_PT_M, N, &pt_m)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_ITEMS, N, &items)) != LOM_OK) return rc;
    if ((rc = ensure_rest(m, m->scr[S_BKT_CNT], (size_t)m->cap * 4, 0)) != LOM_OK) return rc;
    if ((rc = ensure_rest(m, m->scr[S_BKT_HEAD], (size_t)m->cap * 4, 0xFF)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_BKT_OFF, m->cap, &boff)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_BKT_OLD, m->cap, &bold)) != LOM_OK) return rc;
    if (!one_pass) {
        if ((rc = scratch(m, S_FLAG, N, &flag64)) != LOM_OK) return rc;
        if ((rc = scratch(m, S_RANK, N, &scan64)) != LOM_OK) return rc;
        if ((rc = scratch(m, S_SCAN, scan_tmp_words(N), &scan_tmp)) != LOM_OK) return rc;
    }
    uint32_t *bcnt = m->scr[S_BKT_CNT].as<uint32_t>(), *bhead = m->scr[S_BKT_HEAD].as<uint32_t>();
    uint32_t *words = d_word(m, 0);
    const uint32_t seq = ++m->call_seq;
    m->mutations++;
    const MapView v = view_of(m);
    const dim3 g(blocks_for(N)), b(kThreads);
    hipLaunchKernelGGL(k_ins_claim2, g, b, 0, m->stream, m->d_table, v.mask, v.shift, d_xyz, stride, N, m->voxel_size,
                       pt_slot, pt_pos, bcnt, bhead, seq, words);
    LOM_HIP(m, hipGetLastError());
    // Nothing below depends on a host decision: the slabs are grown for the worst case up front (memory is
    // not the constraint on a 288 GB device; the voxel counter lives on the device), so the call only
    // enqueues.  The exact voxel count is read back by whoever needs it (refresh_nvox).
    if (worst > m->slabs.cap && (rc = ensure_slabs(m, worst + worst / 2)) != LOM_OK) return rc;
    if (!one_pass) {
        // large batches: flags, one 64-bit scan (1-3 launches), assignment
        hipLaunchKernelGGL(k_ins_heads, g, b, 0, m->stream, m->d_table, N, pt_slot, bcnt, bhead, flag64, seq, words);
        LOM_HIP(m, hipGetLastError());
        unsigned long long *d_total64 = m->scr[S_MISC].as<unsigned long long>();
        if ((rc = scan_exclusive<unsigned long long>(m, flag64, scan64, N, d_total64, scan_tmp)) != LOM_OK) return rc;
        hipLaunchKernelGGL(k_ins_assign, g, b, 0, m->stream, m->d_table, N, pt_slot, bhead, flag64, scan64, d_nvox(m),
                           m->slabs.key, boff, bold, seq, words);
    } else {
        hipLaunchKernelGGL(k_ins_assign2, g, b, 0, m->stream, m->d_table, N, pt_slot, bcnt, bhead, boff, bold, d_nvox(m),
                           m->slabs.key, d_agg(m), seq, words, take_test_fail_from(m));
        set_pending(m, d_xyz, d_nrm, n, stride, seq);  // (its scan gave up: redone with the multi-launch scan)
    }
    hipLaunchKernelGGL(k_ins_scatter2, g, b, 0, m->stream, N, pt_slot, pt_pos, boff, bcnt, items, pt_off, pt_m, seq, words);
    hipLaunchKernelGGL(k_ins_place2, g, b, 0, m->stream, m->d_table, N, pt_slot, pt_off, pt_m, bcnt, bhead, bold, items,
                       d_xyz, d_nrm, stride, m->K, m->max_points, m->slabs.pts, m->slabs.nrm, m->slabs.count, d_nvox(m), seq, words);
    LOM_HIP(m, hipGetLastError());
    note_insert_enqueued(m, worst);
    if (sync_status && (!validated_on_host || multi_launch)) {
        if ((rc = map_status(m)) != LOM_OK) return rc;
    }
    if (allow_shrink && N > kOnePassMax && (rc = shrink_after_bulk(m)) != LOM_OK) return rc;
    return LOM_OK;
}

// pinned bounce buffer: the caller's (pageable) memory is copied once on the CPU, the H2D copy is
// then truly asynchronous and the call can return before the GPU has consumed it
static int stage_pinned(lom_map *m, size_t bytes, char **out)
{
    if (m->stage_ev) LOM_HIP(m, hipEventSynchronize(m->stage_ev));  // the previous H2D has read the buffer
    const int rc = ensure_pinned(m, m->h_stage, bytes, std::max(bytes + bytes / 2, (size_t)1 << 20), hipHostMallocDefault,
                                 "hipHostMalloc(stage)");
    if (rc != LOM_OK) return rc;
    if (!m->stage_ev) LOM_HIP(m, hipEventCreateWithFlags(&m->stage_ev, hipEventDisableTiming));
    *out = (char *)m->h_stage.h;
    return LOM_OK;
}

static int stage_host_points(lom_map *m, const float *xyz, const float *nrm, size_t n, size_t stride,
                             const char **d_xyz, const char **d_nrm)
{
    // Copy the caller's (possibly interleaved) records as they are; the kernels
    // read them with the caller's stride, so PCL structs need no repacking.
    int rc;
    const size_t bytes = (n - 1) * stride + 12;
    const char *hx = (const char *)xyz, *hn = (const char *)nrm;
    char *pin = nullptr;
    *d_nrm = nullptr;
    if (nrm && hn >= hx && (size_t)(hn - hx) + 12 <= stride) {  // normals inside the same record
        const size_t all = (n - 1) * stride + (size_t)(hn - hx) + 12;
        if ((rc = ensure(m, m->scr[S_IN_XYZ], all)) != LOM_OK) return rc;
        if ((rc = stage_pinned(m, all, &pin)) != LOM_OK) return rc;
        std::memcpy(pin, hx, all);
        LOM_HIP(m, hipMemcpyAsync(m->scr[S_IN_XYZ].p, pin, all, hipMemcpyHostToDevice, m->stream));
        LOM_HIP(m, hipEventRecord(m->stage_ev, m->stream));
        *d_xyz = m->scr[S_IN_XYZ].as<const char>();
        *d_nrm = *d_xyz + (hn - hx);
        return LOM_OK;
    }
    const size_t padded = (bytes + 255) & ~size_t(255);
    if ((rc = ensure(m, m->scr[S_IN_XYZ], bytes)) != LOM_OK) return rc;
    if (nrm && (rc = ensure(m, m->scr[S_IN_NRM], bytes)) != LOM_OK) return rc;
    if ((rc = stage_pinned(m, nrm ? 2 * padded : padded, &pin)) != LOM_OK) return rc;
    std::memcpy(pin, hx, bytes);
    LOM_HIP(m, hipMemcpyAsync(m->scr[S_IN_XYZ].p, pin, bytes, hipMemcpyHostToDevice, m->stream));
    *d_xyz = m->scr[S_IN_XYZ].as<const char>();
    if (nrm) {
        std::memcpy(pin + padded, hn, bytes);
        LOM_HIP(m, hipMemcpyAsync(m->scr[S_IN_NRM].p, pin + padded, bytes, hipMemcpyHostToDevice, m->stream));
        *d_nrm = m->scr[S_IN_NRM].as<const char>();
    }
    LOM_HIP(m, hipEventRecord(m->stage_ev, m->stream));
    return LOM_OK;
}

// the single-pass scan of a radius cleanup: flags, new slab numbers, number of voxels kept (words[4]); `from` as k_cleanup_scan's
static bool launch_cleanup_scan(lom_map *m, uint32_t nv, const float center[3], float r2, uint32_t seq, const AlignState *from)
{
    // consecutive voxels per thread: the smallest form whose grid stays within kOnePassMax threads
    static const struct {
        uint32_t items;
        decltype(&k_cleanup_scan<1>) kernel;
    } forms[] = {{1, k_cleanup_scan<1>}, {4, k_cleanup_scan<4>}, {16, k_cleanup_scan<16>}};
    uint32_t *keep = m->scr[S_FLAG].as<uint32_t>(), *newid = m->scr[S_RANK].as<uint32_t>();
    for (const auto &f : forms) {
        if (nv > f.items * kOnePassMax) continue;
        hipLaunchKernelGGL(f.kernel, dim3(blocks_for((nv + f.items - 1) / f.items)), dim3(kThreads), 0, m->stream,
                           m->slabs.pts, m->slabs.count, m->K, nv, center[0], center[1], center[2], r2, keep, newid, d_agg(m), seq,
                           d_word(m, 0), take_test_fail_from(m), from);
        return true;
    }
    return false;
}

// the same through kernels that wait for nobody: flags, multi-launch scan; the number of voxels kept in word 4
static int cleanup_scan_multi_launch(lom_map *m, uint32_t nv, const float center[3], float r2)
{
    uint32_t *keep = m->scr[S_FLAG].as<uint32_t>(), *newid = m->scr[S_RANK].as<uint32_t>();
    hipLaunchKernelGGL(k_cleanup_flag, dim3(blocks_for(nv)), dim3(kThreads), 0, m->stream, m->slabs.pts, m->slabs.count, m->K, nv,
                       center[0], center[1], center[2], r2, keep);
    LOM_HIP(m, hipGetLastError());
    return scan_exclusive(m, keep, newid, nv, d_word(m, 4), m->scr[S_SCAN].as<uint32_t>());
}

// lidar_odometry.cpp:65-67 calls radiusCleanup with the translation the align has just produced: the scan of that cleanup
// only reads the map and writes scratch, so it can run right behind the align's last solve -- with the centre taken from
// the align's state in HBM -- instead of a host round trip, a thread hand-off and a launch later.  The caller arms it
// (lom_map_radius_cleanup_after_align), the next device-resident align on the handle enqueues scan and read-back behind
// its first five (k_match, k_lm) pairs (align.hip), and lom_map_radius_cleanup takes the result if, and only if, it was
// made for exactly its arguments on exactly this state of the map; everything else is the plain path below.
constexpr size_t kSpecWordsOffset = 768;  // of h_report / d_report: the words of a scan enqueued behind an align
constexpr int kSpecWords = 6;             // words 4 (kept), 7 (scan gave up), 12 (made for this call), 13..15 (centre used)

void cleanup_scan_behind_align(lom_map *m)
{
    const float radius = m->spec_radius;
    m->spec_radius = 0.f;  // armed for one align
    // (a scan nobody has asked for since -- the caller did something else with the map -- is simply superseded: the
    // read-back of this one follows it on the stream and carries the next tag)
    m->spec_inflight = false;
    if (!(radius > 0.f) || m->parent || m->n_vox_stale || m->pending_n.load() || m->n_vox == 0 || !m->align_state.p) return;
    const uint32_t nv = m->n_vox;
    // (scratch that has to grow: the plain path does that; an allocation here would wait for the align)
    if (m->scr[S_FLAG].bytes < (size_t)nv * 4 || m->scr[S_RANK].bytes < (size_t)nv * 4 || nv > 16 * kOnePassMax) return;
    const float zero[3] = {0.f, 0.f, 0.f};
    const uint32_t seq = ++m->call_seq;
    if (!launch_cleanup_scan(m, nv, zero, radius * radius, seq, m->align_state.as<const AlignState>())) return;
    WordPtrs w;
    const int idx[kSpecWords] = {4, 7, 12, 13, 14, 15};
    for (int i = 0; i < 32; i++) w.p[i] = i < kSpecWords ? d_word(m, idx[i]) : nullptr;
    if (++m->spec_tag == 0) m->spec_tag = 1;
    hipLaunchKernelGGL(k_gather_words, dim3(1), dim3(64), 0, m->stream, w, kSpecWords,
                       reinterpret_cast<unsigned long long *>((char *)m->d_report + kSpecWordsOffset), m->spec_tag);
    if (hipGetLastError() != hipSuccess) return;  // (nothing in flight that anybody will wait for)
    m->spec_inflight = true;
    m->spec_seq = seq;
    m->spec_nv = nv;
    m->spec_r = radius;
    m->spec_mutations = m->mutations.load();
}

}  // namespace lom

using namespace lom;

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int64_t lom_map_debug_counter(const lom_map *m, int which)
{
    if (!m) return LOM_ERR_ARG;
    if (which == LOM_COUNTER_GRID_REDOS) return (int64_t)m->grid_redos;
    if (which == LOM_COUNTER_CLEANUPS_BEHIND_ALIGN) return (int64_t)m->cleanups_taken;
    if (which == LOM_COUNTER_EMPTY_SLABS) return (int64_t)m->n_dead;
    return LOM_ERR_ARG;
}

int lom_map_clear(lom_map *m, float voxel_size)
{
    if (!m || !(voxel_size > 0.f)) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    m->voxel_size = voxel_size;
    m->n_vox = 0;
    m->n_dead = 0;
    m->n_vox_ub = 0;
    m->n_vox_stale = false;
    m->n_points = 0;
    m->pending_n = 0;
    m->mutations++;
    if (!m->table_clean) {
        hipLaunchKernelGGL(k_table_init, dim3(blocks_for(m->cap)), dim3(kThreads), 0, m->stream, m->d_table, m->cap);
        LOM_HIP(m, hipMemsetAsync(d_nvox(m), 0, 4, m->stream));
        LOM_HIP(m, hipGetLastError());
        m->table_clean = true;
    }
    return LOM_OK;
}

int lom_map_set_max_points(lom_map *m, size_t max_points)
{
    if (!m || max_points == 0 || max_points > 65535) return LOM_ERR_ARG;
    if (m->parent) return fail(m, LOM_ERR_ARG, "a scan context cannot change its keyframe");
    LOM_HIP(m, hipSetDevice(m->device));
    {
        const int rcn = refresh_nvox(m);  // also resolves a pending insert: it was made under the old value
        if (rcn != LOM_OK) return rcn;
    }
    // voxel_grid.h:56-59: max_points_ = max_points, nothing else -- stored voxels keep what they hold, and :86-90
    // appends to a voxel only while size() < max_points_.  The row stride K follows the largest value seen while
    // voxels exist (a raise re-strides the slabs); an empty map starts over with stride = max_points.
    if (m->n_vox == 0 && max_points != m->K) {
        LOM_HIP(m, hipStreamSynchronize(m->stream));
        slabs_free(m->slabs);
        slabs_free(m->alt);
        m->K = (uint32_t)max_points;
    } else if (max_points > m->K) {
        if ((uint64_t)m->slabs.cap > 0x7FFFFFFFull / max_points) return fail(m, LOM_ERR_OOM, "map too large");
        m->mutations++;
        const uint32_t K0 = m->K, K1 = (uint32_t)max_points;
        const size_t pb = (size_t)m->slabs.cap * K1 * 3 * sizeof(float);
        float *p1 = nullptr, *n1 = nullptr;
        if (hipMalloc(&p1, pb + kRowPadBytes) != hipSuccess || hipMalloc(&n1, pb + kRowPadBytes) != hipSuccess) {
            (void)hipGetLastError();
            if (p1) (void)hipFree(p1);
            return fail(m, LOM_ERR_OOM, "hipMalloc(slabs)");
        }
        const size_t work = (size_t)m->n_vox * K0;
        hipLaunchKernelGGL(k_restride, dim3(blocks_for(work)), dim3(kThreads), 0, m->stream, m->slabs.pts, m->slabs.nrm,
                           m->slabs.count, m->n_vox, K0, K1, p1, n1);
        LOM_HIP(m, hipGetLastError());
        LOM_HIP(m, hipStreamSynchronize(m->stream));
        (void)hipFree(m->slabs.pts);
        (void)hipFree(m->slabs.nrm);
        m->slabs.pts = p1;
        m->slabs.nrm = n1;
        slabs_free(m->alt);  // the cleanup's second set of slabs has the old stride: it is allocated again when needed
        m->K = K1;
    }
    m->max_points = (uint32_t)max_points;
    return LOM_OK;
}

int lom_map_add_points_device(lom_map *m, const float *d_xyz, const float *d_nrm, size_t n, size_t stride)
{
    if (!m || (n && !d_xyz) || stride < 12 || (stride & 3)) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    return add_points_device(m, (const char *)d_xyz, (const char *)d_nrm, n, stride, false, true);
}

int lom_map_add_points_device_nowait(lom_map *m, const float *d_xyz, const float *d_nrm, size_t n, size_t stride)
{
    if (!m || (n && !d_xyz) || stride < 12 || (stride & 3)) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    return add_points_device(m, (const char *)d_xyz, (const char *)d_nrm, n, stride, false, false);
}

int lom_profile_insert(lom_map *m, const float *d_xyz, const float *d_nrm, size_t n, size_t stride, double *total_us_out)
{
    if (!m || !d_xyz || !n || !total_us_out || stride < 12 || (stride & 3)) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    // capacity and scratch first, so that the bracket holds the insert's kernels only
    int rc = refresh_nvox(m);
    if (rc != LOM_OK) return rc;
    const uint64_t worst = (uint64_t)m->n_vox + n;
    if ((uint64_t)m->cap < 2 * worst && (rc = rehash(m, next_pow2(4 * worst))) != LOM_OK) return rc;
    if (worst > m->slabs.cap && (rc = ensure_slabs(m, worst + worst / 2)) != LOM_OK) return rc;
    if (n > kOnePassMax && n <= kBiMaxPoints && !m->opt_no_bulk &&
        (rc = bulk_scratch(m, (uint32_t)n, bulk_shape((uint32_t)n, m->cap, m->bulk_ppt))) != LOM_OK)
        return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    LOM_HIP(m, hipEventCreate(&e0));
    LOM_HIP(m, hipEventCreate(&e1));
    LOM_HIP(m, hipStreamSynchronize(m->stream));
    hipError_t e = hipEventRecord(e0, m->stream);
    rc = add_points_device(m, (const char *)d_xyz, (const char *)d_nrm, n, stride, false, false, false);
    if (e == hipSuccess) e = hipEventRecord(e1, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc != LOM_OK) return rc;
    if (e != hipSuccess) return fail(m, LOM_ERR_HIP, "lom_profile_insert", e);
    *total_us_out = (double)ms * 1e3;
    if ((rc = map_status(m)) != LOM_OK) return rc;
    // what lom_map_add_points_device does after a bulk insert: ~16 slots per voxel
    const uint32_t target = std::max(m->min_cap, next_pow2((uint64_t)m->table_slots_per_voxel * m->n_vox));
    if (m->cap > target) return rehash(m, target);
    return LOM_OK;
}

int lom_map_status(lom_map *m)
{
    if (!m) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    return map_status(m);
}

int lom_map_add_points(lom_map *m, const float *xyz, const float *nrm, size_t n, size_t stride)
{
    if (!m || (n && !xyz) || stride < 12 || (stride & 3)) return LOM_ERR_ARG;
    if (n == 0) return LOM_OK;
    LOM_HIP(m, hipSetDevice(m->device));
    // the points are in host memory: range-check them here (same f32 division and bounds as the
    // device's voxel_index) instead of paying a kernel and a synchronisation
    {
        const float vs = m->voxel_size;
        bool bad = false;
        for (size_t i = 0; i < n; i++) {
            const float *p = reinterpret_cast<const float *>(reinterpret_cast<const char *>(xyz) + i * stride);
            const float fx = p[0] / vs, fy = p[1] / vs, fz = p[2] / vs;
            bad |= !(fx > -kIdxLimit && fx < kIdxLimit) || !(fy > -kIdxLimit && fy < kIdxLimit) ||
                   !(fz > -kIdxLimit && fz < kIdxLimit);
        }
        if (bad) return fail(m, LOM_ERR_RANGE, "coordinate / voxel_size out of range or not finite");
    }
    const char *dx = nullptr, *dn = nullptr;
    int rc = resolve_pending(m);  // before the staging buffers (a pending insert's input) are overwritten
    if (rc != LOM_OK) return rc;
    if ((rc = stage_host_points(m, xyz, nrm, n, stride, &dx, &dn)) != LOM_OK) return rc;
    // the caller's buffer has been copied into the pinned bounce buffer: no need to wait for the GPU
    return add_points_device(m, dx, dn, n, stride, true, false);
}

int lom_map_radius_cleanup_after_align(lom_map *m, float radius)
{
    if (!m) return LOM_ERR_ARG;
    m->spec_radius = (radius > 0.f && !m->parent) ? radius : 0.f;
    return LOM_OK;
}

// the result of a scan enqueued behind an align, if it was made for this call: 1 = h_flags[0] (kept) and h_flags[3]
// (give-up word) are set as read_words(m, 4, 4) would have, *seq_out = the scan's sequence number; 0 = not usable
static int take_cleanup_behind_align(lom_map *m, const float center[3], float radius, uint32_t *seq_out)
{
    if (!m->spec_inflight) return 0;
    m->spec_inflight = false;
    volatile unsigned long long *hw = reinterpret_cast<volatile unsigned long long *>((char *)m->h_report + kSpecWordsOffset);
    uint32_t got[kSpecWords];
    uint64_t spins = 0;
    for (int i = 0; i < kSpecWords; i++) {
        while ((uint32_t)(hw[i] >> 32) != m->spec_tag) {
            __builtin_ia32_pause();
            if ((++spins & 0x3FFF) != 0) continue;
            const hipError_t e = hipStreamQuery(m->stream);
            if (e == hipSuccess) {
                if ((uint32_t)(hw[i] >> 32) == m->spec_tag) break;
                return 0;
            }
            if (e != hipErrorNotReady) return 0;  // (the plain path meets the same stream and reports it)
        }
        got[i] = (uint32_t)hw[i];
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    uint32_t cb[3];
    std::memcpy(cb, center, 12);
    const bool usable = got[2] == m->spec_seq && got[3] == cb[0] && got[4] == cb[1] && got[5] == cb[2] &&
                        std::memcmp(&radius, &m->spec_r, 4) == 0 && m->call_seq == m->spec_seq &&
                        m->mutations.load() == m->spec_mutations && m->n_vox == m->spec_nv && !m->n_vox_stale;
    if (!usable) return 0;
    m->h_flags[0] = got[0];
    m->h_flags[3] = got[1];
    *seq_out = m->spec_seq;
    return 1;
}

// The back half of an erase, shared by lom_map_radius_cleanup and the ray carve: keep[] / newid[] of the `nv` slabs are in
// S_FLAG / S_RANK and `n_keep` of them are kept.  Few holes: the erased voxels' slabs are emptied in place
// (k_cleanup_mark); holes from a quarter of the slabs on (or LOM_DENSE_CLEANUP): compaction and a rebuilt table.
static int erase_unkept(lom_map *m, uint32_t nv, uint32_t n_keep)
{
    int rc;
    uint32_t *keep = m->scr[S_FLAG].as<uint32_t>(), *newid = m->scr[S_RANK].as<uint32_t>();
    const uint32_t n_live = nv - m->n_dead;
    if (n_keep == n_live) return LOM_OK;
    if (!m->opt_dense_cleanup && (uint64_t)(nv - n_keep) * 4u <= (uint64_t)nv) {
        // few holes: the erased voxels' slabs stay where they are, empty (see k_cleanup_mark)
        const MapView v = view_of(m);
        hipLaunchKernelGGL(k_cleanup_mark, dim3(blocks_for(nv)), dim3(kThreads), 0, m->stream, m->d_table, v.mask, v.shift, keep, nv,
                           m->slabs.key, m->slabs.count);
        LOM_HIP(m, hipGetLastError());
        m->n_dead = nv - n_keep;
        m->dead_below = nv;
        return LOM_OK;
    }
    // stable compaction into the second (persistent) set of slab arrays, swap, rebuild the table
    if (m->alt.cap != m->slabs.cap) {
        LOM_HIP(m, hipStreamSynchronize(m->stream));
        slabs_free(m->alt);
        if ((rc = slabs_alloc(m, m->slabs.cap, m->alt)) != LOM_OK) return rc;
    }
    const size_t work = (size_t)nv * m->K;
    hipLaunchKernelGGL(k_compact, dim3(blocks_for(work)), dim3(kThreads), 0, m->stream, keep, newid, nv, m->K,
                       m->slabs.key, m->slabs.count, m->slabs.pts, m->slabs.nrm, m->alt.key, m->alt.count, m->alt.pts,
                       m->alt.nrm, d_nvox(m), n_keep);
    LOM_HIP(m, hipGetLastError());
    std::swap(m->slabs, m->alt);  // (of equal capacity)
    m->n_vox = n_keep;
    m->n_vox_ub = n_keep;
    m->n_dead = 0;  // (the holes are closed)
    const MapView v = view_of(m);
    hipLaunchKernelGGL(k_table_init, dim3(blocks_for(m->cap)), dim3(kThreads), 0, m->stream, m->d_table, m->cap);
    if (n_keep) {
        hipLaunchKernelGGL(k_rebuild, dim3(blocks_for(n_keep)), dim3(kThreads), 0, m->stream, m->d_table, v.mask,
                           v.shift, m->slabs.key, m->slabs.count, n_keep);
    }
    LOM_HIP(m, hipGetLastError());
    return LOM_OK;
}

int lom_map_radius_cleanup(lom_map *m, const float center[3], float radius)
{
    if (!m || !center) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    int rc;
    if ((rc = refresh_nvox(m)) != LOM_OK) return rc;
    uint32_t seq = 0;
    const bool taken = take_cleanup_behind_align(m, center, radius, &seq) == 1;
    if (m->n_vox == 0) return LOM_OK;
    const uint32_t nv = m->n_vox;
    // (twice what this call needs: a scan enqueued behind an align does not allocate, a growing keyframe should not
    // outgrow the scratch every few frames)
    // (a scan that has been taken left its flags and new slab numbers in these two: they stay where they are)
    if (!taken) {
        if ((rc = ensure(m, m->scr[S_FLAG], (size_t)nv * 8)) != LOM_OK) return rc;
        if ((rc = ensure(m, m->scr[S_RANK], (size_t)nv * 8)) != LOM_OK) return rc;
    }
    if ((rc = ensure(m, m->scr[S_SCAN], scan_tmp_words(nv) * 4)) != LOM_OK) return rc;
    const float r2 = radius * radius;  // voxel_grid.h:238
    if (!taken) seq = ++m->call_seq;
    m->mutations++;
    bool one_pass = true;
    if (!taken) {
        one_pass = launch_cleanup_scan(m, nv, center, r2, seq, nullptr);
        if (!one_pass && (rc = cleanup_scan_multi_launch(m, nv, center, r2)) != LOM_OK) return rc;
        LOM_HIP(m, hipGetLastError());
        if ((rc = read_words(m, 4, 4)) != LOM_OK) return rc;
    } else {
        m->cleanups_taken++;
    }
    if (one_pass && m->h_flags[3] == seq) {
        // the in-kernel scan gave up (it has written scratch only): flags + multi-launch scan instead
        m->grid_redos++;
        m->status_seq = std::max(m->status_seq, seq);
        if ((rc = cleanup_scan_multi_launch(m, nv, center, r2)) != LOM_OK) return rc;
        if ((rc = read_words(m, 4, 1)) != LOM_OK) return rc;
    }
    return erase_unkept(m, nv, m->h_flags[0]);
}

// ---- ray carving (lidar_odometry_amd.h, "ray carving"; kernels: k_carve.hpp) ------------------------------------------
// arguments first, then the state: nothing here touches HIP
static int carve_args(const lom_map *m, const float *origin, const float *xyz, size_t n, size_t stride, const lom_carve_params *p)
{
    if (!carve_params_ok(p)) return LOM_ERR_ARG;
    if (!m || !origin || (n && !xyz) || stride < 12 || (stride & 3) || n >= 0x7FFFFFFFull) return LOM_ERR_ARG;
    return LOM_OK;
}

// hits and walk of one call over the map's `nv` slabs (settled by the caller): cross[] / hit[] / the carve's words are
// left on the device.  The origin's range verdict is the host's (the array is the host's in every entry point).
static int carve_count(lom_map *m, uint32_t nv, const float origin[3], const char *d_xyz, uint32_t n, size_t stride,
                       const lom_carve_params &p)
{
    const float vs = m->voxel_size;
    for (int a = 0; a < 3; a++) {
        const float f = origin[a] / vs;
        if (!(f > -kIdxLimit && f < kIdxLimit))
            return fail(m, LOM_ERR_RANGE, "carve: origin / voxel_size out of range or not finite");
    }
    int rc;
    uint32_t *cross, *hit, *words;
    const size_t room = std::max<size_t>((size_t)nv * 2, 64);  // (twice: a growing keyframe; never nothing: an empty map)
    if ((rc = scratch(m, S_CARVE_CROSS, room, &cross)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_CARVE_HIT, room, &hit)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_CARVE_WORDS, (size_t)CW_COUNT, &words)) != LOM_OK) return rc;
    if (nv) {
        LOM_HIP(m, hipMemsetAsync(cross, 0, (size_t)nv * 4, m->stream));
        LOM_HIP(m, hipMemsetAsync(hit, 0, (size_t)nv * 4, m->stream));
    }
    LOM_HIP(m, hipMemsetAsync(words, 0, (size_t)CW_COUNT * 4, m->stream));
    CarveArgs a;
    for (int k = 0; k < 3; k++) a.o[k] = origin[k];
    a.voxel_size = vs;
    a.margin = p.margin;
    a.min_range = p.min_range;
    a.max_range = p.max_range;
    // (no ray is longer than the index range: 2^21 cells per axis)
    const double cells = std::min(std::ceil((double)p.max_range / (double)vs), 2097152.0);
    a.max_steps = 3u * ((uint32_t)cells + 2u);
    const MapView v = view_of(m);
    hipLaunchKernelGGL(k_carve_hits, dim3(blocks_for(n)), dim3(kThreads), 0, m->stream, d_xyz, stride, n, vs, v.table, v.mask,
                       v.shift, nv, hit, words);
    hipLaunchKernelGGL(k_carve_walk, dim3(blocks_for(n)), dim3(kThreads), 0, m->stream, d_xyz, stride, n, a, v.table, v.mask,
                       v.shift, nv, cross, words);
    LOM_HIP(m, hipGetLastError());
    return LOM_OK;
}

static int carve_rays(lom_map *m, const float origin[3], const float *xyz, size_t n, size_t stride, const lom_carve_params *p,
                      lom_carve_stats *stats, bool on_host)
{
    int rc = carve_args(m, origin, xyz, n, stride, p);
    if (rc != LOM_OK) return rc;
    if (m->parent) return fail(m, LOM_ERR_ARG, "a scan context cannot change its keyframe");
    if (stats) *stats = lom_carve_stats();
    if (n == 0) return LOM_OK;
    LOM_HIP(m, hipSetDevice(m->device));
    if ((rc = refresh_nvox(m)) != LOM_OK) return rc;  // (settles a pending insert first: before the staging buffers are reused)
    const uint32_t nv = m->n_vox;  // (an empty map: hits and walk run all the same, for the range verdict and the stats)
    const char *d_xyz = (const char *)xyz, *d_none = nullptr;
    if (on_host && (rc = stage_host_points(m, xyz, nullptr, n, stride, &d_xyz, &d_none)) != LOM_OK) return rc;
    uint32_t *keep = nullptr, *newid = nullptr, *scan_tmp = nullptr;
    if (nv) {
        if ((rc = scratch(m, S_FLAG, (size_t)nv * 2, &keep)) != LOM_OK) return rc;
        if ((rc = scratch(m, S_RANK, (size_t)nv * 2, &newid)) != LOM_OK) return rc;
        if ((rc = scratch(m, S_SCAN, scan_tmp_words(nv), &scan_tmp)) != LOM_OK) return rc;
    }
    // keep / newid go where a cleanup scan armed behind an align may have left its own: that scan is never taken now
    m->spec_inflight = false;
    ++m->call_seq;
    m->mutations++;
    if ((rc = carve_count(m, nv, origin, d_xyz, (uint32_t)n, stride, *p)) != LOM_OK) return rc;
    uint32_t *cross = m->scr[S_CARVE_CROSS].as<uint32_t>(), *hit = m->scr[S_CARVE_HIT].as<uint32_t>(),
             *words = m->scr[S_CARVE_WORDS].as<uint32_t>();
    if (nv) {
        hipLaunchKernelGGL(k_carve_flag, dim3(blocks_for(nv)), dim3(kThreads), 0, m->stream, cross, hit, m->slabs.count, nv,
                           p->min_crossings, keep, words);
        LOM_HIP(m, hipGetLastError());
        if ((rc = scan_exclusive(m, keep, newid, nv, d_word(m, 4), scan_tmp)) != LOM_OK) return rc;
    }
    // the one read-back: error word and stats with the kept count, before anything is erased
    const uint32_t *ptrs[CW_COUNT + 1];
    for (int i = 0; i < CW_COUNT; i++) ptrs[i] = words + i;
    ptrs[CW_COUNT] = d_word(m, 4);
    uint32_t got[CW_COUNT + 1];
    if ((rc = gather_words(m, ptrs, CW_COUNT + 1, got)) != LOM_OK) return rc;
    if (got[CW_ERROR]) return fail(m, LOM_ERR_RANGE, "carve: coordinate / voxel_size out of range or not finite");
    const uint32_t n_keep = nv ? got[CW_COUNT] : 0u, n_live = nv - m->n_dead;
    if (stats) {
        stats->rays_walked = (uint64_t)got[CW_WALKED] | ((uint64_t)got[CW_WALKED + 1] << 32);
        stats->rays_skipped = n - stats->rays_walked;
        stats->cells_visited = (uint64_t)got[CW_VISITED] | ((uint64_t)got[CW_VISITED + 1] << 32);
        stats->voxels_crossed = got[CW_CROSSED];
        stats->voxels_protected = got[CW_PROTECTED];
        stats->voxels_erased = n_live - n_keep;
    }
    return nv ? erase_unkept(m, nv, n_keep) : LOM_OK;
}

int lom_map_carve_rays(lom_map *m, const float origin[3], const float *xyz, size_t n, size_t stride, const lom_carve_params *p,
                       lom_carve_stats *stats)
{
    return carve_rays(m, origin, xyz, n, stride, p, stats, true);
}

int lom_map_carve_rays_device(lom_map *m, const float origin[3], const float *d_xyz, size_t n, size_t stride,
                              const lom_carve_params *p, lom_carve_stats *stats)
{
    return carve_rays(m, origin, d_xyz, n, stride, p, stats, false);
}

int64_t lom_map_carve_counts(lom_map *m, const float origin[3], const float *xyz, size_t n, size_t stride,
                             const lom_carve_params *p, uint32_t *cross_out, uint8_t *hit_out, size_t cap)
{
    int rc = carve_args(m, origin, xyz, n, stride, p);
    if (rc != LOM_OK) return rc;
    if (m->parent) return fail(m, LOM_ERR_ARG, "carve counts are the map's, not a scan context's");
    LOM_HIP(m, hipSetDevice(m->device));
    if ((rc = refresh_nvox(m)) != LOM_OK) return rc;
    const uint32_t nv = m->n_vox;  // (an empty map: the kernels run all the same, for the range verdict)
    std::vector<uint32_t> cross(nv, 0u), hit(nv, 0u), count(nv), words(CW_COUNT, 0u);
    if (n) {
        const char *d_xyz = nullptr, *d_none = nullptr;
        if ((rc = stage_host_points(m, xyz, nullptr, n, stride, &d_xyz, &d_none)) != LOM_OK) return rc;
        if ((rc = carve_count(m, nv, origin, d_xyz, (uint32_t)n, stride, *p)) != LOM_OK) return rc;
        if (nv) {
            LOM_HIP(m, hipMemcpyAsync(cross.data(), m->scr[S_CARVE_CROSS].p, (size_t)nv * 4, hipMemcpyDeviceToHost, m->stream));
            LOM_HIP(m, hipMemcpyAsync(hit.data(), m->scr[S_CARVE_HIT].p, (size_t)nv * 4, hipMemcpyDeviceToHost, m->stream));
        }
        LOM_HIP(m, hipMemcpyAsync(words.data(), m->scr[S_CARVE_WORDS].p, (size_t)CW_COUNT * 4, hipMemcpyDeviceToHost, m->stream));
    }
    if (nv) LOM_HIP(m, hipMemcpyAsync(count.data(), m->slabs.count, (size_t)nv * 4, hipMemcpyDeviceToHost, m->stream));
    LOM_HIP(m, hipStreamSynchronize(m->stream));
    if (words[CW_ERROR]) return fail(m, LOM_ERR_RANGE, "carve: coordinate / voxel_size out of range or not finite");
    size_t live = 0;
    for (uint32_t s = 0; s < nv; s++) {
        if (!count[s]) continue;  // (the export skips empty slabs)
        if (live < cap) {
            if (cross_out) cross_out[live] = cross[s];
            if (hit_out) hit_out[live] = hit[s] ? 1 : 0;
        }
        live++;
    }
    return (int64_t)live;
}

int64_t lom_map_size(const lom_map *cm)
{
    lom_map *m = const_cast<lom_map *>(cm);
    if (!m) return LOM_ERR_ARG;
    if (m->n_vox_stale || m->pending_n) {
        if (hipSetDevice(m->device) != hipSuccess) return LOM_ERR_HIP;
        const int rc = refresh_nvox(m);
        if (rc != LOM_OK) return rc;
    }
    return (int64_t)(m->n_vox - m->n_dead);  // (slabs in use minus those whose voxel a cleanup erased)
}

int64_t lom_map_point_count(const lom_map *cm)
{
    // the stored points are exactly what the full export would return
    return lom_map_export(const_cast<lom_map *>(cm), LOM_EXPORT_FULL_NO_NORMALS, nullptr, nullptr, 0);
}

// shared body of the down-samplers: device input, results left in the workspace's scratch
// (S_ITEMS: xyz, S_PT_POS: normals), voxel count in word 4, range flag in word 5 of S_MISC.
// wait: read the count and the verdict back (one synchronisation); otherwise the call only enqueues and
// the count stays on the device (d_word(m, 4)) for the kernels that consume the result.
static int downsample_core(lom_map *m, float voxel_size, const char *dx, const char *dn, uint32_t N, size_t stride,
                           bool want_normals, bool wait, const uint32_t *n_dev = nullptr, bool multi_launch = false)
{
    int rc;
    if ((uint64_t)m->cap < 2ull * N) {
        if ((rc = rehash(m, next_pow2(4ull * N))) != LOM_OK) return rc;
    }
    const bool one_pass = N <= 4 * kOnePassMax && !multi_launch;
    uint32_t *pt_slot, *head;
    float *oxyz, *onrm;
    if ((rc = scratch(m, S_PT_SLOT, N, &pt_slot)) != LOM_OK) return rc;
    if ((rc = ensure_rest(m, m->scr[S_DS_HEAD], (size_t)m->cap * 4, 0xFF)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_ITEMS, (size_t)N * 3, &oxyz)) != LOM_OK) return rc;   // compacted xyz
    if ((rc = scratch(m, S_PT_POS, (size_t)N * 3, &onrm)) != LOM_OK) return rc;  // compacted normals
    head = m->scr[S_DS_HEAD].as<uint32_t>();
    if (!want_normals) onrm = nullptr;
    const uint32_t seq = ++m->call_seq;
    const MapView v = view_of(m);
    const dim3 g(blocks_for(N)), b(kThreads);
    if (n_dev && !one_pass) return fail(m, LOM_ERR_ARG, "device-side point count: at most 262144 points");
    hipLaunchKernelGGL(k_ds_claim, g, b, 0, m->stream, m->d_table, v.mask, v.shift, dx, stride, N, n_dev, voxel_size,
                       pt_slot, head, seq, d_word(m, 5));
    if (one_pass) {
        const uint32_t items = N <= kOnePassMax ? 1u : 4u;  // consecutive points per thread
        hipLaunchKernelGGL(items == 1 ? k_ds_emit<1> : k_ds_emit<4>, dim3(blocks_for((N + items - 1) / items)), b, 0, m->stream,
                           m->d_table, N, n_dev, pt_slot, head, dx, dn, stride, oxyz, onrm, d_agg(m), seq, d_word(m, 0),
                           take_test_fail_from(m));
        LOM_HIP(m, hipGetLastError());
    } else {
        uint32_t *flag, *rank, *scan_tmp;
        if ((rc = scratch(m, S_FLAG, N, &flag)) != LOM_OK) return rc;
        if ((rc = scratch(m, S_RANK, N, &rank)) != LOM_OK) return rc;
        if ((rc = scratch(m, S_SCAN, scan_tmp_words(N), &scan_tmp)) != LOM_OK) return rc;
        hipLaunchKernelGGL(k_ds_flag, g, b, 0, m->stream, N, pt_slot, head, flag);
        LOM_HIP(m, hipGetLastError());
        if ((rc = scan_exclusive(m, flag, rank, N, d_word(m, 4), scan_tmp)) != LOM_OK) return rc;
        // the kept point of every voxel also frees its table slot and head word: the workspace is at rest again
        hipLaunchKernelGGL(k_ds_write, g, b, 0, m->stream, N, flag, rank, dx, dn, stride, oxyz, onrm, m->d_table, pt_slot,
                           head);
        LOM_HIP(m, hipGetLastError());
    }
    if (!wait) return LOM_OK;
    if ((rc = read_words(m, 4, 4)) != LOM_OK) return rc;  // [0] voxels, [1] range flag, [3] grid error
    m->status_seq = seq;
    if (m->h_flags[3] == seq) {
        // the in-kernel scan gave up: every kept point has still put its slot and head word back to rest, so the
        // workspace is empty again; same call through the flag / scan / write kernels, which wait for nobody
        if (n_dev) return fail(m, LOM_ERR_HIP, "a workgroup timed out waiting for the others of its grid");
        m->grid_redos++;
        return downsample_core(m, voxel_size, dx, dn, N, stride, want_normals, true, nullptr, true);
    }
    if (m->h_flags[1] == seq) return fail(m, LOM_ERR_RANGE, "coordinate / voxel_size out of range or not finite");
    return LOM_OK;
}

int64_t lom_voxel_downsample(lom_map *ws, float voxel_size, const float *xyz, const float *nrm, size_t n,
                             size_t stride, float *xyz_out, float *nrm_out, size_t cap)
{
    lom_map *m = ws;
    if (!m || !(voxel_size > 0.f) || (n && !xyz) || stride < 12 || (stride & 3) || (n && !xyz_out)) return LOM_ERR_ARG;
    if (n >= 0x7FFFFFFFull) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    int rc = lom_map_clear(m, voxel_size);  // the workspace grid ends up cleared, like a fresh VoxelGrid(voxel, 1)
    if (rc != LOM_OK || n == 0) return rc;
    const char *dx = nullptr, *dn = nullptr;
    if ((rc = stage_host_points(m, xyz, nrm, n, stride, &dx, &dn)) != LOM_OK) return rc;
    // the range rule of addCloud is checked by the claim kernel (flag read back with the count)
    if ((rc = downsample_core(m, voxel_size, dx, dn, (uint32_t)n, stride, nrm_out != nullptr, true)) != LOM_OK) return rc;
    const size_t total = m->h_flags[0];
    const size_t take = std::min(total, cap);
    if (take) {
        LOM_HIP(m, hipMemcpyAsync(xyz_out, m->scr[S_ITEMS].p, take * 12, hipMemcpyDeviceToHost, m->stream));
        if (nrm_out)
            LOM_HIP(m, hipMemcpyAsync(nrm_out, m->scr[S_PT_POS].p, take * 12, hipMemcpyDeviceToHost, m->stream));
        LOM_HIP(m, hipStreamSynchronize(m->stream));
    }
    return (int64_t)total;
}

int64_t lom_voxel_downsample_device(lom_map *ws, float voxel_size, const float *d_xyz, const float *d_nrm, size_t n,
                                    size_t stride, const float **d_xyz_out, const float **d_nrm_out)
{
    lom_map *m = ws;
    if (!m || !(voxel_size > 0.f) || (n && !d_xyz) || stride < 12 || (stride & 3) || !d_xyz_out) return LOM_ERR_ARG;
    if (n >= 0x7FFFFFFFull) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    *d_xyz_out = nullptr;
    if (d_nrm_out) *d_nrm_out = nullptr;
    int rc = lom_map_clear(m, voxel_size);
    if (rc != LOM_OK || n == 0) return rc;
    if ((rc = downsample_core(m, voxel_size, (const char *)d_xyz, (const char *)d_nrm, (uint32_t)n, stride,
                              d_nrm_out != nullptr, true)) != LOM_OK)
        return rc;
    *d_xyz_out = m->scr[S_ITEMS].as<const float>();
    if (d_nrm_out) *d_nrm_out = m->scr[S_PT_POS].as<const float>();
    return (int64_t)m->h_flags[0];
}

int lom_voxel_downsample_device_nowait(lom_map *ws, float voxel_size, const float *d_xyz, const float *d_nrm,
                                       size_t n_bound, const uint32_t *d_n, size_t stride, const float **d_xyz_out,
                                       const float **d_nrm_out, const uint32_t **d_count_out)
{
    lom_map *m = ws;
    if (!m || !(voxel_size > 0.f) || (n_bound && !d_xyz) || stride < 12 || (stride & 3) || !d_xyz_out || !d_count_out)
        return LOM_ERR_ARG;
    if (n_bound >= 0x7FFFFFFFull) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    *d_xyz_out = nullptr;
    if (d_nrm_out) *d_nrm_out = nullptr;
    int rc = lom_map_clear(m, voxel_size);
    if (rc != LOM_OK) return rc;
    *d_count_out = d_word(m, 4);
    if (n_bound == 0) {
        LOM_HIP(m, hipMemsetAsync(d_word(m, 4), 0, 4, m->stream));
        return LOM_OK;
    }
    if ((rc = downsample_core(m, voxel_size, (const char *)d_xyz, (const char *)d_nrm, (uint32_t)n_bound, stride,
                              d_nrm_out != nullptr, false, d_n)) != LOM_OK)
        return rc;
    *d_xyz_out = m->scr[S_ITEMS].as<const float>();
    if (d_nrm_out) *d_nrm_out = m->scr[S_PT_POS].as<const float>();
    return LOM_OK;
}

int lom_map_wait_event(lom_map *m, void *hip_event)
{
    if (!m || !hip_event) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    LOM_HIP(m, hipStreamWaitEvent(m->stream, (hipEvent_t)hip_event, 0));
    return LOM_OK;
}

int lom_map_status_words(lom_map *m, const uint32_t **d_range, const uint32_t **d_grid, uint32_t *seq)
{
    if (!m || !d_range || !d_grid || !seq) return LOM_ERR_ARG;
    *d_range = d_word(m, 5);
    *d_grid = d_word(m, 7);
    *seq = m->call_seq;
    m->status_seq = m->call_seq;  // the caller looks at the words itself
    return LOM_OK;
}

int lom_map_read_device_words(lom_map *m, const uint32_t *const *d_ptrs, int n, uint32_t *out)
{
    if (!m || !d_ptrs || !out || n < 0 || n > 32) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    for (int i = 0; i < n; i++)
        if (!d_ptrs[i]) return LOM_ERR_ARG;
    return gather_words(m, d_ptrs, n, out);
}

int lom_map_read_device_words_begin(lom_map *m, const uint32_t *const *d_ptrs, int n)
{
    if (!m || !d_ptrs || n < 0 || n > 32) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    for (int i = 0; i < n; i++)
        if (!d_ptrs[i]) return LOM_ERR_ARG;
    return gather_words_begin(m, d_ptrs, n);
}

int lom_map_read_device_words_end(lom_map *m, uint32_t *out)
{
    if (!m || !out) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    return gather_words_end(m, out);
}

int lom_upload_points(lom_map *m, const float *xyz, const float *nrm, size_t n, size_t stride, const float **d_xyz_out,
                      const float **d_nrm_out)
{
    if (!m || (n && !xyz) || stride < 12 || (stride & 3) || !d_xyz_out) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    *d_xyz_out = nullptr;
    if (d_nrm_out) *d_nrm_out = nullptr;
    if (n == 0) return LOM_OK;
    const char *dx = nullptr, *dn = nullptr;
    int rc = resolve_pending(m);
    if (rc != LOM_OK) return rc;
    if ((rc = stage_host_points(m, xyz, nrm, n, stride, &dx, &dn)) != LOM_OK) return rc;
    *d_xyz_out = (const float *)dx;
    if (d_nrm_out) *d_nrm_out = (const float *)dn;
    return LOM_OK;
}

int lom_transform_points_device(lom_map *m, const lom_pose *pose, const float *d_xyz, const float *d_nrm, size_t n,
                                size_t stride, const float **d_xyz_out, const float **d_nrm_out)
{
    if (!m || !pose || (n && !d_xyz) || stride < 12 || (stride & 3) || !d_xyz_out) return LOM_ERR_ARG;
    if (n >= 0x7FFFFFFFull) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    *d_xyz_out = nullptr;
    if (d_nrm_out) *d_nrm_out = nullptr;
    if (n == 0) return LOM_OK;
    int rc;
    if ((rc = resolve_pending(m)) != LOM_OK) return rc;
    const bool with_n = d_nrm && d_nrm_out;
    if ((rc = ensure(m, m->scr[S_IN_XYZ], n * 12)) != LOM_OK) return rc;
    if (with_n && (rc = ensure(m, m->scr[S_IN_NRM], n * 12)) != LOM_OK) return rc;
    RigidArgs A;
    rotation_matrix(pose->q, A.R);
    for (int i = 0; i < 3; i++) A.t[i] = pose->t[i];
    hipLaunchKernelGGL(k_transform, dim3(blocks_for((uint32_t)n)), dim3(kThreads), 0, m->stream, (const char *)d_xyz,
                       (const char *)d_nrm, stride, (uint32_t)n, A, m->scr[S_IN_XYZ].as<float>(),
                       with_n ? m->scr[S_IN_NRM].as<float>() : (float *)nullptr);
    LOM_HIP(m, hipGetLastError());
    *d_xyz_out = m->scr[S_IN_XYZ].as<const float>();
    if (with_n) *d_nrm_out = m->scr[S_IN_NRM].as<const float>();
    return LOM_OK;
}

int64_t lom_map_export(lom_map *m, int mode, float *xyz_out, float *nrm_out, size_t cap)
{
    if (!m || mode < 0 || mode > 2) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    int rc;
    if ((rc = refresh_nvox(m)) != LOM_OK) return rc;
    if (m->n_vox == 0) return 0;
    const uint32_t nv = m->n_vox;
    uint32_t *cnt, *off, *scan_tmp;
    if ((rc = scratch(m, S_FLAG, nv, &cnt)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_RANK, nv, &off)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_SCAN, scan_tmp_words(nv), &scan_tmp)) != LOM_OK) return rc;
    hipLaunchKernelGGL(k_export_counts, dim3(blocks_for(nv)), dim3(kThreads), 0, m->stream, m->slabs.count, nv, mode, cnt);
    LOM_HIP(m, hipGetLastError());
    if ((rc = scan_exclusive(m, cnt, off, nv, d_word(m, 4), scan_tmp)) != LOM_OK) return rc;
    if ((rc = read_words(m, 4, 1)) != LOM_OK) return rc;
    const size_t total = m->h_flags[0];
    if (!xyz_out || cap == 0) return (int64_t)total;
    const bool want_n = nrm_out && mode == LOM_EXPORT_FULL;
    if ((rc = ensure(m, m->scr[S_IN_XYZ], total * 12)) != LOM_OK) return rc;
    if (want_n && (rc = ensure(m, m->scr[S_IN_NRM], total * 12)) != LOM_OK) return rc;
    const size_t work = (size_t)nv * m->K;
    hipLaunchKernelGGL(k_export_write, dim3(blocks_for(work)), dim3(kThreads), 0, m->stream, off, m->slabs.count, nv,
                       m->K, mode, m->slabs.pts, m->slabs.nrm, m->scr[S_IN_XYZ].as<float>(),
                       want_n ? m->scr[S_IN_NRM].as<float>() : (float *)nullptr);
    LOM_HIP(m, hipGetLastError());
    const size_t take = std::min(total, cap);
    LOM_HIP(m, hipMemcpyAsync(xyz_out, m->scr[S_IN_XYZ].p, take * 12, hipMemcpyDeviceToHost, m->stream));
    if (want_n) LOM_HIP(m, hipMemcpyAsync(nrm_out, m->scr[S_IN_NRM].p, take * 12, hipMemcpyDeviceToHost, m->stream));
    LOM_HIP(m, hipStreamSynchronize(m->stream));
    return (int64_t)total;
}

}  // extern "C"

// ---- the carve's erase for a decision made elsewhere (lom_internal.hpp; vote.hip) ---------------------------------------
namespace lom {

int map_settle_nvox(lom_map *m) { return refresh_nvox(m); }

int erase_begin(lom_map *m, uint32_t **keep)
{
    int rc;
    const uint32_t nv = m->n_vox;
    *keep = nullptr;
    if (nv) {
        uint32_t *newid = nullptr, *scan_tmp = nullptr;
        if ((rc = scratch(m, S_FLAG, (size_t)nv * 2, keep)) != LOM_OK) return rc;
        if ((rc = scratch(m, S_RANK, (size_t)nv * 2, &newid)) != LOM_OK) return rc;
        if ((rc = scratch(m, S_SCAN, scan_tmp_words(nv), &scan_tmp)) != LOM_OK) return rc;
    }
    // keep / newid go where a cleanup scan armed behind an align may have left its own: that scan is never taken now
    m->spec_inflight = false;
    ++m->call_seq;
    m->mutations++;
    return LOM_OK;
}

int erase_rank(lom_map *m, const uint32_t **d_kept)
{
    *d_kept = d_word(m, 4);
    return scan_exclusive(m, m->scr[S_FLAG].as<uint32_t>(), m->scr[S_RANK].as<uint32_t>(), m->n_vox, d_word(m, 4),
                          m->scr[S_SCAN].as<uint32_t>());
}

int erase_finish(lom_map *m, uint32_t n_keep) { return erase_unkept(m, m->n_vox, n_keep); }

}  // namespace lom
