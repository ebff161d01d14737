// Device-resident voxel map: the MI355X counterpart of the reference's
// VoxelGrid container (src/voxel_grid.h:17-257) and VoxelWithPlanes payload
// (src/voxel_with_planes.h:10-36).
//
//   addCloud / addCloudWithoutNormals (:77-110)  -> lom_map_add_points[_device]   (map_insert.hip)
//   radiusCleanup (:236-246)                     -> lom_map_radius_cleanup        (map_erase.hip)
//   getCloud / getCloudWithoutNormals /
//   getSparseCloudWithoutNormals (:112-162)      -> lom_map_export                (map_cloud.hip)
//   setVoxelSize / setMaxPoints / size (:56-66, :248-251)                         (here)
//
// The reference inserts serially; a voxel keeps the first max_points points in
// call order and that order is the nearest-neighbour tie-break order.  The
// insert is data-parallel but a pure function of the input order:
// hash slots are claimed with a 64-bit CAS (which voxel gets which slot does
// not matter), creation order comes from a prefix scan over "first point of a
// new voxel" flags, and a point's position inside its voxel is its rank among
// the batch's points of that voxel by input index -- no result depends on the
// order in which atomics land.
//
// Built with -ffp-contract=off: the f32 index and distance expressions must
// round like the reference's (plain -O3 x86-64 build, no FMA contraction).
//
// This file is the map's core: table and slabs, the status words and their read-back, the settle / pending / redo
// protocol, the scan service, host staging, and the entries that are only state.  It is the one translation unit that
// instantiates and launches the kernels of k_table.hpp and k_scan.hpp.  The operations are map_insert.hip,
// map_erase.hip, map_carve.hip and map_cloud.hip (map_internal.hpp: who owns what).  Handles, scan contexts and
// options are handle.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "grid_scan.hpp"
#include "k_scan.hpp"
#include "k_table.hpp"
#include "lom_internal.hpp"
#include "map_internal.hpp"

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
// table and slabs
// ---------------------------------------------------------------------------
uint32_t next_pow2(uint64_t v)
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

int rehash(lom_map *m, uint32_t new_cap)
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

int table_rebuild(lom_map *m, uint32_t n_vox)
{
    const MapView v = view_of(m);
    hipLaunchKernelGGL(k_table_init, dim3(blocks_for(m->cap)), dim3(kThreads), 0, m->stream, m->d_table, m->cap);
    if (n_vox) {
        hipLaunchKernelGGL(k_rebuild, dim3(blocks_for(n_vox)), dim3(kThreads), 0, m->stream, m->d_table, v.mask,
                           v.shift, m->slabs.key, m->slabs.count, n_vox);
    }
    LOM_HIP(m, hipGetLastError());
    return LOM_OK;
}

void slabs_free(Slabs &s)
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
int slabs_alloc(lom_map *m, uint32_t cap, Slabs &s)
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

int ensure_slabs(lom_map *m, uint64_t want)
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

// grow-only scratch that is kept at rest (every byte == fill) between calls: a fresh allocation is
// filled once; whoever dirties a word puts it back
int ensure_rest(lom_map *m, DeviceBuf &b, size_t bytes, int fill)
{
    if (bytes <= b.bytes) return LOM_OK;
    const int rc = ensure(m, b, bytes);
    if (rc != LOM_OK) return rc;
    LOM_HIP(m, hipMemsetAsync(b.p, fill, b.bytes, m->stream));
    return LOM_OK;
}

// ---------------------------------------------------------------------------
// device words to the host
// ---------------------------------------------------------------------------
hipError_t launch_gather_words(lom_map *m, const uint32_t *const *ptrs, int n, size_t offset, uint32_t tag)
{
    WordPtrs w;
    for (int i = 0; i < 32; i++) w.p[i] = i < n ? ptrs[i] : nullptr;
    hipLaunchKernelGGL(k_gather_words, dim3(1), dim3(64), 0, m->stream, w, n,
                       reinterpret_cast<unsigned long long *>((char *)m->d_report + offset), tag);
    return hipGetLastError();
}

WordsPoll poll_words(lom_map *m, size_t offset, uint32_t tag, int n, uint32_t *out, hipError_t *err)
{
    volatile unsigned long long *hw = reinterpret_cast<volatile unsigned long long *>((char *)m->h_report + offset);
    uint64_t spins = 0;
    for (int i = 0; i < n; i++) {
        while ((uint32_t)(hw[i] >> 32) != tag) {
            __builtin_ia32_pause();
            if ((++spins & 0x3FFF) != 0) continue;
            const hipError_t e = hipStreamQuery(m->stream);
            if (e == hipSuccess) {
                if ((uint32_t)(hw[i] >> 32) == tag) break;
                return WORDS_MISSING;
            }
            if (e != hipErrorNotReady) {
                *err = e;
                return WORDS_STREAM_FAILED;
            }
        }
        out[i] = (uint32_t)hw[i];
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return WORDS_ARRIVED;
}

int gather_words_begin(lom_map *m, const uint32_t *const *ptrs, int n)
{
    m->words_pending = 0;
    if (n <= 0) return LOM_OK;
    if (++m->words_tag == 0) m->words_tag = 1;  // the block starts zeroed: 0 is "nothing yet"
    const hipError_t e = launch_gather_words(m, ptrs, n, kWordsOffset, m->words_tag);
    if (e != hipSuccess) return fail(m, LOM_ERR_HIP, "hipGetLastError()", e);
    m->words_pending = n;
    return LOM_OK;
}

int gather_words_end(lom_map *m, uint32_t *out)
{
    const int n = m->words_pending;
    m->words_pending = 0;
    hipError_t e = hipSuccess;
    switch (poll_words(m, kWordsOffset, m->words_tag, n, out, &e)) {
    case WORDS_MISSING: return fail(m, LOM_ERR_HIP, "device words did not arrive");
    case WORDS_STREAM_FAILED: return fail(m, LOM_ERR_HIP, "stream failed while reading device words", e);
    default: return LOM_OK;
    }
}

int gather_words(lom_map *m, const uint32_t *const *ptrs, int n, uint32_t *out)
{
    const int rc = gather_words_begin(m, ptrs, n);
    return rc != LOM_OK ? rc : gather_words_end(m, out);
}

int read_words(lom_map *m, MapWord first, MapWord last, WordsRead *out)
{
    const uint32_t *ptrs[8];
    const int n = last - first + 1;
    for (int i = 0; i < n; i++) ptrs[i] = d_word(m, MapWord(first + i));
    out->first = first;
    return gather_words(m, ptrs, n, out->v);
}

// ---------------------------------------------------------------------------
// settle / pending / redo
// ---------------------------------------------------------------------------
int refresh_nvox(lom_map *m)
{
    int rc = resolve_pending(m);
    if (rc != LOM_OK) return rc;
    if (!m->n_vox_stale) return LOM_OK;
    WordsRead r;
    rc = read_words(m, MW_NVOX, MW_NVOX, &r);
    if (rc != LOM_OK) return rc;
    m->n_vox = r[MW_NVOX];
    m->n_vox_ub = m->n_vox;
    m->n_vox_stale = false;
    return LOM_OK;
}

uint32_t take_test_fail_from(lom_map *m)
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
int map_status(lom_map *m)
{
    // range error, voxel counter, grid give-up, bulk insert sent back: three of them sequence numbers of failed calls
    WordsRead r;
    int rc = read_words(m, MW_RANGE, MW_BULK_BACK, &r);
    if (rc != LOM_OK) return rc;
    const uint32_t checked = m->status_seq;
    m->status_seq = m->call_seq;
    // (a cleanup scan behind an align that gave up is no call of the user's: taken, the cleanup redoes it; not taken, or
    // not yet, its number in MW_GRID is skipped below)
    peek_cleanup_behind_align(m);
    if (m->n_vox_stale) {
        m->n_vox = r[MW_NVOX];
        m->n_vox_ub = m->n_vox;
        m->n_vox_stale = false;
    }
    const uint32_t range_seq = r[MW_RANGE];
    const size_t pending = m->pending_n;
    m->pending_n = 0;  // the last single-pass / bulk insert is through, one way or the other
    // a bulk insert with a partition beyond k_bi_group's LDS wrote nothing: the four-kernel path redoes it, like a
    // single-pass insert whose scan gave up
    const uint32_t grid_seq = (pending && r[MW_BULK_BACK] == m->pending_seq) ? r[MW_BULK_BACK] : r[MW_GRID];
    if (grid_seq > checked && grid_seq != m->grid_resolved_seq && grid_seq != m->spec_gave_up_seq) {
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
    WordsRead r;
    int rc = read_words(m, MW_GRID, MW_BULK_BACK, &r);  // scan gave up / bulk insert sent back
    if (rc != LOM_OK) return rc;
    const size_t n = m->pending_n;
    m->pending_n = 0;
    if (r[MW_GRID] != m->pending_seq && r[MW_BULK_BACK] != m->pending_seq) return LOM_OK;
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
    // status / counter words + the block aggregates of the single-pass kernels (256 x 2 granules): map_words.hpp
    int rc = ensure(m, m->scr[S_MISC], kMapWordsBytes + 256 * 2 * sizeof(Granule));
    if (rc == LOM_OK) {
        if (hipMemsetAsync(m->scr[S_MISC].p, 0, m->scr[S_MISC].bytes, m->stream) != hipSuccess) rc = LOM_ERR_HIP;
    }
    if (rc == LOM_OK) rc = table_alloc(m, m->min_cap, &m->d_table);
    if (rc == LOM_OK) m->cap = m->min_cap;
    if (rc == LOM_OK && hipStreamSynchronize(m->stream) != hipSuccess) rc = LOM_ERR_HIP;
    return rc;
}

// An insert whose verdict nobody has read yet: should its in-kernel scan have given up (single-pass) or a partition have
// been too large (bulk), lom_map_status() / whoever consumes the map next redoes it -- the caller keeps the input valid
// until then.  pending_n is what other threads read (resolve_pending's fast path): it is stored last.
void set_pending(lom_map *m, const char *d_xyz, const char *d_nrm, size_t n, size_t stride, uint32_t seq)
{
    m->pending_xyz = d_xyz;
    m->pending_nrm = d_nrm;
    m->pending_stride = stride;
    m->pending_seq = seq;
    m->pending_n = n;
}

// the insert's kernels are enqueued: the table has keys, the voxel count is the device's to know
void note_insert_enqueued(lom_map *m, uint64_t worst)
{
    m->table_clean = false;
    m->n_vox_ub = (uint32_t)std::min<uint64_t>(worst, 0xFFFFFFFFull);
    m->n_vox_stale = true;
}

// ---------------------------------------------------------------------------
// the scan service
// ---------------------------------------------------------------------------
size_t scan_tmp_words(uint32_t n)
{
    size_t w = 0;
    while (n > (uint32_t)kScanTile) {
        n = (n + kScanTile - 1) / kScanTile;
        w += 2 * (size_t)n;
    }
    return w + 16;
}

int scan_u32(lom_map *m, const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *d_total, uint32_t *tmp)
{
    return scan_exclusive<uint32_t>(m, in, out, n, d_total, tmp);
}

int scan_u64(lom_map *m, const unsigned long long *in, unsigned long long *out, uint32_t n, unsigned long long *d_total,
             unsigned long long *tmp)
{
    return scan_exclusive<unsigned long long>(m, in, out, n, d_total, tmp);
}

// ---------------------------------------------------------------------------
// host staging
// ---------------------------------------------------------------------------
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

int stage_host_points(lom_map *m, const float *xyz, const float *nrm, size_t n, size_t stride,
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

}  // namespace lom

using namespace lom;

// ---------------------------------------------------------------------------
// C ABI: the entries that are only state
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
        LOM_HIP(m, hipMemsetAsync(d_word(m, MW_NVOX), 0, 4, m->stream));
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

int lom_map_status(lom_map *m)
{
    if (!m) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    return map_status(m);
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
    *d_range = d_word(m, MW_RANGE);
    *d_grid = d_word(m, MW_GRID);
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

}  // extern "C"
