// The core every device handle shares (device_handle.hpp): the device checks of a create, allocation into DeviceBuf /
// PinnedBuf and their grow-only ensure / ensure_pinned.  Then what the map handle owns besides a map, and nothing that
// launches a kernel: scan uploads, device queries, stream and pinned blocks (handle_setup), scan contexts (lom_scan_*:
// creation, destruction and the forwarders to the lom_match_* entries of match.hip, align.hip, align_batch.hip and
// quality_report.hip), lom_map_create / destroy and the run-time switches.  What these need from the map side -- the
// first table, settling a pending insert, freeing table and slabs -- are lom:: functions of voxel_map.hip
// (lom_internal.hpp).
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "lom_internal.hpp"

namespace lom {

// ---------------------------------------------------------------------------
// the handle core (device_handle.hpp)
// ---------------------------------------------------------------------------
static thread_local std::string g_create_error;
std::string &map_create_error() { return g_create_error; }

int check_device(int device, std::string &slot, bool name_device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return create_fail(slot, LOM_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    }
    if (device < 0 || device >= ndev) return create_fail(slot, LOM_ERR_ARG, "device index out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return create_fail(slot, LOM_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::string s = "kernels are built for gfx950 only";
        if (name_device) s = std::string("device is ") + prop.gcnArchName + ", " + s;
        return create_fail(slot, LOM_ERR_NO_DEVICE, s.c_str());
    }
    return LOM_OK;
}

hipError_t alloc(DeviceBuf &b, size_t bytes)
{
    const hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return e;
    }
    b.bytes = bytes;
    return hipSuccess;
}

hipError_t alloc(PinnedBuf &b, size_t bytes, unsigned flags)
{
    hipError_t e = hipHostMalloc(&b.h, bytes, flags);
    if (e != hipSuccess) b.h = nullptr;
    if (e == hipSuccess && (flags & hipHostMallocMapped)) e = hipHostGetDevicePointer(&b.d, b.h, 0);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        release(b);
        return e;
    }
    b.bytes = bytes;
    return hipSuccess;
}

int ensure(DeviceHandle *h, DeviceBuf &b, size_t bytes)
{
    if (bytes <= b.bytes) return LOM_OK;
    const size_t nb = grown_bytes(b.bytes, bytes);
    if (b.p) {
        LOM_HIP(h, hipStreamSynchronize(h->stream));
        release(b);
    }
    const hipError_t e = alloc(b, nb);
    return e == hipSuccess ? LOM_OK : fail(h, LOM_ERR_OOM, "hipMalloc", e);
}

int ensure_pinned(DeviceHandle *h, PinnedBuf &b, size_t need, size_t grow_to, unsigned flags, const char *what, bool *fresh)
{
    if (fresh) *fresh = false;
    if (b.h && need <= b.bytes) return LOM_OK;
    LOM_HIP(h, hipStreamSynchronize(h->stream));
    release(b);
    const hipError_t e = alloc(b, grow_to, flags);
    if (e != hipSuccess) return fail(h, LOM_ERR_OOM, what, e);
    if (fresh) *fresh = true;
    return LOM_OK;
}

static inline size_t scan_bytes(size_t n, size_t stride) { return n ? (n - 1) * stride + 12 : 0; }

int upload_scan(lom_map *m, DeviceBuf &buf, const void *src, size_t n, size_t stride, const char **d_src)
{
    const size_t bytes = scan_bytes(n, stride);
    const int rc = ensure(m, buf, std::max<size_t>(bytes, 16));
    if (rc != LOM_OK) return rc;
    if (bytes) LOM_HIP(m, hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, m->stream));
    *d_src = buf.as<const char>();
    return LOM_OK;
}

int upload_distinct(lom_map *m, DeviceBuf &buf, const HostCloud *clouds, int count, const char **d_src)
{
    struct Distinct {
        HostCloud c;
        size_t off;
    };
    std::vector<Distinct> distinct;
    std::vector<size_t> off((size_t)count);
    size_t total = 0;
    for (int i = 0; i < count; i++) {
        const HostCloud &c = clouds[i];
        off[i] = total;
        if (!c.n) continue;
        // (many problems on one cloud hit it at once: the newest is looked at first)
        size_t k = distinct.size();
        while (k-- > 0)
            if (distinct[k].c.p == c.p && distinct[k].c.n == c.n && distinct[k].c.stride == c.stride) break;
        if (k != (size_t)-1) {
            off[i] = distinct[k].off;
            continue;
        }
        distinct.push_back(Distinct{c, total});
        total += (scan_bytes(c.n, c.stride) + 255) & ~size_t(255);
    }
    const int rc = ensure(m, buf, std::max<size_t>(total, 256));
    if (rc != LOM_OK) return rc;
    for (const Distinct &d : distinct)
        LOM_HIP(m, hipMemcpyAsync(buf.as<char>() + d.off, d.c.p, scan_bytes(d.c.n, d.c.stride), hipMemcpyHostToDevice, m->stream));
    for (int i = 0; i < count; i++) d_src[i] = buf.as<const char>() + off[i];
    return LOM_OK;
}

}  // namespace lom

using namespace lom;

extern "C" {

int lom_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int lom_device_local_cpus(int device, char *out, size_t cap)
{
    // CPUs of the NUMA node the GPU hangs off: /sys/bus/pci/devices/<bdf>/local_cpulist.  The align
    // is a chain of host<->device round trips over PCIe; a caller running on the far socket pays
    // for it (measured: 0.47 ms instead of 0.33 ms per C2 frame).  The caller decides what to do
    // with the list (bench.py pins itself to it).
    if (!out || cap < 2) return LOM_ERR_ARG;
    out[0] = 0;
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess) {
        (void)hipGetLastError();
        return LOM_ERR_NO_DEVICE;
    }
    for (char *c = bdf; *c; c++) *c = (char)tolower(*c);
    std::string path = std::string("/sys/bus/pci/devices/") + bdf + "/local_cpulist";
    FILE *f = std::fopen(path.c_str(), "r");
    if (!f) return LOM_ERR_STATE;
    const bool ok = std::fgets(out, (int)cap, f) != nullptr;
    std::fclose(f);
    if (!ok) return LOM_ERR_STATE;
    for (char *c = out; *c; c++)
        if (*c == '\n') *c = 0;
    return LOM_OK;
}

const char *lom_last_error(const lom_map *m) { return m ? m->error.c_str() : g_create_error.c_str(); }

// what every handle owns besides a map: a stream and the pinned blocks the align talks to the host through
// (part >= 0: the stream runs on partition `part` of `nparts` equal slices of the device's compute units)
static hipError_t create_stream(lom_map *m, int part, int nparts)
{
    if (part < 0) return hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking);
    int cus = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m->device);
    if (e != hipSuccess) return e;
    // Bit i of the mask is the device's i-th compute unit in the driver's enumeration, which deals consecutive bits
    // round-robin over the XCDs: a contiguous range of bits is the same number of CUs on every XCD.
    const uint32_t lo = (uint32_t)((uint64_t)cus * (uint32_t)part / (uint32_t)nparts);
    const uint32_t hi = (uint32_t)((uint64_t)cus * ((uint32_t)part + 1u) / (uint32_t)nparts);
    // What the slice holds AT ONCE of a grid whose workgroups wait for each other (k_lm): the dispatcher deals workgroups
    // round-robin over the 8 XCDs and, inside an XCD, over its 4 shader engines, whatever the mask says; a slice of c CUs
    // has at least floor(c / 32) of them in each of the 32 (XCD, engine) pairs, so that many workgroups per pair always find
    // a CU.  2, 4, 8 slices: 128, 64, 32 (all of the slice); 3 slices: 64 of 85; 5, 6, 7 slices: 32 of 51, 42, 36 -- with
    // the whole 42 counted, a solve of 42 workgroups found one pair short and waited out its patience on every align.
    constexpr uint32_t kDispatchPairs = 32;
    uint32_t usable = hi - lo;
    if ((uint32_t)cus % kDispatchPairs == 0u && usable >= kDispatchPairs) usable = usable / kDispatchPairs * kDispatchPairs;
    std::vector<uint32_t> mask(((size_t)cus + 31) / 32, 0u);
    for (uint32_t c = lo; c < hi; c++) mask[c >> 5] |= 1u << (c & 31);
    e = hipExtStreamCreateWithCUMask(&m->own_stream, (uint32_t)mask.size(), mask.data());
    if (e == hipSuccess) m->partition_cus = std::max(usable, 1u);
    return e;
}

static int handle_setup(lom_map *m, int part = -1, int nparts = 1)
{
    constexpr unsigned kMapped = hipHostMallocMapped | hipHostMallocCoherent;
    hipError_t e;
    if ((e = hipSetDevice(m->device)) != hipSuccess || (e = create_stream(m, part, nparts)) != hipSuccess ||
        (e = alloc(m->pin_results, 1024 * sizeof(double), hipHostMallocDefault)) != hipSuccess ||
        (e = alloc(m->pin_flags, 64 * sizeof(uint32_t), hipHostMallocDefault)) != hipSuccess ||
        (e = alloc(m->pin_mail, 64 * 32 * sizeof(double), kMapped)) != hipSuccess ||
        (e = alloc(m->pin_cmd, 256, kMapped)) != hipSuccess || (e = alloc(m->pin_report, 1024, kMapped)) != hipSuccess)
        return create_fail(g_create_error, LOM_ERR_HIP, "handle setup", e);
    m->stream = m->own_stream;
    m->h_results = m->pin_results.as<double>();
    m->h_flags = m->pin_flags.as<uint32_t>();
    m->h_mail = m->pin_mail.as<double>(), m->d_mail = static_cast<double *>(m->pin_mail.d);
    m->h_cmd = m->pin_cmd.h, m->d_cmd = m->pin_cmd.d;
    m->h_report = m->pin_report.h, m->d_report = m->pin_report.d;
    std::memset(m->h_mail, 0, 64 * 32 * sizeof(double));
    std::memset(m->h_cmd, 0, 256);
    std::memset(m->h_report, 0, 1024);
    return LOM_OK;
}

// ---- scan contexts ---------------------------------------------------------------------------------------------
// The reference's search and align take the grid by const reference (voxel_grid.h:164,206; cloud_matcher.h:15-16):
// any number of callers may align against one keyframe at a time.  A context is a handle without a map of its own
// -- stream, per-scan buffers, solve state, report block -- whose kernels read the keyframe's table and slabs.
int lom_scan_create(lom_map *map, lom_scan **out) { return lom_scan_create_on_partition(map, -1, 1, out); }

int lom_scan_create_on_partition(lom_map *map, int part, int nparts, lom_scan **out)
{
    if (!map || !out) return LOM_ERR_ARG;
    *out = nullptr;
    if (part >= 0 && (nparts < 1 || nparts > 8 || part >= nparts))
        return fail(map, LOM_ERR_ARG, "partition index / count: 0 <= part < nparts <= 8");
    if (map->parent) return fail(map, LOM_ERR_ARG, "a scan context cannot be the keyframe of another");
    LOM_HIP(map, hipSetDevice(map->device));
    // settles a pending insert (nothing mutates the keyframe while contexts read it)
    const int rc = settle_map(map);
    if (rc != LOM_OK) return rc;
    lom_map *c = new (std::nothrow) lom_map();
    if (!c) return fail(map, LOM_ERR_OOM, "host allocation");
    c->device = map->device;
    c->parent = map;
    c->opt_host_lm = map->opt_host_lm;
    c->opt_debug_lm = map->opt_debug_lm;
    c->opt_debug_timing = map->opt_debug_timing;
    c->opt_no_temporal = map->opt_no_temporal;
    c->opt_count = map->opt_count;
    c->opt_replay_fold = map->opt_replay_fold;
    c->patience_ticks = map->patience_ticks;
    if (handle_setup(c, part, nparts) != LOM_OK) {
        map->error = g_create_error;
        lom_map_destroy(c);
        return LOM_ERR_HIP;
    }
    *out = reinterpret_cast<lom_scan *>(c);
    return LOM_OK;
}

static lom_map *as_map(lom_scan *s) { return reinterpret_cast<lom_map *>(s); }

void lom_scan_destroy(lom_scan *s) { lom_map_destroy(as_map(s)); }
const char *lom_scan_last_error(const lom_scan *s) { return s ? reinterpret_cast<const lom_map *>(s)->error.c_str() : ""; }
int lom_scan_set_option(lom_scan *s, int option, int64_t value) { return lom_map_set_option(as_map(s), option, value); }
int lom_scan_set_stream(lom_scan *s, void *hip_stream) { return lom_map_set_stream(as_map(s), hip_stream); }
void *lom_scan_get_stream(lom_scan *s) { return lom_map_get_stream(as_map(s)); }
// cast-and-forward to the lom_match_* entry of the same name, one macro per signature shape
#define LOM_SCAN_ALIGN(name)                                                                                              \
    int lom_scan_##name(lom_scan *s, const float *src, size_t n, size_t stride, const float guess_t[3],                  \
                        const float guess_q[4], float out_t[3], float out_q[4], lom_align_stats *stats)                  \
    {                                                                                                                     \
        return lom_match_##name(as_map(s), src, n, stride, guess_t, guess_q, out_t, out_q, stats);                        \
    }
#define LOM_SCAN_ALIGN_BATCH(name)                                                                                        \
    int lom_scan_##name(lom_scan *s, const lom_align_problem *p, int count, lom_align_result *out, int *best)            \
    {                                                                                                                     \
        return lom_match_##name(as_map(s), p, count, out, best);                                                          \
    }
#define LOM_SCAN_FIND_PAIRS(name, dist_t)                                                                                 \
    int64_t lom_scan_##name(lom_scan *s, const float *src, size_t n, size_t stride, const float t[3], const float q[4],  \
                            dist_t max_dist, lom_correspondence *out)                                                     \
    {                                                                                                                     \
        return lom_match_##name(as_map(s), src, n, stride, t, q, max_dist, out);                                          \
    }
#define LOM_SCAN_QUALITY(name)                                                                                            \
    int lom_scan_##name(lom_scan *s, const float *src, size_t n, size_t stride, const float t[3], const float q[4],      \
                        float max_dist, float min_eig_t, float min_eig_r, lom_quality_report *out, float *residual_out)  \
    {                                                                                                                     \
        return lom_match_##name(as_map(s), src, n, stride, t, q, max_dist, min_eig_t, min_eig_r, out, residual_out);      \
    }
#define LOM_SCAN_QUALITY_SUMS(name)                                                                                       \
    int lom_scan_##name(lom_scan *s, const lom_quality_problem *p, int count, float max_dist, double *sums_out)          \
    {                                                                                                                     \
        return lom_match_##name(as_map(s), p, count, max_dist, sums_out);                                                 \
    }
#define LOM_SCAN_QUALITY_BATCH(name)                                                                                      \
    int lom_scan_##name(lom_scan *s, const lom_quality_problem *p, int count, float max_dist, float min_eig_t,           \
                        float min_eig_r, lom_quality_report *out, int *best)                                              \
    {                                                                                                                     \
        return lom_match_##name(as_map(s), p, count, max_dist, min_eig_t, min_eig_r, out, best);                          \
    }
LOM_SCAN_ALIGN(align)
LOM_SCAN_ALIGN(align_device)
LOM_SCAN_ALIGN_BATCH(align_batch)
LOM_SCAN_ALIGN_BATCH(align_batch_device)
LOM_SCAN_FIND_PAIRS(find_pairs, float)
LOM_SCAN_FIND_PAIRS(find_pairs_sq, double)
LOM_SCAN_QUALITY(quality)
LOM_SCAN_QUALITY(quality_device)
LOM_SCAN_QUALITY_SUMS(quality_batch_sums)
LOM_SCAN_QUALITY_SUMS(quality_batch_sums_device)
LOM_SCAN_QUALITY_BATCH(quality_batch)
LOM_SCAN_QUALITY_BATCH(quality_batch_device)
int lom_scan_align_repeat(lom_scan *s, const float *d_src, size_t n, size_t stride, const float guess_t[3],
                          const float guess_q[4], int reps, float out_t[3], float out_q[4], lom_align_stats *total)
{
    return lom_match_align_repeat(as_map(s), d_src, n, stride, guess_t, guess_q, reps, out_t, out_q, total);
}

int lom_map_create(float voxel_size, size_t max_points, size_t capacity_hint, int device, lom_map **out)
{
    if (!out) return LOM_ERR_ARG;
    *out = nullptr;
    if (!(voxel_size > 0.f) || max_points == 0 || max_points > 65535)
        return create_fail(g_create_error, LOM_ERR_ARG, "voxel_size must be > 0 and 1 <= max_points <= 65535");
    if (const int rc = check_device(device, g_create_error, true); rc != LOM_OK) return rc;
    lom_map *m = new (std::nothrow) lom_map();
    if (!m) return create_fail(g_create_error, LOM_ERR_OOM, "host allocation");
    m->device = device;
    m->voxel_size = voxel_size;
    m->K = (uint32_t)max_points;
    m->max_points = m->K;
    // the environment is looked at here and nowhere on the align path (lom_map_set_option changes the switches later)
    m->opt_host_lm = getenv("LOM_HOST_LM") != nullptr;
    if (const char *e = getenv("LOM_TABLE_SLOTS_PER_VOXEL")) m->table_slots_per_voxel = (uint32_t)std::min(256, std::max(2, atoi(e)));
    m->opt_debug_lm = getenv("LOM_DEBUG_LM") != nullptr;
    m->opt_debug_lm_twice = getenv("LOM_DEBUG_LM_TWICE") != nullptr;
    m->opt_debug_timing = getenv("LOM_DEBUG_TIMING") != nullptr;
    m->opt_no_temporal = getenv("LOM_NO_TEMPORAL") != nullptr;
    if (const char *e = getenv("LOM_COUNT_CANDIDATES")) m->opt_count = atoi(e) != 0;
    m->opt_no_bulk = getenv("LOM_NO_BULK_INSERT") != nullptr;
    m->opt_dense_cleanup = getenv("LOM_DENSE_CLEANUP") != nullptr;
    if (const char *e = getenv("LOM_BULK_PPT")) m->bulk_ppt = (uint32_t)atoi(e);  // development: points per thread of k_bi_claim
    if (handle_setup(m) != LOM_OK) {
        lom_map_destroy(m);
        return LOM_ERR_HIP;
    }
    const int rc = map_init(m, capacity_hint);
    if (rc != LOM_OK) {
        g_create_error = m->error.empty() ? "map setup failed" : m->error;
        lom_map_destroy(m);
        return rc;
    }
    *out = m;
    return LOM_OK;
}

void lom_map_destroy(lom_map *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->server_alive && m->h_cmd) {  // a resident evaluation server leaves on op = 2 (stop)
        unsigned long long *w = reinterpret_cast<unsigned long long *>(m->h_cmd);
        reinterpret_cast<unsigned int *>(w + 1)[0] = 2u;
        __atomic_store_n(w, ++m->mail_seq, __ATOMIC_RELEASE);
        m->server_alive = false;
    }
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->comm || m->host_comm) lom_comm_finalize(m);
    map_free(m);
    for (hipEvent_t e : {m->stage_ev, m->parent_ev, m->multi_ev})
        if (e) (void)hipEventDestroy(e);
    for (auto &e : m->prof_events)
        if (e) (void)hipEventDestroy(e);
    if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
    delete m;  // the buffers go with it
}

int lom_map_set_stream(lom_map *m, void *hip_stream)
{
    if (!m) return LOM_ERR_ARG;
    (void)hipSetDevice(m->device);
    LOM_HIP(m, hipStreamSynchronize(m->stream));
    m->stream = hip_stream ? (hipStream_t)hip_stream : m->own_stream;
    return LOM_OK;
}

int lom_map_set_profiling(lom_map *m, int period)
{
    if (!m || period < 0) return LOM_ERR_ARG;
    m->profile_period = period;
    m->profiling = false;
    m->align_count = 0;
    return LOM_OK;
}

int lom_map_set_option(lom_map *m, int option, int64_t value)
{
    if (!m) return LOM_ERR_ARG;
    switch (option) {
    case LOM_OPT_HOST_LM: m->opt_host_lm = value != 0; return LOM_OK;
    case LOM_OPT_DEVICE_PATIENCE_TICKS:
        if (value < 1) return LOM_ERR_ARG;
        m->patience_ticks = (unsigned long long)value;
        return LOM_OK;
    case LOM_OPT_DEBUG_LM_STAMPS: m->opt_debug_lm = value != 0; return LOM_OK;
    case LOM_OPT_DEBUG_TIMING: m->opt_debug_timing = value != 0; return LOM_OK;
    case LOM_OPT_NO_TEMPORAL_BOUND: m->opt_no_temporal = value != 0; return LOM_OK;
    case LOM_OPT_COUNT_CANDIDATES: m->opt_count = value != 0; return LOM_OK;
    case LOM_OPT_NO_BULK_INSERT: m->opt_no_bulk = value != 0; return LOM_OK;
    case LOM_OPT_REPLAY_FOLD: m->opt_replay_fold = value != 0; return LOM_OK;
    case LOM_OPT_TEST_BULK_PARTITION_MAX:
        if (value < 0 || value > (int64_t)kBiPartMax) return LOM_ERR_ARG;
        m->test_bulk_part_max = (uint32_t)value;
        return LOM_OK;
    case LOM_OPT_TEST_GIVE_UP_AT_OUTER:
        if (value < -1 || value >= 35) return LOM_ERR_ARG;
        m->test_give_up_outer = (int)value;
        return LOM_OK;
    case LOM_OPT_TEST_GRID_GIVE_UP:
        if (value < -1 || value >= (1 << 20)) return LOM_ERR_ARG;
        m->test_grid_give_up = (int)value;
        return LOM_OK;
    case LOM_OPT_TEST_BATCH_ROUND_MAX:
        if (value < 0 || value > (1 << 20)) return LOM_ERR_ARG;
        m->batch.test_round_max = (int)value;
        return LOM_OK;
    case LOM_OPT_TEST_QUALITY_ROUND_MAX:
        if (value < 0 || value > (1 << 20)) return LOM_ERR_ARG;
        m->qualb.test_round_max = (int)value;
        return LOM_OK;
    case LOM_OPT_TEST_VOTE_SLICE_MAX:
        if (value < 0 || value > 64) return LOM_ERR_ARG;
        m->vote.test_slice_max = (uint32_t)value;
        return LOM_OK;
    default: return fail(m, LOM_ERR_ARG, "unknown option");
    }
}

void *lom_map_get_stream(lom_map *m) { return m ? (void *)m->stream : nullptr; }

}  // extern "C"
