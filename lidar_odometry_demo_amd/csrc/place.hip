// Place recognition: scan descriptors (a polar height image in the style of Scan Context, Kim and Kim, IROS 2018) and
// a database of them that lives in HBM.  Definitions: include/lidar_odometry_amd.h; kernels: k_place.hpp; DESIGN.md 7e.
// New code beside the align path: nothing here touches a map handle, and no default path launches any of it.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <new>
#include <string>

#include "k_place.hpp"

using namespace lom;

// The database owns its stream, its entries and every buffer below; calls on one database are serialised by `lock`.
struct lom_place_db : DeviceHandle {
    lom_place_params params{};
    std::mutex lock;
    uint64_t size = 0, cap = 0;  // entries; cap is a multiple of kPlaceGroup
    DeviceBuf raw;   // f32 [cap][R][S]
    DeviceBuf unit;  // f32 [cap / 8][S][R][8]
    DeviceBuf mask;  // u64 [cap]
    DeviceBuf acc;   // u32: R * S accumulation words, all zero between calls; then err[2]
    // per-call buffers, grow-only: uploaded clouds; uploaded descriptors; the queries' raw / unit / mask; pairs;
    // distances alone; matches
    DeviceBuf cloud, stage, q_raw, q_unit, q_mask, pairs, alld, match;
#ifdef LOM_PLACE_TUNE  // the measuring build of tools/place_throughput.py only (make tune): E = 1, 2, 4 beside the shipped 8
    int query_entries = kPlaceGroup;  // LOM_PLACE_QUERY_ENTRIES at create: entries per LDS read
#endif

    float *d_raw() const { return raw.as<float>(); }
    float *d_unit() const { return unit.as<float>(); }
    unsigned long long *d_mask() const { return mask.as<unsigned long long>(); }
    uint32_t *d_acc() const { return acc.as<uint32_t>(); }
    uint32_t *d_err() const { return d_acc() + (size_t)params.rings * params.sectors; }
};

namespace {

thread_local std::string g_place_create_error;

bool params_ok(const lom_place_params *p)
{
    return p && p->rings >= 1 && p->rings <= (uint32_t)kPlaceMaxDim && p->sectors >= 1 &&
           p->sectors <= (uint32_t)kPlaceMaxDim && std::isfinite(p->max_range) && p->max_range > 0.f &&
           std::isfinite(p->z_floor);
}

bool cloud_args_ok(const void *xyz, size_t n, size_t stride)
{
    return (n == 0 || xyz) && stride >= 12 && (stride & 3) == 0 && n < 0x7FFFFFFFull;
}

size_t cells_of(const lom_place_db *db) { return (size_t)db->params.rings * db->params.sectors; }

PlaceShape shape_of(const lom_place_db *db)
{
    PlaceShape sh;
    sh.R = db->params.rings;
    sh.S = db->params.sectors;
    sh.ring_width = (double)db->params.max_range / (double)db->params.rings;
    sh.sector_width = 6.283185307179586476925286766559 / (double)db->params.sectors;
    sh.z_floor = db->params.z_floor;
    return sh;
}

// room for `need` entries: geometric growth; the entries move on the database's stream, ids and bytes stay
int reserve_entries(lom_place_db *db, uint64_t need)
{
    if (need <= db->cap) return LOM_OK;
    uint64_t cap = std::max<uint64_t>(need, db->cap * 2);
    cap = (cap + kPlaceGroup - 1) / kPlaceGroup * kPlaceGroup;
    const size_t rs = cells_of(db);
    DeviceBuf raw, unit, mask;
    if (alloc(raw, cap * rs * 4) != hipSuccess || alloc(unit, cap * rs * 4) != hipSuccess || alloc(mask, cap * 8) != hipSuccess)
        return fail(db, LOM_ERR_OOM, "hipMalloc (database entries)");
    hipError_t e = hipMemsetAsync(unit.p, 0, cap * rs * 4, db->stream);  // a group's unused places are read, never reported
    if (e == hipSuccess) e = hipMemsetAsync(mask.p, 0, cap * 8, db->stream);
    if (db->cap) {
        if (e == hipSuccess) e = hipMemcpyAsync(raw.p, db->raw.p, db->cap * rs * 4, hipMemcpyDeviceToDevice, db->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(unit.p, db->unit.p, db->cap * rs * 4, hipMemcpyDeviceToDevice, db->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(mask.p, db->mask.p, db->cap * 8, hipMemcpyDeviceToDevice, db->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
    if (e != hipSuccess) return fail(db, LOM_ERR_HIP, "growing the database", e);
    db->raw = std::move(raw), db->unit = std::move(unit), db->mask = std::move(mask), db->cap = cap;  // the old blocks go
    return LOM_OK;
}

// a descriptor from the host: every value finite and >= 0
bool descriptor_ok(const float *d, size_t count)
{
    for (size_t i = 0; i < count; i++)
        if (!(d[i] >= 0.f) || !std::isfinite(d[i])) return false;
    return true;
}

// d_xyz -> accumulation words (enqueued)
int enqueue_bin(lom_place_db *db, const void *d_xyz, size_t n, size_t stride)
{
    if (!n) return LOM_OK;
    const uint32_t blocks = (uint32_t)std::min<size_t>((n + kPlaceBinThreads - 1) / kPlaceBinThreads, 1024);
    hipLaunchKernelGGL(k_place_bin, dim3(blocks), dim3(kPlaceBinThreads), 0, db->stream, (const char *)d_xyz, stride, (uint32_t)n,
                       shape_of(db), db->d_acc(), db->d_err());
    LOM_HIP(db, hipGetLastError());
    return LOM_OK;
}

// `count` descriptors from src (accumulation words, or uploaded raw descriptors) into the database's slots from
// `first_slot` (grouped) or into the query slots (plain)
int enqueue_finish(lom_place_db *db, uint32_t *src, bool from_acc, uint32_t count, float *dst_raw, float *dst_unit,
                   unsigned long long *dst_mask, uint64_t first_slot, bool grouped)
{
    hipLaunchKernelGGL(k_place_finish, dim3(count), dim3(64), 0, db->stream, src, db->params.rings, db->params.sectors,
                       from_acc ? 1 : 0, dst_raw, dst_unit, dst_mask, first_slot, grouped ? 1 : 0, db->d_err());
    LOM_HIP(db, hipGetLastError());
    return LOM_OK;
}

int ensure_query_slots(lom_place_db *db, size_t q)
{
    int rc = ensure(db, db->q_raw, q * cells_of(db) * 4);
    if (rc == LOM_OK) rc = ensure(db, db->q_unit, q * cells_of(db) * 4);
    if (rc == LOM_OK) rc = ensure(db, db->q_mask, q * 8);
    return rc;
}

template <int E>
void launch_query(lom_place_db *db, uint32_t tiles, uint32_t q, uint64_t id_begin, uint64_t id_end, float *all_dist)
{
    const size_t lds = (size_t)db->params.rings * 2 * db->params.sectors * 4;  // <= 32 KB
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_place_query<E>), dim3(tiles, q), dim3(kPlaceQueryWaves * 64), lds, db->stream,
                       (const float *)db->d_unit(), (const unsigned long long *)db->d_mask(), db->q_unit.as<const float>(),
                       db->q_mask.as<const unsigned long long>(), db->params.rings, db->params.sectors, id_begin, id_end,
                       db->pairs.as<PlacePair>(), all_dist);
}

void empty_matches(lom_place_match *out, size_t count)
{
    for (size_t i = 0; i < count; i++) {
        out[i].id = -1;
        out[i].distance = std::numeric_limits<float>::infinity();
        out[i].shift = 0u;
    }
}

// the q descriptors in the query slots against [id_begin, id_end): pairs, top k, the copies back (enqueued)
int enqueue_search(lom_place_db *db, uint32_t q, int64_t id_begin, int64_t id_end, int k, lom_place_match *out,
                   float *all_dist)
{
    const uint64_t n = (uint64_t)(id_end - id_begin);
    int rc = ensure(db, db->pairs, (size_t)q * n * sizeof(PlacePair));
    if (rc == LOM_OK) rc = ensure(db, db->match, (size_t)q * k * sizeof(PlaceMatch));
    if (rc == LOM_OK && all_dist) rc = ensure(db, db->alld, (size_t)q * n * 4);
    if (rc != LOM_OK) return rc;
    const uint64_t base = (uint64_t)id_begin / kPlaceGroup * kPlaceGroup;
    const uint32_t tiles = (uint32_t)(((uint64_t)id_end - base + kPlaceTile - 1) / kPlaceTile);
    float *d_all = all_dist ? db->alld.as<float>() : nullptr;
#ifdef LOM_PLACE_TUNE
    switch (db->query_entries) {
    case 1: launch_query<1>(db, tiles, q, (uint64_t)id_begin, (uint64_t)id_end, d_all); break;
    case 2: launch_query<2>(db, tiles, q, (uint64_t)id_begin, (uint64_t)id_end, d_all); break;
    case 4: launch_query<4>(db, tiles, q, (uint64_t)id_begin, (uint64_t)id_end, d_all); break;
    default: launch_query<kPlaceGroup>(db, tiles, q, (uint64_t)id_begin, (uint64_t)id_end, d_all); break;
    }
#else
    launch_query<kPlaceGroup>(db, tiles, q, (uint64_t)id_begin, (uint64_t)id_end, d_all);
#endif
    LOM_HIP(db, hipGetLastError());
    hipLaunchKernelGGL(k_place_topk, dim3(q), dim3(kPlaceTopkThreads), 0, db->stream, db->pairs.as<const PlacePair>(), (uint32_t)n,
                       (uint64_t)id_begin, k, db->match.as<PlaceMatch>());
    LOM_HIP(db, hipGetLastError());
    LOM_HIP(db, hipMemcpyAsync(out, db->match.p, (size_t)q * k * sizeof(PlaceMatch), hipMemcpyDeviceToHost, db->stream));
    if (all_dist) LOM_HIP(db, hipMemcpyAsync(all_dist, d_all, (size_t)q * n * 4, hipMemcpyDeviceToHost, db->stream));
    return LOM_OK;
}

bool range_ok(const lom_place_db *db, int64_t id_begin, int64_t id_end)
{
    return id_begin >= 0 && id_begin <= id_end && (uint64_t)id_end <= db->size && id_end - id_begin < 0x7FFFFFFFll;
}

// host cloud -> the cloud buffer (enqueued)
int upload_cloud(lom_place_db *db, const void *xyz, size_t n, size_t stride)
{
    if (!n) return LOM_OK;
    const size_t bytes = (n - 1) * stride + 12;
    const int rc = ensure(db, db->cloud, bytes);
    if (rc != LOM_OK) return rc;
    LOM_HIP(db, hipMemcpyAsync(db->cloud.p, xyz, bytes, hipMemcpyHostToDevice, db->stream));
    return LOM_OK;
}

// A call that failed between k_place_bin and k_place_finish leaves points in the accumulation words (and perhaps the
// error word): put them back to rest, so that the next call starts clean.  Error path only.
int fail_at_rest(lom_place_db *db, int rc)
{
    (void)hipGetLastError();
    if (hipMemsetAsync(db->d_acc(), 0, (cells_of(db) + 2) * 4, db->stream) != hipSuccess ||
        hipStreamSynchronize(db->stream) != hipSuccess)
        (void)hipGetLastError();
    return rc;
}

// the error word of the last k_place_finish that emptied the accumulation words, with the stream's work done
int wait_and_check(lom_place_db *db, bool check_points)
{
    uint32_t status = 0;
    if (check_points) LOM_HIP(db, hipMemcpyAsync(&status, db->d_err() + 1, 4, hipMemcpyDeviceToHost, db->stream));
    LOM_HIP(db, hipStreamSynchronize(db->stream));
    if (status) return fail(db, LOM_ERR_RANGE, "a point of the cloud is not finite");
    return LOM_OK;
}

int describe_impl(lom_place_db *db, const void *xyz, size_t n, size_t stride, bool on_device, float *desc_out)
{
    if (!db || !desc_out || !cloud_args_ok(xyz, n, stride)) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> g(db->lock);
    LOM_HIP(db, hipSetDevice(db->device));
    int rc = ensure_query_slots(db, 1);
    if (rc == LOM_OK && !on_device) rc = upload_cloud(db, xyz, n, stride);
    if (rc == LOM_OK) rc = enqueue_bin(db, on_device ? xyz : db->cloud.p, n, stride);
    if (rc == LOM_OK)
        rc = enqueue_finish(db, db->d_acc(), true, 1, db->q_raw.as<float>(), db->q_unit.as<float>(),
                            db->q_mask.as<unsigned long long>(), 0, false);
    if (rc != LOM_OK) return fail_at_rest(db, rc);
    LOM_HIP(db, hipMemcpyAsync(desc_out, db->q_raw.p, cells_of(db) * 4, hipMemcpyDeviceToHost, db->stream));
    return wait_and_check(db, true);  // on LOM_ERR_RANGE desc_out holds no descriptor
}

int64_t add_cloud_impl(lom_place_db *db, const void *xyz, size_t n, size_t stride, bool on_device)
{
    if (!db || !cloud_args_ok(xyz, n, stride)) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> g(db->lock);
    LOM_HIP(db, hipSetDevice(db->device));
    int rc = reserve_entries(db, db->size + 1);
    if (rc == LOM_OK && !on_device) rc = upload_cloud(db, xyz, n, stride);
    if (rc == LOM_OK) rc = enqueue_bin(db, on_device ? xyz : db->cloud.p, n, stride);
    if (rc == LOM_OK) rc = enqueue_finish(db, db->d_acc(), true, 1, db->d_raw(), db->d_unit(), db->d_mask(), db->size, true);
    if (rc != LOM_OK) return fail_at_rest(db, rc);
    // On LOM_ERR_RANGE k_place_finish has written the slot at `size` all the same; the slot stays beyond `size`, no call
    // reads it (queries and get stop at `size`) and the next add overwrites it whole: nothing is stored.
    if ((rc = wait_and_check(db, true)) != LOM_OK) return rc;
    return (int64_t)db->size++;
}

}  // namespace

extern "C" {

int lom_place_db_create(const lom_place_params *params, int device, size_t capacity_hint, lom_place_db **out)
{
    if (!out) return LOM_ERR_ARG;
    *out = nullptr;
    if (!params_ok(params))
        return create_fail(g_place_create_error, LOM_ERR_ARG, "1 <= rings, sectors <= 64, max_range > 0 and finite, z_floor finite");
    if (const int rc = check_device(device, g_place_create_error); rc != LOM_OK) return rc;
    lom_place_db *db = new (std::nothrow) lom_place_db();
    if (!db) return create_fail(g_place_create_error, LOM_ERR_OOM, "host allocation");
    db->params = *params;
    db->device = device;
#ifdef LOM_PLACE_TUNE
    if (const char *e = getenv("LOM_PLACE_QUERY_ENTRIES")) {
        const int v = atoi(e);
        if (v == 1 || v == 2 || v == 4 || v == 8) db->query_entries = v;
    }
#endif
    const size_t acc_bytes = (cells_of(db) + 2) * 4;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = alloc(db->acc, acc_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(db->d_acc(), 0, acc_bytes, db->stream);  // at rest from here on
    if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
    int rc = e == hipSuccess ? LOM_OK : create_fail(g_place_create_error, LOM_ERR_HIP, "database setup", e);
    if (rc == LOM_OK) {
        rc = reserve_entries(db, std::max<size_t>(capacity_hint, 1));
        if (rc != LOM_OK) g_place_create_error = db->error;
    }
    if (rc != LOM_OK) {
        lom_place_db_destroy(db);
        return rc;
    }
    *out = db;
    return LOM_OK;
}

void lom_place_db_destroy(lom_place_db *db)
{
    if (!db) return;
    (void)hipSetDevice(db->device);
    if (db->stream) (void)hipStreamSynchronize(db->stream);
    if (db->stream) (void)hipStreamDestroy(db->stream);
    delete db;  // the buffers go with it
}

const char *lom_place_db_last_error(const lom_place_db *db) { return db ? db->error.c_str() : g_place_create_error.c_str(); }

int64_t lom_place_db_size(const lom_place_db *db)
{
    if (!db) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> g(const_cast<lom_place_db *>(db)->lock);
    return (int64_t)db->size;
}

int lom_place_db_clear(lom_place_db *db)
{
    if (!db) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> g(db->lock);
    db->size = 0;  // ids start again at 0; the slots are overwritten as entries arrive
    return LOM_OK;
}

int lom_place_db_params(const lom_place_db *db, lom_place_params *out)
{
    if (!db || !out) return LOM_ERR_ARG;
    *out = db->params;
    return LOM_OK;
}

void *lom_place_db_stream(lom_place_db *db) { return db ? (void *)db->stream : nullptr; }
int lom_place_db_device(const lom_place_db *db) { return db ? db->device : LOM_ERR_ARG; }

int lom_place_db_wait_event(lom_place_db *db, void *hip_event)
{
    if (!db || !hip_event) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> g(db->lock);
    LOM_HIP(db, hipSetDevice(db->device));
    LOM_HIP(db, hipStreamWaitEvent(db->stream, (hipEvent_t)hip_event, 0));
    return LOM_OK;
}

int lom_place_describe(lom_place_db *db, const float *xyz, size_t n, size_t stride_bytes, float *desc_out)
{
    return describe_impl(db, xyz, n, stride_bytes, false, desc_out);
}

int lom_place_describe_device(lom_place_db *db, const float *d_xyz, size_t n, size_t stride_bytes, float *desc_out)
{
    return describe_impl(db, d_xyz, n, stride_bytes, true, desc_out);
}

int64_t lom_place_db_add(lom_place_db *db, const float *desc)
{
    if (!db || !desc) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> g(db->lock);
    const size_t rs = cells_of(db);
    if (!descriptor_ok(desc, rs)) return fail(db, LOM_ERR_ARG, "a descriptor value is negative or not finite");
    LOM_HIP(db, hipSetDevice(db->device));
    int rc = reserve_entries(db, db->size + 1);
    if (rc == LOM_OK) rc = ensure(db, db->stage, rs * 4);
    if (rc != LOM_OK) return rc;
    LOM_HIP(db, hipMemcpyAsync(db->stage.p, desc, rs * 4, hipMemcpyHostToDevice, db->stream));
    // the same kernel as a cloud's descriptor goes through: an entry has one origin for its unit form
    if ((rc = enqueue_finish(db, db->stage.as<uint32_t>(), false, 1, db->d_raw(), db->d_unit(), db->d_mask(), db->size, true)) != LOM_OK)
        return rc;
    LOM_HIP(db, hipStreamSynchronize(db->stream));  // `desc` is the caller's again
    return (int64_t)db->size++;
}

int64_t lom_place_db_add_cloud(lom_place_db *db, const float *xyz, size_t n, size_t stride_bytes)
{
    return add_cloud_impl(db, xyz, n, stride_bytes, false);
}

int64_t lom_place_db_add_cloud_device(lom_place_db *db, const float *d_xyz, size_t n, size_t stride_bytes)
{
    return add_cloud_impl(db, d_xyz, n, stride_bytes, true);
}

int lom_place_db_get(lom_place_db *db, int64_t id, float *desc_out)
{
    if (!db || !desc_out) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> g(db->lock);
    if (id < 0 || (uint64_t)id >= db->size) return fail(db, LOM_ERR_ARG, "no entry with this id");
    LOM_HIP(db, hipSetDevice(db->device));
    const size_t rs = cells_of(db);
    LOM_HIP(db, hipMemcpyAsync(desc_out, db->d_raw() + (size_t)id * rs, rs * 4, hipMemcpyDeviceToHost, db->stream));
    LOM_HIP(db, hipStreamSynchronize(db->stream));
    return LOM_OK;
}

int lom_place_db_query(lom_place_db *db, const float *desc, int q, int64_t id_begin, int64_t id_end, int k,
                       lom_place_match *out, float *all_dist)
{
    if (!db || !desc || !out || q < 1 || q > 65535 || k < 1 || k > 64 || id_begin > id_end) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> g(db->lock);
    if (!range_ok(db, id_begin, id_end)) return fail(db, LOM_ERR_ARG, "id range outside the database");
    const size_t rs = cells_of(db);
    if (!descriptor_ok(desc, (size_t)q * rs)) return fail(db, LOM_ERR_ARG, "a descriptor value is negative or not finite");
    if (id_begin == id_end) {  // an empty range is valid: k empty slots per query
        empty_matches(out, (size_t)q * k);
        return LOM_OK;
    }
    LOM_HIP(db, hipSetDevice(db->device));
    int rc = ensure(db, db->stage, (size_t)q * rs * 4);
    if (rc == LOM_OK) rc = ensure_query_slots(db, (size_t)q);
    if (rc != LOM_OK) return rc;
    LOM_HIP(db, hipMemcpyAsync(db->stage.p, desc, (size_t)q * rs * 4, hipMemcpyHostToDevice, db->stream));
    rc = enqueue_finish(db, db->stage.as<uint32_t>(), false, (uint32_t)q, nullptr, db->q_unit.as<float>(),
                        db->q_mask.as<unsigned long long>(), 0, false);
    if (rc == LOM_OK) rc = enqueue_search(db, (uint32_t)q, id_begin, id_end, k, out, all_dist);
    if (rc != LOM_OK) return rc;
    return wait_and_check(db, false);
}

int lom_place_db_query_cloud_device(lom_place_db *db, const float *d_xyz, size_t n, size_t stride_bytes, int64_t id_begin,
                                    int64_t id_end, int k, lom_place_match *out)
{
    if (!db || !out || k < 1 || k > 64 || id_begin > id_end || !cloud_args_ok(d_xyz, n, stride_bytes)) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> g(db->lock);
    if (!range_ok(db, id_begin, id_end)) return fail(db, LOM_ERR_ARG, "id range outside the database");
    LOM_HIP(db, hipSetDevice(db->device));
    int rc = ensure_query_slots(db, 1);
    if (rc == LOM_OK) rc = enqueue_bin(db, d_xyz, n, stride_bytes);
    if (rc == LOM_OK)
        rc = enqueue_finish(db, db->d_acc(), true, 1, nullptr, db->q_unit.as<float>(), db->q_mask.as<unsigned long long>(), 0, false);
    if (rc == LOM_OK && id_begin < id_end) rc = enqueue_search(db, 1, id_begin, id_end, k, out, nullptr);
    if (rc != LOM_OK) return fail_at_rest(db, rc);
    if ((rc = wait_and_check(db, true)) != LOM_OK) {
        empty_matches(out, (size_t)k);
        return rc;
    }
    if (id_begin == id_end) empty_matches(out, (size_t)k);
    return LOM_OK;
}

double lom_place_shift_yaw(const lom_place_params *params, uint32_t shift)
{
    if (!params_ok(params)) return std::numeric_limits<double>::quiet_NaN();
    const uint32_t S = params->sectors;
    return (double)((S - shift % S) % S) * 6.283185307179586476925286766559 / (double)S;
}

}  // extern "C"
