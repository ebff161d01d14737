// Scan archive and map assembly: clouds kept in HBM in their own sensor frame, and K of them at K f64 poses put into one
// map by one call.  Definitions: include/lidar_odometry_amd.h ("scan archive and map assembly"); kernels: k_assemble.hpp;
// host planning (checks, quaternion to R, offsets, grids): assemble_host.cpp; DESIGN.md 7h.
// New code beside the map path: the insert is the map's own (lom_map_add_points_device), and no default path launches
// any of this.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "archive_internal.hpp"
#include "assemble_host.hpp"
#include "k_assemble.hpp"
#include "lom_internal.hpp"

using namespace lom;
using assemble::ScanEntry;

// (the handle itself: archive_internal.hpp)

namespace {

thread_local std::string g_archive_create_error;

// room for `need` points: geometric growth, the stored clouds copied device to device in stream order
int reserve_points(lom_archive *a, uint64_t need)
{
    if (need <= a->cap_points && a->xyz.p) return LOM_OK;
    const uint64_t cap = std::max<uint64_t>(std::max(need, a->cap_points * 2), 1);
    DeviceBuf nx, nn;
    if (alloc(nx, cap * 12) != hipSuccess || alloc(nn, cap * 12) != hipSuccess) return fail(a, LOM_ERR_OOM, "hipMalloc (scan archive)");
    hipError_t e = hipSuccess;
    if (a->points) {
        e = hipMemcpyAsync(nx.p, a->xyz.p, a->points * 12, hipMemcpyDeviceToDevice, a->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nn.p, a->nrm.p, a->points * 12, hipMemcpyDeviceToDevice, a->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(a->stream);  // the old blocks are freed below
    if (e != hipSuccess) return fail(a, LOM_ERR_HIP, "growing the scan archive", e);
    a->xyz = std::move(nx), a->nrm = std::move(nn), a->cap_points = cap;
    return LOM_OK;
}

bool stride_ok(size_t stride) { return stride >= 12 && (stride & 3) == 0; }

// a new scan from `xyz` / `nrm` (records of `stride` bytes, host or device memory by `kind`; nrm NULL: zeros are stored);
// the archive's lock is held
int64_t add_scan(lom_archive *a, const float *xyz, const float *nrm, size_t n, size_t stride, hipMemcpyKind kind)
{
    if (a->points + n > assemble::kArchiveMaxPoints)
        return fail(a, LOM_ERR_ARG, "more than 2^32 points in one archive (32-bit indices)");
    if (hipSetDevice(a->device) != hipSuccess) return fail(a, LOM_ERR_HIP, "hipSetDevice");
    if (n) {
        int rc = reserve_points(a, a->points + n);
        if (rc != LOM_OK) return rc;
        float *dx = a->d_xyz() + a->points * 3, *dn = a->d_nrm() + a->points * 3;
        if (stride == 12) {
            LOM_HIP(a, hipMemcpyAsync(dx, xyz, n * 12, kind, a->stream));
            if (nrm) LOM_HIP(a, hipMemcpyAsync(dn, nrm, n * 12, kind, a->stream));
        } else {
            LOM_HIP(a, hipMemcpy2DAsync(dx, 12, xyz, stride, 12, n, kind, a->stream));
            if (nrm) LOM_HIP(a, hipMemcpy2DAsync(dn, 12, nrm, stride, 12, n, kind, a->stream));
        }
        if (!nrm) LOM_HIP(a, hipMemsetAsync(dn, 0, n * 12, a->stream));
        // the caller's buffers are its own again when the call returns
        LOM_HIP(a, hipStreamSynchronize(a->stream));
    }
    a->table.push_back(ScanEntry{a->points, (uint32_t)n});
    a->points += n;
    return (int64_t)a->table.size() - 1;
}

// the two host forms (nrm NULL: lom_archive_add_points); the lock is taken here
int64_t add_host(lom_archive *a, const float *xyz, const float *nrm, size_t n, size_t stride)
{
    std::lock_guard<std::mutex> lk(a->lock);
    for (size_t i = 0; i < n; i++) {
        const float *p = reinterpret_cast<const float *>(reinterpret_cast<const char *>(xyz) + i * stride);
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]))
            return fail(a, LOM_ERR_ARG, ("point " + std::to_string(i) + " has a coordinate that is not finite").c_str());
    }
    return add_scan(a, xyz, nrm, n, stride, hipMemcpyHostToDevice);
}

// the two device forms
int64_t add_device(lom_archive *a, const float *d_xyz, const float *d_nrm, size_t n, size_t stride, void *hip_event_or_null)
{
    std::lock_guard<std::mutex> lk(a->lock);
    if (hip_event_or_null) {
        LOM_HIP(a, hipSetDevice(a->device));
        LOM_HIP(a, hipStreamWaitEvent(a->stream, (hipEvent_t)hip_event_or_null, 0));
    }
    return add_scan(a, d_xyz, d_nrm, n, stride, hipMemcpyDeviceToDevice);
}

template <bool kCull>
int launch_transform(lom_archive *a, const assemble::Plan &plan, const lom_assemble_params *p, float r2)
{
    const size_t count = plan.scans.size();
    for (size_t c0 = 0; c0 < count; c0 += assemble::kAsmScansPerLaunch) {
        const uint32_t ny = (uint32_t)std::min<size_t>(assemble::kAsmScansPerLaunch, count - c0);
        hipLaunchKernelGGL(k_asm_transform<kCull>, dim3(plan.grid_x, ny), dim3(kAsmThreads), 0, a->stream,
                           a->desc.as<const AsmScan>() + c0, a->d_xyz(), a->d_nrm(), a->stage_xyz.as<float>(),
                           a->stage_nrm.as<float>(), kCull ? p->centre[0] : 0.f, kCull ? p->centre[1] : 0.f,
                           kCull ? p->centre[2] : 0.f, r2, a->counts.as<uint32_t>());
        LOM_HIP(a, hipGetLastError());
    }
    return LOM_OK;
}

}  // namespace

extern "C" {

int lom_archive_create(int device, size_t point_hint, size_t scan_hint, lom_archive **out)
{
    if (!out) return LOM_ERR_ARG;
    *out = nullptr;
    if ((uint64_t)point_hint > assemble::kArchiveMaxPoints || scan_hint > assemble::kAsmMaxScans)
        return create_fail(g_archive_create_error, LOM_ERR_ARG, "point_hint <= 2^32, scan_hint <= 2^24");
    if (const int rc = check_device(device, g_archive_create_error); rc != LOM_OK) return rc;
    lom_archive *a = new (std::nothrow) lom_archive();
    if (!a) return create_fail(g_archive_create_error, LOM_ERR_OOM, "host allocation");
    a->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&a->ready_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&a->done_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = alloc(a->h_word, 64, hipHostMallocDefault);
    int rc = e == hipSuccess ? LOM_OK : create_fail(g_archive_create_error, LOM_ERR_HIP, "scan archive setup", e);
    if (rc == LOM_OK) {
        rc = reserve_points(a, std::max<size_t>(point_hint, 1));
        if (rc != LOM_OK) g_archive_create_error = a->error;
    }
    if (rc != LOM_OK) {
        lom_archive_destroy(a);
        return rc;
    }
    a->table.reserve(scan_hint);
    *out = a;
    return LOM_OK;
}

void lom_archive_destroy(lom_archive *a)
{
    if (!a) return;
    (void)hipSetDevice(a->device);
    if (a->stream) (void)hipStreamSynchronize(a->stream);
    if (a->ready_ev) (void)hipEventDestroy(a->ready_ev);
    if (a->done_ev) (void)hipEventDestroy(a->done_ev);
    if (a->stream) (void)hipStreamDestroy(a->stream);
    delete a;  // the buffers go with it
}

const char *lom_archive_last_error(const lom_archive *a) { return a ? a->error.c_str() : g_archive_create_error.c_str(); }

int lom_archive_clear(lom_archive *a)
{
    if (!a) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(a->lock);
    a->table.clear();
    a->points = 0;
    return LOM_OK;
}

void *lom_archive_stream(lom_archive *a) { return a ? (void *)a->stream : nullptr; }
int lom_archive_device(const lom_archive *a) { return a ? a->device : LOM_ERR_ARG; }

int lom_archive_wait_event(lom_archive *a, void *hip_event)
{
    if (!a || !hip_event) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(a->lock);
    LOM_HIP(a, hipSetDevice(a->device));
    LOM_HIP(a, hipStreamWaitEvent(a->stream, (hipEvent_t)hip_event, 0));
    return LOM_OK;
}

int64_t lom_archive_add(lom_archive *a, const float *xyz, const float *nrm, size_t n, size_t stride)
{
    if (!a || (n && (!xyz || !nrm)) || !stride_ok(stride)) return LOM_ERR_ARG;
    return add_host(a, xyz, nrm, n, stride);
}

int64_t lom_archive_add_points(lom_archive *a, const float *xyz, size_t n, size_t stride)
{
    if (!a || (n && !xyz) || !stride_ok(stride)) return LOM_ERR_ARG;
    return add_host(a, xyz, nullptr, n, stride);
}

int64_t lom_archive_add_device(lom_archive *a, const float *d_xyz, const float *d_nrm, size_t n, size_t stride,
                               void *hip_event_or_null)
{
    if (!a || (n && (!d_xyz || !d_nrm)) || !stride_ok(stride)) return LOM_ERR_ARG;
    return add_device(a, d_xyz, d_nrm, n, stride, hip_event_or_null);
}

int64_t lom_archive_add_points_device(lom_archive *a, const float *d_xyz, size_t n, size_t stride, void *hip_event_or_null)
{
    if (!a || (n && !d_xyz) || !stride_ok(stride)) return LOM_ERR_ARG;
    return add_device(a, d_xyz, nullptr, n, stride, hip_event_or_null);
}

int64_t lom_archive_scan_count(const lom_archive *a)
{
    if (!a) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(const_cast<lom_archive *>(a)->lock);
    return (int64_t)a->table.size();
}

int64_t lom_archive_point_count(const lom_archive *a)
{
    if (!a) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(const_cast<lom_archive *>(a)->lock);
    return (int64_t)a->points;
}

int64_t lom_archive_scan_size(const lom_archive *a, int64_t id)
{
    if (!a) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(const_cast<lom_archive *>(a)->lock);
    if (id < 0 || id >= (int64_t)a->table.size()) return fail(const_cast<lom_archive *>(a), LOM_ERR_ARG, "no scan with this id");
    return (int64_t)a->table[(size_t)id].n;
}

int64_t lom_archive_get(lom_archive *a, int64_t id, float *xyz_out, float *nrm_out, size_t cap)
{
    if (!a) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(a->lock);
    if (id < 0 || id >= (int64_t)a->table.size()) return fail(a, LOM_ERR_ARG, "no scan with this id");
    const ScanEntry e = a->table[(size_t)id];
    const size_t n = std::min<size_t>(e.n, cap);
    if (n && (xyz_out || nrm_out)) {
        LOM_HIP(a, hipSetDevice(a->device));
        if (xyz_out) LOM_HIP(a, hipMemcpyAsync(xyz_out, a->d_xyz() + e.offset * 3, n * 12, hipMemcpyDeviceToHost, a->stream));
        if (nrm_out) LOM_HIP(a, hipMemcpyAsync(nrm_out, a->d_nrm() + e.offset * 3, n * 12, hipMemcpyDeviceToHost, a->stream));
        LOM_HIP(a, hipStreamSynchronize(a->stream));
    }
    return (int64_t)e.n;
}

int lom_map_assemble(lom_map *m, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses, size_t count,
                     const lom_assemble_params *params, lom_assemble_stats *stats)
{
    if (!m || !a) return LOM_ERR_ARG;
    std::lock_guard<std::mutex> lk(a->lock);
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (m->parent) return fail(a, LOM_ERR_ARG, "a scan context has no map of its own");
    if (m->device != a->device) return fail(a, LOM_ERR_ARG, "the map and the archive live on different devices");
    bool cull = false;
    std::string why;
    int rc = assemble::cull_of(params, &cull, why);
    assemble::Plan plan;
    if (rc == LOM_OK) rc = assemble::plan(a->table.data(), a->table.size(), ids, poses, count, plan, why);
    if (rc != LOM_OK) return fail(a, rc, why.c_str());
    lom_assemble_stats st;
    std::memset(&st, 0, sizeof st);
    st.scans = (int64_t)count;
    st.points_in = st.points_kept = (int64_t)plan.points_in;
    auto fail_map = [&](int code) { return fail(a, code, (std::string("map: ") + lom_last_error(m)).c_str()); };
    if (stats) {
        st.voxels_before = lom_map_size(m);
        if (st.voxels_before < 0) return fail_map((int)st.voxels_before);
    }
    size_t kept = (size_t)plan.points_in;
    if (kept) {
        LOM_HIP(a, hipSetDevice(a->device));
        // (kept != 0: there is a scan, a point and a block, so none of the seven requests below is for zero bytes)
        const size_t desc_bytes = count * sizeof(AsmScan), cloud_bytes = kept * 12;
        if ((rc = ensure(a, a->desc, desc_bytes)) != LOM_OK) return rc;
        if ((rc = ensure(a, a->stage_xyz, cloud_bytes)) != LOM_OK) return rc;
        if ((rc = ensure(a, a->stage_nrm, cloud_bytes)) != LOM_OK) return rc;
        if (cull) {
            if ((rc = ensure(a, a->counts, (size_t)plan.blocks * 4)) != LOM_OK) return rc;
            if ((rc = ensure(a, a->offsets, ((size_t)plan.blocks + 1) * 4)) != LOM_OK) return rc;
            if ((rc = ensure(a, a->out_xyz, cloud_bytes)) != LOM_OK) return rc;
            if ((rc = ensure(a, a->out_nrm, cloud_bytes)) != LOM_OK) return rc;
        }
        if ((rc = ensure_pinned(a, a->h_desc, desc_bytes, std::max(desc_bytes + desc_bytes / 2, (size_t)1 << 16), hipHostMallocDefault,
                                "hipHostMalloc (assembly descriptors)")) != LOM_OK)
            return rc;
        // the previous call's insert has read the staging before this call writes it
        if (a->done_recorded) LOM_HIP(a, hipStreamWaitEvent(a->stream, a->done_ev, 0));
        std::memcpy(a->h_desc.h, plan.scans.data(), desc_bytes);
        LOM_HIP(a, hipMemcpyAsync(a->desc.p, a->h_desc.h, desc_bytes, hipMemcpyHostToDevice, a->stream));
        const float *cloud_xyz = a->stage_xyz.as<const float>(), *cloud_nrm = a->stage_nrm.as<const float>();
        if (!cull) {
            if ((rc = launch_transform<false>(a, plan, params, 0.f)) != LOM_OK) return rc;
        } else {
            const float r2 = params->radius * params->radius;
            if ((rc = launch_transform<true>(a, plan, params, r2)) != LOM_OK) return rc;
            hipLaunchKernelGGL(k_asm_offsets, dim3(1), dim3(kAsmOffsetThreads), 0, a->stream, a->counts.as<const uint32_t>(),
                               plan.blocks, a->offsets.as<uint32_t>());
            LOM_HIP(a, hipGetLastError());
            for (size_t c0 = 0; c0 < count; c0 += assemble::kAsmScansPerLaunch) {
                const uint32_t ny = (uint32_t)std::min<size_t>(assemble::kAsmScansPerLaunch, count - c0);
                hipLaunchKernelGGL(k_asm_compact, dim3(plan.grid_x, ny), dim3(kAsmThreads), 0, a->stream,
                                   a->desc.as<const AsmScan>() + c0, cloud_xyz, cloud_nrm, params->centre[0], params->centre[1],
                                   params->centre[2], r2, a->offsets.as<const uint32_t>(), a->out_xyz.as<float>(),
                                   a->out_nrm.as<float>());
                LOM_HIP(a, hipGetLastError());
            }
            // the one read-back before the insert: its size
            LOM_HIP(a, hipMemcpyAsync(a->h_word.h, a->offsets.as<const uint32_t>() + plan.blocks, 4, hipMemcpyDeviceToHost, a->stream));
            LOM_HIP(a, hipStreamSynchronize(a->stream));
            kept = a->h_word.as<uint32_t>()[0];
            cloud_xyz = a->out_xyz.as<const float>(), cloud_nrm = a->out_nrm.as<const float>();
        }
        st.points_kept = (int64_t)kept;
        if (kept) {
            LOM_HIP(a, hipEventRecord(a->ready_ev, a->stream));
            LOM_HIP(a, hipStreamWaitEvent(m->stream, a->ready_ev, 0));
            rc = lom_map_add_points_device(m, cloud_xyz, cloud_nrm, kept, 12);  // atomic: all of the cloud or nothing
            LOM_HIP(a, hipEventRecord(a->done_ev, m->stream));
            a->done_recorded = true;
            if (rc != LOM_OK) return fail_map(rc);
        }
    }
    if (stats) {
        st.voxels_after = lom_map_size(m);
        st.points_stored_after = lom_map_point_count(m);
        if (st.voxels_after < 0) return fail_map((int)st.voxels_after);
        if (st.points_stored_after < 0) return fail_map((int)st.points_stored_after);
        *stats = st;
    }
    return LOM_OK;
}

}  // extern "C"
