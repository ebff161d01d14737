// The host core of a posed-scan grid handle (grid_handle.hpp): what lom_occupancy and lom_elevation both own and do
// around their kernels.  No kernel is launched here.
#include "grid_handle.hpp"

namespace lom {

int grid_setup(GridHandle *g, std::string &slot, const char *setup_text, const char *oom_text)
{
    hipError_t e = hipSetDevice(g->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&g->done_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = alloc(g->h_words, 64, hipHostMallocDefault);
    if (e != hipSuccess) return create_fail(slot, LOM_ERR_HIP, setup_text, e);
    return alloc(g->words, 64) == hipSuccess ? LOM_OK : create_fail(slot, LOM_ERR_OOM, oom_text);
}

void grid_destroy(GridHandle *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    if (g->done_ev) (void)hipEventDestroy(g->done_ev);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;  // the buffers go with it, the family's too
}

int grid_wait_event(GridHandle *g, void *hip_event)
{
    if (!g || !hip_event) return LOM_ERR_ARG;
    LOM_HIP(g, hipSetDevice(g->device));
    LOM_HIP(g, hipStreamWaitEvent(g->stream, (hipEvent_t)hip_event, 0));
    return LOM_OK;
}

int grid_upload_packed(GridHandle *g, const float *xyz, size_t n, size_t stride_bytes)
{
    if (!n) return LOM_OK;
    LOM_HIP(g, hipSetDevice(g->device));
    if (const int rc = ensure(g, g->cloud, n * 12); rc != LOM_OK) return rc;
    if (stride_bytes == 12)
        LOM_HIP(g, hipMemcpyAsync(g->cloud.p, xyz, n * 12, hipMemcpyHostToDevice, g->stream));
    else
        LOM_HIP(g, hipMemcpy2DAsync(g->cloud.p, 12, xyz, stride_bytes, 12, n, hipMemcpyHostToDevice, g->stream));
    return LOM_OK;
}

int grid_stage(GridHandle *g, const std::vector<assemble::AsmScan> &scans, uint32_t n_words)
{
    const size_t desc_bytes = scans.size() * sizeof(assemble::AsmScan);
    if (const int rc = ensure(g, g->desc, desc_bytes); rc != LOM_OK) return rc;
    LOM_HIP(g, hipMemsetAsync(g->words.p, 0, (size_t)n_words * 4, g->stream));
    LOM_HIP(g, hipMemcpyAsync(g->desc.p, scans.data(), desc_bytes, hipMemcpyHostToDevice, g->stream));
    return LOM_OK;
}

int grid_read_words(GridHandle *g, uint32_t n_words, bool record_done)
{
    LOM_HIP(g, hipMemcpyAsync(g->h_words.h, g->words.p, (size_t)n_words * 4, hipMemcpyDeviceToHost, g->stream));
    if (record_done) LOM_HIP(g, hipEventRecord(g->done_ev, g->stream));
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    return LOM_OK;
}

int grid_copy_out(GridHandle *g, int8_t *out, const DeviceBuf &cells, size_t n, uint32_t n_words)
{
    if (n) LOM_HIP(g, hipMemcpyAsync(out, cells.p, n, hipMemcpyDeviceToHost, g->stream));
    return grid_read_words(g, n_words, false);
}

int grid_shift_plan(GridHandle *g, const char *name, const lom_occupancy_geometry &geo, int32_t dx, int32_t dy, GridShift &out)
{
    // (the grid's geometry passed its create, so the rule can only refuse the new origin)
    if (const int rc = plane::shift_geometry(&geo, dx, dy, &out.geo); rc != LOM_OK)
        return fail(g, rc, (std::string(name) + ": shift: the origin moved by (dx, dy) cells is not finite").c_str());
    const int64_t w = geo.width, h = geo.height;
    out.keeps = dx > -w && dx < w && dy > -h && dy < h;
    out.dx = (int32_t)std::max(-w, std::min(w, (int64_t)dx)), out.dy = (int32_t)std::max(-h, std::min(h, (int64_t)dy));
    return LOM_OK;
}

int grid_shift_shadow(GridHandle *g, DeviceBuf &shadow, size_t bytes, const char *oom_text)
{
    if (shadow.p) return LOM_OK;  // (a grid's size never changes)
    return alloc(shadow, bytes) == hipSuccess ? LOM_OK : fail(g, LOM_ERR_OOM, oom_text);
}

int grid_shift_wait(GridHandle *g)
{
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    return LOM_OK;
}

}  // namespace lom
