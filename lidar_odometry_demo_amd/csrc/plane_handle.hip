// The host core of a planning grid's handle (plane_handle.hpp): what the seven planning families all own and do around
// their kernels.  No kernel is launched here.
#include "plane_handle.hpp"

namespace lom {

int plane_setup(PlaneHandle *h, std::string &slot, const char *setup_text, int n_in)
{
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->done_ev, hipEventDisableTiming);
    for (int k = 0; k < n_in; k++)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&h->in_ev[k], hipEventDisableTiming);
    return e == hipSuccess ? LOM_OK : create_fail(slot, LOM_ERR_HIP, setup_text, e);
}

void plane_destroy(PlaneHandle *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (hipEvent_t ev : {h->done_ev, h->in_ev[0], h->in_ev[1], h->in_ev[2]})
        if (ev) (void)hipEventDestroy(ev);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;  // the buffers go with it, the family's too
}

const char *plane_last_error(const PlaneHandle *h, const std::string &slot) { return h ? h->error.c_str() : slot.c_str(); }

int plane_get_geometry(const PlaneHandle *h, lom_occupancy_geometry *out)
{
    if (!h || !out) return LOM_ERR_ARG;
    *out = h->geo;
    return LOM_OK;
}

void *plane_stream(PlaneHandle *h) { return h ? (void *)h->stream : nullptr; }
int plane_device(const PlaneHandle *h) { return h ? h->device : LOM_ERR_ARG; }

int plane_wait_event(PlaneHandle *h, void *hip_event)
{
    if (!h || !hip_event) return LOM_ERR_ARG;
    LOM_HIP(h, hipSetDevice(h->device));
    LOM_HIP(h, hipStreamWaitEvent(h->stream, (hipEvent_t)hip_event, 0));
    return LOM_OK;
}

int plane_copy_out(PlaneHandle *h, void *out, const DeviceBuf &buf, size_t n_bytes)
{
    if (!n_bytes) return LOM_OK;
    LOM_HIP(h, hipSetDevice(h->device));
    LOM_HIP(h, hipMemcpyAsync(out, buf.p, n_bytes, hipMemcpyDeviceToHost, h->stream));
    LOM_HIP(h, hipStreamSynchronize(h->stream));
    return LOM_OK;
}

// the producer's geometry `g` against `want`, then its device against the handle's: the two texts of the hand-off, once
static int check_producer(PlaneHandle *h, const char *consumer, const char *producer, const lom_occupancy_geometry &g,
                          const lom_occupancy_geometry &want, const char *differs_tail, int device)
{
    const std::string head = std::string(consumer) + ": the " + producer;
    if (!same_geometry(g, want)) return fail(h, LOM_ERR_ARG, (head + "'s resolution, origin, width or height differs" + differs_tail).c_str());
    if (device != h->device) return fail(h, LOM_ERR_ARG, (head + " lives on another device").c_str());
    return LOM_OK;
}

int plane_check_producer(PlaneHandle *h, const char *consumer, const char *producer, const lom_occupancy_geometry &g, int device)
{
    return check_producer(h, consumer, producer, g, h->geo, "", device);
}

int plane_shifted_geometry(PlaneHandle *h, const char *name, int32_t dx, int32_t dy, lom_occupancy_geometry *out)
{
    // (the handle's geometry passed its create, so the rule can only refuse the new origin)
    if (const int rc = plane::shift_geometry(&h->geo, dx, dy, out); rc != LOM_OK)
        return fail(h, rc, (std::string(name) + ": shift: the origin moved by (dx, dy) cells is not finite").c_str());
    return LOM_OK;
}

int plane_fail_producer(PlaneHandle *h, const char *consumer, const char *call, const char *producer_error)
{
    return fail(h, LOM_ERR_HIP, (std::string(consumer) + ": " + call + ": " + producer_error).c_str());
}

int plane_read_behind(PlaneHandle *h, int k, void *producer_stream)
{
    LOM_HIP(h, hipEventRecord(h->in_ev[k], (hipStream_t)producer_stream));
    LOM_HIP(h, hipStreamWaitEvent(h->stream, h->in_ev[k], 0));
    return LOM_OK;
}

int plane_source_check(PlaneHandle *h, const char *consumer, const PlaneSource &s, const lom_occupancy_geometry &g, const char *differs_tail)
{
    if (!s.clearance) return LOM_OK;
    lom_occupancy_geometry cg{};
    (void)lom_clearance_get_geometry(s.clearance, &cg);
    return check_producer(h, consumer, "clearance grid", cg, g, differs_tail, lom_clearance_device(s.clearance));
}

int plane_source_open(PlaneHandle *h, const char *consumer, const PlaneSource &s, const int8_t **d_plane)
{
    *d_plane = s.device;
    if (s.event) LOM_HIP(h, hipStreamWaitEvent(h->stream, (hipEvent_t)s.event, 0));
    if (!s.clearance) return LOM_OK;
    if (lom_clearance_cost_device(s.clearance, d_plane) != LOM_OK || !*d_plane)
        return plane_fail_producer(h, consumer, "lom_clearance_cost_device", lom_clearance_last_error(s.clearance));
    return plane_read_behind(h, 0, lom_clearance_stream(s.clearance));
}

int plane_source_close(PlaneHandle *h, const char *consumer, const PlaneSource &s)
{
    if (!s.clearance) return LOM_OK;
    return plane_release(h, consumer, s.clearance, lom_clearance_wait_event, "lom_clearance_wait_event");
}

}  // namespace lom
