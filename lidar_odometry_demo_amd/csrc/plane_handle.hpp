// The handle of a planning grid, written once for lom_clearance (clearance.hip), lom_navfield (navfield.hip), lom_regions
// (regions.hip), lom_visibility (visibility.hip), lom_rollout (rollout.hip), lom_navset (navset.hip) and lom_posefield
// (posefield.hip): a dense 2-D grid of one geometry that reads planes other handles leave in HBM on streams of their own.
// What create and destroy do for all seven, the small entry points, the read-back of a buffer, the shift by whole cells,
// the hand-off of a producer's plane between two streams and the three forms in which a cost plane reaches a solver
// (code: plane_handle.hip).  A family keeps its buffers, pinned blocks and options, its refusals, its kernels
// and their launches.  Nothing here launches a kernel.
#pragma once
#include <cstring>
#include <new>
#include <string>

#include "device_handle.hpp"
#include "plane_geometry.hpp"

namespace lom {

// The grid owns its stream and its events, and what the family adds.
struct PlaneHandle : DeviceHandle {
    lom_occupancy_geometry geo{};
    hipEvent_t done_ev = nullptr;                       // recorded behind this handle's reads of a producer's plane
    hipEvent_t in_ev[3] = {nullptr, nullptr, nullptr};  // recorded behind a producer's plane each; a family creates as many as it has producers
    virtual ~PlaneHandle() = default;  // plane_destroy deletes through PlaneHandle *; never through DeviceHandle * (not virtual)

    size_t n_cells() const { return (size_t)geo.width * geo.height; }
};

// bit for bit: 0.0f and -0.0f differ, as do two NaNs of different payload
inline bool same_geometry(const lom_occupancy_geometry &a, const lom_occupancy_geometry &b)
{
    return std::memcmp(&a.resolution, &b.resolution, 4) == 0 && std::memcmp(&a.origin_x, &b.origin_x, 4) == 0 &&
           std::memcmp(&a.origin_y, &b.origin_y, 4) == 0 && a.width == b.width && a.height == b.height;
}

// The common part of a create, on a fresh handle that knows its device: the stream, done_ev and n_in of the in_ev.  A
// failure's text goes to the family's create slot: LOM_ERR_HIP `setup_text`.
int plane_setup(PlaneHandle *h, std::string &slot, const char *setup_text, int n_in);
void plane_destroy(PlaneHandle *h);  // NULL: nothing
// the small entry points; h NULL: the create slot, LOM_ERR_ARG or nullptr, as the public header says per family
const char *plane_last_error(const PlaneHandle *h, const std::string &slot);
int plane_get_geometry(const PlaneHandle *h, lom_occupancy_geometry *out);
void *plane_stream(PlaneHandle *h);
int plane_device(const PlaneHandle *h);
int plane_wait_event(PlaneHandle *h, void *hip_event);
// n_bytes of a device buffer to the caller, then the wait (nothing of either for no bytes)
int plane_copy_out(PlaneHandle *h, void *out, const DeviceBuf &buf, size_t n_bytes);

// ---- the hand-off of a producer's plane -------------------------------------------------------------------------------
// `consumer` heads every text ("clearance", "navigation field", "region grid", "visibility grid"); `producer` is
// "occupancy grid", "elevation grid", "clearance grid" or "navigation field".
// The refusals in front of it: LOM_ERR_ARG and "<consumer>: the <producer>'s resolution, origin, width or height differs"
// or "<consumer>: the <producer> lives on another device", else LOM_OK.  (A caller that words the device's refusal itself
// passes its own device.)
int plane_check_producer(PlaneHandle *h, const char *consumer, const char *producer, const lom_occupancy_geometry &g, int device);
// LOM_ERR_HIP and "<consumer>: <call>: <the producer's last error>": the producer did not give its plane
int plane_fail_producer(PlaneHandle *h, const char *consumer, const char *call, const char *producer_error);
// Read behind a producer: in_ev[k] is recorded on the producer's stream and this handle's stream waits for it, so what is
// enqueued here next sees the plane complete.  The handle's device is current.
int plane_read_behind(PlaneHandle *h, int k, void *producer_stream);
// Release to a producer, behind a done_ev recorded on this handle's stream: the producer's stream waits for it, through
// the producer's own wait_event (`call` names it), so what it does next to its plane comes behind this handle's reads.
template <class P>
int plane_release(PlaneHandle *h, const char *consumer, P *producer, int (*wait_event)(P *, void *), const char *call)
{
    if (wait_event(producer, h->done_ev) == LOM_OK) return LOM_OK;
    return fail(h, LOM_ERR_HIP, (std::string(consumer) + ": " + call).c_str());
}

// ---- the source of a cost plane ("the three forms") -------------------------------------------------------
// In which form a caller gave an int8 cost plane to a solver over it (lom_navfield, lom_navset, lom_posefield): a host
// pointer, a device pointer with an optional event, or a clearance grid.  One of the three is set; none: no plane was given.
struct PlaneSource {
    const int8_t *host = nullptr;
    const int8_t *device = nullptr;
    void *event = nullptr;  // `device` is complete behind it; may be NULL
    lom_clearance *clearance = nullptr;

    bool given() const { return host || device || clearance; }
};
inline PlaneSource plane_from_host(const int8_t *plane) { return PlaneSource{plane, nullptr, nullptr, nullptr}; }
inline PlaneSource plane_from_device(const int8_t *d_plane, void *hip_event_or_null) { return PlaneSource{nullptr, d_plane, hip_event_or_null, nullptr}; }
inline PlaneSource plane_from_clearance(lom_clearance *clearance) { return PlaneSource{nullptr, nullptr, nullptr, clearance}; }

// The producer's refusals for a clearance grid, in plane_check_producer's words, against `g`: the handle's own geometry, or
// the one a shift is about to give it -- `differs_tail` then ends the geometry's text.  LOM_OK for a host or a device pointer.
int plane_source_check(PlaneHandle *h, const char *consumer, const PlaneSource &s, const lom_occupancy_geometry &g, const char *differs_tail = "");
// Open, with the handle's device current: *d_plane is the plane in HBM, and what is enqueued on the handle's stream next
// may read it.  A device pointer: behind its event, if there is one.  A clearance grid: its cost plane, read behind its
// stream through in_ev[0] (plane_fail_producer where it does not give the plane).  A host pointer: *d_plane stays NULL --
// the family uploads, because what an operation reads of a host plane differs.
int plane_source_open(PlaneHandle *h, const char *consumer, const PlaneSource &s, const int8_t **d_plane);
// Close, once the body has returned LOM_OK: plane_release to a clearance grid, nothing otherwise.
int plane_source_close(PlaneHandle *h, const char *consumer, const PlaneSource &s);

// ---- the shift by whole cells (include/lidar_odometry_amd.h, "grid shift") --------------------------------------------
// LOM_ERR_RANGE and "<name>: shift: ..." where the rule of plane_geometry.hpp refuses the new origin, else *out
int plane_shifted_geometry(PlaneHandle *h, const char *name, int32_t dx, int32_t dy, lom_occupancy_geometry *out);
// The geometry moves by the rule and the state becomes what the family's own clear leaves (also for dx == dy == 0): these
// handles are recomputed from their producers anyway.  A refusal comes before the clear and leaves the handle untouched.
// Carrying a clearance grid's distances across a shift is not part of this; a navigation field is carried by
// lom_navfield_shift_resolve* (navfield.hip).
template <class H>
int plane_shift(H *h, const char *name, int32_t dx, int32_t dy, int (*clear)(H *))
{
    if (!h) return LOM_ERR_ARG;
    lom_occupancy_geometry g;
    if (const int rc = plane_shifted_geometry(h, name, dx, dy, &g); rc != LOM_OK) return rc;
    if (const int rc = clear(h); rc != LOM_OK) return rc;
    h->geo = g;
    return LOM_OK;
}

// The head of a create: the geometry rule ("<name> geometry: ..."), the device checks, a fresh H on its device and
// plane_setup.  On a failure *out stays NULL and the text is in the family's create slot.
template <class H>
int plane_new(const lom_occupancy_geometry *geometry, int device, std::string &slot, const char *name, const char *setup_text, int n_in,
              H **out)
{
    *out = nullptr;
    if (!plane::geometry_ok(geometry)) return create_fail(slot, LOM_ERR_ARG, (std::string(name) + " geometry: " + plane::kGeometryRule).c_str());
    if (const int rc = check_device(device, slot); rc != LOM_OK) return rc;
    H *h = new (std::nothrow) H();
    if (!h) return create_fail(slot, LOM_ERR_OOM, "host allocation");
    h->device = device;
    h->geo = *geometry;
    if (const int rc = plane_setup(h, slot, setup_text, n_in); rc != LOM_OK) {
        plane_destroy(h);
        return rc;
    }
    *out = h;
    return LOM_OK;
}

}  // namespace lom
