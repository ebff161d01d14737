// What every device handle is: the device it lives on, the stream its work runs on, the text of its last error -- and
// the blocks of device and pinned host memory it owns.  lom_map, lom_frontend, lom_place_db, lom_graph and lom_archive
// derive from DeviceHandle directly; lom_occupancy and lom_elevation through GridHandle (grid_handle.hpp: grids that
// integrate posed scans); lom_clearance, lom_navfield, lom_regions and lom_visibility through PlaneHandle
// (plane_handle.hpp: grids that read other handles' planes).  What is written once on DeviceHandle * is declared here
// (code: below and in handle.hip).  Host code only; nothing here launches a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>

#include "../../include/lidar_odometry_amd.h"

namespace lom {

struct DeviceHandle {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string error;
};

// ---- errors ---------------------------------------------------------------------------------------------------------
// what[: hipGetErrorString(e)]
inline std::string error_text(const char *what, hipError_t e)
{
    std::string s = what ? what : "";
    if (e != hipSuccess) {
        s += ": ";
        s += hipGetErrorString(e);
    }
    return s;
}

// records the text in the handle (never NULL) and returns `code`
inline int fail(DeviceHandle *h, int code, const char *what, hipError_t e = hipSuccess)
{
    h->error = error_text(what, e);
    return code;
}

// the failures before a handle exists: the public header documents, per family, "NULL: why the last create on this
// thread failed", so every family keeps a thread_local slot of its own and passes it
inline int create_fail(std::string &slot, int code, const char *what, hipError_t e = hipSuccess)
{
    slot = error_text(what, e);
    return code;
}

// h: any pointer convertible to DeviceHandle *
#define LOM_HIP(h, expr)                                                       \
    do {                                                                       \
        hipError_t _e = (expr);                                                \
        if (_e != hipSuccess) return lom::fail((h), LOM_ERR_HIP, #expr, _e);   \
    } while (0)

// handle.hip: the device checks of a create -- a device is visible (LOM_ERR_NO_DEVICE, "... no CPU fallback"), the index
// is in range (LOM_ERR_ARG), its properties can be read and it is a gfx950 (LOM_ERR_NO_DEVICE; name_device: the text
// names the architecture found).  The text goes to the family's create slot.
int check_device(int device, std::string &slot, bool name_device = false);

// ---- owned memory ---------------------------------------------------------------------------------------------------
// A block of device memory and its size.  Owns the block: the destructor frees it; no copy; move and swap work.
struct DeviceBuf {
    void *p = nullptr;
    size_t bytes = 0;

    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf &) = delete;
    DeviceBuf &operator=(const DeviceBuf &) = delete;
    DeviceBuf(DeviceBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    DeviceBuf &operator=(DeviceBuf &&o) noexcept
    {
        DeviceBuf t(std::move(o));
        swap(t);
        return *this;
    }
    ~DeviceBuf()
    {
        if (p) (void)hipFree(p);
    }
    void swap(DeviceBuf &o) noexcept { std::swap(p, o.p), std::swap(bytes, o.bytes); }
    template <typename T>
    T *as() const
    {
        return static_cast<T *>(p);
    }
};

// its pinned host counterpart, with the device view of a mapped block
struct PinnedBuf {
    void *h = nullptr;
    void *d = nullptr;  // hipHostMallocMapped blocks only
    size_t bytes = 0;

    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    PinnedBuf(PinnedBuf &&o) noexcept : h(o.h), d(o.d), bytes(o.bytes) { o.h = o.d = nullptr, o.bytes = 0; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept
    {
        PinnedBuf t(std::move(o));
        swap(t);
        return *this;
    }
    ~PinnedBuf()
    {
        if (h) (void)hipHostFree(h);
    }
    void swap(PinnedBuf &o) noexcept { std::swap(h, o.h), std::swap(d, o.d), std::swap(bytes, o.bytes); }
    template <typename T>
    T *as() const  // the host view
    {
        return static_cast<T *>(h);
    }
};

inline void swap(DeviceBuf &a, DeviceBuf &b) noexcept { a.swap(b); }
inline void swap(PinnedBuf &a, PinnedBuf &b) noexcept { a.swap(b); }

// free now (nothing waits: the caller knows that no enqueued work uses the block)
inline void release(DeviceBuf &b) { DeviceBuf().swap(b); }
inline void release(PinnedBuf &b) { PinnedBuf().swap(b); }

// handle.hip: exactly `bytes` into an EMPTY buffer; on failure the buffer stays empty and HIP's sticky error is cleared.
// (What a create allocates once; the grow-only forms below go through them.)
hipError_t alloc(DeviceBuf &b, size_t bytes);
hipError_t alloc(PinnedBuf &b, size_t bytes, unsigned flags);  // mapped into the device's address space where the flags ask for it

// The size a grow-only buffer of `have` bytes takes when `need` are asked for: `have` when that is enough, else
// max(need, 1.5 * have) rounded up to 256 -- saturating, never wrapping.
inline size_t grown_bytes(size_t have, size_t need)
{
    if (need <= have) return have;
    const size_t step = have / 2 > SIZE_MAX - have ? SIZE_MAX : have + have / 2;
    const size_t nb = std::max(need, step);
    return nb > SIZE_MAX - 255 ? nb : (nb + 255) & ~size_t(255);
}

// handle.hip: grow-only device buffer, nothing carried over.  At least `bytes` are there when it returns LOM_OK (a
// zero-byte request on an empty buffer leaves it empty: a caller that needs a block asks for max(bytes, its minimum)).
// The stream is synchronised only when an old block is replaced (what is enqueued may still use it).  A failed
// allocation is LOM_ERR_OOM, with HIP's sticky error cleared and `b` empty.
int ensure(DeviceHandle *h, DeviceBuf &b, size_t bytes);
// handle.hip: grow-only pinned host block.  One of at least `need` bytes is left alone; else the stream is synchronised
// (what is enqueued may still read the old block), the old block freed and `grow_to` (>= need) bytes allocated with
// `flags`.  *fresh: the block is new, its contents undefined.
int ensure_pinned(DeviceHandle *h, PinnedBuf &b, size_t need, size_t grow_to, unsigned flags, const char *what, bool *fresh = nullptr);

}  // namespace lom
