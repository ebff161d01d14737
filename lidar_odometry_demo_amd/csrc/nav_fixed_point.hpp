// The host loop of a relaxation over tiles, written once for lom_navfield (navfield.hip), lom_navset (navset.hip) and
// lom_posefield (posefield.hip).  Host code; launches nothing itself.
#pragma once
#include "device_handle.hpp"
#include "navfield_host.hpp"

namespace lom {

// A fixed point over tiles, in batches of launches with one wait each.  Launch k reads the marks of parity k & 1 and
// writes the others: launch(cur, nxt, flag) enqueues it.  A parity holds marks_per_parity words: the tiles of a field, or
// of every field of a set.  A launch behind the fixed point finds no active tile (or, with all tiles, changes nothing) and
// marks nothing, so the batch may run ahead of what the host knows.  Both arrays are clear when this returns LOM_OK.
// H has marks, flags (DeviceBuf), h_flags (PinnedBuf), batch, geo and stream.
template <class H, class Launch>
int to_fixed_point(H *f, size_t marks_per_parity, uint64_t &launches, uint64_t &waits, const char *unsettled, Launch launch)
{
    uint32_t *const marks = f->marks.template as<uint32_t>();
    const uint64_t bound = navfield::launch_bound(f->geo.width, f->geo.height);
    const uint32_t B = f->batch;
    for (;;) {
        LOM_HIP(f, hipMemsetAsync(f->flags.p, 0, (size_t)B * 4, f->stream));
        for (uint32_t j = 0; j < B; j++) {
            const uint32_t parity = (uint32_t)(launches & 1u);
            launch(marks + (size_t)parity * marks_per_parity, marks + (size_t)(parity ^ 1u) * marks_per_parity,
                   f->flags.template as<uint32_t>() + j);
            LOM_HIP(f, hipGetLastError());
            launches++;
        }
        LOM_HIP(f, hipMemcpyAsync(f->h_flags.h, f->flags.p, (size_t)B * 4, hipMemcpyDeviceToHost, f->stream));
        LOM_HIP(f, hipStreamSynchronize(f->stream));
        waits++;
        if (f->h_flags.template as<uint32_t>()[B - 1u] == 0u) return LOM_OK;  // the last launch marked nothing: the fixed point
        if (launches > bound) return fail(f, LOM_ERR_HIP, unsettled);
    }
}

// One test option of such a handle (inner_cap, batch, all_tiles, a form): a value above `max` is refused with the option's
// text, a value <= 0 gives the default.
inline int set_test_option(DeviceHandle *f, uint32_t &slot, int64_t value, uint32_t max, uint32_t def, const char *range_text)
{
    if (value > (int64_t)max) return fail(f, LOM_ERR_ARG, range_text);
    slot = value <= 0 ? def : (uint32_t)value;
    return LOM_OK;
}

}  // namespace lom
