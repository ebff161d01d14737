// The typed launchers of the grid shift's kernels (k_grid_shift.hpp; code: grid_shift.hip, the one translation unit that
// launches them).  occupancy.hip and elevation.hip call these; the host part of a shift is the grid core's
// (grid_handle.hpp).  Each enqueues one launch on `stream` and returns hipGetLastError().
// |dx| <= width and |dy| <= height: the core clamps them.  src and dst are different blocks of width * height cells.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lom {

// two u32 planes at once: dst_x(ix, iy) = src_x(ix + dx, iy + dy), or 0
hipError_t launch_shift_u32x2(hipStream_t stream, const uint32_t *src_a, const uint32_t *src_b, uint32_t *dst_a, uint32_t *dst_b,
                              uint32_t width, uint32_t height, int32_t dx, int32_t dy);
// records of 32 bytes (the elevation grid's ElevCell), 32-byte aligned: likewise, or the cleared record
hipError_t launch_shift_rec32(hipStream_t stream, const void *src, void *dst, uint32_t width, uint32_t height, int32_t dx, int32_t dy);

}  // namespace lom
