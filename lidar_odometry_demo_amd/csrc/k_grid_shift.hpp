// Grid shift (include/lidar_odometry_amd.h, "grid shift"): k_shift_u32x2 moves the two u32 count planes of an
// occupancy grid, k_shift_rec32 the 32-byte records of an elevation grid.  Device code only; grid_shift.hip is the one
// translation unit that instantiates and launches it.
//
// Both are byte movers from the old block into a second one (the host swaps the two behind the launch): cell (ix, iy) of
// the destination takes cell (ix + dx, iy + dy) of the source where that lies in the grid, else the cleared value, in the
// same pass.  Every destination byte is written exactly once, by one thread; no thread reads what another writes.  No
// workgroup waits for another; no LDS; no scratch.  The host clamps |dx| <= width and |dy| <= height (a larger shift keeps
// nothing, as these do), so every index below fits 32 bits with room to spare.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lom {

constexpr uint32_t kShiftThreads = 256;

// four u32 that sit at any multiple of 4 bytes: what a row shifted by dx cells is against the destination's 16-byte chunks
struct __attribute__((packed, aligned(4))) ShiftU32x4 {
    uint32_t v[4];
};

// A thread per 16-byte chunk of the destination planes, taken as linear arrays of n = width * height u32 (the blocks are
// 256-byte aligned, so every chunk is): the stores are aligned dwordx4, a wave's cover 1 KiB of consecutive bytes.  A
// chunk whose four cells lie in one row and all have a source loads that source as one 16-byte access 4 * dx bytes off
// the chunk's alignment; a chunk across a row end or the kept box's edge goes cell by cell.  The tail of n % 4 cells is
// stored as single dwords.  Both planes in one launch: the index arithmetic is done once.
__global__ __launch_bounds__(kShiftThreads) void k_shift_u32x2(const uint32_t *__restrict__ src_a, const uint32_t *__restrict__ src_b,
                                                                uint32_t *__restrict__ dst_a, uint32_t *__restrict__ dst_b,
                                                                uint32_t width, uint32_t height, int32_t dx, int32_t dy)
{
    const uint32_t n = width * height;  // <= 2^28
    const uint32_t i0 = (blockIdx.x * kShiftThreads + threadIdx.x) * 4u;
    if (i0 >= n) return;
    const uint32_t iy0 = i0 / width, ix0 = i0 - iy0 * width;
    const int32_t sy0 = (int32_t)iy0 + dy, sx0 = (int32_t)ix0 + dx;
    const bool whole = i0 + 4u <= n;
    if (whole && ix0 + 4u <= width) {  // one row
        const bool row_in = sy0 >= 0 && sy0 < (int32_t)height;
        if (row_in && sx0 >= 0 && sx0 + 4 <= (int32_t)width) {
            const size_t s = (size_t)sy0 * width + (size_t)sx0;
            const ShiftU32x4 a = *reinterpret_cast<const ShiftU32x4 *>(src_a + s);
            const ShiftU32x4 b = *reinterpret_cast<const ShiftU32x4 *>(src_b + s);
            *reinterpret_cast<uint4 *>(dst_a + i0) = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
            *reinterpret_cast<uint4 *>(dst_b + i0) = make_uint4(b.v[0], b.v[1], b.v[2], b.v[3]);
            return;
        }
        if (!row_in || sx0 + 4 <= 0 || sx0 >= (int32_t)width) {  // nothing of it is kept
            *reinterpret_cast<uint4 *>(dst_a + i0) = make_uint4(0u, 0u, 0u, 0u);
            *reinterpret_cast<uint4 *>(dst_b + i0) = make_uint4(0u, 0u, 0u, 0u);
            return;
        }
    }
    // cell by cell: across a row end, across the kept box's edge, or the tail
    uint32_t a[4], b[4];
    uint32_t ix = ix0;
    int32_t sy = sy0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        a[k] = b[k] = 0u;
        const int32_t sx = (int32_t)ix + dx;
        if (i0 + (uint32_t)k < n && sx >= 0 && sx < (int32_t)width && sy >= 0 && sy < (int32_t)height) {
            const size_t s = (size_t)sy * width + (size_t)sx;
            a[k] = src_a[s], b[k] = src_b[s];
        }
        if (++ix == width) ix = 0u, sy++;
    }
    if (whole) {
        *reinterpret_cast<uint4 *>(dst_a + i0) = make_uint4(a[0], a[1], a[2], a[3]);
        *reinterpret_cast<uint4 *>(dst_b + i0) = make_uint4(b[0], b[1], b[2], b[3]);
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (i0 + (uint32_t)k < n) dst_a[i0 + k] = a[k], dst_b[i0 + k] = b[k];
}

// A thread per 16-byte half of a destination record, so that a wave's loads and its stores each cover 1 KiB of consecutive
// bytes: two aligned dwordx4 per cell in each direction, whatever the shift.  The cleared record is k_elev_clear's: sum 0,
// count 0, zmin INT32_MAX | zmax INT32_MIN, pad 0.
__global__ __launch_bounds__(kShiftThreads) void k_shift_rec32(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t width,
                                                                uint32_t height, int32_t dx, int32_t dy)
{
    const uint32_t t = blockIdx.x * kShiftThreads + threadIdx.x;  // < 2^27 + 256
    const uint32_t c = t >> 1, half = t & 1u;
    if (c >= width * height) return;
    const uint32_t iy = c / width, ix = c - iy * width;
    const int32_t sx = (int32_t)ix + dx, sy = (int32_t)iy + dy;
    uint4 v = half ? make_uint4(0x80000000u, 0u, 0u, 0u) : make_uint4(0u, 0u, 0u, 0x7FFFFFFFu);
    if (sx >= 0 && sx < (int32_t)width && sy >= 0 && sy < (int32_t)height) v = src[((size_t)sy * width + (size_t)sx) * 2u + half];
    dst[(size_t)c * 2u + half] = v;
}

}  // namespace lom
