// The launches of the grid shift (grid_shift.hpp): the one translation unit that instantiates k_grid_shift.hpp.
#include "grid_shift.hpp"

#include "k_grid_shift.hpp"

namespace lom {

hipError_t launch_shift_u32x2(hipStream_t stream, const uint32_t *src_a, const uint32_t *src_b, uint32_t *dst_a, uint32_t *dst_b,
                              uint32_t width, uint32_t height, int32_t dx, int32_t dy)
{
    const uint32_t chunks = (width * height + 3u) / 4u;
    hipLaunchKernelGGL(k_shift_u32x2, dim3((chunks + kShiftThreads - 1) / kShiftThreads), dim3(kShiftThreads), 0, stream, src_a, src_b,
                       dst_a, dst_b, width, height, dx, dy);
    return hipGetLastError();
}

hipError_t launch_shift_rec32(hipStream_t stream, const void *src, void *dst, uint32_t width, uint32_t height, int32_t dx, int32_t dy)
{
    const uint32_t halves = width * height * 2u;
    hipLaunchKernelGGL(k_shift_rec32, dim3((halves + kShiftThreads - 1) / kShiftThreads), dim3(kShiftThreads), 0, stream,
                       static_cast<const uint4 *>(src), static_cast<uint4 *>(dst), width, height, dx, dy);
    return hipGetLastError();
}

}  // namespace lom
