// A point of a scan at the scan's pose, written once for k_asm_transform, k_vote_walk, k_occ_walk and k_elev_accumulate.
// No kernel here.  (The grid hit rule of the last two is not shared: as a function of this header it gave both kernels
// other basic blocks and registers than written out in place -- tools/kernel_identity.py: differs -- so each keeps it.)
#pragma once
#include "k_asm_scan.hpp"

namespace lom {

// x' = (f32)((R0 p0 + (R1 p1 + R2 p2)) + t0) in f64 -- k_transform's association, widened, one rounding per component at
// the end -- of the three floats at p, by the descriptor's pose
__device__ __forceinline__ void posed_point(ConstAsm d, const float *__restrict__ p, float &x, float &y, float &z)
{
    const double p0 = p[0], p1 = p[1], p2 = p[2];
    x = (float)((d->R[0] * p0 + (d->R[1] * p1 + d->R[2] * p2)) + d->t[0]);
    y = (float)((d->R[3] * p0 + (d->R[4] * p1 + d->R[5] * p2)) + d->t[1]);
    z = (float)((d->R[6] * p0 + (d->R[7] * p1 + d->R[8] * p2)) + d->t[2]);
}

}  // namespace lom
