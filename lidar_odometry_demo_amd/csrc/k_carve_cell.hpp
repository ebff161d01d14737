// What a walk along a ray does per cell, shared by the ray carve (k_carve.hpp) and the scan votes (k_vote.hpp): the table
// probe that finds a cell's voxel, the plane rule of the truncating index and t_a.  Device functions only, no kernel, so
// that more than one translation unit can include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lom_internal.hpp"

namespace lom {

typedef uint32_t carve_u32x4 __attribute__((ext_vector_type(4)));

// The read side of claim_slot / k_cleanup_mark: the slot that holds `key`, one 16-byte load per probe (key, count and
// slab together, as k_match reads a Slot).  Returns the voxel's slab, kNoSlab where the map has no such voxel -- the
// chain ends on an empty slot, or the key's slot is one an erase or a range error left without a voxel.
__device__ __forceinline__ uint32_t carve_find_slab(const Slot *table, uint32_t mask, uint32_t shift, unsigned long long key)
{
    uint32_t h = hash_key(key, shift) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++) {
        const carve_u32x4 r = *reinterpret_cast<const carve_u32x4 *>(table + h);
        const unsigned long long seen = (unsigned long long)r.x | ((unsigned long long)r.y << 32);
        if (seen == key) return r.w;
        if (seen == kEmptyKey) break;
        h = (h + 1) & mask;
    }
    return kNoSlab;
}

// next plane index of cell c in direction s under the truncating index: cell 0 spans (-V, V), there is no plane at 0
__device__ __forceinline__ int carve_plane(int c, int s) { return s > 0 ? (c >= 0 ? c + 1 : c) : (c <= 0 ? c - 1 : c); }

__device__ __forceinline__ double carve_t(int c, int s, double V, double O, double D)
{
    return D != 0.0 ? ((double)carve_plane(c, s) * V - O) / D : __builtin_inf();
}

}  // namespace lom
