// What the map's kernels share on the device and no kernel of its own: claiming a table slot and the 12-byte point
// accessors.  Inline device functions only, so every kernel header of the map may include it (a kernel header, in
// contrast, belongs to exactly one translation unit).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lom_internal.hpp"

namespace lom {

__device__ inline uint32_t claim_slot(Slot *table, uint32_t mask, uint32_t shift, unsigned long long key)
{
    uint32_t h = hash_key(key, shift) & mask;
    for (;;) {
        // Look before the CAS: a slot that already shows this key needs no atomic (most points of a frame fall
        // into voxels the map already has, and an atomic is a round trip to the memory side).  A stale view
        // -- the slot still looks empty, or shows another key that is itself final -- only costs the CAS
        // (keys never change once set) or moves on to the next slot exactly as the CAS would.
        const unsigned long long seen = __hip_atomic_load(&table[h].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == key) return h;
        if (seen == kEmptyKey) {
            const unsigned long long prev = atomicCAS(&table[h].key, kEmptyKey, key);
            if (prev == kEmptyKey || prev == key) return h;
        }
        h = (h + 1) & mask;
    }
}

__device__ inline const float *point_at(const char *base, size_t i, size_t stride)
{
    return reinterpret_cast<const float *>(base + i * stride);
}

// one 12-byte point as ONE memory instruction: a packed struct tells the compiler that the three floats are
// contiguous and 4-byte aligned, and it issues global_load / global_store_dwordx3 -- on the scattered slab
// writes that is one partial-line transaction per point instead of three
struct __attribute__((packed, aligned(4))) Point3 {
    float x, y, z;
};
__device__ __forceinline__ Point3 load3(const float *p) { return *reinterpret_cast<const Point3 *>(p); }
__device__ __forceinline__ void store3(float *p, Point3 v) { *reinterpret_cast<Point3 *>(p) = v; }

}  // namespace lom
