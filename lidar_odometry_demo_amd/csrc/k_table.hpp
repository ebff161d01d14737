// The hash table itself and what every map kernel shares: k_table_init, claim_slot, k_rebuild, the 12-byte point
// accessors, k_restride, and the device-words-to-host kernel k_gather_words.  Device code only; voxel_map.hip is the one translation unit
// that instantiates and launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grid_scan.hpp"
#include "lom_internal.hpp"

namespace lom {

// ---------------------------------------------------------------------------
// table kernels
// ---------------------------------------------------------------------------
__global__ void k_table_init(Slot *table, uint32_t cap)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) {
        Slot s;
        s.key = kEmptyKey;
        s.count = 0;
        s.slab = kNoSlab;
        table[i] = s;
    }
}

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

// rebuild the table from the slab arrays (after rehash / cleanup)
__global__ void k_rebuild(Slot *table, uint32_t mask, uint32_t shift, const unsigned long long *slab_key,
                          const uint32_t *slab_count, uint32_t n_vox)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_vox) return;
    const uint32_t c = slab_count[s];
    if (!c) return;  // a slab whose voxel a radius cleanup erased (k_cleanup_mark): the key is free again
    const uint32_t h = claim_slot(table, mask, shift, slab_key[s]);
    table[h].count = c;
    table[h].slab = s;
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

__global__ void k_set_word(uint32_t *w, uint32_t v)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *w = v;
}

// Device words -> host in ONE launch and no copy engine: a single wave stores {word, call tag} pairs as
// 64-bit system-scope words into the handle's coherent pinned block; the host watches the tags.  (A
// hipMemcpyAsync per word is a 4 us blit kernel each plus its enqueue: ten of them per frame of the streaming
// path were 15 % of its kernel time.)  The stream is in order, so the words arriving also says that
// everything enqueued before them is through.
struct WordPtrs {
    const uint32_t *p[32];
};

__global__ __launch_bounds__(64) void k_gather_words(WordPtrs w, int n, unsigned long long *host_out, uint32_t tag)
{
    const int i = (int)threadIdx.x;
    if (i >= n) return;
    const uint32_t v = __hip_atomic_load(w.p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(host_out + i, (unsigned long long)v | ((unsigned long long)tag << 32), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}

// rows of every live slab from stride K0 to stride K1 > K0 (setMaxPoints raised on a map that holds voxels)
// (C linkage: the kernel's symbol has always been the plain name)
extern "C" __global__ void k_restride(const float *pts0, const float *nrm0, const uint32_t *slab_count, uint32_t n_vox, uint32_t K0,
                           uint32_t K1, float *pts1, float *nrm1)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t slab = (uint32_t)(i / K0), row = (uint32_t)(i % K0);
    if (slab >= n_vox || row >= slab_count[slab]) return;
    const size_t src = ((size_t)slab * K0 + row) * 3, dst = ((size_t)slab * K1 + row) * 3;
    store3(pts1 + dst, load3(pts0 + src));
    store3(nrm1 + dst, load3(nrm0 + src));
}

}  // namespace lom
