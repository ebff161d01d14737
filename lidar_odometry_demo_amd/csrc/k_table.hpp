// The hash table's own kernels: k_table_init, k_rebuild, k_restride, and the device-words-to-host kernel k_gather_words.
// Device code only; voxel_map.hip is the one translation unit that instantiates and launches it -- the other map files
// reach these kernels through its host functions (map_internal.hpp: table_rebuild, launch_gather_words).  What the other
// kernel headers share with these kernels (claim_slot, the 12-byte point accessors) is table_device.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grid_scan.hpp"
#include "lom_internal.hpp"
#include "table_device.hpp"

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
