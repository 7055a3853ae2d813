// ov_table.hpp — the open-addressing pair table that instances.hip (unet_instance_overlap, unet_partition_pairs) and track.hip
// (unet_link_frames) count into, stated once: 64-bit keys (image or frame, id, id), 24 bits per id, claimed by an agent-scope
// compare-and-swap, one 32-bit counter per slot.  Which slot a key lands in depends on the order of the claims; nothing reads that.
#pragma once
#include "elem.hpp"

namespace unet {

static constexpr unsigned long long OV_EMPTY = ~0ull;        // never a key: b <= 65534
static constexpr int OV_ID_BITS = 24;
static constexpr int OV_ID_MAX = (1 << OV_ID_BITS) - 1;

__device__ __forceinline__ unsigned long long ov_hash(unsigned long long x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}

// adds n to the counter of `key`; false when the key is absent and no slot is free
__device__ __forceinline__ bool ov_insert(unsigned long long *keys, unsigned *cnt, size_t slots, unsigned long long key, unsigned n)
{
    size_t h = ov_hash(key) & (slots - 1);
    for (size_t probe = 0; probe < slots; ++probe) {
        unsigned long long seen = OV_EMPTY;
        if (__hip_atomic_compare_exchange_strong(&keys[h], &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ||
            seen == key) {
            __hip_atomic_fetch_add(&cnt[h], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return true;
        }
        h = (h + 1) & (slots - 1);
    }
    return false;
}

// the table inside a scratch buffer: the keys, then the counters, each 256-aligned
static inline size_t ov_key_bytes(size_t slots) { return align_up(slots * sizeof(unsigned long long), 256); }
static inline size_t ov_scratch_bytes(size_t slots) { return ov_key_bytes(slots) + align_up(slots * sizeof(unsigned), 256); }

}  // namespace unet
