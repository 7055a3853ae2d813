// ov_table.hpp — the open-addressing pair table and the whole protocol of the ops that count into it: instances.hip
// (unet_instance_overlap, unet_partition_pairs, unet_cell_contacts) and track.hip (unet_link_frames); DESIGN.md section 4s-bis.
// 64-bit keys (image or frame, id, id), 24 bits per id, claimed by an agent-scope compare-and-swap, one 32-bit counter per slot.
// Which slot a key lands in depends on the order of the claims; nothing reads that.  Device: the key, a lane's run length, the
// sticky insert, the status flush and pair_fill_kernel, the one wave loop from two id maps into the table.  Host: ov_open.
//
// Coherence (label.hip's rule): inside a fill kernel a table key is only ever touched by an agent-scope compare-and-swap; a
// counter, a histogram bin or a status word only by an agent-scope add.  Whatever reads them plainly is a later kernel of the same
// stream.  No word is handed from one workgroup to another inside a kernel by plain loads and stores.
#pragma once
#include "elem.hpp"

namespace unet {

static constexpr unsigned long long OV_EMPTY = ~0ull;        // never a key: b <= 65534

struct OvTable { unsigned long long *keys; unsigned *cnt; size_t slots; };

// the key (b, i, j), b an image or frame <= 65534 and i, j ids in [0, ID_MAX]: keys sort as their triples do
__device__ __forceinline__ unsigned long long ov_key(unsigned long long b, int i, int j)
{
    return b << (2 * ID_BITS) | (unsigned long long)i << ID_BITS | (unsigned)j;
}
__device__ __forceinline__ size_t ov_key_b(unsigned long long key) { return key >> (2 * ID_BITS); }
__device__ __forceinline__ int ov_key_i(unsigned long long key) { return (int)(key >> ID_BITS) & ID_MAX; }
__device__ __forceinline__ int ov_key_j(unsigned long long key) { return (int)key & ID_MAX; }

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

// The sticky insert, a statement: where `cond` holds, n goes to the counter of `key` in the OvTable `tab`, or to the lane's
// `dropped` once the table is full: it only fills up, so after one failed probe a lane stops probing.  The caller spreads the
// flag once per iteration: full = __any(full).  A macro: around an inlined call the compiler lays the fill kernels out differently
#define OV_ADD_IF(cond, tab, key, n, full, dropped)                                                                   \
    do {                                                                                                              \
        if ((cond) && ((full) || !ov_insert((tab).keys, (tab).cnt, (tab).slots, key, n))) { (dropped) += (n); (full) = true; } \
    } while (0)

// the length of the run that starts at this lane: the lanes from one set `head` flag (lane 0 sets its) up to the next
__device__ __forceinline__ unsigned wave_run_length(bool head, int lane)
{
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    return above ? (unsigned)__ffsll(above) : (unsigned)(64 - lane);
}

// The end of a fill kernel, every lane calls it: the lanes' shares are summed over the wave, and lane 0 adds each sum that is not
// 0 with one agent-scope add: status[b][0] += the refused pixels, status[b][1] += the pixels a full table dropped and, for a
// fill that keeps area histograms (BIN_I, BIN_J), their bins 0 += the background pixels.
template <bool BIN_I = false, bool BIN_J = false>
__device__ __forceinline__ void ov_flush(unsigned long long *status, int b, int lane, unsigned long long bad, unsigned long long dropped,
                                         unsigned *bin_i = nullptr, unsigned long long i0 = 0, unsigned *bin_j = nullptr, unsigned long long j0 = 0)
{
    bad = wave_sum(bad); dropped = wave_sum(dropped);
    if constexpr (BIN_I) i0 = wave_sum(i0);
    if constexpr (BIN_J) j0 = wave_sum(j0);
    if (lane == 0) {
        if (bad) __hip_atomic_fetch_add(&status[2 * b], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (dropped) __hip_atomic_fetch_add(&status[2 * b + 1], dropped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (BIN_I) if (i0) __hip_atomic_fetch_add(bin_i, (unsigned)i0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (BIN_J) if (j0) __hip_atomic_fetch_add(bin_j, (unsigned)j0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the pair fill ------------------------------------------------------------------------------------------------------
// What the fill works on in image or frame b: the maps I and J that give a pixel's two ids (J may be null, which reads as 0
// everywhere, where the source says J_MAY_BE_NULL), the ids' limits, and the area histograms the source says it keeps.
struct PairMaps { const int *I, *J; int i_max, j_max; unsigned *area_i, *area_j; };

// A wave reads 64 consecutive pixels of image b = blockIdx.y, merges the runs of equal (i, j) pairs among them with one ballot,
// and the first lane of a run adds the run's length to the histograms and, for i >= 1 and j >= 1 (j >= 0 with KEEP_J0), to the
// counter of the pair's key.  A pixel with an id outside its limits is counted in status[b][0] and nowhere else.
// Src, the kernel's one argument, says at compile time what differs between the users: npx, tab, status; maps(b); key(b, i, j),
// the three in the field order the entry documents; the flags J_MAY_BE_NULL, AREA_I, AREA_J (which histograms exist), KEEP_J0.
template <class Src>
__global__ __launch_bounds__(256) void pair_fill_kernel(const Src src)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const PairMaps m = src.maps(b);
    unsigned long long bad = 0, dropped = 0, i0 = 0, j0 = 0;      // this lane's share of status[b][0..1] and of the two bins 0
    bool full = false;
    const size_t npx = src.npx, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t base = (size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < npx; base += stride) {   // wave-uniform
        const size_t e = base + lane;
        const bool in = e < npx;
        int i = in ? m.I[e] : -1, j = in && (!Src::J_MAY_BE_NULL || m.J) ? m.J[e] : Src::J_MAY_BE_NULL ? 0 : -1;
        const bool ok = in && (unsigned)i <= (unsigned)m.i_max && (unsigned)j <= (unsigned)m.j_max;
        if (!ok) i = j = in ? -1 : -2;                            // out-of-range pixels form runs of their own; so does the tail past the image
        const int il = __shfl_up(i, 1, 64), jl = __shfl_up(j, 1, 64);
        const bool head = lane == 0 || i != il || j != jl;
        const unsigned n = wave_run_length(head, lane);
        if (head && in) {
            if (!ok) bad += n;
            else {
                if constexpr (Src::AREA_I) { if (i) __hip_atomic_fetch_add(&m.area_i[i], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else i0 += n; }
                if constexpr (Src::AREA_J) { if (j) __hip_atomic_fetch_add(&m.area_j[j], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else j0 += n; }
                OV_ADD_IF(i && (Src::KEEP_J0 || j), src.tab, src.key(b, i, j), n, full, dropped);
            }
        }
        full = __any(full);
    }
    ov_flush<Src::AREA_I, Src::AREA_J>(src.status, b, lane, bad, dropped, m.area_i, i0, m.area_j, j0);
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// the table inside a scratch buffer: the keys, then the counters, each 256-aligned
static inline size_t ov_key_bytes(size_t slots) { return align_up(slots * sizeof(unsigned long long), 256); }
static inline size_t ov_scratch_bytes(size_t slots) { return ov_key_bytes(slots) + align_up(slots * sizeof(unsigned), 256); }

// opens the table of entry `who` at the start of its scratch: the slot count checked; keys, counters and n x 2 status words cleared
static inline int ov_open(const char *who, void *scratch, size_t table_slots, void *status_u64, int n, hipStream_t st, OvTable &t)
{
    ARG_CHECK(table_slots > 0 && (table_slots & (table_slots - 1)) == 0, "%s: table_slots must be a power of two", who);
    t = {(unsigned long long *)scratch, (unsigned *)((char *)scratch + ov_key_bytes(table_slots)), table_slots};
    HIP_TRY(hipMemsetAsync(t.keys, 0xFF, table_slots * sizeof(unsigned long long), st));        // OV_EMPTY
    HIP_TRY(hipMemsetAsync(t.cnt, 0, table_slots * sizeof(unsigned), st));
    HIP_TRY(hipMemsetAsync(status_u64, 0, (size_t)n * 2 * sizeof(unsigned long long), st));
    return 0;
}

}  // namespace unet
