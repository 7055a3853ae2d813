// track.hip — linking the cells of consecutive frames of a time-lapse by overlap (functions.link_frames):
// for every cell c of frame t the cell p of frame t-1 that shares the most pixels with it, on the device, for all frames at once.
//
// unet_link_frames: two id maps [T,H,W] (`from`, whose frame t-1 is set against frame t of `to`; they may be one map) ->
//   1. link_fill    overlap_fill's wave loop (instances.hip): a wave reads 64 consecutive pixels of frame t, merges the runs of
//                   equal (p, c) pairs among them with one ballot, and the first lane of a run adds the run's length to area[t][c]
//                   and, for p, c >= 1, to the counter of the key (t, p, c) in the open-addressing table of ov_table.hpp
//   2. link_pick    one thread per table slot: a 64-bit agent-scope max of count << 24 | (OV_ID_MAX - p) into the word of (t, c).
//                   The larger count wins, and among equal counts the smaller p, whatever the order the slots arrive in
//   3. link_decode  one thread per (t, c): the word -> pred[t][c], pred_overlap[t][c]; a word nobody touched gives 0, 0
// Every count is an integer sum and the max is over a total order: the outputs do not depend on the order of the atomics.
//
// Coherence (label.hip's rule): inside link_fill a table key is only ever touched by an agent-scope compare-and-swap, a counter, an
// area bin or a status word only by an agent-scope add; inside link_pick a word of `best` only by an agent-scope max; link_pick and
// link_decode read what an earlier kernel wrote.  No word is handed from one workgroup to another inside a kernel.
#include "ov_table.hpp"
#include "../../include/unet_hip.h"

namespace unet {

// frame t = blockIdx.y: c from to[t], p from from[t - 1] (frame 0 has no predecessor: p = 0 everywhere, areas only)
__global__ __launch_bounds__(256) void link_fill_kernel(const int *from, const int *to, size_t npx, int n_max, unsigned long long *keys,
                                                        unsigned *cnt, size_t slots, unsigned *area, unsigned long long *status)
{
    const int t = blockIdx.y, lane = threadIdx.x & 63;
    const int *C = to + (size_t)t * npx, *P = t ? from + (size_t)(t - 1) * npx : nullptr;
    unsigned *ar = area + (size_t)t * ((size_t)n_max + 1);
    unsigned long long bad = 0, dropped = 0, c0 = 0;             // this lane's share of status[t][0..1] and of the bin 0
    bool full = false;                                            // the table only fills up: after one failed probe, stop probing
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t base = (size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < npx; base += stride) {   // wave-uniform
        const size_t e = base + lane;
        const bool in = e < npx;
        int c = in ? C[e] : -1, p = in && P ? P[e] : 0;
        const bool ok = in && (unsigned)c <= (unsigned)n_max && (unsigned)p <= (unsigned)n_max;
        if (!ok) c = p = in ? -1 : -2;                            // out-of-range pixels form runs of their own; so does the tail past the image
        const int cl = __shfl_up(c, 1, 64), pl = __shfl_up(p, 1, 64);
        const bool head = lane == 0 || c != cl || p != pl;
        const unsigned long long heads = __ballot(head);
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const unsigned n = above ? (unsigned)__ffsll(above) : (unsigned)(64 - lane);   // run length: up to the next head
        if (head && in) {
            if (!ok) bad += n;
            else {
                if (c) __hip_atomic_fetch_add(&ar[c], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else c0 += n;
                if (c && p) {
                    const unsigned long long key = (unsigned long long)t << (2 * OV_ID_BITS) | (unsigned long long)p << OV_ID_BITS | (unsigned)c;
                    if (full || !ov_insert(keys, cnt, slots, key, n)) { dropped += n; full = true; }
                }
            }
        }
        full = __any(full);
    }
    bad = wave_sum(bad); dropped = wave_sum(dropped); c0 = wave_sum(c0);
    if (lane == 0) {
        if (bad) __hip_atomic_fetch_add(&status[2 * t], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (dropped) __hip_atomic_fetch_add(&status[2 * t + 1], dropped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c0) __hip_atomic_fetch_add(&ar[0], (unsigned)c0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// count < 2^31 and p <= OV_ID_MAX: the packed word fits 55 bits, and it is > 0 for every occupied slot (count >= 1)
__global__ __launch_bounds__(256) void link_pick_kernel(const unsigned long long *__restrict__ keys, const unsigned *__restrict__ cnt,
                                                        size_t slots, int n_max, unsigned long long *best)
{
    for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[s];
        if (key == OV_EMPTY) continue;
        const size_t t = key >> (2 * OV_ID_BITS);
        const unsigned p = (unsigned)(key >> OV_ID_BITS) & OV_ID_MAX, c = (unsigned)key & OV_ID_MAX;
        const unsigned long long word = (unsigned long long)cnt[s] << OV_ID_BITS | (unsigned)(OV_ID_MAX - p);
        __hip_atomic_fetch_max(&best[t * ((size_t)n_max + 1) + c], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void link_decode_kernel(const unsigned long long *__restrict__ best, size_t n, int *__restrict__ pred,
                                                          unsigned *__restrict__ pred_overlap)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long w = best[i];
        pred[i] = w ? OV_ID_MAX - (int)(w & OV_ID_MAX) : 0;
        pred_overlap[i] = (unsigned)(w >> OV_ID_BITS);
    }
}

} // namespace unet

using namespace unet;

static size_t link_rows(int T, int n_max) { return (size_t)T * ((size_t)n_max + 1); }

size_t unet_link_frames_scratch_bytes(int T, int n_max, size_t table_slots)
{
    if (T <= 0 || n_max < 0 || table_slots == 0) return 0;
    return ov_scratch_bytes(table_slots) + align_up(link_rows(T, n_max) * sizeof(unsigned long long), 256);
}

int unet_link_frames(const void *from_i32, const void *to_i32, int T, int H, int W, int n_max, size_t table_slots, void *area_u32,
                     void *pred_i32, void *pred_overlap_u32, void *status_u64, void *scratch, void *stream)
{
    ARG_CHECK(from_i32 && to_i32 && area_u32 && pred_i32 && pred_overlap_u32 && status_u64 && scratch && T > 0 && H > 0 && W > 0,
              "unet_link_frames: bad argument");
    ARG_CHECK((size_t)H * W < (1u << 31) && T <= 65535, "unet_link_frames: image too large or more than 65535 frames");
    ARG_CHECK(n_max >= 0 && n_max <= OV_ID_MAX, "unet_link_frames: n_max must be in [0, %d]", OV_ID_MAX);
    ARG_CHECK(table_slots > 0 && (table_slots & (table_slots - 1)) == 0, "unet_link_frames: table_slots must be a power of two");
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)H * W, rows = link_rows(T, n_max);
    unsigned long long *keys = (unsigned long long *)scratch;
    unsigned *cnt = (unsigned *)((char *)scratch + ov_key_bytes(table_slots));
    unsigned long long *best = (unsigned long long *)((char *)scratch + ov_scratch_bytes(table_slots));
    HIP_TRY(hipMemsetAsync(keys, 0xFF, table_slots * sizeof(unsigned long long), st));          // OV_EMPTY
    HIP_TRY(hipMemsetAsync(cnt, 0, table_slots * sizeof(unsigned), st));
    HIP_TRY(hipMemsetAsync(best, 0, rows * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(area_u32, 0, rows * sizeof(unsigned), st));
    HIP_TRY(hipMemsetAsync(status_u64, 0, (size_t)T * 2 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(link_fill_kernel, dim3(grid_for(npx, 256, 2048), T), dim3(256), 0, st, (const int *)from_i32, (const int *)to_i32,
                       npx, n_max, keys, cnt, table_slots, (unsigned *)area_u32, (unsigned long long *)status_u64);
    hipLaunchKernelGGL(link_pick_kernel, dim3(grid_for(table_slots, 256, 2048)), dim3(256), 0, st, (const unsigned long long *)keys,
                       (const unsigned *)cnt, table_slots, n_max, best);
    hipLaunchKernelGGL(link_decode_kernel, dim3(grid_for(rows, 256, 2048)), dim3(256), 0, st, (const unsigned long long *)best, rows,
                       (int *)pred_i32, (unsigned *)pred_overlap_u32);
    HIP_TRY(hipGetLastError());
    return 0;
}
