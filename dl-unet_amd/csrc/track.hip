// track.hip — linking the cells of consecutive frames of a time-lapse by overlap (functions.link_frames):
// for every cell c of frame t the cell p of frame t-1 that shares the most pixels with it, on the device, for all frames at once.
//
// unet_link_frames: two id maps [T,H,W] (`from`, whose frame t-1 is set against frame t of `to`; they may be one map) ->
//   1. link_fill    ov_table.hpp's pair fill on (p, c), p from frame t-1 of `from` and c from frame t of `to`: the first lane of a
//                   run of equal pairs adds the run's length to area[t][c] and, for p, c >= 1, to the counter of the key (t, p, c)
//   2. link_pick    one thread per table slot: a 64-bit agent-scope max of count << 24 | (ID_MAX - p) into the word of (t, c).
//                   The larger count wins, and among equal counts the smaller p, whatever the order the slots arrive in
//   3. link_decode  one thread per (t, c): the word -> pred[t][c], pred_overlap[t][c]; a word nobody touched gives 0, 0
// Every count is an integer sum and the max is over a total order: the outputs do not depend on the order of the atomics.
//
// Coherence: ov_table.hpp's rule for link_fill; inside link_pick a word of `best` is touched only by an agent-scope max;
// link_pick and link_decode read what an earlier kernel wrote.
#include "ov_table.hpp"
#include "../../include/unet_hip.h"

namespace unet {

// link_fill = pair_fill_kernel (ov_table.hpp) on frame t: the pixel's pair is (c, p), c from to[t] and p from from[t - 1] (frame
// 0 has no predecessor: p = 0 everywhere, areas only), its key (t, p, c); one id limit for both, one histogram, that of c
struct LinkFill {
    const int *from, *to; size_t npx; int n_max; OvTable tab; unsigned *area; unsigned long long *status;
    static constexpr bool J_MAY_BE_NULL = true, AREA_I = true, AREA_J = false, KEEP_J0 = false;
    __device__ unsigned long long key(unsigned long long t, int c, int p) const { return ov_key(t, p, c); }
    __device__ PairMaps maps(int t) const
    {
        return {to + (size_t)t * npx, t ? from + (size_t)(t - 1) * npx : nullptr, n_max, n_max, area + (size_t)t * ((size_t)n_max + 1), nullptr};
    }
};

// count < 2^31 and p <= ID_MAX: the packed word fits 55 bits, and it is > 0 for every occupied slot (count >= 1)
__global__ __launch_bounds__(256) void link_pick_kernel(const unsigned long long *__restrict__ keys, const unsigned *__restrict__ cnt,
                                                        size_t slots, int n_max, unsigned long long *best)
{
    for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[s];
        if (key == OV_EMPTY) continue;
        const size_t t = ov_key_b(key);
        const unsigned p = ov_key_i(key), c = ov_key_j(key);
        const unsigned long long word = (unsigned long long)cnt[s] << ID_BITS | (unsigned)(ID_MAX - p);
        __hip_atomic_fetch_max(&best[t * ((size_t)n_max + 1) + c], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void link_decode_kernel(const unsigned long long *__restrict__ best, size_t n, int *__restrict__ pred,
                                                          unsigned *__restrict__ pred_overlap)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long w = best[i];
        pred[i] = w ? ID_MAX - (int)(w & ID_MAX) : 0;
        pred_overlap[i] = (unsigned)(w >> ID_BITS);
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
    ARG_CHECK(n_max >= 0 && n_max <= ID_MAX, "unet_link_frames: n_max must be in [0, %d]", ID_MAX);
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)H * W, rows = link_rows(T, n_max);
    OvTable t;
    if (int rc = ov_open("unet_link_frames", scratch, table_slots, status_u64, T, st, t)) return rc;
    unsigned long long *best = (unsigned long long *)((char *)scratch + ov_scratch_bytes(table_slots));
    HIP_TRY(hipMemsetAsync(best, 0, rows * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(area_u32, 0, rows * sizeof(unsigned), st));
    const LinkFill src{(const int *)from_i32, (const int *)to_i32, npx, n_max, t, (unsigned *)area_u32, (unsigned long long *)status_u64};
    hipLaunchKernelGGL(pair_fill_kernel<LinkFill>, dim3(grid_for(npx, 256, 2048), T), dim3(256), 0, st, src);
    hipLaunchKernelGGL(link_pick_kernel, dim3(grid_for(table_slots, 256, 2048)), dim3(256), 0, st, (const unsigned long long *)t.keys,
                       (const unsigned *)t.cnt, table_slots, n_max, best);
    hipLaunchKernelGGL(link_decode_kernel, dim3(grid_for(rows, 256, 2048)), dim3(256), 0, st, (const unsigned long long *)best, rows,
                       (int *)pred_i32, (unsigned *)pred_overlap_u32);
    HIP_TRY(hipGetLastError());
    return 0;
}
