// geo.hip — seeded geodesic growth inside a mask (functions.split_cells: the "grow the confident cores back inside the mask and
// stop where two growths meet" step that splits touching cells), batched, on the device.  The region is mask != 0; g(p) is the
// least number of 4-neighbour steps from a seed pixel to p along region pixels; a region pixel with g(p) <= max_steps takes the
// id of the seed pixel at that distance, the smallest id among those at that distance; every other pixel stays 0.  DESIGN.md
// section 4n has the definition in full.
//
// One 64-bit key per pixel:  d << 24 | id  of the best path known so far, GE_UNREACHED for a region pixel no path has reached,
// GE_OUTSIDE for a pixel that is not in the region (so the mask is read once).  The result is the fixed point of
//      key(p) <- min(key(p), min over the 4-neighbours q of key(q) + (1 << 24))        for p in the region
// (a neighbour that is outside or unreached offers a key above GE_UNREACHED, which no region pixel takes).  Monotone and bounded,
// as sweep.hpp asks: every key ever held is the (length, id) of a real path, keys only fall, and the least fixed point is unique.
// With connectivity 8 (unet_geodesic_sweeps_conn) the minimum runs over the eight neighbours and a step is one to any of them that
// lies in the region, whatever the two pixels beside a diagonal step are.  The argument does not look at which pixels count as
// neighbours: a key is still the (length, id) of a real path, now of 8-neighbour steps, keys only fall, and the bound is the same.
//
//   1. geo_init    the key plane from seeds and mask; counts the seed pixels outside the region and the ids outside [0, 2^24)
//   2. geo_sweep   sweep.hpp's tile relaxation over the keys, GE_OUTSIDE past the image.  With a limit, a key with d > max_steps
//                  is never stored: every key with d <= max_steps comes from a path whose every prefix has a smaller d, so none
//                  of them is lost.
//   3. geo_finish  id, distance, the unreached region pixels and the largest distance per image
#include "sweep.hpp"
#include "../../include/unet_hip.h"

namespace unet {

typedef unsigned long long ge_key;

static constexpr int GE_ID_BITS = 24;
static constexpr unsigned GE_ID_MASK = (1u << GE_ID_BITS) - 1;
static constexpr ge_key GE_STEP = 1ull << GE_ID_BITS;          // one more step, the same id
static constexpr ge_key GE_UNREACHED = 1ull << 60;             // above every key (d < 2^31: a key < 2^55)
static constexpr ge_key GE_OUTSIDE = 1ull << 61;               // not in the region; GE_OUTSIDE + GE_STEP does not wrap
static constexpr ge_key GE_UNLIMITED = 1ull << 32;             // above every d

__global__ __launch_bounds__(256) void geo_init_kernel(const int *__restrict__ seeds, const void *__restrict__ mask, int mask_dtype,
                                                       size_t npx, ge_key *__restrict__ key, unsigned *seeds_outside,
                                                       unsigned long long *status)
{
    const size_t img = (size_t)blockIdx.y * npx;
    unsigned outside = 0, bad = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const int id = seeds[img + e], region = mask_on(mask, mask_dtype, img + e);
        const bool seed = id > 0 && id <= (int)GE_ID_MASK;
        bad += id < 0 || id > (int)GE_ID_MASK;
        outside += seed && !region;
        key[img + e] = !region ? GE_OUTSIDE : seed ? (ge_key)id : GE_UNREACHED;
    }
    outside = block_sum256(outside);
    bad = block_sum256(bad);
    if (threadIdx.x == 0 && outside) __hip_atomic_fetch_add(&seeds_outside[blockIdx.y], outside, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == 0 && bad)
        __hip_atomic_fetch_add(&status[blockIdx.y], (unsigned long long)bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the SW_SEG pixels p[k * ALONG] of one line, relaxed forward (from the pixel before and the two ACROSS; with CONN == 8 from the
// four diagonal ones p[(k +- 1) * ALONG +- ACROSS] too) and backward (from the pixel after) in registers: v[k] is the key after
// both, bit k of the result says that it fell
template <int ALONG, int ACROSS, int CONN>
__device__ __forceinline__ unsigned ge_relax_line(const ge_key *p, ge_key lim, ge_key (&v)[SW_SEG])
{
    unsigned fell = 0;
    ge_key run = p[-ALONG];
#pragma unroll
    for (int k = 0; k < SW_SEG; ++k) {
        const ge_key own = p[k * ALONG], a = p[k * ALONG - ACROSS], b = p[k * ALONG + ACROSS];
        ge_key c = a < b ? a : b;
        if constexpr (CONN == 8) {
            const ge_key d0 = p[(k - 1) * ALONG - ACROSS], d1 = p[(k - 1) * ALONG + ACROSS];
            const ge_key d2 = p[(k + 1) * ALONG - ACROSS], d3 = p[(k + 1) * ALONG + ACROSS];
            const ge_key e = d0 < d1 ? d0 : d1, f = d2 < d3 ? d2 : d3;
            c = e < c ? e : c;
            c = f < c ? f : c;
        }
        c = (run < c ? run : c) + GE_STEP;
        const bool take = own <= GE_UNREACHED && c < own && c >> GE_ID_BITS <= lim;
        run = v[k] = take ? c : own;
        fell |= (unsigned)take << k;
    }
    run = p[SW_SEG * ALONG];
#pragma unroll
    for (int k = SW_SEG - 1; k >= 0; --k) {
        const ge_key c = run + GE_STEP;
        const bool take = v[k] <= GE_UNREACHED && c < v[k] && c >> GE_ID_BITS <= lim;
        run = v[k] = take ? c : v[k];
        fell |= (unsigned)take << k;
    }
    return fell;
}

template <int CONN>
__global__ __launch_bounds__(256) void geo_sweep_kernel(const ge_key *__restrict__ src, ge_key *__restrict__ dst, int H, int W,
                                                        ge_key lim, unsigned *changed)
{
    __shared__ ge_key s[SW_STAGED * SW_PITCH];                                       // 34.5 KiB
    const SweepTile tl = sweep_tile(H, W);
    sweep_stage(tl, H, W, [&](int i, bool in, size_t e, int, int, int, int) { s[i] = in ? src[e] : GE_OUTSIDE; });
    sweep_converge(s, [&](int o, ge_key (&v)[SW_SEG]) { return ge_relax_line<1, SW_PITCH, CONN>(s + o, lim, v); },
                   [&](int o, ge_key (&v)[SW_SEG]) { return ge_relax_line<SW_PITCH, 1, CONN>(s + o, lim, v); });
    sweep_write_back(tl, s, src, dst, W, changed, [](ge_key k, ge_key was) { return k < was; });
}

__global__ __launch_bounds__(256) void geo_finish_kernel(const ge_key *__restrict__ key, size_t npx, ge_key lim, int *__restrict__ out,
                                                         int *__restrict__ dist, unsigned *unreached, unsigned *max_dist)
{
    const size_t img = (size_t)blockIdx.y * npx;
    unsigned open = 0, far = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const ge_key k = key[img + e];
        const bool got = k < GE_UNREACHED && k >> GE_ID_BITS <= lim;
        const unsigned d = (unsigned)(k >> GE_ID_BITS);
        out[img + e] = got ? (int)(k & GE_ID_MASK) : 0;
        if (dist) dist[img + e] = got ? (int)d : -1;
        open += !got && k <= GE_UNREACHED;
        far = got && d > far ? d : far;
    }
    block_sum_max256(open, far);
    if (threadIdx.x != 0) return;                              // one add and one max per workgroup: the words are few
    if (open) __hip_atomic_fetch_add(&unreached[blockIdx.y], open, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (far) __hip_atomic_fetch_max(&max_dist[blockIdx.y], far, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace unet

using namespace unet;

static size_t ge_plane(int B, int H, int W) { return plane_bytes(B, H, W, sizeof(ge_key)); }
static ge_key ge_limit(long long max_steps) { return max_steps < 0 || (ge_key)max_steps > GE_UNLIMITED ? GE_UNLIMITED : (ge_key)max_steps; }

// [key plane 0, the current one between calls | key plane 1]
size_t unet_geodesic_scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 2 * ge_plane(B, H, W);
}

int unet_geodesic_init(const void *seeds_i32, const void *mask, int mask_dtype, int B, int H, int W, void *seeds_outside_u32,
                       void *status_u64, void *scratch, void *stream)
{
    ARG_CHECK(seeds_i32 && mask && seeds_outside_u32 && status_u64 && scratch && B > 0 && H > 0 && W > 0, "unet_geodesic_init: bad argument");
    ARG_CHECK(mask_dtype >= 0 && mask_dtype <= 3, "unet_geodesic_init: mask_dtype must be 0 (int64), 1 (float32), 2 (int32) or 3 (uint8)");
    ARG_CHECK(sizes_ok(B, H, W, 65535), "unet_geodesic_init: image too large (the limits of unet_grow_labels)");
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)H * W;
    HIP_TRY(hipMemsetAsync(seeds_outside_u32, 0, (size_t)B * sizeof(unsigned), st));
    HIP_TRY(hipMemsetAsync(status_u64, 0, (size_t)B * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(geo_init_kernel, dim3(grid_for(npx, 256, 2048), B), dim3(256), 0, st, (const int *)seeds_i32, mask, mask_dtype, npx,
                       (ge_key *)scratch, (unsigned *)seeds_outside_u32, (unsigned long long *)status_u64);
    HIP_TRY(hipGetLastError());
    return 0;
}

int unet_geodesic_sweeps_conn(int B, int H, int W, long long max_steps, int connectivity, int n_launches, void *changed_out_u32,
                              int first_slot, void *scratch, void *stream)
{
    ARG_CHECK(changed_out_u32 && scratch && B > 0 && H > 0 && W > 0 && n_launches > 0 && first_slot >= 0, "unet_geodesic_sweeps: bad argument");
    SW_CONN_CHECK("unet_geodesic_sweeps_conn");
    ARG_CHECK(sizes_ok(B, H, W, 65535), "unet_geodesic_sweeps: image too large (the limits of unet_grow_labels)");
    hipStream_t st = (hipStream_t)stream;
    const ge_key lim = ge_limit(max_steps);
    const auto kernel = connectivity == 8 ? geo_sweep_kernel<8> : geo_sweep_kernel<4>;
    return sweep_launches(scratch, (char *)scratch + ge_plane(B, H, W), sizeof(ge_key), B, H, W, n_launches, changed_out_u32, first_slot, st,
                          [&](dim3 grid, void *src, void *dst, unsigned *changed) {
                              hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, (const ge_key *)src, (ge_key *)dst, H, W, lim, changed);
                          });
}

int unet_geodesic_sweeps(int B, int H, int W, long long max_steps, int n_launches, void *changed_out_u32, int first_slot, void *scratch,
                         void *stream)
{
    return unet_geodesic_sweeps_conn(B, H, W, max_steps, 4, n_launches, changed_out_u32, first_slot, scratch, stream);
}

int unet_geodesic_finish(int B, int H, int W, long long max_steps, void *out_i32, void *dist_i32, void *unreached_u32, void *max_dist_u32,
                         void *scratch, void *stream)
{
    ARG_CHECK(out_i32 && unreached_u32 && max_dist_u32 && scratch && B > 0 && H > 0 && W > 0, "unet_geodesic_finish: bad argument");
    ARG_CHECK(sizes_ok(B, H, W, 65535), "unet_geodesic_finish: image too large (the limits of unet_grow_labels)");
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)H * W;
    HIP_TRY(hipMemsetAsync(unreached_u32, 0, (size_t)B * sizeof(unsigned), st));
    HIP_TRY(hipMemsetAsync(max_dist_u32, 0, (size_t)B * sizeof(unsigned), st));
    hipLaunchKernelGGL(geo_finish_kernel, dim3(grid_for(npx, 1024, 512), B), dim3(256), 0, st, (const ge_key *)scratch, npx, ge_limit(max_steps),
                       (int *)out_i32, (int *)dist_i32, (unsigned *)unreached_u32, (unsigned *)max_dist_u32);
    HIP_TRY(hipGetLastError());
    return 0;
}
