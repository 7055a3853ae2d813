// warp.hip — the topology-preserving warp behind the ISBI 2012 warping error (Jain et al. 2010; Ronneberger et al. 2015,
// Table 1), batched, on the device.  L starts as the ground truth and T is the prediction; a pixel with L != T that may flip
// and is simple in L (its flip changes neither the 4-connected foreground components nor the 8-connected background
// components) takes T's value, until no such pixel is left.  DESIGN.md section 4m has the definition in full.
//
//   1. warp_class_map / unet_grow_labels (only with a reach)   the maps  gt != 0  and  gt == 0  grown by max_dist2: a pixel has
//                  the other class within reach exactly when the grown map of the other class is set on it
//   2. warp_init   one state byte per pixel: bit 0 = L, bit 1 = T, bit 2 = may flip (user mask AND reach AND not on the image
//                  border); connectivity 8 stores the complements of L and T.  Counts L != T per image
//   3. warp_sweeps<P>   P passes per launch by temporal blocking.  Pass s of a sweep flips every simple candidate with
//                  (y & 1) * 2 + (x & 1) == s at once; two pixels of one pass are never 8-neighbours, so within a pass no
//                  thread reads a byte another one writes.  A workgroup owns a 64 x 64 tile and stages it with a halo of P
//                  pixels, clipped at the image, into LDS; it never flips the outermost ring of the staged region, so after pass
//                  j every pixel at least j away from an unclipped edge is exact, and the owned tile is after all P (a clipped
//                  edge is the image border, which never flips, and costs nothing).  Only the owned tile is written, to the
//                  other state plane: a neighbour's halo read never sees this launch's stores.
//                  A candidate stays one until it flips and nothing becomes one, so each thread reads its 36 pixels of the
//                  staged region once, keeps "still a candidate" as 36 bits in registers, and afterwards touches LDS only for
//                  those.  A staged region without candidates is copied; a sweep that flips nothing in it ends the launch for
//                  the workgroup (the region is at its fixed point).
//                  Flips of the owned tile go to flips[slot][sweep of the launch][b] by agent-scope adds
//   4. warp_finish L (complemented back for connectivity 8) as int32, the map L != T for unet_label_components, its count
//
// The 256-entry table of simple neighbourhoods is built on the host from the component definition (wp_simple) and handed to the
// kernel by value.
//
// Coherence (label.hip's rule): warp_sweeps reads plane A, which an earlier kernel wrote, and writes plane B, which no workgroup
// of the launch reads; the counters are only touched by agent-scope adds.  No word is handed from one workgroup to another inside
// a kernel.
#include "elem.hpp"
#include <cstdlib>
#include "../../include/unet_hip.h"

namespace unet {

static constexpr int WP_TILE = 64;                           // owned pixels per side of a workgroup's tile
static constexpr int WP_PMAX = 16;                           // most passes per launch = the widest halo
static constexpr int WP_PITCH = WP_TILE + 2 * WP_PMAX;       // LDS row pitch in bytes (96): 9 KiB for the staged region
static constexpr int WP_HALF = WP_PITCH / 2;                 // pixels of one pass per staged row (48), and rows of them
static constexpr int WP_PER_THREAD = WP_HALF * WP_HALF / 256;      // 9 pixels of each pass per thread
static constexpr int WP_SUB = WP_PMAX / 4;                   // sweep counters per slot of flips_out (4)
static constexpr unsigned char WP_L = 1, WP_T = 2, WP_MAY = 4;

struct WarpTable { unsigned w[8]; };                         // bit c: the neighbour code c (clockwise from NW, bits 0..7) is simple

__global__ __launch_bounds__(256) void warp_class_map_kernel(const void *__restrict__ gt, int dtype, size_t n, int invert,
                                                             int *__restrict__ map)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x)
        map[e] = mask_on(gt, dtype, e) ^ invert;
}

// near_fg / near_bg: the grown maps of gt != 0 / gt == 0, or null without a reach; mask: the user mask or null
__global__ __launch_bounds__(256) void warp_init_kernel(const void *__restrict__ gt, int gt_dtype, const void *__restrict__ pred,
                                                        int pred_dtype, const void *__restrict__ mask, int mask_dtype, int H, int W,
                                                        const int *__restrict__ near_fg, const int *__restrict__ near_bg, int complement,
                                                        unsigned char *__restrict__ state, unsigned *mismatch_before)
{
    const size_t npx = (size_t)H * W, img = (size_t)blockIdx.y * npx;
    unsigned n = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(e / W), x = (int)(e - (size_t)y * W);
        const int g = mask_on(gt, gt_dtype, img + e), p = mask_on(pred, pred_dtype, img + e);
        int may = y > 0 && y < H - 1 && x > 0 && x < W - 1;
        if (mask) may &= mask_on(mask, mask_dtype, img + e);
        if (near_fg) may &= (g ? near_bg[img + e] : near_fg[img + e]) != 0;
        n += g != p;
        state[img + e] = (unsigned char)((g ^ complement) * WP_L | (p ^ complement) * WP_T | may * WP_MAY);
    }
    n = block_sum256(n);
    if (threadIdx.x == 0 && n) __hip_atomic_fetch_add(&mismatch_before[blockIdx.y], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the k-th pixel of pass c of thread t in the staged region: pixel i = t + 256 k of the 48 x 48 pixels of that pass
__device__ __forceinline__ void wp_pixel(int t, int c, int k, int &ly, int &lx)
{
    const int i = t + 256 * k, cy = i / WP_HALF;
    ly = 2 * cy + (c >> 1);
    lx = 2 * (i - cy * WP_HALF) + (c & 1);
}

// VEC: W % 4 == 0 and both planes 4-byte aligned, so every staged and every owned row starts and ends on a word
template <int P, bool VEC>
__global__ __launch_bounds__(256) void warp_sweeps_kernel(const unsigned char *__restrict__ src, unsigned char *__restrict__ dst, int H,
                                                          int W, WarpTable tab, unsigned *flips)
{
    static_assert(P % 4 == 0 && P >= 4 && P <= WP_PMAX, "whole sweeps, and the halo fits the staged region");
    __shared__ unsigned sw[WP_PITCH * WP_PITCH / 4];
    __shared__ unsigned simple[8];
    unsigned char *s = (unsigned char *)sw;
    const int t = threadIdx.x, B = gridDim.z, b = blockIdx.z;
    const int oy = blockIdx.y * WP_TILE, ox = blockIdx.x * WP_TILE;                  // the owned tile, and the staged region:
    const int ry0 = max(0, oy - P), rx0 = max(0, ox - P);                            // even origins, so the pass of a pixel is
    const int RH = min(H, oy + WP_TILE + P) - ry0, RW = min(W, ox + WP_TILE + P) - rx0;   // that of its staged coordinates
    const int OH = min(H, oy + WP_TILE) - oy, OW = min(W, ox + WP_TILE) - ox;
    const size_t img = (size_t)b * H * W;
    if (t < 8) simple[t] = tab.w[t];
    if constexpr (VEC) {
        const int RW4 = RW >> 2;
        for (int i = t; i < RH * RW4; i += 256) {
            const int ly = i / RW4, wx = i - ly * RW4;
            sw[ly * (WP_PITCH / 4) + wx] = *(const unsigned *)(src + img + (size_t)(ry0 + ly) * W + rx0 + 4 * wx);
        }
    } else {
        for (int i = t; i < RH * RW; i += 256) {
            const int ly = i / RW, lx = i - ly * RW;
            s[ly * WP_PITCH + lx] = src[img + (size_t)(ry0 + ly) * W + rx0 + lx];
        }
    }
    __syncthreads();

    // bit 9 c + k: the k-th pixel of pass c of this thread is still a candidate / lies in the owned tile
    unsigned long long cand = 0, own = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < WP_PER_THREAD; ++k) {
            int ly, lx;
            wp_pixel(t, c, k, ly, lx);
            const unsigned long long bit = 1ull << (WP_PER_THREAD * c + k);
            if (ly >= 1 && ly < RH - 1 && lx >= 1 && lx < RW - 1) {                  // the outermost staged ring never flips
                const unsigned v = s[ly * WP_PITCH + lx];
                if ((v & WP_MAY) && ((v ^ (v >> 1)) & 1)) cand |= bit;
                const int gy = ry0 + ly - oy, gx = rx0 + lx - ox;
                if (gy >= 0 && gy < OH && gx >= 0 && gx < OW) own |= bit;
            }
        }

    unsigned cnt[P / 4];
#pragma unroll
    for (int q = 0; q < P / 4; ++q) cnt[q] = 0;
    if (__syncthreads_or(cand != 0)) {
        int flipped = 0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int c = j & 3;
            unsigned m = (unsigned)(cand >> (WP_PER_THREAD * c)) & ((1u << WP_PER_THREAD) - 1);
            while (m) {
                const int k = __ffs(m) - 1;
                m &= m - 1;
                int ly, lx;
                wp_pixel(t, c, k, ly, lx);
                unsigned char *q = s + ly * WP_PITCH + lx;
                const unsigned code = (q[-WP_PITCH - 1] & 1u) | (q[-WP_PITCH] & 1u) << 1 | (q[-WP_PITCH + 1] & 1u) << 2 | (q[1] & 1u) << 3 |
                                      (q[WP_PITCH + 1] & 1u) << 4 | (q[WP_PITCH] & 1u) << 5 | (q[WP_PITCH - 1] & 1u) << 6 | (q[-1] & 1u) << 7;
                if (simple[code >> 5] >> (code & 31) & 1) {
                    const unsigned long long bit = 1ull << (WP_PER_THREAD * c + k);
                    q[0] ^= WP_L;                                                    // L = T: never a candidate again
                    cand &= ~bit;
                    cnt[j >> 2] += (own & bit) != 0;
                    flipped = 1;
                }
            }
            if (c < 3) __syncthreads();
            else {
                if (!__syncthreads_or(flipped)) break;                               // an empty sweep: the region is at its fixed point
                flipped = 0;
            }
        }
    }

    if constexpr (VEC) {
        const int OW4 = OW >> 2, lx0 = (ox - rx0) >> 2;
        for (int i = t; i < OH * OW4; i += 256) {
            const int y = i / OW4, wx = i - y * OW4;
            *(unsigned *)(dst + img + (size_t)(oy + y) * W + ox + 4 * wx) = sw[(oy - ry0 + y) * (WP_PITCH / 4) + lx0 + wx];
        }
    } else {
        for (int i = t; i < OH * OW; i += 256) {
            const int y = i / OW, x = i - y * OW;
            dst[img + (size_t)(oy + y) * W + ox + x] = s[(oy - ry0 + y) * WP_PITCH + ox - rx0 + x];
        }
    }
#pragma unroll
    for (int q = 0; q < P / 4; ++q) {
        const unsigned n = wave_sum(cnt[q]);
        if ((t & 63) == 0 && n) __hip_atomic_fetch_add(&flips[(size_t)q * B + b], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void warp_finish_kernel(const unsigned char *__restrict__ state, size_t npx, int complement,
                                                          int *__restrict__ warped, float *__restrict__ mismatch_map, unsigned *mismatch)
{
    const size_t img = (size_t)blockIdx.y * npx;
    unsigned n = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const unsigned v = state[img + e];
        const unsigned differs = (v ^ (v >> 1)) & 1;
        warped[img + e] = (int)((v & WP_L) ^ (unsigned)complement);
        mismatch_map[img + e] = (float)differs;
        n += differs;
    }
    n = block_sum256(n);
    if (threadIdx.x == 0 && n) __hip_atomic_fetch_add(&mismatch[blockIdx.y], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// components of the cells with value v among the 8 neighbours (g[4], the centre, is in neither class), 4- or 8-connected;
// touching: only those that hold a 4-neighbour of the centre
static int wp_components(const int g[9], int v, bool diagonal, bool touching)
{
    bool seen[9] = {false};
    int n = 0;
    for (int s0 = 0; s0 < 9; ++s0) {
        if (s0 == 4 || g[s0] != v || seen[s0]) continue;
        int stack[9], top = 0;
        bool touches = false;
        stack[top++] = s0;
        seen[s0] = true;
        while (top) {
            const int c = stack[--top], cy = c / 3, cx = c % 3;
            touches |= std::abs(cy - 1) + std::abs(cx - 1) == 1;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int ny = cy + dy, nx = cx + dx, q = ny * 3 + nx;
                    if ((!dy && !dx) || (!diagonal && dy && dx) || ny < 0 || ny > 2 || nx < 0 || nx > 2) continue;
                    if (q == 4 || g[q] != v || seen[q]) continue;
                    seen[q] = true;
                    stack[top++] = q;
                }
        }
        n += touching ? touches : 1;
    }
    return n;
}

// the definition: among the 8 neighbours, exactly one 4-connected foreground component that holds a 4-neighbour of the pixel,
// and exactly one 8-connected background component
static bool wp_simple(int code)
{
    static const int cell[8] = {0, 1, 2, 5, 8, 7, 6, 3};       // clockwise from NW
    int g[9] = {0, 0, 0, 0, -1, 0, 0, 0, 0};
    for (int k = 0; k < 8; ++k) g[cell[k]] = code >> k & 1;
    return wp_components(g, 1, false, true) == 1 && wp_components(g, 0, true, false) == 1;
}

static const WarpTable &wp_table()
{
    static const WarpTable t = [] {
        WarpTable w = {};
        for (int c = 0; c < 256; ++c)
            if (wp_simple(c)) w.w[c >> 5] |= 1u << (c & 31);
        return w;
    }();
    return t;
}

} // namespace unet

using namespace unet;

static size_t wp_state(int B, int H, int W) { return plane_bytes(B, H, W, 1); }
static size_t wp_ints(int B, int H, int W) { return plane_bytes(B, H, W, sizeof(int)); }
static bool wp_dtype_ok(int d) { return d >= 0 && d <= 3; }

// [state plane B | class map | grown map of gt != 0 | grown map of gt == 0 | the scratch of unet_grow_labels]
size_t unet_warp_scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return wp_state(B, H, W) + 3 * wp_ints(B, H, W) + unet_grow_labels_scratch_bytes(B, H, W);
}

int unet_warp_init(const void *gt, int gt_dtype, const void *pred, int pred_dtype, const void *mask, int mask_dtype, int B, int H, int W,
                   long long max_dist2, int connectivity, void *state_u8, void *mismatch_before_u32, void *scratch, void *stream)
{
    ARG_CHECK(gt && pred && state_u8 && mismatch_before_u32 && scratch && B > 0 && H > 0 && W > 0, "unet_warp_init: bad argument");
    ARG_CHECK(wp_dtype_ok(gt_dtype) && wp_dtype_ok(pred_dtype) && (!mask || wp_dtype_ok(mask_dtype)),
              "unet_warp_init: a dtype must be 0 (int64), 1 (float32), 2 (int32) or 3 (uint8)");
    ARG_CHECK(connectivity == 4 || connectivity == 8, "unet_warp_init: connectivity must be 4 or 8");
    ARG_CHECK(sizes_ok(B, H, W, 65535), "unet_warp_init: image too large (the limits of unet_grow_labels)");
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)H * W;
    const int *near_fg = nullptr, *near_bg = nullptr;
    if (max_dist2 >= 0) {
        char *s = (char *)scratch + wp_state(B, H, W);
        int *map = (int *)s, *grown[2] = {(int *)(s + wp_ints(B, H, W)), (int *)(s + 2 * wp_ints(B, H, W))};
        void *grow_scratch = s + 3 * wp_ints(B, H, W);
        for (int other = 0; other < 2; ++other) {               // 0: the map gt != 0, 1: the map gt == 0
            hipLaunchKernelGGL(warp_class_map_kernel, dim3(grid_for(B * npx)), dim3(256), 0, st, gt, gt_dtype, B * npx, other, map);
            if (int rc = unet_grow_labels(map, B, H, W, max_dist2, grown[other], grow_scratch, stream)) return rc;
        }
        near_fg = grown[0];
        near_bg = grown[1];
    }
    HIP_TRY(hipMemsetAsync(mismatch_before_u32, 0, (size_t)B * sizeof(unsigned), st));
    hipLaunchKernelGGL(warp_init_kernel, dim3(grid_for(npx, 256, 2048), B), dim3(256), 0, st, gt, gt_dtype, pred, pred_dtype, mask,
                       mask_dtype, H, W, near_fg, near_bg, connectivity == 8 ? 1 : 0, (unsigned char *)state_u8,
                       (unsigned *)mismatch_before_u32);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int P>
static void wp_launch(bool vec, dim3 grid, hipStream_t st, const unsigned char *src, unsigned char *dst, int H, int W, unsigned *flips)
{
    dispatch_bool(vec, [&](auto v) {
        hipLaunchKernelGGL((warp_sweeps_kernel<P, decltype(v)::value>), grid, dim3(256), 0, st, src, dst, H, W, wp_table(), flips);
    });
}

int unet_warp_sweeps(void *state_u8, int B, int H, int W, int passes_per_launch, int n_launches, void *flips_out_u32, int first_slot,
                     void *scratch, void *stream)
{
    ARG_CHECK(state_u8 && flips_out_u32 && scratch && B > 0 && H > 0 && W > 0 && n_launches > 0 && first_slot >= 0,
              "unet_warp_sweeps: bad argument");
    ARG_CHECK(passes_per_launch == 4 || passes_per_launch == 8 || passes_per_launch == 16,
              "unet_warp_sweeps: passes_per_launch must be 4, 8 or 16");
    ARG_CHECK(sizes_ok(B, H, W, 65535), "unet_warp_sweeps: image too large (the limits of unet_grow_labels)");
    hipStream_t st = (hipStream_t)stream;
    const size_t slot = (size_t)WP_SUB * B;
    unsigned *flips = (unsigned *)flips_out_u32 + (size_t)first_slot * slot;
    HIP_TRY(hipMemsetAsync(flips, 0, (size_t)n_launches * slot * sizeof(unsigned), st));
    unsigned char *plane[2] = {(unsigned char *)state_u8, (unsigned char *)scratch};
    const bool vec = W % 4 == 0 && ((uintptr_t)plane[0] | (uintptr_t)plane[1]) % 4 == 0;
    const dim3 grid(cdiv(W, WP_TILE), cdiv(H, WP_TILE), B);
    for (int l = 0; l < n_launches; ++l) {
        const unsigned char *src = plane[l & 1];
        unsigned char *dst = plane[~l & 1];
        if (passes_per_launch == 4) wp_launch<4>(vec, grid, st, src, dst, H, W, flips + l * slot);
        else if (passes_per_launch == 8) wp_launch<8>(vec, grid, st, src, dst, H, W, flips + l * slot);
        else wp_launch<16>(vec, grid, st, src, dst, H, W, flips + l * slot);
    }
    HIP_TRY(hipGetLastError());
    if (n_launches & 1) HIP_TRY(hipMemcpyAsync(plane[0], plane[1], (size_t)B * H * W, hipMemcpyDeviceToDevice, st));
    return 0;
}

int unet_warp_finish(const void *state_u8, int B, int H, int W, int connectivity, void *warped_i32, void *mismatch_map_f32,
                     void *mismatch_u32, void *stream)
{
    ARG_CHECK(state_u8 && warped_i32 && mismatch_map_f32 && mismatch_u32 && B > 0 && H > 0 && W > 0, "unet_warp_finish: bad argument");
    ARG_CHECK(connectivity == 4 || connectivity == 8, "unet_warp_finish: connectivity must be 4 or 8");
    ARG_CHECK(sizes_ok(B, H, W, 65535), "unet_warp_finish: image too large (the limits of unet_grow_labels)");
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)H * W;
    HIP_TRY(hipMemsetAsync(mismatch_u32, 0, (size_t)B * sizeof(unsigned), st));
    hipLaunchKernelGGL(warp_finish_kernel, dim3(grid_for(npx, 256, 2048), B), dim3(256), 0, st, (const unsigned char *)state_u8, npx,
                       connectivity == 8 ? 1 : 0, (int *)warped_i32, (float *)mismatch_map_f32, (unsigned *)mismatch_u32);
    HIP_TRY(hipGetLastError());
    return 0;
}
