// flood.hip — seeded watershed: flooding of an intensity landscape from markers inside a region (functions.watershed), batched, on
// the device.  The region is mask != 0 (everything without a mask); every pixel has an integer level v(p) in [0, 65536); a seed
// pixel inside the region is a source.  The semantics are Vincent-Soille immersion with exact geodesic influence zones on
// plateaus; DESIGN.md section 4r has the definition in full, the argument and the counter-example to a one-key form.
//
// Stage 1, one 64-bit key per pixel:  L << 32 | d,  L the pass height at which the flood reaches the pixel and d the number of
// steps inside the plateau {L} from the pixels that were flooded before that level; 0 on a source, FL_UNREACHED for a region pixel
// no path has reached, FL_OUTSIDE for a pixel that is not in the region.  One 4-neighbour step onto q extends a key (L, d) to
//      ext((L, d), v(q)) = (L, d + 1)  if v(q) <= L,   (v(q), 1)  otherwise
// and the result is the least fixed point of  key(q) <- min(key(q), ext(min over the 4-neighbours p of key(p), v(q))).  ext is
// isotone in the key (a smaller key never extends to a larger one), so the minimum may be taken before the extension, every key
// ever held is the cost of a real path, keys only fall, and any order of relaxation reaches the same fixed point: geo.hip's
// argument with another step.  (An outside or unreached neighbour offers a key above FL_UNREACHED, which no region pixel takes.)
//
// Stage 2, one id per pixel, given the FINAL keys: a neighbour p is a parent of q when ext(key(p), v(q)) == key(q); a source
// keeps its seed id and every other reached pixel takes the least id among its parents.  A parent's key is strictly smaller, so
// the relation has no cycle, ids only fall, and again the fixed point is unique.  The id is not part of the key: extension is
// not isotone in it (a pixel first reached over a high pass by a small id would go on offering that id after a lower path with a
// larger id has taken it over), so the ids wait until the keys are final.
//
//   1. flood_init    quantises the image to the u16 level plane, writes the key plane and the id plane (seed ids on sources,
//                    FL_NONE elsewhere); counts the seed pixels outside the region, the bad ids and the bad image values
//   2. flood_sweep   sweep.hpp's tile relaxation over the keys (geo_sweep with the extension above in the place of + GE_STEP); the
//                    levels are staged beside them.  A key with L > max_level is never stored: every prefix of a path has a
//                    smaller or equal L, so no key below is lost.
//   3. flood_assign  the same relaxation over ids.  The four parent bits of every owned pixel are formed once, while staging, from
//                    the keys and levels in global memory, which this kernel only reads; the loop then works on the staged ids
//                    and those bits: an id moves along any straight run of parent links in one phase.  Two id planes, ping-pong.
//                    (Eight bits and the diagonal ids with connectivity 8, below.)
//   4. flood_finish  ids, pass levels, plateau distances, the unreached region pixels and the largest level reached per image
//
// Monotone and bounded, as sweep.hpp asks: keys and ids are bounded below and only fall.
//
// Connectivity 8 (unet_flood_sweeps_conn, unet_flood_assign_conn): the same ext; a step goes to any of the eight neighbours in
// the region, whatever the two pixels beside a diagonal step are, the minimum of stage 1 runs over eight neighbours and a parent
// in stage 2 is any of the eight whose key extends to exactly key(q).  Neither argument above uses which pixels are neighbours:
// ext is as isotone, a parent's key as strictly smaller.  The eight parent bits fill the staged byte; the diagonal tests carry
// their own bounds, so past the image there is no parent.  Both stages of one flood take the same connectivity.
#include "sweep.hpp"
#include "../../include/unet_hip.h"

namespace unet {

typedef unsigned long long fl_key;

static constexpr int FL_L_SHIFT = 32;                          // key = L << 32 | d, d < 2^31 (H * W < 2^31)
static constexpr int FL_LEVELS = 1 << 16;                      // levels are in [0, FL_LEVELS)
static constexpr int FL_ID_END = 1 << 24;                      // ids are in [1, FL_ID_END)
static constexpr unsigned FL_NONE = 1u << 30;                  // id plane: no id (yet), above every id
static constexpr fl_key FL_UNREACHED = 1ull << 60;             // above every key (L < 2^16: a key < 2^48)
static constexpr fl_key FL_OUTSIDE = 1ull << 61;               // not in the region; its extension does not wrap
static constexpr int FL_LEFT = 1, FL_RIGHT = 2, FL_UP = 4, FL_DOWN = 8;     // parent bits
static constexpr int FL_UP_LEFT = 16, FL_UP_RIGHT = 32, FL_DOWN_LEFT = 64, FL_DOWN_RIGHT = 128;      // connectivity 8: the byte is full

// one step from a pixel with key k onto a pixel of level v
__device__ __forceinline__ fl_key fl_ext(fl_key k, unsigned v)
{
    return k >> FL_L_SHIFT >= v ? k + 1 : (fl_key)v << FL_L_SHIFT | 1;
}

// the level of element e of the image (dtype 0: int64, 1: float32 with `levels`, 2: int32, 3: uint8); bad: not representable
__device__ __forceinline__ unsigned fl_level(const void *image, int dtype, int levels, size_t e, unsigned &bad)
{
    if (dtype == 1) {
        const float x = ((const float *)image)[e];
        bad += !__builtin_isfinite(x);
        const float f = floorf(x * (float)levels), top = (float)(levels - 1);
        return f >= top ? (unsigned)(levels - 1) : f > 0.0f ? (unsigned)f : 0u;            // a NaN gives 0 and is counted
    }
    const long long x = dtype == 0 ? ((const long long *)image)[e] : dtype == 2 ? (long long)((const int *)image)[e]
                                                                                 : (long long)((const unsigned char *)image)[e];
    const bool ok = x >= 0 && x < FL_LEVELS;
    bad += !ok;
    return ok ? (unsigned)x : 0u;
}

__global__ __launch_bounds__(256) void flood_init_kernel(const int *__restrict__ seeds, const void *__restrict__ image, int image_dtype,
                                                         int levels, const void *__restrict__ mask, int mask_dtype, size_t npx,
                                                         fl_key *__restrict__ key, unsigned *__restrict__ ids,
                                                         unsigned short *__restrict__ level, unsigned *seeds_outside,
                                                         unsigned long long *bad_ids, unsigned long long *bad_values)
{
    const size_t img = (size_t)blockIdx.y * npx;
    unsigned outside = 0, bad = 0, badv = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const int id = seeds[img + e], region = mask ? mask_on(mask, mask_dtype, img + e) : 1;
        const bool seed = id > 0 && id < FL_ID_END;
        bad += id < 0 || id >= FL_ID_END;
        outside += seed && !region;
        level[img + e] = (unsigned short)fl_level(image, image_dtype, levels, img + e, badv);
        key[img + e] = !region ? FL_OUTSIDE : seed ? 0ull : FL_UNREACHED;
        ids[img + e] = seed && region ? (unsigned)id : FL_NONE;
    }
    outside = block_sum256(outside);
    bad = block_sum256(bad);
    badv = block_sum256(badv);
    if (threadIdx.x != 0) return;
    if (outside) __hip_atomic_fetch_add(&seeds_outside[blockIdx.y], outside, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (bad) __hip_atomic_fetch_add(&bad_ids[blockIdx.y], (unsigned long long)bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (badv) __hip_atomic_fetch_add(&bad_values[blockIdx.y], (unsigned long long)badv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- stage 1 ------------------------------------------------------------------------------------------------------------------

// geo.hip's ge_relax_line with fl_ext: the SW_SEG pixels p[k * ALONG] of one line and their levels lv[k * ALONG], relaxed forward
// (from the pixel before and the two ACROSS) and backward (from the pixel after) in registers
template <int ALONG, int ACROSS, int CONN>
__device__ __forceinline__ unsigned fl_relax_line(const fl_key *p, const unsigned short *lv, fl_key lim, fl_key (&v)[SW_SEG])
{
    unsigned fell = 0;
    fl_key run = p[-ALONG];
#pragma unroll
    for (int k = 0; k < SW_SEG; ++k) {
        const fl_key own = p[k * ALONG], a = p[k * ALONG - ACROSS], b = p[k * ALONG + ACROSS];
        fl_key c = a < b ? a : b;
        if constexpr (CONN == 8) {
            const fl_key d0 = p[(k - 1) * ALONG - ACROSS], d1 = p[(k - 1) * ALONG + ACROSS];
            const fl_key d2 = p[(k + 1) * ALONG - ACROSS], d3 = p[(k + 1) * ALONG + ACROSS];
            const fl_key e = d0 < d1 ? d0 : d1, f = d2 < d3 ? d2 : d3;
            c = e < c ? e : c;
            c = f < c ? f : c;
        }
        c = fl_ext(run < c ? run : c, lv[k * ALONG]);
        const bool take = own <= FL_UNREACHED && c < own && c >> FL_L_SHIFT <= lim;
        run = v[k] = take ? c : own;
        fell |= (unsigned)take << k;
    }
    run = p[SW_SEG * ALONG];
#pragma unroll
    for (int k = SW_SEG - 1; k >= 0; --k) {
        const fl_key c = fl_ext(run, lv[k * ALONG]);
        const bool take = v[k] <= FL_UNREACHED && c < v[k] && c >> FL_L_SHIFT <= lim;
        run = v[k] = take ? c : v[k];
        fell |= (unsigned)take << k;
    }
    return fell;
}

template <int CONN>
__global__ __launch_bounds__(256) void flood_sweep_kernel(const fl_key *__restrict__ src, fl_key *__restrict__ dst,
                                                          const unsigned short *__restrict__ level, int H, int W, fl_key lim,
                                                          unsigned *changed)
{
    __shared__ fl_key s[SW_STAGED * SW_PITCH];                                       // 34.5 KiB
    __shared__ unsigned short sl[SW_STAGED * SW_PITCH];                              // 8.6 KiB
    const SweepTile tl = sweep_tile(H, W);
    sweep_stage(tl, H, W, [&](int i, bool in, size_t e, int, int, int, int) {
        s[i] = in ? src[e] : FL_OUTSIDE;
        sl[i] = in ? level[e] : (unsigned short)0;
    });
    sweep_converge(s, [&](int o, fl_key (&v)[SW_SEG]) { return fl_relax_line<1, SW_PITCH, CONN>(s + o, sl + o, lim, v); },
                   [&](int o, fl_key (&v)[SW_SEG]) { return fl_relax_line<SW_PITCH, 1, CONN>(s + o, sl + o, lim, v); });
    sweep_write_back(tl, s, src, dst, W, changed, [](fl_key k, fl_key was) { return k < was; });
}

// ---- stage 2 ------------------------------------------------------------------------------------------------------------------

// the SW_SEG ids p[k * ALONG] of one line and their parent bits: forward, an id takes the least of its own, of the pixel before
// (bit PREV) and of the two ACROSS (bits LO, HI); backward, of the pixel after (bit NEXT).  With CONN == 8 the forward pass also
// takes the four diagonal ids p[(k -+ 1) * ALONG -+ ACROSS] under their bits: PREV_LO, PREV_HI before the pixel, NEXT_LO, NEXT_HI after
template <int ALONG, int ACROSS, int PREV, int NEXT, int LO, int HI, int CONN, int PREV_LO = 0, int PREV_HI = 0, int NEXT_LO = 0, int NEXT_HI = 0>
__device__ __forceinline__ unsigned fl_assign_line(const unsigned *p, const unsigned char *par, unsigned (&v)[SW_SEG])
{
    unsigned fell = 0;
    unsigned run = p[-ALONG];
#pragma unroll
    for (int k = 0; k < SW_SEG; ++k) {
        const unsigned own = p[k * ALONG], a = p[k * ALONG - ACROSS], b = p[k * ALONG + ACROSS], bits = par[k * ALONG];
        unsigned c = own;
        c = (bits & PREV) && run < c ? run : c;
        c = (bits & LO) && a < c ? a : c;
        c = (bits & HI) && b < c ? b : c;
        if constexpr (CONN == 8) {
            const unsigned d0 = p[(k - 1) * ALONG - ACROSS], d1 = p[(k - 1) * ALONG + ACROSS];
            const unsigned d2 = p[(k + 1) * ALONG - ACROSS], d3 = p[(k + 1) * ALONG + ACROSS];
            c = (bits & PREV_LO) && d0 < c ? d0 : c;
            c = (bits & PREV_HI) && d1 < c ? d1 : c;
            c = (bits & NEXT_LO) && d2 < c ? d2 : c;
            c = (bits & NEXT_HI) && d3 < c ? d3 : c;
        }
        fell |= (unsigned)(c < own) << k;
        run = v[k] = c;
    }
    run = p[SW_SEG * ALONG];
#pragma unroll
    for (int k = SW_SEG - 1; k >= 0; --k) {
        const bool take = (par[k * ALONG] & NEXT) && run < v[k];
        run = v[k] = take ? run : v[k];
        fell |= (unsigned)take << k;
    }
    return fell;
}

template <int CONN>
__global__ __launch_bounds__(256) void flood_assign_kernel(const fl_key *__restrict__ key, const unsigned short *__restrict__ level,
                                                           const unsigned *__restrict__ src, unsigned *__restrict__ dst, int H, int W,
                                                           unsigned *changed)
{
    __shared__ unsigned s[SW_STAGED * SW_PITCH];                                     // 17.3 KiB
    __shared__ unsigned char sp[SW_STAGED * SW_PITCH];                               // 4.3 KiB
    const SweepTile tl = sweep_tile(H, W);
    sweep_stage(tl, H, W, [&](int i, bool in, size_t, int ly, int lx, int gy, int gx) {      // past the image: no id and no parent
        const size_t e = tl.img + (size_t)(in ? gy : 0) * W + (in ? gx : 0);
        s[i] = in ? src[e] : FL_NONE;
        int bits = 0;
        if (in && ly >= 1 && ly <= SW_TILE && lx >= 1 && lx <= SW_TILE) {            // an owned pixel: which neighbours are parents
            const fl_key k = key[e];
            if (k < FL_UNREACHED) {                                                  // (no extension is 0: a source has none)
                const unsigned v = level[e];
                bits |= gx > 0 && fl_ext(key[e - 1], v) == k ? FL_LEFT : 0;
                bits |= gx < W - 1 && fl_ext(key[e + 1], v) == k ? FL_RIGHT : 0;
                bits |= gy > 0 && fl_ext(key[e - W], v) == k ? FL_UP : 0;
                bits |= gy < H - 1 && fl_ext(key[e + W], v) == k ? FL_DOWN : 0;
                if constexpr (CONN == 8) {                                           // past the image there is no parent
                    bits |= gy > 0 && gx > 0 && fl_ext(key[e - W - 1], v) == k ? FL_UP_LEFT : 0;
                    bits |= gy > 0 && gx < W - 1 && fl_ext(key[e - W + 1], v) == k ? FL_UP_RIGHT : 0;
                    bits |= gy < H - 1 && gx > 0 && fl_ext(key[e + W - 1], v) == k ? FL_DOWN_LEFT : 0;
                    bits |= gy < H - 1 && gx < W - 1 && fl_ext(key[e + W + 1], v) == k ? FL_DOWN_RIGHT : 0;
                }
            }
        }
        sp[i] = (unsigned char)bits;
    });
    sweep_converge(s,
                   [&](int o, unsigned (&v)[SW_SEG]) {
                       return fl_assign_line<1, SW_PITCH, FL_LEFT, FL_RIGHT, FL_UP, FL_DOWN, CONN, FL_UP_LEFT, FL_DOWN_LEFT, FL_UP_RIGHT,
                                             FL_DOWN_RIGHT>(s + o, sp + o, v);
                   },
                   [&](int o, unsigned (&v)[SW_SEG]) {
                       return fl_assign_line<SW_PITCH, 1, FL_UP, FL_DOWN, FL_LEFT, FL_RIGHT, CONN, FL_UP_LEFT, FL_UP_RIGHT,
                                             FL_DOWN_LEFT, FL_DOWN_RIGHT>(s + o, sp + o, v);
                   });
    sweep_write_back(tl, s, src, dst, W, changed, [](unsigned id, unsigned was) { return id < was; });
}

__global__ __launch_bounds__(256) void flood_finish_kernel(const fl_key *__restrict__ key, const unsigned *__restrict__ ids, size_t npx,
                                                           int *__restrict__ out, int *__restrict__ pass_level, int *__restrict__ dist,
                                                           unsigned *unreached, unsigned *max_level)
{
    const size_t img = (size_t)blockIdx.y * npx;
    unsigned open = 0, top = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const fl_key k = key[img + e];
        const unsigned id = ids[img + e];
        const bool got = k < FL_UNREACHED && id < FL_NONE;
        const unsigned L = (unsigned)(k >> FL_L_SHIFT);
        out[img + e] = got ? (int)id : 0;
        if (pass_level) pass_level[img + e] = got ? (int)L : -1;
        if (dist) dist[img + e] = got ? (int)(unsigned)k : -1;
        open += !got && k <= FL_UNREACHED;
        top = got && L > top ? L : top;
    }
    block_sum_max256(open, top);
    if (threadIdx.x != 0) return;                              // one add and one max per workgroup: the words are few
    if (open) __hip_atomic_fetch_add(&unreached[blockIdx.y], open, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (top) __hip_atomic_fetch_max(&max_level[blockIdx.y], top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace unet

using namespace unet;

static fl_key fl_limit(long long max_level) { return max_level < 0 || max_level >= FL_LEVELS ? (fl_key)(FL_LEVELS - 1) : (fl_key)max_level; }

// [key plane 0, the current one between calls | key plane 1 | id plane 0, the current one between calls | id plane 1 | levels]
struct FlScratch {
    fl_key *key[2];
    unsigned *ids[2];
    unsigned short *level;
};
static FlScratch fl_scratch(void *scratch, int B, int H, int W)
{
    const size_t kb = plane_bytes(B, H, W, sizeof(fl_key)), ib = plane_bytes(B, H, W, sizeof(unsigned));
    char *p = (char *)scratch;
    return {{(fl_key *)p, (fl_key *)(p + kb)}, {(unsigned *)(p + 2 * kb), (unsigned *)(p + 2 * kb + ib)}, (unsigned short *)(p + 2 * kb + 2 * ib)};
}

size_t unet_flood_scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 2 * plane_bytes(B, H, W, sizeof(fl_key)) + 2 * plane_bytes(B, H, W, sizeof(unsigned)) + plane_bytes(B, H, W, sizeof(unsigned short));
}

int unet_flood_init(const void *seeds_i32, const void *image, int image_dtype, int levels, const void *mask, int mask_dtype, int B, int H,
                    int W, void *seeds_outside_u32, void *status_u64, void *scratch, void *stream)
{
    ARG_CHECK(seeds_i32 && image && seeds_outside_u32 && status_u64 && scratch && B > 0 && H > 0 && W > 0, "unet_flood_init: bad argument");
    ARG_CHECK(image_dtype >= 0 && image_dtype <= 3, "unet_flood_init: image_dtype must be 0 (int64), 1 (float32), 2 (int32) or 3 (uint8)");
    ARG_CHECK(image_dtype != 1 || (levels >= 1 && levels <= FL_LEVELS), "unet_flood_init: a float32 image needs levels in [1, 65536]");
    ARG_CHECK(!mask || (mask_dtype >= 0 && mask_dtype <= 3), "unet_flood_init: mask_dtype must be 0 (int64), 1 (float32), 2 (int32) or 3 (uint8)");
    ARG_CHECK(sizes_ok(B, H, W, 65535), "unet_flood_init: image too large (the limits of unet_grow_labels)");
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)H * W;
    const FlScratch s = fl_scratch(scratch, B, H, W);
    HIP_TRY(hipMemsetAsync(seeds_outside_u32, 0, (size_t)B * sizeof(unsigned), st));
    HIP_TRY(hipMemsetAsync(status_u64, 0, (size_t)2 * B * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(flood_init_kernel, dim3(grid_for(npx, 256, 2048), B), dim3(256), 0, st, (const int *)seeds_i32, image, image_dtype, levels,
                       mask, mask_dtype, npx, s.key[0], s.ids[0], s.level, (unsigned *)seeds_outside_u32, (unsigned long long *)status_u64,
                       (unsigned long long *)status_u64 + B);
    HIP_TRY(hipGetLastError());
    return 0;
}

int unet_flood_sweeps_conn(int B, int H, int W, long long max_level, int connectivity, int n_launches, void *changed_out_u32, int first_slot,
                           void *scratch, void *stream)
{
    ARG_CHECK(changed_out_u32 && scratch && B > 0 && H > 0 && W > 0 && n_launches > 0 && first_slot >= 0, "unet_flood_sweeps: bad argument");
    SW_CONN_CHECK("unet_flood_sweeps_conn");
    ARG_CHECK(sizes_ok(B, H, W, 65535), "unet_flood_sweeps: image too large (the limits of unet_grow_labels)");
    hipStream_t st = (hipStream_t)stream;
    const FlScratch s = fl_scratch(scratch, B, H, W);
    const fl_key lim = fl_limit(max_level);
    const auto kernel = connectivity == 8 ? flood_sweep_kernel<8> : flood_sweep_kernel<4>;
    return sweep_launches(s.key[0], s.key[1], sizeof(fl_key), B, H, W, n_launches, changed_out_u32, first_slot, st,
                          [&](dim3 grid, void *src, void *dst, unsigned *changed) {
                              hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, (const fl_key *)src, (fl_key *)dst,
                                                 (const unsigned short *)s.level, H, W, lim, changed);
                          });
}

int unet_flood_sweeps(int B, int H, int W, long long max_level, int n_launches, void *changed_out_u32, int first_slot, void *scratch,
                      void *stream)
{
    return unet_flood_sweeps_conn(B, H, W, max_level, 4, n_launches, changed_out_u32, first_slot, scratch, stream);
}

// Takes on trust that the keys are final: a launch of unet_flood_sweeps_conn with the same connectivity that changed nothing has
// been seen by the caller.
int unet_flood_assign_conn(int B, int H, int W, int connectivity, int n_launches, void *changed_out_u32, int first_slot, void *scratch,
                           void *stream)
{
    ARG_CHECK(changed_out_u32 && scratch && B > 0 && H > 0 && W > 0 && n_launches > 0 && first_slot >= 0, "unet_flood_assign: bad argument");
    SW_CONN_CHECK("unet_flood_assign_conn");
    ARG_CHECK(sizes_ok(B, H, W, 65535), "unet_flood_assign: image too large (the limits of unet_grow_labels)");
    hipStream_t st = (hipStream_t)stream;
    const FlScratch s = fl_scratch(scratch, B, H, W);
    const auto kernel = connectivity == 8 ? flood_assign_kernel<8> : flood_assign_kernel<4>;
    return sweep_launches(s.ids[0], s.ids[1], sizeof(unsigned), B, H, W, n_launches, changed_out_u32, first_slot, st,
                          [&](dim3 grid, void *src, void *dst, unsigned *changed) {
                              hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, (const fl_key *)s.key[0], (const unsigned short *)s.level,
                                                 (const unsigned *)src, (unsigned *)dst, H, W, changed);
                          });
}

int unet_flood_assign(int B, int H, int W, int n_launches, void *changed_out_u32, int first_slot, void *scratch, void *stream)
{
    return unet_flood_assign_conn(B, H, W, 4, n_launches, changed_out_u32, first_slot, scratch, stream);
}

int unet_flood_finish(int B, int H, int W, void *out_i32, void *pass_level_i32, void *dist_i32, void *unreached_u32, void *max_level_u32,
                      void *scratch, void *stream)
{
    ARG_CHECK(out_i32 && unreached_u32 && max_level_u32 && scratch && B > 0 && H > 0 && W > 0, "unet_flood_finish: bad argument");
    ARG_CHECK(sizes_ok(B, H, W, 65535), "unet_flood_finish: image too large (the limits of unet_grow_labels)");
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)H * W;
    const FlScratch s = fl_scratch(scratch, B, H, W);
    HIP_TRY(hipMemsetAsync(unreached_u32, 0, (size_t)B * sizeof(unsigned), st));
    HIP_TRY(hipMemsetAsync(max_level_u32, 0, (size_t)B * sizeof(unsigned), st));
    hipLaunchKernelGGL(flood_finish_kernel, dim3(grid_for(npx, 1024, 512), B), dim3(256), 0, st, (const fl_key *)s.key[0],
                       (const unsigned *)s.ids[0], npx, (int *)out_i32, (int *)pass_level_i32, (int *)dist_i32, (unsigned *)unreached_u32,
                       (unsigned *)max_level_u32);
    HIP_TRY(hipGetLastError());
    return 0;
}
