// clean.hip — cleaning a foreground mask between the argmax and the instance map, batched, on the device: fill holes, drop
// small cells and cells on the frame (scipy.ndimage.binary_fill_holes, skimage's remove_small_holes / remove_small_objects /
// clear_border), on label.hip's labelling with its attribute plane (label_roots, common.hpp: passes 1-3).
//
// unet_clean_mask:
//   holes  1-3 on the background with the dual connectivity, then
//   4. cl_fill     filled plane (uint8) = 1 on foreground, 2 on a background pixel whose component has no frame bit and an area
//                  <= max_hole_area, else 0; counts the holes (their roots) and their pixels
//   cells  1-3 on the filled plane's foreground with the connectivity given, then
//   5. cl_select   per pixel the action from the root's word (area < min_area: 3; frame bit and drop_border: 4; else 1 or,
//                  where cl_fill wrote 2, 2), the output mask and the counts
// A fixed list of launches for given arguments, every pixel a fixed number of times: the cost does not depend on how many holes
// or cells there are.  Every count is an integer sum: the results do not depend on the order of the atomics.
//
// Coherence (label.hip's rule): cl_fill and cl_select read what earlier kernels wrote; the info words are only touched by
// agent-scope adds.  Every hand-off is a kernel boundary.
#include "elem.hpp"
#include "../../include/unet_hip.h"

namespace unet {

enum { CI_HOLES = 0, CI_HOLE_PX = 1, CI_SMALL = 2, CI_SMALL_PX = 3, CI_BORDER = 4, CI_BORDER_PX = 5, CI_KEPT = 6, CI_WORDS = 7 };

// ---- 4. fill: the holes of the background labelling ---------------------------------------------------------------------------
// label == nullptr: no labelling was made (fill_holes off), filled = the foreground
__global__ __launch_bounds__(256) void cl_fill_kernel(const void *__restrict__ mask, int dtype, size_t npx, const int *__restrict__ label,
                                                      const unsigned *__restrict__ attr, long long max_hole,
                                                      unsigned char *__restrict__ filled, unsigned long long *info)
{
    const size_t img = (size_t)blockIdx.y * npx;
    unsigned holes = 0, px = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        unsigned char v = mask_on(mask, dtype, img + e) ? 1 : 0;
        if (!v && label) {
            const int r = label[img + e];
            const unsigned a = attr[img + r];
            if (!(a & LB_FRAME) && (max_hole < 0 || (long long)(a & LB_AREA) <= max_hole)) {
                v = 2;
                ++px;
                holes += r == (int)e;
            }
        }
        filled[img + e] = v;
    }
    const unsigned n[2] = {holes, px};
    block_counts(info + blockIdx.y * CI_WORDS + CI_HOLES, n);
}

// ---- 5. select: the action of every pixel from its cell's area and frame bit, the output mask, the counts -------------------
template <typename T>
__global__ __launch_bounds__(256) void cl_select_kernel(const T *__restrict__ mask, const unsigned char *__restrict__ filled,
                                                        const int *__restrict__ label, const unsigned *__restrict__ attr, size_t npx,
                                                        long long min_area, int drop_border, T *__restrict__ out,
                                                        unsigned char *__restrict__ action, unsigned long long *info)
{
    const size_t img = (size_t)blockIdx.y * npx;
    unsigned n[CI_WORDS - CI_SMALL] = {0, 0, 0, 0, 0};
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < npx; e += (size_t)gridDim.x * blockDim.x) {
        const unsigned char f = filled[img + e];
        unsigned char act = 0;
        if (f) {
            const int r = label[img + e];
            const unsigned a = attr[img + r], first = r == (int)e;
            if ((long long)(a & LB_AREA) < min_area) { act = 3; n[CI_SMALL - CI_SMALL] += first; ++n[CI_SMALL_PX - CI_SMALL]; }
            else if (drop_border && (a & LB_FRAME)) { act = 4; n[CI_BORDER - CI_SMALL] += first; ++n[CI_BORDER_PX - CI_SMALL]; }
            else { act = f; n[CI_KEPT - CI_SMALL] += first; }
        }
        out[img + e] = act == 1 ? mask[img + e] : act == 2 ? T(1) : T(0);
        if (action) action[img + e] = act;
    }
    block_counts(info + blockIdx.y * CI_WORDS + CI_SMALL, n);
}

} // namespace unet

using namespace unet;

size_t unet_clean_mask_scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 2 * plane_bytes(B, H, W, sizeof(int)) + plane_bytes(B, H, W, sizeof(unsigned)) + plane_bytes(B, H, W, 1);
}

int unet_clean_mask(const void *mask, int dtype, int B, int H, int W, int connectivity, int fill, long long max_hole_area,
                    long long min_area, int drop_border, void *out, void *action_u8, void *info_i64, void *scratch, void *stream)
{
    ARG_CHECK(mask && out && info_i64 && scratch && B > 0 && H > 0 && W > 0, "unet_clean_mask: bad argument");
    ARG_CHECK(dtype >= 0 && dtype <= 3, "unet_clean_mask: dtype must be 0 (int64), 1 (float32), 2 (int32) or 3 (uint8)");
    ARG_CHECK(connectivity == 4 || connectivity == 8, "unet_clean_mask: connectivity must be 4 or 8");
    ARG_CHECK(max_hole_area >= -1 && min_area >= 0, "unet_clean_mask: max_hole_area must be >= -1 (no limit) and min_area >= 0");
    ARG_CHECK(label_sizes_ok(B, H, W), "unet_clean_mask: image too large");
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)H * W, ib = plane_bytes(B, H, W, sizeof(int));
    char *s = (char *)scratch;
    int *parent = (int *)s, *label = (int *)(s + ib);
    unsigned *attr = (unsigned *)(s + 2 * ib);
    unsigned char *filled = (unsigned char *)(s + 3 * ib);
    unsigned long long *info = (unsigned long long *)info_i64;
    const int conn8 = connectivity == 8;
    const dim3 grid(count_blocks(npx, B), B);
    HIP_TRY(hipMemsetAsync(info, 0, (size_t)B * CI_WORDS * sizeof(unsigned long long), st));
    if (fill) {                                                   // the background takes the dual connectivity
        if (int rc = label_roots(mask, dtype, B, H, W, 0, !conn8, parent, label, attr, nullptr, nullptr, st)) return rc;
    }
    hipLaunchKernelGGL(cl_fill_kernel, grid, dim3(256), 0, st, mask, dtype, npx, fill ? (const int *)label : (const int *)nullptr,
                       (const unsigned *)attr, max_hole_area, filled, info);
    if (int rc = label_roots(filled, 3, B, H, W, 1, conn8, parent, label, attr, nullptr, nullptr, st)) return rc;
    auto select = [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(cl_select_kernel<T>, grid, dim3(256), 0, st, (const T *)mask, (const unsigned char *)filled, (const int *)label,
                           (const unsigned *)attr, npx, min_area, drop_border, (T *)out, (unsigned char *)action_u8, info);
    };
    if (dtype == 0) select((long long)0);
    else if (dtype == 1) select(0.0f);
    else if (dtype == 2) select((int)0);
    else select((unsigned char)0);
    HIP_TRY(hipGetLastError());
    return 0;
}
