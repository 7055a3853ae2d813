// wmap.hip — the U-Net border weight map (Ronneberger et al. 2015, eq. 2; functions.py:7-78), batched, on the device:
//   w = w_c + w0 * exp(-(d1 + d2)^2 / (2 sig2)) on background,  w = 1 on cells,
// d1 / d2 = exact Euclidean distance to the nearest / second-nearest distinct 4-connected foreground component.
//
//   1-3. label_roots (label.hip): label = root (the smallest pixel index of the pixel's component), the component count and the
//        foreground pixel count per image
//   4. wmap_cols   per pixel, along its column within +-R: nearest foreground (dist_a, label_a), nearest label != label_a (dist_b)
//   5. wmap_rows   per pixel, over the column results within +-R in x: d1^2, d2^2, then the weight
//
// Exactness bound: for s = d1 + d2 > R with R = ceil(sqrt(2 sig2 * 104)), expf(-s^2 / (2 sig2)) underflows (e^-104 < 2^-150),
// so a component farther than R from a pixel cannot change that pixel's weight; every component within R is found
// exactly by passes 4-5, whose cost depends on R and not on how many components an image has.
//
// Coherence (label.hip's rule): passes 4-5 read what earlier kernels wrote; every hand-off is a kernel boundary.
#include "elem.hpp"
#include <cmath>
#include "../../include/unet_hip.h"

namespace unet {

static constexpr int WM_ROWS = 256;         // wmap_rows pixels per workgroup
static constexpr unsigned WM_NONE = 0xffffu;

// ---- 4. column pass: nearest foreground (dist_a, label_a) and nearest label != label_a (dist_b) within +-R ------
__global__ __launch_bounds__(256) void wmap_cols_kernel(const int *__restrict__ label, int H, int W, int R,
                                                        int *__restrict__ col_label, unsigned *__restrict__ col_dist)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int *L = label + (size_t)blockIdx.z * H * W + x;
    int la = L[(size_t)y * W];
    unsigned da = la >= 0 ? 0u : WM_NONE, db = WM_NONE;
    for (int k = 1; k <= R && db == WM_NONE; ++k) {
        if (y - k < 0 && y + k >= H) break;
        for (int s = 0; s < 2; ++s) {
            const int yy = s ? y + k : y - k;
            if (yy < 0 || yy >= H) continue;
            const int v = L[(size_t)yy * W];
            if (v < 0) continue;
            if (da == WM_NONE) { la = v; da = k; }
            else if (v != la && db == WM_NONE) db = k;
        }
    }
    const size_t o = ((size_t)blockIdx.z * H + y) * W + x;
    col_label[o] = la;
    col_dist[o] = da | (db << 16);
}

// ---- 5. row pass + weight -----------------------------------------------------------------------------------
// Running (b1, L1, b2) over the columns: b1 = least squared distance seen, L1 its label, b2 = least squared distance
// of a label != L1.  A column is (vA, LA) and vB, the least squared distance of a label != LA; the columns are visited
// by increasing |dx|, and once dx^2 >= b2 no later column can change either distance.
__global__ __launch_bounds__(WM_ROWS) void wmap_rows_kernel(const int *__restrict__ col_label, const unsigned *__restrict__ col_dist,
                                                            int H, int W, int R, int dtype, float w0, float sig2,
                                                            const unsigned long long *__restrict__ counts,
                                                            const int *__restrict__ n_objects, float *__restrict__ w)
{
    extern __shared__ unsigned wm_lds[];
    unsigned *sd = wm_lds;
    int *sl = (int *)(wm_lds + WM_ROWS + 2 * R);
    const int b = blockIdx.z, y = blockIdx.y, x0 = blockIdx.x * WM_ROWS;
    const size_t row = ((size_t)b * H + y) * W;
    for (int i = threadIdx.x; i < WM_ROWS + 2 * R; i += WM_ROWS) {
        const int xx = x0 - R + i;
        const bool in = xx >= 0 && xx < W;
        sd[i] = in ? col_dist[row + xx] : (WM_NONE | (WM_NONE << 16));
        sl[i] = in ? col_label[row + xx] : -1;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
    const int c = threadIdx.x + R;
    if ((sd[c] & 0xffffu) == 0) { w[row + x] = 1.f; return; }          // a cell: w_c = counts[1] / counts[1], w_d = 0

    const int nobj = n_objects[b];
    const unsigned INF = 0xffffffffu;
    unsigned b1 = INF, b2 = INF;
    int L1 = -1;
    for (int dx = 0; dx <= R; ++dx) {
        const unsigned dx2 = (unsigned)(dx * dx);
        if (dx2 >= b2 || (nobj == 1 && dx2 >= b1)) break;
        for (int s = 0; s < (dx ? 2 : 1); ++s) {
            const int j = s ? c + dx : c - dx;
            const unsigned d = sd[j], da = d & 0xffffu, db = d >> 16;
            if (da == WM_NONE) continue;
            const unsigned va = dx2 + da * da, vb = db == WM_NONE ? INF : dx2 + db * db;
            const int la = sl[j];
            if (la == L1) { b1 = min(b1, va); b2 = min(b2, vb); }
            else if (va < b1) { b2 = min(b1, vb); b1 = va; L1 = la; }
            else b2 = min(b2, va);
        }
    }
    const float n1 = (float)counts[b], n0 = (float)((size_t)H * W - counts[b]);
    float wc = n1 / n0;                                      // counts[1] / counts[0] ...
    if (dtype == 0) wc = truncf(wc);                         // ... stored in torch.empty_like(gt): int64 labels truncate
    float wd = 0.f;
    if (b1 != INF && (nobj == 1 || b2 != INF)) {
        const float s = sqrtf((float)b1) + (nobj == 1 ? 0.f : sqrtf((float)b2));
        if (s <= (float)R) wd = w0 * expf(-(s * s) / (2.f * sig2));
    }
    w[row + x] = wc + wd;
}

static int wmap_radius(float sig2)
{
    return (int)std::ceil(std::sqrt(2.0 * (double)sig2 * 104.0));
}

} // namespace unet

using namespace unet;

size_t unet_weighted_map_scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 3 * plane_bytes(B, H, W, sizeof(int));
}

int unet_weighted_map(const void *labels, int labels_dtype, int B, int H, int W, float w0, float sig2, void *weights_f32,
                      void *counts_u64, void *n_objects_i32, void *scratch, void *stream)
{
    ARG_CHECK(labels && weights_f32 && counts_u64 && n_objects_i32 && scratch && B > 0 && H > 0 && W > 0,
              "unet_weighted_map: bad argument");
    ARG_CHECK(labels_dtype == 0 || labels_dtype == 1, "unet_weighted_map: labels_dtype must be 0 (int64) or 1 (float32)");
    ARG_CHECK(label_sizes_ok(B, H, W), "unet_weighted_map: image too large");
    ARG_CHECK(std::isfinite(w0) && std::isfinite(sig2) && sig2 > 0.f, "unet_weighted_map: need finite w0 and sig2 > 0");
    const int R = wmap_radius(sig2);
    ARG_CHECK(R <= 1024, "unet_weighted_map: sig2 %g gives a reach of %d px (at most 1024)", (double)sig2, R);
    hipStream_t st = (hipStream_t)stream;
    char *s = (char *)scratch;
    const size_t plane = plane_bytes(B, H, W, sizeof(int));
    int *parent = (int *)s, *label = (int *)(s + plane);
    unsigned *col_dist = (unsigned *)(s + 2 * plane);
    int *col_label = parent;                                  // the parent words are dead after label_roots
    if (int rc = label_roots(labels, labels_dtype, B, H, W, 1, 0, parent, label, nullptr, (int *)n_objects_i32,
                             (unsigned long long *)counts_u64, st))
        return rc;
    hipLaunchKernelGGL(wmap_cols_kernel, dim3(cdiv(W, 64), cdiv(H, 4), B), dim3(256), 0, st, (const int *)label, H, W, R,
                       col_label, col_dist);
    const size_t lds = (size_t)(WM_ROWS + 2 * R) * 2 * sizeof(unsigned);
    hipLaunchKernelGGL(wmap_rows_kernel, dim3(cdiv(W, WM_ROWS), H, B), dim3(WM_ROWS), lds, st, (const int *)col_label,
                       (const unsigned *)col_dist, H, W, R, labels_dtype, w0, sig2, (const unsigned long long *)counts_u64,
                       (const int *)n_objects_i32, (float *)weights_f32);
    HIP_TRY(hipGetLastError());
    return 0;
}
