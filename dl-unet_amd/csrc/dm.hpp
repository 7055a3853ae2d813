// dm.hpp — the two passes of the exact squared Euclidean distance to the nearest "site" pixel of a plane, which shape.hip (the
// distance map of a region: the sites are the pixels outside it) and boundary.hip (the distance to a contour: the sites are the
// contour's pixels) instantiate from this one copy.  What a site is, is the template parameter of the column pass: a functor
// `bool site(size_t e)` over the element offsets of the [B,H,W] plane.
//   1. dm_cols   a downward and an upward sweep leave g, the row distance to the nearest site of the column (DM_FAR when the
//                column has none; with edge 1 the pixels above row 0 and below row H - 1 count as sites).  A sweep is a chain of H
//                dependent steps, so a column is cut into four segments, one wave each: every thread first finds the first and
//                last site row of its segment (independent loads), the segments swap them through LDS, and each sweeps its rows
//                from the distance its neighbours hand it
//   2. dm_row_best   for one pixel: min over x' of g(x')^2 + (x - x')^2, by a scan outwards from x' = x that ends once dx^2
//                reaches the running minimum (every column further out offers at least dx^2), so a pixel at distance d looks at
//                about 2 d columns.  The caller gives the start of the minimum (g(x)^2, less with edge 1) and decides which
//                pixels scan at all
#pragma once
#include "elem.hpp"

namespace unet {

static constexpr int DM_EDGE = 32767;                          // H, W <= DM_EDGE: H^2 + W^2 < 2^31
static constexpr int DM_FAR = 46340;                           // "no site in this column": DM_FAR^2 is above every H^2 + W^2 and
                                                               // DM_FAR^2 + dx^2 < 2^32
static constexpr unsigned DM_FAR2 = (unsigned)DM_FAR * DM_FAR;
static constexpr int DM_SEGS = 4;                              // row segments of a column, one wave each, in dm_cols

template <typename Site>
__global__ __launch_bounds__(256) void dm_cols_kernel(const Site site, int H, int W, int edge, int *__restrict__ g)
{
    __shared__ int first[DM_SEGS][64], last[DM_SEGS][64];      // per segment and column: its first and last site row
    const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane;
    const bool live = x < W;
    const int rows = (H + DM_SEGS - 1) / DM_SEGS, y0 = min(seg * rows, H), y1 = min(y0 + rows, H);
    const size_t o = (size_t)blockIdx.y * H * W + (live ? x : 0);
    int *G = g + o;
    int lo = -1, hi = -1;
    if (live) {
#pragma unroll 8
        for (int y = y0; y < y1; ++y) {                        // no value depends on the one before: the loads overlap
            const bool out = site(o + (size_t)y * W);
            lo = out && lo < 0 ? y : lo;
            hi = out ? y : hi;
        }
    }
    first[seg][lane] = lo;
    last[seg][lane] = hi;
    __syncthreads();
    if (!live) return;
    int d = edge ? y0 : DM_FAR;                                // the distance in row y0 - 1: edge 1 has a site in row -1
    for (int s = seg - 1; s >= 0; --s)
        if (last[s][lane] >= 0) { d = y0 - 1 - last[s][lane]; break; }
#pragma unroll 8
    for (int y = y0; y < y1; ++y) {                            // downward: the nearest site at or above y
        d = site(o + (size_t)y * W) ? 0 : d >= DM_FAR ? DM_FAR : d + 1;
        G[(size_t)y * W] = d;
    }
    d = edge ? H - y1 : DM_FAR;                                // the distance in row y1: edge 1 has a site in row H
    for (int s = seg + 1; s < DM_SEGS; ++s)
        if (first[s][lane] >= 0) { d = first[s][lane] - y1; break; }
#pragma unroll 8
    for (int y = y1 - 1; y >= y0; --y) {                       // upward: the nearest at or below y, merged with the word above
        const int dn = G[(size_t)y * W];                       // this thread's own store
        d = dn == 0 ? 0 : d >= DM_FAR ? DM_FAR : d + 1;
        G[(size_t)y * W] = min(dn, d);
    }
}

// G: the row of g that holds column x, best: the minimum so far (at most G[x]^2).  At least DM_FAR2 if the plane has no site
__device__ __forceinline__ unsigned dm_row_best(const int *__restrict__ G, int x, int W, unsigned best)
{
    for (int dx = 1; ; ++dx) {
        const unsigned dd = (unsigned)dx * dx;
        const int l = x - dx, r = x + dx;
        if (dd >= best || (l < 0 && r >= W)) break;            // every column further out offers at least dd
        if (l >= 0) { const unsigned v = (unsigned)G[l]; best = min(best, v * v + dd); }
        if (r < W) { const unsigned v = (unsigned)G[r]; best = min(best, v * v + dd); }
    }
    return best;
}

}  // namespace unet
