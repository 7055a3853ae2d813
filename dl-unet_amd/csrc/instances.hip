// instances.hip — the per-cell overlaps of two instance maps (label.hip makes such maps from a mask) that the Cell Tracking
// Challenge SEG measure needs (Ronneberger et al. 2015, Table 2), and their contingency table, batched, on the device.
//
// unet_instance_overlap: two id maps -> per-id areas, and for every ground-truth id the one predicted id that covers more than
// half of it, with the size of that overlap:
//   1. overlap_fill   ov_table.hpp's pair fill on (gt, pred): the first lane of a run of equal pairs adds the run's length to both
//                     area histograms and, for gt, pred >= 1, to the counter of the key (b, gt, pred) in the pair table
//   2. overlap_match  one thread per table slot: 2 * count > area_gt[g] -> match[g] = p, inter[g] = count (at most one p per g)
// Every count is an integer sum: the outputs do not depend on the order of the atomics.  Which slot a key lands in does, and
// nothing reads that.
//
// unet_partition_pairs: the contingency table of two id maps restricted to ground-truth foreground, which the Rand and information
// scores of the ISBI 2012 challenge (Ronneberger et al. 2015, Table 1) are sums over:
//   1. overlap_fill<FG>  the same pair fill and table, for every pixel with gt >= 1 and any pred >= 0; no histograms
//   2. pairs_compact     a wave reads 64 slots, one agent-scope add on n_pairs gives it a block of the dense (key, count) list
// The list's order depends on the order of those adds; its content does not.
//
// unet_cell_contacts: the same table and compaction for one id map against itself, shifted: for every pair of ids i < j the unit
// pixel sides at which they are 4-adjacent (functions.cell_neighbours):
//   1. contact_fill      every pixel looks right (one insert per side) and down (one insert per run of equal (id, id below) pairs)
//   2. pairs_compact     as above
//
// Coherence: ov_table.hpp's rule for overlap_fill and contact_fill; n_pairs in pairs_compact is likewise touched by agent-scope
// adds only; overlap_match and pairs_compact read what an earlier kernel wrote.
#include "ov_table.hpp"
#include "../../include/unet_hip.h"

namespace unet {

// ---- overlaps ---------------------------------------------------------------------------------------------------------
// overlap_fill = pair_fill_kernel (ov_table.hpp) on image b of gt and pred, key (b, g, p).  FG = false: unet_instance_overlap
// (both area histograms, pairs with g, p >= 1).  FG = true: unet_partition_pairs (no histogram, pairs with g >= 1 and any p >= 0:
// the table restricted to ground-truth foreground, "predicted background" being the column 0)
template <bool FG>
struct OverlapFill {
    const int *gt, *pred; size_t npx; int ng_max, np_max; OvTable tab; unsigned *area_gt, *area_pred; unsigned long long *status;
    static constexpr bool J_MAY_BE_NULL = false, AREA_I = !FG, AREA_J = !FG, KEEP_J0 = FG;
    __device__ unsigned long long key(unsigned long long b, int g, int p) const { return ov_key(b, g, p); }
    __device__ PairMaps maps(int b) const
    {
        return {gt + (size_t)b * npx, pred + (size_t)b * npx, ng_max, np_max, FG ? nullptr : area_gt + (size_t)b * (ng_max + 1),
                FG ? nullptr : area_pred + (size_t)b * (np_max + 1)};
    }
};

__global__ __launch_bounds__(256) void overlap_match_kernel(const unsigned long long *__restrict__ keys, const unsigned *__restrict__ cnt,
                                                            size_t slots, int ng_max, const unsigned *__restrict__ area_gt,
                                                            int *__restrict__ match, unsigned *__restrict__ inter)
{
    for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[s];
        if (key == OV_EMPTY) continue;
        const size_t b = ov_key_b(key);
        const int g = ov_key_i(key), p = ov_key_j(key);
        const size_t o = b * (ng_max + 1) + g;
        const unsigned c = cnt[s];
        if (2ull * c > area_gt[o]) { match[o] = p; inter[o] = c; }      // strict: no two p can both hold more than half of g
    }
}

// the occupied slots, densely: a wave reads 64 consecutive slots and its first occupied lane takes the wave's block of output
// indices with one agent-scope add on n_pairs; which block a wave gets depends on the order of those adds, so the list's order is
// unspecified (the caller sorts it).  At most `slots` slots are occupied: every index is inside the [slots] outputs.
__global__ __launch_bounds__(256) void pairs_compact_kernel(const unsigned long long *__restrict__ keys, const unsigned *__restrict__ cnt,
                                                            size_t slots, unsigned long long *__restrict__ pair_keys,
                                                            unsigned *__restrict__ pair_counts, unsigned long long *n_pairs)
{
    const int lane = threadIdx.x & 63;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t base = (size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < slots; base += stride) {   // wave-uniform
        const size_t s = base + lane;
        const unsigned long long key = s < slots ? keys[s] : OV_EMPTY;
        const unsigned long long occupied = __ballot(key != OV_EMPTY);
        if (!occupied) continue;
        const int leader = __ffsll(occupied) - 1;
        unsigned long long first = 0;
        if (lane == leader) first = __hip_atomic_fetch_add(n_pairs, (unsigned long long)__popcll(occupied), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        first = __shfl(first, leader, 64);
        if (key != OV_EMPTY) {
            const size_t o = first + __popcll(occupied & ((1ull << lane) - 1));
            pair_keys[o] = key;
            pair_counts[o] = cnt[s];
        }
    }
}

// ---- contacts ---------------------------------------------------------------------------------------------------------
// unet_cell_contacts: for every unordered pair of ids 1 <= i < j of image b = blockIdx.y, the unit pixel sides at which a pixel of
// i is 4-adjacent to a pixel of j.  Every pixel looks right and down, so each side is counted once.  A side to the right is one
// insert; the sides below are merged per run of equal (id, id below) pairs along a row with one ballot, as overlap_fill merges
// its pairs.  A pixel with an id outside [0, n_max] is counted in status[b][0] and is nobody's neighbour.
template <typename LT>
__global__ __launch_bounds__(256) void contact_fill_kernel(const LT *__restrict__ labels, int H, int W, int n_max, const OvTable tab,
                                                           unsigned long long *status)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const size_t npx = (size_t)H * W;
    const LT *M = labels + (size_t)b * npx;
    auto id_at = [&](size_t e) { const LT v = M[e]; return (v < 0 || v > (LT)n_max) ? -1 : (int)v; };
    auto key_of = [&](int i, int j) { return ov_key(b, min(i, j), max(i, j)); };
    unsigned long long bad = 0, dropped = 0;                      // this lane's share of status[b][0..1]
    bool full = false;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t base = (size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < npx; base += stride) {   // wave-uniform
        const size_t e = base + lane;
        const bool in = e < npx;
        const int y = in ? (int)(e / W) : 0, x = in ? (int)(e - (size_t)y * W) : 0;
        const int a = in ? id_at(e) : -2;
        const int right = in && x + 1 < W ? id_at(e + 1) : 0;
        int down = in && y + 1 < H ? id_at(e + W) : 0;
        bad += a == -1;
        if (a < 1 || down < 1 || down == a) down = 0;             // no contact below: such pixels form runs too, and add nothing
        const int al = __shfl_up(a, 1, 64), dl = __shfl_up(down, 1, 64);
        const bool head = lane == 0 || a != al || down != dl || x == 0;
        const unsigned n = wave_run_length(head, lane);
        OV_ADD_IF(a >= 1 && right >= 1 && right != a, tab, key_of(a, right), 1u, full, dropped);
        OV_ADD_IF(head && down, tab, key_of(a, down), n, full, dropped);
        full = __any(full);
    }
    ov_flush(status, b, lane, bad, dropped);
}

} // namespace unet

using namespace unet;

// what unet_instance_overlap (FG = false) and unet_partition_pairs (FG = true) share: the checks, the open table, the clears of
// the histograms overlap_fill adds to (FG: there are none, area_gt and area_pred are null) and its launch
template <bool FG>
static int ov_fill(const char *who, const void *gt_i32, const void *pred_i32, int B, int H, int W, int ng_max, int np_max,
                   size_t table_slots, void *area_gt_u32, void *area_pred_u32, void *status_u64, void *scratch, hipStream_t st, OvTable &t)
{
    ARG_CHECK(gt_i32 && pred_i32 && status_u64 && scratch && B > 0 && H > 0 && W > 0, "%s: bad argument", who);
    ARG_CHECK((size_t)H * W < (1u << 31) && B <= 65535, "%s: image too large", who);
    ARG_CHECK(ng_max >= 0 && np_max >= 0 && ng_max <= ID_MAX && np_max <= ID_MAX, "%s: ng_max and np_max must be in [0, %d]", who, ID_MAX);
    if (int rc = ov_open(who, scratch, table_slots, status_u64, B, st, t)) return rc;
    const size_t npx = (size_t)H * W;
    if (!FG) {
        HIP_TRY(hipMemsetAsync(area_gt_u32, 0, B * ((size_t)ng_max + 1) * sizeof(unsigned), st));
        HIP_TRY(hipMemsetAsync(area_pred_u32, 0, B * ((size_t)np_max + 1) * sizeof(unsigned), st));
    }
    const OverlapFill<FG> src{(const int *)gt_i32, (const int *)pred_i32, npx, ng_max, np_max, t, (unsigned *)area_gt_u32,
                              (unsigned *)area_pred_u32, (unsigned long long *)status_u64};
    hipLaunchKernelGGL(pair_fill_kernel<OverlapFill<FG>>, dim3(grid_for(npx, 256, 2048), B), dim3(256), 0, st, src);
    return 0;
}

size_t unet_instance_overlap_scratch_bytes(int B, int ng_max, int np_max, size_t table_slots)
{
    if (B <= 0 || ng_max < 0 || np_max < 0 || table_slots == 0) return 0;
    return ov_scratch_bytes(table_slots);
}

int unet_instance_overlap(const void *gt_i32, const void *pred_i32, int B, int H, int W, int ng_max, int np_max, size_t table_slots,
                          void *area_gt_u32, void *area_pred_u32, void *match_i32, void *inter_u32, void *status_u64, void *scratch,
                          void *stream)
{
    ARG_CHECK(area_gt_u32 && area_pred_u32 && match_i32 && inter_u32, "unet_instance_overlap: bad argument");
    hipStream_t st = (hipStream_t)stream;
    OvTable t;
    if (int rc = ov_fill<false>("unet_instance_overlap", gt_i32, pred_i32, B, H, W, ng_max, np_max, table_slots, area_gt_u32,
                                area_pred_u32, status_u64, scratch, st, t))
        return rc;
    const size_t ng1 = (size_t)ng_max + 1;
    HIP_TRY(hipMemsetAsync(match_i32, 0, B * ng1 * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(inter_u32, 0, B * ng1 * sizeof(unsigned), st));
    hipLaunchKernelGGL(overlap_match_kernel, dim3(grid_for(table_slots, 256, 2048)), dim3(256), 0, st,
                       (const unsigned long long *)t.keys, (const unsigned *)t.cnt, table_slots, ng_max, (const unsigned *)area_gt_u32,
                       (int *)match_i32, (unsigned *)inter_u32);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t unet_partition_pairs_scratch_bytes(int B, size_t table_slots)
{
    if (B <= 0 || table_slots == 0) return 0;
    return ov_scratch_bytes(table_slots);
}

int unet_partition_pairs(const void *gt_i32, const void *pred_i32, int B, int H, int W, int ng_max, int np_max, size_t table_slots,
                         void *pair_keys_u64, void *pair_counts_u32, void *n_pairs_u64, void *status_u64, void *scratch, void *stream)
{
    ARG_CHECK(pair_keys_u64 && pair_counts_u32 && n_pairs_u64, "unet_partition_pairs: bad argument");
    hipStream_t st = (hipStream_t)stream;
    OvTable t;
    if (int rc = ov_fill<true>("unet_partition_pairs", gt_i32, pred_i32, B, H, W, ng_max, np_max, table_slots, nullptr, nullptr,
                               status_u64, scratch, st, t))
        return rc;
    HIP_TRY(hipMemsetAsync(n_pairs_u64, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(pairs_compact_kernel, dim3(grid_for(table_slots, 256, 2048)), dim3(256), 0, st,
                       (const unsigned long long *)t.keys, (const unsigned *)t.cnt, table_slots, (unsigned long long *)pair_keys_u64,
                       (unsigned *)pair_counts_u32, (unsigned long long *)n_pairs_u64);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t unet_cell_contacts_scratch_bytes(int B, size_t table_slots)
{
    if (B <= 0 || table_slots == 0) return 0;
    return ov_scratch_bytes(table_slots);
}

int unet_cell_contacts(const void *labels, int label_dtype, int B, int H, int W, int n_max, size_t table_slots, void *pair_keys_u64,
                       void *pair_counts_u32, void *n_pairs_u64, void *status_u64, void *scratch, void *stream)
{
    ARG_CHECK(labels && pair_keys_u64 && pair_counts_u32 && n_pairs_u64 && status_u64 && scratch && B > 0 && H > 0 && W > 0,
              "unet_cell_contacts: bad argument");
    ARG_CHECK(label_dtype == 0 || label_dtype == 2, "unet_cell_contacts: label dtype must be 0 (int64) or 2 (int32)");
    ARG_CHECK(measure_sizes_ok(B, H, W, n_max), "unet_cell_contacts: H, W must be <= 32768, B <= 65535 and n_max in [0, 2^24)");
    hipStream_t st = (hipStream_t)stream;
    OvTable t;
    if (int rc = ov_open("unet_cell_contacts", scratch, table_slots, status_u64, B, st, t)) return rc;
    HIP_TRY(hipMemsetAsync(n_pairs_u64, 0, sizeof(unsigned long long), st));
    const dim3 grid(grid_for((size_t)H * W, 256, 2048), B);
    if (label_dtype == 0)
        hipLaunchKernelGGL(contact_fill_kernel<long long>, grid, dim3(256), 0, st, (const long long *)labels, H, W, n_max, t,
                           (unsigned long long *)status_u64);
    else
        hipLaunchKernelGGL(contact_fill_kernel<int>, grid, dim3(256), 0, st, (const int *)labels, H, W, n_max, t,
                           (unsigned long long *)status_u64);
    hipLaunchKernelGGL(pairs_compact_kernel, dim3(grid_for(table_slots, 256, 2048)), dim3(256), 0, st, (const unsigned long long *)t.keys,
                       (const unsigned *)t.cnt, table_slots, (unsigned long long *)pair_keys_u64, (unsigned *)pair_counts_u32,
                       (unsigned long long *)n_pairs_u64);
    HIP_TRY(hipGetLastError());
    return 0;
}
