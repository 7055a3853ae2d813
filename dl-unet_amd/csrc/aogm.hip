// aogm.hip — the graph stage of the Cell Tracking Challenge's DET and TRA measures (AOGM: Matula et al. 2015; ctc.aogm_counts;
// DESIGN.md section 4s-ter): the vertices, in-edges and edit operations of a result against a reference, both labelled by track,
// from the per-frame areas and majority matches that unet_instance_overlap gives on the two stacks.  No pixel is read here.
//
// Every vertex (t, L) has at most one in-edge (L's previous presence, or the parent track's last presence), and a reference
// vertex at most one match, so the comparison of the two graphs is one independent decision per vertex:
//   1. aogm_spans    one thread per label and side walks t = 0..T-1 over area[t][L] (row-major over L: a wave's loads coalesce):
//                    prev[t][L] = L's latest presence before t (-1: none, or no vertex), last[L] = its last presence; the
//                    same launch clears claims, claimant and counts
//   2. aogm_claims   one thread per reference (t, g) with a match m: claims[t][m] += 1, claimant[t][m] = max(.., g)
//   3. aogm_compare  one wave per 64 consecutive labels of one frame and side: a lane resolves its vertex's in-edge (and, through
//                    the same function, those of its partner and of its edge's other end), decides FN / EA / EC or TP / FP / NS /
//                    ED, writes the in-edge and the flag byte, and the wave adds its share of the twelve counters to counts[t]
// Every count is an integer sum and the claimant an integer max: the outputs do not depend on the order of the atomics.
//
// Coherence (ov_table.hpp's rule): inside aogm_claims a word of claims or claimant, and inside aogm_compare a word of counts, is
// touched only by agent-scope integer atomics (aogm_spans, an earlier kernel, stored their zeros); everything read plainly was
// written by an earlier kernel of the stream.
#include "elem.hpp"
#include "../../include/unet_hip.h"

namespace unet {

enum : unsigned { AOGM_PRESENT = 1, AOGM_EDGE = 2, AOGM_PARENT = 4, AOGM_BAD = 8, AOGM_MATCHED = 16, AOGM_EA = 32, AOGM_EC = 64,
                  AOGM_TP = 16, AOGM_FP = 32, AOGM_ED = 64 };
enum { N_REF, N_RES, E_REF, E_RES, C_TP, C_FN, C_FP, C_NS, C_EA, C_ED, C_EC, C_BAD, AOGM_COUNTS };

// one side's graph as the kernels read it: rows may be null (no table)
struct AogmSide { const unsigned *area; const int *rows; int *prev, *last; int n_max; };

__device__ __forceinline__ size_t aogm_at(const AogmSide &s, int t, int L) { return (size_t)t * ((size_t)s.n_max + 1) + L; }

// It also clears what the next two kernels add to: claims and claimant [T][nr_max+1], counts [T][12]
__global__ __launch_bounds__(256) void aogm_spans_kernel(const AogmSide gt, const AogmSide res, int T, unsigned *__restrict__ claims,
                                                         int *__restrict__ claimant, unsigned long long *__restrict__ counts)
{
    const size_t ng1 = (size_t)gt.n_max + 1, n = ng1 + res.n_max + 1, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x, n_claims = (size_t)T * ((size_t)res.n_max + 1);
    for (size_t i = first; i < n_claims; i += stride) { claims[i] = 0; claimant[i] = 0; }
    for (size_t i = first; i < (size_t)T * AOGM_COUNTS; i += stride) counts[i] = 0;
    for (size_t i = first; i < n; i += stride) {
        const AogmSide &s = i < ng1 ? gt : res;
        const int L = (int)(i < ng1 ? i : i - ng1);
        int seen = -1;
        for (int t = 0; t < T; ++t) {
            const size_t o = aogm_at(s, t, L);
            const bool on = L > 0 && s.area[o] != 0;
            s.prev[o] = on ? seen : -1;
            if (on) seen = t;
        }
        s.last[L] = seen;
    }
}

__global__ __launch_bounds__(256) void aogm_claims_kernel(const unsigned *__restrict__ area_gt, const int *__restrict__ match, size_t n,
                                                          int ng_max, int nr_max, unsigned *claims, int *claimant)
{
    const size_t ng1 = (size_t)ng_max + 1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t t = i / ng1;
        const int g = (int)(i - t * ng1), m = match[i];
        if (g == 0 || area_gt[i] == 0 || m < 1 || m > nr_max) continue;
        const size_t o = t * ((size_t)nr_max + 1) + m;
        __hip_atomic_fetch_add(&claims[o], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&claimant[o], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the in-edge of the vertex (t, L) of side s, which the caller knows to be present: its source (frame, label), or (-1, 0),
// and the vertex's flags PRESENT, EDGE, PARENT, BAD
struct AogmEdge { int t, L; unsigned flags; };

__device__ __forceinline__ AogmEdge aogm_inedge(const AogmSide &s, int t, int L)
{
    AogmEdge e{-1, 0, AOGM_PRESENT};
    int P = 0;
    if (s.rows) {
        const int B = s.rows[3 * (size_t)L], E = s.rows[3 * (size_t)L + 1];
        if (B < 0 || t < B || t > E) e.flags |= AOGM_BAD;
        if (B >= 0) P = s.rows[3 * (size_t)L + 2];
    }
    const int before = s.prev[aogm_at(s, t, L)];
    if (before >= 0) { e.t = before; e.L = L; e.flags |= AOGM_EDGE; }
    else if (P > 0) {
        const int end = P <= s.n_max ? s.last[P] : -1;
        if (end >= 0 && end < t) { e.t = end; e.L = P; e.flags |= AOGM_EDGE | AOGM_PARENT; }
        else e.flags |= AOGM_BAD;
    }
    return e;
}

// the result label that matches the reference vertex (t, g) and is TP, else 0
__device__ __forceinline__ int aogm_tp_match(const int *match, const unsigned *claims, int t, int g, int ng_max, int nr_max)
{
    const int m = match[(size_t)t * ((size_t)ng_max + 1) + g];
    return m >= 1 && m <= nr_max && claims[(size_t)t * ((size_t)nr_max + 1) + m] == 1 ? m : 0;
}

__device__ __forceinline__ unsigned wave_count(bool v) { return (unsigned)__popcll(__ballot(v)); }

// A wave's task: 64 consecutive labels of one frame of one side (tasks [0, T * cg) the reference's, cg = chunks of 64 per frame,
// then T * cr the result's), so that frame and side are wave-uniform and one add per counter serves the wave.
__global__ __launch_bounds__(256) void aogm_compare_kernel(const AogmSide gt, const AogmSide res, const int *__restrict__ match,
                                                           const unsigned *__restrict__ claims, const int *__restrict__ claimant, int T,
                                                           int *__restrict__ inedge_gt, int *__restrict__ inedge_res,
                                                           unsigned char *__restrict__ flags_gt, unsigned char *__restrict__ flags_res,
                                                           unsigned long long *counts)
{
    const int lane = threadIdx.x & 63;
    const size_t cg = ((size_t)gt.n_max + 64) / 64, cr = ((size_t)res.n_max + 64) / 64, ref_tasks = (size_t)T * cg;
    const size_t tasks = ref_tasks + (size_t)T * cr, waves = (size_t)gridDim.x * (blockDim.x / 64);
    for (size_t task = (size_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); task < tasks; task += waves) {   // wave-uniform
        const bool is_ref = task < ref_tasks;
        const AogmSide s = is_ref ? gt : res;
        const size_t k = is_ref ? task : task - ref_tasks, per = is_ref ? cg : cr;
        const int t = (int)(k / per);
        const long long Lw = (long long)(k - (size_t)t * per) * 64 + lane;
        const bool in = Lw <= s.n_max;
        const int L = in ? (int)Lw : 0;
        const size_t o = aogm_at(s, t, L);
        const bool on = in && L > 0 && s.area[o] != 0;
        AogmEdge e{-1, 0, 0};
        unsigned ns = 0;
        if (on) {
            e = aogm_inedge(s, t, L);
            const bool edge = e.flags & AOGM_EDGE;
            if (is_ref) {
                const int m = match[o];
                if (m >= 1 && m <= res.n_max) e.flags |= AOGM_MATCHED;
                if (edge) {
                    // reproduced: both ends matched by TP result vertices, and the head's in-edge comes from the tail's
                    const int sv = aogm_tp_match(match, claims, t, L, gt.n_max, res.n_max);
                    const int ru = aogm_tp_match(match, claims, e.t, e.L, gt.n_max, res.n_max);
                    bool same = false, parent = false;
                    if (sv && ru && res.area[aogm_at(res, t, sv)] != 0) {
                        const AogmEdge r = aogm_inedge(res, t, sv);
                        same = (r.flags & AOGM_EDGE) && r.t == e.t && r.L == ru;
                        parent = r.flags & AOGM_PARENT;
                    }
                    if (!same) e.flags |= AOGM_EA;
                    else if (parent != (bool)(e.flags & AOGM_PARENT)) e.flags |= AOGM_EC;
                }
            } else {
                const unsigned c = claims[o];
                if (c == 1) e.flags |= AOGM_TP;
                if (c == 0) e.flags |= AOGM_FP;
                if (c > 1) ns = c - 1;
                if (edge && c == 1 && claims[aogm_at(res, e.t, e.L)] == 1) {
                    // both ends TP: the partners are the claimants, both present reference vertices in [1, ng_max]
                    const int v = claimant[o], u = claimant[aogm_at(res, e.t, e.L)];
                    const AogmEdge g = aogm_inedge(gt, t, v);
                    if (!((g.flags & AOGM_EDGE) && g.t == e.t && g.L == u)) e.flags |= AOGM_ED;
                }
            }
        }
        if (in) {
            int *ie = is_ref ? inedge_gt : inedge_res;
            ie[2 * o] = e.t; ie[2 * o + 1] = e.L;
            (is_ref ? flags_gt : flags_res)[o] = (unsigned char)e.flags;
        }
        // the wave's sums (the flag bits 16, 32, 64 mean MATCHED, EA, EC on one side and TP, FP, ED on the other); lane c adds
        // the sum of counter c
        const unsigned n_on = wave_count(on), n_edge = wave_count(e.flags & AOGM_EDGE), n_bad = wave_count(e.flags & AOGM_BAD);
        const unsigned n16 = wave_count(e.flags & 16), n32 = wave_count(e.flags & 32), n64 = wave_count(e.flags & 64);
        unsigned mine = lane == C_BAD ? n_bad : 0;
        if (is_ref)
            mine = lane == N_REF ? n_on : lane == E_REF ? n_edge : lane == C_FN ? n_on - n16 : lane == C_EA ? n32 : lane == C_EC ? n64 : mine;
        else {
            const unsigned n_ns = wave_sum(ns);
            mine = lane == N_RES ? n_on : lane == E_RES ? n_edge : lane == C_TP ? n16 : lane == C_FP ? n32 : lane == C_ED ? n64 :
                   lane == C_NS ? n_ns : mine;
        }
        if (lane < AOGM_COUNTS && mine)
            __hip_atomic_fetch_add(&counts[(size_t)t * AOGM_COUNTS + lane], (unsigned long long)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

} // namespace unet

using namespace unet;

static bool aogm_sizes_ok(int T, int ng_max, int nr_max)
{
    return T > 0 && T <= 65535 && ng_max >= 0 && ng_max <= ID_MAX && nr_max >= 0 && nr_max <= ID_MAX;
}
static size_t aogm_words(int T, int n_max) { return align_up((size_t)T * ((size_t)n_max + 1) * sizeof(int), 256); }
static size_t aogm_last(int n_max) { return align_up(((size_t)n_max + 1) * sizeof(int), 256); }

size_t unet_aogm_counts_scratch_bytes(int T, int ng_max, int nr_max)
{
    if (!aogm_sizes_ok(T, ng_max, nr_max)) return 0;
    return aogm_words(T, ng_max) + aogm_words(T, nr_max) + aogm_last(ng_max) + aogm_last(nr_max);
}

int unet_aogm_counts(const void *area_gt_u32, const void *area_res_u32, const void *match_i32, const void *rows_gt_i32,
                     const void *rows_res_i32, int T, int ng_max, int nr_max, void *claims_u32, void *claimant_i32, void *inedge_gt_i32,
                     void *inedge_res_i32, void *flags_gt_u8, void *flags_res_u8, void *counts_u64, void *scratch, void *stream)
{
    ARG_CHECK(area_gt_u32 && area_res_u32 && match_i32 && claims_u32 && claimant_i32 && inedge_gt_i32 && inedge_res_i32 && flags_gt_u8 &&
              flags_res_u8 && counts_u64 && scratch, "unet_aogm_counts: bad argument");
    ARG_CHECK(aogm_sizes_ok(T, ng_max, nr_max), "unet_aogm_counts: T must be in [1, 65535], ng_max and nr_max in [0, %d]", ID_MAX);
    hipStream_t st = (hipStream_t)stream;
    char *p = (char *)scratch;
    AogmSide gt{(const unsigned *)area_gt_u32, (const int *)rows_gt_i32, (int *)p, nullptr, ng_max};
    p += aogm_words(T, ng_max);
    AogmSide res{(const unsigned *)area_res_u32, (const int *)rows_res_i32, (int *)p, nullptr, nr_max};
    p += aogm_words(T, nr_max);
    gt.last = (int *)p;
    res.last = (int *)(p + aogm_last(ng_max));
    const size_t ng1 = (size_t)ng_max + 1, nr1 = (size_t)nr_max + 1;
    const size_t span_work = ng1 + nr1 > T * nr1 ? ng1 + nr1 : T * nr1;
    hipLaunchKernelGGL(aogm_spans_kernel, dim3(grid_for(span_work, 256, 2048)), dim3(256), 0, st, gt, res, T, (unsigned *)claims_u32,
                       (int *)claimant_i32, (unsigned long long *)counts_u64);
    hipLaunchKernelGGL(aogm_claims_kernel, dim3(grid_for(T * ng1, 256, 2048)), dim3(256), 0, st, gt.area, (const int *)match_i32, T * ng1,
                       ng_max, nr_max, (unsigned *)claims_u32, (int *)claimant_i32);
    const size_t tasks = (size_t)T * ((ng1 + 63) / 64 + (nr1 + 63) / 64);
    hipLaunchKernelGGL(aogm_compare_kernel, dim3(grid_for(tasks * 64, 256, 2048)), dim3(256), 0, st, gt, res, (const int *)match_i32,
                       (const unsigned *)claims_u32, (const int *)claimant_i32, T, (int *)inedge_gt_i32, (int *)inedge_res_i32,
                       (unsigned char *)flags_gt_u8, (unsigned char *)flags_res_u8, (unsigned long long *)counts_u64);
    HIP_TRY(hipGetLastError());
    return 0;
}
