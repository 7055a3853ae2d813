// kernel_parts.hpp — the device-side vocabulary of the MFMA kernels (igemm, igemmx, igemmb, wino, wgrad, wgradw), stated once:
// tile order, pixel decomposition, destination rows, LDS-DMA and the pinned kernel arguments.  All of it inlines; a change
// here is checked by comparing the kernels' code before and after (tools/isa_diff.py).
#pragma once
#include "common.hpp"

namespace unet {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// XCD-aware tile order: the logical slot of this workgroup.  The hardware deals blocks round-robin to the 8 XCDs, so blocks b
// and b+8 share an XCD (and its L2); every XCD gets a contiguous run of slots, and a kernel that makes the tiles which
// re-read each other's operands neighbours in slot order keeps that reuse inside one L2.
__device__ __forceinline__ int xcd_slot()
{
    const int nblk = gridDim.x, q = nblk >> 3, r = nblk & 7, xcd = blockIdx.x & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (blockIdx.x >> 3);
}

__device__ __forceinline__ int fdiv(int n, const FastDiv &f) { return (int)(((unsigned long long)(unsigned)n * f.mul) >> f.shift); }

// pixel index m of the output domain [NB, OH, OW] -> (image, row, column); P: IgemmP or its pinned copy IgEp, ohw = OH * OW
// (the caller's: once per tile, in front of its row loop)
template <class P>
__device__ __forceinline__ void pixel_of(const P &p, int ohw, int m, int &img, int &oy, int &ox)
{
    img = fdiv(m, p.d_ohw);
    const int rem = m - img * ohw;
    oy = fdiv(rem, p.d_ow);
    ox = rem - oy * p.OW;
}

// element offset in dst of row i of the tile that starts at output pixel m0 (IgemmP::scatter 0 / 1 / 2); flag: the pixel lies
// inside the deferred-ReLU window.  Rows past M get row M - 1's (valid) offset, so that loads through it can be unconditional.
// The statement order is the row tables' own and the kernels' code depends on it (tools/isa_diff.py): the bf16 row table
// (igemmb.hip), which also flags the rows past M, compiles to other code through this function and keeps its own copy.
template <class P>
__device__ __forceinline__ unsigned dst_row(const P &p, int m0, int i, unsigned char &flag)
{
    const bool relu_win = p.rw1 > p.rw0;
    int m = m0 + i;
    m = m < p.M ? m : p.M - 1;
    unsigned off;
    flag = 0;
    if (!p.scatter && !relu_win) {
        off = (unsigned)m * (unsigned)p.DC;
    } else {
        int img, oy, ox;
        pixel_of(p, p.OH * p.OW, m, img, oy, ox);
        if (p.scatter == 1) off = (unsigned)((img * p.DH + 2 * oy) * p.DW + 2 * ox) * (unsigned)p.DC;
        else if (p.scatter == 2) off = (unsigned)((img * p.DH + oy + p.dwy0) * p.DW + ox + p.dwx0) * (unsigned)p.DC;
        else off = (unsigned)m * (unsigned)p.DC;
        flag = relu_win && oy >= p.rw0 && oy < p.rw1 && ox >= p.rw0 && ox < p.rw1;
    }
    return off;
}

// ---- LDS-DMA, 16 bytes per lane: global pointer form ...
#define GLDS16(gptr, lptr)                                                                    \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gptr),  \
                                     (__attribute__((address_space(3))) void *)(lptr), 16, 0, 0)

// ... and buffer-descriptor form (buffer_load_dwordx4 ... offen lds): 32-bit byte offsets, a per-lane vector offset plus a
// uniform scalar offset; the range check sees only the vector part and returns zeros beyond num_records, which is how taps in
// the zero padding are staged (LDS_DMA_OOB).  Needs the tensor below 2 GiB (fits_buffer, common.hpp).
// The builtin must stay inside this plain __device__ function: used directly in a lambda nested in a kernel template, the host
// pass drops the kernel's stub without a diagnostic.
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t r, unsigned char *lds, int voff, int soff)
{
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void *)lds, 16, voff, soff, 0, 0);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *ptr, int bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)ptr, 0, bytes, 0x00020000);      // raw buffer, 32-bit data format
}
constexpr int LDS_DMA_OOB = (int)0x80000000;      // a vector offset beyond any num_records

// ---- kernel arguments pinned in SGPRs.
// The epilogue's (and the K loop's) kernel arguments are copied into locals up front and pinned in SGPRs (IGB_PIN): fetched where
// they are used, every one of them is a scalar-load round trip behind the branch that needs it — dozens in a row per workgroup,
// some of them once per K step (found with in-kernel stamps on the fp32 Winograd kernel).
#define IGB_PIN(x) asm volatile("" : "+s"(x))
struct IgEp {
    int rw0, rw1, scatter, DC, OH, OW, DH, DW, dwy0, dwx0, M, cout, Nn, dn0, relu;
    FastDiv d_ohw, d_ow;
    const float *bias, *mask, *add;
    float *dst;
};
__device__ __forceinline__ IgEp igb_epilogue_args(const IgemmP &p)
{
    IgEp e;
    e.rw0 = p.rw0; e.rw1 = p.rw1; e.scatter = p.scatter; e.DC = p.DC; e.OH = p.OH; e.OW = p.OW; e.DH = p.DH; e.DW = p.DW;
    e.dwy0 = p.dwy0; e.dwx0 = p.dwx0; e.M = p.M; e.cout = p.cout; e.Nn = p.Nn; e.dn0 = p.dn0; e.relu = p.relu;
    e.d_ohw = p.d_ohw; e.d_ow = p.d_ow;
    e.bias = p.bias; e.mask = p.mask; e.add = p.add; e.dst = p.dst;
    IGB_PIN(e.rw0); IGB_PIN(e.rw1); IGB_PIN(e.scatter); IGB_PIN(e.DC); IGB_PIN(e.OH); IGB_PIN(e.OW); IGB_PIN(e.DH); IGB_PIN(e.DW);
    IGB_PIN(e.dwy0); IGB_PIN(e.dwx0); IGB_PIN(e.M); IGB_PIN(e.cout); IGB_PIN(e.Nn); IGB_PIN(e.dn0); IGB_PIN(e.relu);
    IGB_PIN(e.d_ohw.mul); IGB_PIN(e.d_ohw.shift); IGB_PIN(e.d_ow.mul); IGB_PIN(e.d_ow.shift);
    // (the pointers are not pinned: behind the asm they would be generic pointers, i.e. FLAT instructions)
    return e;
}

}  // namespace unet
