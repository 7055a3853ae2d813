"""Data, samplers and references for tests/test_large_tensors_gpu.py: the per-op kernels on tensors just below 2 GiB, just
above 2 GiB and just above 4 GiB, held to exact results.  A plain helper module (imported like kernel_paths and guarded),
checked without a device by tests/test_large_tensors_cpu.py.  Everything here runs on any torch device; the only tools are
torch's generators, 64-bit index gathers and einsum in fp64.

Why the results are exact.  Every input is a small integer:

    activations x        |x|   <= XMAX   = 3        filters w        |w|   <= WMAX = 2
    bias b               |b|   <= BMAX   = 4        add (skip grad)  |add| <= AMAX = 8
    gradients dz         |dz|  <= DZMAX  = 2        mask in {0, 1}

An fp32 sum of such products is exact in every order as long as every partial sum is an integer below 2^24 (or a multiple
of 2^-k below 2^(24-k)): the partial sums of s = sum a_i are bounded by A = sum |a_i|, so A 2^k < 2^24 = EXACT is enough.

  * direct forward / dgrad (igemm, igemmx, the bf16 kernels' fp32 accumulators): A <= 9 C XMAX WMAX + BMAX + AMAX = 54 C + 12,
    3468 at C = 64, 6924 over a 128-channel virtual concat; k = 0.  direct_bound().
  * bf16x3 (mode 1): an integer below 2^8 is its own first bf16 piece and the second piece is 0, so the three products of
    the split are the exact product and two zeros: the same sum.
  * bf16 tensors (mode 2): the integers are exact in bf16, the accumulator is the exact fp32 sum, and the one rounding of
    the store is kernel_bounds.rne_bf16 of the exact value.
  * Winograd F(2x2, 3x3) forward / dgrad (wino32): the input transform B^T d B has entries +-1, at most two per row:
    |V| <= 4 XMAX, integers.  The filter transform G g G^T has rows of absolute sum <= 3/2 and entries that are multiples of
    1/2: U is a multiple of 1/4 with |U| <= 9/4 WMAX.  The 16 GEMMs sum C products each, and the output transform A^T M A
    adds 3 x 3 of them: A <= 9 C (4 XMAX) (9/4 WMAX) + BMAX + AMAX = 486 C + 12 in units of 1/4 (k = 2): 31116 x 4 < 2^24
    at C = 64.  wino_fwd_bound().
  * weight gradient, direct (wgrad<..split0>, <..split3>, wgradb): dw[k][c][t] = sum over ALL pixels of x dz, the partial
    sums of a workgroup are register-resident over many pixels and the slabs are then added: any order, so the bound is
    A[k][c][t] = sum |x| |dz| itself.  Dense data would pass 2^24 (16.8 M pixels x 3 x 2), so dz is thinned: DENSITY of its
    pixels are non-zero, plus forced ones (thin()).  The bound is asserted from the actual data (wgrad_ref returns A).
  * weight gradient, Winograd F(3x3 <- 2x2) (wgradw): V as above (|V| <= 4 |x|, integers); the dz transform G2 dz G2^T has
    coefficients of absolute value <= 1 and multiples of 1/4: |Z| <= sum of the tile's |dz|, in units of 1/4.  The 16
    accumulators sum V Z over all tiles and the output transform adds 3 x 3 of them:
    A_w <= 9 x 4 x max|x| x sum_pixels |dz[.][k]|  in units of 1/4 (k = 2).  wgradw_bound(), asserted from the data.
  * bias gradient: db[k] = sum dz[.][k], A = sum |dz[.][k]| (asserted from the data; the dense dz of the dx-only pass is
    never summed).
No path of the 3x3 and up-conv kernels is left inexact by this, so kernel_bounds.acc_slack is not used by these tests."""
import numpy as np
import torch

EXACT = 1 << 24
XMAX, WMAX, BMAX, AMAX, DZMAX = 3, 2, 4, 8, 2
DENSITY = 2.0 ** -10
LIMITS = (1 << 31, 1 << 32)          # the byte offsets a 32-bit offset loses its sign bit / wraps at
N_SAMPLES = 1 << 16

# the standard transform matrices (Lavin & Gray 2016; points 0, 1, -1, inf)
BT = ((1, 0, -1, 0), (0, 1, 1, 0), (0, -1, 1, 0), (0, 1, 0, -1))
G3 = ((1, 0, 0), (.5, .5, .5), (.5, -.5, .5), (0, 0, 1))          # F(2, 3): filter 3 -> 4
AT2 = ((1, 1, 1, 0), (0, 1, -1, -1))                              # F(2, 3): 4 -> 2 outputs
G2 = ((1, 0), (.5, .5), (.5, -.5), (0, 1))                        # F(3, 2): "filter" (the dz tile) 2 -> 4
AT3 = ((1, 1, 1, 0), (0, 1, -1, 0), (0, 1, 1, -1))                # F(3, 2): 4 -> 3 outputs (the 3 x 3 gradient)


# ---- bounds -----------------------------------------------------------------------------------------------------------------
def direct_bound(C):
    return 9 * C * XMAX * WMAX + BMAX + AMAX


def wino_fwd_bound(C):
    """In units of 1/4."""
    return 4 * (9 * C * (4 * XMAX) * (9 * WMAX / 4.0) + BMAX + AMAX)


def wgradw_bound(xmax, dz_abs_sums):
    """In units of 1/4; dz_abs_sums = sum over pixels of |dz| per channel."""
    return 4 * 9 * 4 * xmax * float(dz_abs_sums.max())


# ---- data -------------------------------------------------------------------------------------------------------------------
def gen(device, seed):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return g


def ints(t, amax, g):
    """Fill t (any float dtype, in place: a guarded.Arena output) with integers uniform in [-amax, amax]."""
    return t.random_(-amax, amax + 1, generator=g)


def bits01(t, g):
    return t.random_(0, 2, generator=g)


def thin(dz, g, forced, density=DENSITY):
    """Zero all but `density` of the pixels of dz [B, H, W, K] (whole pixels, so the fp64 weight gradient is a contraction over
    the few that are left), then make the `forced` pixels (flat indices) non-zero in every channel.  Returns the flat indices
    of the non-zero pixels, sorted."""
    K = dz.shape[-1]
    flat = dz.view(-1, K)
    keep = torch.rand(flat.shape[0], generator=g, device=dz.device) < density
    flat.masked_fill_(~keep[:, None], 0)
    forced = torch.as_tensor(sorted(set(int(p) for p in forced)), dtype=torch.int64, device=dz.device)
    pattern = torch.tensor([1, -2, 2, -1], dtype=dz.dtype, device=dz.device).repeat((K + 3) // 4)[:K]
    flat[forced] = pattern
    keep[forced] = True
    return keep.nonzero().flatten()


# ---- strategic pixels -------------------------------------------------------------------------------------------------------
def straddlers(npix, bytes_per_pixel, limits=LIMITS):
    """The pixels (flat indices) of a tensor that hold the last byte below and the first byte at or above each limit."""
    out = []
    for lim in limits:
        for byte in (lim - 1, lim):
            p = byte // bytes_per_pixel
            if 0 <= p < npix:
                out.append(p)
    return sorted(set(out))


def readers(q, src, dst, pad, taps=3, stride=1):
    """The output pixels (flat, in dst = (B, OH, OW)) one of whose taps reads source pixel q (flat, in src = (B, H, W)): output
    (oy, ox) reads source (oy stride + ty - pad, ox stride + tx - pad)."""
    B, H, W = src
    _, OH, OW = dst
    b, r = divmod(q, H * W)
    iy, ix = divmod(r, W)
    out = []
    for ty in range(taps):
        for tx in range(taps):
            ny, nx = iy - ty + pad, ix - tx + pad
            if ny % stride or nx % stride:
                continue
            oy, ox = ny // stride, nx // stride
            if 0 <= oy < OH and 0 <= ox < OW:
                out.append((b * OH + oy) * OW + ox)
    return out


def corners(B, OH, OW):
    """Corner pixels of the first and last image, and the pixels on both sides of each image boundary."""
    out = []
    for b in sorted({0, B - 1}):
        for oy in (0, OH - 1):
            for ox in (0, OW - 1):
                out.append((b * OH + oy) * OW + ox)
    for b in range(1, B):
        out += [b * OH * OW - 1, b * OH * OW]
    return sorted(set(out))


def strategic(dst, dst_bpp, sources, limits=LIMITS, taps=3, stride=1):
    """{kind: pixels} of the output domain dst = (B, OH, OW) with dst_bpp bytes per pixel, for sources = [((B, H, W), bytes per
    pixel, pad), ...]: "corner", "dst" (destination straddlers) and "src" (every reader of a source straddler)."""
    B, OH, OW = dst
    kinds = {"corner": corners(B, OH, OW), "dst": straddlers(B * OH * OW, dst_bpp, limits), "src": []}
    for shape, bpp, pad in sources:
        for q in straddlers(shape[0] * shape[1] * shape[2], bpp, limits):
            kinds["src"] += readers(q, shape, dst, pad, taps, stride)
    kinds["src"] = sorted(set(kinds["src"]))
    return kinds


def sample_pixels(dst, dst_bpp, sources, seed, n=N_SAMPLES, limits=LIMITS, taps=3, stride=1, keep_strategic=True):
    """At least min(n, all) distinct output pixels, sorted (int64, CPU): the strategic ones, the rest random.
    keep_strategic=False drops the straddling pixels - the broken sampler of the CPU tests."""
    B, OH, OW = dst
    npix = B * OH * OW
    kinds = strategic(dst, dst_bpp, sources, limits, taps, stride)
    must = set(kinds["corner"])
    if keep_strategic:
        must |= set(kinds["dst"]) | set(kinds["src"])
    g = torch.Generator().manual_seed(seed)
    if npix <= n:
        rest = torch.arange(npix)
    else:
        rest = torch.empty(0, dtype=torch.int64)
        while len(rest) < n:                                      # (draws repeat: top up until n distinct ones)
            rest = torch.unique(torch.cat([rest, torch.randint(0, npix, (n - len(rest) + 64,), generator=g)]))
    if not keep_strategic:
        drop = torch.tensor(sorted(set(kinds["dst"]) | set(kinds["src"])) or [-1])
        rest = rest[~torch.isin(rest, drop)]
    return torch.unique(torch.cat([torch.tensor(sorted(must), dtype=torch.int64), rest]))


# ---- fp64 references --------------------------------------------------------------------------------------------------------
def gather_patches(src, pix, dst, pad, taps=3, stride=1):
    """[n, taps^2, C] fp64: the taps of the output pixels `pix` (flat in dst = (B, OH, OW)) in src [B, H, W, C], zero outside;
    all indices are int64."""
    B, H, W, C = src.shape
    _, OH, OW = dst
    pix = pix.to(src.device, torch.int64)
    b = pix // (OH * OW)
    r = pix - b * (OH * OW)
    oy = r // OW
    ox = r - oy * OW
    flat = src.view(-1, C)
    out = torch.zeros(len(pix), taps * taps, C, dtype=torch.float64, device=src.device)
    for t in range(taps * taps):
        iy, ix = oy * stride + t // taps - pad, ox * stride + t % taps - pad
        ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
        idx = (b * H + iy) * W + ix
        out[ok, t] = flat[idx[ok]].double()
    return out


def rows(t, pix):
    """The rows `pix` of t [..., C] flattened to pixels, fp64."""
    return t.view(-1, t.shape[-1])[pix.to(t.device, torch.int64)].double()


def conv_fwd_ref(xs, w, bias, pix, dst, relu=True):
    """y[pix] [n, K] of the valid 3 x 3 conv over the virtual concat of xs = [(x [B, H_i, W_i, C_i], pad_i), ...] (channels in
    that order), + bias, ReLU.  Returns (y, A)."""
    K = w.shape[0]
    y = torch.zeros(len(pix), K, dtype=torch.float64, device=w.device)
    A = torch.zeros_like(y)
    c0 = 0
    for x, pad in xs:
        C = x.shape[-1]
        p = gather_patches(x, pix, dst, pad)
        wk = w[:, c0:c0 + C].double().reshape(K, C, 9)
        y += torch.einsum("ntc,kct->nk", p, wk)
        A += torch.einsum("ntc,kct->nk", p.abs(), wk.abs())
        c0 += C
    if bias is not None:
        y += bias.double()
        A += bias.double().abs()
    return (y.clamp_(min=0) if relu else y), A


def conv_dgrad_ref(dz, w, c0, C, pix, dst, o0, mask=None, add=None):
    """dx[pix] [n, C] of source channels [c0, c0 + C): the full correlation of dz [B, OH, OW, K] with the flipped filter over
    the window of extent dst[1] at offset o0 of the conv's (virtual) input, + add, masked (mask > 0).  Returns (dx, A)."""
    K = w.shape[0]
    p = gather_patches(dz, pix, dst, 2 - o0)
    wk = w[:, c0:c0 + C].double().flip(2, 3).reshape(K, C, 9)
    dx = torch.einsum("ntk,kct->nc", p, wk)
    A = torch.einsum("ntk,kct->nc", p.abs(), wk.abs())
    if add is not None:
        dx += rows(add, pix)
        A += rows(add, pix).abs()
    if mask is not None:
        dx = torch.where(rows(mask, pix) > 0, dx, torch.zeros_like(dx))
    return dx, A


def wgrad_ref(x, pad, dz, nz):
    """dw [K, C, 3, 3] and db [K] in fp64 from the non-zero pixels nz of dz [B, OH, OW, K] - every pixel that contributes - against
    source x [B, H, W, C] zero-padded by pad; with them A_w (the same contraction of absolute values) and A_b."""
    B, OH, OW, K = dz.shape
    C = x.shape[-1]
    p = gather_patches(x, nz, (B, OH, OW), pad)
    d = rows(dz, nz)
    dw = torch.einsum("ntc,nk->kct", p, d).reshape(K, C, 3, 3)
    Aw = torch.einsum("ntc,nk->kct", p.abs(), d.abs()).reshape(K, C, 3, 3)
    return dw, Aw, d.sum(0), d.abs().sum(0)


def upconv_fwd_ref(x, w, bias, pix, dst):
    """y[pix] [n, Co] of the 2 x 2 stride-2 transposed conv (w [Ci, Co, 2, 2]): output (2 y + a, 2 x + b) = x[y][x] . w[:, :, a, b]."""
    B, OH, OW = dst
    pix = pix.to(x.device, torch.int64)
    b = pix // (OH * OW)
    r = pix - b * (OH * OW)
    oy = r // OW
    ox = r - oy * OW
    src = rows(x, (b * (OH // 2) + oy // 2) * (OW // 2) + ox // 2)
    wk = w.double()[:, :, oy % 2, ox % 2]                        # [Ci, Co, n]
    y = torch.einsum("nc,con->no", src, wk)
    A = torch.einsum("nc,con->no", src.abs(), wk.abs())
    return y + bias.double(), A + bias.double().abs()


def upconv_dgrad_ref(dy, w, pix, dst, mask=None):
    """dx[pix] [n, Ci] = sum_{a, b, co} dy[2 y + a][2 x + b][co] w[ci][co][a][b], masked."""
    p = gather_patches(dy, pix, dst, 0, taps=2, stride=2)        # [n, 4, Co]
    wk = w.double().reshape(w.shape[0], w.shape[1], 4)           # [Ci, Co, 4]
    dx = torch.einsum("nto,cot->nc", p, wk)
    A = torch.einsum("nto,cot->nc", p.abs(), wk.abs())
    if mask is not None:
        dx = torch.where(rows(mask, pix) > 0, dx, torch.zeros_like(dx))
    return dx, A


def upconv_wgrad_ref(x, dy, nz):
    """dw [Ci, Co, 2, 2], db [Co] from the pixels nz of x [B, H, W, Ci] (flat) whose 2 x 2 block of dy is non-zero, and A's."""
    B, H, W, Ci = x.shape
    p = gather_patches(dy, nz, (B, H, W), 0, taps=2, stride=2)   # [n, 4, Co]
    xi = rows(x, nz)
    dw = torch.einsum("nc,nto->cot", xi, p).reshape(Ci, -1, 2, 2)
    Aw = torch.einsum("nc,nto->cot", xi.abs(), p.abs()).reshape(Ci, -1, 2, 2)
    return dw, Aw, p.sum((0, 1)), p.abs().sum((0, 1))


# ---- comparison -------------------------------------------------------------------------------------------------------------
def assert_sampled(got, pix, ref, what, post=None):
    """Every channel of the rows `pix` of got [..., C] equals ref [n, C] (fp64; post: the expected rounding of ref, e.g.
    kernel_bounds.rne_bf16 for a bf16 output)."""
    g = rows(got, pix)
    r = ref if post is None else torch.from_numpy(post(ref.cpu().numpy())).to(ref.device)
    bad = ~(g == r)                                               # (a NaN is bad)
    if bool(bad.any()):
        i, c = (int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d sampled elements differ from the fp64 reference, first at pixel %d channel %d: %r != %r"
                             % (what, int(bad.sum()), bad.numel(), int(pix[i]), c, float(g[i, c]), float(r[i, c])))


def same_bits(a, b):
    """Device-side: the two tensors hold the same bytes."""
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- fp32 evaluations for the CPU proof of exactness ------------------------------------------------------------------------
def direct_fwd(x, w, bias, dtype, reverse=False):
    """The whole valid 3 x 3 conv of x [B, H, W, C] in `dtype`, one product at a time: taps then channels, or in the reverse order."""
    B, H, W, C = x.shape
    K = w.shape[0]
    y = torch.zeros(B, H - 2, W - 2, K, dtype=dtype)
    order = [(t, c) for t in range(9) for c in range(C)]
    for t, c in (reversed(order) if reverse else order):
        y += x[:, t // 3:t // 3 + H - 2, t % 3:t % 3 + W - 2, c, None].to(dtype) * w[:, c, t // 3, t % 3].to(dtype)
    return y + bias.to(dtype)


def _m(rows_, dtype):
    return torch.tensor(rows_, dtype=dtype)


def _tiles(x, n, step):
    """[B, TY, TX, n, n, C] windows of x [B, H, W, C] at stride `step`."""
    return x.unfold(1, n, step).unfold(2, n, step).permute(0, 1, 2, 4, 5, 3)


def wino_fwd(x, w, bias, dtype):
    """F(2x2, 3x3) in `dtype` with the standard matrices (even output extents)."""
    B, H, W, C = x.shape
    K = w.shape[0]
    assert H % 2 == 0 and W % 2 == 0
    bt, g, at = _m(BT, dtype), _m(G3, dtype), _m(AT2, dtype)
    V = torch.einsum("ai,...ijc,bj->...abc", bt, _tiles(x.to(dtype), 4, 2), bt)
    U = torch.einsum("ai,kcij,bj->kcab", g, w.to(dtype), g)
    M = torch.einsum("...abc,kcab->...abk", V, U)
    Y = torch.einsum("pa,...abk,qb->...pqk", at, M, at)                       # [B, TY, TX, 2, 2, K]
    return Y.permute(0, 1, 3, 2, 4, 5).reshape(B, H - 2, W - 2, K) + bias.to(dtype)


def wino_wgrad(x, dz, dtype):
    """F(3x3 <- 2x2) weight gradient in `dtype`: dw [K, C, 3, 3] (even dz extents)."""
    B, H, W, C = x.shape
    assert dz.shape[1] % 2 == 0 and dz.shape[2] % 2 == 0
    bt, g, at = _m(BT, dtype), _m(G2, dtype), _m(AT3, dtype)
    V = torch.einsum("ai,...ijc,bj->...abc", bt, _tiles(x.to(dtype), 4, 2), bt)
    Z = torch.einsum("ai,...ijk,bj->...abk", g, _tiles(dz.to(dtype), 2, 2), g)
    M = torch.einsum("nyxabc,nyxabk->abkc", V, Z)
    return torch.einsum("pa,abkc,qb->kcpq", at, M, at)


def direct_wgrad(x, dz, dtype, reverse=False):
    B, H, W, C = x.shape
    K = dz.shape[-1]
    dw = torch.zeros(K, C, 3, 3, dtype=dtype)
    imgs = range(B - 1, -1, -1) if reverse else range(B)
    for b in imgs:
        for t in (range(8, -1, -1) if reverse else range(9)):
            xs = x[b, t // 3:t // 3 + H - 2, t % 3:t % 3 + W - 2].to(dtype).reshape(-1, C)
            d = dz[b].to(dtype).reshape(-1, K)
            if reverse:
                xs, d = xs.flip(0), d.flip(0)
            for r in range(0, xs.shape[0], 7):                                # short partial sums, added one after the other
                dw[:, :, t // 3, t % 3] += d[r:r + 7].T @ xs[r:r + 7]
    return dw


def np64(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)
