"""fp64 numpy restatements of the layer-side memory-bound kernels of csrc/direct.hip (conv11c forward, weight / bias and
input gradient, the 2 x 2 max-pool forward and backward, column sums), written from the definitions, with the test data, the
error bounds and the shape arithmetic that tests/test_layer_ops_gpu.py uses.  tests/test_layer_ref_cpu.py pins every function
here without a device.  A plain helper module (imported like step_ref), not a conftest.

Layouts are the library's: images [B,S,S], activations NHWC, conv11c weights [K,3,3] (the reference's [K,1,3,3] without the
unit axis), tap t = 3 ty + tx.

Every floating-point result comes with A, the per-element sum of the magnitudes of its terms (plus |bias|): the scale of the
bound.

The bound (bound()).  A kernel forms each output as a sum of n terms in some order (registers, wave shuffles, LDS, a reduce
kernel), every product and every addition rounded once to fp32, u = 2^-24.  Higham (Accuracy and Stability of Numerical
Algorithms, 2nd ed., section 4.2 and eq. 3.5): for any order of summation |computed - exact| <= gamma_n A with
gamma_n = n u / (1 - n u).  The tests hold a kernel to (n + 2) u A: that is gamma_n with slack for the denominator up to
n = 5791 (n (n + 2) u <= 2), and beyond it the stricter of the two by the factor 1 - n u (0.96 at the largest n here, 729316), which
no kernel that sums in blocks comes near: its constant grows with the depth of the summation, not with n.  A sum without
products (the bias gradients) and a fused multiply-add (one rounding instead of two) only lower the constant.  ReLU and the pool's
selection are 1-Lipschitz and add no rounding.  A bf16 output is the fp32 result r rounded once more, to nearest, to
bf16's 8 significant bits (7 stored and the hidden one): neighbours are 2^-7 |r| apart at worst, so |bf16(r) - r| <= 2^-8 |r|
<= 2^-8 (|ref| + fp32 bound), which is added.  (2^-9 would be the unit roundoff of a 9-bit significand; bf16 rounds 1 + 2^-8
to 1.)  Nothing here is measured."""
import numpy as np

U32 = 2.0 ** -24          # unit roundoff of fp32
U16 = 2.0 ** -8           # unit roundoff of bf16 (8 significant bits: 7 stored and the hidden one)
EXACT_LIMIT = 2 ** 24     # every integer of magnitude <= 2^24 is an fp32 number


# ---- restatements -----------------------------------------------------------------------------------------------------------
def _windows(x):
    """x [B,S,S] -> the nine shifted views [9][B,So,So]: tap t = 3 ty + tx reads x[b, oy + ty, ox + tx]."""
    S = x.shape[1]
    So = S - 2
    return [x[:, ty:ty + So, tx:tx + So] for ty in range(3) for tx in range(3)]


def conv11c_fwd(x, w, bias):
    """y[b,oy,ox,k] = max(0, bias[k] + sum_t x[b,oy+ty,ox+tx] w[k,t]);  returns (y, A) as [B,So,So,K], n = 9."""
    x, w, bias = np.asarray(x, np.float64), np.asarray(w, np.float64).reshape(-1, 9), np.asarray(bias, np.float64)
    B, S, _ = x.shape
    z = np.broadcast_to(bias, (B, S - 2, S - 2, len(bias))).copy()
    A = np.abs(z)
    for t, xv in enumerate(_windows(x)):
        z += xv[..., None] * w[:, t]
        A += np.abs(xv)[..., None] * np.abs(w[:, t])
    return np.maximum(z, 0.0), A


def conv11c_wgrad(x, dz, chunk_rows=256):
    """dw[k,t] = sum_{b,oy,ox} x[b,oy+ty,ox+tx] dz[b,oy,ox,k],  db[k] = sum_{b,oy,ox} dz[b,oy,ox,k];  n = B So^2.
    Returns (dw [K,3,3], A_dw, db [K], A_db).  dz may be any float array: it is widened a block of rows at a time."""
    x = np.asarray(x, np.float64)
    B, S, _ = x.shape
    So = S - 2
    K = dz.shape[-1]
    assert dz.shape == (B, So, So, K)
    P = np.stack([v.reshape(B * So, So) for v in _windows(x)], -1)           # [rows, So, 9]
    Z = dz.reshape(B * So, So, K)
    dw = np.zeros((9, K)); Aw = np.zeros((9, K)); db = np.zeros(K); Ab = np.zeros(K)
    for r0 in range(0, B * So, chunk_rows):
        p = P[r0:r0 + chunk_rows].reshape(-1, 9)
        z = np.asarray(Z[r0:r0 + chunk_rows], np.float64).reshape(-1, K)
        dw += p.T @ z
        Aw += np.abs(p).T @ np.abs(z)
        db += z.sum(0)
        Ab += np.abs(z).sum(0)
    return dw.T.reshape(K, 3, 3).copy(), Aw.T.reshape(K, 3, 3).copy(), db, Ab


def conv11c_dgrad(dz, w):
    """dx[b,y,x] = sum_{k,ty,tx} dz[b,y-ty,x-tx,k] w[k,ty,tx] over the taps that land inside dz: the full correlation of dz
    with the flipped filter.  Returns (dx [B,S,S], A); n = 9 K."""
    dz, w = np.asarray(dz, np.float64), np.asarray(w, np.float64).reshape(-1, 3, 3)
    B, So, _, K = dz.shape
    S = So + 2
    dx = np.zeros((B, S, S)); A = np.zeros((B, S, S))
    for ty in range(3):
        for tx in range(3):
            dx[:, ty:ty + So, tx:tx + So] += dz @ w[:, ty, tx]
            A[:, ty:ty + So, tx:tx + So] += np.abs(dz) @ np.abs(w[:, ty, tx])
    return dx, A


def _quad(x):
    """x [B,H,W,C] -> its 2 x 2 windows [B,H/2,W/2,C,4] in row-major window order (00, 01, 10, 11)."""
    return np.stack([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]], -1)


def maxpool2_fwd(x):
    """y = the maximum of each 2 x 2 window, in x's dtype.  The maximum is one of the four stored values; where it is a zero
    it is +0.0 if any zero of the window is +0.0 (IEEE 754-2019 maximum: -0 < +0)."""
    q = _quad(np.asarray(x))
    y = q.max(-1)
    pos_zero = ((q == 0) & ~np.signbit(q)).any(-1)
    return np.where(y == 0, np.where(pos_zero, 0.0, -0.0).astype(y.dtype), y)


def maxpool2_bwd(pre, dy):
    """dpre = dy routed to the FIRST maximum of each window in row-major window order, times (max > 0): the pool's backward
    fused with the ReLU backward of the pooled tensor's producer.  Every other element, and every element of a window whose
    maximum is not positive, is +0.0.  (-0.0 == 0.0: neither beats the other.)"""
    pre, dy = np.asarray(pre), np.asarray(dy)
    q = _quad(pre)
    first = q.argmax(-1)                                                   # numpy's argmax returns the first maximum
    live = q.max(-1) > 0
    out = np.zeros(q.shape, dy.dtype)
    for i in range(4):
        out[..., i] = np.where(live & (first == i), dy, 0)
    d = np.zeros(pre.shape, dy.dtype)
    d[:, 0::2, 0::2], d[:, 0::2, 1::2], d[:, 1::2, 0::2], d[:, 1::2, 1::2] = (out[..., i] for i in range(4))
    return d


def column_sums(z):
    """s[k] = sum_m z[m,k] of an [M,K] matrix (any leading axes are flattened).  Returns (s, A); n = M."""
    z = np.asarray(z, np.float64).reshape(-1, np.shape(z)[-1])
    return z.sum(0), np.abs(z).sum(0)


# ---- bounds -----------------------------------------------------------------------------------------------------------------
def bound(n, A, ref=None, bf16_out=False):
    """Per-element bound of a sum of n terms in any order (module docstring); bf16_out adds the storage rounding."""
    b = (n + 2) * U32 * np.asarray(A, np.float64)
    if bf16_out:
        b = b + U16 * (np.abs(ref) + b)
    return b


def ratio(got, ref, bnd):
    """Worst |got - ref| / bound.  Where the bound is 0 (no non-zero term) the result must be exactly the reference."""
    got, ref, bnd = (np.asarray(a, np.float64) for a in (got, ref, bnd))
    err = np.abs(got - ref)
    assert np.all(err[bnd == 0] == 0), "a result without a non-zero term differs from the reference"
    return float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0


def bits(a):
    """The array as unsigned integers of its element size: equality of these is equality bit for bit (signed zeros included)."""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- test data --------------------------------------------------------------------------------------------------------------
def ints(seed, shape, lim):
    """Seeded integers in [-lim, lim] as float32: exact in fp32 and, for lim <= 256, in bf16."""
    return np.random.RandomState(seed).randint(-lim, lim + 1, size=shape).astype(np.float32)


def plant_zeros(a, seed, every=7):
    """Exact zeros in about one element of `every`, in place (seeded); returns a."""
    a[np.random.RandomState(seed).randint(0, every, size=a.shape) == 0] = 0
    return a


POOL_VALUES = np.array([-2.0, -0.5, -0.0, 0.0, 0.25, 1.0, 1.5, 3.0], np.float32)      # all exact in bf16; 3.0 is the largest
POOL_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
POOL_PATTERNS = ["four equal positive", "four equal +0.0", "four equal -0.0", "mixed zeros"] + \
                ["pair %d%d maximal" % p for p in POOL_PAIRS] + ["all non-positive"]


def pool_case(seed, B, H, W, C):
    """(pre [B,H,W,C] float32, dy [B,H/2,W/2,C] float32, pattern [B,H/2,W/2,C] int: -1 = left random, else the index into
    POOL_PATTERNS planted in that window).  Values are drawn from POOL_VALUES, so ties abound even where none is planted;
    every second window takes the next pattern of the list in turn."""
    rs = np.random.RandomState(seed)
    pre = POOL_VALUES[rs.randint(0, len(POOL_VALUES), size=(B, H, W, C))]
    q = _quad(pre).copy()                                                  # [B,Ho,Wo,C,4]
    nwin = q[..., 0].size
    flat = q.reshape(nwin, 4)
    pattern = np.full(nwin, -1)
    for j in range(0, nwin, 2):
        p = (j // 2) % len(POOL_PATTERNS)
        pattern[j] = p
        if p == 0:
            flat[j] = 1.5
        elif p == 1:
            flat[j] = 0.0
        elif p == 2:
            flat[j] = -0.0
        elif p == 3:
            flat[j] = (-0.0, 0.0, -0.0, 0.0) if (j // 2) % 2 else (0.0, -0.0, -0.0, -0.5)
        elif p < 4 + len(POOL_PAIRS):
            flat[j] = POOL_VALUES[rs.randint(0, 7, size=4)]                # anything below 3.0
            flat[j, list(POOL_PAIRS[p - 4])] = 3.0
        else:
            flat[j] = POOL_VALUES[rs.randint(0, 4, size=4)]                # -2, -0.5, -0.0, 0.0
    q = flat.reshape(q.shape)
    pre = np.empty_like(pre)
    pre[:, 0::2, 0::2], pre[:, 0::2, 1::2], pre[:, 1::2, 0::2], pre[:, 1::2, 1::2] = (q[..., i] for i in range(4))
    dy = ints(seed + 1, (B, H // 2, W // 2, C), 8)
    dy[dy == 0] = 5                                                        # a routed gradient is never mistaken for a zero
    return pre, dy, pattern.reshape(q.shape[:-1])


# ---- shape arithmetic of the launches (what the test shapes are chosen against) ----------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def conv11c_rows(B, S):
    return B * (S - 2)


def conv11c_fwd_grid(B, S):
    """Workgroups of the forward: one per output row up to 2048, rows beyond that by grid stride."""
    return min(conv11c_rows(B, S), 2048)


def conv11c_pixels_per_pass(K):
    """Pixels a 256-thread workgroup covers per pass: K / 4 lanes hold one pixel's channels."""
    return 256 // (K // 4)


def conv11c_wgrad_split(B, S):
    """(rows per workgroup, workgroups = partial vectors, rows of the last workgroup): at most 1024 partials."""
    nrows = conv11c_rows(B, S)
    rpb = cdiv(nrows, 1024)
    nb = cdiv(nrows, rpb)
    return rpb, nb, nrows - (nb - 1) * rpb


def conv11c_wgrad_lds_floats(S, K):
    """LDS floats of the weight-gradient workgroup: the three staged input rows or the [4 waves][10][K] reduction, whichever
    is larger; the rows win once 3 S > 40 K."""
    return max(3 * S, 40 * K)


def conv11c_wgrad_scratch_bytes(B, S, K):
    return conv11c_wgrad_split(B, S)[1] * 10 * K * 4


def pool_threads(B, H, W, C):
    """One thread per output pixel and group of four channels."""
    return B * (H // 2) * (W // 2) * (C // 4)


BIAS_ROWS = 2048


def bias_grad_blocks(M):
    return cdiv(M, BIAS_ROWS)


def bias_grad_slots(K):
    """(lanes per row = K / 4, rows a workgroup reads at once, idle threads of its 256)."""
    cg = K // 4
    return cg, 256 // cg, 256 - cg * (256 // cg)


# ---- the shapes of tests/test_layer_ops_gpu.py ------------------------------------------------------------------------------
FWD_CASES = [(B, S, K) for K in (32, 64) for S in (4, 8, 20, 36, 68) for B in (1, 3)] + [(1030, 4, 32), (1030, 4, 64)]
WGRAD_CASES = [(B, S, K) for K in (32, 64) for B, S in ((1, 4), (32, 4), (33, 4), (512, 4), (513, 4), (1025, 4), (103, 12), (3, 36))] + \
              [(1, 424, 32), (1, 428, 32)]
WGRAD_LARGE = (1, 856, 64)
DGRAD_CASES = [(B, S, K) for K in (32, 64) for S in (4, 8, 20) for B in (1, 3)] + [(2, 188, 64)]
POOL_CASES = [(1, 2, 2, 4), (3, 6, 10, 12), (1, 2, 34, 60), (1, 2, 32, 64), (1, 2, 514, 4), (2, 14, 6, 128), (1, 4, 2, 1024)]
BIAS_SHAPES = [(1, 3), (7, 19), (2, 34), (57, 8), (2, 73), (8, 50)]             # (B, H) of the conv's input; M = B (H - 2)^2
BIAS_K = {4: (32, 64, 96, 256, 1024), 2: (64, 256)}                             # by element size of dz
BIAS_UP_CASES = [(2, 16, 64, 64), (1, 5, 64, 32)]                               # (B, H, Ci, Co); M = 4 B H^2 rows of Co
