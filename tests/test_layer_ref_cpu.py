"""tests/layer_ref.py without a device: every restatement against fp64 torch.nn.functional on random data and against
hand-worked cases, the planted pool patterns, the bound helpers, and the shape arithmetic that the cases of
tests/test_layer_ops_gpu.py are chosen against (block counts, rows per block, element totals)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_ref as lr


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def rand(seed, *shape):
    return np.random.RandomState(seed).standard_normal(shape)


# ---- conv11c ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,K", [(1, 4, 32), (3, 8, 64), (2, 20, 5)])
def test_conv11c_against_torch(B, S, K):
    x, w, b = rand(1, B, S, S), rand(2, K, 3, 3), rand(3, K)
    dz = rand(4, B, S - 2, S - 2, K)
    xt, wt = t64(x)[:, None].requires_grad_(True), t64(w)[:, None].requires_grad_(True)
    z = F.conv2d(xt, wt, t64(b))
    z.backward(t64(dz).permute(0, 3, 1, 2))
    y, A = lr.conv11c_fwd(x, w, b)
    assert np.allclose(y, F.relu(z).detach().permute(0, 2, 3, 1).numpy(), rtol=1e-13, atol=1e-13)
    assert np.all(A >= np.abs(y)) and A.shape == y.shape
    dw, Aw, db, Ab = lr.conv11c_wgrad(x, dz)
    dw2, Aw2, db2, Ab2 = lr.conv11c_wgrad(x, dz.astype(np.float32).astype(np.float64), chunk_rows=3)      # the blocked walk
    assert np.allclose(dw, wt.grad[:, 0].numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(db, dz.sum((0, 1, 2)), rtol=1e-12, atol=1e-12)
    assert np.allclose(dw2, dw, rtol=1e-6, atol=1e-6) and np.allclose(Aw2, Aw, rtol=1e-6) and np.allclose(db2, db, atol=1e-5) and np.allclose(Ab2, Ab, rtol=1e-6)
    assert np.all(Aw >= np.abs(dw)) and np.all(Ab >= np.abs(db))
    dx, Ax = lr.conv11c_dgrad(dz, w)
    assert np.allclose(dx, xt.grad[:, 0].numpy(), rtol=1e-12, atol=1e-12)
    assert np.all(Ax >= np.abs(dx) - 1e-12)


def test_conv11c_hand_worked_4x4():
    """x[i][j] = 4 i + j.  Filter 0: all ones, bias 1; filter 1: -1 at tap (0, 1), bias 0 (every output clipped by the ReLU);
    filter 2: 2 at tap (2, 2), bias -20 (one output exactly 0 before the ReLU)."""
    x = np.arange(16.0).reshape(1, 4, 4)
    w = np.zeros((3, 3, 3)); w[0] = 1; w[1, 0, 1] = -1; w[2, 2, 2] = 2
    b = np.array([1.0, 0.0, -20.0])
    y, A = lr.conv11c_fwd(x, w, b)
    assert y.shape == (1, 2, 2, 3)
    assert y[0, :, :, 0].tolist() == [[46, 55], [82, 91]]
    assert y[0, :, :, 1].tolist() == [[0, 0], [0, 0]]
    assert y[0, :, :, 2].tolist() == [[0, 2], [8, 10]]
    assert A[0, :, :, 0].tolist() == [[46, 55], [82, 91]]
    assert A[0, :, :, 1].tolist() == [[1, 2], [5, 6]]                       # |x[oy][ox+1]|, although y is 0
    assert A[0, :, :, 2].tolist() == [[40, 42], [48, 50]]                   # 2 x[oy+2][ox+2] + |-20|
    # weight gradient of one filter for dz = [[1, 2], [3, 4]]: dw[ty][tx] = 10 (4 ty + tx) + 34, db = 10
    dz = np.array([[1.0, 2.0], [3.0, 4.0]]).reshape(1, 2, 2, 1)
    dw, Aw, db, Ab = lr.conv11c_wgrad(x, dz)
    assert dw[0].tolist() == [[34, 44, 54], [74, 84, 94], [114, 124, 134]]
    assert Aw[0].tolist() == dw[0].tolist() and db.tolist() == [10] and Ab.tolist() == [10]
    dw, _, db, Ab = lr.conv11c_wgrad(x, -dz)
    assert dw[0, 0, 0] == -34 and db.tolist() == [-10] and Ab.tolist() == [10]
    # input gradient: the full convolution of dz with w = [[1,2,3],[4,5,6],[7,8,9]], by the definition's four loops
    wk = np.arange(1.0, 10.0).reshape(1, 3, 3)
    dx, Ax = lr.conv11c_dgrad(dz, wk)
    want = np.zeros((4, 4))
    for oy in range(2):
        for ox in range(2):
            for ty in range(3):
                for tx in range(3):
                    want[oy + ty, ox + tx] += dz[0, oy, ox, 0] * wk[0, ty, tx]
    assert dx[0].tolist() == want.tolist() and Ax[0].tolist() == want.tolist()
    assert dx[0, 0, 0] == 1 and dx[0, 0, 1] == 4 and dx[0, 1, 1] == 23 and dx[0, 3, 3] == 36 and dx[0, 0, 3] == 6 and dx[0, 3, 0] == 21


# ---- max-pool ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", [(2, 6, 10, 3), (1, 2, 2, 4), (1, 8, 4, 5)])
def test_maxpool_against_torch(B, H, W, C):
    pre = np.round(rand(1, B, H, W, C) * 2) / 2                             # halves: many ties, zeros and negatives
    dy = rand(2, B, H // 2, W // 2, C)
    p = t64(pre).permute(0, 3, 1, 2).requires_grad_(True)
    y = F.max_pool2d(F.relu(p), 2, 2)
    y.backward(t64(dy).permute(0, 3, 1, 2))
    mine = lr.maxpool2_fwd(pre)
    assert np.array_equal(mine, F.max_pool2d(p.detach(), 2, 2).permute(0, 2, 3, 1).numpy())
    assert np.array_equal(np.maximum(mine, 0), y.detach().permute(0, 2, 3, 1).numpy())
    assert np.array_equal(lr.maxpool2_bwd(pre, dy), p.grad.permute(0, 2, 3, 1).numpy())


def test_maxpool_hand_worked_ties():
    one = lambda a: np.array(a, np.float32).reshape(1, 2, 2, 1)
    dy = np.full((1, 1, 1, 1), 7.0, np.float32)
    assert lr.maxpool2_fwd(one([[2, 2], [2, 2]])).tolist() == [[[[2]]]]
    assert lr.maxpool2_bwd(one([[2, 2], [2, 2]]), dy)[0, :, :, 0].tolist() == [[7, 0], [0, 0]]         # four-way tie: the first
    assert lr.maxpool2_bwd(one([[1, 2], [2, 2]]), dy)[0, :, :, 0].tolist() == [[0, 7], [0, 0]]
    assert lr.maxpool2_bwd(one([[1, 1], [2, 2]]), dy)[0, :, :, 0].tolist() == [[0, 0], [7, 0]]
    assert lr.maxpool2_bwd(one([[1, 1], [1, 2]]), dy)[0, :, :, 0].tolist() == [[0, 0], [0, 7]]
    for zeros in ([[0, 0], [0, 0]], [[-0.0, 0.0], [-1, -2]], [[-3, -1], [-1, -2]]):
        d = lr.maxpool2_bwd(one(zeros), dy)
        assert np.all(d == 0) and not np.signbit(d).any()                                             # (max > 0) fails: +0.0 everywhere
    # signed zeros of the forward: +0.0 wins wherever it stands, -0.0 only survives alone
    for win, neg in (([[-0.0, 0.0], [-1, -2]], False), ([[0.0, -0.0], [-0.0, -0.0]], False), ([[-0.0, -0.0], [-0.0, -0.0]], True),
                     ([[-1, -0.0], [-2, -3]], True), ([[-1, -2], [-3, 0.0]], False)):
        y = lr.maxpool2_fwd(one(win))
        assert y[0, 0, 0, 0] == 0 and bool(np.signbit(y[0, 0, 0, 0])) == neg, win
    assert lr.maxpool2_fwd(one([[-1, -2], [-0.5, -3]]))[0, 0, 0, 0] == -0.5
    assert lr.maxpool2_fwd(one([[1, 2], [3, 4]])).dtype == np.float32


def test_pool_cases_plant_every_pattern():
    seen = set()
    for i, (B, H, W, C) in enumerate(lr.POOL_CASES):
        pre, dy, pat = lr.pool_case(10 + i, B, H, W, C)
        assert pre.shape == (B, H, W, C) and dy.shape == pat.shape == (B, H // 2, W // 2, C) and pre.dtype == dy.dtype == np.float32
        assert np.isin(pre, lr.POOL_VALUES).all() and (dy != 0).all() and np.abs(dy).max() <= 8
        assert np.array_equal(pre, torch.from_numpy(pre).bfloat16().float().numpy())                  # exact in bf16
        q = lr._quad(pre)
        m = q.max(-1)
        for p, name in enumerate(lr.POOL_PATTERNS):
            sel = pat == p
            if not sel.any():
                continue
            seen.add(p)
            w = q[sel]
            if name == "four equal positive":
                assert np.all(w == 1.5)
            elif name == "four equal +0.0":
                assert np.all(w == 0) and not np.signbit(w).any()
            elif name == "four equal -0.0":
                assert np.all(w == 0) and np.signbit(w).all()
            elif name == "mixed zeros":
                assert np.all(m[sel] == 0) and np.signbit(w).any() and (~np.signbit(w)).any()
            elif name.startswith("pair"):
                a, b = lr.POOL_PAIRS[p - 4]
                assert np.all(m[sel] == 3.0) and np.all((w == 3.0).sum(-1) == 2) and np.all(w[:, a] == 3.0) and np.all(w[:, b] == 3.0)
            else:
                assert np.all(m[sel] <= 0)
        if pat.size >= 2 * len(lr.POOL_PATTERNS):
            assert set(range(len(lr.POOL_PATTERNS))) <= set(pat.ravel().tolist()), (B, H, W, C)
        # the reference routes each of them as stated
        d = lr._quad(lr.maxpool2_bwd(pre, dy))
        assert np.all((d != 0).sum(-1) == (m > 0))
        first = np.argmax(q == m[..., None], -1)
        assert np.array_equal(np.take_along_axis(d, first[..., None], -1)[..., 0], np.where(m > 0, dy, 0))
    assert seen == set(range(len(lr.POOL_PATTERNS)))
    assert sorted(lr.pool_threads(*c) for c in lr.POOL_CASES) == [1, 135, 255, 256, 257, 512, 1344]     # either side of one 256-thread block
    assert sorted(c[3] // 4 for c in lr.POOL_CASES) == [1, 1, 3, 15, 16, 32, 256]                          # C / 4 not a power of two: 3, 15


# ---- column sums, bounds, data ----------------------------------------------------------------------------------------------
def test_column_sums_bounds_and_data():
    z = rand(5, 3, 7, 11, 8)
    s, A = lr.column_sums(z)
    assert np.allclose(s, t64(z).sum((0, 1, 2)).numpy(), rtol=1e-13) and np.allclose(A, np.abs(z).sum((0, 1, 2)), rtol=1e-13)
    s, A = lr.column_sums(np.array([[1.0, -2.0], [3.0, 2.0]]))
    assert s.tolist() == [4, 0] and A.tolist() == [4, 4]
    # the bound: (n + 2) u A, and for a bf16 output one more rounding of |ref| + that
    assert lr.bound(9, np.array([2.0]))[0] == 11 * 2.0 ** -24 * 2
    b = lr.bound(9, np.array([2.0]), ref=np.array([1.0]), bf16_out=True)[0]
    assert b == 22 * 2.0 ** -24 + 2.0 ** -8 * (1 + 22 * 2.0 ** -24)
    # bf16 keeps 8 significant bits: rounding to nearest errs by up to 2^-8 relative, and by more than 2^-9 somewhere
    v = torch.linspace(1.0, 2.0, 100001, dtype=torch.float64)
    rel = ((v.float().bfloat16().double() - v).abs() / v).max().item()
    assert 2.0 ** -9 < rel <= lr.U16 == 2.0 ** -8 and torch.tensor(1 + 2.0 ** -8).bfloat16().item() == 1.0
    assert lr.ratio(np.array([1.0, 0.0]), np.array([1.5, 0.0]), np.array([1.0, 0.0])) == 0.5
    with pytest.raises(AssertionError):
        lr.ratio(np.array([1.0, 1e-30]), np.array([1.0, 0.0]), np.array([1.0, 0.0]))
    # (n + 2) u covers gamma_n = n u / (1 - n u) up to n = 5791; beyond that it is the stricter of the two, by 1 - n u
    for n in (9, 576, 2052, 4100, 5791):
        assert n * lr.U32 / (1 - n * lr.U32) <= (n + 2) * lr.U32
    for n in (5792, 18432, 729316):
        assert (1 - n * lr.U32) * n * lr.U32 / (1 - n * lr.U32) <= (n + 2) * lr.U32 < n * lr.U32 / (1 - n * lr.U32)
    # bit equality tells the zeros apart; integer data is what it says
    assert not np.array_equal(lr.bits(np.float32([0.0])), lr.bits(np.float32([-0.0])))
    a = lr.ints(3, (1000,), 4)
    assert a.dtype == np.float32 and a.min() == -4 and a.max() == 4 and np.all(a == np.round(a))
    z = lr.plant_zeros(rand(1, 1000).astype(np.float32), 2)
    assert 80 < (z == 0).sum() < 220


# ---- shape arithmetic -------------------------------------------------------------------------------------------------------
def test_shape_arithmetic():
    # forward: a partial pass (So < pixels per pass), ragged passes for both lanes-per-pixel values, more rows than the grid
    assert lr.conv11c_pixels_per_pass(64) == 16 and lr.conv11c_pixels_per_pass(32) == 32
    assert [S - 2 for S in (4, 8, 20, 36, 68)] == [2, 6, 18, 34, 66]          # 2, 6 < 16; 18 = 16 + 2; 34 = 32 + 2 = 2 * 16 + 2; 66 = 2 * 32 + 2
    assert lr.conv11c_rows(1030, 4) == 2060 and lr.conv11c_fwd_grid(1030, 4) == 2048 and lr.conv11c_fwd_grid(3, 68) == 198
    assert all(S % 4 == 0 for _, S, _ in lr.FWD_CASES + lr.WGRAD_CASES + lr.DGRAD_CASES + [lr.WGRAD_LARGE])
    # weight gradient: partial counts around the reduce's 64 lanes, then rows per block 2 and 3 with a short last block
    split = {(B, S): lr.conv11c_wgrad_split(B, S) for B, S, _ in lr.WGRAD_CASES + [lr.WGRAD_LARGE]}
    assert split[(1, 4)] == (1, 2, 1) and split[(32, 4)] == (1, 64, 1) and split[(33, 4)] == (1, 66, 1) and split[(512, 4)] == (1, 1024, 1)
    assert split[(513, 4)] == (2, 513, 2) and lr.conv11c_rows(513, 4) == 1026
    assert split[(1025, 4)] == (3, 684, 1) and lr.conv11c_rows(1025, 4) == 2050                          # the last block has one row
    assert split[(103, 12)] == (2, 515, 2) and split[(3, 36)] == (1, 102, 1)
    assert split[(1, 856)] == (1, 854, 1)
    assert all(nb <= 1024 and (nb - 1) * rpb + last == lr.conv11c_rows(B, S) and 1 <= last <= rpb for (B, S), (rpb, nb, last) in split.items())
    # the LDS switch at 3 S = 40 K
    assert 3 * 424 < 40 * 32 < 3 * 428 and lr.conv11c_wgrad_lds_floats(424, 32) == 1280 and lr.conv11c_wgrad_lds_floats(428, 32) == 1284
    assert 3 * 856 > 40 * 64 and lr.conv11c_wgrad_lds_floats(856, 64) == 2568 and lr.conv11c_wgrad_lds_floats(572, 64) == 2560
    assert lr.conv11c_wgrad_scratch_bytes(1025, 4, 64) == 684 * 10 * 64 * 4
    # the large case: 187 MB of dz in fp32, and integer data of its size stays exact (|x| <= 4, |dz| <= 8)
    B, S, K = lr.WGRAD_LARGE
    assert 186e6 < B * (S - 2) ** 2 * K * 4 < 188e6 and B * (S - 2) ** 2 * 32 > lr.EXACT_LIMIT          # the worst case would not be: the test asserts max(A)
    # stand-alone bias gradient: rows per case, blocks of 2048 rows, the slot loop
    M = [B * (H - 2) ** 2 for B, H in lr.BIAS_SHAPES]
    assert M == [1, 2023, 2048, 2052, 10082, 18432]
    assert [lr.bias_grad_blocks(m) for m in M] == [1, 1, 1, 2, 5, 9]                                     # the reduce's unroll by four: tails 1, 1, 1, 2, 1, 1
    assert [lr.bias_grad_blocks(m) % 4 for m in M] == [1, 1, 1, 2, 1, 1] and 9 // 4 == 2
    assert lr.bias_grad_slots(32) == (8, 32, 0) and lr.bias_grad_slots(64) == (16, 16, 0) and lr.bias_grad_slots(96) == (24, 10, 16)
    assert lr.bias_grad_slots(256) == (64, 4, 0) and lr.bias_grad_slots(1024) == (256, 1, 0)
    assert [4 * B * H * H for B, H, _, _ in lr.BIAS_UP_CASES] == [2048, 100]
    assert len(lr.FWD_CASES) == 22 and len(lr.WGRAD_CASES) == 18 and len(lr.DGRAD_CASES) == 13
