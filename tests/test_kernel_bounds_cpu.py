"""The element-level criteria of tests/kernel_bounds.py (used by the bf16x3 and bf16 GPU tests) must discriminate: fed with
numpy emulations on the CPU - contractions of the same K range as the GPU cases, fp32 accumulation emulated in order -
every correct emulation passes and every subtly broken one fails.  No GPU needed."""
import math

import numpy as np
import pytest

import kernel_bounds as kb

KS = [288, 576, 1152, 4608]            # 9 x (32, 64, 128, 512) input channels: the 3x3 contractions of the GPU cases


def fp32_sum(terms):
    """Sequential fp32 accumulation along the last axis (np.cumsum keeps the dtype and the order)."""
    return np.cumsum(np.asarray(terms, dtype=np.float32), axis=-1, dtype=np.float32)[..., -1].astype(np.float64)


def operands(K, seed, n=48, m=24):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, 1, K)).astype(np.float32).astype(np.float64)
    w = (g.standard_normal((1, m, K)) * 0.05).astype(np.float32).astype(np.float64)    # fp32 master weights: not bf16
    b = g.standard_normal((1, m)).astype(np.float32).astype(np.float64)
    return x, w, b


# ---- bf16 outputs (mode 2) -----------------------------------------------------------------------------------------------
def bf16_case(K, seed, packer=kb.rne_bf16, out=kb.rne_bf16, split_at=None):
    """bf16 activations, fp32 weights packed to bf16 by `packer`, fp32 accumulation, fp32 bias, ReLU, output by `out`.
    split_at: the sum is formed in two launches whose first partial sum is stored in bf16 (a second rounding)."""
    x, w, b = operands(K, seed)
    x = kb.rne_bf16(x)
    p = x * packer(w)                                   # exact in fp32 (8 x 8 significant bits)
    if split_at is None:
        acc = fp32_sum(np.concatenate([p, np.broadcast_to(b[..., None], p.shape[:2] + (1,))], -1))
    else:
        part = out(fp32_sum(p[..., :split_at]) + b)
        acc = fp32_sum(np.concatenate([part[..., None], p[..., split_at:]], -1))
    y = out(np.maximum(acc.astype(np.float32).astype(np.float64), 0.0))
    wr = kb.rne_bf16(w)                                 # the reference: w.to(torch.bfloat16) is RNE
    z = (x * wr).sum(-1) + b
    A = (np.abs(x) * np.abs(wr)).sum(-1) + np.abs(b)
    return y, z, kb.acc_slack(A, K + 1)


@pytest.mark.parametrize("K", KS)
def test_rne_output_emulation_passes(K):
    y, z, eps = bf16_case(K, 1)
    st = kb.check_rne(y, z, eps, relu=True)                 # (and >= a quarter of the outputs are decidable)
    assert st["relu_zeros"] > 0


@pytest.mark.parametrize("K", KS)
def test_truncating_output_conversion_fails(K):
    y, z, eps = bf16_case(K, 2, out=kb.trunc_bf16)
    with pytest.raises(AssertionError, match="not RNE_bf16|beyond one rounding"):
        kb.check_rne(y, z, eps, relu=True)


@pytest.mark.parametrize("K", KS)
def test_double_rounding_of_a_split_partial_sum_fails(K):
    """The two-launch split forward with the first partial sum stored in bf16 (what net.hip keeps off in mode 2)."""
    y, z, eps = bf16_case(K, 3, split_at=K // 2)
    with pytest.raises(AssertionError):
        kb.check_rne(y, z, eps, relu=True)


@pytest.mark.parametrize("K", KS)
def test_truncating_weight_packer_fails(K):
    y, z, eps = bf16_case(K, 4, packer=kb.trunc_bf16)
    with pytest.raises(AssertionError):
        kb.check_rne(y, z, eps, relu=True)


def test_rne_bf16_is_exact_and_matches_torch_on_fp32_values():
    import torch
    g = np.random.default_rng(5)
    v = g.standard_normal(100000).astype(np.float32)
    v[:4] = [1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, -(1.0 + 2 ** -8), 2.0 ** -8 + 2 ** -16]      # ties: to even
    ref = torch.from_numpy(v).to(torch.bfloat16).double().numpy()
    assert np.array_equal(kb.rne_bf16(v.astype(np.float64)), ref)
    assert kb.rne_bf16(np.array([1.0 + 2 ** -8]))[0] == 1.0 and kb.rne_bf16(np.array([1.0 + 3 * 2 ** -8]))[0] == 1.0 + 2 ** -6
    # midpoint distance: zero on a midpoint, half an ulp on a bf16 number, and the finer spacing just below a power of two
    assert kb.midpoint_distance(np.array([1.0 + 2 ** -8]))[0] == 0.0
    assert kb.midpoint_distance(np.array([1.5]))[0] == 2 ** -8
    assert kb.midpoint_distance(np.array([1.0]))[0] == 2 ** -9


# ---- bf16x3 (mode 1) -----------------------------------------------------------------------------------------------------
def bf16x3_case(K, seed, lo_round=kb.rne_bf16, drop_cross=False, probe=False):
    x, w, _ = operands(K, seed)
    if probe:
        x = kb.split_probe(x.shape, seed)
        w = np.abs(kb.rne_bf16(w)) + 2.0 ** -10             # positive, bf16-exact weights: lo_w = 0
        w = kb.rne_bf16(w)
    xh, xl = kb.split3(x, lo_round)
    wh, wl = kb.split3(w, lo_round)
    terms = [xh * wh, xh * wl, np.zeros_like(x * w) if drop_cross else xl * wh]
    y = fp32_sum(np.stack(terms, -1).reshape(terms[0].shape[:-1] + (-1,)))
    z = (x * w).sum(-1)
    A = (np.abs(x) * np.abs(w)).sum(-1)
    rh, rl = kb.split3(x)
    qh, ql = kb.split3(w)
    z_split = (rh * qh + rh * ql + rl * qh).sum(-1)
    return y, z, A, z_split


@pytest.mark.parametrize("K", KS)
def test_bf16x3_emulation_passes(K):
    y, z, A, _ = bf16x3_case(K, 6)
    st = kb.check_bf16x3(y, z, A, K)
    assert st["worst_rel"] > 0                                      # not exact: the bound is exercised
    y, z, A, zs = bf16x3_case(K, 7, probe=True)
    kb.check_bf16x3(y, z, A, K)
    assert abs(kb.split_bias(y, zs, A)) <= kb.SPLIT_BIAS_TOL


@pytest.mark.parametrize("K", KS)
def test_bf16x3_with_a_cross_term_dropped_fails(K):
    y, z, A, _ = bf16x3_case(K, 8, drop_cross=True)
    with pytest.raises(AssertionError, match="beyond its bound"):
        kb.check_bf16x3(y, z, A, K)


@pytest.mark.parametrize("K", KS)
def test_bf16x3_with_a_truncated_lo_fails(K):
    """A truncating lo conversion hides under C_SPLIT on random operands (its extra error has a random sign); on the split
    probe every product loses 4 x 2^-18 the same way, and the mean bias shows it."""
    y, z, A, zs = bf16x3_case(K, 9, lo_round=kb.trunc_bf16, probe=True)
    kb.check_bf16x3(y, z, A, K)                                        # inside the magnitude bound ...
    assert abs(kb.split_bias(y, zs, A)) > 2 * kb.SPLIT_BIAS_TOL         # ... but far outside the bias tolerance


def test_bound_constants():
    # the derivation in kernel_bounds: lo*lo, r_a b and a r_b, to first order 2^-16 + 2 x 2^-17
    assert kb.C_SPLIT >= (2 ** -8 * (1 + 2 ** -8)) ** 2 + 2 ** -17 + 2 ** -17 * (1 + 2 ** -17)
    assert kb.LAM_FAIL < 1e-13
    assert math.isclose(float(kb.acc_slack(1.0, 576)), 8 * 24 * 2.0 ** -24)
