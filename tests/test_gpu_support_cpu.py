"""tests/gpu_support.py's data helpers checked on the CPU (guarded.Arena works on CPU tensors): what the GPU test modules
share must hand each of them the bytes, addresses and error figures it expects."""
import ctypes

import numpy as np
import torch

import guarded as gd
import gpu_support as gs


def through(view, strides, shape):
    """The fp32 elements a kernel reads through `view` with the three element strides of strided() and a unit column stride."""
    B, K, H, W = shape
    sB, sK, sH = strides
    span = (B - 1) * sB + (K - 1) * sK + (H - 1) * sH + W
    flat = np.ctypeslib.as_array(ctypes.cast(view, ctypes.POINTER(ctypes.c_float)), shape=(span,))
    return np.lib.stride_tricks.as_strided(flat, shape, (4 * sB, 4 * sK, 4 * sH, 4))


def test_strided_is_the_crop_inside_nan():
    x = np.random.RandomState(0).randn(2, 3, 5, 7).astype(np.float32)
    for margins, (top, left, bottom, right) in (({}, (2, 3, 2, 3)), (dict(top=1, left=4, bottom=0, right=2), (1, 4, 0, 2))):
        mem = gd.Arena("cpu")
        view, strides = gs.strided(mem, x, **margins)
        big = mem.bufs[-1].view
        assert big.shape == (2, 3, 5 + top + bottom, 7 + left + right) and big.dtype == torch.float32
        assert view.value == mem.address(big) + (top * big.shape[3] + left) * 4
        assert np.array_equal(through(view, strides, x.shape), x)
        outside = torch.ones(big.shape, dtype=torch.bool)
        outside[:, :, top:top + 5, left:left + 7] = False
        assert bool(torch.isnan(big[outside]).all()) and int(outside.sum()) == big.numel() - x.size
        mem.check()


def test_strided_two_class_offset_and_strides():
    """K = 2 at the default margins: (2 (W + 6) + 3) * 4 bytes into the tensor, strides 2 (H + 4)(W + 6), (H + 4)(W + 6), W + 6."""
    mem = gd.Arena("cpu")
    x = np.zeros((3, 2, 13, 43), np.float32)                        # H + 4 = 17, W + 6 = 49
    view, strides = gs.strided(mem, x)
    assert view.value - mem.address(mem.bufs[-1].view) == 404       # (2 * 49 + 3) * 4
    assert strides == (1666, 833, 49)


def test_nerr_paths_agree():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(4, 5, generator=g, dtype=torch.float64)
    r = a + 1e-6 * torch.randn(4, 5, generator=g, dtype=torch.float64)
    want = ((a - r).abs().max() / r.abs().max()).item()
    e = gs.nerr(a, r)
    assert type(e) is float and e == want
    assert gs.nerr(a.numpy(), r.numpy()) == want and gs.nerr(a, r.numpy()) == want and gs.nerr(a.tolist(), r) == want
    assert gs.nerr(a.float(), r) == gs.nerr(a.float().numpy(), r.numpy())       # fp32 against fp64: widened, not narrowed
    assert gs.nerr(a.clone().requires_grad_(True), r) == want
    assert gs.nerr(a.to(torch.bfloat16), r) == gs.nerr(a.to(torch.bfloat16).double(), r)


def test_nerr_of_an_all_zero_reference():
    z = np.zeros(6)
    assert gs.nerr(z, z) == 0.0 and gs.nerr(torch.zeros(6), torch.zeros(6)) == 0.0
    assert gs.nerr(z + 1e-3, z) == 1e-3 / 1e-300                    # the floor, not a division by zero
    assert np.isnan(gs.nerr(np.float64([1.0, np.nan]), np.ones(2)))


def test_rnd_forms():
    for fp32 in (False, True):
        a = gs.rnd(3, 4, 5, seed=7, scale=0.05, fp32=fp32)
        assert a.shape == (3, 4, 5) and a.dtype == torch.float64
        assert torch.equal(a, gs.rnd(3, 4, 5, seed=7, scale=0.05, fp32=fp32))
        assert not torch.equal(a, gs.rnd(3, 4, 5, seed=8, scale=0.05, fp32=fp32))
    plain, rounded = gs.rnd(3, 4, 5, seed=7), gs.rnd(3, 4, 5, seed=7, fp32=True)
    assert torch.equal(gs.rnd(3, 4, 5, seed=7, fp32=False), plain)
    assert torch.equal(rounded.float().double(), rounded) and not torch.equal(plain.float().double(), plain)
    assert torch.equal(rounded, plain.float().double()) and not torch.equal(rounded, plain)
    assert torch.equal(gs.rnd(6), gs.rnd(6, seed=0, scale=1.0))


def test_still_poison():
    mem = gd.Arena("cpu")
    for t in (mem.out((3, 5), torch.float32), mem.out(7, torch.int64), mem.scratch(33)):
        assert gs.still_poison(t)
        t.view(torch.uint8).view(-1)[-1] = 0
        assert not gs.still_poison(t)
    x = mem.inp(torch.arange(6.0))
    assert not gs.still_poison(x)
    mem.check()


def test_put_is_a_guarded_copy():
    mem = gd.Arena("cpu")
    a = np.arange(24, dtype=np.int32).reshape(4, 6)[:, ::2]          # not contiguous
    t = gs.put(mem, a, "a")
    assert t.dtype == torch.int32 and t.is_contiguous() and np.array_equal(t.numpy(), a)
    mem.check()


def test_image():
    a = gs.image(5, 2, 19, 31, blobs=12)
    assert a.shape == (2, 19, 31) and a.dtype == np.float32 and np.isfinite(a).all() and a.min() >= 0
    assert np.array_equal(a, gs.image(5, 2, 19, 31, blobs=12))
    assert not np.array_equal(a, gs.image(6, 2, 19, 31, blobs=12))
    assert not np.array_equal(a, gs.image(5, 2, 19, 31, blobs=8))
    assert not np.array_equal(a[0], a[1])
