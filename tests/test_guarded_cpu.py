"""tests/guarded.py checked on the CPU: a correct fake "kernel" passes, and each deliberately broken one is caught by the
assertion meant for it, with a message that names the buffer.  The fakes are numpy / torch code working through raw
addresses (ctypes), the way the library sees the buffers: base pointer + extent, nothing else."""
import ctypes

import numpy as np
import pytest
import torch

import guarded as gd

B, H, W, C = 2, 5, 6, 8


def raw(arena, t, before=0, after=0, dtype=np.float32):
    """numpy window on the memory of an arena buffer, widened by `before` / `after` ELEMENTS of `dtype` on either side -
    what a kernel with a wrong bound would address."""
    es = np.dtype(dtype).itemsize
    n = t.numel() * t.element_size() // es
    addr = arena.address(t) - before * es
    return np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(before + n + after,))


def scale_rows(arena, x, y, sc, rows=H, x_over=0, y_first=0, y_extra=0, sc_bytes=None, clear=True):
    """The fake op: y[b,h,w,c] = 2 x[b,h,w,c] + sum_c x[b,h,w,:] (the row sum goes through scratch: one fp32 per pixel,
    accumulated).  The keyword arguments are the bugs."""
    xin = raw(arena, x, after=x_over)
    n_pix = B * H * W
    s = raw(arena, sc, dtype=np.uint8, after=0 if sc_bytes is None else sc_bytes - sc.numel())
    acc = s[:4 * n_pix].view(np.float32)
    if clear:
        acc[:] = 0.0
    xs = xin[x_over:x_over + n_pix * C].reshape(n_pix, C)        # x_over > 0: the window starts x_over elements late and runs past the end
    acc += xs.sum(1)
    if sc_bytes is not None:
        s[sc_bytes - 1] = 1                                      # a flag byte one past what was asked for
    res = (2.0 * xs + acc[:, None]).reshape(B, H, W, C)
    yo = raw(arena, y, before=-y_first if y_first < 0 else 0, after=y_extra)
    if y_first < 0:
        yo[0] = 1.0                                              # one element before the tensor
    v = yo[(1 if y_first < 0 else 0):][:B * H * W * C].reshape(B, H, W, C)
    v[:, :rows] = res[:, :rows]
    if y_extra:
        yo[-1] = 1.0                                             # one element past it


def setup():
    A = gd.Arena("cpu")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, H, W, C, generator=g)
    xd = A.inp(x, "x")
    y = A.out((B, H, W, C), torch.float32, "y")
    sc = A.scratch(4 * B * H * W, "sums")
    ref = 2.0 * x.double() + x.double().sum(-1, keepdim=True)
    return A, x, xd, y, sc, ref


def test_correct_kernel_passes():
    A, x, xd, y, sc, ref = setup()
    scale_rows(A, xd, y, sc)
    A.assert_written(y)
    A.check()
    A.verify(y)
    assert not torch.isnan(y).any() and (y.double() - ref).abs().max() < 1e-5


def test_views_are_poisoned_aligned_and_exact():
    A = gd.Arena("cpu")
    # a multiple of 256, at least 64 KiB, and at least one workgroup's largest store in one pass: the output tiles (256 x 64,
    # 128 x 128 fp32), the 3x3 weight-gradient slab of one workgroup (9 taps x 64 x 64 fp32) and the Winograd one (+ 64 bias partials)
    assert gd.G % 256 == 0 and gd.G >= 64 * 1024 and gd.G >= 256 * 64 * 4 and gd.G >= 128 * 128 * 4
    assert gd.G >= 9 * 64 * 64 * 4 and gd.G >= (9 * 64 * 64 + 64) * 4
    for shape, dt in (((3, 7, 5, 2), torch.float32), ((1, 3, 3, 64), torch.bfloat16), ((2, 9, 9), torch.int64), ((5,), torch.float32)):
        t = A.out(shape, dt)
        assert tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous()
        assert A.address(t) % 256 == 0 and t.data_ptr() == A.address(t)
        b = A._find(t)
        assert b.start >= gd.G and b.raw.numel() - (b.start + b.nbytes) >= gd.G
        assert bool((b.raw == 0xFF).all())
        if dt.is_floating_point:
            assert bool(torch.isnan(t).all())
        else:
            assert bool((t == -1).all())
    s = A.scratch(100)
    assert s.numel() == 100 and s.dtype == torch.uint8 and A.address(s) % 256 == 0
    x = A.inp(torch.arange(12.0).reshape(3, 4))
    assert torch.equal(x, torch.arange(12.0).reshape(3, 4)) and A.address(x) % 256 == 0
    A.check()
    with pytest.raises(AssertionError):
        gd.Arena("cpu", guard=64 * 1024)         # below G: less than a 3x3 weight-gradient slab
    with pytest.raises(AssertionError):
        gd.Arena("cpu", guard=gd.G + 100)        # not a multiple of 256


def test_scratch_of_zero_bytes_is_exact_and_guarded():
    A = gd.Arena("cpu")
    s = A.scratch(0, "empty")
    assert s.numel() == 0
    assert A.ptr(s).value == A.address(s) and A.address(s) % 256 == 0 and A.address(s) != 0
    A.check()
    A.assert_written(s)
    raw(A, s, dtype=np.uint8, after=1)[0] = 0    # a kernel that was promised 256 bytes
    with pytest.raises(AssertionError, match=r"AFTER empty \(0,\).*first at offset 0 = 0 past its end"):
        A.check()


def test_last_row_unwritten_is_caught_by_assert_written():
    A, x, xd, y, sc, ref = setup()
    scale_rows(A, xd, y, sc, rows=H - 1)
    A.check()                                    # nothing outside was touched
    with pytest.raises(AssertionError, match=r"y \(2, 5, 6, 8\): 96 of 480 elements still hold poison.*first at \(n, h, w, c\) = \(0, 4, 0, 0\), "
                                             r"last at \(1, 4, 5, 7\)"):
        A.assert_written(y)


def test_write_before_the_tensor_is_caught_by_check():
    A, x, xd, y, sc, ref = setup()
    scale_rows(A, xd, y, sc, y_first=-1)
    A.assert_written(y)
    with pytest.raises(AssertionError, match=r"guard BEFORE y \(2, 5, 6, 8\) damaged: \d bytes, first at offset -[1-4] "):
        A.check()


def test_write_past_the_tensor_is_caught_by_check():
    A, x, xd, y, sc, ref = setup()
    scale_rows(A, xd, y, sc, y_extra=1)
    A.assert_written(y)
    with pytest.raises(AssertionError, match=r"guard AFTER y \(2, 5, 6, 8\) damaged: \d bytes, first at offset 19[2-9]\d = [0-3] past its end"):
        A.check()


def test_scratch_overrun_by_one_byte_is_caught_by_check():
    A, x, xd, y, sc, ref = setup()
    scale_rows(A, xd, y, sc, sc_bytes=sc.numel() + 1)
    A.assert_written(y)
    with pytest.raises(AssertionError, match=r"guard AFTER sums \(240,\) damaged: 1 bytes, first at offset 240 = 0 past its end"):
        A.check()


def test_result_from_beyond_an_input_turns_nan():
    A, x, xd, y, sc, ref = setup()
    scale_rows(A, xd, y, sc, x_over=1)           # the last stored pixel includes one element read past x
    A.check()                                    # no guard damaged: only the values tell
    # the NaN that was read keeps the poison's payload through the arithmetic: assert_written names the buffer and the pixel
    with pytest.raises(AssertionError, match=r"y \(2, 5, 6, 8\): 8 of 480 elements still hold poison.*first at \(n, h, w, c\) = \(1, 4, 5, 0\)"):
        A.assert_written(y)
    # the same bug next to an unguarded input would read whatever lies there; the guarded copy makes it NaN for certain
    assert bool(torch.isnan(y[-1, -1, -1]).all()) and not torch.isnan(y[0]).any()


def test_accumulating_into_uncleared_scratch_turns_nan():
    A, x, xd, y, sc, ref = setup()
    scale_rows(A, xd, y, sc, clear=False)        # a slab assumed to be zero
    A.check()
    assert bool(torch.isnan(y).all())
    with pytest.raises(AssertionError, match=r"y \(2, 5, 6, 8\): 480 of 480 elements still hold poison"):
        A.assert_written(y)
    # on zeroed memory - what a fresh process mostly finds - the same bug passes: the case the poison exists for
    sc.zero_()
    scale_rows(A, xd, y, sc, clear=False)
    A.verify(y)
    assert (y.double() - ref).abs().max() < 1e-5


@pytest.mark.parametrize("chunk", [4, 20, 100, 1919, 1920, 4096])
def test_assert_written_in_pieces_means_the_same(chunk):
    """assert_written looks at a buffer in pieces of Arena.chunk bytes (the tensors of tests/test_large_tensors_gpu.py are
    gigabytes): whatever the piece size - one element, pieces that end inside the tensor's last row, exactly the tensor, more
    than it - a fully written tensor passes and a gap is reported with the same count, first and last element."""
    A = gd.Arena("cpu", chunk=chunk)
    y = A.out((B, H, W, C), torch.float32, "y")
    assert y.numel() * 4 == 1920
    y.zero_()
    A.verify(y)
    flat = raw(A, y).view(np.uint32)
    flat[[7, 8, 250, 479]] = 0xFFFFFFFF
    with pytest.raises(AssertionError, match=r"y \(2, 5, 6, 8\): 4 of 480 elements still hold poison.*first at \(n, h, w, c\) = \(0, 0, 0, 7\), "
                                             r"last at \(1, 4, 5, 7\)"):
        A.assert_written(y)
    h = A.out((3, 5), torch.bfloat16, "h")      # two-byte elements: a piece never cuts one in two
    h.zero_()
    raw(A, h, dtype=np.uint16)[14] = 0xFFFF
    with pytest.raises(AssertionError, match=r"h \(3, 5\): 1 of 15 elements still hold poison.*first at index \(2, 4\), last at \(2, 4\)"):
        A.assert_written(h)
