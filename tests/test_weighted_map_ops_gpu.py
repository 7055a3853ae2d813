"""unet_weighted_map (wmap.hip: labelling, column pass, row pass) through the C ABI on guarded.Arena buffers (tests/guarded.py):
labels as a guarded input, weights, counts and n_objects as poisoned outputs, the three-plane scratch exact to the byte, so
the column pass's labels, which reuse the dead parent plane, run with poison all around.  Reference:
weighted_map_ref.weighted_map_batch(lab, w0, sig2) with the assertions of check_against_restatement: counts and component
numbers exact, cells exactly 1, background with nothing within the reach R = ceil(sqrt(208 sig2)) exactly w_c, elsewhere
1e-5 max(1, |w_ref|).  Shapes one past and exactly on the 32-pixel labelling tile, the 64-wide column block and the 256-pixel
row block at the default parameters; reaches of 21, 73, 204 and 1020 on images small enough for the restatement to be exact
at any reach.  The label batches are weighted_map_ref's, proved well-posed by tests/test_weighted_map_cpu.py."""
import numpy as np
import pytest
import torch

import guarded as gd
import weighted_map_ref as ref
from gpu_support import hip, rejected

pytestmark = pytest.mark.gpu


class Call:
    def __init__(self, hip, lab, w0, sig2, dtype_code=None):
        L = hip.lib()
        B, H, W = lab.shape
        self.mem = mem = gd.Arena()
        ld = mem.inp(torch.from_numpy(np.ascontiguousarray(lab)), "labels")
        self.w = mem.out((B, H, W), torch.float32, "weights")
        self.counts = mem.out((B,), torch.int64, "counts")
        self.nobj = mem.out((B,), torch.int32, "n_objects")
        self.nbytes = L.unet_weighted_map_scratch_bytes(B, H, W)
        self.scratch = mem.scratch(self.nbytes, "weighted_map scratch")
        code = (0 if lab.dtype == np.int64 else 1) if dtype_code is None else dtype_code
        self.rc = L.unet_weighted_map(mem.ptr(ld), code, B, H, W, w0, sig2, mem.ptr(self.w), mem.ptr(self.counts), mem.ptr(self.nobj),
                                      mem.ptr(self.scratch), hip.stream())
        torch.cuda.synchronize()

    def check(self, hip, lab, w0, sig2):
        hip.check(self.rc, "unet_weighted_map")
        self.mem.verify(self.w, self.counts, self.nobj)
        assert self.nbytes == 3 * (-(-lab.size * 4 // 256) * 256)           # three int planes, each rounded up to 256 bytes
        # Where the class term is 0 (int64 labels with fewer cells than background) the border term is the whole weight: it is
        # present wherever the reference's is at least 2^-100, far above where fp32 loses it (a shorter reach would drop it)
        w_ref, _ = ref.weighted_map_batch(lab, w0, sig2)
        seen = ref.visible_border(lab, w_ref)
        assert (self.w.cpu().numpy()[seen] > 0).all()
        ref.check_against_restatement(lab, self.w.cpu().numpy(), self.nobj.cpu().numpy(), w0, sig2, ref.reach_of(sig2),
                                      counts=self.counts.cpu().numpy())


@pytest.mark.parametrize("dtype", [np.int64, np.float32], ids=["int64", "float32"])
@pytest.mark.parametrize("B,H,W", ref.THRESHOLD_SHAPES)
def test_weighted_map_threshold_shapes(hip, B, H, W, dtype):
    lab = ref.threshold_labels(B, H, W, dtype)
    Call(hip, lab, 20.0, 25.0).check(hip, lab, 20, 25)


@pytest.mark.parametrize("w0,sig2", ref.PARAMS)
@pytest.mark.parametrize("name", ref.PARAM_CASES)
def test_weighted_map_other_parameters(hip, name, w0, sig2):
    """Reaches of 21, 73, 204 and 1020 pixels: the LDS size and both loop bounds of the column and row passes.  The images are
    at most 74 x 74, where the restatement is exact whatever the reach; int64 and float32 labels alternate."""
    lab = ref.param_labels(name, ref.param_dtype(name, w0, sig2))
    assert max(lab.shape[1:]) <= ref.REACH + 1
    Call(hip, lab, float(w0), float(sig2)).check(hip, lab, w0, sig2)


@pytest.mark.parametrize("sig2,code", [(0.0, 0), (6000.0, 0), (25.0, 2)], ids=["sig2=0", "sig2=6000", "labels_dtype=2"])
def test_weighted_map_rejects_without_touching(hip, sig2, code):
    """sig2 = 0, a reach above 1024 (sig2 = 6000: 1118) and an unknown label type return non-zero; no buffer is touched."""
    lab = ref.param_labels("blobs+far", np.int64)
    c = Call(hip, lab, 20.0, sig2, dtype_code=code)
    rejected(hip, c.rc, c.mem, c.w, c.counts, c.nobj, c.scratch)
