"""The argument checks of functions.py that sit behind the device check, so that only device tensors reach them: the exception's
type and its whole message, row by row, and which of two applicable refusals wins.  The rows have the shape of those of
tests/test_functions_errors_cpu.py, which holds everything a host tensor can reach.  Every row is refused in Python before any
launch of the library; the rows of negative and too large ids need the id range read back first.  The table's one launch is the
cell_sums that makes the sums the cell_hulls rows are given; the one-class refusal at the end sits behind a launch on [1,5,7].  The
refusals by status word (ids outside [0, n_max], bad image values) are held by the ops' own tests."""
import functools
import math

import numpy as np
import pytest
import torch

from gpu_support import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _names(dev):
    import functions as F
    h = torch.zeros(2, 5, 7, dtype=torch.int32)
    d = h.to(dev)
    neg, big = d.clone(), d.clone()
    neg[1, 2, 3] = -1
    big[0, 4, 6] = 1 << 24
    return dict(
        F=F, torch=torch, np=np, math=math,
        h=h, d=d, d2=d[0], d1=d[:1], dv=d[0, 0], de=d[:0], fd=d.float(), neg=neg, big=big,
        wide=torch.zeros(1, 32769, dtype=torch.int32, device=dev),                         # past MEASURE_EDGE
        keep=torch.ones(4, dtype=torch.bool, device=dev),
        good=F.cell_sums(d, n_max=3))                                                        # the one launch of this file's table


ROWS = [
    # weighted_map, label_cells: the shape, behind the device
    ('F.weighted_map(d2)', ValueError,
     'weighted_map takes labels [B,H,W], got (5, 7)'),
    ('F.weighted_map(de)', IndexError,
     'index 1 is out of bounds for dimension 0 with size 0'),
    ('F.label_cells(dv)', ValueError,
     'label_cells takes [H,W] or [B,H,W], got (7,)'),
    ('F.label_cells(de, connectivity=8)', ValueError,
     'label_cells: empty input (0, 5, 7)'),
    # cell_sums: the image, the edge limit, n_max, in that order
    ('F.cell_sums(d, n_max=True)', ValueError,
     'cell_sums: n_max must be None or an integer in [0, 2^24), got True'),
    ('F.cell_sums(d, n_max=-1)', ValueError,
     'cell_sums: n_max must be None or an integer in [0, 2^24), got -1'),
    ('F.cell_sums(d, n_max=1 << 24)', ValueError,
     'cell_sums: n_max must be None or an integer in [0, 2^24), got 16777216'),
    ('F.cell_sums(d2, n_max=1.5)', ValueError,
     'cell_sums: n_max must be None or an integer in [0, 2^24), got 1.5'),
    ('F.cell_sums(d, image=d1)', ValueError,
     "cell_sums: the image must be a tensor of the labels' shape (2, 5, 7), got (1, 5, 7)"),
    ('F.cell_sums(d, image=3)', ValueError,
     "cell_sums: the image must be a tensor of the labels' shape (2, 5, 7), got int"),
    ('F.cell_sums(d, image=d1, n_max=True)', ValueError,
     "cell_sums: the image must be a tensor of the labels' shape (2, 5, 7), got (1, 5, 7)"),
    ('F.cell_sums(d, image=h)', NotImplementedError,
     'cell_sums runs on the HIP device only (unet_cell_sums): move the input to the device first, e.g. with .cuda(); there is no CPU implementation'),
    ('F.cell_sums(d, image=h, n_max=True)', NotImplementedError,
     'cell_sums runs on the HIP device only (unet_cell_sums): move the input to the device first, e.g. with .cuda(); there is no CPU implementation'),
    ('F.cell_sums(wide)', ValueError,
     'cell_sums: H and W must be <= 32768, got 1 x 32769'),
    ('F.cell_sums(wide, n_max=True)', ValueError,
     'cell_sums: H and W must be <= 32768, got 1 x 32769'),
    ('F.cell_sums(wide, image=wide.cpu())', NotImplementedError,
     'cell_sums runs on the HIP device only (unet_cell_sums): move the input to the device first, e.g. with .cuda(); there is no CPU implementation'),
    ('F.cell_sums(wide, image=d)', ValueError,
     "cell_sums: the image must be a tensor of the labels' shape (1, 32769), got (2, 5, 7)"),
    ('F.cell_sums(neg)', ValueError,
     'cell_sums: negative ids (the smallest is -1)'),
    ('F.cell_sums(big, image=fd)', ValueError,
     'cell_sums: ids must be below 2^24, got up to 16777216'),
    ('F.cell_props(neg)', ValueError,
     'cell_sums: negative ids (the smallest is -1)'),
    # cell_hulls: the edge limit, then sums, then n_max against sums
    ('F.cell_hulls(wide)', ValueError,
     'cell_hulls: H and W must be <= 32768, got 1 x 32769'),
    ('F.cell_hulls(wide, good)', ValueError,
     'cell_hulls: H and W must be <= 32768, got 1 x 32769'),
    ('F.cell_hulls(d, n_max=True)', ValueError,
     'cell_sums: n_max must be None or an integer in [0, 2^24), got True'),
    ('F.cell_hulls(d, n_max=-1)', ValueError,
     'cell_sums: n_max must be None or an integer in [0, 2^24), got -1'),
    ('F.cell_hulls(neg)', ValueError,
     'cell_sums: negative ids (the smallest is -1)'),
    ('F.cell_hulls(d, good._replace(bbox=good.bbox.long()))', ValueError,
     'cell_hulls: sums must be the CellSums of cell_sums(labels) (bbox int32 [.., n_max+1, 4])'),
    ('F.cell_hulls(d, good._replace(bbox=good.bbox.cpu().numpy()))', ValueError,
     'cell_hulls: sums must be the CellSums of cell_sums(labels) (bbox int32 [.., n_max+1, 4])'),
    ('F.cell_hulls(d2, good)', ValueError,
     'cell_hulls: sums must be the CellSums of cell_sums(labels) (bbox int32 [.., n_max+1, 4])'),
    ('F.cell_hulls(d1, good)', ValueError,
     'cell_hulls: sums must be the CellSums of cell_sums(labels) (bbox int32 [.., n_max+1, 4])'),
    ('F.cell_hulls(d, good._replace(present=good.present[:, :2]))', ValueError,
     'cell_hulls: sums must be the CellSums of cell_sums(labels) (bbox int32 [.., n_max+1, 4])'),
    ('F.cell_hulls(d, good._replace(bbox=good.bbox[..., :3]), n_max=True)', ValueError,
     'cell_hulls: sums must be the CellSums of cell_sums(labels) (bbox int32 [.., n_max+1, 4])'),
    ('F.cell_hulls(d, good._replace(bbox=good.bbox.cpu(), present=good.present.cpu()))', NotImplementedError,
     'cell_hulls runs on the HIP device only (unet_cell_hulls): move the input to the device first, e.g. with .cuda(); there is no CPU implementation'),
    ('F.cell_hulls(d, good._replace(bbox=good.bbox.cpu(), present=good.present.cpu()), n_max=4)', NotImplementedError,
     'cell_hulls runs on the HIP device only (unet_cell_hulls): move the input to the device first, e.g. with .cuda(); there is no CPU implementation'),
    ('F.cell_hulls(d, good, n_max=4)', ValueError,
     'cell_hulls: n_max = 4 does not match the 4 rows of sums'),
    ('F.cell_hulls(d, good, n_max=True)', ValueError,
     'cell_hulls: n_max = True does not match the 4 rows of sums'),
    ('F.cell_hulls(d, good, n_max=3.0)', ValueError,
     'cell_hulls: n_max = 3.0 does not match the 4 rows of sums'),
    # select_cells: keep, its device, its batch, the edge limit, its length
    ('F.select_cells(d, None)', ValueError,
     'select_cells: keep must be a bool tensor [n_max+1] or [B, n_max+1]'),
    ('F.select_cells(d, keep.int())', ValueError,
     'select_cells: keep must be a bool tensor [n_max+1] or [B, n_max+1]'),
    ('F.select_cells(d, keep[None, None])', ValueError,
     'select_cells: keep must be a bool tensor [n_max+1] or [B, n_max+1]'),
    ('F.select_cells(d, keep[:0])', ValueError,
     'select_cells: keep must be a bool tensor [n_max+1] or [B, n_max+1]'),
    ('F.select_cells(wide, None)', ValueError,
     'select_cells: keep must be a bool tensor [n_max+1] or [B, n_max+1]'),
    ('F.select_cells(d, keep.cpu())', NotImplementedError,
     'select_cells runs on the HIP device only (unet_remap_labels): move the input to the device first, e.g. with .cuda(); there is no CPU implementation'),
    ('F.select_cells(d, keep.expand(3, 4))', ValueError,
     'select_cells: keep holds 3 images, the labels 2'),
    ('F.select_cells(wide, keep.expand(3, 4))', ValueError,
     'select_cells: keep holds 3 images, the labels 1'),
    ('F.select_cells(wide, keep)', ValueError,
     'select_cells: H and W must be <= 32768, got 1 x 32769'),
    ('F.select_cells(wide, keep[:1].expand((1 << 24) + 1))', ValueError,
     'select_cells: H and W must be <= 32768, got 1 x 32769'),
    ('F.select_cells(d2, keep[:1].expand((1 << 24) + 1), renumber=True)', ValueError,
     'select_cells: ids must be below 2^24, keep has 16777217 entries'),
    # cell_neighbours
    ('F.cell_neighbours(wide)', ValueError,
     'cell_neighbours: H and W must be <= 32768, got 1 x 32769'),
    ('F.cell_neighbours(neg)', ValueError,
     'cell_neighbours: negative ids (the smallest is -1)'),
    ('F.cell_neighbours(big)', ValueError,
     'cell_neighbours: ids must be below 2^24, got up to 16777216'),
    # grow_cells: max_distance before the id range; rand_scores hands grow on
    ('F.grow_cells(d, -1)', ValueError,
     'grow_cells: max_distance must be None or a number >= 0, got -1'),
    ('F.grow_cells(d2, math.nan)', ValueError,
     'grow_cells: max_distance must be None or a number >= 0, got nan'),
    ('F.grow_cells(neg, -0.5)', ValueError,
     'grow_cells: max_distance must be None or a number >= 0, got -0.5'),
    ("F.grow_cells(d, 'x')", TypeError,
     "'>=' not supported between instances of 'str' and 'int'"),
    ('F.grow_cells(neg, math.inf)', ValueError,
     'grow_cells: negative ids (the smallest is -1)'),
    ('F.grow_cells(big)', ValueError,
     'grow_cells: ids must be below 2^24, got up to 16777216'),
    ('F.rand_scores(d, d, grow=-1)', ValueError,
     'grow_cells: max_distance must be None or a number >= 0, got -1'),
    # the id range of the other ops, and a second tensor left on the host
    ('F.seg_measure(neg, d)', ValueError,
     'seg_measure: negative ids (the smallest is -1)'),
    ('F.seg_measure(d, big)', ValueError,
     'seg_measure: ids must be below 2^24, got up to 16777216'),
    ('F.seg_measure(d, h)', NotImplementedError,
     'seg_measure runs on the HIP device only (unet_instance_overlap): move the input to the device first, e.g. with .cuda(); there is no CPU implementation'),
    ('F.pair_table(big, d)', ValueError,
     'pair_table: ids must be below 2^24, got up to 16777216'),
    ('F.link_frames(neg)', ValueError,
     'link_frames: negative ids (the smallest is -1)'),
    ('F.track_cells(big, reach=2)', ValueError,
     'track_cells: ids must be below 2^24, got up to 16777216'),
    ('F.split_cells(neg, d)', ValueError,
     'split_cells: negative ids (the smallest is -1)'),
    ('F.split_cells(d, h)', NotImplementedError,
     'split_cells runs on the HIP device only (unet_geodesic_init): move the input to the device first, e.g. with .cuda(); there is no CPU implementation'),
    ('F.watershed(big, d)', ValueError,
     'watershed: ids must be below 2^24, got up to 16777216'),
    ('F.watershed(d, d, mask=h)', NotImplementedError,
     'watershed runs on the HIP device only (unet_flood_init): move the input to the device first, e.g. with .cuda(); there is no CPU implementation'),
    ('F.warp_labels(d, d, mask=h)', NotImplementedError,
     'warp_labels runs on the HIP device only (unet_warp_init): move the input to the device first, e.g. with .cuda(); there is no CPU implementation'),
    ('F.reconstruct(d, h)', NotImplementedError,
     'reconstruct runs on the HIP device only (unet_reconstruct_init): move the input to the device first, e.g. with .cuda(); there is no CPU implementation'),
    ('F.surface_sums(d, h)', NotImplementedError,
     'surface_sums runs on the HIP device only (unet_surface_sums): move the input to the device first, e.g. with .cuda(); there is no CPU implementation'),
    # watershed: levels against the image's dtype, on the device as on the host
    ('F.watershed(d, d, levels=4)', ValueError,
     'watershed: levels is for float images; an integer image is read as it is, got levels=4 for torch.int32'),
    ('F.watershed(d, d.bool(), levels=4, max_level=-1)', ValueError,
     'watershed: levels is for float images; an integer image is read as it is, got levels=4 for torch.bool'),
    ('F.watershed(d, fd)', ValueError,
     'watershed: a float image needs levels, an int in [1, 65536], got None'),
    ('F.watershed(neg, fd, levels=65537)', ValueError,
     'watershed: a float image needs levels, an int in [1, 65536], got 65537'),
    ('F.watershed(neg, d, max_level=-1)', ValueError,
     'watershed: max_level must be None or a number >= 0, got -1'),
    ('F.split_cells(neg, d, max_steps=-1)', ValueError,
     'split_cells: max_steps must be None or a number >= 0, got -1'),
]


@pytest.mark.parametrize("call, exc, message", ROWS, ids=[r[0] for r in ROWS])
def test_the_refusal(dev, call, exc, message):
    with pytest.raises(exc) as caught:
        eval(call, dict(_names(dev)))
    assert type(caught.value) is exc and str(caught.value) == message


def test_a_one_class_image(dev):
    """The one refusal that weighted_map and class_balance share: raised behind their launch, on [1,5,7]."""
    import functions as F
    zeros = torch.zeros(1, 5, 7, dtype=torch.int64, device=dev)
    for op, labels in ((F.weighted_map, zeros), (F.weighted_map, zeros + 1), (F.class_balance, zeros), (F.class_balance, zeros + 1)):
        with pytest.raises(IndexError) as caught:
            op(labels)
        assert type(caught.value) is IndexError and str(caught.value) == "index 1 is out of bounds for dimension 0 with size 1"
