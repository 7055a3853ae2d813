"""The exact image ops on the device held to their own answers (tests/metamorphic.py): an op on a view, a shifted placement, a batch
or a renaming of its input must give the transported answer of the op on the input itself, bit for bit.  There is no reference in
this file: tests/test_metamorphic_cpu.py proves on the *_ref.py restatements that every relation used here belongs to the op's
definition.  So the time is launches and small copies, and the scenes can sit on every seam of the kernels' decompositions.

The ops are reached through the public wrappers (functions.*, data.*) on the current stream; poisoned buffers, guards and raw
pointers stay the business of the per-op files (test_<op>_gpu.py), and none is handed to the library here.

  D   all eight views at (1, 65), (33, 130), (67, 129), (64, 64) and (3, 5), where a 64-lane wave spans several rows, and of the
      scenes the per-op tests already make (serpentine, busy, cells, shifted cells, ties, speckle: metamorphic.reused_scenes)
  T   the composed 41 x 45 scene at the placements of metamorphic.placements in a 131 x 197 canvas, and a 3 x 40 strip in 3 x 300
  B   an empty, a full and an ordinary image in three orders
  R   order-preserving renamings (up to 2^24 - 1) where ties go to the smaller id, permutations onto ids with gaps elsewhere
  F   the fixed points of metamorphic.FIXED
One case of each family runs again under a side stream and must give the same bits."""
import numpy as np
import pytest
import torch

import metamorphic as mm
from gpu_support import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

D_SHAPES = [(1, 65), (33, 130), (67, 129), (64, 64), (3, 5)]


def holding(family):
    return [n for n, op in mm.OPS.items() if op.families.get(family) == mm.HOLDS]


@pytest.fixture(scope="module")
def composed():
    return mm.inputs_of(*mm.composed_scene())


@pytest.fixture(scope="module")
def strip():
    return mm.inputs_of(*mm.strip_scene())


@pytest.fixture(scope="module")
def shaped():
    return {hw: mm.shape_scene(*hw) for hw in D_SHAPES}


@pytest.fixture(scope="module")
def reused():
    return mm.reused_scenes()


def on_side_stream(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = fn()
    side.synchronize()
    return out


@pytest.mark.parametrize("name", holding("D"))
def test_D_views(dev, shaped, reused, name):
    n = sum(mm.relation_D(name, shaped[hw], "gpu") for hw in D_SHAPES) + sum(mm.relation_D(name, x, "gpu") for _, x in reused)
    print("D %s: %d comparisons" % (name, n))


@pytest.mark.parametrize("name", holding("T"))
def test_T_placements(dev, composed, strip, name):
    k = mm.OPS[name].lattice
    plan = mm.placements(41, 45, lattice=k)
    assert mm.seam_gaps(plan, 41, 45, lattice=k) == []
    n = mm.relation_T(name, composed, "gpu", mm.CANVAS, plan)
    lane = [(0, dx - dx % k) for _, dx in mm.placements(3, 40, mm.STRIP_CANVAS, (0,), mm.STRIP_X)]
    n += mm.relation_T(name, strip, "gpu", mm.STRIP_CANVAS, list(dict.fromkeys(lane)))
    print("T %s: %d comparisons" % (name, n))


@pytest.mark.parametrize("name", holding("B"))
def test_B_batches(dev, composed, shaped, name):
    n = mm.relation_B(name, composed, "gpu") + mm.relation_B(name, shaped[(67, 129)], "gpu")
    print("B %s: %d comparisons" % (name, n))


@pytest.mark.parametrize("name", holding("R"))
def test_R_renamings(dev, composed, shaped, reused, name):
    n = 0
    for x in [composed, shaped[(33, 130)]] + [x for _, x in reused]:
        for f in mm.renamings(name, x):
            n += mm.relation_R(name, x, "gpu", f)
    print("R %s: %d comparisons" % (name, n))


def test_R_reaches_the_largest_id_and_ids_with_gaps(composed):
    top = mm.renamings("grow_cells", composed)[1]
    assert int(mm.relabel(composed["ids"], top).max()) == (1 << 24) - 1
    new = mm.relabel(composed["ids"], mm.renamings("cell_sums", composed)[0])
    assert {1, 7, 8, 500} <= set(np.unique(new).tolist())


@pytest.mark.parametrize("name", list(mm.FIXED))
def test_F_fixed_points(dev, composed, shaped, name):
    for x in (composed, shaped[(67, 129)], shaped[(3, 5)]):
        mm.FIXED[name][0](lambda op, x, **kw: mm.run(op, x, "gpu", **kw), x)


SIDE = {"D": "watershed[8]", "T": "shape_seeds[4]", "B": "cell_hulls", "R": "split_cells[4]", "F": "reconstruct"}


@pytest.mark.parametrize("family", list(SIDE))
def test_side_stream_gives_the_same_bits(dev, composed, shaped, family):
    name = SIDE[family]
    x = shaped[(67, 129)] if family == "D" else composed
    relation = {"D": lambda: mm.relation_D(name, x, "gpu", (5,)),
                "T": lambda: mm.relation_T(name, x, "gpu", mm.CANVAS, [(63, 65)]),
                "B": lambda: mm.relation_B(name, x, "gpu", mm.BATCH_ORDERS[1:2]),
                "R": lambda: mm.relation_R(name, x, "gpu", mm.order_map),
                "F": lambda: mm.FIXED[name][0](lambda op, x, **kw: mm.run(op, x, "gpu", **kw), x)}[family]
    on_side_stream(relation)
    for op in (mm.FIXED[name][1] if family == "F" else (name,)):
        here = mm.run(op, x, "gpu")
        assert mm.same(on_side_stream(lambda: mm.run(op, x, "gpu")), here) is None
