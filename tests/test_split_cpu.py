"""The numpy restatement of the seeded geodesic growth (tests/split_ref.py), which tests/test_split_gpu.py holds the device op to,
pinned on the CPU: against a per-seed geodesic distance by masked binary dilation, against hand-worked answers, and that the
inputs of the GPU tests exercise the code.  And the new entry points: declared, in the ctypes table and in the library."""
import functools
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import rand_ref
import split_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_geodesic_scratch_bytes", "unet_geodesic_init", "unet_geodesic_sweeps", "unet_geodesic_finish")


def test_abi_declares_and_exports_the_new_entry_points():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(L, name), name
    assert L.unet_abi_version() == 4
    assert len(_hip._SIGS["unet_geodesic_init"][1]) == 10 and len(_hip._SIGS["unet_geodesic_sweeps"][1]) == 9
    assert len(_hip._SIGS["unet_geodesic_finish"][1]) == 10
    assert L.unet_geodesic_scratch_bytes(2, 33, 31) >= 2 * 33 * 31 * 16     # two planes of 64-bit keys
    assert L.unet_geodesic_scratch_bytes(2, 0, 31) == 0


def test_library_refuses_bad_arguments_before_any_launch():
    """ARG_CHECK answers on the host: no device is needed to be refused."""
    import ctypes as C
    import _hip
    _hip.build()
    L = _hip.lib()
    q = C.c_void_p(4096)                                     # never dereferenced: every call below is refused first
    assert L.unet_geodesic_init(q, q, 4, 1, 8, 8, q, q, q, None) == -2 and b"dtype" in L.unet_last_error()
    assert L.unet_geodesic_init(q, q, -1, 1, 8, 8, q, q, q, None) == -2
    assert L.unet_geodesic_init(None, q, 0, 1, 8, 8, q, q, q, None) == -2
    assert L.unet_geodesic_init(q, None, 0, 1, 8, 8, q, q, q, None) == -2
    assert L.unet_geodesic_init(q, q, 0, 1, 8, 8, None, q, q, None) == -2
    assert L.unet_geodesic_init(q, q, 0, 1, 8, 8, q, None, q, None) == -2
    assert L.unet_geodesic_init(q, q, 0, 1, 8, 8, q, q, None, None) == -2
    assert L.unet_geodesic_init(q, q, 0, 0, 8, 8, q, q, q, None) == -2
    assert L.unet_geodesic_init(q, q, 0, 1, 70000, 1, q, q, q, None) == -2 and b"too large" in L.unet_last_error()
    assert L.unet_geodesic_init(q, q, 0, 1, 65535, 65535, q, q, q, None) == -2 and b"too large" in L.unet_last_error()
    assert L.unet_geodesic_init(q, q, 0, 70000, 8, 8, q, q, q, None) == -2
    assert L.unet_geodesic_sweeps(1, 8, 8, -1, 0, q, 0, q, None) == -2
    assert L.unet_geodesic_sweeps(1, 8, 8, -1, 1, None, 0, q, None) == -2
    assert L.unet_geodesic_sweeps(1, 8, 8, -1, 1, q, -1, q, None) == -2
    assert L.unet_geodesic_sweeps(1, 8, 8, -1, 1, q, 0, None, None) == -2
    assert L.unet_geodesic_sweeps(1, 1, 70000, -1, 1, q, 0, q, None) == -2 and b"too large" in L.unet_last_error()
    assert L.unet_geodesic_finish(1, 8, 8, -1, None, q, q, q, q, None) == -2
    assert L.unet_geodesic_finish(1, 8, 8, -1, q, q, None, q, q, None) == -2
    assert L.unet_geodesic_finish(1, 8, 8, -1, q, q, q, None, q, None) == -2
    assert L.unet_geodesic_finish(1, 8, 8, -1, q, q, q, q, None, None) == -2
    assert L.unet_geodesic_finish(1, 0, 8, -1, q, q, q, q, q, None) == -2
    assert L.unet_geodesic_finish(1, 70000, 1, -1, q, q, q, q, q, None) == -2 and b"too large" in L.unet_last_error()


def test_python_surface():
    import inspect
    import functions
    import tester
    sig = inspect.signature(functions.split_cells)
    P = inspect.Parameter
    assert list(sig.parameters) == ["seeds", "mask", "max_steps", "orphans", "return_distance", "_launches", "connectivity"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, "drop", False, 8, 4]
    assert all(sig.parameters[k].kind is P.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert all(sig.parameters[k].kind is P.POSITIONAL_OR_KEYWORD and sig.parameters[k].default is P.empty for k in ("seeds", "mask"))
    assert functions.SplitInfo._fields == ("seeds_outside", "unreached", "max_distance", "launches")
    assert str(inspect.signature(tester.split_instances)) == "(mask, fg_prob, high, *, connectivity=4)"
    seg = inspect.signature(tester.segment)
    assert [k for k, p in seg.parameters.items() if p.kind is P.POSITIONAL_OR_KEYWORD][-1] == "split" and seg.parameters["split"].default is None
    assert [(k, p.kind, p.default) for k, p in list(seg.parameters.items())[-3:]] == [
        ("measure", P.KEYWORD_ONLY, False), ("watershed", P.KEYWORD_ONLY, None), ("connectivity", P.KEYWORD_ONLY, None)]
    import torch
    s = torch.zeros(2, 5, 7, dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        functions.split_cells(s, s)
    with pytest.raises(NotImplementedError):
        functions.split_cells(s.numpy(), s.numpy())
    with pytest.raises(ValueError, match="equal shape"):
        functions.split_cells(s, s[:1])
    with pytest.raises(ValueError, match="max_steps"):
        functions.split_cells(s, s, max_steps=-1)
    with pytest.raises(ValueError, match="orphans"):
        functions.split_cells(s, s, orphans="merge")
    with pytest.raises(ValueError, match="int32 or int64"):
        functions.split_cells(s.float(), s)


# ---- the independent pin: per seed id, the geodesic distance by masked binary dilation ------------------------------------------

@functools.lru_cache(maxsize=None)
def gpu_inputs():
    """(name, seeds [H,W], mask [H,W]) of every image the GPU tests grow."""
    out = []
    for H, W in ref.SIZES:
        for name, s, m in ref.size_cases(H, W):
            out += [("%s %dx%d[%d]" % (name, H, W, b), s[b], m[b]) for b in range(len(s))]
    s, m = ref.serpentine()
    out.append(("serpentine", s[0], m[0]))
    return out


@functools.lru_cache(maxsize=None)
def by_dilation(k):
    """(ids [n], dist int64 [n,H,W]) of gpu_inputs()[k]: for every seed id with a pixel in the region, the number of masked
    dilations with the 4-neighbour structure after which a pixel is first set (BIG where it never is)."""
    name, seeds, mask = gpu_inputs()[k]
    region = mask != 0
    ids = np.unique(seeds[(seeds > 0) & (seeds < ref.ID_END) & region])
    dist = np.full((len(ids),) + seeds.shape, ref.BIG)
    for j, i in enumerate(ids):
        cur = (seeds == i) & region
        dist[j][cur] = 0
        d = 0
        while True:
            d += 1
            nxt = ndimage.binary_dilation(cur, ref.CROSS, mask=region)
            new = nxt & ~cur
            if not new.any():
                break
            dist[j][new] = d
            cur = nxt
    return ids, dist


def lexicographic_min(ids, dist, shape, max_steps=None):
    if len(ids) == 0:
        return np.zeros(shape, np.int32), np.full(shape, -1, np.int32)
    best = dist.min(axis=0)
    who = np.where(dist == best, ids[:, None, None], ref.BIG).min(axis=0)     # the smallest id among those at the least distance
    ok = best < ref.BIG if max_steps is None else best <= max_steps
    return np.where(ok, who, 0).astype(np.int32), np.where(ok, best, -1).astype(np.int32)


def test_the_restatement_equals_the_dilation_definition_on_the_gpu_inputs():
    for k, (name, seeds, mask) in enumerate(gpu_inputs()):
        ids, dist = by_dilation(k)
        for steps in ref.STEPS:
            want_out, want_dist = lexicographic_min(ids, dist, seeds.shape, steps)
            got = ref.grow(seeds, mask, steps)
            assert np.array_equal(got["out"], want_out) and np.array_equal(got["dist"], want_dist), (name, steps)
            region = mask != 0
            assert got["unreached"] == (region & (want_out == 0)).sum() and got["max_dist"] == want_dist.max(initial=0), (name, steps)
            assert (got["out"][~region] == 0).all() and (got["dist"][got["out"] == 0] == -1).all()


def test_the_gpu_inputs_exercise_the_code():
    """Conditions on the inputs, so that a weak input cannot hide a failure."""
    busy = 0
    for k, (name, seeds, mask) in enumerate(gpu_inputs()):
        if not name.startswith("busy") or not seeds.any() or not mask.any() or mask.all():
            continue                                         # the no-seed, empty-mask and full-mask images of the batch of four
        busy += 1
        ids, dist = by_dilation(k)
        best = dist.min(axis=0)
        tie = ((dist == best).sum(axis=0) >= 2) & (best < ref.BIG)
        got = ref.grow(seeds, mask)
        assert tie.any() and tie[0, 1] and got["out"][0, 1] == 3, name               # two ids at equal least distance
        assert got["unreached"] >= 1 and mask[-1, -1] and got["out"][-1, -1] == 0, name
        assert got["seeds_outside"] >= 1, name
        grown = rand_ref.grow(np.where((seeds > 0) & (seeds < ref.ID_END), seeds, 0)) * (mask != 0)
        assert not np.array_equal(got["out"], grown), name
        # beyond the built-in unreached pixel: a reached pixel whose geodesic owner is not its Euclidean one, where walls fit
        assert min(mask.shape) < 20 or ((got["out"] != grown) & (got["out"] > 0)).any(), name
        assert ref.grow(seeds, mask, 5)["unreached"] > got["unreached"] or mask.size < 40, name
    assert busy >= 3 * (len(ref.SIZES) - 2)
    name, seeds, mask = gpu_inputs()[-1]
    r = ref.grow(seeds, mask)
    assert name == "serpentine" and r["max_dist"] > 4000 and r["unreached"] == 0 and set(np.unique(r["out"])) == {0, 1, 2}


# ---- hand-worked cases --------------------------------------------------------------------------------------------------------

def test_a_line_with_seeds_at_both_ends():
    seeds = np.array([[7, 0, 0, 0, 0, 0, 4]])
    r = ref.grow(seeds, np.ones((1, 7)))
    assert r["out"].tolist() == [[7, 7, 7, 4, 4, 4, 4]]                             # the middle is 3 from both: the smaller id
    assert r["dist"].tolist() == [[0, 1, 2, 3, 2, 1, 0]]
    assert (r["unreached"], r["seeds_outside"], r["max_dist"], r["status"]) == (0, 0, 3, 0)


def test_a_seed_outside_the_mask():
    seeds = np.array([[0, 9, 0, 0],
                      [0, 0, 0, 2]])
    mask = np.array([[1, 0, 1, 1],
                     [1, 0, 1, 1]])
    r = ref.grow(seeds, mask)
    assert r["out"].tolist() == [[0, 0, 2, 2], [0, 0, 2, 2]]                        # 9 is no seed; the left column is never reached
    assert r["dist"].tolist() == [[-1, -1, 2, 1], [-1, -1, 1, 0]]
    assert (r["unreached"], r["seeds_outside"], r["max_dist"], r["status"]) == (2, 1, 2, 0)
    r = ref.grow(np.array([[1 << 24, -3, 5]]), np.array([[1, 1, 1]]))               # ids outside [0, 2^24) index nothing
    assert r["out"].tolist() == [[5, 5, 5]] and r["dist"].tolist() == [[2, 1, 0]] and r["status"] == 2 and r["seeds_outside"] == 0


def test_a_wall_makes_the_geodesic_choice_differ_from_the_euclidean_one():
    seeds = np.array([[1, 0, 0, 0, 0],
                      [0, 0, 0, 0, 0],
                      [0, 0, 0, 0, 2]])
    mask = np.array([[1, 0, 1, 1, 1],
                     [1, 0, 1, 0, 1],
                     [1, 1, 1, 0, 1]])
    r = ref.grow(seeds, mask)
    # (2, 2) is 2 columns from seed 2 as the crow flies but 6 steps round the wall, and 4 steps from seed 1; (0, 2) is 2 columns
    # from seed 1 but 6 steps round its wall, and 4 steps from seed 2; (1, 2) is 5 steps from both: the smaller id
    assert r["out"].tolist() == [[1, 0, 2, 2, 2],
                                 [1, 0, 1, 0, 2],
                                 [1, 1, 1, 0, 2]]
    assert r["dist"].tolist() == [[0, -1, 4, 3, 2],
                                  [1, -1, 5, -1, 1],
                                  [2, 3, 4, -1, 0]]
    grown = rand_ref.grow(seeds) * mask
    assert grown.tolist() == [[1, 0, 1, 2, 2],
                              [1, 0, 1, 0, 2],
                              [1, 1, 2, 0, 2]]
    assert r["max_dist"] == 5 and r["unreached"] == 0


def test_max_steps():
    seeds = np.array([[3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 8]])
    mask = np.ones((1, 14))
    want = {0: [3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 8],
            1: [3, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 8, 8],
            5: [3, 3, 3, 3, 3, 3, 0, 0, 8, 8, 8, 8, 8, 8],
            None: [3, 3, 3, 3, 3, 3, 3, 8, 8, 8, 8, 8, 8, 8]}
    for steps, row in want.items():
        r = ref.grow(seeds, mask, steps)
        assert r["out"].tolist() == [row], steps
        assert r["unreached"] == row.count(0) and r["max_dist"] == (6 if steps is None else steps)
        assert r["dist"][0].tolist() == [-1 if v == 0 else min(x, 13 - x) for x, v in enumerate(row)]


def test_orphans_keep():
    seeds = np.array([[0, 6, 0, 0, 0, 0],
                      [0, 0, 0, 0, 0, 0]])
    mask = np.array([[1, 1, 0, 1, 0, 1],
                     [0, 0, 0, 1, 0, 1]])
    out = ref.grow(seeds, mask)["out"]
    assert out.tolist() == [[6, 6, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]
    assert ref.keep_orphans(out, seeds, mask).tolist() == [[6, 6, 0, 7, 0, 8], [0, 0, 0, 7, 0, 8]]
