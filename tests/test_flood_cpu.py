"""The numpy restatements of the seeded watershed (tests/flood_ref.py), which tests/test_flood_gpu.py holds the device op to,
pinned on the CPU: the heap Dijkstra (a) against the level loop over split_ref.grow (b), which shares no code with it, against
hand-worked answers, and against the geodesic growth on a constant image; that the inputs hold the trap the one-key shortcut falls
into, and that the serpentine needs more than one round of launches; the quantisation rule of float images.  And the new entry
points: declared, in the ctypes table and in the library."""
import os
import re

import numpy as np
import pytest

import flood_ref as ref
import split_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_flood_scratch_bytes", "unet_flood_init", "unet_flood_sweeps", "unet_flood_assign", "unet_flood_finish")


def test_abi_declares_and_exports_the_new_entry_points():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(L, name), name
    assert len(_hip._SIGS["unet_flood_init"][1]) == 13 and len(_hip._SIGS["unet_flood_sweeps"][1]) == 9
    assert len(_hip._SIGS["unet_flood_assign"][1]) == 8 and len(_hip._SIGS["unet_flood_finish"][1]) == 10
    assert L.unet_flood_scratch_bytes(2, 33, 31) >= 2 * 33 * 31 * 26          # two key planes, two id planes, the levels
    assert L.unet_flood_scratch_bytes(2, 33, 31) < 2 * 33 * 31 * 26 + 5 * 256
    assert L.unet_flood_scratch_bytes(2, 0, 31) == 0


def test_library_refuses_bad_arguments_before_any_launch():
    """ARG_CHECK answers on the host: no device is needed to be refused."""
    import ctypes as C
    import _hip
    _hip.build()
    L = _hip.lib()
    q = C.c_void_p(4096)                                     # never dereferenced: every call below is refused first
    init = lambda *a: L.unet_flood_init(*a, None)
    assert init(q, q, 4, 0, q, 0, 1, 8, 8, q, q, q) == -2 and b"image_dtype" in L.unet_last_error()
    assert init(q, q, -1, 0, q, 0, 1, 8, 8, q, q, q) == -2
    assert init(q, q, 1, 0, q, 0, 1, 8, 8, q, q, q) == -2 and b"levels" in L.unet_last_error()
    assert init(q, q, 1, 65537, q, 0, 1, 8, 8, q, q, q) == -2 and b"levels" in L.unet_last_error()
    assert init(q, q, 2, 0, q, 4, 1, 8, 8, q, q, q) == -2 and b"mask_dtype" in L.unet_last_error()
    assert init(q, q, 2, 0, q, -1, 1, 8, 8, q, q, q) == -2
    assert init(None, q, 2, 0, q, 0, 1, 8, 8, q, q, q) == -2
    assert init(q, None, 2, 0, q, 0, 1, 8, 8, q, q, q) == -2
    assert init(q, q, 2, 0, q, 0, 1, 8, 8, None, q, q) == -2
    assert init(q, q, 2, 0, q, 0, 1, 8, 8, q, None, q) == -2
    assert init(q, q, 2, 0, q, 0, 1, 8, 8, q, q, None) == -2
    assert init(q, q, 2, 0, q, 0, 0, 8, 8, q, q, q) == -2
    assert init(q, q, 2, 0, q, 0, 1, 70000, 1, q, q, q) == -2 and b"too large" in L.unet_last_error()
    assert init(q, q, 2, 0, q, 0, 1, 65535, 65535, q, q, q) == -2 and b"too large" in L.unet_last_error()
    assert init(q, q, 2, 0, q, 0, 70000, 8, 8, q, q, q) == -2
    assert L.unet_flood_sweeps(1, 8, 8, -1, 0, q, 0, q, None) == -2
    assert L.unet_flood_sweeps(1, 8, 8, -1, 1, None, 0, q, None) == -2
    assert L.unet_flood_sweeps(1, 8, 8, -1, 1, q, -1, q, None) == -2
    assert L.unet_flood_sweeps(1, 8, 8, -1, 1, q, 0, None, None) == -2
    assert L.unet_flood_sweeps(1, 1, 70000, -1, 1, q, 0, q, None) == -2 and b"too large" in L.unet_last_error()
    assert L.unet_flood_assign(1, 8, 8, 0, q, 0, q, None) == -2
    assert L.unet_flood_assign(1, 8, 8, 1, None, 0, q, None) == -2
    assert L.unet_flood_assign(1, 8, 8, 1, q, -1, q, None) == -2
    assert L.unet_flood_assign(1, 8, 8, 1, q, 0, None, None) == -2
    assert L.unet_flood_assign(1, 70000, 1, 1, q, 0, q, None) == -2 and b"too large" in L.unet_last_error()
    assert L.unet_flood_finish(1, 8, 8, None, q, q, q, q, q, None) == -2
    assert L.unet_flood_finish(1, 8, 8, q, q, q, None, q, q, None) == -2
    assert L.unet_flood_finish(1, 8, 8, q, q, q, q, None, q, None) == -2
    assert L.unet_flood_finish(1, 8, 8, q, q, q, q, q, None, None) == -2
    assert L.unet_flood_finish(1, 0, 8, q, q, q, q, q, q, None) == -2
    assert L.unet_flood_finish(1, 70000, 1, q, q, q, q, q, q, None) == -2 and b"too large" in L.unet_last_error()


def test_python_surface():
    import inspect
    import functions
    import tester
    import torch
    sig = inspect.signature(functions.watershed)
    P = inspect.Parameter
    assert list(sig.parameters) == ["seeds", "image", "mask", "levels", "max_level", "return_levels", "_launches", "connectivity"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, None, None, False, 8, 4]
    assert all(sig.parameters[k].kind is P.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert all(sig.parameters[k].kind is P.POSITIONAL_OR_KEYWORD and sig.parameters[k].default is P.empty for k in ("seeds", "image"))
    assert functions.FloodInfo._fields == ("seeds_outside", "unreached", "max_level", "launches")
    sig = inspect.signature(tester.split_by_watershed)
    assert list(sig.parameters) == ["mask", "fg_prob", "high", "levels", "connectivity"] and sig.parameters["levels"].default == 64
    assert [p.kind for p in sig.parameters.values()] == [P.POSITIONAL_OR_KEYWORD] * 4 + [P.KEYWORD_ONLY]
    assert [p.default for p in sig.parameters.values()] == [P.empty] * 3 + [64, 4]
    s = torch.zeros(2, 5, 7, dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        functions.watershed(s, s)
    with pytest.raises(NotImplementedError):
        functions.watershed(s.numpy(), s.numpy())
    with pytest.raises(NotImplementedError):
        functions.watershed(s, s, mask=s)
    with pytest.raises(ValueError, match="equal shape"):
        functions.watershed(s, s[:1])
    with pytest.raises(ValueError, match="equal shape"):
        functions.watershed(s, s, mask=s[:, :3])
    with pytest.raises(ValueError, match="int32 or int64"):
        functions.watershed(s.float(), s)
    with pytest.raises(ValueError, match="levels"):
        functions.watershed(s, s.float())
    for bad in (0, 65537, 2.5, True):
        with pytest.raises(ValueError, match="levels"):
            functions.watershed(s, s.float(), levels=bad)
    with pytest.raises(ValueError, match="levels"):
        functions.watershed(s, s, levels=4)
    with pytest.raises(ValueError, match="max_level"):
        functions.watershed(s, s, max_level=-1)
    with pytest.raises(ValueError, match="_launches"):
        functions.watershed(s, s, _launches=0)
    # segment's own keyword checks come before any work, and before the device is asked for
    for kw, word in ((dict(watershed=16), "split"), (dict(watershed=16, return_instances=True), "split"),
                     (dict(watershed=16, return_instances=True, split=0.5, shape_split=2.0), "shape_split"),
                     (dict(watershed=16, split=0.5), "return_instances"),
                     (dict(watershed=0, return_instances=True, split=0.5), "watershed"),
                     (dict(watershed=1 << 17, return_instances=True, split=0.5), "watershed"),
                     (dict(watershed=2.5, return_instances=True, split=0.5), "watershed"),
                     (dict(watershed="yes", return_instances=True, split=0.5), "watershed")):
        with pytest.raises(ValueError, match=word):
            tester.segment(None, s.float(), **kw)


# ---- the two statements ---------------------------------------------------------------------------------------------------------

def test_the_dijkstra_equals_the_level_loop():
    """(a) == (b) on every image of the GPU tests up to 65 x 63 with at most 8 levels, on the random small images and on the
    built cases, without a limit and with max_level."""
    cases = [(n, s, im, m) for n, s, im, m in ref.small_cases(8)]
    cases += [("random %d" % k, s, im, m) for k, (s, im, m) in enumerate(ref.random_small())]
    cases += [("plateau 6", *ref.plateau(6), None), ("plateau 5", *ref.plateau(5), None), ("ridge", *ref.ridge(), None),
              ("pit", *ref.pit(), None), ("late low path", *ref.late_low_path())]
    assert len(cases) > 60
    kinds = set()
    for name, s, im, m in cases:
        kinds.add(name.split()[-2] if name.startswith(("busy", "tiny")) else "")
        for limit in (None, 0, 2):
            a = ref.flood(s, im, m, max_level=limit)
            out, pass_level = ref.level_loop(s, im, m, max_level=limit)
            assert np.array_equal(a["out"], out) and np.array_equal(a["pass_level"], pass_level), (name, limit)
            assert ((a["dist"] >= 0) == (out > 0)).all() and ((a["dist"] == 0) == ((a["pass_level"] == 0) & (np.asarray(s) > 0) & (out > 0))).all()
    assert any("random6" in k for k in kinds) and any("random2" in k for k in kinds) and any("constant" in k for k in kinds)


def test_a_constant_image_gives_the_geodesic_growth():
    n = 0
    for H, W in ref.SIZES[:8]:
        for name, s, im, m in ref.size_cases(H, W):
            for b in range(len(s)):
                if (im[b] != 3).any():                        # landscape("constant")
                    continue
                n += 1
                for limit in (None, 3):                       # above the constant 3: no limit at all
                    a, g = ref.flood(s[b], im[b], m[b], max_level=limit), split_ref.grow(s[b], m[b])
                    assert np.array_equal(a["out"], g["out"]), (name, b)
                    # a step off a source onto level 3 starts the plateau's count at 1: d is the geodesic distance everywhere
                    assert np.array_equal(a["dist"], g["dist"]), (name, b)
                    assert (a["unreached"], a["seeds_outside"], a["status"]) == (g["unreached"], g["seeds_outside"], g["status"])
                    assert set(np.unique(a["pass_level"])) <= {-1, 0, 3}
                sources = np.where((s[b] > 0) & (s[b] < ref.ID_END) & (m[b] != 0), s[b], 0)
                assert np.array_equal(ref.flood(s[b], im[b], m[b], max_level=2)["out"], sources)      # below the plateau: the sources
    assert n >= 8


# ---- hand-worked cases --------------------------------------------------------------------------------------------------------

def test_a_plateau_is_cut_at_its_geodesic_midline():
    r = ref.flood(*ref.plateau(6))                           # an even gap: three pixels each
    assert r["out"].tolist() == [[7, 7, 7, 7, 4, 4, 4, 4]]
    assert r["pass_level"].tolist() == [[0, 5, 5, 5, 5, 5, 5, 0]] and r["dist"].tolist() == [[0, 1, 2, 3, 3, 2, 1, 0]]
    r = ref.flood(*ref.plateau(5))                           # an odd gap: the middle pixel is 3 from both, the smaller id
    assert r["out"].tolist() == [[7, 7, 7, 4, 4, 4, 4]]
    assert r["pass_level"].tolist() == [[0, 5, 5, 5, 5, 5, 0]] and r["dist"].tolist() == [[0, 1, 2, 3, 2, 1, 0]]
    assert (r["unreached"], r["seeds_outside"], r["max_level"], r["status"], r["bad_values"]) == (0, 0, 5, 0, 0)


def test_the_cut_follows_a_ridge_and_not_the_middle():
    s, im = ref.ridge()
    r = ref.flood(s, im)
    # level 1: x = 1..4 from the 7, x = 6 from the 4; level 9: x = 5 is one step from both sides, the smaller id
    assert r["out"].tolist() == [[7, 7, 7, 7, 7, 4, 4, 4]]
    assert r["pass_level"].tolist() == [[0, 1, 1, 1, 1, 9, 1, 0]] and r["dist"].tolist() == [[0, 1, 2, 3, 4, 1, 1, 0]]
    assert split_ref.grow(s, np.ones_like(s))["out"].tolist() == [[7, 7, 7, 7, 4, 4, 4, 4]]
    r = ref.flood(s, im, max_level=8)
    assert r["out"].tolist() == [[7, 7, 7, 7, 7, 0, 4, 4]] and (r["unreached"], r["max_level"]) == (1, 1)


def test_a_seedless_pit_behind_a_pass():
    s, im = ref.pit()
    r = ref.flood(s, im)
    assert r["out"].tolist() == [[3, 3, 3, 3, 3]]
    assert r["pass_level"].tolist() == [[0, 2, 6, 6, 6]] and r["dist"].tolist() == [[0, 1, 1, 2, 3]]    # the pit fills at the pass
    assert (r["unreached"], r["max_level"]) == (0, 6)
    r = ref.flood(s, im, max_level=5)
    assert r["out"].tolist() == [[3, 3, 0, 0, 0]] and r["pass_level"].tolist() == [[0, 2, -1, -1, -1]]
    assert (r["unreached"], r["max_level"]) == (3, 2)
    r = ref.flood(s, im, mask=np.array([[0, 1, 1, 1, 1]]))   # the seed is outside: nothing floods
    assert not r["out"].any() and (r["unreached"], r["seeds_outside"], r["max_level"]) == (4, 1, 0)


def test_the_late_low_path():
    s, im, m = ref.late_low_path()
    r = ref.flood(s, im, m)
    assert r["out"].tolist() == [[1, 1, 2, 2, 0],
                                 [0, 0, 2, 0, 0],
                                 [2, 2, 2, 0, 0]]
    assert r["pass_level"].tolist() == [[0, 3, 0, 5, -1],
                                        [-1, -1, 0, -1, -1],
                                        [0, 0, 0, -1, -1]]
    assert r["dist"].tolist() == [[0, 1, 4, 1, -1],
                                  [-1, -1, 3, -1, -1],
                                  [0, 1, 2, -1, -1]]
    wrong = ref.naive(s, im, m)
    assert wrong[0].tolist() == [1, 1, 2, 1, 0] and (wrong[1:] == r["out"][1:]).all()      # r kept the id that came over the wall


def test_the_inputs_can_catch_the_one_key_shortcut():
    differ = [k for k, (s, im, m) in enumerate(ref.random_small()) if not np.array_equal(ref.naive(s, im, m), ref.flood(s, im, m)["out"])]
    print("the one-key relaxation is wrong on random images", differ)
    assert differ
    H, W = 33, 31                                            # and on an input of the GPU tests
    hit = 0
    for name, s, im, m in ref.size_cases(H, W):
        hit += sum(not np.array_equal(ref.naive(s[b], im[b], m[b]), ref.flood(s[b], im[b], m[b])["out"]) for b in range(len(s)))
    assert hit


def test_the_serpentine_needs_more_than_one_round_of_launches():
    s, im, m = ref.serpentine()
    r = ref.flood(s[0], im[0], m[0])
    corridor = im[0] == 0
    assert r["unreached"] == 0 and r["max_level"] == 5 and set(np.unique(r["out"])) == {1, 2}
    assert (r["pass_level"][corridor] == 0).all() and (r["pass_level"][~corridor] == 5).all() and (r["dist"][~corridor] == 1).all()
    g = split_ref.grow(*[a[0] for a in split_ref.serpentine()])
    assert np.array_equal(r["dist"][corridor], g["dist"][corridor]) and np.array_equal(r["out"][corridor], g["out"][corridor])
    y, x = np.unravel_index(np.argmax(np.where(corridor, r["dist"], -1)), corridor.shape)
    assert r["dist"][y, x] > 4000
    assert ref.tile_borders_crossed(r, im[0], y, x) > 8      # each launch carries a key one tile further


# ---- float images ---------------------------------------------------------------------------------------------------------------

def test_the_quantisation_of_float_images():
    for levels in (1, 6, 64, 65536):
        under = np.nextafter(np.float32(1) / np.float32(levels), np.float32(0))
        x = np.array([0.0, under, 1.0, np.nextafter(np.float32(1), np.float32(2)), -0.25, -1e30, 0.5, 3e38], np.float32)
        v, bad = ref.quantise(x, levels)
        first = 0 if np.float32(under) * np.float32(levels) < 1 else min(1, levels - 1)
        assert v.tolist() == [0, first, levels - 1, levels - 1, 0, 0, int(np.floor(np.float32(0.5) * np.float32(levels))) if levels > 1 else 0,
                              levels - 1] and bad == 0, levels
    assert ref.quantise(np.array([np.float32(1) / np.float32(64)], np.float32), 64)[0].tolist() == [1]
    assert ref.quantise(np.array([np.nextafter(np.float32(1 / 64), np.float32(0))], np.float32), 64)[0].tolist() == [0]
    v, bad = ref.quantise(np.array([np.nan, np.inf, -np.inf, 0.3], np.float32), 10)
    assert bad == 3 and v.tolist() == [0, 9, 0, 3]
    v, bad = ref.quantise(np.array([0, 65535, 65536, -1], np.int64))
    assert bad == 2 and v.tolist() == [0, 65535, 0, 0]
    # the product is formed in float32: float32(0.7) is 0.69999999, times 10 it rounds to 7 where exact arithmetic gives 6.9999999
    assert ref.quantise(np.array([0.7], np.float32), 10)[0].tolist() == [7]
