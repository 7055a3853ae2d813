"""Linking cells across frames without a GPU: the C ABI and the Python surface are there, functions.tracks_from_links (pure
host) gives the tables worked by hand below and equals the independent restatement tests/track_ref.tracks on every seeded
time-lapse, and the restatement of the links (what the GPU tests compare the device with) gives hand-worked answers too."""
import inspect
import io
import os
import re

import numpy as np
import pytest
import torch

import track_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_link_frames_scratch_bytes", "unet_link_frames")


def rows(*frames):
    """Three int64 arrays [T][N] from per-frame lists of (area, pred, overlap) per id 1.."""
    T, N = len(frames), 1 + max(len(f) for f in frames)
    out = np.zeros((3, T, N), np.int64)
    for t, f in enumerate(frames):
        for c, triple in enumerate(f, 1):
            out[:, t, c] = triple
    return out


def table_of(links, **kw):
    import functions
    t = functions.tracks_from_links(links, **kw)
    assert t.table.dtype == np.int64 and t.table.shape[1:] == (4,) and t.track_of.dtype == np.int32 and t.track_of.shape == links[0].shape
    ref.check_structure(t.table, t.track_of, links[0])
    return t.table.tolist(), t.track_of.tolist()


def test_abi_declares_and_exports_the_new_entry_points():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(L, name), name
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr).group(1).split(",")
        assert len(_hip._SIGS[name][1]) == len(params), name
    assert len(_hip._SIGS["unet_link_frames"][1]) == 13 and len(_hip._SIGS["unet_link_frames_scratch_bytes"][1]) == 3
    assert L.unet_abi_version() == 4
    assert L.unet_link_frames_scratch_bytes(3, 10, 0) == 0 and L.unet_link_frames_scratch_bytes(0, 10, 64) == 0
    assert L.unet_link_frames_scratch_bytes(3, -1, 64) == 0
    assert L.unet_link_frames_scratch_bytes(3, 10, 1024) >= 1024 * 12 + 3 * 11 * 8


def test_python_surface_and_argument_errors():
    import functions
    import tester
    z = torch.zeros(3, 4, 4, dtype=torch.int32)
    for f in (functions.link_frames, functions.track_cells):
        with pytest.raises(NotImplementedError, match="device"):
            f(z)
        with pytest.raises(ValueError, match=r"\[T,H,W\]"):
            f(z[0])
        with pytest.raises(ValueError, match="65535"):
            f(torch.zeros(65536, 1, 1, dtype=torch.int32))
        with pytest.raises(ValueError, match="int32 or int64"):
            f(z.float())
        with pytest.raises(ValueError, match="reach"):
            f(z, reach=-1)
    with pytest.raises(ValueError, match="min_overlap"):
        functions.track_cells(z, min_overlap=2)
    one = rows([(5, 0, 0)])
    for kw in ({"min_overlap": -0.1}, {"min_overlap": None}, {"max_children": 0}, {"max_children": 1.5}, {"divisions": 2}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            functions.tracks_from_links(one, **kw)
    with pytest.raises(ValueError, match="one shape"):
        functions.tracks_from_links((one[0], one[1], one[2][:, :1]))
    with pytest.raises(ValueError, match="no cell of frame 0"):
        functions.tracks_from_links(rows([(5, 0, 0)], [(5, 2, 3)]))
    assert functions.FrameLinks._fields == ("area", "pred", "pred_overlap") and functions.Tracks._fields == ("table", "track_of")
    p = inspect.signature(tester.track).parameters
    assert [k for k in p][:2] == ["unet", "frames"] and p["reach"].default is None and p["min_overlap"].default == 0.0
    assert p["divisions"].default is True and p["max_children"].default == 2 and p["reach"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "segment_kwargs" in p
    with pytest.raises(ValueError, match="return_probs"):
        tester.track(None, z, return_probs=True)
    assert "track" not in inspect.signature(tester.segment).parameters


# ---- tracks_from_links: hand-worked tables -------------------------------------------------------------------------------------

def test_one_drifting_cell():
    links = rows([(5, 0, 0)], [(5, 1, 4)], [(6, 1, 5)], [(5, 1, 3)])
    assert table_of(links) == ([[1, 0, 3, 0]], [[0, 1]] * 4)


def test_a_division_at_frame_2():
    links = rows([(10, 0, 0)], [(10, 1, 9)], [(4, 1, 4), (4, 1, 3)], [(4, 1, 4), (4, 2, 4)])
    assert table_of(links)[0] == [[1, 0, 1, 0], [2, 2, 3, 1], [3, 2, 3, 1]]


def test_three_claimants():
    """Ids 2 and 3 overlap the mother by 5, id 1 by 3: ranked 2, 3, 1.  Labels go by id, so the one left over is label 2."""
    links = rows([(20, 0, 0)], [(3, 1, 3), (5, 1, 5), (6, 1, 5)])
    assert table_of(links) == ([[1, 0, 0, 0], [2, 1, 1, 0], [3, 1, 1, 1], [4, 1, 1, 1]], [[0, 1, 0, 0], [0, 2, 3, 4]])
    assert table_of(links, max_children=3)[0] == [[1, 0, 0, 0], [2, 1, 1, 1], [3, 1, 1, 1], [4, 1, 1, 1]]
    assert table_of(links, max_children=1)[0] == [[1, 0, 0, 0], [2, 1, 1, 0], [3, 1, 1, 1], [4, 1, 1, 0]]


def test_without_divisions_the_best_claimant_continues():
    links = rows([(20, 0, 0)], [(3, 1, 3), (5, 1, 5), (6, 1, 5)])
    assert table_of(links, divisions=False) == ([[1, 0, 1, 0], [2, 1, 1, 0], [3, 1, 1, 0]], [[0, 1, 0, 0], [0, 2, 1, 3]])


def test_min_overlap_rejects_a_link():
    links = rows([(10, 0, 0)], [(10, 1, 4)])
    assert table_of(links)[0] == [[1, 0, 1, 0]]
    assert table_of(links, min_overlap=0.4)[0] == [[1, 0, 1, 0]]            # 4 >= 0.4 * 10 holds in float64
    assert table_of(links, min_overlap=0.5)[0] == [[1, 0, 0, 0], [2, 1, 1, 0]]


def test_a_merge():
    links = rows([(9, 0, 0), (7, 0, 0)], [(30, 1, 9)])
    assert table_of(links) == ([[1, 0, 1, 0], [2, 0, 0, 0]], [[0, 1, 2], [0, 1, 0]])


def test_a_vanish_and_an_appear():
    links = rows([(0, 0, 0), (0, 0, 0), (8, 0, 0)], [(0, 0, 0), (0, 0, 0), (8, 0, 0)])
    assert table_of(links) == ([[1, 0, 0, 0], [2, 1, 1, 0]], [[0, 0, 0, 1], [0, 0, 0, 2]])


def test_an_empty_middle_frame():
    links = rows([(5, 0, 0)], [], [(5, 0, 0)], [(5, 1, 5)])
    assert table_of(links) == ([[1, 0, 0, 0], [2, 2, 3, 0]], [[0, 1], [0, 0], [0, 2], [0, 2]])


def test_a_single_frame_and_no_cells():
    import functions
    assert table_of(np.array([[[5, 3, 0, 2]], [[0, 0, 0, 0]], [[0, 0, 0, 0]]])) == ([[1, 0, 0, 0], [2, 0, 0, 0]], [[0, 1, 0, 2]])
    t = functions.tracks_from_links(np.zeros((3, 2, 4), np.int64))
    assert t.table.shape == (0, 4) and not t.track_of.any() and t.ctc_text() == ""


# ---- the restatements ------------------------------------------------------------------------------------------------------------

def test_links_of_hand_worked_frames():
    """tie_frames: 2 x 2 pixels of the one cell on each of two cells: the smaller id, whichever side it is on.  Then ids out of
    range: counted apart, and their pixels count nowhere."""
    for left, right in ((3, 8), (8, 3)):
        area, pred, over, status, n_pairs = ref.links(*[ref.tie_frames(left, right)] * 2)
        assert pred[1].tolist() == [0, 3] + [0] * 7 and over[1].tolist() == [0, 4] + [0] * 7 and n_pairs == 2
        assert area[0, [0, 3, 8]].tolist() == [24, 12, 12] and area[1, :2].tolist() == [40, 8] and not status.any()
        assert not pred[0].any() and not over[0].any()
    f = np.array([[[1, 1, 2, 2, 0, 9]], [[1, 1, 1, 2, -1, 2]]])
    area, pred, over, status, n_pairs = ref.links(f, f, n_max=2)
    assert status.tolist() == [[1, 0], [2, 0]]                            # frame 0: the 9; pair 1: the -1, and the 2 above the 9
    assert area.tolist() == [[1, 2, 2], [0, 3, 1]]
    assert pred.tolist() == [[0, 0, 0], [0, 1, 2]] and over.tolist() == [[0, 0, 0], [0, 2, 1]] and n_pairs == 3


def test_the_dividing_sequence_by_hand():
    """Mother 1 (radius 10) has three daughters, mother 2 two: the labels go by (frame, id)."""
    import functions
    m = ref.dividing_discs()
    area, pred, over, status, _ = ref.links(m, m)
    assert pred[2].tolist() == [0, 2, 1, 1, 1, 2] and over[2, 1] == over[2, 5] and over[2, 3] > over[2, 4] > over[2, 2]
    t = functions.tracks_from_links((area, pred, over))
    assert t.table.tolist() == [[1, 0, 1, 0], [2, 0, 1, 0], [3, 2, 3, 2], [4, 2, 3, 0], [5, 2, 3, 1], [6, 2, 3, 1], [7, 2, 3, 2]]


@pytest.mark.parametrize("kw", [{}, {"min_overlap": 0.5}, {"divisions": False}, {"max_children": 3}, {"max_children": 1, "min_overlap": 0.2}],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "default")
def test_tracks_from_links_equals_the_restatement(kw):
    import functions
    n_tracks = 0
    for name, m in ref.sequences():
        for reach in (None, 3):
            src = m if reach is None else np.stack([grown(f, reach) for f in m])
            area, pred, over, status, _ = ref.links(src, m)
            assert not status.any()
            got = functions.tracks_from_links(functions.FrameLinks(area, pred, over), **kw)
            want = ref.tracks(area, pred, over, **kw)
            assert np.array_equal(got.table, want[0]) and np.array_equal(got.track_of, want[1]), (name, reach)
            ref.check_structure(got.table, got.track_of, area)
            n_tracks += len(got.table)
    assert n_tracks > 100


def grown(frame, reach):
    import rand_ref
    return rand_ref.grow(frame, rand_ref.dist2(reach))


def test_the_seeded_sequences_show_what_they_are_named_for():
    import functions
    tr = {name: functions.tracks_from_links(ref.links(m, m)[:3]) for name, m in ref.sequences()}
    assert tr["drift"].table.tolist() == [[k, 0, 4, 0] for k in range(1, 7)]
    assert tr["merge"].table.tolist() == [[1, 0, 3, 0], [2, 0, 1, 0]]
    assert tr["vanish"].table.tolist() == [[1, 0, 3, 0], [2, 0, 1, 0], [3, 2, 3, 0]]
    assert tr["empty middle"].table.tolist() == [[1, 0, 1, 0], [2, 0, 1, 0], [3, 3, 4, 0], [4, 3, 4, 0]]
    assert tr["tie 3 8"].table.tolist() == tr["tie 8 3"].table.tolist() == [[1, 0, 1, 0], [2, 0, 0, 0]]
    assert tr["sparse"].track_of.shape == (2, 70002) and len(tr["sparse"].table) == 5 and (tr["sparse"].table[:, 2] == 1).all()
    assert (tr["cells"].table[:, 3] > 0).any() and (tr["cells"].table[:, 2] < 5).any()


def test_ctc_text_round_trips():
    import functions
    m = ref.dividing_discs()
    t = functions.tracks_from_links(ref.links(m, m)[:3])
    text = t.ctc_text()
    assert text.endswith("\n") and text.splitlines()[2] == "3 2 3 2"
    assert np.array_equal(np.loadtxt(io.StringIO(text), dtype=np.int64, ndmin=2), t.table)
    one = functions.tracks_from_links(rows([(5, 0, 0)]))
    assert one.ctc_text() == "1 0 0 0\n"
