"""The challenge's DET / TRA measures without a GPU: the C ABI and the Python surface of ctc.py are there, every refusal of the
host is worded, ctc.aogm_from_counts gives hand-made scores, and the restatement tests/ctc_ref.py (what the GPU tests compare
the device with) gives the hand-worked answers of the mother-and-two-daughters example and of every edge rule."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ctc_ref as ref
import track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_aogm_counts_scratch_bytes", "unet_aogm_counts")
DEVICE_OPS = ("aogm_counts", "det_measure", "tra_measure")
REFUSAL = ("aogm_counts runs on the HIP device only (unet_aogm_counts): move the input to the device first, e.g. with .cuda(); "
           "there is no CPU implementation")


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
    assert len(_hip._SIGS["unet_aogm_counts"][1]) == 17 and len(_hip._SIGS["unet_aogm_counts_scratch_bytes"][1]) == 3
    assert L.unet_abi_version() == 4
    for bad in ((0, 5, 5), (65536, 5, 5), (3, -1, 5), (3, 5, -1), (3, 1 << 24, 5), (3, 5, 1 << 24)):
        assert L.unet_aogm_counts_scratch_bytes(*bad) == 0, bad
    assert L.unet_aogm_counts_scratch_bytes(3, 10, 20) >= 4 * (3 * 11 + 3 * 21 + 11 + 21)
    assert L.unet_aogm_counts_scratch_bytes(1, 0, 0) > 0
    for bit in ("1 = present", "2 = has an in-edge", "4 = that edge is of kind parent", "8 = bad", "16 = matched", "32 = EA", "64 = EC",
                "16 = TP", "32 = FP", "64 = ED"):
        assert bit in hdr, bit


def test_every_launching_function_of_ctc_refuses_host_tensors():
    """functions.py's rule (tests/test_functions_errors_cpu.py), held to ctc.py: a public function whose source launches, directly
    or through aogm_counts, is in DEVICE_OPS, and each of them ends at the standard refusal on host tensors."""
    import ctc
    public = [k for k, v in vars(ctc).items() if inspect.isfunction(v) and v.__module__ == ctc.__name__ and not k.startswith("_")]
    launching = [k for k in public
                 if re.search(r"_hip\.run|_table_call|_overlap_call|_link_frames\(|aogm_counts\(", inspect.getsource(getattr(ctc, k)))]
    assert sorted(launching) == sorted(DEVICE_OPS)
    z = torch.zeros(3, 4, 4, dtype=torch.int32)
    table = np.zeros((0, 4), np.int64)
    for call in (lambda: ctc.aogm_counts(z, z), lambda: ctc.aogm_counts(z.long(), z, table, None, return_vertices=True),
                 lambda: ctc.det_measure(z, z), lambda: ctc.tra_measure(z, table, z, table)):
        with pytest.raises(NotImplementedError) as caught:
            call()
        assert str(caught.value) == REFUSAL


ERRORS = [
    ("shapes differ", lambda c, z: c.aogm_counts(z, z[:, :3]), "aogm_counts takes id maps of equal shape [H,W] or [B,H,W], got (3, 4, 4), (3, 3, 4)"),
    ("not 3-D", lambda c, z: c.aogm_counts(z[0], z[0]), "aogm_counts takes two time-lapses of id maps [T,H,W], got (4, 4)"),
    ("4-D", lambda c, z: c.det_measure(z[None], z[None]), "aogm_counts takes two time-lapses of id maps [T,H,W], got (1, 3, 4, 4)"),
    ("a float map", lambda c, z: c.aogm_counts(z, z.float()), "aogm_counts takes int32 or int64 id maps, got torch.float32"),
    ("T > 65535", lambda c, z: c.det_measure(torch.zeros(65536, 1, 1, dtype=torch.int32), torch.zeros(65536, 1, 1, dtype=torch.int32)),
     "aogm_counts: at most 65535 frames, got 65536"),
    ("duplicate L", lambda c, z: c.aogm_counts(z, z, [[1, 0, 1, 0], [2, 0, 1, 0], [2, 1, 1, 0]]), "aogm_counts: res_tracks lists label 2 more than once"),
    ("B > E", lambda c, z: c.tra_measure(z, [[1, 0, 1, 0]], z, [[1, 0, 1, 0], [5, 2, 1, 0]]), "aogm_counts: gt_tracks has B > E for label 5"),
    ("P = L", lambda c, z: c.aogm_counts(z, z, None, "3 0 1 3\n"), "aogm_counts: gt_tracks makes label 3 its own parent"),
    ("unknown P", lambda c, z: c.aogm_counts(z, z, "1 0 1 0\n2 2 3 7\n"), "aogm_counts: res_tracks names a parent 7 that is no listed label"),
    ("label 0", lambda c, z: c.aogm_counts(z, z, [[0, 0, 1, 0]]), "aogm_counts: res_tracks holds a label outside [1, 2^24)"),
    ("label 2^24", lambda c, z: c.aogm_counts(z, z, [[1 << 24, 0, 1, 0]]), "aogm_counts: res_tracks holds a label outside [1, 2^24)"),
    ("negative frame", lambda c, z: c.aogm_counts(z, z, None, [[1, -1, 1, 0]]), "aogm_counts: gt_tracks holds a frame outside [0, 2^31)"),
    ("a float table", lambda c, z: c.aogm_counts(z, z, np.zeros((2, 4))), "tracks_table takes text, a Tracks or an integer array [n,4], got float64 (2, 4)"),
    ("three columns", lambda c, z: c.aogm_counts(z, z, np.zeros((2, 3), np.int64)), "tracks_table takes text, a Tracks or an integer array [n,4], got int64 (2, 3)"),
    ("a short line", lambda c, z: c.tracks_table("1 0 1 0\n2 0 1\n"), "tracks_table: line 2 is not `L B E P`: '2 0 1'"),
    ("a word", lambda c, z: c.tracks_table("1 0 x 0\n"), "tracks_table: line 1 is not `L B E P`: '1 0 x 0'"),
    ("weights", lambda c, z: c.aogm_from_counts(c.AogmCounts(*[[0]] * 12), {"tp": 1}), "aogm_from_counts: weights takes finite numbers >= 0 for ns, fn, fp, ed, ea, ec, got 'tp': 1"),
]


@pytest.mark.parametrize("what, call, message", ERRORS, ids=[e[0] for e in ERRORS])
def test_the_value_errors(what, call, message):
    """All of them on host tensors: the refusal of the arguments comes before the refusal of the device."""
    import ctc
    with pytest.raises(ValueError) as caught:
        call(ctc, torch.zeros(3, 4, 4, dtype=torch.int32))
    assert str(caught.value) == message


def test_tracks_table_round_trips():
    import ctc
    import functions
    m = track_ref.dividing_discs()
    tracks = functions.tracks_from_links(track_ref.links(m, m)[:3])
    text = tracks.ctc_text()
    for given in (text, text.encode(), tracks, tracks.table, tracks.table.astype(np.int32), torch.from_numpy(tracks.table), "\n" + text + "\n"):
        got = ctc.tracks_table(given)
        assert got.dtype == np.int64 and np.array_equal(got, tracks.table)
    assert ctc.tracks_table("").shape == (0, 4) and ctc.tracks_table(np.zeros((0, 4), np.int64)).shape == (0, 4)
    assert ctc.tracks_table("7 0 3 0").tolist() == [[7, 0, 3, 0]]
    assert "".join("%d %d %d %d\n" % tuple(r) for r in ctc.tracks_table(text)) == text


def counts_of(**kw):
    import ctc
    return ctc.AogmCounts(*[np.array([kw.get(k, 0)]) for k in ctc.COUNT_NAMES])


def test_scores_from_hand_made_counts():
    import ctc
    assert ctc.COUNT_NAMES == ref.NAMES and ctc.AogmCounts._fields == ref.NAMES
    assert ctc.AogmScores._fields == ("tra", "det", "aogm", "aogm0", "aogm_d", "aogm_d0", "per_frame_det")
    assert ctc.WEIGHTS == {"ns": 5, "fn": 10, "fp": 1, "ed": 1, "ea": 1.5, "ec": 1}
    assert (ctc.PRESENT, ctc.HAS_EDGE, ctc.PARENT_EDGE, ctc.BAD, ctc.MATCHED, ctc.EA, ctc.EC, ctc.TP, ctc.FP, ctc.ED) == (1, 2, 4, 8, 16, 32, 64, 16, 32, 64)
    # 6 vertices, 5 edges: AOGM_0 = 60 + 7.5; NS 1, FN 2, FP 3, ED 4, EA 5, EC 6: AOGM-D = 5 + 20 + 3 = 28, AOGM = 28 + 4 + 7.5 + 6 = 45.5
    s = ctc.aogm_from_counts(counts_of(n_ref=6, e_ref=5, ns=1, fn=2, fp=3, ed=4, ea=5, ec=6))
    assert (s.aogm, s.aogm0, s.aogm_d, s.aogm_d0) == (45.5, 67.5, 28.0, 60.0)
    assert s.tra == 1 - 45.5 / 67.5 and s.det == 1 - 28 / 60 and s.per_frame_det.tolist() == [1 - 28 / 60]
    assert all(type(v) is np.float64 for v in (s.tra, s.det)) and all(type(v) is float for v in s[2:6])
    # more operations than building the reference from nothing costs: both scores clip to 0
    s = ctc.aogm_from_counts(counts_of(n_ref=1, e_ref=0, fp=11))
    assert (s.aogm, s.aogm0, s.tra, s.det) == (11.0, 10.0, 0.0, 0.0)
    s = ctc.aogm_from_counts(counts_of(n_ref=2, e_ref=1, n_res=2, ed=30))
    assert s.tra == 0.0 and s.det == 1.0
    # an empty reference has no score, whatever the result holds
    for kw in ({}, {"fp": 3, "n_res": 3}):
        s = ctc.aogm_from_counts(counts_of(**kw))
        assert np.isnan(s.tra) and np.isnan(s.det) and np.isnan(s.per_frame_det).all() and s.aogm0 == 0.0
    # per frame: frame 0 has no reference vertex, frame 1 has two of which one is missed
    c = ctc.AogmCounts(*[np.array(v) for v in ([0, 2], [1, 1], [0, 0], [0, 0], [0, 1], [0, 1], [1, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0])])
    s = ctc.aogm_from_counts(c)
    assert np.isnan(s.per_frame_det[0]) and s.per_frame_det[1] == 1 - 10 / 20 and s.det == 1 - 11 / 20 and s.tra == 1 - 11 / 20
    assert c.total() == ctc.AogmCounts(2, 2, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0) and all(type(v) is int for v in c.total())
    assert ctc.aogm_from_counts(c.total()).det == s.det
    # other weights
    s = ctc.aogm_from_counts(counts_of(n_ref=6, e_ref=5, fn=1, ea=2), {"fn": 1, "ea": 1})
    assert (s.aogm, s.aogm0, s.aogm_d0) == (3.0, 11.0, 6.0) and s.tra == 1 - 3 / 11 and s.det == 1 - 1 / 6


def test_the_combined_rankings():
    import ctc
    import functions
    assert ctc.ctc_scores(0.5) == (None, None)
    assert ctc.ctc_scores(0.5, 1.0) == (0.75, None) and ctc.ctc_scores(0.5, tra=0.25) == (None, 0.375)
    seg = functions.seg_from_counts([[0, 4]], [[0, 4]], [[0, 1]], [[0, 2]])
    scores = ctc.aogm_from_counts(counts_of(n_ref=1, e_ref=0, fp=5))
    got = ctc.ctc_scores(seg, ctc.CtcMeasure(scores.det, scores, None), ctc.CtcMeasure(scores.tra, scores, None))
    assert seg.seg == 2 / 6 and got == ((2 / 6 + 0.5) / 2, (2 / 6 + 0.5) / 2) and got._fields == ("op_csb", "op_ctb")


# ---- the restatement, by hand -------------------------------------------------------------------------------------------------
# The reference (ctc_ref.hand_reference): mother 1, a 4 x 6 box, in frames 0-1; daughters 2 and 3, 4 x 4 boxes, in frames 2-3,
# both with parent 1.  Vertices (0,1) (1,1) (2,2) (3,2) (2,3) (3,3): |V| = 6.  In-edges: (0,1)->(1,1) track, (1,1)->(2,2) and
# (1,1)->(2,3) parent, (2,2)->(3,2) and (2,3)->(3,3) track: |E| = 5.  AOGM_0 = 10 * 6 + 1.5 * 5 = 67.5, AOGM-D_0 = 60.
#
#  itself       every vertex is covered whole by its own copy, every edge is there with its kind: nothing to do.
#  empty        six vertices without a match (FN 6); none of the five edges has matched ends (EA 5).
#               AOGM-D = 60 -> DET 0; AOGM = 60 + 7.5 = 67.5 -> TRA 0.
#  label kept   result: 1 in frames 0-3 (the mother's box, then daughter 2's), 3 in frames 2-3 without parent.  All six match one to
#               one.  (1,1)->(2,2): the result's (2,1) has the in-edge from (1,1), kind track against parent: EC.  (1,1)->(2,3):
#               the result's (2,3) has no in-edge: EA.  The other three are reproduced in kind.  Result edges: (1,1)->(2,1) has the
#               partners (1,1)->(2,2), which is the reference's: no ED.  AOGM = 1.5 + 1 = 2.5.
#  merged       result: 1 in frames 0-1, one 4 x 12 box 2 over both daughters in frames 2-3 with parent 1.  It covers each daughter
#               whole, so it matches two reference vertices in each of the frames 2 and 3: NS 1 + 1 = 2, and it is no TP.  Every
#               reference edge but (0,1)->(1,1) has an end matched by it: EA 4.  Its own edges have an end that is no TP: they cost
#               nothing.  AOGM-D = 10, AOGM = 10 + 6 = 16.
#  gap          the reference with frame 1 emptied: (1,1) has no match: FN 1.  The three edges that touch (1,1) cannot be
#               reproduced: EA 3.  The result's daughters take their parent edge from the mother's last presence, (0,1): both
#               ends are TP with the partners (0,1) and (2,2) / (2,3), whose reference in-edges come from (1,1): ED 2.
#               AOGM-D = 10, AOGM = 10 + 4.5 + 2 = 16.5.
#  extra cell   a 2 x 2 cell 4 in frame 0 that touches nothing: FP 1.  AOGM-D = AOGM = 1.

HAND_SCORES = {"itself": (1.0, 1.0), "empty": (0.0, 0.0), "label kept": (1.0, 1 - 2.5 / 67.5), "merged": (1 - 10 / 60, 1 - 16 / 67.5),
               "gap": (1 - 10 / 60, 1 - 16.5 / 67.5), "extra cell": (1 - 1 / 60, 1 - 1 / 67.5)}


def test_the_hand_worked_example():
    gt, gt_table = ref.hand_reference()
    assert len(ref.hand_cases()) == 6
    for name, res, res_table, ops in ref.hand_cases():
        c = ref.compare(gt, res, gt_table, res_table)
        n = ref.totals(c)
        assert (n["n_ref"], n["e_ref"], n["bad"]) == (6, 5, 0), name
        assert {k: n[k] for k in ("fn", "fp", "ns", "ea", "ed", "ec") if n[k]} == ops, name
        s = ref.scores(n)
        assert (s["det"], s["tra"]) == HAND_SCORES[name] and s["aogm0"] == 67.5 and s["aogm_d0"] == 60.0, name
    c = ref.compare(gt, ref.hand_cases()[4][1], gt_table, gt_table)                        # where the operations of `gap` are booked
    assert c.fn == {(1, 1)} and c.ea == {(1, 1), (2, 2), (2, 3)} and c.ed == {(2, 2), (2, 3)}
    assert c.res_edge[(2, 3)] == ((0, 1), "parent") and c.gt_edge[(2, 3)] == ((1, 1), "parent")
    assert ref.counts(c)[:, [5, 8, 9]].tolist() == [[0, 0, 0], [1, 1, 0], [0, 2, 2], [0, 0, 0]]
    a = ref.arrays(c, 3, 5)
    assert a["flags_gt"].tolist() == [[0, 1 | 16, 0, 0], [0, 1 | 2 | 32, 0, 0], [0, 0, 1 | 2 | 4 | 16 | 32, 1 | 2 | 4 | 16 | 32], [0, 0, 1 | 2 | 16, 1 | 2 | 16]]
    assert a["flags_res"][2].tolist() == [0, 0, 1 | 2 | 4 | 16 | 64, 1 | 2 | 4 | 16 | 64, 0, 0] and a["inedge_res"][2, 2].tolist() == [0, 1]
    assert a["inedge_gt"][0, 1].tolist() == [-1, 0] and a["claimant"][3].tolist() == [0, 0, 2, 3, 0, 0] and a["area_gt"][1, 1] == 24


def frames(*rows):
    """[T,1,W] maps from one row of ids per frame."""
    return np.array(rows, np.int32)[:, None, :]


def test_exactly_half_is_no_match():
    gt = frames([1, 1, 1, 1, 0, 0])
    c = ref.compare(gt, frames([0, 0, 2, 2, 2, 2]))
    assert not c.match and ref.totals(c)["fn"] == 1 and ref.totals(c)["fp"] == 1
    c = ref.compare(gt, frames([0, 2, 2, 2, 2, 2]))
    assert c.match == {(0, 1): (0, 2)} and c.tp == {(0, 2)}


def test_the_parent_edge_comes_from_the_last_presence():
    """The mother's row ends in frame 2, but frame 2 holds no pixel of hers: the daughters' edges come from frame 1."""
    gt = frames([1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [2, 0, 3, 0])
    table = [[1, 0, 2, 0], [2, 3, 3, 1], [3, 3, 3, 1]]
    c = ref.compare(gt, gt, table, table)
    assert c.gt_edge[(3, 2)] == ((1, 1), "parent") and c.gt_edge[(3, 3)] == ((1, 1), "parent") and not c.gt_bad
    n = ref.totals(c)
    assert (n["n_ref"], n["e_ref"], n["tp"]) == (4, 3, 4) and not any(n[k] for k in ("fn", "fp", "ns", "ea", "ed", "ec", "bad"))


def test_a_gap_that_both_sides_share_costs_nothing():
    gt = frames([1, 1, 0], [0, 0, 0], [0, 0, 0], [1, 1, 0])
    c = ref.compare(gt, frames([5, 5, 0], [0, 0, 0], [0, 0, 0], [5, 5, 5]), [[1, 0, 3, 0]], [[5, 0, 3, 0]])
    assert c.gt_edge == {(3, 1): ((0, 1), "track")} and c.res_edge == {(3, 5): ((0, 5), "track")}
    assert ref.totals(c)["ea"] == 0 and ref.totals(c)["ed"] == 0 and ref.totals(c)["tp"] == 2
    c = ref.compare(gt, frames([5, 5, 0], [0, 0, 0], [0, 0, 5], [5, 5, 0]))         # the result closes a frame of the gap: another edge
    assert ref.totals(c)["ea"] == 1 and ref.totals(c)["fp"] == 1 and ref.totals(c)["ed"] == 0


def test_the_bad_vertices():
    gt = frames([1, 0], [1, 2], [0, 2])
    assert ref.graph(gt, [[1, 0, 1, 0], [2, 1, 2, 1]])[2] == {(1, 2)}        # the child begins in the mother's last frame
    assert ref.graph(gt, [[1, 0, 1, 0], [2, 1, 2, 0]])[2] == set()
    assert ref.graph(gt, [[1, 0, 0, 0], [2, 1, 2, 0]])[2] == {(1, 1)}        # present outside [B, E]
    assert ref.graph(gt, [[1, 1, 1, 0], [2, 1, 2, 0]])[2] == {(0, 1)}
    assert ref.graph(gt, [[2, 1, 2, 0]])[2] == {(0, 1), (1, 1)}              # no row
    assert ref.graph(gt, [[1, 0, 1, 0], [2, 1, 2, 9], [9, 0, 0, 0]])[2] == {(1, 2)}   # a parent that is never present
    assert ref.graph(gt, None)[2] == set() and ref.graph(gt, None)[1] == {(1, 1): ((0, 1), "track"), (2, 2): ((1, 2), "track")}
    c = ref.compare(gt, gt, [[2, 1, 2, 0]], [[1, 0, 1, 0], [2, 1, 2, 1]])
    assert ref.totals(c)["bad"] == 3 and ref.arrays(c, 2, 2)["flags_res"][1].tolist() == [0, 1 | 2 | 16, 1 | 8 | 16]


def test_the_seeded_tables_hold_every_kind_of_bad_vertex():
    m = ref.staggered(track_ref.random_frames(0, 3, 67, 130))
    table = ref.faulty_table(m, 0)
    v, edge, bad, _ = ref.graph(m, table)
    rows = {r[0]: r for r in table.tolist()}
    assert 0 < len(bad) < len(v) and any(k == "parent" for _, k in edge.values()) and any(k == "track" for _, k in edge.values())
    assert any(L not in rows for _, L in bad) and any(L in rows and not rows[L][1] <= t <= rows[L][2] for t, L in bad)
    assert any(L in rows and rows[L][1] <= t <= rows[L][2] and rows[L][3] for t, L in bad)                # a bad parent link
    assert ref.rows_by_label([[2, 1, 3, 1], [9, 0, 0, 0]], 3).tolist() == [[-1, 0, 0], [-1, 0, 0], [1, 3, 1], [-1, 0, 0]]
