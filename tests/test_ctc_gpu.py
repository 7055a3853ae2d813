"""The challenge's DET / TRA counting on the device (unet_aogm_counts; ctc.aogm_counts, det_measure, tra_measure) against the
restatement tests/ctc_ref.py (pinned to hand-worked answers by tests/test_ctc_cpu.py).  Everything is integers, and the scores
are float64 quotients of small integers: every comparison is exact.  Every pointer handed to the raw entry point is a poisoned
guarded.Arena buffer."""
import numpy as np
import pytest
import torch

import ctc_ref as ref
import guarded
import track_ref
from gpu_support import dev, hip, rejected  # noqa: F401
from test_ctc_cpu import HAND_SCORES

pytestmark = pytest.mark.gpu

OUTPUTS = ("claims", "claimant", "inedge_gt", "inedge_res", "flags_gt", "flags_res", "counts")
OPS = ("fn", "fp", "ns", "ea", "ed", "ec")


def perturbed(gt, seed, sparse=False):
    """A result for the reference gt: moved one pixel to the right, the labels dealt anew (dense: 3, 4, ...; sparse: among
    themselves), two labels merged in the last frame and one cell missing in the first."""
    rs = np.random.RandomState(300 + seed)
    ids = np.unique(gt[gt > 0])
    if not len(ids):
        return np.roll(gt, 1, axis=2)
    new = rs.permutation(ids) if sparse else rs.permutation(len(ids)) + 3
    lut = np.zeros(int(ids.max()) + 1, np.int32)
    lut[ids] = new
    res = lut[np.roll(gt, 1, axis=2)]
    if len(ids) >= 2:
        res[-1][res[-1] == new[0]] = new[1]
    if len(ids) >= 3:
        res[0][res[0] == new[2]] = 0
    return res


def long_sparse():
    """T = 8 of track_ref.sparse_ids (labels up to 70001): T * (n_max + 1) = 560 016 vertices' worth of words per side, more than
    the 2048 * 256 = 524 288 threads of a capped grid: the kernels' loops iterate."""
    m = np.concatenate([track_ref.sparse_ids()] * 4)
    assert m.shape[0] == 8 and m.max() == 70001 and 8 * 70002 > 2048 * 256
    return m


def tracked_on_the_host(maps):
    """(maps labelled by track, table) of a time-lapse of instance maps by the restatement of the tracker (track_ref)."""
    area, pred, over, _, _ = track_ref.links(maps, maps)
    table, track_of = track_ref.tracks(area, pred, over)
    return track_ref.remap(maps, track_of), table


def raw_cases():
    """name -> (gt, res, [(gt_table, res_table)]): None tables always, the seeded faulty ones, for the hand cases their own, and
    two tracked sequences with the tables of their tracks (parent links on both sides)."""
    out = {}
    for name, m in (("4x40x72 divide", track_ref.dividing_discs()), ("6x96x120 cells", track_ref.shifted_cells(5, 6, 96, 120, 20))):
        (gt, gt_table), (res, res_table) = tracked_on_the_host(m), tracked_on_the_host(perturbed(m, 5))
        out[name] = (gt, res, [(gt_table, res_table), (res_table, gt_table)])
    one = np.ones((1, 1, 1), np.int32)
    out["1x1x1"] = (one, one, [([[1, 0, 0, 0]], [[1, 0, 0, 0]])])
    out["1x1x1 empty result"] = (one, 0 * one, [([[1, 0, 0, 0]], np.zeros((0, 4), np.int64))])
    two = np.array([1, 1], np.int32).reshape(2, 1, 1)
    out["2x1x1"] = (two, np.array([2, 0], np.int32).reshape(2, 1, 1), [([[1, 0, 1, 0]], [[2, 0, 0, 0]]), ([[1, 1, 1, 0]], None)])
    gt, gt_table = ref.hand_reference()
    for name, res, res_table, _ in ref.hand_cases():
        out["hand " + name] = (gt, res, [(gt_table, res_table), (None, res_table), (res_table, gt_table)])
    for name, m, sparse in (("3x5x17", ref.staggered(track_ref.random_frames(0, 3, 5, 17)), False),
                            ("5x48x72 discs", track_ref.drifting_discs(shuffle=False), False),
                            ("3x67x130", ref.staggered(track_ref.random_frames(0, 3, 67, 130)), False),
                            ("8x33x31 sparse", long_sparse(), True)):
        res = perturbed(m, len(out), sparse)
        out[name] = (m, res, [(ref.faulty_table(m, 1), ref.faulty_table(res, 2)), (ref.table_of(m), None)])
    return out


RAW = raw_cases()


def raw_aogm(dev, want, rows_gt, rows_res, T, ng_max, nr_max, zeroed=False):
    """unet_aogm_counts on guarded buffers, the inputs from the restatement's arrays (with something in the areas' column 0, as
    unet_instance_overlap leaves the background there): the seven outputs as device tensors, and the arena."""
    import _hip
    a = guarded.Arena(dev)

    def put(x, label):
        return None if x is None else a.inp(torch.from_numpy(np.ascontiguousarray(x, np.int32)), label)

    area_gt, area_res = want["area_gt"].copy(), want["area_res"].copy()
    area_gt[:, 0], area_res[:, 0] = 7, 9
    ins = [put(area_gt, "area_gt"), put(area_res, "area_res"), put(want["match"], "match"), put(rows_gt, "rows_gt"), put(rows_res, "rows_res")]
    outs = [a.out((T, nr_max + 1), torch.int32, "claims"), a.out((T, nr_max + 1), torch.int32, "claimant"),
            a.out((T, ng_max + 1, 2), torch.int32, "inedge_gt"), a.out((T, nr_max + 1, 2), torch.int32, "inedge_res"),
            a.out((T, ng_max + 1), torch.uint8, "flags_gt"), a.out((T, nr_max + 1), torch.uint8, "flags_res"),
            a.out((T, 12), torch.int64, "counts")]
    if zeroed:
        for o in outs:
            o.zero_()
    scratch = a.scratch(_hip.lib().unet_aogm_counts_scratch_bytes(T, ng_max, nr_max), "scratch")
    _hip.run("unet_aogm_counts", dev, *(a.ptr(i) for i in ins), T, ng_max, nr_max, *(a.ptr(o) for o in outs), a.ptr(scratch))
    torch.cuda.synchronize()
    if zeroed:
        a.check()
    else:
        a.verify(outs[0], outs[1], outs[4], outs[5], outs[6])    # an in-edge of (-1, 0) is poison's own bytes: the zeroed run holds those
    return outs


def same_arrays(got, want, what):
    for k, g in zip(OUTPUTS, got):
        g = g.cpu().numpy().astype(np.int64)
        assert g.shape == want[k].shape and np.array_equal(g, want[k]), (what, k, np.argwhere(g != want[k])[:4].tolist())


@pytest.mark.parametrize("name", list(RAW))
def test_every_output_equals_the_restatement(dev, name):
    """With every pair of tables of the case and with none, with the exact id maxima and with slack on either side; each time a
    second run on zeroed instead of poisoned outputs leaves the same bytes: every word is written, and in every run alike."""
    gt, res, tables = RAW[name]
    T = len(gt)
    slack = [(0, 0), (5, 0)] if gt.max() < 1000 else [(0, 3)]
    n_bad, differ = 0, False
    for gt_table, res_table in [(None, None)] + tables:
        c = ref.compare(gt, res, gt_table, res_table)
        n_bad += len(c.gt_bad) + len(c.res_bad)
        for dg, dr in slack:
            ng_max, nr_max = int(gt.max()) + dg, int(res.max()) + dr
            differ |= ng_max != nr_max
            want = ref.arrays(c, ng_max, nr_max)
            rows = [None if t is None else ref.rows_by_label(t, n) for t, n in ((gt_table, ng_max), (res_table, nr_max))]
            first = raw_aogm(dev, want, *rows, T, ng_max, nr_max)
            same_arrays(first, want, (name, gt_table is None, res_table is None, dg))
            again = raw_aogm(dev, want, *rows, T, ng_max, nr_max, zeroed=True)
            for k, x, y in zip(OUTPUTS, first, again):
                assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (name, k)
    assert differ, "ng_max != nr_max at least once"
    if name in ("3x67x130", "5x48x72 discs", "8x33x31 sparse"):
        n = ref.totals(c)
        assert n["tp"] > 3 and n["fn"] and n["ns"] and n["ea"] and n["e_res"] > 3, "the case shows what it is there for"
    if name == "3x67x130":
        assert n_bad > 3


def test_a_rejected_call_writes_nothing(dev, hip):
    a = guarded.Arena(dev)
    T, ng, nr = 2, 3, 4
    ins = [a.inp(torch.zeros(T, ng + 1, dtype=torch.int32), "area_gt"), a.inp(torch.zeros(T, nr + 1, dtype=torch.int32), "area_res"),
           a.inp(torch.zeros(T, ng + 1, dtype=torch.int32), "match")]
    outs = [a.out((T, nr + 1), torch.int32, "claims"), a.out((T, nr + 1), torch.int32, "claimant"), a.out((T, ng + 1, 2), torch.int32, "inedge_gt"),
            a.out((T, nr + 1, 2), torch.int32, "inedge_res"), a.out((T, ng + 1), torch.uint8, "flags_gt"),
            a.out((T, nr + 1), torch.uint8, "flags_res"), a.out((T, 12), torch.int64, "counts")]
    L = hip.lib()
    scratch = a.scratch(L.unet_aogm_counts_scratch_bytes(T, ng, nr), "scratch")

    def call(T=T, ng=ng, nr=nr, null_in=None, null_out=None, no_scratch=False):
        i = [None if k == null_in else a.ptr(x) for k, x in enumerate(ins)]
        o = [None if k == null_out else a.ptr(x) for k, x in enumerate(outs)]
        return L.unet_aogm_counts(*i, None, None, T, ng, nr, *o, None if no_scratch else a.ptr(scratch), None)

    refused = [({"null_in": k}, b"bad argument") for k in range(3)] + [({"null_out": k}, b"bad argument") for k in range(7)]
    refused += [({"no_scratch": True}, b"bad argument"), ({"T": 0}, b"65535"), ({"T": 65536}, b"65535"), ({"T": -1}, b"65535"),
                ({"ng": 1 << 24}, b"ng_max"), ({"nr": 1 << 24}, b"nr_max"), ({"ng": -1}, b"ng_max"), ({"nr": -1}, b"nr_max")]
    for kw, words in refused:
        rejected(hip, call(**kw), a, *outs, scratch)
        assert words in L.unet_last_error(), kw
    assert call() == 0
    torch.cuda.synchronize()
    a.verify(outs[0], outs[1], outs[4], outs[5], outs[6])
    assert not outs[6].any() and (outs[2][..., 0] == -1).all() and not outs[3][..., 1].any()


# ---- the public functions -------------------------------------------------------------------------------------------------------

def on(dev, *maps):
    return tuple(torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in maps)


def same_counts(got, c, what):
    want = ref.counts(c)
    for k, name in enumerate(ref.NAMES):
        g = getattr(got, name)
        assert g.dtype == np.int64 and g.shape == (c.T,) and np.array_equal(g, want[:, k]), (what, name, g.tolist(), want[:, k].tolist())


def test_the_hand_worked_example(dev):
    import ctc
    gt, gt_table = ref.hand_reference()
    for name, res, res_table, ops in ref.hand_cases():
        r, g = on(dev, res, gt)
        tra = ctc.tra_measure(r, res_table, g.long(), gt_table)
        n = tra.counts.total()
        assert {k: getattr(n, k) for k in OPS if getattr(n, k)} == ops and (n.n_ref, n.e_ref, n.bad) == (6, 5, 0), name
        assert (tra.scores.det, tra.scores.tra) == HAND_SCORES[name] and tra.value == tra.scores.tra, name
        assert (tra.scores.aogm0, tra.scores.aogm_d0) == (67.5, 60.0)
        det = ctc.det_measure(r, g)
        assert det.value == HAND_SCORES[name][0] and det.value == det.scores.det, name
        assert all(getattr(det.counts.total(), k) == getattr(n, k) for k in ("n_ref", "n_res", "tp", "fn", "fp", "ns")), name
        same_counts(tra.counts, ref.compare(gt, res, gt_table, res_table), name)


SEQUENCES = dict(track_ref.sequences())


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_tracked_sequences(dev, name):
    """track_cells' own result against itself is perfect; against itself with the middle frame emptied, either way round, it is what
    the restatement says (a ValueError where emptying the frame leaves a child whose parent is never present)."""
    import ctc
    import functions
    (labels,) = on(dev, SEQUENCES[name])
    maps, tracks = functions.track_cells(labels)
    got = ctc.tra_measure(maps, tracks, maps, tracks)
    n = got.counts.total()
    assert got.value == 1.0 and got.scores.det == 1.0 and got.scores.aogm == 0.0 and n.n_ref == n.n_res == n.tp > 0
    assert not any(getattr(n, k) for k in OPS + ("bad",)) and n.e_ref == n.e_res == n.n_ref - (tracks.table[:, 3] == 0).sum()
    full = maps.cpu().numpy()
    cut = full.copy()
    cut[len(cut) // 2] = 0
    (cut_dev,) = on(dev, cut)
    for res, gt, res_dev, gt_dev in ((cut, full, cut_dev, maps), (full, cut, maps, cut_dev)):
        c = ref.compare(gt, res, tracks.table, tracks.table)
        if c.gt_bad or c.res_bad:
            with pytest.raises(ValueError, match="aogm_counts: %d vertices are bad" % (len(c.gt_bad) + len(c.res_bad))):
                ctc.aogm_counts(res_dev, gt_dev, tracks, tracks)
            continue
        counts, v = ctc.aogm_counts(res_dev, gt_dev, tracks, tracks.ctc_text(), return_vertices=True)
        same_counts(counts, c, name)
        same_arrays([torch.from_numpy(x) for x in v] + [torch.from_numpy(np.stack(counts, axis=1))], ref.arrays(c, int(gt.max()), int(res.max())), name)
        s, want = ctc.aogm_from_counts(counts), ref.scores(ref.totals(c))
        assert (s.tra, s.det, s.aogm, s.aogm0) == (want["tra"], want["det"], want["aogm"], want["aogm0"]), name


def test_detection_counts_agree_with_seg_measure(dev):
    """FN is seg_measure's n_gt - n_matched, and FP and NS follow from a host bincount of unet_instance_overlap's match."""
    import _hip
    import ctc
    import functions
    gt = track_ref.shifted_cells(5, 6, 96, 120, 20)
    res = perturbed(gt, 0)
    res[2][(res[2] > 0) & (res[2] < 9)] = 5                                 # a frame with a large merge
    r, g = on(dev, res, gt)
    det, seg = ctc.det_measure(r, g), functions.seg_measure(r, g)
    n = det.counts.total()
    assert n.fn == seg.n_gt - seg.n_matched and n.n_ref == seg.n_gt and n.n_res == seg.n_pred and n.fn > 0
    T, H, W = gt.shape
    ng, nr, slots = int(gt.max()), int(res.max()), 1 << 14
    outs = [torch.empty(T, k + 1, dtype=torch.int32, device=dev) for k in (ng, nr, ng, ng)]
    status = torch.empty(T, 2, dtype=torch.int64, device=dev)
    _hip.run("unet_instance_overlap", dev, _hip.ptr(g), _hip.ptr(r), T, H, W, ng, nr, slots, *(_hip.ptr(o) for o in outs), _hip.ptr(status),
             _hip.ptr(_hip.scratch("unet_instance_overlap", dev, T, ng, nr, slots)))
    assert not status.cpu().numpy().any()
    area_res, match = outs[1].cpu().numpy(), outs[2].cpu().numpy()
    claims = np.stack([np.bincount(m[m > 0], minlength=nr + 1) for m in match])
    present = area_res > 0
    present[:, 0] = False
    assert det.counts.fp.tolist() == (present & (claims == 0)).sum(axis=1).tolist() and n.fp > 0
    assert det.counts.ns.tolist() == np.maximum(claims - 1, 0).sum(axis=1).tolist() and det.counts.ns[2] >= 3
    assert det.counts.tp.tolist() == (present & (claims == 1)).sum(axis=1).tolist()
    assert ctc.ctc_scores(seg, det).op_csb == (seg.seg + det.value) / 2


def test_a_table_that_must_double_gives_the_same_counts(dev):
    import ctc
    gt = track_ref.shifted_cells(5, 6, 96, 120, 20)
    res = perturbed(gt, 1)
    both = (gt > 0) & (res > 0)
    frame = np.broadcast_to(np.arange(len(gt))[:, None, None], gt.shape)
    assert len(np.unique(np.stack([frame[both], gt[both], res[both]]), axis=1).T) > 64, "more distinct (t, g, s) than two tables of 32 hold"
    r, g = on(dev, res, gt)
    small, plain = ctc.aogm_counts(r, g, _table_slots=32), ctc.aogm_counts(r, g)
    assert all(np.array_equal(a, b) for a, b in zip(small, plain))
    same_counts(small, ref.compare(gt, res), "32 slots")


# ---- metamorphic ----------------------------------------------------------------------------------------------------------------

def tracked(dev, name):
    """A reference with parent links (track_cells of a sequence) and a perturbed result with its own tracks."""
    import functions
    (labels,) = on(dev, SEQUENCES[name])
    gt, gt_tracks = functions.track_cells(labels)
    (moved,) = on(dev, perturbed(SEQUENCES[name], 4))
    res, res_tracks = functions.track_cells(moved)
    return gt.cpu().numpy(), gt_tracks.table, res.cpu().numpy(), res_tracks.table


def counts_of(dev, res, res_table, gt, gt_table):
    import ctc
    r, g = on(dev, res, gt)
    return np.stack(ctc.aogm_counts(r, g, res_table, gt_table), axis=1)


@pytest.mark.parametrize("name", ["divide", "cells"])
def test_relations(dev, name):
    gt, gt_table, res, res_table = tracked(dev, name)
    base = counts_of(dev, res, res_table, gt, gt_table)
    assert base[:, ref.NAMES.index("e_ref")].sum() > 0 and (gt_table[:, 3] > 0).any() and base[:, 5:11].sum() > 0
    assert np.array_equal(base, ref.counts(ref.compare(gt, res, gt_table, res_table)))
    # the result's labels permuted, its table alike
    n = int(res.max())
    perm = np.concatenate([[0], np.random.RandomState(8).permutation(n) + 1 + 11]).astype(np.int32)
    table = res_table.copy()
    table[:, 0], table[:, 3] = perm[table[:, 0]], perm[table[:, 3]]
    assert np.array_equal(counts_of(dev, perm[res], table, gt, gt_table), base)
    # H and W exchanged
    assert np.array_equal(counts_of(dev, res.transpose(0, 2, 1), res_table, gt.transpose(0, 2, 1), gt_table), base)
    # two sequences side by side with disjoint labels: the sum of their counts
    gt2, gt_table2, res2, res_table2 = tracked(dev, "merge")
    T, H = max(len(gt), len(gt2)), max(gt.shape[1], gt2.shape[1])

    def beside(a, ta, b, tb):
        off = int(a.max()) + 5
        both = np.zeros((T, H, a.shape[2] + b.shape[2]), np.int32)
        both[:len(a), :a.shape[1], :a.shape[2]] = a
        both[:len(b), :b.shape[1], a.shape[2]:] = np.where(b > 0, b + off, 0)
        tb = tb.copy()
        tb[:, 0] += off
        tb[:, 3] = np.where(tb[:, 3] > 0, tb[:, 3] + off, 0)
        return both, np.concatenate([ta, tb])

    other = counts_of(dev, res2, res_table2, gt2, gt_table2)
    total = np.zeros((T, 12), np.int64)
    total[:len(base)] += base
    total[:len(other)] += other
    assert np.array_equal(counts_of(dev, *beside(res, res_table, res2, res_table2), *beside(gt, gt_table, gt2, gt_table2)), total)


# ---- refusals that only the device can make ---------------------------------------------------------------------------------------

BAD_TABLES = [("no row", [[2, 1, 2, 0]], 2), ("outside [B, E]", [[1, 0, 0, 0], [2, 1, 2, 0]], 1),
              ("a parent that is never present", [[1, 0, 1, 0], [2, 1, 2, 9], [9, 0, 0, 0]], 1),
              ("a parent that is there when the child begins", [[1, 0, 1, 0], [2, 1, 2, 1]], 1)]


@pytest.mark.parametrize("what, table, n", BAD_TABLES, ids=[b[0] for b in BAD_TABLES])
def test_bad_tables_raise_from_the_device_count(dev, what, table, n):
    import ctc
    maps = np.array([[1, 0], [1, 2], [0, 2]], np.int32)[:, None, :]
    good = [[1, 0, 1, 0], [2, 1, 2, 0]]
    (m,) = on(dev, maps)
    assert ctc.tra_measure(m, good, m, good).value == 1.0
    assert len(ref.graph(maps, table)[2]) == n
    for kw in ({"res_tracks": table, "gt_tracks": good}, {"res_tracks": None, "gt_tracks": table}):
        with pytest.raises(ValueError, match="aogm_counts: %d vertices are bad" % n):
            ctc.aogm_counts(m, m, **kw)
    with pytest.raises(ValueError, match="aogm_counts: %d vertices are bad" % (2 * n)):
        ctc.tra_measure(m, table, m.long(), table)


def test_errors_on_the_device(dev):
    import ctc
    z = torch.zeros(2, 3, 5, dtype=torch.int32, device=dev)
    got = ctc.tra_measure(z, None, z, None)
    assert np.isnan(got.value) and np.isnan(got.scores.det) and got.counts.total() == ctc.AogmCounts(*[0] * 12)
    neg = z.clone()
    neg[1, 2, 4] = -3
    with pytest.raises(ValueError, match="negative ids"):
        ctc.det_measure(z, neg)
    big = z.long()
    big[0, 0, 0] = 1 << 24
    with pytest.raises(ValueError, match="below 2\\^24"):
        ctc.det_measure(big, z.long())
    with pytest.raises(NotImplementedError, match="HIP device only"):
        ctc.det_measure(z, z.cpu())
