"""The Cell Tracking Challenge's technical measures of a tracking result: DET and TRA next to functions.seg_measure's SEG, and
the challenge's combined rankings OP_CSB = (SEG + DET) / 2 and OP_CTB = (SEG + TRA) / 2.

Both measures are normalised AOGM costs (Matula et al. 2015, "Cell tracking accuracy measurement based on comparison of acyclic
oriented graphs"): the weighted number of operations that turn the result's graph into the reference's.  The definition in
full is DESIGN.md section 4s-ter; in short, for two time-lapses of id maps labelled by track and their `L B E P` tables:

  vertex    (t, L) with at least one pixel of id L in frame t
  in-edge   from L's latest presence before t (kind track; it spans a gap), else at L's first presence with P > 0 from the last
            presence of P (kind parent), else none
  match     per frame, reference vertex g is matched by result vertex s iff 2 |g n s| > |g|; s is TP iff it matches exactly one
  FN, FP, NS  reference vertices without a match; result vertices that match none; sum of (matches - 1) over those with several
  EA, EC    reference in-edges u -> v that are not reproduced (match(v) = s and match(u) = r both TP and the in-edge of s comes
            from r); reproduced ones whose two kinds differ
  ED        result in-edges r -> s with both ends TP whose partners are not joined by the reference in-edge of s's partner

The per-pixel half is functions.seg_measure's (unet_instance_overlap with one image per frame); the per-vertex graph stage runs
on the device as well (unet_aogm_counts), and only the [T][12] counters come back.  Agreement with the challenge's own evaluation
program has not been checked: it is not available here."""
import collections

import numpy as np
import torch

from functions import MAX_FRAMES, Tracks, _id_maps, _id_range, _overlap_call, _status_words

COUNT_NAMES = ("n_ref", "n_res", "e_ref", "e_res", "tp", "fn", "fp", "ns", "ea", "ed", "ec", "bad")
WEIGHTS = {"ns": 5.0, "fn": 10.0, "fp": 1.0, "ed": 1.0, "ea": 1.5, "ec": 1.0}

# the bits of a vertex's flag byte (include/unet_hip.h): both sides, the reference's, the result's
PRESENT, HAS_EDGE, PARENT_EDGE, BAD = 1, 2, 4, 8
MATCHED, EA, EC = 16, 32, 64
TP, FP, ED = 16, 32, 64


class AogmCounts(collections.namedtuple("AogmCounts", COUNT_NAMES)):
    """Twelve int64 arrays [T], one value per frame: the vertices and in-edges of the reference and of the result (an edge is
    booked to the frame of its head), the TP result vertices, the six operation counts, and the bad vertices."""
    __slots__ = ()

    def total(self):
        """The same twelve summed over the frames, as Python ints."""
        return AogmCounts(*(int(np.asarray(a).sum()) for a in self))


AogmVertices = collections.namedtuple("AogmVertices", "claims claimant gt_inedge res_inedge gt_flags res_flags")
AogmScores = collections.namedtuple("AogmScores", "tra det aogm aogm0 aogm_d aogm_d0 per_frame_det")
CtcMeasure = collections.namedtuple("CtcMeasure", "value scores counts")
CtcScores = collections.namedtuple("CtcScores", "op_csb op_ctb")


def tracks_table(table):
    """The challenge's track table as int64 [n,4], rows `L B E P` with frames as the file counts them: from the text of a
    man_track.txt / res_track.txt (str or bytes; what Tracks.ctc_text() writes), a functions.Tracks, or an integer array
    [n,4].  Empty text gives [0,4].  A line that is not four integers, or an array of another shape or dtype, raises ValueError."""
    if isinstance(table, Tracks):
        table = table.table
    if isinstance(table, bytes):
        table = table.decode("ascii")
    if isinstance(table, str):
        rows = []
        for no, line in enumerate(table.splitlines(), 1):
            words = line.split()
            if not words:
                continue
            try:
                row = [int(w) for w in words]
            except ValueError:
                row = []
            if len(row) != 4:
                raise ValueError("tracks_table: line %d is not `L B E P`: %r" % (no, line))
            rows.append(row)
        return np.array(rows, np.int64).reshape(-1, 4)
    a = table.detach().cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
    if a.ndim != 2 or a.shape[1] != 4 or a.dtype.kind not in "iu":
        raise ValueError("tracks_table takes text, a Tracks or an integer array [n,4], got %s %s" % (a.dtype, a.shape))
    return a.astype(np.int64)


def _checked_table(name, which, table):
    """None, or the table as int64 [n,4] with what the host refuses refused: labels outside [1, 2^24), frames outside
    [0, 2^31), duplicate L, B > E, P = L, a P that is no listed label."""
    if table is None:
        return None
    t = tracks_table(table)
    L, B, E, P = t.T
    if len(t) and (L.min() < 1 or L.max() >= 1 << 24):
        raise ValueError("%s: %s holds a label outside [1, 2^24)" % (name, which))
    if len(t) and (min(B.min(), E.min()) < 0 or max(B.max(), E.max()) >= 1 << 31):
        raise ValueError("%s: %s holds a frame outside [0, 2^31)" % (name, which))
    labels, times = np.unique(L, return_counts=True)
    if (times > 1).any():
        raise ValueError("%s: %s lists label %d more than once" % (name, which, int(labels[times > 1][0])))
    if (B > E).any():
        raise ValueError("%s: %s has B > E for label %d" % (name, which, int(L[B > E][0])))
    if (P == L).any():
        raise ValueError("%s: %s makes label %d its own parent" % (name, which, int(L[P == L][0])))
    unknown = (P != 0) & ~np.isin(P, L)
    if unknown.any():
        raise ValueError("%s: %s names a parent %d that is no listed label" % (name, which, int(P[unknown][0])))
    return t


def _device_rows(table, n_max, dev):
    """The rows (B, E, P) by label as the library reads them: int32 [n_max+1][3] on the device, B = -1 where a label has no row;
    None for no table.  A label above n_max is in no frame: its row is not needed (as a parent it is one that is never present)."""
    if table is None:
        return None
    rows = np.zeros((n_max + 1, 3), np.int32)
    rows[:, 0] = -1
    t = table[table[:, 0] <= n_max]
    rows[t[:, 0]] = t[:, 1:]
    return torch.from_numpy(rows).to(dev)


def aogm_counts(res_maps, gt_maps, res_tracks=None, gt_tracks=None, *, return_vertices=False, _table_slots=None):
    """The per-frame counts behind DET and TRA of a tracking result against a reference: res_maps, gt_maps int32 / int64 id maps
    [T,H,W] of one shape on a HIP device, labelled by track (0 = background, ids in [1, 2^24), T <= 65535), e.g. track_cells'
    track_maps against the challenge's man_track stack; res_tracks, gt_tracks their tables as tracks_table takes them (frames
    counted from 0), or None: no parent links, and every label in the maps is accepted.
    Returns AogmCounts; with return_vertices=True (AogmCounts, AogmVertices): claims, claimant [T][nr_max+1], the in-edge sources
    [T][n_max+1][2] as (frame, label) or (-1, 0), and the flag bytes [T][n_max+1] (the bits are this module's PRESENT .. ED) of
    both sides, as numpy arrays.
    The majority matching runs as seg_measure's does (unet_instance_overlap with one image per frame; the two id maxima are read
    back once, and the pair table is doubled and the call repeated while it overflows), the graph stage behind it on the same
    stream (unet_aogm_counts); only the [T][12] counters are read back unless the vertices are asked for.
    ValueError: maps that are not [T,H,W] of one shape, another dtype, T > 65535, negative ids or ids >= 2^24; a table with a
    duplicate L, B > E, P = L or a P that is no listed label (before anything is launched); and, from the device's count, bad
    vertices: a label in the maps without a row, a presence outside [B, E], a parent that is never present or whose last
    presence is not before the child's first.  Host tensors raise NotImplementedError (no CPU path)."""
    name = "aogm_counts"
    for m in (res_maps, gt_maps):
        if torch.is_tensor(m) and m.dim() != 3:
            raise ValueError("%s takes two time-lapses of id maps [T,H,W], got %s" % (name, tuple(m.shape)))
        if torch.is_tensor(m) and m.shape[0] > MAX_FRAMES:
            raise ValueError("%s: at most %d frames, got %d" % (name, MAX_FRAMES, m.shape[0]))
    res_table = _checked_table(name, "res_tracks", res_tracks)
    gt_table = _checked_table(name, "gt_tracks", gt_tracks)
    res, gt = _id_maps(name, "unet_aogm_counts", res_maps, gt_maps)
    import _hip
    ng_max, nr_max = _id_range(name, gt, res)
    T, dev = gt.shape[0], gt.device

    def words(*shape, dtype=torch.int32):
        return torch.empty(*shape, dtype=dtype, device=dev)

    area_gt, area_res, match, inter = words(T, ng_max + 1), words(T, nr_max + 1), words(T, ng_max + 1), words(T, ng_max + 1)
    _overlap_call("unet_instance_overlap", gt.int(), res.int(), ng_max, nr_max, _table_slots, lambda slots: (T, ng_max, nr_max, slots),
                  lambda slots: (area_gt, area_res, match, inter), name + ": %d pixels hold ids outside [0, %d] / [0, %d]")
    rows_gt, rows_res = _device_rows(gt_table, ng_max, dev), _device_rows(res_table, nr_max, dev)
    claims, claimant = words(T, nr_max + 1), words(T, nr_max + 1)
    inedge_gt, inedge_res = words(T, ng_max + 1, 2), words(T, nr_max + 1, 2)
    flags_gt, flags_res = words(T, ng_max + 1, dtype=torch.uint8), words(T, nr_max + 1, dtype=torch.uint8)
    counts = words(T, len(COUNT_NAMES), dtype=torch.int64)
    scratch = _hip.scratch("unet_aogm_counts", dev, T, ng_max, nr_max)
    _hip.run("unet_aogm_counts", dev, _hip.ptr(area_gt), _hip.ptr(area_res), _hip.ptr(match), _hip.ptr(rows_gt), _hip.ptr(rows_res),
             T, ng_max, nr_max, _hip.ptr(claims), _hip.ptr(claimant), _hip.ptr(inedge_gt), _hip.ptr(inedge_res), _hip.ptr(flags_gt),
             _hip.ptr(flags_res), _hip.ptr(counts), _hip.ptr(scratch))
    bad = _status_words(counts)[COUNT_NAMES.index("bad")]
    if bad:
        raise ValueError("%s: %d vertices are bad: a label without a row, a presence outside [B, E], or a parent that is never "
                         "present or not before its child" % (name, bad))
    out = AogmCounts(*np.ascontiguousarray(counts.cpu().numpy().T))
    if not return_vertices:
        return out
    return out, AogmVertices(*(a.cpu().numpy() for a in (claims, claimant, inedge_gt, inedge_res, flags_gt, flags_res)))


def aogm_from_counts(counts, weights=None):
    """AogmScores(tra, det, aogm, aogm0, aogm_d, aogm_d0, per_frame_det) from an AogmCounts (per frame or .total()), in float64
    on the host.  weights: a dict that overrides any of the challenge's w_NS = 5, w_FN = 10, w_FP = 1, w_ED = 1, w_EA = 1.5,
    w_EC = 1 (keys ns, fn, fp, ed, ea, ec).  AOGM = the weighted sum of the six counts, AOGM_0 = w_FN |V_ref| + w_EA |E_ref| (the
    cost of building the reference from nothing), TRA = 1 - min(AOGM, AOGM_0) / AOGM_0; AOGM-D and DET the same from NS, FN and FP
    alone with AOGM-D_0 = w_FN |V_ref|.  per_frame_det: DET of every frame alone, float64 [T].  Scores are nan where the
    reference has no vertex."""
    w = dict(WEIGHTS)
    for k, v in (weights or {}).items():
        if k not in WEIGHTS or isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v < np.inf:
            raise ValueError("aogm_from_counts: weights takes finite numbers >= 0 for %s, got %r: %r" % (", ".join(WEIGHTS), k, v))
        w[k] = float(v)
    c = AogmCounts(*(np.atleast_1d(np.asarray(a)).astype(np.int64) for a in counts))
    per = {k: getattr(c, k).astype(np.float64) for k in COUNT_NAMES}
    tot = {k: np.float64(int(getattr(c, k).sum())) for k in COUNT_NAMES}

    def costs(n):
        d = w["ns"] * n["ns"] + w["fn"] * n["fn"] + w["fp"] * n["fp"]
        return d + w["ed"] * n["ed"] + w["ea"] * n["ea"] + w["ec"] * n["ec"], w["fn"] * n["n_ref"] + w["ea"] * n["e_ref"], d, w["fn"] * n["n_ref"]

    def score(cost, cost0):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(cost0 > 0, 1.0 - np.minimum(cost, cost0) / cost0, np.nan)

    aogm, aogm0, aogm_d, aogm_d0 = costs(tot)
    empty = tot["n_ref"] == 0
    tra = np.float64(np.nan) if empty else np.float64(score(aogm, aogm0))
    det = np.float64(np.nan) if empty else np.float64(score(aogm_d, aogm_d0))
    _, _, frame_d, frame_d0 = costs(per)
    per_frame = np.where(per["n_ref"] > 0, score(frame_d, frame_d0), np.nan)
    return AogmScores(tra, det, float(aogm), float(aogm0), float(aogm_d), float(aogm_d0), per_frame)


def det_measure(res_maps, gt_maps):
    """The challenge's DET measure of a result against a reference, two stacks of id maps as aogm_counts takes them; no tables are
    needed: detection looks at vertices only.  Returns CtcMeasure(value, scores, counts): value = scores.det, scores the
    AogmScores and counts the AogmCounts of aogm_counts(res_maps, gt_maps) (its edge counts are those of the graphs without parent
    links)."""
    counts = aogm_counts(res_maps, gt_maps)
    scores = aogm_from_counts(counts)
    return CtcMeasure(scores.det, scores, counts)


def tra_measure(res_maps, res_tracks, gt_maps, gt_tracks):
    """The challenge's TRA measure of a result (its maps and table, e.g. the two values of functions.track_cells) against a
    reference (man_track stack and man_track.txt): CtcMeasure(value, scores, counts) with value = scores.tra."""
    counts = aogm_counts(res_maps, gt_maps, res_tracks, gt_tracks)
    scores = aogm_from_counts(counts)
    return CtcMeasure(scores.tra, scores, counts)


def ctc_scores(seg, det=None, tra=None):
    """The challenge's combined rankings from its three technical measures (numbers, or the results of functions.seg_measure,
    det_measure and tra_measure): CtcScores(op_csb, op_ctb) with OP_CSB = (SEG + DET) / 2 and OP_CTB = (SEG + TRA) / 2 in
    float64; None where the second measure is not given."""
    def number(v):
        return np.float64(v.seg if hasattr(v, "seg") else v.value if isinstance(v, CtcMeasure) else v)

    seg = number(seg)
    return CtcScores(None if det is None else (seg + number(det)) / 2, None if tra is None else (seg + number(tra)) / 2)
