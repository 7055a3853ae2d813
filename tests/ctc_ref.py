"""An independent restatement of the Cell Tracking Challenge's DET / TRA counting (imported like track_ref): what ctc.aogm_counts
and unet_aogm_counts are held to.  Written from the definitions, not from ctc.py: sets and dicts of
(t, L), np.unique on masked pixels per frame, one pass per operation.

  graph(maps, table)          the vertices, the in-edge of every vertex that has one, and the bad vertices of one side
  matches(gt, res)            reference vertex -> the result vertex that covers more than half of it
  compare(gt, res, gt_table, res_table)   everything above plus claims, TP, partners and the six operations as sets
  arrays(c, ng_max, nr_max)   the same in the layout of the library's outputs, with the inputs it takes (areas and match)
  scores(totals)              AOGM, AOGM_0, AOGM-D, AOGM-D_0, TRA, DET from a dict of the twelve totals, in plain Python floats
  hand_cases()                the six results of the mother-and-two-daughters example with their tables
"""
import collections

import numpy as np

NAMES = ("n_ref", "n_res", "e_ref", "e_res", "tp", "fn", "fp", "ns", "ea", "ed", "ec", "bad")
PRESENT, HAS_EDGE, PARENT_EDGE, BAD = 1, 2, 4, 8
MATCHED, EA, EC = 16, 32, 64
TP, FP, ED = 16, 32, 64


def graph(maps, table):
    """(vertices: set of (t, L); edge: dict (t, L) -> ((t', L'), kind) with kind 'track' or 'parent'; bad: set of (t, L); and
    pixels: dict (t, L) -> area).  table: rows L B E P or None."""
    frames_of, pixels = collections.defaultdict(list), {}
    for t, frame in enumerate(np.asarray(maps)):
        ids, n = np.unique(frame[frame != 0], return_counts=True)
        for L, k in zip(ids.tolist(), n.tolist()):
            frames_of[L].append(t)
            pixels[(t, L)] = k
    rows = None if table is None else {int(r[0]): tuple(int(v) for v in r[1:]) for r in np.asarray(table).reshape(-1, 4)}
    vertices = set(pixels)
    edge, bad = {}, set()
    for L, frames in frames_of.items():
        row = None if rows is None else rows.get(L)
        for k, t in enumerate(frames):
            if rows is not None and (row is None or not row[0] <= t <= row[1]):
                bad.add((t, L))
            if k > 0:
                edge[(t, L)] = ((frames[k - 1], L), "track")
            elif row is not None and row[2] > 0:
                parent = row[2]
                if parent in frames_of and frames_of[parent][-1] < t:
                    edge[(t, L)] = ((frames_of[parent][-1], parent), "parent")
                else:
                    bad.add((t, L))
    return vertices, edge, bad, pixels


def matches(gt, res):
    """dict (t, g) -> (t, s): per frame the result label s >= 1 with 2 |g n s| > |g|."""
    out = {}
    for t, (G, R) in enumerate(zip(np.asarray(gt), np.asarray(res))):
        for g in np.unique(G[G != 0]).tolist():
            inside = R[G == g]
            ids, n = np.unique(inside[inside != 0], return_counts=True)
            for s, k in zip(ids.tolist(), n.tolist()):
                if 2 * k > inside.size:
                    assert (t, g) not in out
                    out[(t, g)] = (t, s)
    return out


Compared = collections.namedtuple("Compared", "T gt_v gt_edge gt_bad gt_px res_v res_edge res_bad res_px match claims partner "
                                              "tp fn fp ns ea ec ed")


def compare(gt, res, gt_table=None, res_table=None):
    gt, res = np.asarray(gt), np.asarray(res)
    assert gt.shape == res.shape and gt.ndim == 3
    gt_v, gt_edge, gt_bad, gt_px = graph(gt, gt_table)
    res_v, res_edge, res_bad, res_px = graph(res, res_table)
    match = matches(gt, res)
    claims = collections.Counter(match.values())
    partner = {}
    for v in sorted(match):                                   # the largest reference label stays: defined for claims > 1 too
        partner[match[v]] = v
    tp = {s for s in res_v if claims[s] == 1}
    fn = {v for v in gt_v if v not in match}
    fp = {s for s in res_v if claims[s] == 0}
    ns = {s: claims[s] - 1 for s in res_v if claims[s] > 1}
    ea, ec = set(), set()
    for v, (u, kind) in gt_edge.items():
        s, r = match.get(v), match.get(u)
        reproduced = s in tp and r in tp and s in res_edge and res_edge[s][0] == r
        if not reproduced:
            ea.add(v)
        elif res_edge[s][1] != kind:
            ec.add(v)
    ed = set()
    for s, (r, _) in res_edge.items():
        if s in tp and r in tp:
            v, u = partner[s], partner[r]
            if not (v in gt_edge and gt_edge[v][0] == u):
                ed.add(s)
    return Compared(len(gt), gt_v, gt_edge, gt_bad, gt_px, res_v, res_edge, res_bad, res_px, match, claims, partner, tp, fn, fp, ns, ea, ec, ed)


def counts(c):
    """int64 [T][12] in the order of NAMES: every vertex and every edge operation is booked to its own (the head's) frame."""
    out = np.zeros((c.T, len(NAMES)), np.int64)
    for k, members in (("n_ref", c.gt_v), ("n_res", c.res_v), ("e_ref", c.gt_edge), ("e_res", c.res_edge), ("tp", c.tp), ("fn", c.fn),
                       ("fp", c.fp), ("ea", c.ea), ("ed", c.ed), ("ec", c.ec), ("bad", list(c.gt_bad) + list(c.res_bad))):
        for t, _ in members:
            out[t, NAMES.index(k)] += 1
    for (t, _), n in c.ns.items():
        out[t, NAMES.index("ns")] += n
    return out


def totals(c):
    return dict(zip(NAMES, counts(c).sum(axis=0).tolist()))


def arrays(c, ng_max, nr_max):
    """dict of the library's arrays: its inputs area_gt, area_res (int64; index 0 left 0: nothing reads it) and match, and its
    outputs claims, claimant, inedge_gt, inedge_res, flags_gt, flags_res, counts."""
    T = c.T
    a = {"area_gt": np.zeros((T, ng_max + 1), np.int64), "area_res": np.zeros((T, nr_max + 1), np.int64),
         "match": np.zeros((T, ng_max + 1), np.int64), "claims": np.zeros((T, nr_max + 1), np.int64),
         "claimant": np.zeros((T, nr_max + 1), np.int64), "inedge_gt": np.zeros((T, ng_max + 1, 2), np.int64),
         "inedge_res": np.zeros((T, nr_max + 1, 2), np.int64), "flags_gt": np.zeros((T, ng_max + 1), np.int64),
         "flags_res": np.zeros((T, nr_max + 1), np.int64), "counts": counts(c)}
    a["inedge_gt"][..., 0] = a["inedge_res"][..., 0] = -1
    for side, px, edge, bad in (("gt", c.gt_px, c.gt_edge, c.gt_bad), ("res", c.res_px, c.res_edge, c.res_bad)):
        for v, n in px.items():
            a["area_" + side][v] = n
            a["flags_" + side][v] |= PRESENT | (BAD if v in bad else 0)
        for v, (u, kind) in edge.items():
            a["inedge_" + side][v] = u
            a["flags_" + side][v] |= HAS_EDGE | (PARENT_EDGE if kind == "parent" else 0)
    for v, s in c.match.items():
        a["match"][v] = s[1]
        a["flags_gt"][v] |= MATCHED
    for s, n in c.claims.items():
        a["claims"][s] = n
        a["claimant"][s] = c.partner[s][1]
    for bit, side, members in ((EA, "gt", c.ea), (EC, "gt", c.ec), (TP, "res", c.tp), (FP, "res", c.fp), (ED, "res", c.ed)):
        for v in members:
            a["flags_" + side][v] |= bit
    return a


def scores(n):
    """dict of aogm, aogm0, aogm_d, aogm_d0, tra, det from the dict of totals."""
    aogm_d = 5 * n["ns"] + 10 * n["fn"] + 1 * n["fp"]
    aogm = aogm_d + 1 * n["ed"] + 1.5 * n["ea"] + 1 * n["ec"]
    aogm0, aogm_d0 = 10 * n["n_ref"] + 1.5 * n["e_ref"], 10 * n["n_ref"]
    nan = float("nan")
    return {"aogm": float(aogm), "aogm0": float(aogm0), "aogm_d": float(aogm_d), "aogm_d0": float(aogm_d0),
            "tra": 1 - min(aogm, aogm0) / aogm0 if n["n_ref"] else nan, "det": 1 - min(aogm_d, aogm_d0) / aogm_d0 if n["n_ref"] else nan}


def table_of(maps, parents=None):
    """The rows L B E P (int64 [n,4]) of the labels present in maps, B and E their first and last presence, P from the dict
    `parents` (0 where it names none)."""
    maps = np.asarray(maps)
    rows = []
    for L in np.unique(maps[maps != 0]).tolist():
        frames = np.nonzero((maps == L).any(axis=(1, 2)))[0]
        rows.append([L, int(frames[0]), int(frames[-1]), (parents or {}).get(L, 0)])
    return np.array(rows, np.int64).reshape(-1, 4)


def staggered(maps):
    """The maps with label L kept only in the frames L % 3 <= t < T - (L // 3) % 3: labels begin and end at different frames
    (some are gone altogether), so that a parent can end before its child begins."""
    maps = np.array(maps)
    T = len(maps)
    for L in np.unique(maps[maps != 0]).tolist():
        for t in range(T):
            if not L % 3 <= t < T - (L // 3) % 3:
                maps[t][maps[t] == L] = 0
    return maps


def faulty_table(maps, seed):
    """table_of(maps) with parents dealt at random among the labels (some end before their child begins, some do not, some are
    rows of labels that are in no frame), one row dropped and one row's E pulled in where there are rows enough: every kind of
    bad vertex, next to good ones."""
    rs = np.random.RandomState(900 + seed)
    t = table_of(maps)
    n = len(t)
    if n >= 2:
        t[:, 3] = np.where(rs.rand(n) < 0.5, t[rs.randint(0, n, n), 0], 0)
        t[t[:, 3] == t[:, 0], 3] = 0
    if n >= 3:
        longest, second, third = np.argsort(t[:, 1] - t[:, 2], kind="stable")[:3]
        t[longest, 2] = t[longest, 1]                          # E = B: any later presence is outside [B, E]
        ghost = int(t[:, 0].max()) + 3
        t[second, 3] = ghost                                   # a parent that is listed and never present
        t = np.concatenate([np.delete(t, third, axis=0), [[ghost, 0, 0, 0]]])
    return t


def rows_by_label(table, n_max):
    """The library's row array: int32 [n_max+1][3] of (B, E, P) by label, B = -1 where a label has no row."""
    rows = np.zeros((n_max + 1, 3), np.int32)
    rows[:, 0] = -1
    for L, B, E, P in np.asarray(table).reshape(-1, 4).tolist():
        if L <= n_max:
            rows[L] = (B, E, P)
    return rows


# ---- the hand-worked example: T = 4, 8 x 16 ----------------------------------------------------------------------------------
# Mother 1 is the 4 x 6 box rows 2-5, columns 1-6 in frames 0-1; daughters 2 and 3 are the 4 x 4 boxes rows 2-5, columns 1-4 and
# columns 9-12 in frames 2-3, both with parent 1.

def hand_reference():
    gt = np.zeros((4, 8, 16), np.int32)
    gt[:2, 2:6, 1:7] = 1
    gt[2:, 2:6, 1:5] = 2
    gt[2:, 2:6, 9:13] = 3
    return gt, np.array([[1, 0, 1, 0], [2, 2, 3, 1], [3, 2, 3, 1]], np.int64)


def hand_cases():
    """[(name, result maps, result table, the operation counts that are not 0)]"""
    gt, table = hand_reference()
    empty = np.zeros_like(gt)
    kept = gt.copy()
    kept[kept == 2] = 1                                        # daughter 2 keeps the mother's label; 3 is a track without parent
    merged = gt.copy()
    merged[2:] = 0
    merged[2:, 2:6, 1:13] = 2                                  # one detection over both daughters
    gap = gt.copy()
    gap[1] = 0
    extra = gt.copy()
    extra[0, 6:8, 13:15] = 4
    return [("itself", gt, table, {}),
            ("empty", empty, np.zeros((0, 4), np.int64), {"fn": 6, "ea": 5}),
            ("label kept", kept, np.array([[1, 0, 3, 0], [3, 2, 3, 0]]), {"ea": 1, "ec": 1}),
            ("merged", merged, np.array([[1, 0, 1, 0], [2, 2, 3, 1]]), {"ns": 2, "ea": 4}),
            ("gap", gap, table, {"fn": 1, "ea": 3, "ed": 2}),
            ("extra cell", extra, np.concatenate([table, [[4, 0, 0, 0]]]), {"fp": 1})]
