"""numpy restatement of the frame linking and of the tracks made from it (imported like rand_ref): what functions.link_frames /
unet_link_frames, functions.tracks_from_links and functions.track_cells are held to, and the small seeded time-lapses the tests
feed them.

  links(from_maps, to_maps, n_max)   per pair of frames: np.bincount areas, np.unique on c * (n_max + 1) + p for the pair counts,
                                     then for every c the largest count, the first (smallest) p among equal ones; pixels with an id
                                     out of range are counted apart and nowhere else
  tracks(area, pred, over, ...)      not frame by frame as functions.tracks_from_links does it: first who continues whom and who
                                     is whose daughter, over the whole sequence; then the cells nobody continues into are the track
                                     starts, numbered in (frame, id) order, and each track is followed recursively to its end
"""
import numpy as np

import instances_ref


def links(from_maps, to_maps, n_max=None):
    """[T,H,W] id maps -> int64 area, pred, pred_overlap [T][n_max+1], status [T][2] (second column 0: no table here), and the
    number of distinct (t, p, c) with p, c >= 1: the slots a pair table needs."""
    f, g = np.asarray(from_maps).astype(np.int64), np.asarray(to_maps).astype(np.int64)
    assert f.shape == g.shape and g.ndim == 3
    T = len(g)
    n_max = max(int(f.max()), int(g.max()), 0) if n_max is None else n_max
    area, pred, over = (np.zeros((T, n_max + 1), np.int64) for _ in range(3))
    status = np.zeros((T, 2), np.int64)
    n_pairs = 0
    for t in range(T):
        c = g[t].ravel()
        p = f[t - 1].ravel() if t else np.zeros_like(c)
        ok = (c >= 0) & (c <= n_max) & (p >= 0) & (p <= n_max)
        status[t, 0] = (~ok).sum()
        c, p = c[ok], p[ok]
        area[t] = np.bincount(c, minlength=n_max + 1)
        both = (c > 0) & (p > 0)
        keys, counts = np.unique(c[both] * (n_max + 1) + p[both], return_counts=True)      # sorted by (c, p)
        n_pairs += len(keys)
        for key, n in zip(keys.tolist(), counts.tolist()):
            ci, pi = divmod(key, n_max + 1)
            if n > over[t, ci]:                              # strict: among equal overlaps the first, i.e. the smallest p, stays
                pred[t, ci], over[t, ci] = pi, n
    return area, pred, over, status, n_pairs


def tracks(area, pred, over, min_overlap=0.0, divisions=True, max_children=2):
    """(table int64 [n,4] of L B E P, track_of int32 [T][n_max+1]) from the three link arrays."""
    area, pred, over = (np.asarray(a).astype(np.int64) for a in (area, pred, over))
    T, N = area.shape
    accepted = (pred > 0) & (area > 0) & (over.astype(np.float64) >= min_overlap * area.astype(np.float64))
    accepted[:, 0] = False
    continues, mother = {}, {}                               # (t-1, p) -> (t, c);  (t, c) -> (t-1, p)
    for t in range(1, T):
        for p in (np.nonzero(area[t - 1, 1:])[0] + 1).tolist():
            cl = np.nonzero(accepted[t] & (pred[t] == p))[0].tolist()
            cl.sort(key=lambda c: (-int(over[t, c]), c))
            if len(cl) == 1 or (cl and not divisions):
                continues[(t - 1, p)] = (t, cl[0])
            else:
                for c in cl[:max_children]:
                    mother[(t, c)] = (t - 1, p)
    continued = set(continues.values())
    starts = [(t, c) for t in range(T) for c in (np.nonzero(area[t, 1:])[0] + 1).tolist() if (t, c) not in continued]
    track_of = np.zeros((T, N), np.int32)

    def follow(t, c, label):
        track_of[t, c] = label
        return follow(*continues[(t, c)], label) if (t, c) in continues else t

    table = []
    for label, (t, c) in enumerate(starts, 1):               # a mother's track starts in an earlier frame: it is numbered already
        end = follow(t, c, label)
        table.append([label, t, end, int(track_of[mother[(t, c)]]) if (t, c) in mother else 0])
    return np.array(table, np.int64).reshape(-1, 4), track_of


def remap(labels, track_of):
    """The host relabelling: track_of[t][labels[t]]."""
    return np.stack([track_of[t][np.asarray(l)] for t, l in enumerate(labels)]).astype(np.int32)


def check_structure(table, track_of, area):
    """What every track table obeys: labels 1..n in (B, first id) order; each label's frames are exactly B..E; every present id
    has a label and no absent one; a parent ends in the frame before each child begins."""
    n = len(table)
    assert table[:, 0].tolist() == list(range(1, n + 1))
    assert np.array_equal((track_of > 0)[:, 1:], (np.asarray(area) > 0)[:, 1:]) and not track_of[:, 0].any()
    first = []
    for L, B, E, P in table.tolist():
        frames = np.nonzero((track_of == L).any(axis=1))[0].tolist()
        assert frames == list(range(B, E + 1)), (L, frames)
        assert all((track_of[t] == L).sum() == 1 for t in frames)
        first.append((B, int(np.nonzero(track_of[B] == L)[0][0])))
        assert 0 <= P < L
        if P:
            assert table[P - 1, 2] == B - 1, (L, P)
    assert first == sorted(first)


# ---- seeded time-lapses, all int32 [T,H,W] ------------------------------------------------------------------------------------

def disc(shape, cy, cx, r):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return (yy - cy) ** 2 + (xx - cx) ** 2 < r * r


def drifting_discs(seed=0, T=5, H=48, W=72, shuffle=True):
    """Six discs of radius 4-6 on a 24-px grid, each moving by a constant step of at most 1 px per frame and axis: neighbours
    stay apart, every disc overlaps its own past.  shuffle: the ids 1..6 are dealt anew in every frame."""
    rs = np.random.RandomState(100 + seed)
    cells = [(12 + 24 * i, 12 + 24 * j, rs.uniform(4, 6), rs.randint(-1, 2), rs.randint(-1, 2)) for i in range(H // 24) for j in range(W // 24)]
    out = np.zeros((T, H, W), np.int32)
    for t in range(T):
        ids = rs.permutation(len(cells)) + 1 if shuffle else np.arange(len(cells)) + 1
        for k, (cy, cx, r, vy, vx) in enumerate(cells):
            out[t][disc((H, W), cy + t * vy, cx + t * vx, r)] = ids[k]
    return out


def dividing_discs():
    """Frames 0-1: a mother of radius 8 (id 2) and a mother of radius 10 (id 1).  Frames 2-3: the first is two daughters of
    radius 3, the second three daughters of radius 3, 4 and 3.5, all inside their mother's outline and apart from one another."""
    out = np.zeros((4, 40, 72), np.int32)
    for t in (0, 1):
        out[t][disc((40, 72), 20, 16, 8)] = 2
        out[t][disc((40, 72), 20, 50, 10)] = 1
    for t in (2, 3):
        out[t][disc((40, 72), 20, 12, 3)] = 5
        out[t][disc((40, 72), 20, 20, 3)] = 1
        out[t][disc((40, 72), 14, 50, 3)] = 2
        out[t][disc((40, 72), 25, 45, 4)] = 3
        out[t][disc((40, 72), 25, 55, 3.5)] = 4
    return out


def merging_discs():
    """Frames 0-1: discs of radius 5 (id 1) and 4 (id 2); frames 2-3: one disc (id 1) over both."""
    out = np.zeros((4, 32, 48), np.int32)
    for t in (0, 1):
        out[t][disc((32, 48), 16, 14, 5)] = 1
        out[t][disc((32, 48), 16, 30, 4)] = 2
    for t in (2, 3):
        out[t][disc((32, 48), 16, 22, 14)] = 1
    return out


def vanish_and_appear():
    """A cell (id 3) in frames 0-1 only; another (id 3 again) from frame 2 on, elsewhere; a third (id 1) throughout."""
    out = np.zeros((4, 32, 48), np.int32)
    for t in range(4):
        out[t][disc((32, 48), 8, 40, 4)] = 1
        out[t][disc((32, 48), 24, 8 if t < 2 else 30, 5)] = 3
    return out


def empty_middle():
    out = drifting_discs(3, 5, 24, 48, shuffle=False)
    out[2] = 0
    return out


def tie_frames(left, right):
    """Frame 0: two 4 x 3 cells side by side, ids (left, right); frame 1: one 2 x 4 cell (id 1) with 2 x 2 pixels on each."""
    out = np.zeros((2, 6, 8), np.int32)
    out[0, 1:5, 1:4] = left
    out[0, 1:5, 4:7] = right
    out[1, 2:4, 2:6] = 1
    return out


def sparse_ids(H=33, W=31):
    """Few cells, ids up to 70001: above 16 bits, far apart, not in raster order."""
    ids = (70001, 300, 65537, 7, 69999)
    out = np.zeros((2, H, W), np.int32)
    for t in range(2):
        for k, i in enumerate(ids):
            out[t][disc((H, W), 6 + 5 * k + t, 5 + 5 * k + 2 * t, 3.5)] = ids[(k + t) % len(ids)]
    return out


def random_frames(seed, T, H, W):
    """Any shape: blocks of 3 x 5 pixels with ids 0..11 that slide by a pixel per frame, rows that are one run from end to end
    (and go on in the next row), and a speckle of single pixels with ids up to 40."""
    rs = np.random.RandomState(500 + seed + 7 * T + 31 * H + W)
    coarse = rs.randint(0, 12, (-(-(H + T) // 3), -(-(W + T) // 5)))
    big = np.kron(coarse, np.ones((3, 5), np.int64))
    out = np.zeros((T, H, W), np.int32)
    for t in range(T):
        f = big[t:t + H, t:t + W].copy()
        for y in range(1, H, 7):
            f[y] = 1 + (y + t) % 3
            if y + 1 < H:
                f[y + 1, :W // 2] = f[y, 0]
        speck = rs.rand(H, W) < 0.03
        f[speck] = rs.randint(1, 41, int(speck.sum()))
        out[t] = f
    return out


def shifted_cells(seed, T, H, W, n, step=2):
    """A cells_case ground truth sliding by `step` pixels per frame along both axes, ids dealt anew per frame."""
    rs = np.random.RandomState(seed)
    gt = instances_ref.cells_case(seed, n, H + step * T, W + step * T)[0]
    out = np.zeros((T, H, W), np.int32)
    for t in range(T):
        perm = np.concatenate([[0], rs.permutation(int(gt.max())) + 1])
        out[t] = perm[gt[step * t:step * t + H, step * t:step * t + W]]
    return out


def sequences():
    """[(name, maps)]: every maker above."""
    return [("drift", drifting_discs()), ("drift, ids kept", drifting_discs(1, shuffle=False)), ("divide", dividing_discs()),
            ("merge", merging_discs()), ("vanish", vanish_and_appear()), ("empty middle", empty_middle()),
            ("tie 3 8", tie_frames(3, 8)), ("tie 8 3", tie_frames(8, 3)), ("sparse", sparse_ids()),
            ("random", random_frames(0, 4, 20, 33)), ("cells", shifted_cells(5, 6, 96, 120, 20))]
