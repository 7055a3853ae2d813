"""Python-integer restatement of the per-cell convex hulls of functions.cell_hulls (unet_cell_hulls) and of the contact list of
functions.cell_neighbours (unet_cell_contacts), imported like measure_ref.  Nothing here follows the device's method: the corner
points of a cell come from np.unique, the hull from Andrew's monotone chain over ALL of them (no level table), area, Feret
diameter and width from brute force in Python integers and fractions.Fraction, the contacts from shifted comparisons and
np.unique.  tests/test_hull_cpu.py pins it to hand-worked answers and to scipy.spatial.ConvexHull; tests/test_hull_gpu.py holds
the device to it.

  corners(mask)                     the distinct integer corner points (x, y) of the pixels of a bool mask, sorted
  hull(points)                      the hull's vertices in the device's order: down the left side from the top, up the right side
  measure(verts, lt=...)            (area2, feret_max2, (c, l2)) of a vertex list
  hulls(labels, n_max, bbox=None)   one image or a batch -> dict of arrays named like functions.CellHulls (width as [.., 2])
  contacts(labels)                  [B,H,W] -> (b, i, j, sides) int64, sorted by (b, i, j)
"""
import fractions

import numpy as np

SIZES = ((1, 1), (1, 2), (2, 1), (1, 65), (5, 17), (17, 5), (64, 64), (65, 63), (37, 300), (300, 37), (129, 97))


def corners(mask):
    ys, xs = np.nonzero(np.asarray(mask))
    pts = np.concatenate([np.stack([xs + dx, ys + dy], axis=1) for dy in (0, 1) for dx in (0, 1)]) if len(ys) else np.zeros((0, 2), np.int64)
    return [(int(x), int(y)) for x, y in np.unique(pts, axis=0)]


def cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull(points):
    """Andrew's monotone chain with strict turns (collinear points dropped) over distinct points, given in any order; then the
    order the device writes: from the top-left vertex (smallest y, then smallest x) down the left side to the bottom-left one,
    from the bottom-right one up the right side to the top-right one."""
    pts = sorted(set(points))
    if len(pts) < 3:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    ring = (lower[:-1] + upper[:-1])[::-1]                  # x to the right, y downwards: reversed, the ring goes down the left side
    start = min(range(len(ring)), key=lambda k: (ring[k][1], ring[k][0]))
    return ring[start:] + ring[:start]


def less_exact(c_a, l_a, c_b, l_b):
    """width a < width b: c_a^2 / l_a < c_b^2 / l_b, then the smaller l2"""
    ra, rb = fractions.Fraction(c_a * c_a, l_a), fractions.Fraction(c_b * c_b, l_b)
    return ra < rb or (ra == rb and l_a < l_b)


def less_wrapped64(c_a, l_a, c_b, l_b):
    """The same comparison with every product kept to its low 64 bits: what a kernel without 128-bit integers would compute."""
    m = (1 << 64) - 1
    lhs, rhs = (((c_a * c_a) & m) * l_b) & m, (((c_b * c_b) & m) * l_a) & m
    return lhs < rhs or (lhs == rhs and l_a < l_b)


def widths(verts):
    """(c, l2) of every edge (verts[e], verts[e + 1]), closing edge included"""
    out = []
    for e, p in enumerate(verts):
        q = verts[(e + 1) % len(verts)]
        out.append((max(abs(cross(p, q, v)) for v in verts), (q[0] - p[0]) ** 2 + (q[1] - p[1]) ** 2))
    return out


def measure(verts, less=less_exact):
    """area2 (shoelace), feret_max2 (all pairs), and the (c, l2) of the edge of smallest width under `less`, edges taken in order"""
    k = len(verts)
    if k == 0:
        return 0, 0, (0, 0)
    area2 = abs(sum(verts[e][0] * verts[(e + 1) % k][1] - verts[(e + 1) % k][0] * verts[e][1] for e in range(k)))
    feret = max((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 for p in verts for q in verts)
    best = None
    for c, l2 in widths(verts):
        if best is None or less(c, l2, best[0], best[1]):
            best = (c, l2)
    return area2, feret, best


def hulls(labels, n_max=None, bbox=None):
    """labels [H,W] or [B,H,W] -> dict: n_vertices int32, area2, feret_max2 int64, width int64 [.., 2] over [B, n_max+1] (the
    leading B dropped for one image), offset int64 [rows + 1], vertices int32 [2 L, 2].  bbox [.., n_max+1, 4]: only the pixels of
    an id inside its box count and the box sets the level count (None: the tight boxes)."""
    lab = np.asarray(labels).astype(np.int64)
    single = lab.ndim == 2
    lab = lab[None] if single else lab
    B, H, W = lab.shape
    n_max = int(lab.max()) if n_max is None else int(n_max)
    N = n_max + 1
    nv, a2, f2, wd = np.zeros((B, N), np.int32), np.zeros((B, N), np.int64), np.zeros((B, N), np.int64), np.zeros((B, N, 2), np.int64)
    levels, verts = np.zeros((B, N), np.int64), {}
    bbox = None if bbox is None else np.asarray(bbox).reshape(B, N, 4)
    for b in range(B):
        ids = np.unique(lab[b])
        flat_order = np.argsort(lab[b].ravel(), kind="stable")
        bounds = np.searchsorted(lab[b].ravel()[flat_order], ids, side="left").tolist() + [lab[b].size]
        for n, i in enumerate(ids.tolist()):
            if i < 1 or i > n_max:
                continue
            e = flat_order[bounds[n]:bounds[n + 1]]
            ys, xs = e // W, e % W
            if bbox is None:
                y0, y1 = int(ys.min()), int(ys.max()) + 1
            else:
                y0, x0, y1, x1 = (int(v) for v in bbox[b, i])
                keep = (ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)
                ys, xs = ys[keep], xs[keep]
            levels[b, i] = y1 - y0 + 1
            pts = np.unique(np.concatenate([np.stack([xs + dx, ys + dy], axis=1) for dy in (0, 1) for dx in (0, 1)]), axis=0)
            v = hull([(int(x), int(y)) for x, y in pts])
            verts[b, i] = v
            nv[b, i] = len(v)
            a2[b, i], f2[b, i], wd[b, i] = measure(v)
    offset = np.concatenate([[0], np.cumsum(levels.ravel())]).astype(np.int64)
    vertices = np.zeros((2 * int(offset[-1]), 2), np.int32)
    for (b, i), v in verts.items():
        if v:
            s = 2 * int(offset[b * N + i])
            vertices[s:s + len(v)] = v
    out = {"n_vertices": nv, "area2": a2, "feret_max2": f2, "width": wd}
    if single:
        out = {k: v[0] for k, v in out.items()}
    out.update(offset=offset, vertices=vertices)
    return out


def contacts(labels, n_max=None):
    """(b, i, j, sides): per image and unordered pair of ids 1 <= i < j (<= n_max), the unit sides between 4-adjacent pixels."""
    lab = np.asarray(labels).astype(np.int64)
    lab = lab[None] if lab.ndim == 2 else lab
    n_max = int(lab.max()) if n_max is None else int(n_max)
    keys = []
    for b in range(len(lab)):
        for p, q in ((lab[b][:, :-1], lab[b][:, 1:]), (lab[b][:-1, :], lab[b][1:, :])):
            on = (p != q) & (p >= 1) & (q >= 1) & (p <= n_max) & (q <= n_max)
            lo, hi = np.minimum(p, q)[on], np.maximum(p, q)[on]
            keys.append(np.stack([np.full(lo.shape, b, np.int64), lo, hi], axis=1))
    keys = np.concatenate(keys) if keys else np.zeros((0, 3), np.int64)
    u, n = np.unique(keys, axis=0, return_counts=True) if len(keys) else (keys, np.zeros(0, np.int64))
    return u[:, 0].astype(np.int64), u[:, 1].astype(np.int64), u[:, 2].astype(np.int64), n.astype(np.int64)


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def disc(r=12):
    """bool [2r+1, 2r+1]: the pixels whose centre is within r of the centre pixel (441 of them for r = 12)"""
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return yy * yy + xx * xx <= r * r


def disc_pair(r=12, gap=22, ident=1):
    """Two such discs, centres `gap` columns apart, under one id, with a one-pixel margin: int32 [2r+3, 2r+gap+3]"""
    m = np.zeros((2 * r + 3, 2 * r + gap + 3), np.int32)
    d = disc(r)
    m[1:2 * r + 2, 1:2 * r + 2][d] = ident
    m[1:2 * r + 2, 1 + gap:2 * r + 2 + gap][d] = ident
    return m


def block_map(seed, H, W, n_max=None):
    """Random blocks of random ids over background: runs of every length that cross the 64-lane boundary and the row ends, ids
    that touch, ids in several parts."""
    rs = np.random.RandomState(seed)
    top = max(2, min(40, H * W // 6 + 2)) if n_max is None else n_max
    m = np.zeros((H, W), np.int32)
    for _ in range(max(3, H * W // 40)):
        y, x = rs.randint(0, H), rs.randint(0, W)
        h, w = rs.randint(1, max(2, H // 3 + 1)), rs.randint(1, max(2, W // 2 + 1))
        m[y:y + h, x:x + w] = rs.randint(0, top + 1)
    return m


def sparse_ids(H, W, top=70001):
    """A few ids up to `top`, far apart in value, one of them in two parts"""
    m = np.zeros((H, W), np.int32)
    rs = np.random.RandomState(H * 31 + W)
    ids = [top, 1, 4097, 65536, top - 2]
    for i in ids:
        y, x = rs.randint(0, H), rs.randint(0, W)
        m[y:y + 1 + H // 5, x:x + 1 + W // 5] = i
    m[0, 0] = m[H - 1, W - 1] = 4097
    return m


def strip_case():
    """int32 [6, 30000]: id 1 is four scattered pixels in a strip of six rows, found by search (tests/test_hull_cpu.py asserts
    what it is for): the width comparison of its hull edges picks another edge when the products wrap at 64 bits (c^2 l2 is
    about 2^64.3 for its long edges)."""
    m = np.zeros((6, 30000), np.int32)
    for y, x in ((0, 0), (1, 29999), (5, 27789), (2, 19957)):
        m[y, x] = 1
    return m
