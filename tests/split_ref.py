"""numpy restatement of the seeded geodesic growth inside a mask (functions.split_cells, unet_geodesic_init / _sweeps / _finish),
and the inputs of its tests.  The region is mask != 0; g(p) is the least number of 4-neighbour steps from a seed pixel to p along
region pixels; a region pixel with g(p) <= max_steps takes the id of the seed pixel at distance g(p), the smallest id among those
at that distance, and every other pixel gets 0.  grow() is a level-by-level breadth-first search: level d is the set of region
pixels without an id that touch level d - 1, and each takes the least id among its 4-neighbours of level d - 1.
tests/test_split_cpu.py pins it to a per-seed geodesic distance by masked binary dilation and to hand-worked answers."""
import numpy as np
from scipy import ndimage

import instances_ref

ID_END = 1 << 24                                             # ids are in [1, ID_END)
BIG = np.int64(1) << 40
CROSS = ndimage.generate_binary_structure(2, 1)
# either side of the 64-pixel tile and of its one-pixel halo
SIZES = [(1, 1), (1, 40), (2, 2), (5, 7), (33, 31), (64, 64), (63, 65), (65, 63), (129, 97), (257, 255)]
STEPS = (None, 0, 1, 5)
SERPENTINE = (41, 400)


def neighbour_min(a):
    """The minimum of a over the four neighbours of every pixel (BIG past the image)."""
    p = np.pad(a, 1, constant_values=BIG)
    return np.minimum(np.minimum(p[:-2, 1:-1], p[2:, 1:-1]), np.minimum(p[1:-1, :-2], p[1:-1, 2:]))


def grow(seeds, mask, max_steps=None):
    """One image -> dict(out int32 [H,W], dist int32 [H,W], unreached, seeds_outside, max_dist, status)."""
    seeds = np.asarray(seeds).astype(np.int64)
    region = np.asarray(mask) != 0
    valid = (seeds > 0) & (seeds < ID_END)
    out = np.where(valid & region, seeds, 0)
    dist = np.where(out > 0, 0, -1).astype(np.int64)
    level, d = out > 0, 0
    while level.any() and (max_steps is None or d < max_steps):
        d += 1
        offer = neighbour_min(np.where(level, out, BIG))     # the least id among the neighbours of level d - 1
        level = region & (dist < 0) & (offer < BIG)
        out[level] = offer[level]
        dist[level] = d
    return {"out": out.astype(np.int32), "dist": dist.astype(np.int32), "unreached": int((region & (out == 0)).sum()),
            "seeds_outside": int((valid & ~region).sum()), "max_dist": int(dist.max(initial=0)) if (dist >= 0).any() else 0,
            "status": int(((seeds < 0) | (seeds >= ID_END)).sum())}


INTS = ("unreached", "seeds_outside", "max_dist", "status")


def grow_batch(seeds, mask, max_steps=None):
    """[B,H,W] -> dict: out, dist int32 [B,H,W]; the counts int64 [B]."""
    per = [grow(s, m, max_steps) for s, m in zip(seeds, mask)]
    res = {k: np.stack([r[k] for r in per]) for k in ("out", "dist")}
    res.update({k: np.array([r[k] for r in per], np.int64) for k in INTS})
    return res


def keep_orphans(out, seeds, mask):
    """orphans='keep' on one image: the 4-connected components of {mask != 0 and out == 0}, in raster order of their first pixel,
    get the ids n0 + 1, ... with n0 the largest seed id of the image."""
    rest, n = ndimage.label((np.asarray(mask) != 0) & (out == 0), CROSS)
    n0 = int(np.asarray(seeds).max(initial=0))
    return np.where(rest > 0, rest + n0, out).astype(np.int32)


# ---- seeded inputs --------------------------------------------------------------------------------------------------------

def busy(H, W, seed=0):
    """(seeds int32 [H,W], mask uint8 [H,W]) of one image with everything the growth can meet, for W >= 6: a region with holes
    and walls with gaps (so geodesic and Euclidean neighbours differ), one- and many-pixel seeds with ids up to 2^24 - 1, seeds
    that fall outside the region, and built in by hand: in row 0 the ids 5 and 3 two pixels apart with one free region pixel
    between them (a tie, which goes to 3); in the last row a region pixel cut off from everything, without a seed (unreached),
    and next to it a seed on a pixel outside the region."""
    assert W >= 6
    rs = np.random.RandomState(5000 + 97 * H + W + seed)
    region = rs.rand(H, W) < 0.88
    for x in list(range(9, W - 1, 13))[:3]:                   # a few walls with two gaps each
        region[:, x] = False
        region[rs.randint(0, H, 2), x] = True
    for y in list(range(7, H - 1, 17))[:2]:
        region[y, :] = False
        region[y, rs.randint(0, W, 2)] = True
    seeds = np.zeros((H, W), np.int64)
    n = max(2, min(6, H * W // 160))
    ids = rs.choice(np.arange(6, 5000), n, replace=False)
    ids[-1] = ID_END - 1
    for i in ids:
        y, x = rs.randint(0, H), rs.randint(0, W)
        r = int(rs.randint(0, 3))
        seeds[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = i
    region[0, 0:3], seeds[0, 0:3] = True, (5, 0, 3)
    if H > 1:
        region[1, 0:3], seeds[1, 0:3] = False, 0
    region[max(0, H - 2):, W - 2:], seeds[max(0, H - 2):, W - 2:] = False, 0
    region[H - 1, W - 1] = True
    seeds[H - 1, W - 2] = 77
    return seeds.astype(np.int32), region.astype(np.uint8) * 3


def size_cases(H, W, seed=0):
    """[(name, seeds int32 [B,H,W], mask uint8 [B,H,W])], B 1-4 (1 and 4 at the largest size).  With W >= 6 the names that start
    with "busy" hold a busy() image; the batch of four holds, next to it, an image without seeds, one with an empty mask and one
    with a full mask."""
    rs = np.random.RandomState(6000 + 97 * H + W + seed)
    out = []
    if W < 6:
        for B in (1, 2, 3, 4):
            out.append(("tiny B%d" % B, rs.randint(0, 4, (B, H, W)).astype(np.int32) * (rs.rand(B, H, W) < 0.6),
                        (rs.rand(B, H, W) < 0.8).astype(np.uint8)))
        return out
    for B in (1, 2, 3) if H * W <= 129 * 97 else (1,):         # above, the CPU pin's time decides
        pairs = [busy(H, W, seed + 10 * B + b) for b in range(B)]
        out.append(("busy B%d" % B, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])))
    s, m = busy(H, W, seed + 50)
    s2, m2 = busy(H, W, seed + 51)
    out.append(("busy B4", np.stack([np.zeros_like(s), s, s2, s]), np.stack([m, np.zeros_like(m), m2, np.ones_like(m)])))
    return out


def serpentine(H=SERPENTINE[0], W=SERPENTINE[1]):
    """(seeds, mask) [1,H,W]: instances_ref.serpentine, every other row open and joined at alternating ends, with the seed 2 on
    the corridor's first pixel and the seed 1 on its last."""
    m = instances_ref.serpentine(H, W)
    s = np.zeros((H, W), np.int32)
    s[0, 0] = 2
    last = (H - 1) // 2 * 2                                   # the last open row; the corridor ends where it was not entered
    s[last, W - 1 if (last // 2) % 2 == 0 else 0] = 1
    return s[None], m[None].astype(np.uint8)
