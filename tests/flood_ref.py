"""numpy restatements of the seeded watershed (functions.watershed, unet_flood_init / _sweeps / _assign / _finish) and the inputs
of its tests.  The region is mask != 0 (everything without a mask); every pixel has a level v in [0, 65536); a seed pixel in the
region is a source with key (L, d) = (0, 0); one 4-neighbour step onto a region pixel q turns (L, d) into (L, d + 1) if
v(q) <= L and into (v(q), 1) otherwise.  key(q) is the lexicographic minimum over all region paths from a source; a neighbour p is
a parent of q when its key extends to exactly key(q); a source keeps its id and every other reached pixel takes the least id among
its parents.  Two statements of it that share no code:
  (a) flood():      a heap Dijkstra over (L, d), then the ids in ascending key order (a parent's key is strictly smaller);
  (b) level_loop(): for h = 0 .. the top level, labels = split_ref.grow(labels, region & (v <= h | labels > 0)): the geodesic
                    growth of tests/split_ref.py, which knows nothing of levels, once per level.
naive() is the one-key shortcut (L, d, id) relaxed by min in raster order, which is WRONG (extension is not isotone in the id) and
is kept only so that tests/test_flood_cpu.py can show which inputs hold the trap."""
import heapq

import numpy as np

import instances_ref
import split_ref

ID_END = split_ref.ID_END
LEVELS = 1 << 16
SIZES = split_ref.SIZES
SERPENTINE = split_ref.SERPENTINE
KINDS = ("constant", "random2", "random6", "random65536", "ramp")
NBRS = ((-1, 0), (1, 0), (0, -1), (0, 1))


def quantise(image, levels=None):
    """(v int64, bad): the level of every pixel and the number of pixels that have none.  Integer images are read as they are
    (bad: outside [0, 65536)); float images need levels and give min(levels - 1, max(0, floor(x * levels))), the product in
    float32 (bad: not finite)."""
    image = np.asarray(image)
    if image.dtype.kind == "f":
        assert levels is not None and 1 <= levels <= LEVELS
        x = image.astype(np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            f = np.floor(x * np.float32(levels))
        v = np.clip(np.where(np.isnan(f), 0, f), 0, levels - 1).astype(np.int64)         # (a NaN reads as 0, and is counted)
        return v, int((~np.isfinite(x)).sum())
    x = image.astype(np.int64)
    ok = (x >= 0) & (x < LEVELS)
    return np.where(ok, x, 0), int((~ok).sum())


def ext(L, d, v):
    return (L, d + 1) if v <= L else (v, 1)


def flood(seeds, image, mask=None, levels=None, max_level=None):
    """Statement (a) on one image -> dict(out, pass_level, dist int32 [H,W]; unreached, seeds_outside, max_level, status,
    bad_values)."""
    seeds = np.asarray(seeds).astype(np.int64)
    H, W = seeds.shape
    region = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    v, bad_values = quantise(image, levels)
    valid = (seeds > 0) & (seeds < ID_END)
    source = valid & region
    key = {}                                                 # final keys
    best = {(y, x): (0, 0) for y, x in zip(*np.nonzero(source))}
    heap = [(0, 0, y, x) for (y, x) in best]
    heapq.heapify(heap)
    while heap:
        L, d, y, x = heapq.heappop(heap)
        if (y, x) in key:
            continue
        key[(y, x)] = (L, d)
        for dy, dx in NBRS:
            qy, qx = y + dy, x + dx
            if 0 <= qy < H and 0 <= qx < W and region[qy, qx] and (qy, qx) not in key:
                k = ext(L, d, v[qy, qx])
                if k < best.get((qy, qx), (LEVELS, 0)):
                    best[(qy, qx)] = k
                    heapq.heappush(heap, k + (qy, qx))
    out = np.zeros((H, W), np.int64)
    pass_level = np.full((H, W), -1, np.int64)
    dist = np.full((H, W), -1, np.int64)
    for (y, x), (L, d) in sorted(key.items(), key=lambda kv: kv[1]):
        if max_level is not None and L > max_level:
            break                                            # every later key is above it, too
        if source[y, x]:
            out[y, x] = seeds[y, x]
        else:
            ids = [out[y + dy, x + dx] for dy, dx in NBRS
                   if (y + dy, x + dx) in key and ext(*key[(y + dy, x + dx)], v[y, x]) == (L, d)]
            assert ids and min(ids) > 0                      # a reached pixel has a parent, and the parent came first
            out[y, x] = min(ids)
        pass_level[y, x], dist[y, x] = L, d
    return {"out": out.astype(np.int32), "pass_level": pass_level.astype(np.int32), "dist": dist.astype(np.int32),
            "unreached": int((region & (out == 0)).sum()), "seeds_outside": int((valid & ~region).sum()),
            "max_level": int(pass_level.max(initial=0)), "status": int(((seeds < 0) | (seeds >= ID_END)).sum()),
            "bad_values": bad_values}


MAPS = ("out", "pass_level", "dist")
INTS = ("unreached", "seeds_outside", "max_level", "status", "bad_values")


def flood_batch(seeds, image, mask=None, levels=None, max_level=None):
    """[B,H,W] -> dict: the maps int32 [B,H,W]; the counts int64 [B]."""
    per = [flood(s, im, None if mask is None else mask[b], levels, max_level) for b, (s, im) in enumerate(zip(seeds, image))]
    res = {k: np.stack([r[k] for r in per]) for k in MAPS}
    res.update({k: np.array([r[k] for r in per], np.int64) for k in INTS})
    return res


def level_loop(seeds, image, mask=None, levels=None, max_level=None):
    """Statement (b) on one image -> (out int32 [H,W], pass_level int32 [H,W])."""
    seeds = np.asarray(seeds).astype(np.int64)
    region = np.ones(seeds.shape, bool) if mask is None else np.asarray(mask) != 0
    v, _ = quantise(image, levels)
    labels = np.where((seeds > 0) & (seeds < ID_END) & region, seeds, 0)
    pass_level = np.where(labels > 0, 0, -1)
    top = int(v.max(initial=0)) if max_level is None else min(int(v.max(initial=0)), max_level)
    for h in range(top + 1):
        grown = split_ref.grow(labels, region & ((v <= h) | (labels > 0)))["out"].astype(np.int64)
        pass_level[(grown > 0) & (labels == 0)] = h
        labels = grown
    return labels.astype(np.int32), pass_level.astype(np.int32)


def naive(seeds, image, mask=None, levels=None):
    """The one-key shortcut on one image -> out int32 [H,W]: the triple (L, d, id) of every pixel relaxed by min, in raster order
    and in place, until a pass changes nothing."""
    seeds = np.asarray(seeds).astype(np.int64)
    H, W = seeds.shape
    region = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    v, _ = quantise(image, levels)
    source = (seeds > 0) & (seeds < ID_END) & region
    none = (LEVELS, 0, 0)
    key = [[(0, 0, int(seeds[y, x])) if source[y, x] else none for x in range(W)] for y in range(H)]
    changed = True
    while changed:
        changed = False
        for y in range(H):
            for x in range(W):
                if not region[y, x] or source[y, x]:
                    continue
                for dy, dx in NBRS:
                    py, px = y + dy, x + dx
                    if 0 <= py < H and 0 <= px < W and key[py][px] != none:
                        L, d, i = key[py][px]
                        k = ext(L, d, v[y, x]) + (i,)
                        if k < key[y][x]:
                            key[y][x], changed = k, True
    return np.array([[0 if k == none else k[2] for k in row] for row in key], np.int32)


def tile_borders_crossed(res, image, y, x, levels=None, tile=64):
    """The number of times a chain of parents from (y, x) back to a source changes its tile: at every pixel the first parent in
    the order up, down, left, right."""
    v, _ = quantise(image, levels)
    L, d = res["pass_level"], res["dist"]
    H, W = L.shape
    n = 0
    while (L[y, x], d[y, x]) != (0, 0):
        for dy, dx in NBRS:
            py, px = y + dy, x + dx
            if 0 <= py < H and 0 <= px < W and L[py, px] >= 0 and ext(int(L[py, px]), int(d[py, px]), v[y, x]) == (L[y, x], d[y, x]):
                n += (py // tile, px // tile) != (y // tile, x // tile)
                y, x = py, px
                break
        else:
            raise AssertionError("a reached pixel without a parent")
    return n


# ---- seeded inputs --------------------------------------------------------------------------------------------------------

def landscape(kind, H, W, seed=0):
    """One int32 [H,W] image of a kind in KINDS."""
    rs = np.random.RandomState(7000 + 97 * H + W + seed)
    if kind == "constant":
        return np.full((H, W), 3, np.int32)
    if kind.startswith("random"):
        return rs.randint(0, int(kind[6:]), (H, W)).astype(np.int32)
    assert kind == "ramp"
    yy, xx = np.mgrid[0:H, 0:W]
    return ((3 * xx + 2 * yy) // 5).astype(np.int32)


def size_cases(H, W, seed=0):
    """[(name, seeds int32 [B,H,W], image int32 [B,H,W], mask uint8 [B,H,W])]: split_ref.size_cases (B 1-4; with W >= 6 a busy
    image per batch, and in the batch of four an image without seeds, one with an empty mask and one with a full mask), image b
    of case k with the landscape KINDS[(k + b) % 5], so that every size sees every kind."""
    out = []
    for k, (name, s, m) in enumerate(split_ref.size_cases(H, W, seed)):
        kinds = [KINDS[(k + b) % len(KINDS)] for b in range(len(s))]
        out.append(("%s %s" % (name, "/".join(kinds)), s, np.stack([landscape(kd, H, W, seed + b) for b, kd in enumerate(kinds)]), m))
    return out


def small_cases(max_levels=8):
    """[(name, seeds [H,W], image [H,W], mask [H,W])]: every image of size_cases up to 65 x 63 with at most max_levels levels."""
    out = []
    for H, W in SIZES:
        if H * W > 65 * 63:
            continue
        for name, s, im, m in size_cases(H, W):
            out += [("%s %dx%d[%d]" % (name, H, W, b), s[b], im[b], m[b]) for b in range(len(s)) if im[b].max() < max_levels]
    return out


def random_small(n=40, seed=0):
    """n random images up to 13 x 13 with 1 to 40 levels, about 8 % seed pixels and 85 % region: (seeds, image, mask) each."""
    rs = np.random.RandomState(8000 + seed)
    out = []
    for _ in range(n):
        H, W = rs.randint(3, 14, 2)
        image = rs.randint(0, rs.randint(1, 41), (H, W)).astype(np.int32)
        seeds = (rs.randint(1, 9, (H, W)) * (rs.rand(H, W) < 0.08)).astype(np.int32)
        out.append((seeds, image, (rs.rand(H, W) < 0.85).astype(np.uint8)))
    return out


def plateau(gap):
    """(seeds, image) [1, gap + 2]: the seed 7 at the left end and the seed 4 at the right end of a row, `gap` pixels of a plateau
    of level 5 between them."""
    s = np.zeros((1, gap + 2), np.int32)
    s[0, 0], s[0, -1] = 7, 4
    im = np.full((1, gap + 2), 5, np.int32)
    im[0, 0] = im[0, -1] = 0
    return s, im


def ridge():
    """(seeds, image) [1,8]: the seeds 7 and 4 at the ends of a row of level 1 with a ridge of level 9 at x = 5: the cut is at the
    ridge, not at the middle."""
    s, im = plateau(6)
    im[0, 1:7] = (1, 1, 1, 1, 9, 1)
    return s, im


def pit():
    """(seeds, image) [1,5]: the seed 3, then a pass of level 6 with a pit of level 1 behind it that holds no seed."""
    return np.array([[3, 0, 0, 0, 0]], np.int32), np.array([[0, 2, 6, 1, 1]], np.int32)


def late_low_path():
    """(seeds, image, mask) [3,5].  q = (0, 2) is two steps from the seed 1 over a wall of level 3, and four steps from the seed 2
    along a valley of level 0 that comes up from below; r = (0, 3), of level 5, has q as its only neighbour.  The flood reaches
    q along the valley, (0, 4), so q and r belong to 2; a relaxation in raster order reaches q over the wall first and hands r
    the key (5, 1) with the id 1, which the later (5, 1) with the id 2 does not lower."""
    seeds = np.array([[1, 0, 0, 0, 0],
                      [0, 0, 0, 0, 0],
                      [2, 0, 0, 0, 0]], np.int32)
    image = np.array([[0, 3, 0, 5, 0],
                      [0, 0, 0, 0, 0],
                      [0, 0, 0, 0, 0]], np.int32)
    mask = np.array([[1, 1, 1, 1, 0],
                     [0, 0, 1, 0, 0],
                     [1, 1, 1, 0, 0]], np.uint8)
    return seeds, image, mask


def serpentine(H=SERPENTINE[0], W=SERPENTINE[1]):
    """(seeds, image, mask) [1,H,W]: split_ref.serpentine's corridor as a valley of level 0 between walls of level 5 that are
    region pixels too (the mask is full), with the seed 2 on the corridor's first pixel and the seed 1 on its last.  Within a tile
    the keys first spread across the walls, (5, d); they fall to (0, d) when the valley path arrives."""
    s, m = split_ref.serpentine(H, W)
    return s, np.where(m != 0, 0, 5).astype(np.int32), np.ones_like(m)


def two_cells(H=40, W=72):
    """(mask uint8, fg_prob float32, membrane x) [H,W]: a large and a small disc that overlap; the foreground probability is 0.95
    on a core in each, 0.8 on the rest of the mask and 0.55 on the column x = membrane, the true border: it crosses the small disc
    just right of the neck (the large disc ends at x = 40), cuts the mask in two, and is not halfway between the cores (about
    x = 35); 0.1 outside the mask."""
    yy, xx = np.mgrid[0:H, 0:W]
    big = (yy - 20) ** 2 + (xx - 22) ** 2 <= 18 ** 2
    small = (yy - 20) ** 2 + (xx - 52) ** 2 <= 14 ** 2
    membrane = 41
    mask = big | small
    p = np.where(mask, 0.8, 0.1).astype(np.float32)
    p[(yy - 20) ** 2 + (xx - 14) ** 2 <= 4 ** 2] = 0.95      # the large cell's core is off-centre, away from the border
    p[(yy - 20) ** 2 + (xx - 56) ** 2 <= 4 ** 2] = 0.95
    p[mask & (xx == membrane)] = 0.55
    return mask.astype(np.uint8), p, membrane
