"""numpy restatement, with a connectivity argument, of the four seeded sweeps (functions.split_cells, functions.watershed,
functions.reconstruct, functions.shape_seeds; unet_geodesic_sweeps_conn, unet_flood_sweeps_conn, unet_flood_assign_conn,
unet_reconstruct_sweeps_conn), and the inputs of its tests.  connectivity is 4 or 8; with 8 a step goes to any of the eight
neighbours that lies in the region, whatever the two pixels beside a diagonal step are.

  grow()         the growth: a breadth-first search by levels, each new pixel taking the least id among its neighbours of the
                 level before
  flood()        the watershed: a heap Dijkstra over (L, d), then the ids in ascending key order
  level_loop()   the watershed as one growth per level (flood_ref.level_loop's statement)
  fixed_point()  the reconstruction: the pixels settled from the highest value down, through a heap
  seeds()        the h-maxima of the distance map's heights, labelled with the connectivity's structure

At connectivity 4 tests/test_conn_cpu.py holds all of it equal to split_ref, flood_ref and shape_ref bit for bit; at 8 it pins the
growth to a per-seed dilation distance, the reconstruction to a synchronous grey dilation, the flood to the level loop, and all
of them to hand-worked answers."""
import heapq

import numpy as np
from scipy import ndimage

import flood_ref
import shape_ref
import split_ref

ID_END = split_ref.ID_END
BIG = split_ref.BIG
LOW = shape_ref.LOW
TILE = 64
STEPS4 = ((-1, 0), (1, 0), (0, -1), (0, 1))
STEPS8 = STEPS4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))
# the sizes of the device tests: either side of the 64-pixel tile and of its one-pixel halo
GROW_SIZES = [(1, 1), (1, 40), (2, 2), (5, 7), (33, 31), (64, 64), (63, 65), (65, 63), (129, 97)]
FLOOD_SIZES = GROW_SIZES[:-1]
RECON_SIZES = [(1, 65), (63, 64), (65, 66), (129, 127)]
SEED_SIZES = [(65, 66), (129, 127)]
SEED_HS = (0, 2)
DISC_HS = (0, 0.5, 1, 2)


def steps(connectivity):
    assert connectivity in (4, 8)
    return STEPS4 if connectivity == 4 else STEPS8


def structure(connectivity):
    return ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)


def shifted(a, fill, connectivity):
    """The planes a[y + dy, x + dx] for every step (dy, dx) of the connectivity, `fill` past the image."""
    p = np.pad(a, 1, constant_values=fill)
    H, W = a.shape
    return [p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in steps(connectivity)]


# ---- growth -----------------------------------------------------------------------------------------------------------------

def grow(seeds, mask, max_steps=None, connectivity=4):
    """One image -> dict(out int32 [H,W], dist int32 [H,W], unreached, seeds_outside, max_dist, status), as split_ref.grow."""
    seeds = np.asarray(seeds).astype(np.int64)
    region = np.asarray(mask) != 0
    valid = (seeds > 0) & (seeds < ID_END)
    out = np.where(valid & region, seeds, 0)
    dist = np.where(out > 0, 0, -1).astype(np.int64)
    front, d = out > 0, 0
    while front.any() and (max_steps is None or d < max_steps):
        d += 1
        offer = np.minimum.reduce(shifted(np.where(front, out, BIG), BIG, connectivity))
        front = region & (dist < 0) & (offer < BIG)
        out[front] = offer[front]
        dist[front] = d
    return {"out": out.astype(np.int32), "dist": dist.astype(np.int32), "unreached": int((region & (out == 0)).sum()),
            "seeds_outside": int((valid & ~region).sum()), "max_dist": int(dist.max(initial=0)) if (dist >= 0).any() else 0,
            "status": int(((seeds < 0) | (seeds >= ID_END)).sum())}


def grow_batch(seeds, mask, max_steps=None, connectivity=4):
    per = [grow(s, m, max_steps, connectivity) for s, m in zip(seeds, mask)]
    res = {k: np.stack([r[k] for r in per]) for k in ("out", "dist")}
    res.update({k: np.array([r[k] for r in per], np.int64) for k in split_ref.INTS})
    return res


def keep_orphans(out, seeds, mask, connectivity=4):
    """orphans='keep' on one image: the components of {mask != 0 and out == 0}, in raster order of their first pixel, get the ids
    n0 + 1, ... with n0 the largest seed id of the image."""
    rest, _ = ndimage.label((np.asarray(mask) != 0) & (out == 0), structure(connectivity))
    n0 = int(np.asarray(seeds).max(initial=0))
    return np.where(rest > 0, rest + n0, out).astype(np.int32)


def dilation_distance(seeds, mask, connectivity):
    """The pin of grow(): per seed id, the geodesic distance by masked binary dilation, one step at a time; then per pixel the
    least distance and, among the ids at that distance, the smallest -> (out, dist) int64, 0 / -1 where no seed reaches."""
    seeds = np.asarray(seeds).astype(np.int64)
    region = np.asarray(mask) != 0
    best_d = np.full(seeds.shape, BIG, np.int64)
    best_id = np.zeros(seeds.shape, np.int64)
    for i in np.unique(seeds[(seeds > 0) & (seeds < ID_END) & region]):
        reached = (seeds == i) & region
        d = np.where(reached, 0, BIG)
        n = 0
        while True:
            n += 1
            grown = ndimage.binary_dilation(reached, structure(connectivity), mask=region)
            new = grown & ~reached
            if not new.any():
                break
            d[new] = n
            reached = grown
        better = (d < best_d) | ((d == best_d) & (d < BIG) & (i < best_id))
        best_d[better], best_id[better] = d[better], i
    return best_id, np.where(best_d < BIG, best_d, -1)


# ---- flood ------------------------------------------------------------------------------------------------------------------

def flood(seeds, image, mask=None, levels=None, max_level=None, connectivity=4):
    """One image -> dict(out, pass_level, dist int32 [H,W]; unreached, seeds_outside, max_level, status, bad_values), as
    flood_ref.flood."""
    seeds = np.asarray(seeds).astype(np.int64)
    H, W = seeds.shape
    region = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    v, bad_values = flood_ref.quantise(image, levels)
    valid = (seeds > 0) & (seeds < ID_END)
    source = valid & region
    nbrs = steps(connectivity)
    far = (flood_ref.LEVELS, 0)
    key = {}
    best = {(int(y), int(x)): (0, 0) for y, x in zip(*np.nonzero(source))}
    heap = [(0, 0, y, x) for (y, x) in best]
    heapq.heapify(heap)
    while heap:
        L, d, y, x = heapq.heappop(heap)
        if (y, x) in key:
            continue
        key[(y, x)] = (L, d)
        for dy, dx in nbrs:
            q = (y + dy, x + dx)
            if 0 <= q[0] < H and 0 <= q[1] < W and region[q] and q not in key:
                k = flood_ref.ext(L, d, int(v[q]))
                if k < best.get(q, far):
                    best[q] = k
                    heapq.heappush(heap, k + q)
    out = np.zeros((H, W), np.int64)
    pass_level = np.full((H, W), -1, np.int64)
    dist = np.full((H, W), -1, np.int64)
    for (y, x), (L, d) in sorted(key.items(), key=lambda kv: kv[1]):
        if max_level is not None and L > max_level:
            break
        if source[y, x]:
            out[y, x] = seeds[y, x]
        else:
            ids = [out[y + dy, x + dx] for dy, dx in nbrs
                   if (y + dy, x + dx) in key and flood_ref.ext(*key[(y + dy, x + dx)], int(v[y, x])) == (L, d)]
            assert ids and min(ids) > 0
            out[y, x] = min(ids)
        pass_level[y, x], dist[y, x] = L, d
    return {"out": out.astype(np.int32), "pass_level": pass_level.astype(np.int32), "dist": dist.astype(np.int32),
            "unreached": int((region & (out == 0)).sum()), "seeds_outside": int((valid & ~region).sum()),
            "max_level": int(pass_level.max(initial=0)), "status": int(((seeds < 0) | (seeds >= ID_END)).sum()),
            "bad_values": bad_values}


def flood_batch(seeds, image, mask=None, levels=None, max_level=None, connectivity=4):
    per = [flood(s, im, None if mask is None else mask[b], levels, max_level, connectivity) for b, (s, im) in enumerate(zip(seeds, image))]
    res = {k: np.stack([r[k] for r in per]) for k in flood_ref.MAPS}
    res.update({k: np.array([r[k] for r in per], np.int64) for k in flood_ref.INTS})
    return res


def level_loop(seeds, image, mask=None, levels=None, max_level=None, connectivity=4):
    """flood_ref.level_loop with grow() above: (out int32 [H,W], pass_level int32 [H,W])."""
    seeds = np.asarray(seeds).astype(np.int64)
    region = np.ones(seeds.shape, bool) if mask is None else np.asarray(mask) != 0
    v, _ = flood_ref.quantise(image, levels)
    labels = np.where((seeds > 0) & (seeds < ID_END) & region, seeds, 0)
    pass_level = np.where(labels > 0, 0, -1)
    top = int(v.max(initial=0)) if max_level is None else min(int(v.max(initial=0)), max_level)
    for h in range(top + 1):
        grown = grow(labels, region & ((v <= h) | (labels > 0)), None, connectivity)["out"].astype(np.int64)
        pass_level[(grown > 0) & (labels == 0)] = h
        labels = grown
    return labels.astype(np.int32), pass_level.astype(np.int32)


def parents_across_a_tile_corner(res, image, connectivity=8, levels=None, tile=TILE):
    """The pixels of one flood() result whose only parents lie diagonally in another tile row and another tile column."""
    v, _ = flood_ref.quantise(image, levels)
    L, d = res["pass_level"], res["dist"]
    H, W = L.shape
    n = 0
    for y, x in zip(*np.nonzero((L >= 0) & ((L > 0) | (d > 0)))):
        where = set()
        for dy, dx in steps(connectivity):
            py, px = y + dy, x + dx
            if 0 <= py < H and 0 <= px < W and L[py, px] >= 0 and \
                    flood_ref.ext(int(L[py, px]), int(d[py, px]), int(v[y, x])) == (L[y, x], d[y, x]):
                where.add((py // tile != y // tile) and (px // tile != x // tile))
        n += where == {True}
    return n


# ---- reconstruction and seeds -----------------------------------------------------------------------------------------------

def fixed_point(start, under, region, connectivity=4):
    """The least R >= min(start, under) with R(p) >= min(under(p), R(n)) for every region neighbour n, int64, LOW outside the
    region: the pixels are settled from the highest value down (a heap; a settled pixel offers min(under(n), its value) to its
    neighbours, which is at most its own value, so nothing settled rises again)."""
    H, W = region.shape
    R = np.pad(np.where(region, np.minimum(start, under), LOW).astype(np.int64), 1, constant_values=LOW).tolist()
    U = np.pad(np.where(region, under, LOW).astype(np.int64), 1, constant_values=LOW).tolist()
    low = int(LOW)
    nbrs = steps(connectivity)
    heap = [(-R[y][x], y, x) for y in range(1, H + 1) for x in range(1, W + 1) if U[y][x] != low]
    heapq.heapify(heap)
    while heap:
        neg, y, x = heapq.heappop(heap)
        if -neg != R[y][x]:
            continue                                         # raised since it was pushed
        for dy, dx in nbrs:
            qy, qx = y + dy, x + dx
            offer = min(U[qy][qx], -neg)
            if offer > R[qy][qx]:                            # (never outside the region: there U is LOW)
                R[qy][qx] = offer
                heapq.heappush(heap, (-offer, qy, qx))
    return np.array(R, np.int64)[1:-1, 1:-1]


def dilation_fixed_point(start, under, region, connectivity):
    """The pin of fixed_point(): the synchronous R <- min(under, grey_dilation(R)) over the connectivity's footprint (which holds
    the centre), from R = min(start, under), to a fixed point."""
    R = np.where(region, np.minimum(start, under), LOW).astype(np.int64)
    U = np.where(region, under, LOW).astype(np.int64)
    while True:
        N = np.minimum(U, ndimage.grey_dilation(R, footprint=structure(connectivity), mode="constant", cval=float(LOW)))
        if (N == R).all():
            return R
        R = N


def reconstruct(marker, under, mask=None, connectivity=4):
    """One image -> dict(out int32 [H,W], raised, status), as shape_ref.reconstruct."""
    marker, under = np.asarray(marker).astype(np.int64), np.asarray(under).astype(np.int64)
    region = np.ones(marker.shape, bool) if mask is None else np.asarray(mask) != 0
    bad_m, bad_u = (marker < 0) | (marker > shape_ref.TOP), (under < 0) | (under > shape_ref.TOP)
    marker, under = np.where(bad_m, 0, marker), np.where(bad_u, 0, under)
    R = fixed_point(marker, under, region, connectivity)
    return {"out": np.where(region, R, 0).astype(np.int32), "raised": int((region & (R > np.minimum(marker, under))).sum()),
            "status": int((bad_m | bad_u).sum())}


def reconstruct_batch(marker, under, mask=None, connectivity=4):
    per = [reconstruct(m, u, None if mask is None else mask[b], connectivity) for b, (m, u) in enumerate(zip(marker, under))]
    return {"out": np.stack([r["out"] for r in per]), "raised": np.array([r["raised"] for r in per], np.int64),
            "status": np.array([r["status"] for r in per], np.int64)}


def seeds(mask, h=2.0, min_radius=0.0, edge="ignore", connectivity=4):
    """One image -> (ids int32 [H,W], n): DESIGN section 4o's seeds with both reconstructions and the labelling of the given
    connectivity; the heights are shape_ref's (the distance map is Euclidean)."""
    region = np.asarray(mask) != 0
    hq, rq = shape_ref.quanta(h, min_radius)
    q = shape_ref.heights(region, edge)
    R1 = fixed_point(q - hq, q, region, connectivity)
    R2 = fixed_point(R1 - 1, R1, region, connectivity)
    ids, n = ndimage.label(region & (R2 < R1) & (R1 + hq >= rq), structure(connectivity))
    return ids.astype(np.int32), int(n)


def seeds_batch(mask, h=2.0, min_radius=0.0, edge="ignore", connectivity=4):
    per = [seeds(m, h, min_radius, edge, connectivity) for m in mask]
    return np.stack([p[0] for p in per]), np.array([p[1] for p in per], np.int32)


# ---- hand-worked inputs -----------------------------------------------------------------------------------------------------

def diagonal_discs():
    """uint8 [64,64]: two discs of r = 12 on a diagonal.  Seeds at h = (0, 0.5, 1, 2): [9, 3, 2, 2] 4-connected (the staircase
    along the diagonal ridge makes maxima), [2, 2, 2, 2] 8-connected."""
    return (shape_ref.disc(64, 64, 25, 25, 12) | shape_ref.disc(64, 64, 39, 39, 12)).astype(np.uint8)


def eye_corridor(n=130, mirror=False):
    """(seeds, mask) [1,n,n]: the diagonal as a corridor one pixel thick, every step of it diagonal and two of them across a tile
    corner; the seed 2 on its first pixel and the seed 1 on its last.  mirror: the anti-diagonal, left and right swapped."""
    m = np.eye(n, dtype=np.uint8)
    s = np.zeros((n, n), np.int32)
    s[0, 0], s[n - 1, n - 1] = 2, 1
    if mirror:
        m, s = m[:, ::-1].copy(), s[:, ::-1].copy()
    return s[None], m[None]


def checkerboard(H=65, W=67):
    """(seeds, mask) [1,H,W]: the pixels with (y + x) even, which touch only at corners, and one seed at (0, 0)."""
    yy, xx = np.mgrid[0:H, 0:W]
    s = np.zeros((H, W), np.int32)
    s[0, 0] = 1
    return s[None], ((yy + xx) % 2 == 0).astype(np.uint8)[None]


def membrane():
    """(seeds, image) [8,8]: an anti-diagonal membrane of level 9, one pixel thick, on a zero image, and the seed 4 at (0, 0).
    Four-connected, the far side is reached only over the membrane (pass level 9); eight-connected, between two of its pixels
    (pass level 0)."""
    im = np.zeros((8, 8), np.int32)
    im[np.arange(8), 7 - np.arange(8)] = 9
    s = np.zeros((8, 8), np.int32)
    s[0, 0] = 4
    return s, im


def diagonal_tie():
    """(seeds, mask) [3,3], full mask: the seeds 7 at (0, 0) and 3 at (2, 2).  Eight-connected, the centre and the two other
    corners are one diagonal or two steps from both: they go to 3."""
    s = np.zeros((3, 3), np.int32)
    s[0, 0], s[2, 2] = 7, 3
    return s, np.ones((3, 3), np.uint8)


def corner_pairs(n=129, tile=TILE):
    """(seeds, mask) [8,n,n]: per image a region of two pixels that touch at one corner of the tile at (tile, tile) only, one of
    them the seed: at each of the tile's four corners, along both diagonals (the seed inside the tile, then outside it)."""
    out_s, out_m = [], []
    for cy, cx, oy, ox in ((tile, tile, -1, -1), (tile, 2 * tile - 1, -1, 1), (2 * tile - 1, tile, 1, -1), (2 * tile - 1, 2 * tile - 1, 1, 1)):
        for inside_seeds in (True, False):
            s, m = np.zeros((n, n), np.int32), np.zeros((n, n), np.uint8)
            m[cy, cx] = m[cy + oy, cx + ox] = 1
            s[(cy, cx) if inside_seeds else (cy + oy, cx + ox)] = 9
            out_s.append(s)
            out_m.append(m)
    return np.stack(out_s), np.stack(out_m)


def corner_flood(n=130):
    """(seeds, image, mask) [1,n,n]: eye_corridor as the region, under a ramp of levels along it: every parent link is diagonal
    and two of them cross a tile corner."""
    s, m = eye_corridor(n)
    yy, _ = np.mgrid[0:n, 0:n]
    return s, (np.minimum(yy, n - 1 - yy) // 9).astype(np.int32)[None], m
