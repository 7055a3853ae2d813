"""numpy restatement of the shape ops (functions.distance_map, functions.reconstruct, functions.shape_seeds; unet_distance_map,
unet_reconstruct_init / _sweeps / _finish, unet_shape_heights / _lower / _maxima), and the inputs of their tests.

distance2: brute force, first along every column (the row distance g to the nearest pixel outside the region), then along every
row (the minimum over all x' of g(x')^2 + (x - x')^2); distance2_brute is the minimum over every pixel outside the region, for
small images.  reconstruct: the synchronous iteration R <- min(under, max(R, 4-neighbours)) from R = min(marker, under) to a fixed
point.  seeds: the h-maxima of q = isqrt(256 d2) as DESIGN section 4o defines them, with q - hq not cut off at 0, labelled with
scipy.ndimage.label's default cross.  tests/test_shape_cpu.py pins all of it to scipy's distance transform, to an independent
count of the maxima by their dynamics, to a plateau search and to hand-worked answers."""
import collections
import math

import numpy as np
from scipy import ndimage

import instances_ref

TOP = 1 << 30                                                # marker and under are in [0, TOP]
LOW = -(np.int64(1) << 40)                                   # below every value: a pixel outside the region, or past the image
CROSS = ndimage.generate_binary_structure(2, 1)
EDGES = ("ignore", "background")
# either side of the 64-pixel tile and of its one-pixel halo
SIZES = [(1, 1), (1, 65), (63, 64), (64, 64), (65, 66), (129, 127), (257, 255)]
HS = (0, 0.5, 2, 5)
RADII = (0, 4)
SERPENTINE = (41, 400)
TILE = 64


# ---- the distance map -----------------------------------------------------------------------------------------------------

def distance2_brute(region, edge="ignore"):
    """int64 [H,W]: the minimum over every pixel outside the region (with edge='background' the ring around the image too)."""
    region = np.asarray(region) != 0
    H, W = region.shape
    if edge == "background":
        return distance2_brute(np.pad(region, 1), "ignore")[1:-1, 1:-1]
    oy, ox = np.nonzero(~region)
    if len(oy) == 0:
        return np.full((H, W), H * H + W * W, np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy[..., None] - oy) ** 2 + (xx[..., None] - ox) ** 2
    return d.min(axis=2).astype(np.int64) * region


def distance2(region, edge="ignore"):
    """int64 [H,W], in two brute-force passes."""
    region = np.asarray(region) != 0
    H, W = region.shape
    far = np.int64(1) << 20
    ys = np.arange(H)
    g = np.full((H, W), far, np.int64)
    for x in range(W):
        out = ys[~region[:, x]]
        if edge == "background":
            out = np.concatenate([out, [-1, H]])
        if len(out):
            g[:, x] = np.abs(ys[:, None] - out[None]).min(axis=1)
    xs = np.arange(W)
    dx2 = (xs[:, None] - xs[None]) ** 2                      # [x, x']
    d2 = np.stack([(row[None] ** 2 + dx2).min(axis=1) for row in g])
    if edge == "background":
        d2 = np.minimum(d2, np.minimum(xs + 1, W - xs)[None] ** 2)
    return np.where(d2 >= far * far, H * H + W * W, d2).astype(np.int64)


def isqrt256(d2):
    """floor(sqrt(256 d2)) in integers."""
    v = 256 * np.asarray(d2).astype(np.int64)
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r -= r * r > v
    r += (r + 1) * (r + 1) <= v
    assert (r * r <= v).all() and ((r + 1) * (r + 1) > v).all()
    return r


# ---- reconstruction ---------------------------------------------------------------------------------------------------------

def neighbour_max(a):
    p = np.pad(a, 1, constant_values=LOW)
    return np.maximum(np.maximum(p[:-2, 1:-1], p[2:, 1:-1]), np.maximum(p[1:-1, :-2], p[1:-1, 2:]))


def fixed_point(start, under, region):
    """The least R >= start with R(p) >= min(under(p), R(n)) on the region, int64, LOW outside it; and the synchronous steps."""
    R = np.where(region, np.minimum(start, under), LOW).astype(np.int64)
    U = np.where(region, under, LOW).astype(np.int64)
    steps = 0
    while True:
        N = np.minimum(U, np.maximum(R, neighbour_max(R)))
        if (N == R).all():
            return R, steps
        R, steps = N, steps + 1


def reconstruct(marker, under, mask=None):
    """One image -> dict(out int32 [H,W], raised, status): values outside [0, TOP] count as 0 and are counted in status."""
    marker, under = np.asarray(marker).astype(np.int64), np.asarray(under).astype(np.int64)
    region = np.ones(marker.shape, bool) if mask is None else np.asarray(mask) != 0
    bad_m, bad_u = (marker < 0) | (marker > TOP), (under < 0) | (under > TOP)
    marker, under = np.where(bad_m, 0, marker), np.where(bad_u, 0, under)
    R, _ = fixed_point(marker, under, region)
    return {"out": np.where(region, R, 0).astype(np.int32), "raised": int((region & (R > np.minimum(marker, under))).sum()),
            "status": int((bad_m | bad_u).sum())}


def reconstruct_batch(marker, under, mask=None):
    per = [reconstruct(m, u, None if mask is None else mask[b]) for b, (m, u) in enumerate(zip(marker, under))]
    return {"out": np.stack([r["out"] for r in per]), "raised": np.array([r["raised"] for r in per], np.int64),
            "status": np.array([r["status"] for r in per], np.int64)}


def tiled_launches(source, region, tile=TILE):
    """The launches unet_reconstruct_sweeps needs, the idle last one included, when one value spreads from `source` (y, x) over
    a connected region under a flat ceiling: a launch carries the value as far as it gets inside each 64 x 64 tile, and a step
    into another tile waits for the next launch.  So a pixel's launch is 1 + the fewest tile borders a path from the source to
    it crosses (a breadth-first search with steps of cost 0 and 1), and one more launch finds nothing to do."""
    region = np.asarray(region) != 0
    H, W = region.shape
    level = np.full((H, W), -1, np.int64)
    level[source] = 1
    todo = collections.deque([source])
    while todo:
        y, x = todo.popleft()
        for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if not (0 <= ny < H and 0 <= nx < W) or not region[ny, nx]:
                continue
            cost = int((ny // tile, nx // tile) != (y // tile, x // tile))
            if level[ny, nx] < 0 or level[y, x] + cost < level[ny, nx]:
                level[ny, nx] = level[y, x] + cost
                (todo.append if cost else todo.appendleft)((ny, nx))
    assert (level[region] > 0).all()
    return int(level.max()) + 1


# ---- seeds ------------------------------------------------------------------------------------------------------------------

def quanta(h, min_radius):
    return int(round(16 * h)), int(math.ceil(16 * min_radius))


def heights(mask, edge="ignore"):
    region = np.asarray(mask) != 0
    return isqrt256(distance2(region, edge)) * region


def h_maxima(q, region, hq):
    """(R1, R2) int64 with R1 = the reconstruction of q - hq under q (not cut off at 0) and R2 that of R1 - 1 under R1."""
    R1, _ = fixed_point(q - hq, q, region)
    R2, _ = fixed_point(R1 - 1, R1, region)
    return R1, R2


def seeds_at(mask, h, radii, edge="ignore"):
    """One image -> [(ids int32 [H,W], n) for each min_radius of radii]: the two reconstructions do not depend on it."""
    region = np.asarray(mask) != 0
    hq = quanta(h, 0)[0]
    R1, R2 = h_maxima(heights(region, edge), region, hq)
    out = []
    for r in radii:
        ids, n = ndimage.label(region & (R2 < R1) & (R1 + hq >= quanta(h, r)[1]), CROSS)
        out.append((ids.astype(np.int32), int(n)))
    return out


def seeds(mask, h=2.0, min_radius=0.0, edge="ignore"):
    """One image -> (ids int32 [H,W], n)."""
    return seeds_at(mask, h, (min_radius,), edge)[0]


def seeds_batch(mask, h=2.0, radii=(0.0,), edge="ignore"):
    """[B,H,W] -> [(ids int32 [B,H,W], n int32 [B]) for each min_radius of radii]"""
    per = [seeds_at(m, h, radii, edge) for m in mask]
    return [(np.stack([p[k][0] for p in per]), np.array([p[k][1] for p in per], np.int32)) for k in range(len(radii))]


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------

def disc(H, W, cy, cx, r):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def blobs(H, W, seed=0, sigma=4.0, level=0.02):
    return ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal((H, W)), sigma) > level


def busy(H, W, seed=0):
    """uint8 [H,W], H, W >= 63: Gaussian blobs, and built in by hand, each inside a cleared frame: top left two discs of r = 7
    on a diagonal (one component, two seeds at h = 2, more maxima than that at h = 0); bottom right a 3 x 3 square in the corner
    (under 'ignore' its peak is the corner pixel, 3 px: a seed that min_radius = 4 drops; under 'background' it is the centre)."""
    assert H >= 63 and W >= 63
    m = blobs(H, W, 7000 + 97 * H + W + seed, sigma=3.0)
    m[:28, :28] = False
    m[:27, :27] = disc(27, 27, 9, 9, 7) | disc(27, 27, 17, 17, 7)
    m[H - 5:, W - 5:] = False
    m[H - 3:, W - 3:] = True
    return m.astype(np.uint8) * 3


def size_cases(H, W, seed=0):
    """[(name, mask uint8 [B,H,W])], B 1-4.  From 63 x 63 on, the names that start with "busy" hold busy() images and the batch of
    four holds an empty and a full image next to two of them; below, random masks."""
    rs = np.random.RandomState(8000 + 97 * H + W + seed)
    if H < 63 or W < 63:
        return [("tiny B%d" % B, (rs.rand(B, H, W) < 0.8).astype(np.uint8)) for B in (1, 2, 3, 4)] + \
               [("tiny full", np.ones((1, H, W), np.uint8))]
    out = []
    for B in (1, 2, 3) if H * W <= 65 * 66 else (1,):          # above, the CPU pin's time decides
        out.append(("busy B%d" % B, np.stack([busy(H, W, seed + 10 * B + b) for b in range(B)])))
    m = busy(H, W, seed + 50)
    out.append(("busy B4", np.stack([np.zeros_like(m), m, np.ones_like(m), busy(H, W, seed + 51)])))
    return out


def recon_case(H, W, B, seed=0, with_mask=True):
    """(marker int64, under int64, mask uint8 or None) [B,H,W]: a rough under with plateaus, few high markers (so values travel
    far), both ends of the value range, and a mask with holes."""
    rs = np.random.RandomState(9000 + 97 * H + W + 7 * B + seed)
    under = (rs.randint(0, 6, (B, H, W)) * 50 + rs.randint(0, 3, (B, H, W))).astype(np.int64)
    marker = np.where(rs.rand(B, H, W) < 0.02, rs.randint(0, 400, (B, H, W)), 0).astype(np.int64)
    under[:, 0, 0], marker[:, 0, 0] = TOP, TOP
    under[:, H - 1, W - 1] = 0
    mask = (rs.rand(B, H, W) < 0.9).astype(np.uint8) * 2 if with_mask else None
    return marker, under, mask


def serpentine(H=SERPENTINE[0], W=SERPENTINE[1]):
    """(marker, under, mask) [1,H,W]: instances_ref.serpentine as the region under a flat ceiling of 500, one marker of 900 on
    the corridor's first pixel and 0 everywhere else: the whole corridor rises to 500, one tile per launch."""
    m = instances_ref.serpentine(H, W)
    marker = np.zeros((H, W), np.int64)
    marker[0, 0] = 900
    return marker[None], np.full((1, H, W), 500, np.int64), m[None].astype(np.uint8)
