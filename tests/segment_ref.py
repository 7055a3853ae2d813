"""Plain numpy restatement of overlap-tile segmentation (tester.segment): the tile batch by numpy.pad(mode='reflect') and
slicing, and the stitch of the tiles' logits into an [B,H,W] mask (+ fp64 foreground probability).

tile_windows is an independent statement of tester.tile_grid's geometry (a brute-force search for the smallest grid, its
overhang split evenly with the odd pixel at the bottom / right); tests/test_segment_cpu.py pins the two together."""
import numpy as np

MARGIN = 92


def grid_1d(n, So):
    """(count, origin) along one axis: the fewest So-wide tiles that cover n pixels, the grid centred on the image."""
    k = 1
    while k * So < n:
        k += 1
    over = k * So - n
    return k, -(over // 2)


def tile_windows(H, W, S):
    """Per tile t = (i*nx + j) of one image: (input row0, input col0, output row0, output col0) in image coordinates, and
    (ny, nx).  Inputs are S wide, outputs So = S - 184 wide, each input centred on its output."""
    So = S - 2 * MARGIN
    ny, oy0 = grid_1d(H, So)
    nx, ox0 = grid_1d(W, So)
    wins = []
    for i in range(ny):
        for j in range(nx):
            oy, ox = oy0 + i * So, ox0 + j * So
            wins.append((oy - MARGIN, ox - MARGIN, oy, ox))
    return wins, ny, nx


def normalise(img):
    """(x - min) / (max - min) per image in float32, the reference's (inp - min) / ptp (data.py:188)."""
    img = np.asarray(img, np.float32)
    lo = img.min(axis=(-2, -1), keepdims=True)
    hi = img.max(axis=(-2, -1), keepdims=True)
    return (img - lo) / (hi - lo)


def tiles(img, S, norm=False):
    """img [B,H,W] float32 -> [B*ny*nx, 1, S, S]: np.pad(reflect) wide enough for every window, then slices."""
    img = np.asarray(img, np.float32)
    if norm:
        img = normalise(img)
    B, H, W = img.shape
    wins, ny, nx = tile_windows(H, W, S)
    P = S                                           # wider than any window reaches outside the image (< 92 + So)
    out = np.empty((B * len(wins), 1, S, S), np.float32)
    for b in range(B):
        pad = np.pad(img[b], P, mode="reflect")
        for t, (r0, c0, _, _) in enumerate(wins):
            out[b * len(wins) + t, 0] = pad[r0 + P:r0 + P + S, c0 + P:c0 + P + S]
    return out


def stitch_plane(values, B, H, W, S):
    """values [B*ny*nx, So, So] -> [B,H,W]: each tile's output window, clipped to the image."""
    values = np.asarray(values)
    So = S - 2 * MARGIN
    wins, _, _ = tile_windows(H, W, S)
    out = np.empty((B, H, W), values.dtype)
    for b in range(B):
        for t, (_, _, oy, ox) in enumerate(wins):
            y0, x0 = max(oy, 0), max(ox, 0)
            out[b, y0:min(oy + So, H), x0:min(ox + So, W)] = values[b * len(wins) + t, y0 - oy:min(So, H - oy), x0 - ox:min(So, W - ox)]
    return out


def stitch(logits, B, H, W, S):
    """logits [B*ny*nx, 2, So, So] -> (mask int64 [B,H,W], ties -> class 0; prob float64 [B,H,W] = softmax class 1)."""
    logits = np.asarray(logits)
    So = S - 2 * MARGIN
    wins, ny, nx = tile_windows(H, W, S)
    mask = np.full((B, H, W), -1, np.int64)
    prob = np.full((B, H, W), np.nan)
    for b in range(B):
        for t, (_, _, oy, ox) in enumerate(wins):
            lg = logits[b * len(wins) + t].astype(np.float64)
            y0, x0 = max(oy, 0), max(ox, 0)
            y1, x1 = min(oy + So, H), min(ox + So, W)
            l0 = lg[0, y0 - oy:y1 - oy, x0 - ox:x1 - ox]
            l1 = lg[1, y0 - oy:y1 - oy, x0 - ox:x1 - ox]
            mask[b, y0:y1, x0:x1] = (l1 > l0).astype(np.int64)
            prob[b, y0:y1, x0:x1] = 1.0 / (1.0 + np.exp(l0 - l1))
    return mask, prob
