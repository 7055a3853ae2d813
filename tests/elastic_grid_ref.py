"""fp64 numpy restatement of the paper's elastic deformation as DESIGN 4l defines it (imported like prepare_ref): the
displacement field of a coarse grid through per-axis weight matrices, the bilinear warp, and the fused training sample.
tests/test_elastic_grid_cpu.py pins it to torch's bicubic interpolate (a = -0.75) and to scipy's map_coordinates; the GPU tests
compare the library with it."""
import numpy as np


def keys_weight(d, a):
    """Keys' cubic convolution kernel of parameter a at distances d >= 0"""
    d = np.asarray(d, np.float64)
    near = ((a + 2.0) * d - (a + 3.0)) * d * d + 1.0
    far = ((a * d - 5.0 * a) * d + 8.0 * a) * d - 4.0 * a
    return np.where(d <= 1.0, near, np.where(d < 2.0, far, 0.0))


def axis_matrix(n, G, a):
    """[n, G]: row p holds the weights of the G nodes for pixel p of an axis of n pixels on a corner-aligned grid: position
    u = p (G-1)/(n-1), taps at the nodes floor(u)-1 .. floor(u)+2 (floor(u) held to G-1), indices clamped to [0, G-1]"""
    p = np.arange(n, dtype=np.float64)
    u = p * (G - 1) / (n - 1)
    i0 = np.minimum(np.floor(u).astype(np.int64), G - 1)
    M = np.zeros((n, G), np.float64)
    for k in range(4):
        node = i0 - 1 + k
        np.add.at(M, (np.arange(n), np.clip(node, 0, G - 1)), keys_weight(np.abs(u - node), a))
    return M


def field(g, H, W, a=-0.5):
    """g [2,G,G] -> [2,H,W]: plane 0 the row displacement of every pixel, plane 1 the column displacement"""
    g = np.asarray(g, np.float64)
    G = g.shape[-1]
    assert g.shape == (2, G, G) and G >= 2 and H >= 2 and W >= 2
    My, Mx = axis_matrix(H, G, a), axis_matrix(W, G, a)
    return np.stack([My @ g[0] @ Mx.T, My @ g[1] @ Mx.T])


def coordinates(g, H, W, a=-0.5):
    f = field(g, H, W, a)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return yy + f[0], xx + f[1]


def bilinear(img, cy, cx):
    """scipy.ndimage.map_coordinates(img, (cy, cx), order=1, mode='constant', cval=0) in fp64: bilinear inside
    [0,H-1] x [0,W-1], 0 for any coordinate outside it"""
    img = np.asarray(img, np.float64)
    H, W = img.shape
    inside = (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
    sy, sx = np.where(inside, cy, 0.0), np.where(inside, cx, 0.0)
    y0 = np.minimum(np.floor(sy).astype(np.int64), H - 2)
    x0 = np.minimum(np.floor(sx).astype(np.int64), W - 2)
    fy, fx = sy - y0, sx - x0
    v = (1 - fy) * ((1 - fx) * img[y0, x0] + fx * img[y0, x0 + 1]) + fy * ((1 - fx) * img[y0 + 1, x0] + fx * img[y0 + 1, x0 + 1])
    return np.where(inside, v, 0.0)


def warp(planes, grids, a=-0.5):
    """planes [P,B,H,W], grids [B,2,G,G] -> fp64 [P,B,H,W]"""
    planes = np.asarray(planes)
    P, B, H, W = planes.shape
    out = np.empty((P, B, H, W), np.float64)
    for b in range(B):
        cy, cx = coordinates(grids[b], H, W, a)
        for p in range(P):
            out[p, b] = bilinear(planes[p, b], cy, cx)
    return out


def round_levels(v, levels):
    return np.clip(np.floor(v + 0.5), 0, levels) if levels else v


def sample(img, mask, grids, a, levels, pad, crop):
    """The fused training sample.  img, mask [B,S,S], grids [B,2,G,G].  Returns a dict: raw_img [B,S,S] and raw_mask
    [B,crop,crop], the fp64 warped values before rounding (the mask's for the window [pad, pad+crop)^2); out_img = raw_img
    rounded to the levels (float32); out_gt = (raw_mask rounded > 127) int64; minmax [B,2] of out_img; reads [B,S,S] bool: the
    mask pixels the window's bilinear footprints touch."""
    B, S, _ = img.shape
    raw_img = np.empty((B, S, S), np.float64)
    raw_mask = np.empty((B, crop, crop), np.float64)
    reads = np.zeros((B, S, S), bool)
    win = slice(pad, pad + crop)
    for b in range(B):
        cy, cx = coordinates(grids[b], S, S, a)
        raw_img[b] = bilinear(img[b], cy, cx)
        raw_mask[b] = bilinear(mask[b], cy, cx)[win, win]
        wy, wx = cy[win, win], cx[win, win]
        inside = (wy >= 0) & (wy <= S - 1) & (wx >= 0) & (wx <= S - 1)
        y0 = np.minimum(np.floor(wy[inside]).astype(np.int64), S - 2)
        x0 = np.minimum(np.floor(wx[inside]).astype(np.int64), S - 2)
        for dy in (0, 1):
            for dx in (0, 1):
                reads[b, y0 + dy, x0 + dx] = True
    out_img = round_levels(raw_img, levels).astype(np.float32)
    out_gt = (round_levels(raw_mask, levels) > 127).astype(np.int64)
    minmax = np.stack([out_img.reshape(B, -1).min(1), out_img.reshape(B, -1).max(1)], 1)
    return dict(raw_img=raw_img, raw_mask=raw_mask, out_img=out_img, out_gt=out_gt, minmax=minmax, reads=reads)


def normalise01(x, minmax):
    """(x - lo) / (hi - lo) in fp32, x [B,...] float32, minmax [B,2] float32"""
    x = np.asarray(x, np.float32)
    shape = (x.shape[0],) + (1,) * (x.ndim - 1)
    lo, hi = minmax[:, 0].astype(np.float32).reshape(shape), minmax[:, 1].astype(np.float32).reshape(shape)
    return (x - lo) / (hi - lo)
