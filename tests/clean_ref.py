"""numpy/scipy restatement of the mask clean-up (imported like instances_ref): what functions.clean_mask,
functions.label_cells(connectivity=8) and the two entry points behind them (unet_clean_mask, unet_label_components_conn) are
held to, and the seeded and hand-made masks the tests feed them.  Integers only; everything is compared bit for bit.

  label(mask, connectivity, phase)   scipy.ndimage.label with the cross (4) or the full 3 x 3 structure (8) on mask != 0
                                     (phase 1) or mask == 0 (phase 0): raster numbering by first pixel
  clean(mask, ...)                   the background labelled with the dual structure, np.bincount areas, the ids seen in the
                                     first and last row and column; the holes that are filled; the filled mask labelled with
                                     the structure given, areas and frame ids again; the action plane, the output, the counts
"""
import numpy as np
from scipy import ndimage

import instances_ref

CROSS = ndimage.generate_binary_structure(2, 1)
FULL = ndimage.generate_binary_structure(2, 2)
SIZES = [(1, 1), (1, 65), (31, 33), (63, 64), (64, 64), (65, 66), (129, 127)]       # zero, one, partial, several tiles per axis
BIG = (257, 255)
INFO = ("holes_filled", "pixels_filled", "cells_small", "pixels_small", "cells_border", "pixels_border", "cells_kept")
HOLE_AREAS = (None, 0, 6)
MIN_AREAS = (0, 5)
POCKET = (16, 2)                                             # a background pixel of busy() inside the pocket open to the frame


def structure(connectivity):
    assert connectivity in (4, 8)
    return CROSS if connectivity == 4 else FULL


def dual(connectivity):
    return 12 - connectivity


def label(mask, connectivity=4, phase=1):
    """(labels int32 [H,W], n) of one mask: the components of mask != 0 (phase 1) or mask == 0 (phase 0)."""
    lab, n = ndimage.label((np.asarray(mask) != 0) == bool(phase), structure(connectivity))
    return lab.astype(np.int32), int(n)


def label_batch(masks, connectivity=4, phase=1):
    got = [label(m, connectivity, phase) for m in masks]
    return np.stack([g[0] for g in got]), np.array([g[1] for g in got], np.int32)


def attributes(lab, n):
    """(area int64 [n+1], on_frame bool [n+1]) of a label image."""
    area = np.bincount(lab.ravel(), minlength=n + 1)
    on_frame = np.zeros(n + 1, bool)
    for edge in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
        on_frame[edge] = True
    return area, on_frame


def holes(mask, connectivity=4):
    """(labels of the background with the dual connectivity, area, is_hole [n+1]) of one mask; is_hole[0] is False."""
    lab, n = label(mask, dual(connectivity), 0)
    area, on_frame = attributes(lab, n)
    is_hole = ~on_frame
    is_hole[0] = False
    return lab, area, is_hole


def clean(mask, *, fill_holes=True, max_hole_area=None, min_area=0, drop_border=False, connectivity=4):
    """One image.  dict: out (mask's dtype), action uint8, info int64 [7] in the order of INFO."""
    mask = np.asarray(mask)
    fg = mask != 0
    lab, area, is_hole = holes(mask, connectivity)
    fill = is_hole & bool(fill_holes)
    if max_hole_area is not None:
        fill &= area <= max_hole_area
    filled = fill[lab]
    cells, n = label(fg | filled, connectivity)
    area_c, on_frame = attributes(cells, n)
    small = area_c < min_area
    small[0] = False
    border = on_frame & ~small & bool(drop_border)
    border[0] = False
    action = np.where(fg, 1, 0).astype(np.uint8)
    action[filled] = 2
    action[small[cells]] = 3
    action[border[cells]] = 4
    out = np.where(action == 1, mask, (action == 2).astype(mask.dtype)).astype(mask.dtype)
    info = np.array([fill.sum(), filled.sum(), small.sum(), area_c[small].sum(), border.sum(), area_c[border].sum(),
                     n - small.sum() - border.sum()], np.int64)
    return {"out": out, "action": action, "info": info}


def clean_batch(masks, **kw):
    got = [clean(m, **kw) for m in masks]
    return {k: np.stack([g[k] for g in got]) for k in ("out", "action", "info")}


# ---- hand-made masks ----------------------------------------------------------------------------------------------------------

def checkerboard(n=64):
    yy, xx = np.mgrid[0:n, 0:n]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def diagonal(n=64, anti=False):
    m = np.eye(n, dtype=np.uint8)
    return m[:, ::-1].copy() if anti else m


def diamond(n=64, c=32, r=20):
    yy, xx = np.mgrid[0:n, 0:n]
    return (np.abs(yy - c) + np.abs(xx - c) == r).astype(np.uint8)


def nested():
    m = np.zeros((40, 40), np.uint8)
    for k, (a, b) in enumerate(((4, 36), (8, 32), (12, 28), (16, 24), (19, 21))):
        m[a:b, a:b] = 1 - k % 2
    return m


def diagonal_pocket():
    m = np.zeros((8, 8), np.uint8)
    m[0:5, 0:5] = 1
    m[1:4, 1:4] = 0
    m[0, 0] = 0
    return m


def two_squares():
    m = np.zeros((9, 9), np.uint8)
    m[0:3, 0:3] = 1
    m[3:6, 3:6] = 1
    return m


def ring_cell(n=64, c=32, a=28, b=14, r_in=6):
    """An elliptic cell with a dark nucleus: the distance map of the ring has a ring-shaped ridge, high at the two ends of the
    cell and low beside the nucleus."""
    yy, xx = np.mgrid[0:n, 0:n]
    inside = ((yy - c) / b) ** 2 + ((xx - c) / a) ** 2 <= 1
    return (inside & ((yy - c) ** 2 + (xx - c) ** 2 > r_in * r_in)).astype(np.uint8)


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------

def speckle(H, W, seed, p=0.5):
    return (np.random.RandomState(4100 + seed).rand(H, W) < p).astype(np.uint8)


def busy(H, W, seed=0):
    """Cells with flipped pixels and speckle between them, H >= 31 and W >= 33, and in the top left corner, hand-placed: a ring
    with a hole of 48 pixels and a one-pixel island in it; holes of 1 and of 6 pixels; a C open to the first column (a pocket of
    the background that is no hole, in a cell on the frame); cells of 1, 4 and 5 pixels; a diamond outline, which leaks through
    its diagonals when the foreground is 4-connected and holds a hole of 13 pixels when it is 8-connected."""
    assert H >= 31 and W >= 33
    rs = np.random.RandomState(4000 + 7 * seed + H * 1000 + W)
    m = instances_ref.discs(rs, H, W, 4 + H * W // 600)
    m &= rs.rand(H, W) >= 0.04                               # dark pixels inside the cells
    m |= rs.rand(H, W) < 0.05                                # speckle
    m = m.astype(np.uint8)
    m[0:28, 0:32] = 0
    m[2:11, 2:11] = 1; m[3:10, 3:10] = 0; m[6, 6] = 1        # ring, hole of 48, island
    m[2:5, 13:16] = 1; m[3, 14] = 0                          # hole of 1
    m[7:11, 13:18] = 1; m[8:10, 14:17] = 0                   # hole of 6
    m[14:19, 0:5] = 1; m[15:18, 0:4] = 0                     # C open to column 0
    m[14, 8] = 1; m[14:16, 10:12] = 1; m[17, 8:13] = 1       # cells of 1, 4 and 5 pixels
    yy, xx = np.mgrid[0:H, 0:W]
    m[np.abs(yy - 23) + np.abs(xx - 20) == 3] = 1            # diamond outline
    return m


def size_cases(H, W, seed=0):
    """[(name, masks uint8 [B,H,W])] at one size, B 1-4; the batch of four holds an empty and a full image."""
    one = busy if H >= 31 and W >= 33 else speckle
    name = "busy" if one is busy else "thin"
    imgs = [one(H, W, seed + k) for k in range(6)]
    zeros, ones = np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)
    return [(name + " B1", np.stack(imgs[:1])), (name + " B2", np.stack(imgs[1:3])), (name + " B3", np.stack(imgs[3:6])),
            (name + " B4", np.stack([zeros, imgs[0], ones, imgs[4]]))]
