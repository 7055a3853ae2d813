"""numpy restatement of the per-cell table of functions.cell_sums (unet_cell_sums) and of functions.select_cells, imported like
instances_ref: every integer field from per-pixel coordinates with np.bincount on int64 and shifted comparisons for the edges.
tests/test_measure_cpu.py pins it to hand-worked answers and to scipy.ndimage; tests/test_measure_gpu.py holds the device to it.

  sums(labels, image=None, n_max=None)   one image [H,W] -> dict of arrays [n_max+1, ...] named like functions.CellSums
  sums_batch(labels, images, n_max)      [B,H,W] -> the same with a leading B
  scipy_route(labels, image, n_max)      the host route a user takes today: the scipy.ndimage calls, one quantity at a time
  select(labels, keep, renumber)         np.where(keep[lab], lab, 0) and its renumbered form
"""
import numpy as np
from scipy import ndimage

FIELDS = ("area", "bbox", "moments", "frame", "open", "contact", "v_sum", "v_sum2", "v_min", "v_max", "present")
SIZES = ((1, 1), (1, 2), (2, 1), (1, 65), (5, 17), (17, 5), (64, 64), (65, 63), (37, 300), (300, 37), (129, 97))


def edge_counts(lab):
    """(frame, open, contact) int64 [H,W]: per pixel, how many of its four sides lie on the image frame, face id 0 from an id
    != 0, face another id (from id 0: any non-zero id)."""
    lab = np.asarray(lab).astype(np.int64)
    H, W = lab.shape
    pad = np.full((H + 2, W + 2), -1, np.int64)
    pad[1:-1, 1:-1] = lab
    frame, opened, contact = (np.zeros((H, W), np.int64) for _ in range(3))
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        nb = pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        frame += nb == -1
        opened += (nb == 0) & (lab != 0)
        contact += (nb > 0) & (nb != lab)
    return frame, opened, contact


def sums(labels, image=None, n_max=None):
    """The table of one image.  Integer images give int64 sums and int32 extrema, float ones float64 sums (np.bincount adds in
    raster order) and float32 extrema; without an image the four are None.  Ids must lie in [0, n_max]."""
    lab = np.asarray(labels).astype(np.int64)
    H, W = lab.shape
    n_max = int(lab.max()) if n_max is None else int(n_max)
    assert lab.min() >= 0 and lab.max() <= n_max
    N = n_max + 1
    flat = lab.ravel()
    yy, xx = (c.ravel().astype(np.int64) for c in np.mgrid[0:H, 0:W])

    def count(w=None):
        if w is None:
            return np.bincount(flat, minlength=N).astype(np.int64)
        if w.dtype.kind == "f":
            return np.bincount(flat, weights=w, minlength=N)
        out = np.zeros(N, np.int64)
        np.add.at(out, flat, w)                                  # bincount's weights are float64: integers above 2^53 would round
        return out

    def extreme(v, op, start):
        out = np.full(N, start, v.dtype)
        op.at(out, flat, v)
        return out

    area = count()
    on = area > 0
    bbox = np.stack([extreme(yy, np.minimum, H), extreme(xx, np.minimum, W), extreme(yy, np.maximum, -1) + 1,
                     extreme(xx, np.maximum, -1) + 1], axis=1)
    bbox[~on] = 0
    frame, opened, contact = (count(e.ravel()) for e in edge_counts(lab))
    out = {"area": area, "bbox": bbox.astype(np.int32), "moments": np.stack([count(yy), count(xx), count(yy * yy), count(xx * xx), count(xx * yy)], axis=1),
           "frame": frame, "open": opened, "contact": contact, "v_sum": None, "v_sum2": None, "v_min": None, "v_max": None, "present": on}
    if image is not None:
        img = np.asarray(image)
        assert img.shape == lab.shape
        if img.dtype.kind == "f":
            v = img.astype(np.float32).ravel()
            assert np.isfinite(v).all()
            d = v.astype(np.float64)
            out["v_sum"], out["v_sum2"] = count(d), count(d * d)
            lo, hi = extreme(v, np.minimum, np.float32(np.inf)), extreme(v, np.maximum, np.float32(-np.inf))
            out["v_min"], out["v_max"] = np.where(on, lo, np.float32(0)), np.where(on, hi, np.float32(0))
        else:
            v = img.astype(np.int64).ravel()
            assert v.min() >= 0 and v.max() < 65536
            out["v_sum"], out["v_sum2"] = count(v), count(v * v)
            lo, hi = extreme(v, np.minimum, 1 << 40), extreme(v, np.maximum, -1)
            out["v_min"], out["v_max"] = np.where(on, lo, 0).astype(np.int32), np.where(on, hi, 0).astype(np.int32)
    return out


def sums_batch(labels, images=None, n_max=None):
    labels = np.asarray(labels)
    n_max = int(labels.max()) if n_max is None else n_max
    rows = [sums(labels[b], None if images is None else images[b], n_max) for b in range(len(labels))]
    return {k: None if rows[0][k] is None else np.stack([r[k] for r in rows]) for k in FIELDS}


def abs_sums(labels, image, n_max):
    """(sum |v|, sum v^2) per id in float64: what the bounds on the float sums are stated in."""
    flat = np.asarray(labels).astype(np.int64).ravel()
    d = np.asarray(image).astype(np.float64).ravel()
    return np.bincount(flat, weights=np.abs(d), minlength=n_max + 1), np.bincount(flat, weights=d * d, minlength=n_max + 1)


def scipy_route(labels, image, n_max):
    """area, bbox, intensity sums, extrema and centroid of ids 1..n_max with scipy.ndimage, one call per quantity (the host
    route); ids that are absent give area 0, bbox None and whatever scipy gives for the rest."""
    lab = np.asarray(labels)
    index = np.arange(1, n_max + 1)
    img = np.asarray(image).astype(np.float64)
    return {"area": ndimage.sum_labels(np.ones_like(img), lab, index), "bbox": ndimage.find_objects(lab.astype(np.int32), n_max),
            "v_sum": ndimage.sum_labels(img, lab, index), "v_sum2": ndimage.sum_labels(img * img, lab, index),
            "v_min": ndimage.minimum(img, lab, index), "v_max": ndimage.maximum(img, lab, index),
            "centroid": ndimage.center_of_mass(np.ones_like(img), lab, index)}


def select(labels, keep, renumber=False):
    """labels [H,W] or [B,H,W], keep bool [n_max+1] or [B, n_max+1] -> int32 map."""
    lab = np.asarray(labels).astype(np.int64)
    keep = np.array(keep, dtype=bool)
    keep[..., 0] = False
    ids = np.cumsum(keep, axis=-1) if renumber else np.broadcast_to(np.arange(keep.shape[-1]), keep.shape)
    table = np.where(keep, ids, 0)
    if keep.ndim == 1:
        return table[lab].astype(np.int32)
    return np.stack([table[b][lab[b]] for b in range(len(lab))]).astype(np.int32)


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def hand_case():
    """The 3 x 5 map worked by hand in tests/test_measure_cpu.py: id 2 on the frame, id 5 inside, touching it."""
    return np.array([[2, 2, 0, 0, 0],
                     [2, 5, 5, 0, 0],
                     [0, 0, 0, 0, 0]], np.int32)


def every_pixel_its_own(H, W):
    return (np.arange(H * W, dtype=np.int32) + 1).reshape(H, W)


def wrapped_rows(H=7, W=5, ident=3):
    """Width 5 with the same id at the end of one row and the start of the next, all the way down: a run must break at the end
    of a row although the ids on either side of the break are equal."""
    m = np.zeros((H, W), np.int32)
    m[:, W - 2:] = ident
    m[1:, :2] = ident
    return m


def gaps_and_parts(H, W, n_max):
    """Ids with gaps up to n_max, one of them made of two disconnected parts, two that touch, background between."""
    m = np.zeros((H, W), np.int32)
    rs = np.random.RandomState(H * 1000 + W)
    ids = sorted(set(int(v) for v in rs.randint(1, n_max + 1, 6)) | {n_max})
    for k, i in enumerate(ids):
        y, x = rs.randint(0, H), rs.randint(0, W)
        m[y:y + 1 + H // 4, x:x + 1 + W // 4] = i
    m[0, 0] = ids[0]
    m[H - 1, W - 1] = ids[0]                                      # a second part, far from the first
    return m


def int_image(seed, shape, top=65536):
    return np.random.RandomState(seed).randint(0, top, shape).astype(np.int32)
