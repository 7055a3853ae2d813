"""Drop-in for the reference's tester.py: `from tester import testing`, same signature (tester.py:13),
output tree (images/ labels/ preds/ + test_iou.out, test_pe.out) and metrics; forward and argmax run
on the HIP path (unet_forward, unet_argmax2).  torchvision is absent here, so the three TIFFs are
written with PIL using torchvision.utils.save_image's conversion (clamp to [0,1], x255, round, RGB).

An extension: segment(unet, images) is the paper's overlap-tile inference (Ronneberger et al. 2015, Fig. 2) for
images of any size and shape, [H,W] in, [H,W] mask out (unet_tile_gather, unet_forward, unet_tile_stitch); tile_grid
is its geometry.  segment(..., views=...) averages the class probabilities over dihedral views of each image (apply_view,
undo_view, view_shape, parse_views; unet_tile_gather_view, unet_tile_stitch_view).  track(unet, frames) segments a time-lapse
and links its cells across frames (functions.track_cells; unet_link_frames)."""
import os
from time import time

import numpy as np
import torch

import _hip
from functions import (FLOOD_LEVELS, _area, _check_connectivity, cell_props, clean_mask, evaluation_metrics, label_cells,
                       metrics_from_counts, shape_seeds, split_cells, track_cells, watershed)
import optim as hip_optim

TILE_MARGIN = 92        # context each side of a tile's output that the valid convolutions eat: (S - So) / 2
TILE_CAP = 1212         # segment(tile_size=None) never picks a larger tile: the measured winner


def maybe_mkdir_p(path):
    os.makedirs(path, exist_ok=True)


def save_image(tensor, path):
    from PIL import Image
    t = tensor.detach().float().cpu()
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.shape[0] == 1:
        t = t.expand(3, -1, -1)
    arr = t.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
    Image.fromarray(arr).save(path)


def testing(unet, test_loader, batch_size, device, output_dir):
    n_classes = getattr(unet, 'n_classes', 2)
    if n_classes != 2:
        raise ValueError("testing() writes the reference's binary masks and IoU / PE; this net has %d classes - use segment() and "
                         "optim.crop_argmax_confusion / functions.metrics_from_confusion" % n_classes)
    t0 = time()
    for sub in ('images', 'preds', 'labels'):
        maybe_mkdir_p(os.path.join(output_dir, sub))
    first = None                      # Q5: the reference keeps only the first sample's metrics

    for n, (image, label) in enumerate(test_loader):
        with torch.no_grad():      # the reference leaves autograd on here (Q8); only memory differs
            logits = unet(image.to(device))
        side = label.shape[-1]
        off = int((logits.shape[-1] - side) / 2)
        # crop + argmax + IoU / pixel-error counts in one pass on the device (no per-image mask download)
        mask, stats = hip_optim.crop_argmax_metrics(logits, label)
        for sub, stem, t in (('images', 'image', image[0, 0, off:side + off, off:side + off]),
                             ('labels', 'label', label[0, 0].float()),
                             ('preds', 'pred', mask[0].float())):
            save_image(t, os.path.join(output_dir, sub, '%s%d.tif' % (stem, n)))
        if first is None:
            inter, union, diff = (int(v) for v in stats[0].tolist())
            first = metrics_from_counts(inter, union, diff, side * label.shape[-2])

    mean, std = np.mean(first, axis=1), np.std(first, axis=1)
    for k, fname in enumerate(('test_iou.out', 'test_pe.out')):
        np.savetxt(os.path.join(output_dir, fname), [mean[k], std[k]])

    for label_, value in (('Mean IoU testing:', mean[0]), ('Mean PE testing :', mean[1])):
        print(label_, "{:.6f}".format(value))
    print('Testing took    :', "{:.6f}".format(time() - t0), 's')
    print(' ')
    print('Testing is finished')


# ---- overlap-tile segmentation -------------------------------------------------------------------------------------------

def valid_tile_size(S):
    """S = 16L+60 with L even >= 8 (the sizes unet_forward accepts): 188, 220, 252, ..."""
    return S >= 188 and (S - 188) % 32 == 0


def _check_tile_size(S):
    if not valid_tile_size(S):
        hi = 188 + 32 * max(0, -(-(S - 188) // 32))
        near = [hi] if S < 188 else [hi - 32, hi]
        raise ValueError("tile_size %d is not a valid input size (16L+60, L even >= 8); the nearest valid size%s %s"
                         % (S, "s are" if len(near) > 1 else " is", " and ".join(str(v) for v in near)))


def reflect_index(i, n):
    """numpy.pad(mode='reflect') as an index map: ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ..., the edge pixel not repeated;
    period 2(n-1), so a pad wider than the image reflects again.  n >= 2.  (Not data.mirror_transform's asymmetric map.)"""
    period = 2 * (n - 1)
    i %= period
    return i if i < n else period - i


def tile_grid(H, W, S):
    """Overlap-tile geometry of an H x W image for tiles of input size S: returns (ny, nx, oy0, ox0).

    Output tiles are So = S - 184 square; the ny x nx grid of them is centred on the image with its top-left corner at
    (oy0, ox0) <= 0 in image coordinates.  Tile (b, i, j), linear index t = (b*ny + i)*nx + j, reads image rows
    [oy0 + i*So - 92, +S) and columns [ox0 + j*So - 92, +S), coordinates outside the image mapped by reflect_index
    (numpy.pad(mode='reflect'), the mirroring the reference trains with, data.py:111 — not the asymmetric
    mirror_transform of its test path), and its output covers rows [oy0 + i*So, +So), columns [ox0 + j*So, +So), clipped
    to the image.  These output rectangles partition the image."""
    So = S - 2 * TILE_MARGIN
    if So <= 0 or H < 1 or W < 1:
        raise ValueError("tile_grid: bad arguments H=%d W=%d S=%d" % (H, W, S))
    ny, nx = -(-H // So), -(-W // So)
    return ny, nx, -((ny * So - H) // 2), -((nx * So - W) // 2)


def auto_tile_size(H, W, cap=TILE_CAP):
    """The smallest valid S whose output So = S - 184 covers max(H, W), so the image is one tile, if that S is at most
    `cap`; otherwise `cap`."""
    S = 188 + 32 * max(0, -(-(max(H, W) - 4) // 32))
    return S if S <= cap else cap


# ---- dihedral views ---------------------------------------------------------------------------------------------------------

VIEW_SETS = {'rot4': (0, 3, 6, 5), 'flips': (0, 2, 4, 6), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}


def _view_code(v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 7:
        raise ValueError("view code %r is not an int in 0..7" % (v,))
    return int(v)


def view_shape(H, W, v):
    """(Hv, Wv) of view v of an H x W image: (W, H) for the transposed codes (v odd)."""
    return (W, H) if _view_code(v) & 1 else (H, W)


def apply_view(x, v):
    """View v (0..7) of x [..., H, W], a torch tensor (any device) or a numpy array; the result is a view, not a copy.
    With t = v & 1, fy = (v >> 1) & 1, fx = (v >> 2) & 1:  V = x.T if t else x;  if fy: V = V[::-1];  if fx: V = V[:, ::-1]
    (on the last two axes).  np.rot90(x, k), k = 0..3, are the codes 0, 3, 6, 5."""
    v = _view_code(v)
    tensor = torch.is_tensor(x)
    if v & 1:
        x = x.transpose(-1, -2) if tensor else np.swapaxes(x, -1, -2)
    axes = [a for a, on in ((-2, v & 2), (-1, v & 4)) if on]
    if axes:
        x = torch.flip(x, axes) if tensor else np.flip(x, axes)
    return x


def undo_view(x, v):
    """The inverse of apply_view(., v): undo_view(apply_view(x, v), v) == x."""
    v = _view_code(v)
    tensor = torch.is_tensor(x)
    axes = [a for a, on in ((-2, v & 2), (-1, v & 4)) if on]
    if axes:
        x = torch.flip(x, axes) if tensor else np.flip(x, axes)
    if v & 1:
        x = x.transpose(-1, -2) if tensor else np.swapaxes(x, -1, -2)
    return x


def parse_views(views):
    """A tuple of distinct view codes from 'rot4' (0, 3, 6, 5: the four rotations), 'flips' (0, 2, 4, 6), 'd4' (all 8) or any
    non-empty sequence of distinct ints in 0..7, whose order is kept."""
    if isinstance(views, str):
        if views not in VIEW_SETS:
            raise ValueError("views %r is not one of %s or a sequence of view codes 0..7" % (views, ", ".join(map(repr, VIEW_SETS))))
        return VIEW_SETS[views]
    try:
        vs = tuple(views)
    except TypeError:
        raise ValueError("views %r is not one of %s or a sequence of view codes 0..7" % (views, ", ".join(map(repr, VIEW_SETS))))
    if not vs:
        raise ValueError("views %r is empty" % (views,))
    vs = tuple(_view_code(v) for v in vs)
    if len(set(vs)) != len(vs):
        raise ValueError("views %r repeats the code %d" % (views, next(v for k, v in enumerate(vs) if v in vs[:k])))
    return vs


VIEW_FIRST, VIEW_LAST = 1, 2        # unet_tile_stitch_view's phase bits: store (not add) the probability; finalise after it


def _view_chunks(n_views, Tv, nb):
    """The tile list of n_views views of Tv tiles each, cut into chunks of at most nb: yields (t0, n, segments), a segment
    being (index of the view in the list, first tile within that view, number of tiles, offset in the chunk).  One view: every
    chunk is the one segment (0, t0, n, 0)."""
    T = n_views * Tv
    for t0 in range(0, T, nb):
        n = min(nb, T - t0)
        segs, off = [], 0
        while off < n:
            k, a = divmod(t0 + off, Tv)
            m = min(Tv - a, n - off)
            segs.append((k, a, m, off))
            off += m
        yield t0, n, segs


def split_instances(mask, fg_prob, high, *, connectivity=4):
    """The instance map of a foreground mask with touching cells split: the cores label_cells(fg_prob >= high)[0] are the seeds,
    functions.split_cells grows them back inside mask != 0 until two growths meet, and a component of the mask without a core
    stays a cell (orphans='keep').  mask and fg_prob [H,W] or [B,H,W] on a HIP device; returns int32 ids of the same shape.
    connectivity: 4 or 8 (else ValueError, checked first), for the cores' labelling, the growth and the orphans alike."""
    _check_connectivity("split_instances", connectivity)
    seeds = label_cells(fg_prob >= high, connectivity=connectivity)[0]
    return split_cells(seeds, mask, orphans='keep', connectivity=connectivity)[0]


def split_by_shape(mask, h=2.0, min_radius=0.0, edge='ignore', *, connectivity=4):
    """The instance map of a foreground mask with touching cells split by their shape alone, no probabilities needed: the seeds
    are functions.shape_seeds(mask, h, min_radius=min_radius, edge=edge)[0], the h-maxima of the mask's distance map whose peak
    reaches min_radius; functions.split_cells grows them back inside mask != 0 until two growths meet, and a component of the mask
    without a seed stays a cell (orphans='keep').  mask [H,W] or [B,H,W] on a HIP device; returns int32 ids of the same shape.
    connectivity: 4 or 8 (else ValueError), for the seeds (shape_seeds), the growth and the orphans alike."""
    seeds = shape_seeds(mask, h, min_radius=min_radius, edge=edge, connectivity=connectivity)[0]
    return split_cells(seeds, mask, orphans='keep', connectivity=connectivity)[0]


def split_by_watershed(mask, fg_prob, high, levels=64, *, connectivity=4):
    """The instance map of a foreground mask with touching cells split where the foreground probability dips: the cores
    label_cells(fg_prob >= high)[0] are the seeds, functions.watershed floods the landscape 1 - fg_prob (float32, quantised to
    `levels` levels) from them inside mask != 0, so two growths meet on the ridge of low probability between two cores and not
    halfway between them as in split_instances; a component of the mask without a core stays a cell, numbered after the seeds
    as split_cells(orphans='keep') numbers it.  mask and fg_prob [H,W] or [B,H,W] on a HIP device; returns int32 ids of the same
    shape.  connectivity: 4 or 8 (else ValueError, checked first), for the cores' labelling, the flood and the orphans alike."""
    _check_connectivity("split_by_watershed", connectivity)
    seeds = label_cells(fg_prob >= high, connectivity=connectivity)[0]
    labels = watershed(seeds, 1 - fg_prob.float(), mask=mask, levels=levels, connectivity=connectivity)[0]
    rest = label_cells((mask != 0) & (labels == 0), connectivity=connectivity)[0]
    return torch.where(rest > 0, rest + seeds.amax(dim=(-2, -1), keepdim=True), labels)


def _parse_shape_split(v):
    """shape_split of segment -> (h, min_radius); ValueError for anything but a number >= 0 or a pair of them."""
    def number(x):
        return not isinstance(x, bool) and isinstance(x, (int, float)) and 0 <= x <= 1 << 24
    if number(v):
        return float(v), 0.0
    if isinstance(v, (tuple, list)) and len(v) == 2 and number(v[0]) and number(v[1]):
        return float(v[0]), float(v[1])
    raise ValueError("segment: shape_split must be None, a number h >= 0 or a pair (h, min_radius) of numbers >= 0, got %r" % (v,))


_CLEAN_KEYS = ("fill_holes", "max_hole_area", "min_area", "drop_border", "connectivity")


def _parse_clean(v, n_classes):
    """clean of segment -> the keyword arguments of functions.clean_mask, or None; ValueError for anything but None, a bool or a
    dict of them, for values clean_mask refuses, and for filling holes in a mask of more than two classes."""
    if v is None or v is False:
        return None
    if v is True:
        kw = {}
    elif isinstance(v, dict) and all(k in _CLEAN_KEYS for k in v):
        kw = dict(v)
    else:
        raise ValueError("segment: clean must be None, True (fill all holes) or a dict with keys among %s, got %r" % (", ".join(_CLEAN_KEYS), v))
    if kw.get("connectivity", 4) not in (4, 8):
        raise ValueError("segment: clean: connectivity must be 4 or 8, got %r" % (kw["connectivity"],))
    _area("segment: clean", "max_hole_area", kw.get("max_hole_area"), none_ok=True)
    _area("segment: clean", "min_area", kw.get("min_area", 0))
    if n_classes > 2 and kw.get("fill_holes", True):
        raise ValueError("segment: clean with fill_holes on a %d-class net: a filled pixel has no class; pass "
                         "clean={'fill_holes': False, ...} to drop small or border cells only" % n_classes)
    return kw


def _check_keywords(return_instances, shape_split, split, measure, watershed, connectivity):
    """The rules of segment's keywords that need no device, each stated once and checked in this order whatever else is given;
    ValueError for the first one broken.  Returns (shape_split as (h, min_radius) or None, watershed as its levels or None)."""
    if connectivity is not None:
        _check_connectivity("segment", connectivity)
    if measure not in (False, True):
        raise ValueError("segment: measure must be False or True, got %r" % (measure,))
    if watershed is False:
        watershed = None
    if watershed is not None and watershed is not True and not (isinstance(watershed, int) and 1 <= watershed <= FLOOD_LEVELS):
        raise ValueError("segment: watershed must be None, True (64 levels) or an int in [1, %d], got %r" % (FLOOD_LEVELS, watershed))
    if measure and not return_instances:
        raise ValueError("segment: measure needs return_instances=True")
    if connectivity is not None and not return_instances:
        raise ValueError("segment: connectivity is the instance map's; it needs return_instances=True")
    if watershed is not None and split is None:
        raise ValueError("segment: watershed needs split=high, the cores it floods from")
    if watershed is not None and shape_split is not None:
        raise ValueError("segment: watershed floods the probabilities from the cores of split; it does not combine with shape_split")
    if split is not None:
        if not return_instances:
            raise ValueError("segment: split needs return_instances=True")
        if isinstance(split, bool) or not isinstance(split, (int, float)) or not 0 < split <= 1:
            raise ValueError("segment: split must be None or a number in (0, 1], got %r" % (split,))
    if shape_split is not None:
        if not return_instances:
            raise ValueError("segment: shape_split needs return_instances=True")
        if split is not None:
            raise ValueError("segment: shape_split and split are two ways to seed one growth; give one of them")
        shape_split = _parse_shape_split(shape_split)
    return shape_split, 64 if watershed is True else watershed


def _instance_map(mask, fg_prob, split, shape_split, watershed, connectivity):
    """The instance map segment returns, of the (cleaned) mask: split, shape_split and watershed as _check_keywords left them;
    fg_prob is read only with split."""
    if watershed is not None:
        return split_by_watershed(mask, fg_prob, float(split), watershed, connectivity=connectivity)
    if split is not None:
        return split_instances(mask, fg_prob, float(split), connectivity=connectivity)
    if shape_split is not None:
        return split_by_shape(mask, *shape_split, connectivity=connectivity)
    return label_cells(mask, connectivity=connectivity)[0]


def segment(unet, images, tile_size=None, max_batch=16, normalise=True, return_probs=False, return_instances=False, views=None,
            clean=None, shape_split=None, split=None, *, measure=False, watershed=None, connectivity=None):
    """Segment images of any size and shape with the overlap-tile strategy; returns the int64 argmax mask of the same
    shape as `images` (and the float32 foreground probability softmax(logits)[1] with return_probs).  A K-class net
    (Unet(n_classes=K), K > 2) gives the K-way argmax (ties -> the lowest class) and, with return_probs, the softmax of all
    K classes, [B,K,H,W] ([K,H,W] for a single image) (unet_tile_stitch_k).  With return_instances the returned tuple gains,
    as its last element, the int32 instance map of the mask, shaped like the mask: 0 where mask == 0, else the number 1..n of
    the pixel's 4-connected component of mask != 0 in raster order (functions.label_cells, unet_label_components), computed
    on the device right after the last stitch, on the same stream.

    images: device tensor [H,W] or [B,H,W], float32 (uint8 / uint16 are converted once), H, W >= 2.
    tile_size: the network's input size S per tile (16L+60, L even >= 8); None = auto_tile_size(H, W).
    max_batch: tiles per forward (with bf16 tensors, fewer when max_batch tiles would make an activation tensor of 2 GiB
        or more).  The tiles go through the module's own no-grad forward (its handle, unet_set_math and
        base_ch apply) in chunks: gather (unet_tile_gather), forward (unet_forward), stitch (unet_tile_stitch), all on the
        current stream; tile, logit and workspace buffers are allocated once per call.
    normalise: each image becomes (x - min) / (max - min) first, as the reference's ImageDataset_test does (data.py:188);
        the min / max are read back once before the first chunk, and a constant image raises ValueError.
    views: None, or what parse_views accepts ('rot4', 'flips', 'd4', a sequence of view codes): the class probabilities are
        averaged over these dihedral views of each image (apply_view) and the mask is taken from the average: prob > 0.5, or
        for K > 2 the argmax of the summed probabilities, ties -> the lowest class.  No view is materialised: the tiles of all
        views form one list, in the order of the codes, which is cut into the same chunks of max_batch, so one forward may hold
        tiles of several views (unet_tile_gather_view per view in the chunk, one unet_forward, unet_tile_stitch_view per view).
        The sum runs in the order of the codes and is deterministic.  views=(0,) gives the probabilities of views=None bit for
        bit; its mask is prob > 0.5 and not l1 > l0, which differ only where prob == 0.5 exactly (logit differences below
        about 6e-8, where 1 + exp(l0 - l1) rounds to 2).
    clean: None, True or a dict of functions.clean_mask's keyword arguments (fill_holes, max_hole_area, min_area, drop_border,
        connectivity): the mask is cleaned on the device right after the last stitch, on the same stream, before the instance map
        is made of it: holes filled, small cells and cells on the frame dropped.  True fills all holes and does nothing else.
        The mask returned is the cleaned one; the probabilities are untouched; it does not need return_instances.  A hole in a
        cell is background to the distance map, so shape_split over-splits a cell that has one.  With a K > 2 net a filled
        pixel would have no class: fill_holes true raises ValueError there, min_area and drop_border alone (fill_holes=False)
        are allowed and a kept pixel keeps its class.
    split: None, or a float in (0, 1] (needs return_instances, else ValueError): the instance map becomes
        split_instances(mask, fg_prob, split), touching cells split by growing the cores fg_prob >= split back inside the mask
        (functions.split_cells), on the same stream after the last stitch.  fg_prob is the foreground probability of the call:
        prob for K = 2, 1 - prob[:, 0] for K > 2 (allocated internally without return_probs; the mask does not depend on it).
    shape_split: None, a number h >= 0 or a pair (h, min_radius) (needs return_instances, not together with split, else
        ValueError): the instance map becomes split_by_shape(mask, h, min_radius), touching cells split at the h-maxima of the
        mask's own distance map (functions.shape_seeds, functions.split_cells), on the same stream after the last stitch.  It
        reads the mask alone, so it works with views= as it does without.
    measure: False or True (needs return_instances, else ValueError): the returned tuple gains, after the instance map, the
        functions.CellProps of functions.cell_props(instances, images): one row of shape and intensity properties per cell of
        the instance map as returned (after clean and split), the intensities those of the input images as given (not
        normalised).  The tuple is then (mask[, prob], instances, props).
    watershed: None, True (64 levels) or an int in [1, 65536] (needs split, not together with shape_split, else ValueError):
        the instance map becomes split_by_watershed(mask, fg_prob, split, levels): the cores fg_prob >= split flood the
        landscape 1 - fg_prob inside the mask (functions.watershed), so the cut between two touching cells follows the dip in
        foreground probability where split alone puts it halfway between the cores.  clean and measure compose with it as they
        do with split.  Flooding the inverted distance map from the seeds of functions.shape_seeds is a composition of
        functions.watershed and functions.distance_map and has no option here.
    connectivity: None (not given: 4), 4 or 8 (given, it needs return_instances, else ValueError): the connectivity of the
        instance map, throughout: label_cells(mask, connectivity=c), or with split, shape_split or split + watershed,
        split_instances, split_by_shape or split_by_watershed with connectivity=c (cores or seeds, growth or flood, and orphans
        alike).  The mask and the probabilities do not depend on it; clean keeps its own connectivity key.
    The keywords are checked before anything else, in one order (_check_keywords): the values of connectivity, measure and
    watershed, what each of them needs, then split and shape_split; then the images, device first; then max_batch, clean, views
    and the tile size.
    Geometry and mirroring: tile_grid."""
    shape_split, watershed = _check_keywords(return_instances, shape_split, split, measure, watershed, connectivity)
    if not images.is_cuda:
        raise RuntimeError("segment: the HIP path needs the images on a HIP device (got %s); there is no CPU fallback - "
                           "use unet.to('cuda:0') and images.to('cuda:0')" % images.device)
    if images.dim() not in (2, 3):
        raise ValueError("segment: expected images [H,W] or [B,H,W], got %s" % (tuple(images.shape),))
    if images.dtype not in (torch.float32, torch.uint8, torch.uint16):
        raise ValueError("segment: expected float32, uint8 or uint16 images, got %s" % images.dtype)
    single = images.dim() == 2
    x = (images[None] if single else images).to(torch.float32).contiguous()
    B, H, W = x.shape
    if H < 2 or W < 2:
        raise ValueError("segment: images must be at least 2x2 to be mirrored, got %dx%d" % (H, W))
    if B < 1:
        raise ValueError("segment: empty batch")
    if max_batch < 1:
        raise ValueError("segment: max_batch must be >= 1")
    K = getattr(unet, 'n_classes', 2)
    clean = _parse_clean(clean, K)
    vs = None if views is None else parse_views(views)

    S = auto_tile_size(H, W) if tile_size is None else int(tile_size)
    _check_tile_size(S)
    So = S - 2 * TILE_MARGIN
    # one tile grid per view, whose tiles form one list; a transposed view has as many tiles: its grid is (nx, ny)
    grids = [tile_grid(*view_shape(H, W, v), S) for v in ((0,) if vs is None else vs)]
    Tv = B * grids[0][0] * grids[0][1]
    nb = min(max_batch, len(grids) * Tv)
    dev = x.device
    h = unet._get_handle(dev.index)
    L = _hip.lib()
    if L.unet_activation_bytes(h.h) == 2:
        # bf16 tensors (unet_set_math(2)): the bf16 kernels address each activation tensor through a 32-bit buffer
        # descriptor, so a chunk's largest one, conv11c's output [nb, S-2, S-2, base_ch], must stay below 2 GiB
        nb = max(1, min(nb, (2 ** 31 - 2) // ((S - 2) ** 2 * unet.base_ch * 2)))
    with torch.cuda.device(dev):
        ptab = _hip.ptr_table([p.detach() for p in unet._params()])
        mm = None
        if normalise:
            mm = torch.empty(B, 2, dtype=torch.float32, device=dev)
            _hip.check(L.unet_minmax(_hip.ptr(x), B, H * W, _hip.ptr(mm), _hip.stream(dev)), "unet_minmax")
            lohi = mm.cpu()
            flat = (lohi[:, 0] == lohi[:, 1]).nonzero().flatten().tolist()
            if flat:
                raise ValueError("segment: image(s) %s are constant; normalise=True would divide by zero" % flat)
        tiles = torch.empty(nb, 1, S, S, dtype=torch.float32, device=dev)
        logits = torch.empty(nb, K, So, So, dtype=torch.float32, device=dev)
        nbytes = h.workspace_bytes(nb, S, False)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        mask = torch.empty(B, H, W, dtype=torch.int64, device=dev)
        prob = None
        if return_probs or vs is not None or split is not None:
            prob = torch.empty((B, H, W) if K == 2 else (B, K, H, W), dtype=torch.float32, device=dev)
        st = _hip.stream(dev)

        # without views a chunk is one segment (0, t0, n, 0) of the one grid: the plain entries, the mask from l1 > l0
        for _, n, segs in _view_chunks(len(grids), Tv, nb):
            for k, a, m, off in segs:
                gy, gx, y0, x0 = grids[k]
                if vs is None:
                    _hip.check(L.unet_tile_gather(_hip.ptr(x), B, H, W, _hip.ptr(mm), S, y0, x0, gy, gx, a, m, _hip.ptr(tiles[off:]), st),
                               "unet_tile_gather")
                else:
                    _hip.check(L.unet_tile_gather_view(_hip.ptr(x), B, H, W, _hip.ptr(mm), S, vs[k], y0, x0, gy, gx, a, m,
                                                       _hip.ptr(tiles[off:]), st), "unet_tile_gather_view")
            _hip.check(L.unet_forward(h.h, ptab, _hip.ptr(tiles), _hip.ptr(logits), n, S, _hip.ptr(ws), nbytes, 0, st),
                       "unet_forward")
            for k, a, m, off in segs:
                gy, gx, y0, x0 = grids[k]
                if vs is not None:
                    phase = (VIEW_FIRST if k == 0 else 0) | (VIEW_LAST if k == len(vs) - 1 else 0)
                    _hip.check(L.unet_tile_stitch_view(_hip.ptr(logits[off:]), So, K, vs[k], y0, x0, gy, gx, a, m, B, H, W, phase,
                                                       len(vs), _hip.ptr(prob), _hip.ptr(mask), st), "unet_tile_stitch_view")
                elif K == 2:
                    _hip.check(L.unet_tile_stitch(_hip.ptr(logits[off:]), So, y0, x0, gy, gx, a, m, B, H, W, _hip.ptr(mask),
                                                  _hip.ptr(prob), st), "unet_tile_stitch")
                else:
                    _hip.check(L.unet_tile_stitch_k(_hip.ptr(logits[off:]), So, K, y0, x0, gy, gx, a, m, B, H, W, _hip.ptr(mask),
                                                    _hip.ptr(prob), st), "unet_tile_stitch_k")

        if clean is not None:
            mask = clean_mask(mask, **clean)
        inst = None
        if return_instances:
            fg = None if split is None else prob if K == 2 else 1 - prob[:, 0]
            inst = _instance_map(mask, fg, split, shape_split, watershed, 4 if connectivity is None else connectivity)

    if single:
        mask = mask[0]
        prob = prob[0] if return_probs else None
        inst = inst[0] if return_instances else None
    out = (mask,) + ((prob,) if return_probs else ()) + ((inst,) if return_instances else ())
    if measure:
        out += (cell_props(inst, images if images.dtype == torch.float32 else images.to(torch.float32)),)
    return out if len(out) > 1 else mask


def track(unet, frames, *, reach=None, min_overlap=0.0, divisions=True, max_children=2, **segment_kwargs):
    """Segment a time-lapse and follow its cells: segment(unet, frames, return_instances=True, **segment_kwargs) on frames
    [T,H,W], then functions.track_cells(instances, reach=.., min_overlap=.., divisions=.., max_children=..) on the instance map,
    on the device.  segment_kwargs are segment's own (tile_size, views, clean, split, shape_split, watershed, ...);
    return_instances, return_probs and measure are not among them.  Returns (mask, track_maps, tracks): the mask of segment;
    track_maps int32 [T,H,W], 0 where the instance map is 0, else the label of the cell's track, the same from the track's first
    frame to its last; tracks the functions.Tracks, whose table and ctc_text() are the Cell Tracking Challenge's res_track.txt."""
    taken = [k for k in ("return_instances", "return_probs", "measure") if k in segment_kwargs]
    if taken:
        raise ValueError("track: %s cannot be passed on; track returns (mask, track_maps, tracks)" % ", ".join(taken))
    if not torch.is_tensor(frames) or frames.dim() != 3:
        raise ValueError("track: expected frames [T,H,W], got %s" % (tuple(frames.shape) if torch.is_tensor(frames) else type(frames),))
    mask, instances = segment(unet, frames, return_instances=True, **segment_kwargs)
    track_maps, tracks = track_cells(instances, reach=reach, min_overlap=min_overlap, divisions=divisions, max_children=max_children)
    return mask, track_maps, tracks
