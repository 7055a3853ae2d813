"""Drop-in for the reference's functions.py helpers that sit either side of the hot path.

input_size_compute / evaluation_metrics / IoU / Pixel_error / class_balance keep the reference's
names, arguments and results (functions.py:82-213).  They are host-side bookkeeping on labels and
388^2 masks (SURVEY §2 rows 5,7,8: out of scope as kernels).  weighted_map (functions.py:7-78, the paper's
border-weighted loss map) runs on the device only (unet_weighted_map); the reference's own OpenCV path has no
host counterpart here.  label_cells and seg_measure are extensions, device only as well: the cell instances of a mask
(unet_label_components) and the Cell Tracking Challenge SEG measure of two instance maps (unet_instance_overlap), the score
the goals of trainer.py:20-26 are stated in.  grow_cells, pair_table and rand_scores extend them to the other table those goals
quote (Ronneberger et al. 2015, Table 1, ISBI 2012): nearest-cell growth of an instance map (unet_grow_labels), the contingency
table of two instance maps on ground-truth foreground (unet_partition_pairs), and the Rand and information scores formed from it.
warp_labels and warping_error add that table's third column: the topology-preserving warp of a ground-truth mask towards a
prediction (unet_warp_init / unet_warp_sweeps / unet_warp_finish) and the disagreement it leaves.
split_cells is the instance post-processing after label_cells: seeds grown back inside a mask along 4-neighbour steps until two
growths meet (unet_geodesic_init / unet_geodesic_sweeps / unet_geodesic_finish), which splits touching cells.
split_cells, watershed, reconstruct and shape_seeds take connectivity=8 as label_cells does: 8-neighbour steps (the _conn entries).
watershed is the same growth led by an image: seeded flooding of an intensity landscape, plateaus cut at their geodesic midline
(unet_flood_init / unet_flood_sweeps / unet_flood_assign / unet_flood_finish).
distance_map, reconstruct and shape_seeds give it seeds from the shape of the mask alone: the exact interior distance map
(unet_distance_map), grey reconstruction by dilation (unet_reconstruct_init / unet_reconstruct_sweeps / unet_reconstruct_finish),
and the h-maxima of the distance map with a minimum radius, labelled (unet_shape_heights / unet_shape_lower / unet_shape_maxima).
clean_mask, fill_holes and remove_small are the clean-up in front of all that, between the argmax and the instance map: holes
filled, small cells and cells on the frame dropped, with either connectivity (unet_clean_mask); label_cells(connectivity=8) is the
8-connected labelling that goes with it (unet_label_components_conn).
cell_sums, props_from_sums, cell_props and select_cells are the step after the instance map: one row of exact integers per cell
(unet_cell_sums), the usual shape and intensity properties formed from them on the host, and the per-id remap that drops or
renumbers cells by any decision taken on those rows (unet_remap_labels).
cell_hulls, hull_props, cell_neighbours and neighbour_counts measure what that table cannot see: the convex hull of every cell
with its area and calliper widths as exact integers (unet_cell_hulls), solidity and the Feret diameters formed from them on the
host, and the list of touching pairs of cells with the length of their common border (unet_cell_contacts).
mask_boundary, surface_sums, scores_from_surface and boundary_scores score a mask by where its contour lies: the contour of a
region (unet_mask_boundary), per image and direction the exact integers and the fp64 sum of the distances from one contour to the
other (unet_surface_sums), and the Hausdorff distance, its percentile, the average symmetric surface distance and the normalised
surface Dice formed from them on the host.
link_frames, tracks_from_links and track_cells carry the instance maps of a time-lapse across frames: for every cell the cell of the
frame before that it overlaps most (unet_link_frames), the tracks, divisions and the Cell Tracking Challenge's res_track.txt table
formed from those links on the host, and the maps relabelled by track on the device (unet_remap_labels).
"""
import collections
import fractions
import math

import numpy as np
import torch


# ---- what the device-only ops share: the checks of their inputs and the table protocol ------------------------------------

def _device_only(name, entry, *tensors):
    if not all(torch.is_tensor(t) and t.is_cuda for t in tensors):
        raise NotImplementedError("%s runs on the HIP device only (%s): move the input to the device first, e.g. with .cuda(); "
                                  "there is no CPU implementation" % (name, entry))


def _planes(name, t):
    """[H,W] or [B,H,W] -> contiguous [B,H,W]"""
    if t.dim() not in (2, 3):
        raise ValueError("%s takes [H,W] or [B,H,W], got %s" % (name, tuple(t.shape)))
    if t.numel() == 0:
        raise ValueError("%s: empty input %s" % (name, tuple(t.shape)))
    return (t[None] if t.dim() == 2 else t).contiguous()


_CODES = {torch.int64: 0, torch.float32: 1, torch.int32: 2, torch.uint8: 3}      # the dtype codes of the library's entry points


def _int_code(x, uint8_ok=False, int32_ok=True):
    """The tensor in one of the widths the library reads, and its dtype code: float -> float32 (1), int64 and the unsigned
    types int32 cannot hold -> int64 (0), uint8 stays where the entry point takes it (3), every other integer type (uint16
    from a numpy-born image included) and bool -> int32 (2), or int64 (0) where the entry point reads only that and float32."""
    if x.is_floating_point():
        x = x.float()
    elif x.dtype == torch.uint8 and uint8_ok:
        pass
    elif not int32_ok or x.dtype in (torch.int64, torch.uint32, torch.uint64):
        x = x.to(torch.int64)
    else:
        x = x.to(torch.int32)
    return x, _CODES[x.dtype]


def _id_code(lab):
    """The dtype code of an id map, which _id_maps has held to int32 or int64 and which goes in as it is."""
    return _CODES[lab.dtype]


def _unbatch(like, *ts):
    """ts ([B,H,W] tensors or tables [B, ...], None passes through) without the batch axis that _planes gave an input `like` of
    [H,W]: one value for one t, else a tuple."""
    if like.dim() == 2:
        ts = tuple(t if t is None else t[0] for t in ts)
    return ts[0] if len(ts) == 1 else ts


# The checks that the ops on two or three planes of one shape open with, in the order every one of them keeps: _all_tensors,
# _same_shape, the dtype rules (_need_ids, ...), then _device_planes.  An op's checks of its other arguments sit between them.

def _all_tensors(name, entry, tensors):
    for t in tensors:
        if not torch.is_tensor(t):
            raise NotImplementedError("%s takes tensors on the HIP device (%s); there is no CPU implementation" % (name, entry))


def _same_shape(name, what, tensors, ranked=True):
    """One shape (and, if ranked, [H,W] or [B,H,W]), else ValueError("<name> takes <what>, got <the shapes>")."""
    shape = tensors[0].shape
    for t in tensors:
        if t.shape != shape or (ranked and len(shape) not in (2, 3)):
            raise ValueError("%s takes %s, got %s" % (name, what, ", ".join(str(tuple(t.shape)) for t in tensors)))


def _need_ids(name, what, *tensors):
    for t in tensors:
        if t.dtype not in (torch.int32, torch.int64):
            raise ValueError("%s takes int32 or int64 %s, got %s" % (name, what, t.dtype))


def _device_planes(name, entry, tensors, sizes=None):
    """The tensors as contiguous [B,H,W] (_planes, then sizes(name, B, H, W): ValueError on any device), then the device
    (NotImplementedError)."""
    planes = [_planes(name, t) for t in tensors]
    if sizes is not None:
        sizes(name, *planes[0].shape)
    _device_only(name, entry, *tensors)
    return planes


def _id_maps(name, entry, *maps):
    """The checks of the ops that take one or two id maps: equal shape, rank, dtype, size (ValueError, on any device), then the
    device (NotImplementedError); returns them as contiguous [B,H,W]."""
    _same_shape(name, "id maps of equal shape [H,W] or [B,H,W]", maps)
    _need_ids(name, "id maps", *maps)
    return _device_planes(name, entry, maps)


# ---- the checks of the other arguments: one statement of each rule, the message is the caller's ----------------------------

_INTEGERS = (int, np.integer)


def _int_in(v, lo, hi, message, types=_INTEGERS):
    """v if it is one of `types`, no bool, with lo <= v < hi; else ValueError(message % (v,))."""
    if isinstance(v, bool) or not isinstance(v, types) or not lo <= v < hi:
        raise ValueError(message % (v,))
    return v


def _real_in(v, lo, hi, message, types=(int, float)):
    """v if it is one of `types`, no bool, with lo <= v <= hi (which refuses nan); else ValueError(message % (v,))."""
    if isinstance(v, bool) or not isinstance(v, types) or not lo <= v <= hi:
        raise ValueError(message % (v,))
    return v


def _limit(name, what, v, cap=1 << 40, square=False):
    """An optional limit as the library takes it: None and inf -> -1 (none), else min(floor(v) or floor(v^2), cap); anything
    that is not >= 0, nan included, raises ValueError."""
    if v is None or v == math.inf:
        return -1
    if not v >= 0:
        raise ValueError("%s: %s must be None or a number >= 0, got %r" % (name, what, v))
    return min(int(math.floor(float(v) ** 2 if square else v)), cap)


def _host(t):
    """A device tensor, host tensor or array as a numpy array."""
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _status_words(status):
    """The status words [B] or [B, k] of a call summed over its images, read back in one copy: k Python ints."""
    return status.cpu().numpy().reshape(len(status), -1).sum(axis=0).tolist()


def _id_range(name, *maps):
    """(max id of each map), read back in one copy; negative ids and ids >= 2^24 raise ValueError."""
    lo = maps[0].min()
    for t in maps[1:]:
        lo = torch.minimum(lo, t.min())
    vals = [int(v) for v in torch.stack([lo.long()] + [t.max().long() for t in maps]).tolist()]
    if vals[0] < 0:
        raise ValueError("%s: negative ids (the smallest is %d)" % (name, vals[0]))
    if max(vals[1:]) >= 1 << 24:
        raise ValueError("%s: ids must be below 2^24, got up to %d" % (name, max(vals[1:])))
    return vals[1:]


def _table_call(entry, dev, n, head, slots, room, scratch_dims, outputs, bad, limits):
    """The protocol of the entries that count into the pair table (csrc/ov_table.hpp), from slots (None: the power of two with
    room + 1024 slots): allocate the entry's outputs (outputs(slots)) and scratch (scratch_dims(slots)), call entry(*head, slots,
    *outputs, status, scratch), read the [n, 2] status words back once; status[:, 0], the pixels whose ids the entry refuses,
    raises ValueError(bad % ((count,) + limits)); status[:, 1], the pixels a full table dropped, doubles the table and repeats,
    which ends: a table with more slots than pixels cannot fill up.  Returns (outputs, slots)."""
    import _hip
    status = torch.empty(n, 2, dtype=torch.int64, device=dev)
    slots = 1 << (room + 1024 - 1).bit_length() if slots is None else int(slots)
    while True:
        outs = outputs(slots)
        scratch = _hip.scratch(entry, dev, *scratch_dims(slots))
        _hip.run(entry, dev, *head, slots, *[_hip.ptr(o) for o in outs], _hip.ptr(status), _hip.ptr(scratch))
        refused, dropped = _status_words(status)
        if refused:
            raise ValueError(bad % ((refused,) + limits))
        if not dropped:
            return outs, slots
        slots *= 2


def _overlap_call(entry, gt, pred, ng_max, np_max, slots, scratch_dims, outputs, bad):
    """_table_call for unet_instance_overlap and unet_partition_pairs on int32 maps [B,H,W]; returns the outputs."""
    import _hip
    head = (_hip.ptr(gt), _hip.ptr(pred)) + tuple(gt.shape) + (ng_max, np_max)
    return _table_call(entry, gt.device, len(gt), head, slots, 4 * (ng_max + np_max), scratch_dims, outputs, bad, (ng_max, np_max))[0]


def _sorted_pairs(keys, counts, n_pairs):
    """The compacted (key, count) list of unet_partition_pairs or unet_cell_contacts as int64 numpy arrays (b, i, j, n), sorted by
    (b, i, j): the keys are distinct and unsigned, b << 48 | i << 24 | j, so their order is that of the triples."""
    n = int(n_pairs.item())
    k, c = keys[:n].cpu().numpy().view(np.uint64), counts[:n].cpu().numpy().astype(np.int64)
    order = np.argsort(k)
    k, c = k[order], c[order]
    return tuple((k >> np.uint64(s) & np.uint64(m)).astype(np.int64) for s, m in ((48, 0xFFFF), (24, 0xFFFFFF), (0, 0xFFFFFF))) + (c,)


def weighted_map(gt_batch, *, w0=20, sig2=25, return_objects=False):
    """Border weight map of Ronneberger et al. 2015, eq. 2 (functions.py:7-78) for {0,1} labels [B,H,W] on a HIP device:
    1 on cells; on background w_c + w0 * exp(-(d1 + d2)^2 / (2 sig2)), d1 / d2 the exact distances to the nearest and
    second-nearest distinct 4-connected cell (d2 = 0 when the image has one).  w_c = count(1) / count(0) takes the
    label's dtype as in the reference (torch.empty_like(gt)): truncated for integer labels (DESIGN Q9), fp32 for float
    labels.  Returns float32 [B,H,W] (and the int32 [B] component counts with return_objects=True).  A one-class image
    raises IndexError as the reference does at counts[1]; host tensors raise NotImplementedError (no CPU path)."""
    _device_only("weighted_map", "unet_weighted_map", gt_batch)
    import _hip
    if gt_batch.dim() != 3:
        raise ValueError("weighted_map takes labels [B,H,W], got %s" % (tuple(gt_batch.shape),))
    gt, code = _int_code(gt_batch.contiguous(), int32_ok=False)
    B, H, W = gt.shape
    w = torch.empty(B, H, W, dtype=torch.float32, device=gt.device)
    counts = torch.empty(B, dtype=torch.int64, device=gt.device)
    n_objects = torch.empty(B, dtype=torch.int32, device=gt.device)
    if B * H * W == 0:
        raise IndexError("index 1 is out of bounds for dimension 0 with size 0")
    scratch = _hip.scratch("unet_weighted_map", gt.device, B, H, W)
    _hip.run("unet_weighted_map", gt.device, _hip.ptr(gt), code, B, H, W, float(w0), float(sig2), _hip.ptr(w), _hip.ptr(counts),
             _hip.ptr(n_objects), _hip.ptr(scratch))
    if bool(((counts == 0) | (counts == H * W)).any()):      # the reference indexes counts[1]: a one-class image raises
        raise IndexError("index 1 is out of bounds for dimension 0 with size 1")
    return (w, n_objects) if return_objects else w


def label_cells(mask, connectivity=4):
    """The cell instances of a foreground mask [H,W] or [B,H,W] on a HIP device (foreground = value != 0; bool / integer masks
    go in as int64, float ones as float32): returns (labels, n_objects), labels int32 of the mask's shape, 0 on background
    and 1..n on the 4-connected components, numbered in raster order of their first pixel like scipy.ndimage.label and
    cv.connectedComponents(connectivity=4) (functions.py:47); n_objects int32 [B] ([1] for a single image) = n.
    connectivity=8 joins diagonal neighbours too (scipy.ndimage.label with the full 3 x 3 structure, the same numbering;
    unet_label_components_conn, which reads uint8 and int32 masks as they are); anything but 4 or 8 raises ValueError.
    Host tensors raise NotImplementedError (no CPU path)."""
    _check_connectivity("label_cells", connectivity)
    entry = "unet_label_components" if connectivity == 4 else "unet_label_components_conn"
    _device_only("label_cells", entry, mask)
    import _hip
    m, code = _int_code(_planes("label_cells", mask), uint8_ok=connectivity == 8, int32_ok=connectivity == 8)
    B, H, W = m.shape
    labels = torch.empty(B, H, W, dtype=torch.int32, device=m.device)
    n_objects = torch.empty(B, dtype=torch.int32, device=m.device)
    scratch = _hip.scratch(entry, m.device, B, H, W)
    _hip.run(entry, m.device, _hip.ptr(m), code, B, H, W, *((8, 1) if connectivity == 8 else ()), _hip.ptr(labels), _hip.ptr(n_objects),
             _hip.ptr(scratch))
    return _unbatch(mask, labels), n_objects


CleanInfo = collections.namedtuple("CleanInfo", "holes_filled pixels_filled cells_small pixels_small cells_border pixels_border cells_kept")


def _area(name, what, v, none_ok=False):
    if v is None and none_ok:
        return -1
    return min(int(_int_in(v, 0, math.inf, "%s: %s must be %san integer >= 0, got %%r" % (name, what, "None or " if none_ok else ""))), 1 << 62)


def clean_mask(mask, *, fill_holes=True, max_hole_area=None, min_area=0, drop_border=False, connectivity=4, return_info=False,
               return_action=False):
    """Clean a foreground mask [H,W] or [B,H,W] on a HIP device between the argmax and the instance map (foreground = value
    != 0): fill holes, drop small cells and cells on the frame, what scipy.ndimage.binary_fill_holes and skimage's
    remove_small_holes, remove_small_objects and clear_border do on the host.  connectivity 4 or 8 is the foreground's; the
    background takes the dual one (8 or 4), as in warp_labels, so no digital curve is both closed and leaky.
      hole   a component of the background with no pixel in the first or last row or column; its area is its own pixel count
             (foreground islands inside it do not count: remove_small_holes' convention).  Filled when fill_holes is true and
             max_hole_area is None or area <= max_hole_area.
      cell   a component of the mask after filling (an island inside a filled hole is part of the cell round it).  Dropped as
             small when area < min_area (remove_small_objects' convention: 0 and 1 drop nothing); with drop_border, a cell that
             is not small and has a pixel in the first or last row or column is dropped too.
    Returns the cleaned mask of the input's shape and dtype (bool comes back as bool; the other types follow _int_code with
    uint8 as it is): the input value on a kept foreground pixel, 1 on a filled one, 0 elsewhere.  With return_info it is followed
    by CleanInfo(holes_filled, pixels_filled, cells_small, pixels_small, cells_border, pixels_border, cells_kept), numpy int64
    [B] each, read back in one copy; with return_action by the uint8 action plane of the input's shape: 0 background that stays,
    1 foreground kept, 2 filled, 3 dropped as small, 4 dropped on the border.  Without return_info nothing is read back and
    nothing waits.  Exact integers on the device (unet_clean_mask: two labellings and two per-pixel passes, whatever the number
    of holes and cells).  A connectivity other than 4 or 8 and areas that are no integers >= 0 raise ValueError; host tensors
    raise NotImplementedError (no CPU path)."""
    _check_connectivity("clean_mask", connectivity)
    hole = _area("clean_mask", "max_hole_area", max_hole_area, none_ok=True)
    small = _area("clean_mask", "min_area", min_area)
    if not torch.is_tensor(mask):
        raise NotImplementedError("clean_mask takes a tensor on the HIP device (unet_clean_mask); there is no CPU implementation")
    (mk,) = _device_planes("clean_mask", "unet_clean_mask", [mask])
    import _hip
    m, code = _int_code(mk, uint8_ok=True)
    B, H, W = m.shape
    dev = m.device
    out = torch.empty_like(m)
    action = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if return_action else None
    info = torch.empty(B, 7, dtype=torch.int64, device=dev)
    scratch = _hip.scratch("unet_clean_mask", dev, B, H, W)
    _hip.run("unet_clean_mask", dev, _hip.ptr(m), code, B, H, W, connectivity, int(bool(fill_holes)), hole, small, int(bool(drop_border)),
             _hip.ptr(out), _hip.ptr(action), _hip.ptr(info), _hip.ptr(scratch))
    if out.dtype != mask.dtype:
        out = out.to(mask.dtype)
    res = (_unbatch(mask, out),)
    if return_info:
        res += (CleanInfo(*info.cpu().numpy().T.copy()),)
    if return_action:
        res += (_unbatch(mask, action),)
    return res if len(res) > 1 else res[0]


def fill_holes(mask, max_area=None, connectivity=4):
    """clean_mask(mask, max_hole_area=max_area, connectivity=connectivity): the holes of the mask filled, all of them or those
    of at most max_area pixels; nothing is dropped."""
    return clean_mask(mask, max_hole_area=max_area, connectivity=connectivity)


def remove_small(mask, min_area, connectivity=4):
    """clean_mask(mask, fill_holes=False, min_area=min_area, connectivity=connectivity): the cells of fewer than min_area
    pixels dropped; nothing is filled."""
    return clean_mask(mask, fill_holes=False, min_area=min_area, connectivity=connectivity)


CellSums = collections.namedtuple("CellSums", "area bbox moments frame open contact v_sum v_sum2 v_min v_max present")
CellProps = collections.namedtuple("CellProps", "area centroid bbox moments_central axis_major axis_minor eccentricity orientation "
                                                "equivalent_diameter extent perimeter contact_fraction touches_frame mean std min max")
MEASURE_EDGE = 32768                                                    # H, W of cell_sums: every integer sum fits 64 bits


def _measure_sizes(name, B, H, W):
    if max(H, W) > MEASURE_EDGE:
        raise ValueError("%s: H and W must be <= %d, got %d x %d" % (name, MEASURE_EDGE, H, W))


def cell_sums(labels, image=None, *, n_max=None):
    """One row of exact integers per cell of an instance map, on the device (unet_cell_sums): int32 / int64 ids [H,W] or
    [B,H,W] on a HIP device, 0 = background, ids in [0, 2^24), not necessarily consecutive or connected (the convention of
    grow_cells and seg_measure).  image: None or a tensor of the same shape under the map: uint8 / integer images with values in
    [0, 65536), or float images (read as float32) with finite values.  Returns CellSums of device tensors [B, n_max+1, ...]
    ([n_max+1, ...] for a single image); row 0 is the background, treated like any other id.  For id i over its pixels (y, x):
      area     int64
      bbox     int32 [.., 4]: (y0, x0, y1, x1), half-open like scipy.ndimage.find_objects
      moments  int64 [.., 5]: (sum y, sum x, sum y^2, sum x^2, sum x y)
      frame, open, contact  int64, counts over the four sides of every pixel: the side lies on the image frame; the neighbour
               has id 0 and i != 0; the neighbour has another id (for i = 0 any non-zero id).  Their sum is the crack-length
               perimeter; an edge between two ids is counted once for each
      v_sum, v_sum2, v_min, v_max  None without an image; int64 sums and int32 extrema, all exact, for an integer image;
               float64 sums (v^2 is exact in fp64; the adds round, in an order that can differ between runs) and exact float32
               extrema for a float image
      present  bool, area > 0; every field of an absent id is 0
    n_max: None reads the largest id back once (and checks the ids are in [0, 2^24)); an integer >= 0 skips that, and the call
    then waits for nothing until the status words are read at its end.  Pixels with an id outside [0, n_max], image values
    outside [0, 65536) and non-finite ones raise ValueError, as do shapes that differ and H or W above 32768; host tensors raise
    NotImplementedError (no CPU path).  Exact, every integer the same in every run, at a cost independent of the number of cells.
    props_from_sums turns the table into the usual shape and intensity properties."""
    (lab,) = _id_maps("cell_sums", "unet_cell_sums", labels)
    import _hip
    img, icode = None, 0
    if image is not None:
        if not torch.is_tensor(image) or image.shape != labels.shape:
            raise ValueError("cell_sums: the image must be a tensor of the labels' shape %s, got %s"
                             % (tuple(labels.shape), tuple(image.shape) if torch.is_tensor(image) else type(image).__name__))
        _device_only("cell_sums", "unet_cell_sums", image)
        img, icode = _int_code(_planes("cell_sums", image), uint8_ok=True)
    B, H, W = lab.shape
    _measure_sizes("cell_sums", B, H, W)
    if n_max is None:
        (n_max,) = _id_range("cell_sums", lab)
    n_max = int(_int_in(n_max, 0, 1 << 24, "cell_sums: n_max must be None or an integer in [0, 2^24), got %r"))
    dev, N = lab.device, n_max + 1
    isfloat = icode == 1
    area = torch.empty(B, N, dtype=torch.int64, device=dev)
    bbox = torch.empty(B, N, 4, dtype=torch.int32, device=dev)
    moments = torch.empty(B, N, 5, dtype=torch.int64, device=dev)
    edges = torch.empty(B, N, 3, dtype=torch.int64, device=dev)
    vsum = None if img is None else torch.empty(B, N, 2, dtype=torch.float64 if isfloat else torch.int64, device=dev)
    vrange = None if img is None else torch.empty(B, N, 2, dtype=torch.float32 if isfloat else torch.int32, device=dev)
    present = torch.empty(B, N, dtype=torch.bool, device=dev)
    status = torch.empty(B, 2, dtype=torch.int64, device=dev)
    scratch = _hip.scratch("unet_cell_sums", dev, B, n_max)
    _hip.run("unet_cell_sums", dev, _hip.ptr(lab), _id_code(lab), _hip.ptr(img), icode, B, H, W, n_max, _hip.ptr(area), _hip.ptr(bbox),
             _hip.ptr(moments), _hip.ptr(edges), _hip.ptr(vsum), _hip.ptr(vrange), _hip.ptr(present), _hip.ptr(status), _hip.ptr(scratch))
    bad_id, bad_v = _status_words(status)
    if bad_id:
        raise ValueError("cell_sums: %d pixels hold ids outside [0, %d]" % (bad_id, n_max))
    if bad_v:
        raise ValueError("cell_sums: %d pixels of the image hold %s" % (bad_v, "values that are not finite" if isfloat
                                                                       else "values outside [0, 65536)"))
    out = [area, bbox, moments, edges[..., 0], edges[..., 1], edges[..., 2]]
    out += [None] * 4 if img is None else [vsum[..., 0], vsum[..., 1], vrange[..., 0], vrange[..., 1]]
    out.append(present)
    return CellSums(*_unbatch(labels, *out))


def _exact_variance(on, n, s2, p, q):
    """(n * s2 - p * q) / n^2 in float64 where `on`, nan elsewhere: the numerator in Python integers (it reaches 2^90 for int64
    inputs at the limits of cell_sums), then the one division, correctly rounded.  A loop over the present rows only."""
    out = np.full(n.shape, np.nan)
    N, S2, P, Q = (v[on].astype(object) for v in (n, s2, p, q))
    out[on] = [a / b for a, b in zip(N * S2 - P * Q, N * N)]
    return out


def props_from_sums(sums):
    """The usual shape and intensity properties of every id from the table of cell_sums (a CellSums of device tensors, host
    tensors or arrays, [n_max+1, ...] or [B, n_max+1, ...]): pure numpy on the host.  Returns CellProps of float64 arrays of the
    table's leading shape (nan wherever an id is absent) unless stated:
      area                 float64 (nan for an absent id)
      centroid             [.., 2]: (mean y, mean x) in pixel coordinates (a pixel's centre is its integer index)
      bbox                 int32 [.., 4] as in the table (0 for an absent id)
      moments_central      [.., 3]: (mu_yy, mu_xx, mu_xy) / area, the second moments about the centroid per pixel, every pixel a
                           point mass at its centre.  Formed exactly: the raw sums are first re-centred on the box origin (y0, x0)
                           in integers, then area * S_yy' - S_y'^2 (and so on) in integers that cannot overflow, then one division
                           by area^2.  Never sum y^2 / area - (sum y / area)^2 on image coordinates
      axis_major, axis_minor   4 sqrt(lambda) of the two eigenvalues of that 2 x 2 tensor (the axes of the ellipse with the same
                           second moments; an h x w rectangle has 4 sqrt((w^2 - 1) / 12) and 4 sqrt((h^2 - 1) / 12))
      eccentricity         sqrt(1 - lambda_min / lambda_max), 0 for a cell whose moments vanish (a single pixel) or are isotropic
      orientation          the angle of the major axis in radians in (-pi/2, pi/2], measured from the x axis (the direction of
                           growing column index) towards the y axis (growing row index, downwards on a displayed image):
                           0.5 atan2(2 mu_xy, mu_xx - mu_yy).  A cell along y = x has +pi/4, along y = -x it has -pi/4, a tall one
                           pi/2; an isotropic one 0.  (skimage's regionprops measures from the row axis instead.)
      equivalent_diameter  sqrt(4 area / pi)
      extent               area / box area
      perimeter            frame + open + contact, the crack length (not skimage's sub-pixel estimate)
      contact_fraction     contact / perimeter
      touches_frame        bool, frame > 0 (False for an absent id)
      mean, std, min, max  of the image (std is the population one); None when the table has no image.  For an integer image
                           the variance is (area * sum v^2 - (sum v)^2) / area^2 with exact integers."""
    s = CellSums(*(None if t is None else _host(t) for t in sums))
    on = s.present.astype(bool) & (s.area > 0)
    nan = np.where(on, 0.0, np.nan)
    a = s.area.astype(np.int64)
    y0, x0 = s.bbox[..., 0].astype(np.int64), s.bbox[..., 1].astype(np.int64)
    bh, bw = s.bbox[..., 2] - y0, s.bbox[..., 3] - x0
    sy, sx, syy, sxx, sxy = (s.moments[..., k].astype(np.int64) for k in range(5))
    # re-centred on the box origin: the results lie in [0, 2^60], so int64 arithmetic (which wraps) is exact
    ry, rx = sy - a * y0, sx - a * x0
    ryy, rxx = syy - 2 * y0 * sy + a * y0 * y0, sxx - 2 * x0 * sx + a * x0 * x0
    rxy = sxy - y0 * sx - x0 * sy + a * x0 * y0
    myy, mxx, mxy = _exact_variance(on, a, ryy, ry, ry), _exact_variance(on, a, rxx, rx, rx), _exact_variance(on, a, rxy, ry, rx)
    with np.errstate(invalid="ignore", divide="ignore"):
        af = a.astype(np.float64) + nan
        centroid = np.stack([y0 + ry / af, x0 + rx / af], axis=-1)
        half, diff = (mxx + myy) / 2, (mxx - myy) / 2
        root = np.hypot(diff, mxy)
        l1, l2 = half + root, np.maximum(half - root, 0.0)
        ecc = np.where(l1 > 0, np.sqrt(np.clip(1 - l2 / np.where(l1 > 0, l1, 1.0), 0.0, 1.0)), 0.0) + nan
        orientation = 0.5 * np.arctan2(2 * mxy, mxx - myy)
        perimeter = (s.frame + s.open + s.contact).astype(np.float64) + nan
        contact_fraction = s.contact / perimeter
        extent = af / (bh * bw).astype(np.float64)
        mean = std = lo = hi = None
        if s.v_sum is not None:
            mean = s.v_sum / af
            if s.v_sum.dtype.kind == "f":
                var = s.v_sum2 / af - mean * mean
            else:
                var = _exact_variance(on, a, s.v_sum2.astype(np.int64), s.v_sum.astype(np.int64), s.v_sum.astype(np.int64))
            std = np.sqrt(np.maximum(var, 0.0))
            lo, hi = s.v_min.astype(np.float64) + nan, s.v_max.astype(np.float64) + nan
    return CellProps(area=af, centroid=centroid, bbox=s.bbox, moments_central=np.stack([myy, mxx, mxy], axis=-1),
                     axis_major=4 * np.sqrt(l1), axis_minor=4 * np.sqrt(l2), eccentricity=ecc, orientation=orientation,
                     equivalent_diameter=np.sqrt(4 * af / np.pi), extent=extent, perimeter=perimeter, contact_fraction=contact_fraction,
                     touches_frame=(s.frame > 0) & on, mean=mean, std=std, min=lo, max=hi)


def cell_props(labels, image=None):
    """props_from_sums(cell_sums(labels, image)): the per-cell properties of an instance map (and of an image under it)."""
    return props_from_sums(cell_sums(labels, image))


def select_cells(labels, keep, *, renumber=False):
    """Drop or renumber cells by any per-id decision (unet_remap_labels), e.g.
    select_cells(lab, torch.from_numpy(props.eccentricity < 0.95).cuda()), which generalises remove_small to every measured
    property.  labels: int32 / int64 ids [H,W] or [B,H,W] on a HIP device, as cell_sums takes them; keep: a bool tensor
    [n_max+1] (one decision for the batch) or [B, n_max+1] (one per image) on the same device.  Returns an int32 map of the
    labels' shape: a pixel keeps its id if keep[id] is true, else becomes 0; keep[0] is ignored (background stays 0).
    renumber=True maps the kept ids to 1..k in increasing order of the old id (per image with a per-image keep).  A pixel whose
    id is outside [0, n_max] raises ValueError (the status word is read back once); host tensors raise NotImplementedError."""
    (lab,) = _id_maps("select_cells", "unet_remap_labels", labels)
    if not torch.is_tensor(keep) or keep.dtype != torch.bool or keep.dim() not in (1, 2) or keep.shape[-1] < 1:
        raise ValueError("select_cells: keep must be a bool tensor [n_max+1] or [B, n_max+1]")
    _device_only("select_cells", "unet_remap_labels", keep)
    import _hip
    B, H, W = lab.shape
    if keep.dim() == 2 and keep.shape[0] != B:
        raise ValueError("select_cells: keep holds %d images, the labels %d" % (keep.shape[0], B))
    _measure_sizes("select_cells", B, H, W)
    n_max = keep.shape[-1] - 1
    if n_max >= 1 << 24:
        raise ValueError("select_cells: ids must be below 2^24, keep has %d entries" % (n_max + 1))
    k = keep.clone()
    k[..., 0] = False
    ids = torch.cumsum(k, dim=-1, dtype=torch.int32) if renumber else torch.arange(n_max + 1, dtype=torch.int32, device=lab.device)
    table = torch.where(k, ids, torch.zeros((), dtype=torch.int32, device=lab.device)).contiguous()
    out = torch.empty(B, H, W, dtype=torch.int32, device=lab.device)
    status = torch.empty(B, dtype=torch.int64, device=lab.device)
    _hip.run("unet_remap_labels", lab.device, _hip.ptr(lab), _id_code(lab), B, H, W, _hip.ptr(table), n_max, n_max + 1 if keep.dim() == 2 else 0,
             _hip.ptr(out), _hip.ptr(status))
    (bad,) = _status_words(status)
    if bad:
        raise ValueError("select_cells: %d pixels hold ids outside [0, %d]" % (bad, n_max))
    return _unbatch(labels, out)


# ---- convex hulls and neighbours of the cells ---------------------------------------------------------------------------

CellHulls = collections.namedtuple("CellHulls", "n_vertices area2 feret_max2 width_cross width_len2 offset vertices")
HullProps = collections.namedtuple("HullProps", "convex_area solidity feret_max feret_min convex_perimeter n_vertices")
Neighbours = collections.namedtuple("Neighbours", "b i j sides")


def cell_hulls(labels, sums=None, *, n_max=None):
    """The convex hull of every cell of an instance map and the exact integers measured on it, on the device (unet_cell_hulls):
    labels as cell_sums takes them.  A pixel (y, x) is the closed unit square [x, x+1] x [y, y+1] in corner coordinates; the hull
    of id i >= 1 is the convex hull of the union of its pixels' squares.  Ids need not be connected; id 0 is skipped and its row
    is 0, as is the row of every absent id.  sums: the CellSums of cell_sums(labels, ..., n_max=n_max) (its boxes are used), or
    None to form it here.  Returns CellHulls of device tensors [B, n_max+1] ([n_max+1] for a single image) unless stated:
      n_vertices   int32, the vertices of the hull, collinear points dropped
      area2        int64, twice the hull's area
      feret_max2   int64, the largest squared distance between two vertices
      width_cross, width_len2   int64 (c, l2) of the hull edge with the smallest width c / sqrt(l2): c = the largest |cross| of a
                   vertex against the edge, l2 = the edge's squared length; the smaller l2 among edges of equal width
      offset       int64 [B (n_max+1) + 1] ([n_max+2]): row r owns vertices[2 offset[r] : 2 offset[r+1]]
      vertices     int32 [2 L, 2], (x, y): the row's n_vertices vertices, down the left side from the top and up the right side
                   from the bottom, then zeros
    The offsets are a cumulative sum on the device and their total L is read back once to size the tables; the status words are
    read at the end.  Pixels with an id outside [0, n_max] and boxes that do not hold their id's pixels raise ValueError; host
    tensors raise NotImplementedError (no CPU path).  hull_props turns the table into areas, solidity and Feret diameters."""
    (lab,) = _id_maps("cell_hulls", "unet_cell_hulls", labels)
    import _hip
    B, H, W = lab.shape
    _measure_sizes("cell_hulls", B, H, W)
    if sums is None:
        sums = cell_sums(labels, n_max=n_max)
    bbox, present = sums.bbox, sums.present
    if not (torch.is_tensor(bbox) and torch.is_tensor(present)) or bbox.dtype != torch.int32 or bbox.dim() != labels.dim() \
            or bbox.shape[-1] != 4 or present.shape != bbox.shape[:-1] or (labels.dim() == 3 and bbox.shape[0] != B):
        raise ValueError("cell_hulls: sums must be the CellSums of cell_sums(labels) (bbox int32 [.., n_max+1, 4])")
    _device_only("cell_hulls", "unet_cell_hulls", bbox, present)
    N = bbox.shape[-2]
    if n_max is not None:
        _int_in(n_max, N - 1, N, "cell_hulls: n_max = %%r does not match the %d rows of sums" % N)
    n_max, dev = N - 1, lab.device
    bbox, present = bbox.reshape(B, N, 4).contiguous(), present.reshape(B, N).bool()
    levels = torch.where(present, (bbox[..., 2] - bbox[..., 0] + 1).long(), torch.zeros((), dtype=torch.int64, device=dev))
    levels[:, 0] = 0
    offset = torch.zeros(B * N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(levels.flatten(), dim=0, out=offset[1:])
    L = int(offset[-1])
    n_vertices = torch.empty(B, N, dtype=torch.int32, device=dev)
    area2 = torch.empty(B, N, dtype=torch.int64, device=dev)
    feret_max2 = torch.empty(B, N, dtype=torch.int64, device=dev)
    width = torch.empty(B, N, 2, dtype=torch.int64, device=dev)
    vertices = torch.empty(2 * L, 2, dtype=torch.int32, device=dev)
    status = torch.empty(B, 2, dtype=torch.int64, device=dev)
    scratch = _hip.scratch("unet_cell_hulls", dev, L)
    _hip.run("unet_cell_hulls", dev, _hip.ptr(lab), _id_code(lab), B, H, W, n_max, _hip.ptr(bbox), _hip.ptr(offset), L, _hip.ptr(n_vertices),
             _hip.ptr(area2), _hip.ptr(feret_max2), _hip.ptr(width), _hip.ptr(vertices) if L else None, _hip.ptr(status),
             _hip.ptr(scratch) if L else None)
    bad_id, outside = _status_words(status)
    if bad_id:
        raise ValueError("cell_hulls: %d pixels hold ids outside [0, %d]" % (bad_id, n_max))
    if outside:
        raise ValueError("cell_hulls: %d pixels lie outside the box that sums gives for their id" % outside)
    out = [n_vertices, area2, feret_max2, width[..., 0], width[..., 1]]
    return CellHulls(*_unbatch(labels, *out), offset, vertices)


def hull_props(hulls, sums):
    """The hull-based shape properties of every id from the tables of cell_hulls and cell_sums (device tensors, host tensors or
    arrays): pure numpy on the host.  Returns HullProps of float64 arrays of the tables' leading shape, nan wherever an id is
    absent (row 0 included):
      convex_area       area2 / 2
      solidity          area / convex area = 2 area / area2, at most 1 and exactly 1 for a rectangle; a cell with a concavity
                        (two touching discs under one id) falls well below a convex one
      feret_max         sqrt(feret_max2), the largest calliper width
      feret_min         c / sqrt(l2), the smallest calliper width
      convex_perimeter  the sum of the vertex-to-vertex lengths around the hull
      n_vertices        int32 as in the table (0 for an absent id)"""
    h = CellHulls(*(_host(t) for t in hulls))
    k = h.n_vertices.astype(np.int64)
    on = k > 0
    nan = np.where(on, 0.0, np.nan)
    area = _host(sums.area).astype(np.float64)
    if area.shape != k.shape:
        raise ValueError("hull_props: hulls %s and sums %s do not belong together" % (k.shape, area.shape))
    with np.errstate(invalid="ignore", divide="ignore"):
        a2 = h.area2.astype(np.float64) + nan
        feret_min = h.width_cross.astype(np.float64) / np.sqrt(h.width_len2.astype(np.float64)) + nan
    kf = k.ravel()
    row = np.repeat(np.arange(kf.size), kf)                             # one entry per vertex: its row, its place in the row
    pos = np.arange(row.size) - np.repeat(np.cumsum(kf) - kf, kf)
    start = 2 * h.offset.astype(np.int64)[row]
    v = h.vertices.astype(np.float64)
    p, q = v[start + pos], v[start + (pos + 1) % np.maximum(kf[row], 1)]
    perimeter = np.bincount(row, weights=np.hypot(q[:, 0] - p[:, 0], q[:, 1] - p[:, 1]), minlength=kf.size).reshape(k.shape) + nan
    return HullProps(convex_area=a2 / 2, solidity=2 * area / a2, feret_max=np.sqrt(h.feret_max2.astype(np.float64)) + nan,
                     feret_min=feret_min, convex_perimeter=perimeter, n_vertices=h.n_vertices)


def cell_neighbours(labels, *, _table_slots=None):
    """Who touches whom in an instance map, and along how much border (unet_cell_contacts): labels as cell_sums takes them.
    Returns Neighbours(b, i, j, sides) of int64 numpy arrays sorted by (b, i, j): one entry per image b and unordered pair of ids
    1 <= i < j with at least one unit pixel side at which a pixel of i is 4-adjacent to a pixel of j, and the number of such sides.
    Summed over the pairs that hold an id they give CellSums.contact of that id.  The counting is exact and on the device; the
    protocol is pair_table's: the largest id is read back once, and the table is doubled and the call repeated while it reports
    an overflow.  Negative ids and ids >= 2^24 raise ValueError; host tensors raise NotImplementedError (no CPU path)."""
    (lab,) = _id_maps("cell_neighbours", "unet_cell_contacts", labels)
    import _hip
    B, H, W = lab.shape
    _measure_sizes("cell_neighbours", B, H, W)
    (n_max,) = _id_range("cell_neighbours", lab)
    dev = lab.device
    n_pairs = torch.empty(1, dtype=torch.int64, device=dev)
    (keys, counts, _), _ = _table_call(
        "unet_cell_contacts", dev, B, (_hip.ptr(lab), _id_code(lab), B, H, W, n_max), _table_slots, 8 * n_max, lambda slots: (B, slots),
        lambda slots: (torch.empty(slots, dtype=torch.int64, device=dev), torch.empty(slots, dtype=torch.int32, device=dev), n_pairs),
        "cell_neighbours: %d pixels hold ids outside [0, %d]", (n_max,))
    return Neighbours(*_sorted_pairs(keys, counts, n_pairs))


def neighbour_counts(neigh, B, n_max):
    """int64 [B, n_max+1]: the number of distinct neighbours of every cell, from the list of cell_neighbours."""
    out = np.zeros((int(B), int(n_max) + 1), np.int64)
    b = np.asarray(neigh.b, np.int64)
    np.add.at(out, (b, np.asarray(neigh.i, np.int64)), 1)
    np.add.at(out, (b, np.asarray(neigh.j, np.int64)), 1)
    return out


SegMeasure = collections.namedtuple("SegMeasure", "seg jaccard_sum n_gt n_matched n_pred per_image jaccard")


def seg_from_counts(area_gt, area_pred, match, inter):
    """SegMeasure from the integers of unet_instance_overlap, all [B][ids + 1] (host arrays): for every ground-truth id g >= 1
    with area_gt > 0, J = inter / (area_gt + area_pred[match] - inter) in float64 if a predicted cell matched (it covers more
    than half of g), else 0; seg = the mean of J over those cells of the whole batch, nan when there are none."""
    area_gt, area_pred, match, inter = (np.asarray(a).astype(np.int64) for a in (area_gt, area_pred, match, inter))
    jaccard, per_image = [], np.full(len(area_gt), np.nan)
    for b in range(len(area_gt)):
        g = np.nonzero(area_gt[b, 1:])[0] + 1
        m = match[b, g]
        j = np.where(m > 0, inter[b, g] / (area_gt[b, g] + area_pred[b, m] - inter[b, g]), 0.0)
        jaccard.append(j)
        if len(j):
            per_image[b] = j.mean()
    every = np.concatenate(jaccard)
    n_gt = len(every)
    return SegMeasure(seg=every.mean() if n_gt else np.float64(np.nan), jaccard_sum=float(every.sum()), n_gt=n_gt,
                      n_matched=int((match[:, 1:] > 0).sum()), n_pred=int((area_pred[:, 1:] > 0).sum()), per_image=per_image,
                      jaccard=jaccard)


def seg_measure(pred_labels, gt_labels, *, _table_slots=None):
    """The Cell Tracking Challenge SEG measure (the score of Ronneberger et al. 2015, Table 2, which the goals of
    trainer.py:20-26 quote) of predicted against ground-truth instance maps: int32 / int64 id maps of equal shape [H,W] or
    [B,H,W] on a HIP device, 0 = background, e.g. label_cells(mask)[0] against the dataset's man_seg image.  A ground-truth
    cell R is matched by the predicted cell S with |R n S| > |R| / 2 and scores J = |R n S| / |R u S|, or 0 without one.
    Returns SegMeasure(seg, jaccard_sum, n_gt, n_matched, n_pred, per_image, jaccard): seg = float64 mean of J over the
    ground-truth cells present in the batch (nan when none); jaccard_sum, n_gt, n_matched, n_pred Python numbers to pool over
    a dataset; per_image float64 [B]; jaccard a list of B float64 arrays, one J per present ground-truth id in increasing id
    order.  The counting is exact and on the device (unet_instance_overlap); the two id maxima are read back once to size the
    tables, and the pair table is doubled and the call repeated while it reports an overflow.  Negative ids raise ValueError;
    host tensors raise NotImplementedError (no CPU path)."""
    pred, gt = _id_maps("seg_measure", "unet_instance_overlap", pred_labels, gt_labels)
    ng_max, np_max = _id_range("seg_measure", gt, pred)
    B, dev = gt.shape[0], gt.device
    area_gt = torch.empty(B, ng_max + 1, dtype=torch.int32, device=dev)         # the library's u32 / u64 words: counts of at
    area_pred = torch.empty(B, np_max + 1, dtype=torch.int32, device=dev)       # most H * W < 2^31, so the signed views agree
    match = torch.empty(B, ng_max + 1, dtype=torch.int32, device=dev)
    inter = torch.empty(B, ng_max + 1, dtype=torch.int32, device=dev)
    _overlap_call("unet_instance_overlap", gt.int(), pred.int(), ng_max, np_max, _table_slots, lambda slots: (B, ng_max, np_max, slots),
                  lambda slots: (area_gt, area_pred, match, inter), "seg_measure: %d pixels hold ids outside [0, %d] / [0, %d]")
    return seg_from_counts(area_gt.cpu().numpy(), area_pred.cpu().numpy(), match.cpu().numpy(), inter.cpu().numpy())


def grow_cells(labels, max_distance=None):
    """Nearest-cell growth of an instance map (border thinning; skimage.segmentation.expand_labels with an exact metric and a
    stated tie rule): int32 / int64 ids [H,W] or [B,H,W] on a HIP device, 0 = background, ids in [1, 2^24), not necessarily
    consecutive or connected.  Returns an int32 map of the same shape: a pixel with id != 0 keeps it; a background pixel takes
    the id of the labelled pixel at the smallest exact squared Euclidean distance d^2, the smallest id among those at that d^2.
    max_distance (a float >= 0): only labelled pixels with d^2 <= floor(max_distance^2) count, and a pixel with none in reach
    stays 0; 0 is the identity.  None: unlimited; an image without labels stays all 0.  data.preprocess_gt carves borders of
    4 px reach between touching cells, so label_cells(mask) loses every cell's rim against the man_seg ids: grow_cells(., 4)
    hands it back before seg_measure.  Exact, on the device (unet_grow_labels), at a cost independent of the number of cells.
    Negative ids and ids >= 2^24 raise ValueError; host tensors raise NotImplementedError (no CPU path)."""
    (lab,) = _id_maps("grow_cells", "unet_grow_labels", labels)
    import _hip
    max_dist2 = _limit("grow_cells", "max_distance", max_distance, square=True)
    _id_range("grow_cells", lab)
    lab = lab.int()
    B, H, W = lab.shape
    out = torch.empty_like(lab)
    scratch = _hip.scratch("unet_grow_labels", lab.device, B, H, W)
    _hip.run("unet_grow_labels", lab.device, _hip.ptr(lab), B, H, W, max_dist2, _hip.ptr(out), _hip.ptr(scratch))
    return _unbatch(labels, out)


def pair_table(pred_labels, gt_labels, *, _table_slots=None):
    """The contingency table of predicted against ground-truth instance maps (as seg_measure takes them) restricted to
    ground-truth foreground: int64 numpy arrays (b, g, p, n), one entry per distinct (image, gt id >= 1, pred id >= 0) with
    n > 0 pixels, sorted by (b, g, p).  p = 0 is "predicted background"; pixels with gt = 0 are in no entry.  The counting is
    exact and on the device (unet_partition_pairs); the protocol is seg_measure's: the two id maxima are read back once, and
    the table is doubled and the call repeated while it reports an overflow.  Negative ids (the kernel counts them in its
    status words) and ids >= 2^24 raise ValueError;
    host tensors raise NotImplementedError (no CPU path)."""
    pred, gt = _id_maps("pair_table", "unet_partition_pairs", pred_labels, gt_labels)
    B, dev = gt.shape[0], gt.device
    ng_max, np_max = (max(0, int(v)) for v in torch.stack([gt.max().long(), pred.max().long()]).tolist())
    if max(ng_max, np_max) >= 1 << 24:
        raise ValueError("pair_table: ids must be below 2^24, got up to %d" % max(ng_max, np_max))
    n_pairs = torch.empty(1, dtype=torch.int64, device=dev)
    keys, counts, _ = _overlap_call(
        "unet_partition_pairs", gt.int(), pred.int(), ng_max, np_max, _table_slots, lambda slots: (B, slots),
        lambda slots: (torch.empty(slots, dtype=torch.int64, device=dev), torch.empty(slots, dtype=torch.int32, device=dev), n_pairs),
        "pair_table: %d pixels hold negative ids (outside [0, %d] / [0, %d])")
    return _sorted_pairs(keys, counts, n_pairs)


# ---- linking cells across frames ----------------------------------------------------------------------------------------

MAX_FRAMES = 65535                                                      # T of unet_link_frames: the frame index is the key's top 16 bits
FrameLinks = collections.namedtuple("FrameLinks", "area pred pred_overlap")


def _link_frames(name, labels, reach, slots):
    """The checks and the device half of link_frames: (int32 labels [T,H,W], n_max, FrameLinks)."""
    if torch.is_tensor(labels) and labels.dim() != 3:
        raise ValueError("%s takes a time-lapse of id maps [T,H,W], got %s" % (name, tuple(labels.shape)))
    if torch.is_tensor(labels) and labels.shape[0] > MAX_FRAMES:
        raise ValueError("%s: at most %d frames, got %d" % (name, MAX_FRAMES, labels.shape[0]))
    if reach is not None:
        _real_in(reach, 0, math.inf, name + ": reach must be None or a number >= 0, got %r")
    (lab,) = _id_maps(name, "unet_link_frames", labels)
    (n_max,) = _id_range(name, lab)
    import _hip
    lab = lab.int()
    src = lab if reach is None else grow_cells(lab, reach)              # grown ids are ids of the frame: still in [0, n_max]
    T, H, W = lab.shape
    dev = lab.device
    out = torch.empty(3, T, n_max + 1, dtype=torch.int32, device=dev)   # the library's u32 words: counts of at most H * W < 2^31
    _table_call("unet_link_frames", dev, T, (_hip.ptr(src), _hip.ptr(lab), T, H, W, n_max), slots, min(4 * (T - 1) * n_max, T * H * W),
                lambda slots: (T, n_max, slots), lambda slots: tuple(out), name + ": %d pixels hold ids outside [0, %d]", (n_max,))
    return lab, n_max, FrameLinks(*out.cpu().numpy().astype(np.int64))


def link_frames(labels, *, reach=None, _table_slots=None):
    """The overlap links between the consecutive frames of a time-lapse of instance maps, e.g. the instance map of
    tester.segment(unet, frames, return_instances=True): labels int32 / int64 ids [T,H,W] on a HIP device, 0 = background, ids
    in [1, 2^24) that mean nothing across frames, not necessarily consecutive or connected.  Returns FrameLinks(area, pred,
    pred_overlap), int64 numpy arrays [T][n_max+1]: area[t][c] the pixels of id c in frame t (index 0 = background); pred[t][c],
    for t >= 1 and c >= 1, the id p >= 1 of frame t-1 with the largest |p n c| > 0, the smallest such p on equal overlaps, 0 when
    no cell of frame t-1 touches c; pred_overlap[t][c] that |p n c|, else 0; row 0 and column 0 are 0.
    reach=r (a float >= 0): frame t is set against grow_cells(labels, r)[t-1], so a cell that moved up to r px beyond its old
    outline still finds its predecessor; the areas are those of labels; reach=0 is reach=None.  Exact and on the device
    (unet_link_frames), the same in every run; the protocol is seg_measure's: the id maximum is read back once, and the pair
    table is doubled and the call repeated while it reports an overflow.  Negative ids, ids >= 2^24, an input that is not
    [T,H,W] and T > 65535 raise ValueError; host tensors raise NotImplementedError (no CPU path).
    tracks_from_links makes tracks of the links; track_cells does both and relabels the maps."""
    return _link_frames("link_frames", labels, reach, _table_slots)[2]


class Tracks(collections.namedtuple("Tracks", "table track_of")):
    """table: int64 [n,4], one row L B E P per track as in the Cell Tracking Challenge's res_track.txt: label (1..n), first and
    last frame (counted from 0), label of the parent track or 0.  track_of: int32 [T][n_max+1], track label of id c of frame t,
    0 for absent ids."""
    __slots__ = ()

    def ctc_text(self):
        """The text of res_track.txt: one line `L B E P` per track."""
        return "".join("%d %d %d %d\n" % tuple(int(v) for v in row) for row in self.table)


def _track_rules(name, min_overlap, divisions, max_children):
    _real_in(min_overlap, 0, 1, name + ": min_overlap must be a number in [0, 1], got %r")
    _int_in(max_children, 1, math.inf, name + ": max_children must be an int >= 1, got %r")
    if divisions not in (False, True):
        raise ValueError("%s: divisions must be False or True, got %r" % (name, divisions))


def tracks_from_links(links, *, min_overlap=0.0, divisions=True, max_children=2):
    """Tracks from the FrameLinks of link_frames (or any three integer arrays [T][n_max+1] of that meaning), on the host: the
    greedy overlap tracker of the U-Net submissions to the Cell Tracking Challenge.  Frames in order, ids in increasing order.
    The link c -> p = pred[t][c] is accepted iff p > 0 and pred_overlap[t][c] >= min_overlap * area[t][c] (float64).  A cell p
    of frame t-1 with one accepted claimant is continued by it.  With several, ranked by overlap descending, then id ascending:
    divisions=True: the first max_children each start a track whose parent is p's track, the rest start tracks with parent 0, and
    p's track ends at t-1; divisions=False: the first continues p's track and the rest start tracks with parent 0.  A cell
    nobody claims ends its track; a cell without an accepted link starts a track with parent 0.  Track labels are 1, 2, ... in
    order of (first frame, cell id).  Returns Tracks(table, track_of)."""
    _track_rules("tracks_from_links", min_overlap, divisions, max_children)
    area, pred, over = (np.asarray(a).astype(np.int64) for a in links)
    if area.ndim != 2 or area.shape[1] < 1 or pred.shape != area.shape or over.shape != area.shape:
        raise ValueError("tracks_from_links: area, pred and pred_overlap must be three arrays [T][n_max+1] of one shape, got %s"
                         % ", ".join(str(a.shape) for a in (area, pred, over)))
    T, N = area.shape
    track_of = np.zeros((T, N), np.int32)
    table = []
    for t in range(T):
        cells = (np.nonzero(area[t, 1:])[0] + 1).tolist()
        claimants = {}
        for c in cells if t else ():
            p = int(pred[t, c])
            if p > 0 and float(over[t, c]) >= min_overlap * float(area[t, c]):
                if p >= N or not track_of[t - 1, p]:
                    raise ValueError("tracks_from_links: pred[%d][%d] = %d is no cell of frame %d" % (t, c, p, t - 1))
                claimants.setdefault(p, []).append(c)
        fate = {}                                                       # c -> (track it continues or 0, parent of the track it starts)
        for p, cs in claimants.items():
            mother = int(track_of[t - 1, p])
            cs.sort(key=lambda c: (-over[t, c], c))
            if len(cs) == 1 or not divisions:
                fate[cs[0]] = (mother, 0)
            else:
                fate.update((c, (0, mother)) for c in cs[:max_children])
        for c in cells:
            goes_on, parent = fate.get(c, (0, 0))
            if goes_on:
                table[goes_on - 1][2] = t
            else:
                table.append([len(table) + 1, t, t, parent])
                goes_on = len(table)
            track_of[t, c] = goes_on
    return Tracks(np.array(table, np.int64).reshape(-1, 4), track_of)


def track_cells(labels, *, reach=None, min_overlap=0.0, divisions=True, max_children=2, _table_slots=None):
    """A time-lapse of instance maps relabelled so that the same cell keeps the same id: link_frames(labels, reach=reach), then
    tracks_from_links(links, min_overlap=.., divisions=.., max_children=..), then every pixel's id replaced by its track label on
    the device (unet_remap_labels with one map per frame); only the [T][n_max+1] rows cross to the host and back.  labels as
    link_frames takes them, H, W <= 32768.  Returns (track_maps, tracks): track_maps int32 [T,H,W] on the labels' device, 0 where
    labels is 0; tracks the Tracks, whose ctc_text() is the challenge's res_track.txt for these maps."""
    if torch.is_tensor(labels) and labels.dim() == 3:
        _measure_sizes("track_cells", *labels.shape)
    _track_rules("track_cells", min_overlap, divisions, max_children)
    lab, n_max, links = _link_frames("track_cells", labels, reach, _table_slots)
    tracks = tracks_from_links(links, min_overlap=min_overlap, divisions=divisions, max_children=max_children)
    import _hip
    T, H, W = lab.shape
    table = torch.from_numpy(tracks.track_of).to(lab.device)
    out = torch.empty(T, H, W, dtype=torch.int32, device=lab.device)
    status = torch.empty(T, dtype=torch.int64, device=lab.device)
    _hip.run("unet_remap_labels", lab.device, _hip.ptr(lab), 2, T, H, W, _hip.ptr(table), n_max, n_max + 1, _hip.ptr(out), _hip.ptr(status))
    return out, tracks


RandScores = collections.namedtuple("RandScores", "rand_split rand_merge v_rand rand_error info_split info_merge v_info voi_split "
                                                  "voi_merge rand_error_mean v_info_mean N S_pair S_pred S_gt c")


def _quot(num, den):
    """num / den of two exact rationals as the nearest float64; nan for 0 / 0 (and for any x / 0: no score here has one)."""
    return float(fractions.Fraction(num) / den) if den else math.nan


def _ratio(num, den):
    return num / den if den else math.nan


def rand_from_pairs(b, g, p, n, B, alpha=0.5):
    """RandScores from a pair table (b, g, p, n) of B images, as pair_table returns it (any order; host arrays, no GPU).  Per
    image, with n_gp the counts, a_g = sum_p n_gp (p = 0 included), b_p = sum_g n_gp for p >= 1, c = sum_g n_g0, N = sum a_g;
    the c predicted-background pixels inside ground-truth foreground are singleton segments:
        S_pair = sum_{p>=1} n_gp^2 + c      S_pred = sum_{p>=1} b_p^2 + c      S_gt = sum a_g^2
        rand_split = S_pair / S_gt    rand_merge = S_pair / S_pred    v_rand = S_pair / (alpha S_pred + (1 - alpha) S_gt)
        rand_error = 1 - v_rand       (alpha = 1/2: the adapted Rand error of the ISBI 2012 / SNEMI3D evaluation)
    each one quotient of exact integers (alpha enters as the rational its float is), rounded once: equal integers give equal
    floats everywhere.  With natural logarithms and every sum formed by math.fsum (no dependence on order),
        N H_pred = N ln N - sum_{p>=1} b ln b     N H_gt = N ln N - sum a ln a     N H_joint = N ln N - sum_{p>=1} n ln n
        I = H_pred + H_gt - H_joint    info_split = I / H_pred    info_merge = I / H_gt
        v_info = I / ((1 - alpha) H_pred + alpha H_gt)    voi_split = H_joint - H_gt = H(pred | gt)    voi_merge = H_joint - H_pred
    (singletons add 0 to every sum of x ln x).  0 / 0 is nan: an image with N = 0 has nan for every score, a prediction that is
    one segment has H_pred = 0 and info_split = nan.  rand_error_mean and v_info_mean are the means over the images where the
    score is not nan (nan if there is none); N, S_pair, S_pred, S_gt, c are int64 [B], to pool over a data set."""
    b, g, p, n = (np.asarray(a).astype(np.int64).ravel() for a in (b, g, p, n))
    alpha_q = fractions.Fraction(float(alpha))
    names = RandScores._fields[:9]
    out = {k: np.full(B, np.nan) for k in names}
    ints = {k: np.zeros(B, np.int64) for k in ("N", "S_pair", "S_pred", "S_gt", "c")}
    xlnx = lambda v: [x * math.log(x) for x in v]
    for i in range(B):
        sel = b == i
        gi, pi, ni = g[sel], p[sel], n[sel]
        fg = pi >= 1
        a = [int(v) for v in _group_sums(gi, ni)]
        bp = [int(v) for v in _group_sums(pi[fg], ni[fg])]
        nn = [int(v) for v in ni[fg]]
        c = int(ni[~fg].sum())
        N = sum(a)
        S_pair, S_pred, S_gt = sum(v * v for v in nn) + c, sum(v * v for v in bp) + c, sum(v * v for v in a)
        for k, v in zip(("N", "S_pair", "S_pred", "S_gt", "c"), (N, S_pair, S_pred, S_gt, c)):
            ints[k][i] = v
        if N == 0:
            continue
        den = alpha_q * S_pred + (1 - alpha_q) * S_gt
        out["rand_split"][i], out["rand_merge"][i] = _quot(S_pair, S_gt), _quot(S_pair, S_pred)
        out["v_rand"][i] = _quot(S_pair, den)
        out["rand_error"][i] = _quot(den - S_pair, den)
        T = N * math.log(N)
        X_pair, X_pred, X_gt = xlnx(nn), xlnx(bp), xlnx(a)
        neg = lambda v: [-x for x in v]
        H_pred, H_gt = math.fsum([T] + neg(X_pred)) / N, math.fsum([T] + neg(X_gt)) / N
        I = math.fsum([T] + neg(X_pred) + neg(X_gt) + X_pair) / N
        out["info_split"][i], out["info_merge"][i] = _ratio(I, H_pred), _ratio(I, H_gt)
        out["v_info"][i] = _ratio(I, (1 - alpha) * H_pred + alpha * H_gt)
        out["voi_split"][i] = math.fsum(X_gt + neg(X_pair)) / N
        out["voi_merge"][i] = math.fsum(X_pred + neg(X_pair)) / N
    mean = lambda v: np.float64(v[~np.isnan(v)].mean()) if (~np.isnan(v)).any() else np.float64(np.nan)
    return RandScores(rand_error_mean=mean(out["rand_error"]), v_info_mean=mean(out["v_info"]), **out, **ints)


def _group_sums(ids, weights):
    """Sums of the int64 weights per distinct id (exact: integer adds)."""
    if len(ids) == 0:
        return np.zeros(0, np.int64)
    u, inv = np.unique(ids, return_inverse=True)
    s = np.zeros(len(u), np.int64)
    np.add.at(s, inv, weights)
    return s


def rand_scores(pred_labels, gt_labels, *, grow=None, alpha=0.5):
    """The foreground-restricted Rand and information scores of predicted against ground-truth instance maps (as seg_measure
    takes them): the ranking scores of the ISBI 2012 challenge, Ronneberger et al. 2015, Table 1.  grow = True or a number:
    pred_labels first goes through grow_cells(pred_labels, None if grow is True else grow), the challenge's border thinning (a
    prediction is scored after its border pixels have gone to the neighbouring segments).  Returns the RandScores of
    rand_from_pairs (see there for every definition) on pair_table(pred, gt).
    This is not the warping error (that is warping_error); it is not bit-equal to the Fiji script of the challenge, whose thinning leaves borders one
    pixel wide where grow=True leaves none; and label_cells stays 4-connected.  Errors as pair_table and grow_cells."""
    pred, gt = _id_maps("rand_scores", "unet_partition_pairs", pred_labels, gt_labels)
    if grow is not None and grow is not False:
        pred = grow_cells(pred, None if grow is True else grow)
    b, g, p, n = pair_table(pred, gt)
    return rand_from_pairs(b, g, p, n, gt.shape[0], alpha)


WarpCounts = collections.namedtuple("WarpCounts", "mismatch mismatch_before flips sweeps mismatch_map")
WarpScores = collections.namedtuple("WarpScores", "warping_error mismatch mismatch_before flips sweeps error_regions warping_error_mean")


def warp_labels(gt_mask, pred_mask, *, reach=None, mask=None, connectivity=4, _passes=16, _launches=8):
    """The topology-preserving warp of a ground-truth mask towards a predicted one (Jain et al. 2010): masks of equal shape
    [H,W] or [B,H,W] on a HIP device, foreground = value != 0, of any dtype _int_code takes.  L starts as gt_mask; a pixel with
    L != pred that may flip and is simple in L (flipping it changes neither the 4-connected foreground components nor the
    8-connected background components of L) takes the prediction's value.  Pass s = 0..3 flips every such pixel with
    (y & 1) * 2 + (x & 1) == s at once, a sweep is the four passes in that order, and sweeps repeat until one flips nothing.
    The first and last row and column never flip.  reach (a number >= 0): only pixels whose exact squared distance to the nearest
    pixel of the other class of gt_mask is <= floor(reach^2) may flip (none in a one-class image); mask: only pixels where it is
    != 0 may (ANDed with the reach).  connectivity=8: foreground 8-connected, background 4-connected, by definition the same
    warp of the two complements.  Returns (warped, WarpCounts): warped int32 {0,1} of the input's shape, and mismatch,
    mismatch_before, flips (int64 numpy [B]: |warped != pred|, |gt != pred|, pixels flipped), sweeps (the sweeps of the image
    that needed most, the final empty one counted) and mismatch_map (float32 on the device, 1 where warped != pred).
    Exact, on the device (unet_warp_init / unet_warp_sweeps / unet_warp_finish): _launches launches of _passes passes are
    enqueued, their flip counts read back in one copy, and the loop ends at the first launch that flipped nothing; neither
    changes any result.  Unequal shapes, a bad connectivity and reach < 0 raise ValueError; host tensors raise
    NotImplementedError (no CPU path)."""
    tensors = [gt_mask, pred_mask] + ([] if mask is None else [mask])
    _all_tensors("warp_labels", "unet_warp_init", tensors)
    _same_shape("warp_labels", "masks of equal shape", tensors, ranked=False)
    _check_connectivity("warp_labels", connectivity)
    max_dist2 = _limit("warp_labels", "reach", reach, square=True)
    coded = [_int_code(t, uint8_ok=True) for t in _device_planes("warp_labels", "unet_warp_init", tensors)]
    import _hip
    (gt, gt_code), (pred, pred_code) = coded[:2]
    user, user_code = coded[2] if mask is not None else (None, 0)
    B, H, W = gt.shape
    dev = gt.device
    state = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, B, dtype=torch.int32, device=dev)          # the library's u32 words: at most H * W < 2^31
    scratch = _hip.scratch("unet_warp", dev, B, H, W)
    _hip.run("unet_warp_init", dev, _hip.ptr(gt), gt_code, _hip.ptr(pred), pred_code, _hip.ptr(user), user_code, B, H, W, max_dist2,
             connectivity, _hip.ptr(state), _hip.ptr(counts[0]), _hip.ptr(scratch))
    per_sweep = []                                                      # flips of every sweep so far, [B] each
    while True:
        slots = torch.empty(_launches, 4, B, dtype=torch.int32, device=dev)
        _hip.run("unet_warp_sweeps", dev, _hip.ptr(state), B, H, W, _passes, _launches, _hip.ptr(slots), 0, _hip.ptr(scratch))
        slots = slots.cpu().numpy().astype(np.int64)
        per_sweep.extend(slots[:, :_passes // 4].reshape(-1, B))
        if not slots.any(axis=(1, 2)).all():                            # a launch that flipped nothing: so did all after it
            break
    per_sweep = np.stack(per_sweep)
    warped = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    mismatch_map = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    _hip.run("unet_warp_finish", dev, _hip.ptr(state), B, H, W, connectivity, _hip.ptr(warped), _hip.ptr(mismatch_map), _hip.ptr(counts[1]))
    before, after = counts.cpu().numpy().astype(np.int64)
    warped, mismatch_map = _unbatch(gt_mask, warped, mismatch_map)
    return warped, WarpCounts(mismatch=after, mismatch_before=before, flips=per_sweep.sum(axis=0),
                              sweeps=int(np.argmin(per_sweep.any(axis=1))) + 1, mismatch_map=mismatch_map)


def warping_error(pred_mask, gt_mask, *, reach=None, mask=None, connectivity=4):
    """The warping error of predicted against ground-truth masks (the ranking score of the ISBI 2012 challenge, Ronneberger et
    al. 2015, Table 1): the disagreement that is left after warp_labels(gt_mask, pred_mask, ...) has moved the ground truth
    towards the prediction as far as its topology allows.  Returns WarpScores: warping_error float64 [B] = mismatch / (H W);
    mismatch, mismatch_before, flips int64 [B] and sweeps as WarpCounts has them; error_regions int64 [B] = the 4-connected
    components of {warped != pred} (label_cells); warping_error_mean float64.  Arguments and errors as warp_labels.
    Not bit-equal to the Fiji plug-in of the challenge, which flips in another order, restricts the flips by another mask and
    thresholds a probability map at many levels; error_regions is not its split / merge / hole classification."""
    warped, c = warp_labels(gt_mask, pred_mask, reach=reach, mask=mask, connectivity=connectivity)
    H, W = warped.shape[-2:]
    err = c.mismatch / np.float64(H * W)
    regions = label_cells(c.mismatch_map)[1].cpu().numpy().astype(np.int64)
    return WarpScores(warping_error=err, mismatch=c.mismatch, mismatch_before=c.mismatch_before, flips=c.flips, sweeps=c.sweeps,
                      error_regions=regions, warping_error_mean=np.float64(err.mean()))


def _sweep_to_idle(entry, dev, B, launches, before, after=(), behind_first=None):
    """Runs a sweep entry (unet_*_sweeps / unet_flood_assign: ..., n_launches, slots, first_slot, ...) to its first idle launch:
    `launches` launches are enqueued, their change counts [launches, B] read back in one copy, and the loop ends at the first
    launch that changed nothing (so did all after it).  Returns the launches needed, that idle one included.  behind_first()
    runs once, behind the first enqueued round: a read of status words there needs no wait of its own.  (warp_labels keeps its
    own loop: slots [launches, 4, B], per-sweep flip counts, state updated in place.)"""
    import _hip
    n = 0
    while True:
        slots = torch.empty(launches, B, dtype=torch.int32, device=dev)
        _hip.run(entry, dev, *before, launches, _hip.ptr(slots), 0, *after)
        if n == 0 and behind_first is not None:
            behind_first()
        idle = ~slots.cpu().numpy().any(axis=1)
        if idle.any():
            return n + int(np.argmax(idle)) + 1
        n += launches


def _check_connectivity(name, connectivity):
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError("%s: connectivity must be 4 or 8, got %r" % (name, connectivity))


SplitInfo = collections.namedtuple("SplitInfo", "seeds_outside unreached max_distance launches")


def split_cells(seeds, mask, *, max_steps=None, orphans='drop', return_distance=False, _launches=8, connectivity=4):
    """Seeded geodesic growth inside a mask: split touching cells by growing seeds (confident cores, e.g.
    label_cells(fg_prob >= high)[0]) back inside the mask until two growths meet.  seeds: int32 / int64 ids [H,W] or [B,H,W] on a
    HIP device, 0 = no seed, ids in [1, 2^24), not necessarily consecutive or connected; mask: the same shape, of any dtype
    _int_code takes, the region is mask != 0.  g(p) is the least number of 4-neighbour steps from a seed pixel to p along region
    pixels (0 on a seed pixel).  A region pixel with g(p) <= max_steps takes the id of the seed pixel at distance g(p), the smallest
    id among those at that distance (grow_cells' tie rule with the geodesic metric); every other pixel gets 0: pixels outside the
    region (a seed pixel there is no seed), pixels no seed reaches, pixels beyond max_steps.  max_steps None: unlimited; 0: the
    seeds restricted to the mask.  orphans='keep': what is left of the mask, the 4-connected components of
    {mask != 0 and labels == 0}, gets the ids n0[b] + 1, ... in label_cells' raster order per image, n0[b] the largest seed id of
    image b, so a cell without a seed stays a cell (label_cells and a select; the counts below are taken before it).
    Returns (labels, SplitInfo) or, with return_distance, (labels, SplitInfo, dist): labels int32 of the input's shape; dist
    int32, g(p) where the growth gave an id and -1 elsewhere; SplitInfo(seeds_outside, unreached, max_distance, launches):
    int64 numpy [B], the seed pixels outside the region, the region pixels the growth left 0 and the largest g(p) written, and
    the launches the growth needed, the final one that changed nothing included.
    Exact, on the device (unet_geodesic_init / unet_geodesic_sweeps / unet_geodesic_finish): _launches launches are enqueued,
    their change counts read back in one copy, and the loop ends at the first launch that changed nothing; _launches changes no
    result.  The growth is blind to any image and 4-connected; watershed (below) is the one that follows an intensity landscape,
    and equals this on a constant image.
    connectivity: keyword only, 4 (the default, all of the above) or 8.  With 8 a step goes to any of the eight neighbours that
    lies in the region, whatever the two pixels beside a diagonal step are, so a one-pixel-thick diagonal wall does not separate.
    g(p) is the least number of 8-neighbour steps, max_steps counts those, the id rule is the same, and orphans='keep' labels
    the rest with label_cells(..., connectivity=8) (unet_geodesic_sweeps_conn).
    A connectivity other than 4 or 8 (checked first), unequal shapes, max_steps < 0, a bad orphans,
    negative ids and ids >= 2^24 raise ValueError; host tensors raise NotImplementedError (no CPU path)."""
    _check_connectivity("split_cells", connectivity)
    _all_tensors("split_cells", "unet_geodesic_init", (seeds, mask))
    _same_shape("split_cells", "seeds and a mask of equal shape [H,W] or [B,H,W]", (seeds, mask))
    _need_ids("split_cells", "seed ids", seeds)
    if orphans not in ('drop', 'keep'):
        raise ValueError("split_cells: orphans must be 'drop' or 'keep', got %r" % (orphans,))
    steps = _limit("split_cells", "max_steps", max_steps)
    if int(_launches) < 1:
        raise ValueError("split_cells: _launches must be >= 1")
    sd, mk = _device_planes("split_cells", "unet_geodesic_init", (seeds, mask))
    import _hip
    _id_range("split_cells", sd)
    sd = sd.int()
    mk, code = _int_code(mk, uint8_ok=True)
    B, H, W = sd.shape
    dev = sd.device
    counts = torch.empty(3, B, dtype=torch.int32, device=dev)          # the library's u32 words: at most H * W < 2^31
    status = torch.empty(B, dtype=torch.int64, device=dev)
    scratch = _hip.scratch("unet_geodesic", dev, B, H, W)
    _hip.run("unet_geodesic_init", dev, _hip.ptr(sd), _hip.ptr(mk), code, B, H, W, _hip.ptr(counts[0]), _hip.ptr(status), _hip.ptr(scratch))
    launches = _sweep_to_idle("unet_geodesic_sweeps_conn", dev, B, _launches, (B, H, W, steps, connectivity), (_hip.ptr(scratch),))
    labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    dist = torch.empty(B, H, W, dtype=torch.int32, device=dev) if return_distance else None
    _hip.run("unet_geodesic_finish", dev, B, H, W, steps, _hip.ptr(labels), _hip.ptr(dist), _hip.ptr(counts[1]), _hip.ptr(counts[2]),
             _hip.ptr(scratch))
    if orphans == 'keep':
        rest, _ = label_cells((mk != 0) & (labels == 0), connectivity=connectivity)
        n0 = sd.amax(dim=(1, 2)).view(B, 1, 1)
        labels = torch.where(rest > 0, rest + n0, labels)
    outside, unreached, far = counts.cpu().numpy().astype(np.int64)
    out = (_unbatch(seeds, labels), SplitInfo(seeds_outside=outside, unreached=unreached, max_distance=far, launches=launches))
    return out + (_unbatch(seeds, dist),) if return_distance else out


FloodInfo = collections.namedtuple("FloodInfo", "seeds_outside unreached max_level launches")
FLOOD_LEVELS = 1 << 16                                                 # levels of watershed are in [0, FLOOD_LEVELS)


def watershed(seeds, image, *, mask=None, levels=None, max_level=None, return_levels=False, _launches=8, connectivity=4):
    """Seeded watershed: flood an intensity landscape from markers, Vincent-Soille immersion with exact geodesic influence zones
    on plateaus.  seeds: int32 / int64 ids [H,W] or [B,H,W] on a HIP device, 0 = no seed, ids in [1, 2^24); image: the same
    shape; mask: optional, the same shape, of any dtype _int_code takes: the region is mask != 0, everything without a mask.
    Every pixel has an integer level v in [0, 65536): an integer (or bool) image is read as it is (levels must be None), a float
    image (taken as float32) needs levels in [1, 65536] and gives v = min(levels - 1, max(0, floor(x * levels))), the product in
    fp32.  A seed pixel in the region is a source with key (L, d) = (0, 0), whatever its own level: the markers are imposed as
    minima.  A 4-neighbour step onto a region pixel q turns (L, d) into (L, d + 1) if v(q) <= L and into (v(q), 1) otherwise;
    key(q) is the lexicographic minimum over all region paths from a source: L(q) the pass height at which the flood reaches q,
    d(q) the steps inside the plateau of that height from the pixels flooded before it.  Neighbour p is a parent of q when its key
    extends to exactly key(q); a source keeps its seed id and every other reached pixel takes the least id among its parents.
    Every other pixel gets 0: pixels outside the region (a seed pixel there is no seed), pixels no source reaches, pixels with
    L > max_level (None: unlimited).  So plateaus are cut at their geodesic midline, ties go to the smaller id, and on a constant
    image the result is split_cells', bit for bit.  It is not bit-equal to skimage.segmentation.watershed, whose plateau
    handling depends on the order of its queue.
    Returns (labels, FloodInfo) or, with return_levels, (labels, FloodInfo, pass_level, dist): labels int32 of the input's
    shape; pass_level and dist int32, L and d where labels != 0 and -1 elsewhere; FloodInfo(seeds_outside, unreached, max_level,
    launches): int64 numpy [B], the seed pixels outside the region, the region pixels left 0 and the largest L written, and the
    pair (launches of stage 1, launches of stage 2), the final one of each that changed nothing included.
    Exact, on the device (unet_flood_init / unet_flood_sweeps / unet_flood_assign / unet_flood_finish), with split_cells' loop
    for each stage: _launches launches are enqueued, their change counts read back in one copy, and the loop ends at the first
    launch that changed nothing; _launches changes no result.  To flood a shape instead of an intensity, pass the inverted
    distance map as the image: watershed(shape_seeds(mask)[0], d.max() - d, mask=mask) with d = distance_map(mask) scaled into
    [0, 65536).
    connectivity: keyword only, 4 (the default, all of the above) or 8.  With 8 a step goes to any of the eight neighbours that
    lies in the region, whatever the two pixels beside a diagonal step are, so a one-pixel-thick diagonal wall does not separate.
    The extension of a key is the same, the minimum runs over eight neighbours, a parent is any of the eight whose key extends
    to exactly key(q), and on a constant image the result is split_cells(connectivity=8)'s, bit for bit (unet_flood_sweeps_conn,
    unet_flood_assign_conn).
    A connectivity other than 4 or 8 (checked first), unequal shapes, other seed dtypes, levels or max_level out of range, image values outside [0, 65536) or not
    finite (counted by the kernel), negative ids and ids >= 2^24 raise ValueError; host tensors raise NotImplementedError (no CPU
    path)."""
    _check_connectivity("watershed", connectivity)
    tensors = [seeds, image] + ([] if mask is None else [mask])
    _all_tensors("watershed", "unet_flood_init", tensors)
    _same_shape("watershed", "seeds, an image and a mask of equal shape [H,W] or [B,H,W]", tensors)
    _need_ids("watershed", "seed ids", seeds)
    if image.is_complex():
        raise ValueError("watershed takes a real image, got %s" % image.dtype)
    if image.is_floating_point():
        _int_in(levels, 1, FLOOD_LEVELS + 1, "watershed: a float image needs levels, an int in [1, %d], got %%r" % FLOOD_LEVELS, (int,))
    elif levels is not None:
        raise ValueError("watershed: levels is for float images; an integer image is read as it is, got levels=%r for %s" % (levels, image.dtype))
    top = _limit("watershed", "max_level", max_level, cap=FLOOD_LEVELS)
    if int(_launches) < 1:
        raise ValueError("watershed: _launches must be >= 1")
    planes = _device_planes("watershed", "unet_flood_init", tensors)
    import _hip
    _id_range("watershed", planes[0])
    sd = planes[0].int()
    im, im_code = _int_code(planes[1], uint8_ok=True)
    mk, mk_code = _int_code(planes[2], uint8_ok=True) if mask is not None else (None, 0)
    B, H, W = sd.shape
    dev = sd.device
    counts = torch.empty(3, B, dtype=torch.int32, device=dev)          # the library's u32 words: at most H * W < 2^31
    status = torch.empty(2, B, dtype=torch.int64, device=dev)
    scratch = _hip.scratch("unet_flood", dev, B, H, W)
    _hip.run("unet_flood_init", dev, _hip.ptr(sd), _hip.ptr(im), im_code, levels or 0, _hip.ptr(mk), mk_code, B, H, W, _hip.ptr(counts[0]),
             _hip.ptr(status), _hip.ptr(scratch))
    def values_ok():
        bad = int(status[1].sum())
        if bad:
            raise ValueError("watershed: %d pixels hold an image value that is not finite" % bad if im_code == 1 else
                             "watershed: %d pixels hold an image value outside [0, %d)" % (bad, FLOOD_LEVELS))

    launches = [_sweep_to_idle("unet_flood_sweeps_conn", dev, B, _launches, (B, H, W, top, connectivity), (_hip.ptr(scratch),), values_ok),
                _sweep_to_idle("unet_flood_assign_conn", dev, B, _launches, (B, H, W, connectivity), (_hip.ptr(scratch),))]   # after an idle stage-1 launch
    labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    lev, dist = (torch.empty(2, B, H, W, dtype=torch.int32, device=dev) if return_levels else (None, None))
    _hip.run("unet_flood_finish", dev, B, H, W, _hip.ptr(labels), _hip.ptr(lev), _hip.ptr(dist), _hip.ptr(counts[1]), _hip.ptr(counts[2]),
             _hip.ptr(scratch))
    outside, unreached, high = counts.cpu().numpy().astype(np.int64)
    out = (_unbatch(seeds, labels), FloodInfo(seeds_outside=outside, unreached=unreached, max_level=high, launches=tuple(launches)))
    return out + _unbatch(seeds, lev, dist) if return_levels else out


_EDGES = {'ignore': 0, 'background': 1}
SHAPE_EDGE = 32767                                                     # H, W of the shape ops: H^2 + W^2 fits int32


def _shape_sizes(name, B, H, W):
    if H > SHAPE_EDGE or W > SHAPE_EDGE or H * W >= 1 << 31 or B > 65535:
        raise ValueError("%s: H and W are at most %d with H * W < 2^31 (a squared distance is an int32) and B at most 65535, got %s"
                         % (name, SHAPE_EDGE, (B, H, W)))


def distance_map(mask, *, edge='ignore'):
    """The exact squared Euclidean distance map of the interior of a mask [H,W] or [B,H,W] on a HIP device (the region is
    mask != 0, of any dtype split_cells takes): int32 of the mask's shape, d2(p) = the squared distance from region pixel p to the
    nearest pixel outside the region, 0 outside the region.  edge='ignore': pixels beyond the image are nothing
    (scipy.ndimage.distance_transform_edt's convention), and an image with no pixel outside the region gets H^2 + W^2 everywhere,
    above every real value (at most (H-1)^2 + (W-1)^2).  edge='background': pixels beyond the image are background, so the pixel in
    row y, column x is at distance min(x+1, W-x, y+1, H-y) from it.  On the device (unet_distance_map), nothing is read back.
    H or W above 32767 or H*W >= 2^31 and a bad edge raise ValueError; host tensors raise NotImplementedError (no CPU path)."""
    if not torch.is_tensor(mask):
        raise NotImplementedError("distance_map takes a tensor on the HIP device (unet_distance_map); there is no CPU implementation")
    if edge not in _EDGES:
        raise ValueError("distance_map: edge must be 'ignore' or 'background', got %r" % (edge,))
    mk, code = _int_code(*_device_planes("distance_map", "unet_distance_map", [mask], _shape_sizes), uint8_ok=True)
    import _hip
    B, H, W = mk.shape
    d2 = torch.empty(B, H, W, dtype=torch.int32, device=mk.device)
    scratch = _hip.scratch("unet_distance_map", mk.device, B, H, W)
    _hip.run("unet_distance_map", mk.device, _hip.ptr(mk), code, B, H, W, _EDGES[edge], _hip.ptr(d2), _hip.ptr(scratch))
    return _unbatch(mask, d2)


ReconInfo = collections.namedtuple("ReconInfo", "launches raised")
RECON_TOP = 1 << 30


def reconstruct(marker, under, *, mask=None, connectivity=4, _launches=8):
    """Grey reconstruction by dilation, 4-connected (8-connected with connectivity=8), on integers: marker and under int32 / int64 [H,W] or [B,H,W] on a HIP device
    with values in [0, 2^30]; the region is mask != 0 (the same shape, of any dtype split_cells takes), everything when mask is
    None.  R is the least function on the region with R >= min(marker, under), R <= under and R(p) >= min(under(p), R(n)) for
    every region 4-neighbour n; equivalently R(p) is the maximum over region pixels q of min(marker(q), the minimum of under along
    the best 4-path from q to p inside the region).  With connectivity=8 the neighbours are the eight and the paths 8-paths, a
    diagonal step allowed whatever the two pixels beside it are (skimage.morphology.reconstruction's default footprint;
    unet_reconstruct_sweeps_conn).  Outside the region R is 0.  Returns (R, ReconInfo): R int32 of the input's
    shape; ReconInfo(launches, raised): the launches the reconstruction needed, the final one that raised nothing included
    (counted as SplitInfo.launches is), and raised int64 numpy [B], the pixels whose final value exceeds min(marker, under).
    Exact, on the device (unet_reconstruct_init / unet_reconstruct_sweeps / unet_reconstruct_finish): _launches launches are
    enqueued, their change counts read back in one copy, and the loop ends at the first launch that raised nothing; _launches
    changes no result.  A connectivity other than 4 or 8 (checked first), unequal shapes, other dtypes, values outside [0, 2^30]
    (counted by the kernel), H or W above 32767 raise ValueError; host tensors raise NotImplementedError (no CPU path)."""
    _check_connectivity("reconstruct", connectivity)
    tensors = [marker, under] + ([] if mask is None else [mask])
    _all_tensors("reconstruct", "unet_reconstruct_init", tensors)
    _same_shape("reconstruct", "marker, under and mask of equal shape [H,W] or [B,H,W]", tensors)
    _need_ids("reconstruct", "marker and under", marker, under)
    if int(_launches) < 1:
        raise ValueError("reconstruct: _launches must be >= 1")
    planes = _device_planes("reconstruct", "unet_reconstruct_init", tensors, _shape_sizes)
    import _hip
    B, H, W = planes[0].shape
    (mr, mr_code), (un, un_code) = _int_code(planes[0]), _int_code(planes[1])
    mk, mk_code = _int_code(planes[2], uint8_ok=True) if mask is not None else (None, 0)
    dev = mr.device
    status = torch.empty(B, dtype=torch.int64, device=dev)
    raised = torch.empty(B, dtype=torch.int32, device=dev)             # the library's u32 words: at most H * W < 2^31
    scratch = _hip.scratch("unet_reconstruct", dev, B, H, W)
    _hip.run("unet_reconstruct_init", dev, _hip.ptr(mr), mr_code, _hip.ptr(un), un_code, _hip.ptr(mk), mk_code, B, H, W, _hip.ptr(status),
             _hip.ptr(scratch))
    def values_ok():
        bad = int(status.sum())
        if bad:
            raise ValueError("reconstruct: %d pixels hold a marker or under value outside [0, 2^30]" % bad)

    launches = _sweep_to_idle("unet_reconstruct_sweeps_conn", dev, B, _launches, (B, H, W, connectivity), (_hip.ptr(scratch),), values_ok)
    out = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    _hip.run("unet_reconstruct_finish", dev, B, H, W, _hip.ptr(out), _hip.ptr(raised), _hip.ptr(scratch))
    return _unbatch(marker, out), ReconInfo(launches=launches, raised=raised.cpu().numpy().astype(np.int64))


def shape_seeds(mask, h=2.0, *, min_radius=0.0, edge='ignore', connectivity=4):
    """Seeds for split_cells from the shape of a mask alone: the h-maxima of its distance map.  mask [H,W] or [B,H,W] on a HIP
    device (the region is mask != 0, of any dtype split_cells takes); returns (seeds, n): seeds int32 of the mask's shape, 0 = no
    seed, the seeds numbered 1..n[b] in label_cells' raster order; n int32 [B].  Integers throughout: q = isqrt(256 d2) is the
    floor of distance_map(mask, edge=edge) in 1/16 pixel, hq = round(16 h), rq = ceil(16 min_radius).  R1 is the h-maxima
    transform of q inside the region, the reconstruction of q - hq under q; its regional maxima are the region pixels where the
    reconstruction R2 of R1 - 1 under R1 stays below R1; a seed pixel is such a pixel with R1 + hq >= rq (on a maximal plateau
    R1 + hq is the dome's peak, so a whole dome is kept or dropped); the seeds are label_cells of the seed pixels.  The transform
    runs on heights lifted by hq (the reconstruction of q under q + hq, which is R1 + hq), so q - hq is never cut off at 0: inside
    a component with a pixel above hq the cut changes nothing, and a component that lies at or below hq everywhere is one dome
    and one seed where the cut would leave it flat at 0 and without any.
    Consequences: two peaks merge iff the saddle between them, by the best 4-path inside the region, is >= the lower peak - h
    (in 1/16 pixel: lower peak - saddle <= hq); h = 0 gives all regional maxima of q; every region component with max q >= rq
    gets at least one seed.  The default h = 2: along a diagonal ridge the 4-connected staircase makes spurious maxima less than
    1 px deep (two discs of r = 12 on a diagonal give 9 seeds at h = 0, 3 at 0.5 and 2 from 1 on).
    connectivity=8: both reconstructions are 8-connected ("4-path" above reads "8-path") and the seed pixels are labelled with
    label_cells(..., connectivity=8); the distance map is Euclidean and does not change.  A diagonal ridge is then no staircase
    and has no spurious maxima: the same two discs give 2 seeds at every h >= 0, as skimage.morphology.h_maxima's default
    footprint does.
    On the device throughout (unet_distance_map, unet_shape_heights / _lower / _maxima, two reconstruct calls,
    unet_label_components), on the current stream.  A connectivity other than 4 or 8 (checked first), h < 0 or above 2^24,
    min_radius < 0, a bad edge and the shapes distance_map refuses raise ValueError; host tensors raise NotImplementedError (no CPU path)."""
    _check_connectivity("shape_seeds", connectivity)
    if not torch.is_tensor(mask):
        raise NotImplementedError("shape_seeds takes a tensor on the HIP device (unet_distance_map); there is no CPU implementation")
    _real_in(h, 0, 1 << 24, "shape_seeds: h must be a number in [0, 2^24], got %r")
    _real_in(min_radius, 0, math.inf, "shape_seeds: min_radius must be a number >= 0, got %r")
    hq, rq = int(round(16 * h)), int(min(math.ceil(16 * min(min_radius, 1 << 26)), 1 << 30))
    d2 = _planes("shape_seeds", distance_map(mask, edge=edge))
    import _hip
    B, H, W = d2.shape
    dev = d2.device
    mk = _planes("shape_seeds", mask)
    q, lifted = torch.empty_like(d2), torch.empty_like(d2)
    _hip.run("unet_shape_heights", dev, _hip.ptr(d2), B, H, W, hq, _hip.ptr(q), _hip.ptr(lifted))
    r1 = reconstruct(q, lifted, mask=mk, connectivity=connectivity)[0]
    _hip.run("unet_shape_lower", dev, _hip.ptr(r1), B, H, W, 1, _hip.ptr(q))
    r2 = reconstruct(q, r1, mask=mk, connectivity=connectivity)[0]
    peaks = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    _hip.run("unet_shape_maxima", dev, _hip.ptr(r1), _hip.ptr(r2), B, H, W, rq, _hip.ptr(peaks))
    seeds, n = label_cells(peaks, connectivity=connectivity)
    return _unbatch(mask, seeds), n


# ---- boundary scores: Hausdorff, its percentile, surface distance, surface Dice -------------------------------------------

SurfaceSums = collections.namedtuple("SurfaceSums", "record d2_pred d2_gt t2 q_num q_den")
BoundaryScores = collections.namedtuple("BoundaryScores", "hausdorff hd_percentile assd nsd precision recall boundary_f1 n_pred n_gt")
SURFACE_TOLERANCES = 4                                                 # thresholds of one unet_surface_sums call
SURFACE_Q_DEN = 1 << 20                                                # its percentile is q_num / q_den with q_den below this


def _boundary_rules(name, select, connectivity, edge):
    _check_connectivity(name, connectivity)
    if edge not in _EDGES:
        raise ValueError("%s: edge must be 'ignore' or 'background', got %r" % (name, edge))
    if select is None:
        return -1
    return int(_int_in(select, 0, 1 << 31, name + ": select must be None or a class index in [0, 2^31), got %r"))


def _boundary_masks(name, entry, *masks):
    """The checks of the boundary ops on one or two masks: tensors (NotImplementedError), rank, dtype, equal shapes, sizes
    (ValueError, on any device), then the device (NotImplementedError).  Returns [(contiguous [B,H,W], dtype code)]."""
    _all_tensors(name, entry, masks)
    for m in masks:
        if m.is_complex():
            raise ValueError("%s takes masks of a real dtype, got %s" % (name, m.dtype))
    _same_shape(name, "masks of equal shape", masks, ranked=False)
    return [_int_code(p, uint8_ok=True) for p in _device_planes(name, entry, masks, _shape_sizes)]


def mask_boundary(mask, *, select=None, connectivity=4, edge='background'):
    """The contour of a mask [H,W] or [B,H,W] on a HIP device (unet_mask_boundary): uint8 of the mask's shape, 1 on the region
    pixels that have a neighbour outside the region, 0 elsewhere.  The region is mask != 0, with select=k it is mask == k (the
    class-k region of a label map).  connectivity 4 or 8: which neighbours count.  edge='background' (the default; what
    scipy.ndimage.binary_erosion(border_value=0) and MONAI's get_mask_edges do): pixels past the image are outside the region, so
    region pixels on the frame are contour; edge='ignore': pixels past the image are nothing.  Nothing is read back.  A bad
    connectivity, edge, select, rank or size raise ValueError; host tensors raise NotImplementedError (no CPU path)."""
    k = _boundary_rules("mask_boundary", select, connectivity, edge)
    ((mk, code),) = _boundary_masks("mask_boundary", "unet_mask_boundary", mask)
    import _hip
    B, H, W = mk.shape
    out = torch.empty(B, H, W, dtype=torch.uint8, device=mk.device)
    _hip.run("unet_mask_boundary", mk.device, _hip.ptr(mk), code, k, B, H, W, connectivity, _EDGES[edge], _hip.ptr(out))
    return _unbatch(mask, out)


def _surface_fraction(name, what, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating, fractions.Fraction)) or not math.isfinite(v):
        raise ValueError("%s: %s must be a finite number, got %r" % (name, what, v))
    return fractions.Fraction(v.item() if isinstance(v, np.generic) else v)


def _percentile_fraction(name, percentile):
    """percentile in [0, 100] -> q = q_num / q_den exactly; a float whose binary value needs q_den >= 2^20 (99.9) is read by its
    shortest decimal form (999 / 1000), and only past that rounded to the nearest fraction with a smaller denominator."""
    p = _surface_fraction(name, "percentile", percentile)
    if not 0 <= p <= 100:
        raise ValueError("%s: percentile must be in [0, 100], got %r" % (name, percentile))
    q = p / 100
    if q.denominator >= SURFACE_Q_DEN and isinstance(percentile, (float, np.floating)):
        q = fractions.Fraction(repr(float(percentile))) / 100
    if q.denominator >= SURFACE_Q_DEN:
        q = q.limit_denominator(SURFACE_Q_DEN - 1)
    return q.numerator, q.denominator


def surface_sums(pred, gt, *, tolerances=(1.0,), percentile=95, select=None, connectivity=4, edge='background', return_maps=False):
    """What the boundary scores of a predicted mask against the ground truth are formed from, on the device (unet_surface_sums):
    pred, gt [H,W] or [B,H,W] of equal shape, of any dtype split_cells takes.  Region, contour, connectivity, edge and select as
    mask_boundary (select applies to both masks).  For both directions, pred -> gt (index 0) and gt -> pred (index 1), with d2(p) the
    exact squared Euclidean distance from contour pixel p to the nearest pixel of the other contour:
      record   int64 [B, 2, 10] ([2, 10] for a single image): n = the contour's pixels, max d2, lo, hi, rem (the two order statistics
               of d2 around the percentile and the numerator of the interpolation weight), the pixels with d2 <= T2[i] for up to 4
               tolerances (T2 = floor(tolerance^2), exactly), and, as the bits of word 9, the fp64 sum of sqrt(d2)
      d2_pred, d2_gt   with return_maps: int32 of the masks' shape, d2 on the contour of pred (gt), -1 elsewhere; else None
      t2, q_num, q_den   the squared tolerances and the percentile as the exact fraction the device used (host values)
    tolerances are in pixels.  percentile is a number in [0, 100].  Nothing is read back; every word is the same in every run.
    scores_from_surface forms the scores.  More than 4 tolerances, a negative or non-finite one, a percentile outside [0, 100], a
    bad connectivity, edge or select, shapes that differ and sizes distance_map refuses raise ValueError; host tensors raise
    NotImplementedError (no CPU path)."""
    k = _boundary_rules("surface_sums", select, connectivity, edge)
    tol = tuple(tolerances)
    if len(tol) > SURFACE_TOLERANCES:
        raise ValueError("surface_sums: at most %d tolerances, got %d" % (SURFACE_TOLERANCES, len(tol)))
    t2 = []
    for t in tol:
        f = _surface_fraction("surface_sums", "a tolerance", t)
        if f < 0:
            raise ValueError("surface_sums: a tolerance must not be negative, got %r" % (t,))
        t2.append(min(math.floor(f * f), (1 << 31) - 1))               # no d2 is above 2^31 - 1
    q_num, q_den = _percentile_fraction("surface_sums", percentile)
    (p, pcode), (g, gcode) = _boundary_masks("surface_sums", "unet_surface_sums", pred, gt)
    import ctypes
    import _hip
    B, H, W = p.shape
    dev = p.device
    record = torch.empty(B, 2, 10, dtype=torch.int64, device=dev)
    maps = [torch.empty(B, H, W, dtype=torch.int32, device=dev) if return_maps else None for _ in range(2)]
    scratch = _hip.scratch("unet_surface_sums", dev, B, H, W)
    _hip.run("unet_surface_sums", dev, _hip.ptr(p), pcode, k, _hip.ptr(g), gcode, k, B, H, W, connectivity, _EDGES[edge], q_num, q_den,
             (ctypes.c_int * 4)(*(t2 + [0] * (4 - len(t2)))), len(t2), _hip.ptr(record), _hip.ptr(maps[0]), _hip.ptr(maps[1]), _hip.ptr(scratch))
    return SurfaceSums(*_unbatch(pred, record, *maps), tuple(t2), q_num, q_den)


def _check_spacing(name, spacing):
    if isinstance(spacing, bool) or not isinstance(spacing, (int, float, np.integer, np.floating)) or not (math.isfinite(spacing) and spacing > 0):
        raise ValueError("%s: spacing must be a positive finite number, got %r" % (name, spacing))


def scores_from_surface(sums, *, spacing=1.0):
    """The boundary scores of every image from the record of surface_sums (a device tensor, a host tensor or an array): pure numpy
    on the host.  Returns BoundaryScores of float64 arrays [B] (scalars for a single image), nsd, precision, recall and boundary_f1
    [B, tolerances]:
      hausdorff      sqrt(the larger of the two max d2)
      hd_percentile  the larger of the two directed percentiles of the distances, each numpy.percentile(d, p, method='linear'):
                     MONAI's convention, not medpy's percentile of the pooled distances
      assd           the average symmetric surface distance: (sum pred -> gt + sum gt -> pred) / (n_pred + n_gt)
      nsd            the normalised surface Dice at each tolerance: the contour pixels of both masks within it / (n_pred + n_gt)
      precision, recall, boundary_f1   the share of pred's contour within the tolerance of gt's, the reverse, their harmonic mean
      n_pred, n_gt   int64, the pixels of the two contours
    spacing, the size of a pixel, multiplies the distances; the tolerances were given to surface_sums in pixels (boundary_scores
    divides them).  Both contours empty: the distances are 0, nsd and boundary_f1 are 1; exactly one empty: inf and 0; precision
    (recall) is nan where pred's (gt's) contour is empty."""
    _check_spacing("scores_from_surface", spacing)
    rec = _host(sums.record)
    if rec.dtype != np.int64 or rec.ndim not in (2, 3) or rec.shape[-2:] != (2, 10):
        raise ValueError("scores_from_surface: record must be int64 [B, 2, 10] or [2, 10], got %s %s" % (rec.dtype, rec.shape))
    single = rec.ndim == 2
    rec = np.ascontiguousarray(rec.reshape(-1, 2, 10))
    k, spacing = len(sums.t2), float(spacing)
    n = rec[:, :, 0]
    both, none = (n > 0).all(axis=1), (n == 0).all(axis=1)
    total = n.sum(axis=1).astype(np.float64)

    def distance(v):                                                   # v: per image, valid where both contours exist
        return np.where(both, v, np.where(none, 0.0, np.inf)) * spacing
    lo, hi = np.sqrt(rec[:, :, 2].astype(np.float64)), np.sqrt(rec[:, :, 3].astype(np.float64))
    directed = lo + rec[:, :, 4].astype(np.float64) / float(sums.q_den) * (hi - lo)
    dsum = rec[:, :, 9].copy().view(np.float64)
    within = rec[:, :, 5:5 + k].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        assd = dsum.sum(axis=1) / total
        share = np.where(both[:, None], within.sum(axis=1) / total[:, None], np.where(none[:, None], 1.0, 0.0))
        precision, recall = within[:, 0] / n[:, 0, None], within[:, 1] / n[:, 1, None]          # 0 / 0 = nan: an empty side
        f1 = np.where(both[:, None], np.where(precision + recall > 0, 2 * precision * recall / (precision + recall), 0.0),
                      np.where(none[:, None], 1.0, 0.0))
    out = BoundaryScores(hausdorff=distance(np.sqrt(rec[:, :, 1].max(axis=1).astype(np.float64))), hd_percentile=distance(directed.max(axis=1)),
                         assd=distance(assd), nsd=share, precision=precision, recall=recall, boundary_f1=f1, n_pred=n[:, 0].copy(),
                         n_gt=n[:, 1].copy())
    return BoundaryScores(*(t[0] for t in out)) if single else out


def boundary_scores(pred, gt, *, tolerances=(1.0,), percentile=95, spacing=1.0, select=None, connectivity=4, edge='background'):
    """scores_from_surface(surface_sums(pred, gt, ...), spacing=spacing): the Hausdorff distance, its percentile, the average
    symmetric surface distance and the normalised surface Dice of a predicted mask against the ground truth, one read-back.
    tolerances are in the unit of spacing: they are divided by it, exactly, before they are squared."""
    _check_spacing("boundary_scores", spacing)
    s = _surface_fraction("boundary_scores", "spacing", spacing)
    tol = tuple(tolerances)
    for t in tol:
        _surface_fraction("boundary_scores", "a tolerance", t)
    sums = surface_sums(pred, gt, tolerances=[fractions.Fraction(t.item() if isinstance(t, np.generic) else t) / s for t in tol],
                        percentile=percentile, select=select, connectivity=connectivity, edge=edge)
    return scores_from_surface(sums, spacing=spacing)


def class_balance(gt_batch):
    """Per-image class-frequency weight map (functions.py:82-117): every pixel of value v gets
    count(second unique value) / count(v).  gt_batch: [B,H,W] -> float [B,H,W].
    Host tensors take the reference's CPU algorithm; {0,1} int64 labels already on the HIP device
    use unet_class_balance (two counting reductions and a select, no host round trip)."""
    if gt_batch.is_cuda:
        import _hip
        gt = gt_batch.contiguous()
        if gt.dtype != torch.int64:
            gt = gt.long()
        B, H, W = gt.shape
        w = torch.empty(B, H, W, dtype=torch.float32, device=gt.device)
        counts = torch.empty(B, dtype=torch.int64, device=gt.device)
        _hip.run("unet_class_balance", gt.device, _hip.ptr(gt), B, H, W, _hip.ptr(w), _hip.ptr(counts))
        if bool(((counts == 0) | (counts == H * W)).any()):      # the reference indexes counts[1]: a one-class image raises
            raise IndexError("index 1 is out of bounds for dimension 0 with size 1")
        return w
    gt_batch = gt_batch.cpu()
    w_batch = torch.empty_like(gt_batch).float()
    for b in range(gt_batch.shape[0]):
        gt = gt_batch[b]
        uval, counts = torch.unique(gt, return_counts=True)
        w_c = torch.ones(gt.shape)
        for pos in range(len(uval)):
            w_c[gt == uval[pos]] = counts[1].float() / counts[pos].float()
        w_batch[b] = w_c
    return w_batch


def input_size_compute(image):
    """(original, input, output) sizes for the overlap-tile strategy (functions.py:121-146):
    smallest even L >= 20 with 16L-124 >= original; input = 16L+60; output = 16L-124."""
    original_size = image.shape[-1]
    lowest_res = 20
    while 16 * lowest_res - 124 < original_size:
        lowest_res += 2
    return original_size, 16 * lowest_res + 60, 16 * lowest_res - 124


def Pixel_error(pred, label):
    pred_np = pred.cpu().numpy()
    label_np = label.cpu().numpy()
    return np.sum(abs(pred_np - label_np)) / pred_np.size


def IoU(pred, label):
    pred_np = pred.cpu().numpy()
    label_np = label.cpu().numpy()
    return np.sum(np.logical_and(pred_np, label_np)) / np.sum(np.logical_or(pred_np, label_np))


def metrics_from_counts(inter, union, diff, size):
    """IoU and pixel error from the integer counts unet_eval_masks produces on the device."""
    out = np.empty([2, 1])
    out[0] = inter / union
    out[1] = diff / size
    return out


def metrics_from_confusion(conf_b):
    """[[IoU],[pixel error]] of one image from its K x K confusion counts (optim.crop_argmax_confusion, conf[i, j] = pixels
    labelled i predicted j), the same (2,1) shape as metrics_from_counts: IoU = mean over the foreground classes 1..K-1 with
    a nonzero union of inter / union (nan when there is none, like the binary 0/0); PE = mismatched pixels / pixels.
    At K = 2 both equal metrics_from_counts' values exactly."""
    conf = np.asarray(conf_b, dtype=np.int64)
    K = conf.shape[0]
    out = np.empty([2, 1])
    ious = []
    for c in range(1, K):
        inter = int(conf[c, c])
        union = int(conf[c, :].sum() + conf[:, c].sum() - conf[c, c])
        if union:
            ious.append(inter / union)
    with np.errstate(invalid='ignore'):
        out[0] = np.float64(np.nan) if not ious else (ious[0] if len(ious) == 1 else np.mean(ious))
    size = int(conf.sum())
    out[1] = (size - int(np.trace(conf))) / size
    return out


def dice_from_confusion(conf):
    """The hard per-class Dice 2 TP / (2 TP + FP + FN) from K x K confusion counts (optim.crop_argmax_confusion, conf[..., i, j] =
    pixels labelled i predicted j; any leading axes, e.g. [B,K,K]): float64 [..., K], NaN for a class that is absent from
    both the labels and the prediction."""
    conf = np.asarray(conf.cpu() if hasattr(conf, 'cpu') else conf, dtype=np.int64)
    tp = np.diagonal(conf, axis1=-2, axis2=-1).astype(np.float64)
    denom = (conf.sum(axis=-1) + conf.sum(axis=-2)).astype(np.float64)        # (TP + FN) + (TP + FP)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(denom > 0, 2.0 * tp / denom, np.nan)


def evaluation_metrics(pred, label):
    """[[IoU],[pixel error]] as a (2,1) array (functions.py:150-170)."""
    out = np.empty([2, 1])
    out[0] = IoU(pred, label)
    out[1] = Pixel_error(pred, label)
    return out
