"""Drop-in for the reference's functions.py helpers that sit either side of the hot path.

input_size_compute / evaluation_metrics / IoU / Pixel_error / class_balance keep the reference's
names, arguments and results (functions.py:82-213).  They are host-side bookkeeping on labels and
388^2 masks (SURVEY §2 rows 5,7,8: out of scope as kernels).  weighted_map (functions.py:7-78, the paper's
border-weighted loss map) runs on the device only (unet_weighted_map); the reference's own OpenCV path has no
host counterpart here.  label_cells and seg_measure are extensions, device only as well: the cell instances of a mask
(unet_label_components) and the Cell Tracking Challenge SEG measure of two instance maps (unet_instance_overlap), the score
the goals of trainer.py:20-26 are stated in.
"""
import collections

import numpy as np
import torch


def weighted_map(gt_batch, *, w0=20, sig2=25, return_objects=False):
    """Border weight map of Ronneberger et al. 2015, eq. 2 (functions.py:7-78) for {0,1} labels [B,H,W] on a HIP device:
    1 on cells; on background w_c + w0 * exp(-(d1 + d2)^2 / (2 sig2)), d1 / d2 the exact distances to the nearest and
    second-nearest distinct 4-connected cell (d2 = 0 when the image has one).  w_c = count(1) / count(0) takes the
    label's dtype as in the reference (torch.empty_like(gt)): truncated for integer labels (DESIGN Q9), fp32 for float
    labels.  Returns float32 [B,H,W] (and the int32 [B] component counts with return_objects=True).  A one-class image
    raises IndexError as the reference does at counts[1]; host tensors raise NotImplementedError (no CPU path)."""
    if not gt_batch.is_cuda:
        raise NotImplementedError("weighted_map runs on the HIP device only (unet_weighted_map): move the labels to the "
                                  "device first, e.g. weighted_map(gt_batch.cuda()); there is no CPU implementation")
    import _hip
    if gt_batch.dim() != 3:
        raise ValueError("weighted_map takes labels [B,H,W], got %s" % (tuple(gt_batch.shape),))
    gt = gt_batch.contiguous()
    if gt.is_floating_point():
        gt, code = gt.float(), 1
    else:
        gt, code = gt.long(), 0
    B, H, W = gt.shape
    w = torch.empty(B, H, W, dtype=torch.float32, device=gt.device)
    counts = torch.empty(B, dtype=torch.int64, device=gt.device)
    n_objects = torch.empty(B, dtype=torch.int32, device=gt.device)
    if B * H * W == 0:
        raise IndexError("index 1 is out of bounds for dimension 0 with size 0")
    scratch = torch.empty(_hip.lib().unet_weighted_map_scratch_bytes(B, H, W), dtype=torch.uint8, device=gt.device)
    _hip.run("unet_weighted_map", gt.device, _hip.ptr(gt), code, B, H, W, float(w0), float(sig2), _hip.ptr(w), _hip.ptr(counts),
             _hip.ptr(n_objects), _hip.ptr(scratch))
    if bool(((counts == 0) | (counts == H * W)).any()):      # the reference indexes counts[1]: a one-class image raises
        raise IndexError("index 1 is out of bounds for dimension 0 with size 1")
    return (w, n_objects) if return_objects else w


def label_cells(mask):
    """The cell instances of a foreground mask [H,W] or [B,H,W] on a HIP device (foreground = value != 0; bool / integer masks
    go in as int64, float ones as float32): returns (labels, n_objects), labels int32 of the mask's shape, 0 on background
    and 1..n on the 4-connected components, numbered in raster order of their first pixel like scipy.ndimage.label and
    cv.connectedComponents(connectivity=4) (functions.py:47); n_objects int32 [B] ([1] for a single image) = n.
    Host tensors raise NotImplementedError (no CPU path)."""
    if not mask.is_cuda:
        raise NotImplementedError("label_cells runs on the HIP device only (unet_label_components): move the mask to the "
                                  "device first, e.g. label_cells(mask.cuda()); there is no CPU implementation")
    import _hip
    if mask.dim() not in (2, 3):
        raise ValueError("label_cells takes a mask [H,W] or [B,H,W], got %s" % (tuple(mask.shape),))
    m = (mask[None] if mask.dim() == 2 else mask).contiguous()
    if m.is_floating_point():
        m, code = m.float(), 1
    else:
        m, code = m.long(), 0
    B, H, W = m.shape
    if B * H * W == 0:
        raise ValueError("label_cells: empty mask %s" % (tuple(mask.shape),))
    labels = torch.empty(B, H, W, dtype=torch.int32, device=m.device)
    n_objects = torch.empty(B, dtype=torch.int32, device=m.device)
    scratch = torch.empty(_hip.lib().unet_label_components_scratch_bytes(B, H, W), dtype=torch.uint8, device=m.device)
    _hip.run("unet_label_components", m.device, _hip.ptr(m), code, B, H, W, _hip.ptr(labels), _hip.ptr(n_objects), _hip.ptr(scratch))
    return (labels[0] if mask.dim() == 2 else labels), n_objects


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
    if not (pred_labels.is_cuda and gt_labels.is_cuda):
        raise NotImplementedError("seg_measure runs on the HIP device only (unet_instance_overlap): move the label maps to the "
                                  "device first, e.g. seg_measure(pred.cuda(), gt.cuda()); there is no CPU implementation")
    import _hip
    if pred_labels.shape != gt_labels.shape or pred_labels.dim() not in (2, 3):
        raise ValueError("seg_measure takes two id maps of equal shape [H,W] or [B,H,W], got %s and %s"
                         % (tuple(pred_labels.shape), tuple(gt_labels.shape)))
    for t in (pred_labels, gt_labels):
        if t.dtype not in (torch.int32, torch.int64):
            raise ValueError("seg_measure takes int32 or int64 id maps, got %s" % t.dtype)
    if pred_labels.numel() == 0:
        raise ValueError("seg_measure: empty id maps %s" % (tuple(pred_labels.shape),))
    pred, gt = ((t[None] if t.dim() == 2 else t).contiguous() for t in (pred_labels, gt_labels))
    B, H, W = gt.shape
    dev = gt.device
    lo, ng_max, np_max = (int(v) for v in torch.stack([torch.minimum(gt.min(), pred.min()).long(), gt.max().long(), pred.max().long()]).tolist())
    if lo < 0:
        raise ValueError("seg_measure: negative ids (the smallest is %d)" % lo)
    if max(ng_max, np_max) >= 1 << 24:
        raise ValueError("seg_measure: ids must be below 2^24, got up to %d" % max(ng_max, np_max))
    gt, pred = gt.int(), pred.int()
    area_gt = torch.empty(B, ng_max + 1, dtype=torch.int32, device=dev)         # the library's u32 / u64 words: counts of at
    area_pred = torch.empty(B, np_max + 1, dtype=torch.int32, device=dev)       # most H * W < 2^31, so the signed views agree
    match = torch.empty(B, ng_max + 1, dtype=torch.int32, device=dev)
    inter = torch.empty(B, ng_max + 1, dtype=torch.int32, device=dev)
    status = torch.empty(B, 2, dtype=torch.int64, device=dev)
    slots = 1 << (4 * (ng_max + np_max) + 1024 - 1).bit_length() if _table_slots is None else int(_table_slots)
    while True:
        scratch = torch.empty(_hip.lib().unet_instance_overlap_scratch_bytes(B, ng_max, np_max, slots), dtype=torch.uint8, device=dev)
        _hip.run("unet_instance_overlap", dev, _hip.ptr(gt), _hip.ptr(pred), B, H, W, ng_max, np_max, slots, _hip.ptr(area_gt),
                 _hip.ptr(area_pred), _hip.ptr(match), _hip.ptr(inter), _hip.ptr(status), _hip.ptr(scratch))
        st = status.cpu()
        if int(st[:, 0].sum()):
            raise ValueError("seg_measure: %d pixels hold ids outside [0, %d] / [0, %d]" % (int(st[:, 0].sum()), ng_max, np_max))
        if not int(st[:, 1].sum()):
            break
        slots *= 2                      # ends: a table with more slots than pixels cannot fill up
    return seg_from_counts(area_gt.cpu().numpy(), area_pred.cpu().numpy(), match.cpu().numpy(), inter.cpu().numpy())


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


def evaluation_metrics(pred, label):
    """[[IoU],[pixel error]] as a (2,1) array (functions.py:150-170)."""
    out = np.empty([2, 1])
    out[0] = IoU(pred, label)
    out[1] = Pixel_error(pred, label)
    return out
