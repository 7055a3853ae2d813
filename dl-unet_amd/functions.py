"""Drop-in for the reference's functions.py helpers that sit either side of the hot path.

input_size_compute / evaluation_metrics / IoU / Pixel_error / class_balance keep the reference's
names, arguments and results (functions.py:82-213).  They are host-side bookkeeping on labels and
388^2 masks (SURVEY §2 rows 5,7,8: out of scope as kernels).  weighted_map (functions.py:7-78, the paper's
border-weighted loss map) runs on the device only (unet_weighted_map); the reference's own OpenCV path has no
host counterpart here.
"""
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
