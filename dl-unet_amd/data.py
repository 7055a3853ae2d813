"""GPU versions of the reference's data.py transforms that sit directly either side of the hot path
(SURVEY §8f).  Same names and meaning as the reference functions; tensors stay on the HIP device.

  mirror_transform(image)            data.py:249-277   overlap-tile border (N2), asymmetric reflection kept
  mirror_transform_tensor(image)     data.py:281-312
  test_input(images)                 data.py:184-188   mirror + (x-min)/ptp for a batch (ImageDataset_test)
  elastic_transform(images, a, s)    data.py:225-245   Simard-2003 elastic deformation (N1)
  grid_displacements(rs, B, G, s)    -                 the paper's random displacement vectors on a coarse G x G grid
  elastic_grid(images, disp, a)      -                 the paper's elastic deformation: that grid, bicubic, bilinear warp
  reflect_rotate_crop(images, deg)   data.py:106-125   reflect pad + cubic-spline rotation + centre crop, fused (N1)
  grey_parameters(rs, B, ...)        -                 the random gamma, contrast, brightness, noise level, inversion per sample
  grey_variation(images, params)     -                 the paper's grey-value variation: those, applied in one fused pass
  augment(image, target, ...)        data.py:97-135    ImageDataset.__getitem__ after the file reads, on the device
  preprocess_gt(img)                 data.py:195-221   borders carved between touching cells of an instance image
  binary_target(img)                 data.py:63-64     preprocess_gt + cv.threshold(gt, 0, 255): the {0,255} training target
  crop_distribution(target, crop)    data.py:67-82     the crop origins and their weights (foreground share close to one half)
  draw_crop(rng, pairs, p, ...)      data.py:98-103    one origin from that distribution + jitter, in the reference's RNG order
  CropDataset(images, instances, ..) data.py:23-137    ImageDataset on arrays that are already read: an iterable of batches

File and TIFF reading, the ST/GT folder handling of ImageDataset.__init__ and the downloaders are out of scope (SURVEY §2
rows 9, 13).
"""
import ctypes as _C

import numpy as np
import torch

import _hip
from functions import _device_only, _int_code, _planes, input_size_compute


def _as_batch(image):
    if image.dim() == 2:
        return image[None]
    return image.reshape(-1, image.shape[-2], image.shape[-1])


def mirror_transform(image, normalise=False):
    """image: device tensor [n,n] (or [B,n,n] / [B,1,n,n]); returns [input_size,input_size] (or
    [B,1,S,S]) mirrored outwards like the reference (reflection without the edge pixel on the top/left
    band, with it on the bottom/right band)."""
    single = image.dim() == 2
    x = _as_batch(image).contiguous().float()
    if x.shape[-1] != x.shape[-2]:
        raise ValueError("mirror_transform expects square images")
    B, n, _ = x.shape
    _, S, _ = input_size_compute(x)
    mm = None
    if normalise:
        mm = torch.empty(B, 2, dtype=torch.float32, device=x.device)
        _hip.run("unet_minmax", x.device, _hip.ptr(x), B, n * n, _hip.ptr(mm))
    out = torch.empty(B, 1, S, S, dtype=torch.float32, device=x.device)
    _hip.run("unet_mirror_pad", x.device, _hip.ptr(x), B, n, S, _hip.ptr(mm), _hip.ptr(out))
    return out[0, 0] if single else out


def mirror_transform_tensor(image):
    """[(1),(1),n,n] -> [1,1,S,S] (data.py:281-312)."""
    n = image.shape[-1]
    return mirror_transform(image.reshape(1, n, n))


def test_input(images):
    """What ImageDataset_test.__getitem__ produces for the network (data.py:184-188), batched on the
    device: mirror to the input size, then (x - min) / ptp per image."""
    return mirror_transform(images if images.dim() >= 3 else images[None], normalise=True)


def gaussian_taps(sigma, truncate=4.0):
    radius = int(truncate * float(sigma) + 0.5)
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * k * k)
    return (w / w.sum()).astype(np.float32), radius


def elastic_transform(images, alpha, sigma, random_state=None, fields=None):
    """images: tuple of device tensors of equal shape [H,W] or [B,H,W]; every image of a sample is warped
    with the SAME displacement field (image and mask, data.py:128).  The two uniform[0,1) fields come
    from `fields`, from a numpy RandomState (drawn on the host exactly like the reference), or from
    torch.rand on the device.  Returns a list of warped tensors."""
    ref = _as_batch(images[0]).contiguous().float()
    B, H, W = ref.shape
    dev = ref.device
    # (host arrays are narrowed to fp32 by numpy: a torch CPU op on half a million elements goes through the intra-op thread
    #  pool, which on a GPU host's share of cores costs tens of milliseconds per call - measured 54 ms for one .float())
    if fields is not None:
        f0, f1 = [(f.to(dev, torch.float32) if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(dev))
                  .reshape(B, H, W).contiguous() for f in fields]
    elif random_state is not None:
        draws = [(random_state.rand(H, W), random_state.rand(H, W)) for _ in range(B)]    # per sample: dx field, then dy field
        f0 = torch.from_numpy(np.stack([d[0] for d in draws]).astype(np.float32)).to(dev)
        f1 = torch.from_numpy(np.stack([d[1] for d in draws]).astype(np.float32)).to(dev)
    else:
        f0 = torch.rand(B, H, W, device=dev); f1 = torch.rand(B, H, W, device=dev)
    w, radius = gaussian_taps(sigma)
    wd = torch.from_numpy(w).to(dev)
    tmp = torch.empty_like(f0)
    dx = torch.empty_like(f0); dy = torch.empty_like(f0)
    # dx displaces rows (axis 0), dy columns (axis 1) — the reference's naming (data.py:238-243)
    _hip.run("unet_gaussian_filter", dev, _hip.ptr((f0 * 2 - 1).contiguous()), B, H, W, _hip.ptr(wd), radius, float(alpha), _hip.ptr(tmp), _hip.ptr(dx))
    _hip.run("unet_gaussian_filter", dev, _hip.ptr((f1 * 2 - 1).contiguous()), B, H, W, _hip.ptr(wd), radius, float(alpha), _hip.ptr(tmp), _hip.ptr(dy))
    outs = []
    for im in images:
        x = _as_batch(im).contiguous().float()
        o = torch.empty_like(x)
        _hip.run("unet_warp_bilinear", dev, _hip.ptr(x), _hip.ptr(dx), _hip.ptr(dy), B, H, W, _hip.ptr(o))
        outs.append(o.reshape(im.shape))
    return outs


def grid_displacements(random_state, B, grid=3, sigma=10.0):
    """The random input of the paper's elastic deformation (Ronneberger et al. 3.1: "random displacement vectors on a coarse 3
    by 3 grid ... sampled from a Gaussian distribution with 10 pixels standard deviation"): float64 [B,2,grid,grid] in pixels,
    equal to random_state.normal(0, sigma, (B, 2, grid, grid)).  The draw order is the contract: sample after sample, for one
    sample the grid x grid row displacements (plane 0, row-major) before its column displacements (plane 1) - 2 grid^2 normal
    draws per sample and nothing else, so a caller can replay or interleave them."""
    G = int(grid)
    if G < 2:
        raise ValueError("grid_displacements: a grid of %d nodes per side, need at least 2" % G)
    if random_state is None:
        raise ValueError("grid_displacements draws from a numpy RandomState; got None")
    return random_state.normal(0, sigma, (int(B), 2, G, G))


MAX_ELASTIC_GRID = 16      # UNET_ELASTIC_MAX_GRID


def _grid_tensor(disp, B, dev, name):
    """disp [2,G,G] (every sample) or [B,2,G,G], numpy or tensor of any float type -> contiguous fp64 [B,2,G,G] on dev"""
    d = disp.detach() if torch.is_tensor(disp) else torch.from_numpy(np.ascontiguousarray(disp, dtype=np.float64))
    if d.dim() == 3:
        d = d[None].expand(B, *d.shape)
    if d.dim() != 4 or d.shape[0] != B or d.shape[1] != 2 or d.shape[2] != d.shape[3]:
        raise ValueError("%s: disp must be [2,G,G] or [%d,2,G,G], got %s" % (name, B, tuple(disp.shape)))
    if not 2 <= d.shape[2] <= MAX_ELASTIC_GRID:
        raise ValueError("%s: a grid of %d nodes per side, need 2 .. %d" % (name, d.shape[2], MAX_ELASTIC_GRID))
    return d.to(dev, torch.float64).contiguous()


def elastic_grid(images, disp, a=-0.5):
    """The paper's elastic deformation (Ronneberger et al. 3.1).  images: tuple of device tensors of equal shape
    [H,W] or [B,H,W]; every image of a sample is warped with the SAME displacements (image and mask).  disp: [B,2,G,G], or
    [2,G,G] for every sample alike - displacement vectors in pixels on a coarse corner-aligned G x G grid (plane 0 moves rows,
    plane 1 columns, elastic_transform's dx and dy; grid_displacements draws them), numpy or a tensor of any float type, used
    as fp64.  They are brought to every pixel by Keys' cubic convolution with parameter a (-0.5: Keys' third-order kernel,
    "bicubic" as MATLAB has it; -0.75: what torch's bicubic interpolate computes) and the images sampled bilinearly at the
    displaced coordinates, 0 outside the image, in one kernel in fp64 - no field exists in memory.  Returns the list of warped
    float32 tensors.  ValueError on host tensors, on shapes that do not agree and on G < 2; there is no CPU implementation."""
    if len(images) == 0:
        raise ValueError("elastic_grid: no image")
    for im in images:
        if not torch.is_tensor(im) or not im.is_cuda:
            raise ValueError("elastic_grid runs on the HIP device only (unet_elastic_grid): move the images to the device first")
        if im.dim() not in (2, 3) or im.shape != images[0].shape:
            raise ValueError("elastic_grid takes images of one shape [H,W] or [B,H,W], got %s" % ([tuple(i.shape) for i in images],))
    B, H, W = _as_batch(images[0]).shape
    if H < 2 or W < 2:
        raise ValueError("elastic_grid: a sample of %d x %d, need at least 2 x 2" % (H, W))
    dev = images[0].device
    d = _grid_tensor(disp, B, dev, "elastic_grid")
    outs = []
    for im in images:
        x = _as_batch(im).contiguous().float()
        o = torch.empty_like(x)
        _hip.run("unet_elastic_grid", dev, _hip.ptr(x), 1, B, H, W, _hip.ptr(d), d.shape[2], float(a), _hip.ptr(o))
        outs.append(o.reshape(im.shape))
    return outs


def reflect_rotate_crop(images, angles_deg, input_size=None, levels=255):
    """images: device tensor [n,n] or [B,n,n] (the random crop of the sample, e.g. 388^2); angles_deg: one angle or B angles
    (the reference draws one of 0,30,...,330 per sample, data.py:113).  Returns [S,S] / [B,S,S] with S = input_size: the centre
    of scipy.ndimage.rotate(np.pad(image, S, 'reflect'), deg) (data.py:106-125), fused so the 1532^2 padded / rotated
    images never exist.  levels=255 / 65535 reproduces scipy's rounding and clamping for the uint8 / uint16 images the reference loads;
    levels=0 keeps the float spline value."""
    single = images.dim() == 2
    x = _as_batch(images).contiguous().float()
    B, n, _ = x.shape
    if input_size is None:
        _, input_size, _ = input_size_compute(x)
    S = int(input_size)
    ang = np.atleast_1d(np.asarray(angles_deg, dtype=np.float32))
    if ang.size == 1 and B > 1:
        ang = np.repeat(ang, B)
    if ang.size != B:
        raise ValueError("need one angle per image")
    outs = []
    for lo in range(0, B, 64):                                    # the kernel takes up to 64 samples per call
        xb = x[lo:lo + 64]
        b = xb.shape[0]
        out = torch.empty(b, S, S, dtype=torch.float32, device=x.device)
        sc = _hip.scratch("unet_rotate", x.device, b, S)
        arr = (_C.c_float * b)(*[float(a) for a in ang[lo:lo + b]])
        _hip.run("unet_reflect_rotate_crop", x.device, _hip.ptr(xb), b, n, S, S, arr, int(levels), _hip.ptr(out), _hip.ptr(sc))
        outs.append(out)
    out = torch.cat(outs) if len(outs) > 1 else outs[0]
    return out[0] if single else out


MAX_GREY_SAMPLES = 64      # UNET_GREY_MAX_SAMPLES
GREY_NO_CLIP = 1           # UNET_GREY_NO_CLIP
GREY_IDENTITY = (1.0, 1.0, 0.0, 0.0, 0.0)      # gamma, contrast, brightness, sigma, invert: every stage skipped


def grey_parameters(random_state, B, *, gamma=(0.7, 1.5), contrast=(0.75, 1.25), brightness=(-0.1, 0.1), noise=(0.0, 0.05), p_invert=0.0):
    """The random input of grey_variation: float64 [B,5], row b = (gamma, contrast, brightness, sigma, invert) of sample b,
    drawn from random_state (a numpy RandomState).  The draw order is the contract: sample after sample, and for one sample
        gamma      = exp(random_state.uniform(log(gamma[0]), log(gamma[1])))     log-uniform: 0.7 and 1 / 0.7 are equally likely
        contrast   = random_state.uniform(contrast[0], contrast[1])
        brightness = random_state.uniform(brightness[0], brightness[1])
        sigma      = random_state.uniform(noise[0], noise[1])
        invert     = 1.0 if random_state.uniform(0.0, 1.0) < p_invert else 0.0
    - five uniform draws per sample and nothing else, whatever the ranges are: a degenerate range (v, v) still consumes its
    draw (and gives v), so the generator's state after B samples does not depend on the ranges."""
    if random_state is None:
        raise ValueError("grey_parameters draws from a numpy RandomState; got None")
    ranges = {"gamma": gamma, "contrast": contrast, "brightness": brightness, "noise": noise}
    for name, r in ranges.items():
        if len(r) != 2 or not np.all(np.isfinite(r)) or r[0] > r[1]:
            raise ValueError("grey_parameters: %s must be a finite range (lo, hi) with lo <= hi, got %r" % (name, r))
    if gamma[0] <= 0 or contrast[0] < 0 or noise[0] < 0 or not 0.0 <= p_invert <= 1.0:
        raise ValueError("grey_parameters: need gamma > 0, contrast >= 0, noise >= 0 and 0 <= p_invert <= 1")
    out = np.empty((int(B), 5), np.float64)
    for b in range(int(B)):
        out[b, 0] = np.exp(random_state.uniform(np.log(gamma[0]), np.log(gamma[1])))
        out[b, 1] = random_state.uniform(contrast[0], contrast[1])
        out[b, 2] = random_state.uniform(brightness[0], brightness[1])
        out[b, 3] = random_state.uniform(noise[0], noise[1])
        out[b, 4] = 1.0 if random_state.uniform(0.0, 1.0) < p_invert else 0.0
    return out


def _grey_rows(params, B, name):
    """params [B,5] (or [5] for one sample), numpy or tensor -> checked float64 numpy [B,5]"""
    p = params.detach().cpu().numpy() if torch.is_tensor(params) else np.asarray(params)
    p = np.ascontiguousarray(p, dtype=np.float64)
    if p.ndim == 1 and B == 1:
        p = p[None]
    if p.shape != (B, 5):
        raise ValueError("%s: params must be [%d,5] (gamma, contrast, brightness, sigma, invert per sample), got %s" % (name, B, p.shape))
    if not np.isfinite(p).all():
        raise ValueError("%s: a parameter is not finite" % name)
    if (p[:, 0] <= 0).any() or (p[:, 1] < 0).any() or (p[:, 3] < 0).any() or not np.isin(p[:, 4], (0.0, 1.0)).all():
        raise ValueError("%s: need gamma > 0, contrast >= 0, sigma >= 0 and invert 0 or 1" % name)
    return p


def _grey_run(x, out, rows, seed, step, first_sample, clip, mm):
    """unet_grey_vary on contiguous device fp32 x, out [B, ...] (out may be x) in chunks of 64 samples; mm [B,2] or None"""
    B = x.shape[0]
    n = x[0].numel()
    if int(first_sample) < 0 or int(first_sample) + B > 2 ** 32 or not 0 <= int(seed) < 2 ** 64 or not 0 <= int(step) < 2 ** 64:
        raise ValueError("grey variation: seed and step are unsigned 64-bit numbers, the sample index first_sample + b an unsigned 32-bit one")
    for lo in range(0, B, MAX_GREY_SAMPLES):
        b = min(MAX_GREY_SAMPLES, B - lo)
        sc = _hip.scratch("unet_grey", x.device, b, n)
        arr = (_C.c_double * (5 * b))(*rows[lo:lo + b].ravel().tolist())
        _hip.run("unet_grey_vary", x.device, _hip.ptr(x[lo:lo + b]), _hip.ptr(out[lo:lo + b]), b, n, int(first_sample) + lo, arr,
                 None if mm is None else _hip.ptr(mm[lo:lo + b]), int(seed), int(step), 0 if clip else GREY_NO_CLIP, _hip.ptr(sc))


def grey_variation(images, params, *, seed=0, step=0, first_sample=0, clip=True, minmax=None, out=None):
    """Grey-value variation (Ronneberger et al. 3.1; unet_grey_vary in include/unet_hip.h states the arithmetic) of
    device float32 images [H,W], [B,H,W] or [B,1,H,W], meant for images in [0,1].  params: [B,5] ([5] for one image), row b =
    (gamma, contrast, brightness, sigma, invert) of sample b, as grey_parameters draws them.  Per sample, in fp64: contrast
    about the sample's own mean plus brightness, clamped to [0,1]; u^gamma (1 - (1 - u)^gamma with invert); + sigma * z with z
    standard normal from Philox4x32-10 of (seed, step, first_sample + b, pixel) - no generator state, so equal arguments give
    equal bits on every run and stream; the clip to [0,1] unless clip=False.  A stage with identity parameters (contrast 1
    and brightness 0; gamma 1; sigma 0) is skipped.  minmax: device float32 [B,2] = (lo, hi) per sample; (x - lo) / (hi - lo)
    then runs first, in the same pass.  out: None (a new tensor), or a contiguous tensor of images' shape, which may be images
    itself.  A NaN pixel stays NaN, and a NaN anywhere in a sample whose contrast or brightness is not the identity makes that
    whole sample NaN (its mean is).  ValueError on host tensors, other dtypes, and parameters outside gamma > 0, contrast >= 0,
    sigma >= 0, invert in {0, 1} or not finite; there is no CPU implementation."""
    if not torch.is_tensor(images) or not images.is_cuda:
        raise ValueError("grey_variation runs on the HIP device only (unet_grey_vary): move the images to the device first")
    if images.dtype != torch.float32:
        raise ValueError("grey_variation takes float32 images, got %s" % images.dtype)
    if images.dim() not in (2, 3, 4) or (images.dim() == 4 and images.shape[1] != 1) or images.numel() == 0:
        raise ValueError("grey_variation takes images [H,W], [B,H,W] or [B,1,H,W], got %s" % (tuple(images.shape),))
    B = 1 if images.dim() == 2 else images.shape[0]
    rows = _grey_rows(params, B, "grey_variation")
    if out is None:
        out = torch.empty(images.shape, dtype=torch.float32, device=images.device)
    elif (not torch.is_tensor(out) or out.device != images.device or out.dtype != torch.float32 or out.shape != images.shape
          or not out.is_contiguous()):
        raise ValueError("grey_variation: out must be a contiguous float32 tensor of the images' shape on their device")
    if out is images and not images.is_contiguous():
        raise ValueError("grey_variation: in place needs contiguous images")
    mm = None
    if minmax is not None:
        if not torch.is_tensor(minmax) or minmax.device != images.device or minmax.dtype != torch.float32 or tuple(minmax.shape) != (B, 2):
            raise ValueError("grey_variation: minmax must be a float32 [%d,2] tensor on the images' device" % B)
        mm = minmax.contiguous()
    x = images if out is images else images.contiguous()
    _grey_run(x.reshape(B, -1), out.reshape(B, -1), rows, seed, step, first_sample, clip, mm)
    return out


def _grey_of(grey, random_state, B, name):
    """augment's grey argument -> checked [B,5] rows: given, or drawn from random_state by a dict of grey_parameters' ranges"""
    if isinstance(grey, dict):
        if random_state is None:
            raise ValueError("%s(grey={...}) draws the parameters from random_state (a numpy RandomState): pass one, or pass the "
                             "parameters [B,5]" % name)
        _grey_ranges(grey, name)
        grey = grey_parameters(random_state, B, **grey)
    return _grey_rows(grey, B, name)


def _grey_ranges(grey, name):
    unknown = set(grey) - {"gamma", "contrast", "brightness", "noise", "p_invert"}
    if unknown:
        raise ValueError("%s: grey takes the ranges gamma, contrast, brightness, noise and p_invert, got %s" % (name, sorted(unknown)))


def _grid_stage(both, crop, disp, a, levels, grey=None):
    """augment's elastic='grid' stage: both [2B,S,S] = the rotated images, then the rotated masks -> (inp [B,S,S] in [0,1],
    gt [B,crop,crop] int64).  One small upload (the nodes) and the library's two calls; no ATen arithmetic.  grey = (rows [B,5],
    seed, step): unet_grey_vary with the min / max table takes unet_normalise01's place."""
    B, S = both.shape[0] // 2, both.shape[-1]
    dev = both.device
    pad = int((S - crop) / 2)
    d = _grid_tensor(disp, B, dev, "augment")
    inp = torch.empty(B, S, S, dtype=torch.float32, device=dev)
    gt = torch.empty(B, crop, crop, dtype=torch.int64, device=dev)
    mm = torch.empty(B, 2, dtype=torch.float32, device=dev)
    _hip.run("unet_elastic_grid_sample", dev, _hip.ptr(both[:B]), _hip.ptr(both[B:]), B, S, _hip.ptr(d), d.shape[2], float(a),
             int(levels), pad, int(crop), _hip.ptr(inp), _hip.ptr(gt), _hip.ptr(mm))
    if grey is None:
        _hip.run("unet_normalise01", dev, _hip.ptr(inp), B, S * S, _hip.ptr(mm))
    else:
        rows, seed, step = grey
        _grey_run(inp.reshape(B, -1), inp.reshape(B, -1), rows, seed, step, 0, True, mm)
    return inp, gt


def augment(image, target, crop_xy, crop, rot_deg, alpha, sigma, random_state=None, fields=None, levels=255, elastic='field', grid=3,
            disp=None, a=-0.5, grey=None, grey_seed=0, grey_step=0):
    """What ImageDataset.__getitem__ does to one sample after reading it (data.py:97-135), on the device.  The random draws
    stay with the caller (crop origin from the weighted distribution + jitter, rot_deg from np.arange(0,360,30), the elastic
    fields), so the host RNG sequence can follow the reference's:  crop -> reflect pad + rotate + centre crop -> the same
    elastic deformation for image and mask -> mask cropped to the label extent and thresholded at 127 -> image to [0,1].
    image / target: device tensors [H,W] (grey levels / {0,255}); returns (inp [1,S,S] float32, gt [1,crop,crop] int64).
    A whole batch in one call (the DataLoader's collate, vectorised): image / target [B,H,W], crop_xy a list of B origins,
    rot_deg B angles; returns (inp [B,1,S,S], gt [B,1,crop,crop]) - every kernel then runs once for the batch.
    elastic='field' (default) is the reference's deformation, elastic_transform.  elastic='grid' is the paper's (elastic_grid):
    sigma is then the standard deviation in pixels of the displacements of the grid x grid nodes, and alpha and fields are
    ignored.  The node displacements are disp ([B,2,G,G], or [2,G,G] for one sample) or, when disp is None,
    grid_displacements(random_state, B, grid, sigma): random_state must then be given, the device generator is not used.
    After the rotation the grid path is two kernels: unet_elastic_grid_sample (warp of image and mask, rounding, crop and
    threshold of the mask, per-sample min / max) and unet_normalise01.
    grey=None (default) ends there.  grey = parameters [B,5] ([5] for one sample), or a dict of grey_parameters' ranges (e.g.
    {} for its defaults), adds the grey-value variation of grey_variation as the last stage, with seed grey_seed, step
    grey_step and the sample's position in the batch as its sample index.  With a dict the parameters are drawn from
    random_state (required then) after this call's elastic draws.  On the grid path the stage takes unet_normalise01's place
    (unet_grey_vary normalises in the same pass); on the field path it runs after the normalisation."""
    if elastic not in ('field', 'grid'):
        raise ValueError("augment: elastic is 'field' or 'grid', got %r" % (elastic,))
    if elastic == 'grid' and disp is None and random_state is None:
        raise ValueError("augment(elastic='grid') draws the node displacements from random_state (a numpy RandomState): "
                         "pass one, or pass disp")
    if isinstance(grey, dict) and random_state is None:
        raise ValueError("augment(grey={...}) draws the parameters from random_state (a numpy RandomState): pass one, or pass "
                         "the parameters [B,5]")
    batched = image.dim() == 3
    imgs = image if batched else image[None]
    tgts = target if batched else target[None]
    B = imgs.shape[0]
    origins = list(crop_xy) if batched else [crop_xy]
    angles = [float(a) for a in (rot_deg if batched else [rot_deg])]
    if len(origins) != B or len(angles) != B:
        raise ValueError("need one crop origin and one angle per sample")
    img = torch.stack([imgs[b, x0:x0 + crop, y0:y0 + crop] for b, (x0, y0) in enumerate(origins)]).float()
    tgt = torch.stack([tgts[b, x0:x0 + crop, y0:y0 + crop] for b, (x0, y0) in enumerate(origins)]).float()
    _, S, _ = input_size_compute(img)
    both = reflect_rotate_crop(torch.cat((img, tgt)), angles + angles, S, levels=levels)            # [2B,S,S]: images, then masks
    if elastic == 'grid':
        disp = grid_displacements(random_state, B, grid, sigma) if disp is None else disp
        rows = None if grey is None else (_grey_of(grey, random_state, B, "augment"), grey_seed, grey_step)
        inp, gt = _grid_stage(both, crop, disp, a, levels, rows)
        if batched:
            return inp[:, None], gt[:, None]
        return inp[0][None], gt[0][None]
    inp, gt = elastic_transform((both[:B], both[B:]), alpha, sigma, random_state=random_state, fields=fields)
    if levels:
        # the reference warps the uint8 / uint16 arrays it loaded: scipy's map_coordinates writes its result in the input's
        # type, i.e. rounds t + 0.5 down and clamps to the type's range (data.py:245 on the rotated integer images)
        inp = torch.floor(inp + 0.5).clamp_(0, levels)
        gt = torch.floor(gt + 0.5).clamp_(0, levels)
    pad = int((S - crop) / 2)
    gt = (gt[:, pad:crop + pad, pad:crop + pad] > 127).long()
    lo, hi = inp.amin(dim=(1, 2), keepdim=True), inp.amax(dim=(1, 2), keepdim=True)
    inp = (inp - lo) / (hi - lo)
    if grey is not None:
        inp = inp.contiguous()
        _grey_run(inp.reshape(B, -1), inp.reshape(B, -1), _grey_of(grey, random_state, B, "augment"), grey_seed, grey_step, 0, True, None)
    if batched:
        return inp[:, None], gt[:, None]
    return inp[0][None], gt[0][None]


# ---- from instance images to targets and weighted crops (prepare.hip) -----------------------------------------------------

def _reach(kernel, iterations):
    kernel, iterations = int(kernel), int(iterations)
    if kernel < 1 or kernel % 2 == 0 or iterations < 0:
        raise ValueError("preprocess_gt: kernel must be odd and positive, iterations non-negative")
    reach = iterations * (kernel - 1) // 2
    if reach > 8:
        raise ValueError("preprocess_gt: iterations * (kernel - 1) / 2 = %d, the device op reaches 8 pixels at the most" % reach)
    return reach


def _carve(img, name, kernel, iterations, want):
    """unet_carve_borders on img; want = which of (gt, edges, bin) to form.  One read-back: the status words."""
    _device_only(name, "unet_carve_borders", img)
    reach = _reach(kernel, iterations)
    x, code = _int_code(_planes(name, img))
    B, H, W = x.shape
    dev = x.device
    outs = [torch.empty(B, H, W, dtype=dt, device=dev) if w else None
            for w, dt in zip(want, (torch.float32, torch.float32, torch.uint8))]
    status = torch.empty(B, dtype=torch.int64, device=dev)
    _hip.run("unet_carve_borders", dev, _hip.ptr(x), code, B, H, W, reach, _hip.ptr(outs[0]), _hip.ptr(outs[1]), _hip.ptr(outs[2]),
             _hip.ptr(status))
    bad = int(status.sum())
    if bad:
        raise ValueError("%s: %d pixels hold ids outside [0, 2^24)" % (name, bad))
    return [o if o is None or img.dim() == 3 else o[0] for o in outs]


def preprocess_gt(img, kernel=5, iterations=2):
    """The reference's preprocess_gt (data.py:195-221) on a HIP device: img is an instance image [H,W] or a stack [B,H,W], 0 =
    background and any ids in [1, 2^24) on the cells, of any integer dtype or float (a uint16 image born in numpy goes through
    int32).  Every cell is dilated `iterations` times with a kernel x kernel rectangle, and the ring it gained counts 255 in
    mask_global; gt = img - mask_global clipped at 0, so touching cells are carved apart.  Returns (gt, mask_global) of the
    input's shape.  Same name and meaning as the reference; only the float width differs: float32 here, float64 there, and every
    value is an integer below 2^24, which both hold exactly.  The cost does not depend on the number of cells.
    Ids outside [0, 2^24) raise ValueError (one read-back); host tensors raise NotImplementedError (no CPU path)."""
    gt, edges, _ = _carve(img, "preprocess_gt", kernel, iterations, (True, True, False))
    return gt, edges


def binary_target(img, kernel=5, iterations=2):
    """The training target the reference's datasets keep (data.py:63-64, :162-163): preprocess_gt, then
    cv.threshold(gt, 0, 255, THRESH_BINARY).  uint8 {0,255} of img's shape, formed in the same kernel."""
    return _carve(img, "binary_target", kernel, iterations, (False, False, True))[2]


def crop_probabilities(counts, crop):
    """Host half of crop_distribution: counts [..., ny, nx] = foreground pixels per window -> float64 [..., ny * nx], the
    reference's weights (data.py:73-82): x = np.mean(window) / 255 with its two roundings, 0 outside [0.1, 0.9], else
    10 * norm.pdf(x, 0.5, 0.05) written out; each image's row is divided by its sum, or uniform when the sum is 0."""
    c = np.asarray(counts).astype(np.float64)
    c = c.reshape(c.shape[:-2] + (-1,))
    x = ((255.0 * c) / (crop * crop)) / 255
    z = (x - 0.5) / 0.05
    prob = np.where((x < 0.1) | (x > 0.9), 0.0, 10 * (np.exp(-z ** 2 / 2.0) / np.sqrt(2 * np.pi) / 0.05))
    out = np.empty_like(prob)
    for idx in np.ndindex(prob.shape[:-1]):
        row = prob[idx]
        total = np.sum(row)
        out[idx] = np.ones(len(row)) / len(row) if total == 0 else row / total
    return out


def crop_distribution(target, crop, skip=10):
    """The reference's weighted crop distribution (data.py:67-82) of a target [H,W] or [B,H,W] on a HIP device (foreground =
    value != 0, e.g. binary_target's output): returns (pairs, p), pairs the list of window origins (ii, jj) over
    range(0, H - crop, skip) x range(0, W - crop, skip), p float64 numpy [B, len(pairs)] ([1, ...] for a single image), each
    row the distribution of one image.  The window counts are exact integers from the device (unet_crop_counts), read back
    once; the weights are formed from them on the host in float64 (crop_probabilities).  An image no larger than the crop has
    no window: ValueError.  Host tensors raise NotImplementedError (no CPU path)."""
    _device_only("crop_distribution", "unet_crop_counts", target)
    x, code = _int_code(_planes("crop_distribution", target), uint8_ok=True)
    B, H, W = x.shape
    crop, skip = int(crop), int(skip)
    if crop < 1 or skip < 1 or H <= crop or W <= crop:
        raise ValueError("crop_distribution: no window of %d in a %d x %d image with skip %d" % (crop, H, W, skip))
    pairs = [(ii, jj) for ii in range(0, H - crop, skip) for jj in range(0, W - crop, skip)]
    ny, nx = len(range(0, H - crop, skip)), len(range(0, W - crop, skip))
    counts = torch.empty(B, ny, nx, dtype=torch.int32, device=x.device)      # the library's u32 words: at most crop^2 < 2^31
    scratch = _hip.scratch("unet_crop_counts", x.device, B, H, W, crop, skip)
    _hip.run("unet_crop_counts", x.device, _hip.ptr(x), code, B, H, W, crop, skip, _hip.ptr(counts), _hip.ptr(scratch))
    return pairs, crop_probabilities(counts.cpu().numpy(), crop)


def draw_crop(rng, pairs, p_row, shape, crop, skip=10):
    """One crop origin (x, y) as ImageDataset.__getitem__ draws it (data.py:98-103), host only: rng is a
    numpy.random.RandomState (the reference uses the global one) and is consumed in the reference's order: choice over the
    pairs with weights p_row, randint for the row jitter, randint for the column jitter; both are then clamped to
    [0, dim - crop].  The reference draws the angle next: rng.choice(np.arange(0, 360, 30)) (data.py:115)."""
    crop_id = rng.choice(range(len(pairs)), 1, p=p_row)[0]
    x, y = pairs[crop_id]
    x += rng.randint(-skip / 2, (skip / 2) + 1)
    y += rng.randint(-skip / 2, (skip / 2) + 1)
    x = min(max(0, x), shape[0] - crop)
    y = min(max(0, y), shape[1] - crop)
    return int(x), int(y)


class CropDataset:
    """The reference's ImageDataset (data.py:23-137) on arrays that are already read: images [N,H,W] grey levels and instances
    [N,H,W] man_seg instance images (numpy arrays or tensors).  At construction binary_target and crop_distribution run once
    for all N on the device; a [N,H,W] stack has one shape, so `pairs` is built from that shape and applies to every image, as
    the reference builds it from its first image (data.py:67-68).  Iterating yields len(self) batches of batch_size consecutive
    samples (the last may be shorter): per sample the crop origin (draw_crop) and then the angle are drawn from rng in the
    reference's order, and the batch goes through one data.augment call, so each item is (inp [B,1,S,S] float32,
    gt [B,1,crop,crop] int64) on the device - usable as train_loader / val_loader of trainer.training as it is.  The elastic
    fields come from random_state (a numpy RandomState, drawn as the reference's elastic_transform draws them), or from the
    device generator when it is None.  elastic='grid' deforms with the paper's grid x grid displacement grid instead
    (augment(elastic='grid'): sigma is the nodes' standard deviation in pixels, alpha is ignored, random_state is required).
    grey = a dict of grey_parameters' ranges ({} for its defaults) adds the grey-value variation as augment's last stage: each
    batch's parameters are drawn from random_state (required) after that batch's elastic draws - rng's sequence is untouched -
    and its noise is that of (grey_seed, grey_step, position in the batch).  grey_step is a public integer that starts at 0 and
    advances by one per batch; a resumed run sets it.  grey=None (default) is the reference's pipeline."""

    def __init__(self, images, instances, alpha, sigma, crop, batch_size, rng, levels=255, *, random_state=None, skip=10, device=None,
                 elastic='field', grid=3, grey=None, grey_seed=0):
        if elastic not in ('field', 'grid'):
            raise ValueError("CropDataset: elastic is 'field' or 'grid', got %r" % (elastic,))
        if elastic == 'grid' and random_state is None:
            raise ValueError("CropDataset(elastic='grid') draws the node displacements from random_state (a numpy RandomState)")
        if elastic == 'grid' and int(grid) < 2:
            raise ValueError("CropDataset: a grid of %d nodes per side, need at least 2" % int(grid))
        if grey is not None:
            if not isinstance(grey, dict):
                raise ValueError("CropDataset: grey is None or a dict of grey_parameters' ranges, got %r" % (grey,))
            if random_state is None:
                raise ValueError("CropDataset(grey={...}) draws the parameters from random_state (a numpy RandomState)")
            _grey_ranges(grey, "CropDataset")
        self.elastic, self.grid = elastic, int(grid)
        self.grey, self.grey_seed, self.grey_step = grey, int(grey_seed), 0
        if device is None:
            device = images.device if torch.is_tensor(images) and images.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        as_tensor = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(self.device)
        self.image = as_tensor(images).float()
        inst = as_tensor(instances)
        if self.image.dim() != 3 or inst.shape != self.image.shape:
            raise ValueError("CropDataset takes images and instances of one shape [N,H,W], got %s and %s"
                             % (tuple(self.image.shape), tuple(inst.shape)))
        self.alpha, self.sigma, self.crop, self.skip, self.levels = alpha, sigma, int(crop), int(skip), levels
        self.batch_size = int(batch_size)
        self.rng, self.random_state = rng, random_state
        self.target = binary_target(inst)
        self.pairs, self.target_weighted_crop_distribution = crop_distribution(self.target, self.crop, self.skip)

    def __len__(self):
        return -(-self.image.shape[0] // self.batch_size)

    def draw(self, idx):
        """(crop origin, angle) of sample idx, consuming rng as the reference's __getitem__ does"""
        xy = draw_crop(self.rng, self.pairs, self.target_weighted_crop_distribution[idx], self.image.shape[1:], self.crop, self.skip)
        return xy, self.rng.choice(np.arange(0, 360, 30))

    def __iter__(self):
        N = self.image.shape[0]
        for lo in range(0, N, self.batch_size):
            idx = list(range(lo, min(N, lo + self.batch_size)))
            draws = [self.draw(i) for i in idx]
            step = self.grey_step
            if self.grey is not None:
                self.grey_step += 1
            yield augment(self.image[idx], self.target[idx], [d[0] for d in draws], self.crop, [d[1] for d in draws], self.alpha,
                          self.sigma, random_state=self.random_state, levels=self.levels, elastic=self.elastic, grid=self.grid,
                          grey=self.grey, grey_seed=self.grey_seed, grey_step=step)
