"""PanoSwin's panorama training augmentation on the device: PanoStretch, RollAug, RandomFlip, AutoAugment / Resize, Normalize and Pad.

The reference runs these in its CPU data pipeline (configs/swin/faster_rcnn_panoswin_tiny_patch4_window7_mstrain_480800_adamw_1x_
streetwin.py:62-91; PanoStretch and RollAug at mmdet/datasets/pipelines/transforms.py:992-1068, which call
lzx/yolo/extensions/xzaug.py getAug / _xzaug, rollaug.py roll_aug_raw and padding2.py merge_adjbox).  Here the pixels go through two
launches of HIP kernels (csrc/pswin_pano.hip) and the boxes stay on the host in numpy, with the reference's dtypes, order and rounding.

Image contract: the warp (stretch, roll, flip) is byte-identical to the reference.  For output pixel (x, y) of an H x W image
(W even: sin u = 0 at x = (W-1)/2 otherwise) the stretch samples the source at (refy, refx), in float64 and in this order:

    u  = ((x+0.5)/W - 0.5)*2*pi            v  = ((y+0.5)/H - 0.5)*pi
    u0 = atan2(sin u * kx / ky, cos u)     v0 = atan(tan v * sin u0 / sin u * ky)
    refx = (u0/(2*pi) + 0.5)*W - 0.5       refy = (v0/pi + 0.5)*H - 0.5

Quirks that are part of the contract:
  * scipy's map_coordinates(order=1, mode='wrap') is not a periodic wrap: the period is n-1 and the first and last samples coincide,
    along both axes.  Wherever refy < 0 the top row blends rows H-2 and H-1; wherever refx < 0 column 0 blends columns W-2 and W-1.
    The weights are w0 = 1 - t and w1 = 1 - w0, the taps accumulate row-major as (value * wy) * wx, and the sum is rounded half-up
    and clamped to uint8 (1.5 -> 2, 2.5 -> 3).
  * with kx == ky the columns 0 and W-1 sit on that seam (refx = 0 or W-1 up to the last bit of atan2), so which side of the seam
    they sample depends on how the platform's atan2 rounds; random draws never give kx == ky.
  * a stretch that is not drawn copies the image; roll_dist = (int(r*100000) % 100000) / 100000, shift = int(roll_dist*W),
    out[:, x] = in[:, (x - shift) mod W] (np.roll); the flip is out[:, x] = in[:, W-1-x] (mmcv.imflip, horizontal).

Boxes (transform_boxes), in the reference's order and precision:
  1. PanoStretch: both corners through the inverse map u' = atan2(sin u0 * ky/kx, cos u0), v' = atan(tan v0 * sin u' / sin u0 / ky),
     then np.round.  A corner at x = W wraps: at W = 128, kx = 1.7, ky = 0.6 the box [100, 20, 128, 40] gets x2 = -0.32 before
     rounding.  Labels pass through float64 and are rounded back to int64.
  2. RollAug: normalise by (W, H), add roll_dist to x1 and x2; a box with x2 > 1 whose centre is past 1 moves back by 1 (with clip01
     x1 is clamped at 0), otherwise, with clip01, x2 = 1.  Then merge_adjbox: every box with x1 == roll_dist is paired with every box
     with x2 == roll_dist (eps 1e-9), a cross product; the merged row is the second box's row (label and y included) with x2 of the
     first, and that row is modified in place, so a row merged twice shows the last partner's x2 everywhere it was emitted.
     Un-normalise, np.round.
  3. RandomFlip: x1' = W - x2, x2' = W - x1.
A batch image without boxes stays without boxes (the reference's RollAug raises on an empty box array).

Random draws per image, in the reference's order: rand() < stretch_chance, uniform(1, kxy[0]), uniform(1, kxy[1]), rand() < 0.5
(kx = 1/kx), rand() < 0.5 (ky = 1/ky); rand() < roll_chance, rand() for roll_dist; choice(['horizontal', None], p=[r, 1-r]);
PanoTrainTransform then draws the Resize scale with randint(len(img_scales)).  Seeded, one image after the other, this reproduces
the reference pipeline for a recipe without AutoAugment.

Resize, Normalize, Pad (pswin_pano_resize_normalize_pad): mmdet Resize(keep_ratio=True) with one scale per image
(sf = min(max(scale)/max(h, w), min(scale)/min(h, w)), new size int(w*sf + 0.5) x int(h*sf + 0.5), boxes times (new_w/w, new_h/h)
in float32 and clipped); the pixels are resampled bilinearly with the geometry of cv2 INTER_LINEAR (src = (dst+0.5)*(in/out) - 0.5,
border replicated) in float32 and rounded half-up.  This is NOT bit-exact to cv2, which rounds with fixed-point weights: the resized
uint8 image may differ from mmcv.imresize by 1 LSB.  Normalize is mmcv.imnormalize: BGR -> RGB, then (v - mean) * (1/std) in float32
(mean and 1/std rounded to float32 first, as cv2 does with the scalar).  Pad writes zeros up to a multiple of size_divisor and to
the largest image of the batch (mmdet Pad followed by collate).

AutoAugment (PanoTrainTransform(auto_augment=STREETWIN_AUTO_AUGMENT); the streetwin config, lines 65-89, wraps its Resize in it): per
image np.random.choice over the two policies, which consumes the stream like randint(0, 2).  Policy 0 is the Resize above.  Policy 1 is
Resize(first scales) -> RandomCrop('absolute_range', (384, 600), allow_negative_crop=True) -> Resize(train scales, override=True); its
draws, in order: randint(len(first scales)); crop_h = randint(min(h1, 384), min(h1, 600) + 1); crop_w from the SAME height-based
range (transforms.py:948-950 passes h for both); offset_h = randint(0, max(h1 - crop_h, 0) + 1); offset_w likewise;
randint(len(train scales)).  The crop taken is min(crop, dim) per axis (numpy slicing truncates).  A Resize with one scale draws
nothing.  Pixels: pswin_pano_resize_crop_resize_normalize_pad does both resizes and the crop in one launch (the intermediate uint8
image is never stored), so the uint8 stages may differ from cv2 by 1 LSB twice.  Boxes: resize_boxes -> crop_boxes (float32 subtract,
clip to the crop, keep x2 > x1 and y2 > y1; an empty result is valid) -> resize_boxes on the crop's size.  pano_ratio_v is
[y1 / h1, y2 / h1] of the crop (transforms.py:874, PanoCheck 1128-1132), [0.0, 1.0] without one.

Row provenance (row_map= of transform_one, transform_boxes, crop_boxes, auto_augment_boxes): boxes change rows on the way, and whatever
is attached to a box (its instance mask) must follow.  A map is int32 [n_out, 2]: the input rows output row r came from, the second
entry -1 where there is one source.  An unpaired row maps to itself.  A row the seam merge emits maps to (j, left[-1]): j the right row that
is emitted, left[-1] the last left partner in _roll_rows' iteration order, the row whose x2 the emitted row shows.  crop_boxes selects
the rows of the map it is given; auto_augment_boxes(row_map=transform_one's map) returns the composition, which is what
pswin_pano_masks takes.

Instance masks (transform_masks_one is the definition, warp_resize_masks the launch, PanoTrainTransform.with_targets the entry): every
Mask R-CNN config of the reference sends gt_masks (BitmapMasks) through RandomFlip -> AutoAugment -> Pad; there Resize is
mmcv.imrescale / imresize(interpolation='nearest') per bitmap, RandomCrop a slice, Pad zeros.  Here one launch writes
PaddedTargets.masks: output pixel (y, x) of row r shows pixel (sy, sx) of the warped source planes of the row map, with
nn(d, n_in, n_out) = min(int(floor(d * (1 / (n_out / n_in)))), n_in - 1) in float64 along each axis -- the index rule of
cv2.resize(INTER_NEAREST) -- chained through resize, crop offset and resize.  PARITY: unpinned -- neither cv2 nor mmcv is installed
next to this project or shipped in the reference tree, so the rule is stated from cv2's source, not compared with it; the fixture
tests/golden/pano_masks.npz pins order, row keeping, crop arithmetic and sizes to the reference, with this rule standing in for
mmcv's resampling.  PanoStretch and RollAug have NO mask path in the reference.  The project's choice: the mask goes where the image
goes, by the same expression -- the 0 / 1 plane `mask != 0` through the image's warp as a one-channel image (float64 coordinates, the
wrap quirk, the taps, half-up rounding, then roll, then flip).  On a 0 / 1 plane that rounding is "blend + 0.5 >= 1", so the result is
again 0 / 1, and pano_warp on a [n, H, W, 1] batch states the same planes independently.  A merged seam pair shows the OR of its two
pieces.
"""
import numpy as np
import torch

from . import _lib
from ._lib import PswinError

STRETCH, FLIP = 1, 2

# streetwin config (configs/swin/faster_rcnn_panoswin_tiny_patch4_window7_mstrain_480800_adamw_1x_streetwin.py:47-58)
TRAIN_RESIZE_SCALES = [(480, 1333), (512, 1333), (544, 1333), (576, 1333), (608, 1333), (640, 1333), (672, 1333), (704, 1333),
                       (736, 1333), (768, 1333), (800, 1333)]
IMG_NORM_MEAN = (123.675, 116.28, 103.53)
IMG_NORM_STD = (58.395, 57.12, 57.375)
# the second policy of that config's AutoAugment (lines 56, 74-88); the first policy and the last Resize use TRAIN_RESIZE_SCALES
STREETWIN_AUTO_AUGMENT = dict(first_scales=[(400, 1333), (500, 1333), (600, 1333)], crop_size=(384, 600), crop_type="absolute_range")
PLAN_KEYS = ("h1", "w1", "cy", "cx", "ch", "cw", "oh", "ow")


# ------------------------------------------------------------------------------------------------------------------------------
# random draws
# ------------------------------------------------------------------------------------------------------------------------------

def draw_pano_params(batch, W, kxy=(2., 2.), stretch_chance=1., roll_chance=1., flip_ratio=.5, rng=np.random):
    """Draw PanoStretch, RollAug and RandomFlip parameters for `batch` images of width W, image after image, in the reference's order.

    Returns a dict of host arrays of length `batch`: stretch (bool), kx, ky (float64, 1 when not stretched), roll (bool), roll_dist
    (float64, 0 when not rolled), shift (int64), flip (bool).  rng: np.random or a np.random.RandomState."""
    p = dict(stretch=np.zeros(batch, bool), kx=np.ones(batch), ky=np.ones(batch), roll=np.zeros(batch, bool),
             roll_dist=np.zeros(batch), shift=np.zeros(batch, np.int64), flip=np.zeros(batch, bool))
    for i in range(batch):
        if rng.rand() < stretch_chance:
            kx = rng.uniform(1.0, kxy[0])
            ky = rng.uniform(1.0, kxy[1])
            if rng.rand() < 0.5:
                kx = 1.0 / kx
            if rng.rand() < 0.5:
                ky = 1.0 / ky
            p["stretch"][i], p["kx"][i], p["ky"][i] = True, kx, ky
        if rng.rand() < roll_chance:
            roll_dist = (int(rng.rand() * 100000) % 100000) / 100000
            p["roll"][i], p["roll_dist"][i], p["shift"][i] = True, roll_dist, int(roll_dist * W)
        if flip_ratio is not None:
            p["flip"][i] = rng.choice(2, p=[flip_ratio, 1 - flip_ratio]) == 0
    return p


def draw_auto_augment(h, w, cfg, rng=np.random, img_scales=TRAIN_RESIZE_SCALES):
    """One h x w image's AutoAugment policy and plan, with the reference's draws in the reference's order (module docstring).

    cfg: STREETWIN_AUTO_AUGMENT or a dict of the same keys.  Returns a dict: policy (0 or 1), scale_idx and scale (the final Resize),
    plan (h1, w1, cy, cx, ch, cw, oh, ow; all zero but oh, ow for policy 0), draws (every integer drawn, in order), crop ((y1, x1, y2,
    x2) or None), pano_ratio_v, pano_lr_noadj (None without a crop: the reference leaves the key out), and for policy 1 first_idx,
    first_scale, h1, w1, crop_h, crop_w (as drawn), offset_h, offset_w, ch, cw (as taken)."""
    if cfg.get("crop_type", "absolute_range") != "absolute_range":
        raise PswinError(f"draw_auto_augment: only crop_type 'absolute_range' is implemented, got {cfg.get('crop_type')!r}")
    lo, hi = cfg["crop_size"]
    if not (isinstance(lo, int) and isinstance(hi, int) and 0 < lo <= hi):
        raise PswinError(f"draw_auto_augment: crop_size must be two positive ints (low, high), got {cfg['crop_size']}")
    policy = int(rng.randint(0, 2))
    draws = [policy]

    def pick(scales):
        if len(scales) > 1:
            draws.append(int(rng.randint(len(scales))))
            return draws[-1], tuple(scales[draws[-1]])
        return 0, tuple(scales[0])                                           # mmdet's Resize draws nothing for one scale

    if policy == 0:
        i, scale = pick(img_scales)
        oh, ow = rescale_size(h, w, scale)
        return dict(policy=0, scale_idx=i, scale=scale, plan=(0, 0, 0, 0, 0, 0, oh, ow), draws=draws, crop=None,
                    pano_ratio_v=[0.0, 1.0], pano_lr_noadj=None)
    fi, fscale = pick(cfg["first_scales"])
    h1, w1 = rescale_size(h, w, fscale)
    crop_h = int(rng.randint(min(h1, lo), min(h1, hi) + 1))
    crop_w = int(rng.randint(min(h1, lo), min(h1, hi) + 1))                  # the height's range: the reference's quirk
    offset_h = int(rng.randint(0, max(h1 - crop_h, 0) + 1))
    offset_w = int(rng.randint(0, max(w1 - crop_w, 0) + 1))
    draws += [crop_h, crop_w, offset_h, offset_w]
    i, scale = pick(img_scales)
    ch, cw = min(crop_h, h1 - offset_h), min(crop_w, w1 - offset_w)
    oh, ow = rescale_size(ch, cw, scale)
    return dict(policy=1, scale_idx=i, scale=scale, plan=(h1, w1, offset_h, offset_w, ch, cw, oh, ow), draws=draws,
                first_idx=fi, first_scale=fscale, h1=h1, w1=w1, crop_h=crop_h, crop_w=crop_w, offset_h=offset_h,
                offset_w=offset_w, ch=ch, cw=cw, crop=(offset_h, offset_w, offset_h + ch, offset_w + cw),
                pano_ratio_v=[offset_h / h1, (offset_h + crop_h) / h1], pano_lr_noadj=cw == w1)


def make_pano_params(stretch, kx, ky, roll_dist, flip, W):
    """Parameters of one or more images from explicit values (roll_dist None: no roll), in the layout draw_pano_params returns."""
    stretch, kx, ky, flip = (np.atleast_1d(np.asarray(a)) for a in (stretch, kx, ky, flip))
    n = len(stretch)
    rd = [None] * n if roll_dist is None else list(np.atleast_1d(np.asarray(roll_dist, dtype=object)))
    roll = np.array([r is not None for r in rd])
    dist = np.array([0.0 if r is None else (int(float(r) * 100000) % 100000) / 100000 for r in rd])
    return dict(stretch=stretch.astype(bool), kx=np.where(stretch, kx, 1.0).astype(np.float64),
                ky=np.where(stretch, ky, 1.0).astype(np.float64), roll=roll, roll_dist=dist,
                shift=np.array([int(d * W) for d in dist], np.int64), flip=flip.astype(bool))


def params_array(params):
    """Host float64 [B, 4] (kx, ky, shift, flags) of pswin_pano_warp_u8."""
    flags = params["stretch"].astype(np.int64) * STRETCH + params["flip"].astype(np.int64) * FLIP
    return np.stack([params["kx"], params["ky"], params["shift"].astype(np.float64), flags.astype(np.float64)], 1)


def params_tensor(params, device):
    return torch.from_numpy(params_array(params)).to(device=device, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------------------------------------

def _check_images(imgs, what, channels=None):
    if not isinstance(imgs, torch.Tensor) or not imgs.is_cuda:
        raise PswinError(f"{what}: the PanoSwin kernels run on an MI355X (HIP) device only; got a CPU tensor")
    if imgs.dtype != torch.uint8 or imgs.dim() != 4:
        raise PswinError(f"{what}: expected uint8 [B, H, W, C] images, got {imgs.dtype} {tuple(imgs.shape)}")
    if channels is not None and imgs.shape[3] not in channels:
        raise PswinError(f"{what}: expected {channels} channels, got {imgs.shape[3]}")


def _overlaps(a, b):
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _check_buffer(t, what, name, dtype, shape, device, inputs=()):
    """A caller-supplied buffer the kernel writes (or reads) by raw pointer: it must be exactly what the launch assumes."""
    if not isinstance(t, torch.Tensor) or t.device != device or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}, contiguous={t.is_contiguous()}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise PswinError(f"{what}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}; got {got}")
    for other in inputs:
        if _overlaps(t, other):
            raise PswinError(f"{what}: {name} must not overlap an input of the launch")


def pano_warp(imgs_u8, params, out=None):
    """Stretch, roll and flip a batch of uint8 [B, H, W, C] panoramas on the device in one pass.

    params: the dict of draw_pano_params / make_pano_params, or a device float64 [B, 4] tensor (kx, ky, shift, flags) -- the form a
    captured graph replays after new values are copied into it."""
    _check_images(imgs_u8, "pano_warp", (1, 2, 3, 4))
    B, H, W, C = imgs_u8.shape
    if W % 2:
        raise PswinError(f"pano_warp: the width must be even (sin u = 0 at x = (W-1)/2), got {W}")
    if H < 2:
        raise PswinError(f"pano_warp: the height must be at least 2, got {H}")
    if isinstance(params, dict):
        params = params_tensor(params, imgs_u8.device)
    if params.dtype != torch.float64 or tuple(params.shape) != (B, 4) or params.device != imgs_u8.device or not params.is_contiguous():
        raise PswinError("pano_warp: params must be a contiguous float64 [B, 4] tensor on the images' device")
    x = imgs_u8.contiguous()
    if out is None:
        out = torch.empty_like(x)
    else:
        _check_buffer(out, "pano_warp", "out", torch.uint8, (B, H, W, C), x.device, (x, params))
    _lib.call("pswin_pano_warp_u8", x, _lib.ptr(x), _lib.ptr(params), _lib.ptr(out), B, H, W, C, algo_bytes=2 * x.numel())
    return out


def norm_tensor(mean, std, device):
    """f32 [6] (mean, 1/std) per output channel: both rounded to float32 as cv2 rounds the scalars of mmcv.imnormalize."""
    mean = np.asarray(mean, np.float64).reshape(3)
    inv = 1.0 / np.asarray(std, np.float64).reshape(3)
    return torch.tensor(np.concatenate([mean, inv]).astype(np.float32), device=device)


def padded_size(sizes, size_divisor):
    d = max(1, int(size_divisor or 1))
    return (-(-max(h for h, _ in sizes) // d) * d, -(-max(w for _, w in sizes) // d) * d)


def resize_normalize_pad(imgs_u8, out_hw, mean=IMG_NORM_MEAN, std=IMG_NORM_STD, to_rgb=True, size_divisor=32, pad_hw=None, out=None,
                         norm=None):
    """Resize every uint8 [H, W, 3] image of the batch to its own out_hw[b] = (h, w), normalise and zero-pad into float32
    [B, 3, Hp, Wp].  out_hw: host list of (h, w), or a device int32 [B, 2] tensor (then pad_hw = (Hp, Wp) must be given: the
    padded size fixes the launch).  Hp, Wp default to the batch maximum rounded up to size_divisor."""
    _check_images(imgs_u8, "resize_normalize_pad", (3,))
    B, H, W, _ = imgs_u8.shape
    dev = imgs_u8.device
    if isinstance(out_hw, torch.Tensor):
        if pad_hw is None:
            raise PswinError("resize_normalize_pad: pass pad_hw with a device out_hw tensor")
        if out_hw.dtype != torch.int32 or tuple(out_hw.shape) != (B, 2) or out_hw.device != dev or not out_hw.is_contiguous():
            raise PswinError("resize_normalize_pad: out_hw must be a contiguous int32 [B, 2] tensor on the images' device")
        hw_t = out_hw
    else:
        sizes = [(int(h), int(w)) for h, w in out_hw]
        if len(sizes) != B or min(min(s) for s in sizes) < 1:
            raise PswinError(f"resize_normalize_pad: need {B} positive output sizes, got {sizes}")
        if pad_hw is None:
            pad_hw = padded_size(sizes, size_divisor)
        if any(h > pad_hw[0] or w > pad_hw[1] for h, w in sizes):
            raise PswinError(f"resize_normalize_pad: an output size exceeds the padded size {pad_hw}")
        hw_t = torch.tensor(sizes, dtype=torch.int32, device=dev)
    Hp, Wp = int(pad_hw[0]), int(pad_hw[1])
    if Hp < 1 or Wp < 1:
        raise PswinError(f"resize_normalize_pad: the padded size must be positive, got {pad_hw}")
    if norm is None:
        norm = norm_tensor(mean, std, dev)
    else:
        _check_buffer(norm, "resize_normalize_pad", "norm", torch.float32, (6,), dev)
    x = imgs_u8.contiguous()
    if out is None:
        out = torch.empty(B, 3, Hp, Wp, device=dev, dtype=torch.float32)
    else:
        _check_buffer(out, "resize_normalize_pad", "out", torch.float32, (B, 3, Hp, Wp), dev, (x, hw_t, norm))
    _lib.call("pswin_pano_resize_normalize_pad", x, _lib.ptr(x), _lib.ptr(hw_t), _lib.ptr(norm), int(bool(to_rgb)), _lib.ptr(out), B, H,
              W, Hp, Wp, algo_bytes=x.numel() + out.numel() * 4)
    return out


def _host_plan(plan, B, what):
    """Host plan (one dict of PLAN_KEYS or one 8-tuple per image) -> validated list of 8-tuples."""
    rows = []
    for p in plan:
        try:
            rows.append(tuple(int(p[k]) for k in PLAN_KEYS) if isinstance(p, dict) else tuple(int(v) for v in p))
        except (KeyError, TypeError, ValueError) as e:
            raise PswinError(f"{what}: a plan row is a dict of {PLAN_KEYS} or a tuple of those 8 integers; got {p!r}") from e
    if len(rows) != B or any(len(r) != 8 for r in rows):
        raise PswinError(f"{what}: need {B} plan rows of 8 integers, got {rows}")
    for h1, w1, cy, cx, ch, cw, oh, ow in rows:
        if oh < 1 or ow < 1:
            raise PswinError(f"{what}: the output size must be positive, got {(oh, ow)}")
        if h1 == 0:
            continue
        if h1 < 0 or w1 < 1 or ch < 1 or cw < 1:
            raise PswinError(f"{what}: the intermediate size and the crop size must be positive, got {(h1, w1)} and {(ch, cw)}")
        if cy < 0 or cx < 0 or cy + ch > h1 or cx + cw > w1:
            raise PswinError(f"{what}: the crop {ch}x{cw} at ({cy}, {cx}) leaves the intermediate image {h1}x{w1}")
    return rows


def resize_crop_resize_normalize_pad(imgs_u8, plan, mean=IMG_NORM_MEAN, std=IMG_NORM_STD, to_rgb=True, size_divisor=32, pad_hw=None,
                                     out=None, norm=None):
    """resize_normalize_pad with a per-image plan in place of out_hw: (h1, w1, cy, cx, ch, cw, oh, ow).  h1 == 0 resizes the image to
    oh x ow; h1 > 0 resizes it to h1 x w1 (uint8), crops [cy:cy+ch, cx:cx+cw] and resizes the crop to oh x ow -- in one launch, the
    intermediate image is never stored.  plan: host list of dicts (PLAN_KEYS) or 8-tuples, validated here, or a device int32 [B, 8]
    tensor, clamped on the device (then pad_hw must be given).  The other arguments: as resize_normalize_pad."""
    what = "resize_crop_resize_normalize_pad"
    _check_images(imgs_u8, what, (3,))
    B, H, W, _ = imgs_u8.shape
    dev = imgs_u8.device
    if isinstance(plan, torch.Tensor):
        if pad_hw is None:
            raise PswinError(f"{what}: pass pad_hw with a device plan tensor")
        if plan.dtype != torch.int32 or tuple(plan.shape) != (B, 8) or plan.device != dev or not plan.is_contiguous():
            raise PswinError(f"{what}: plan must be a contiguous int32 [B, 8] tensor on the images' device")
        plan_t = plan
    else:
        rows = _host_plan(plan, B, what)
        sizes = [(r[6], r[7]) for r in rows]
        if pad_hw is None:
            pad_hw = padded_size(sizes, size_divisor)
        if any(h > pad_hw[0] or w > pad_hw[1] for h, w in sizes):
            raise PswinError(f"{what}: an output size exceeds the padded size {tuple(pad_hw)}")
        plan_t = torch.tensor(rows, dtype=torch.int32, device=dev)
    Hp, Wp = int(pad_hw[0]), int(pad_hw[1])
    if Hp < 1 or Wp < 1:
        raise PswinError(f"{what}: the padded size must be positive, got {pad_hw}")
    if norm is None:
        norm = norm_tensor(mean, std, dev)
    else:
        _check_buffer(norm, what, "norm", torch.float32, (6,), dev)
    x = imgs_u8.contiguous()
    if out is None:
        out = torch.empty(B, 3, Hp, Wp, device=dev, dtype=torch.float32)
    else:
        _check_buffer(out, what, "out", torch.float32, (B, 3, Hp, Wp), dev, (x, plan_t, norm))
    _lib.call("pswin_pano_resize_crop_resize_normalize_pad", x, _lib.ptr(x), _lib.ptr(plan_t), _lib.ptr(norm), int(bool(to_rgb)),
              _lib.ptr(out), B, H, W, Hp, Wp, algo_bytes=x.numel() + out.numel() * 4)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# boxes (host, numpy)
# ------------------------------------------------------------------------------------------------------------------------------

def _stretch_corners(pts, H, W, kx, ky):
    u0 = ((pts[:, 0] + 0.5) / W - 0.5) * 2 * np.pi
    v0 = ((pts[:, 1] + 0.5) / H - 0.5) * np.pi
    u = np.arctan2(np.sin(u0) * ky / kx, np.cos(u0))
    v = np.arctan(np.tan(v0) * np.sin(u) / np.sin(u0) / ky)
    return np.stack([(u / (2 * np.pi) + 0.5) * W - 0.5, (v / np.pi + 0.5) * H - 0.5], axis=-1)


def _identity_map(n):
    return np.stack([np.arange(n, dtype=np.int32), np.full(n, -1, np.int32)], 1)


def _roll_rows(rows, roll_dist, clip01, eps=1e-9, row_map=False):
    """rows: float64 [n, 5] (label, x1, y1, x2, y2) normalised.  Shifts x by roll_dist, applies the wrap rule and the seam merge of
    the module docstring (RollAug step 2) and returns the new rows; `rows` is modified.  row_map=True: also the int32 [n_out, 2]
    provenance of the returned rows (module docstring, "Row provenance")."""
    x1, x2 = rows[:, 1], rows[:, 3]
    x1 += roll_dist
    x2 += roll_dist
    # wrap rule, per box: past the seam with its centre -> back by one period; past it with the centre inside -> cut (clip01)
    past = x2 > 1.0
    back = past & ((x2 + x1) / 2 > 1.0)
    x2[back] -= 1.0
    x1[back] = np.maximum(x1[back] - 1.0, 0.0) if clip01 else x1[back] - 1.0
    if clip01:
        x2[past & ~back] = 1.0
    # seam merge.  Left pieces start at roll_dist, right pieces end there.  Every (left, right) pair is visited in the order of
    # Python's set iteration over the indices (the reference collects them in sets); the right row takes the left row's x2 in
    # place, so a right row paired several times ends with its last partner's x2, and every emitted copy shows that final state.
    left = list(set(np.flatnonzero(np.abs(x1 - roll_dist) < eps).tolist()))
    right = list(set(np.flatnonzero(np.abs(x2 - roll_dist) < eps).tolist()))
    if not left or not right:
        return (rows.copy(), _identity_map(len(rows))) if row_map else rows.copy()
    emitted = []
    for i in left:
        for j in right:
            rows[j, 3] = rows[i, 3]
            emitted.append(j)
    n_merged = len(emitted)
    paired = set(left) | set(right)
    emitted += [i for i in range(len(rows)) if i not in paired]
    if not row_map:
        return rows[emitted]
    prov = np.array([[j, left[-1] if k < n_merged else -1] for k, j in enumerate(emitted)], np.int32).reshape(-1, 2)
    return rows[emitted], prov


def transform_one(boxes, labels, H, W, stretch, kx, ky, roll, roll_dist, flip, clip01=True, row_map=False):
    """One image's boxes (float32 [n, 4] x1 y1 x2 y2 pixels) and labels (int64 [n]) through PanoStretch, RollAug and RandomFlip.
    row_map=True: a third result, the int32 [n_out, 2] provenance of the returned rows."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    labels = np.asarray(labels, np.int64).reshape(-1)
    if len(boxes) != len(labels):
        raise PswinError(f"transform_boxes: {len(boxes)} boxes but {len(labels)} labels")
    prov = _identity_map(len(boxes))
    if len(boxes) == 0:
        return (boxes.copy(), labels.copy(), prov) if row_map else (boxes.copy(), labels.copy())
    if stretch:
        rows = np.concatenate([labels[:, None], boxes], 1)                       # float64, as the reference's concatenate
        pts = _stretch_corners(rows[:, 1:].copy().reshape(-1, 2), H, W, kx, ky).reshape(-1, 4)
        labels = np.round(rows[:, 0]).astype(np.int64)
        boxes = np.round(pts).astype(np.float32)
    if roll:
        xyxy = boxes.astype(np.float64)
        xyxy[:, [0, 2]] /= W
        xyxy[:, [1, 3]] /= H
        rows, prov = _roll_rows(np.concatenate([labels[:, None], xyxy], 1), roll_dist, clip01, row_map=True)
        labels = np.round(rows[:, 0]).astype(np.int64)
        xyxy = rows[:, 1:]
        xyxy[:, [0, 2]] *= W
        xyxy[:, [1, 3]] *= H
        boxes = np.round(xyxy).astype(np.float32)
    if flip:
        f = boxes.copy()
        f[:, 0] = W - boxes[:, 2]
        f[:, 2] = W - boxes[:, 0]
        boxes = f
    return (boxes, labels, prov) if row_map else (boxes, labels)


def transform_boxes(boxes, labels, H, W, params, clip01=True, row_map=False):
    """Lists of per-image boxes and labels through PanoStretch, RollAug and RandomFlip with the drawn `params`.  row_map=True: a third
    list, the row provenance of every image."""
    if len(boxes) != len(params["stretch"]) or len(labels) != len(boxes):
        raise PswinError("transform_boxes: one boxes and one labels array per image of params")
    out_b, out_l, out_m = [], [], []
    for i in range(len(boxes)):
        b, l, m = transform_one(boxes[i], labels[i], H, W, params["stretch"][i], params["kx"][i], params["ky"][i], params["roll"][i],
                                params["roll_dist"][i], params["flip"][i], clip01, row_map=True)
        out_b.append(b)
        out_l.append(l)
        out_m.append(m)
    return (out_b, out_l, out_m) if row_map else (out_b, out_l)


def rescale_size(h, w, scale):
    """(new_h, new_w) of mmcv.rescale_size((w, h), scale) for a (long, short) or (short, long) scale tuple."""
    sf = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return int(h * float(sf) + 0.5), int(w * float(sf) + 0.5)


def resize_boxes(boxes, h, w, new_h, new_w):
    """mmdet Resize._resize_bboxes: float32 boxes times (new_w/w, new_h/h), clipped to the new image."""
    sf = np.array([new_w / w, new_h / h, new_w / w, new_h / h], dtype=np.float32)
    b = np.asarray(boxes, np.float32).reshape(-1, 4) * sf
    b[:, 0::2] = np.clip(b[:, 0::2], 0, new_w)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, new_h)
    return b


def crop_boxes(boxes, labels, offset_w, offset_h, crop_h, crop_w, row_map=None):
    """mmdet RandomCrop._crop_data on the boxes (transforms.py:881-900): subtract the offset in float32, clip to the crop, keep the
    boxes with x2 > x1 and y2 > y1 and their labels.  crop_h, crop_w: the crop as taken.  An empty result is valid.  row_map (the
    int32 [n, 2] provenance of `boxes`, or True for the identity): a third result, the provenance of the rows kept."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4) - np.array([offset_w, offset_h, offset_w, offset_h], dtype=np.float32)
    labels = np.asarray(labels, np.int64).reshape(-1)
    if len(b) != len(labels):
        raise PswinError(f"crop_boxes: {len(b)} boxes but {len(labels)} labels")
    b[:, 0::2] = np.clip(b[:, 0::2], 0, crop_w)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, crop_h)
    keep = (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])
    if row_map is None:
        return b[keep, :], labels[keep]
    return b[keep, :], labels[keep], _as_row_map(row_map, len(b), "crop_boxes")[keep]


def _as_row_map(row_map, n, what):
    if row_map is True:
        return _identity_map(n)
    m = np.asarray(row_map, np.int32).reshape(-1, 2)
    if len(m) != n:
        raise PswinError(f"{what}: the row map has {len(m)} rows for {n} boxes")
    return m


def auto_augment_boxes(boxes, labels, h, w, aa, row_map=None):
    """One image's boxes and labels through the policy that draw_auto_augment returned for its h x w image.  row_map (the provenance
    of `boxes`, e.g. transform_one's, or True for the identity): a third result, the composed provenance of the returned rows -- what
    pswin_pano_masks takes."""
    h1, w1, cy, cx, ch, cw, oh, ow = aa["plan"]
    if aa["policy"] == 0:
        b, l = resize_boxes(boxes, h, w, oh, ow), np.asarray(labels, np.int64).reshape(-1)
        return (b, l) if row_map is None else (b, l, _as_row_map(row_map, len(b), "auto_augment_boxes").copy())
    if row_map is None:
        b, l = crop_boxes(resize_boxes(boxes, h, w, h1, w1), labels, cx, cy, ch, cw)
        return resize_boxes(b, ch, cw, oh, ow), l
    b, l, m = crop_boxes(resize_boxes(boxes, h, w, h1, w1), labels, cx, cy, ch, cw, row_map)
    return resize_boxes(b, ch, cw, oh, ow), l, m


# ------------------------------------------------------------------------------------------------------------------------------
# instance masks: the definition (host, numpy) and the launch
# ------------------------------------------------------------------------------------------------------------------------------

def nn_index(d, n_in, n_out):
    """Source index of output index d (int or array) of a nearest-neighbour resize n_in -> n_out: cv2.resize(INTER_NEAREST)'s rule,
    min(int(floor(d * (1 / (n_out / n_in)))), n_in - 1) in float64.  PARITY: unpinned (module docstring, "Instance masks")."""
    inv = 1.0 / (np.float64(n_out) / np.float64(n_in))
    return np.minimum(np.floor(np.asarray(d, np.float64) * inv).astype(np.int64), n_in - 1)


def _wrap_taps(c, n):
    """scipy's order-1 taps on axis n with the 'wrap' boundary of period n - 1 (module docstring): i0, i1, w0, w1."""
    sz = n - 1
    c = np.array(c, np.float64)
    neg, big = c < 0, c > n - 1
    c[neg] += sz * ((-c[neg] / sz).astype(np.int64) + 1)
    c[big] -= sz * (c[big] / sz).astype(np.int64)
    f = np.floor(c)
    w0 = 1.0 - (c - f)
    i0 = f.astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), w0, 1.0 - w0


def sample_plane01(p, refy, refx):
    """A float64 0 / 1 plane sampled at (refy, refx) (arrays that broadcast) as the stretch samples the image: wrap taps, the blend
    accumulated row-major as (value * wy) * wx, rounded half-up -- 1 where the blend reaches 0.5, else 0."""
    H, W = p.shape
    ya, yb, wy0, wy1 = _wrap_taps(refy, H)
    xa, xb, wx0, wx1 = _wrap_taps(refx, W)
    t = 0.0 + p[ya, xa] * wy0 * wx0
    t = t + p[ya, xb] * wy0 * wx1
    t = t + p[yb, xa] * wy1 * wx0
    t = t + p[yb, xb] * wy1 * wx1
    return np.floor(t + 0.5)


def warp_plane01(plane, stretch, kx, ky, shift, flip):
    """Wm of one bitmap: the 0 / 1 plane `plane != 0` ([H, W]) through the image's warp as a one-channel image -- the stretch with the
    module docstring's coordinates, taps and half-up rounding, then the roll by `shift` columns, then the flip.  uint8 0 / 1."""
    p = (np.asarray(plane) != 0).astype(np.float64)
    H, W = p.shape
    if stretch:
        u = ((np.arange(W, dtype=np.float64) + 0.5) / W - 0.5) * 2 * np.pi
        v = ((np.arange(H, dtype=np.float64) + 0.5) / H - 0.5) * np.pi
        su = np.sin(u)
        u0 = np.arctan2(su * kx / ky, np.cos(u))
        v0 = np.arctan(np.tan(v)[:, None] * np.sin(u0)[None, :] / su[None, :] * ky)
        p = sample_plane01(p, (v0 / np.pi + 0.5) * H - 0.5, ((u0 / (2 * np.pi) + 0.5) * W - 0.5)[None, :])
    p = np.roll(p, int(shift), axis=1)
    if flip:
        p = p[:, ::-1]
    return np.ascontiguousarray(p).astype(np.uint8)


def mask_source_index(H, W, plan):
    """(sy int64 [oh], sx int64 [ow]) of a plan: the row and the column of the warped H x W plane that output pixel (y, x) shows."""
    h1, w1, cy, cx, ch, cw, oh, ow = (int(v) for v in plan)
    ys, xs = np.arange(oh), np.arange(ow)
    if h1 == 0:
        return nn_index(ys, H, oh), nn_index(xs, W, ow)
    return nn_index(cy + nn_index(ys, ch, oh), H, h1), nn_index(cx + nn_index(xs, cw, ow), W, w1)


def transform_masks_one(src, stretch, kx, ky, shift, flip, plan, rows, pad_hw):
    """The definition of pswin_pano_masks for one image.  src: uint8 [n_in, H, W] bitmaps (a byte is set when it is not zero); plan:
    (h1, w1, cy, cx, ch, cw, oh, ow) as resize_crop_resize_normalize_pad defines it; rows: int32 [n_out, 2] row provenance (entries
    outside [0, n_in) read nothing); pad_hw = (Hp, Wp).  Returns uint8 [n_out, Hp, Wp] of 0 / 1:

        out[r, y, x] = max over the sources a of rows[r] of Wm[a][sy[y], sx[x]]     inside oh x ow, 0 in the pad,

    Wm = warp_plane01, (sy, sx) = mask_source_index.  Resize, crop and resize are nearest-neighbour index chains (nn_index), as
    BitmapMasks.rescale / crop / resize; the stretch and the roll have no mask path in the reference: the mask goes where the image
    goes, by the image's own expression, which on a 0 / 1 plane gives 0 / 1 again."""
    src = np.asarray(src)
    n_in, H, W = src.shape
    Hp, Wp = int(pad_hw[0]), int(pad_hw[1])
    oh, ow = int(plan[6]), int(plan[7])
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    out = np.zeros((len(rows), Hp, Wp), np.uint8)
    sy, sx = mask_source_index(H, W, plan)
    warped = {}
    for r, pair in enumerate(rows):
        for a in pair:
            if 0 <= a < n_in:
                if a not in warped:
                    warped[a] = warp_plane01(src[a], stretch, kx, ky, shift, flip)
                out[r, :oh, :ow] = np.maximum(out[r, :oh, :ow], warped[a][sy][:, sx])
    return out


def transform_masks(masks, params, plans, rows, pad_hw):
    """transform_masks_one over a batch: masks a list of [n_i, H, W], params the drawn dict, plans and rows one entry per image."""
    return [transform_masks_one(masks[i], params["stretch"][i], params["kx"][i], params["ky"][i], params["shift"][i], params["flip"][i],
                                plans[i], rows[i], pad_hw) for i in range(len(masks))]


def masks_addressable(B, Gin, Gmax, H, W, Hp, Wp):
    """What pswin_pano_masks can index: offsets inside a source or an output plane are 32-bit, the bases of the planes 64-bit, the grid
    has B layers and ceil(Hp / 16) rows of workgroups."""
    return H * W < 2 ** 31 and Hp * Wp < 2 ** 31 and B * Gmax < 2 ** 31 and B * Gin < 2 ** 31 and B <= 65535 and -(-Hp // 16) <= 65535


def pack_rows(rows, max_gt):
    """Host lists of per-image row maps -> (int32 [B, max_gt, 2] padded with -1, int32 [B] counts)."""
    maps = [np.asarray(r, np.int32).reshape(-1, 2) for r in rows]
    if max(len(m) for m in maps) > max_gt:
        raise PswinError(f"pack_rows: an image has {max(len(m) for m in maps)} rows, max_gt = {max_gt}")
    packed = np.full((len(maps), max_gt, 2), -1, np.int32)
    for b, m in enumerate(maps):
        packed[b, :len(m)] = m
    return packed, np.array([len(m) for m in maps], np.int32)


def warp_resize_masks(src, params, plan, rows, count=None, pad_hw=None, size_divisor=32, out=None):
    """pswin_pano_masks: the bitmaps of a batch through stretch, roll, flip, resize (-> crop -> resize) and pad in one launch, every
    byte of the result written.  src: device uint8 [B, Gin, H, W]; params: the drawn dict or a device float64 [B, 4] tensor; plan: host
    rows as resize_crop_resize_normalize_pad takes them (validated here) or a device int32 [B, 8] tensor (clamped on the device; then
    pad_hw must be given); rows: a host list of per-image [n_i, 2] maps (count is then theirs, and Gmax that of `out`, else the largest
    n_i, at least 1) or a device int32 [B, Gmax, 2] tensor with count a device int32 [B] tensor.  Returns uint8 [B, Gmax, Hp, Wp]."""
    what = "warp_resize_masks"
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise PswinError(f"{what}: the PanoSwin kernels run on an MI355X (HIP) device only; got a CPU tensor")
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[1] < 1:
        raise PswinError(f"{what}: expected uint8 [B, Gin, H, W] bitmaps with Gin >= 1, got {src.dtype} {tuple(src.shape)}")
    B, Gin, H, W = src.shape
    dev = src.device
    if W % 2:
        raise PswinError(f"{what}: the width must be even (sin u = 0 at x = (W-1)/2), got {W}")
    if H < 2:
        raise PswinError(f"{what}: the height must be at least 2, got {H}")
    if isinstance(params, dict):
        params = params_tensor(params, dev)
    if not isinstance(params, torch.Tensor) or params.dtype != torch.float64 or tuple(params.shape) != (B, 4) or params.device != dev \
            or not params.is_contiguous():
        raise PswinError(f"{what}: params must be a contiguous float64 [B, 4] tensor on the bitmaps' device")
    if isinstance(plan, torch.Tensor):
        if pad_hw is None:
            raise PswinError(f"{what}: pass pad_hw with a device plan tensor")
        if plan.dtype != torch.int32 or tuple(plan.shape) != (B, 8) or plan.device != dev or not plan.is_contiguous():
            raise PswinError(f"{what}: plan must be a contiguous int32 [B, 8] tensor on the bitmaps' device")
        plan_t = plan
    else:
        host = _host_plan(plan, B, what)
        sizes = [(r[6], r[7]) for r in host]
        if pad_hw is None:
            pad_hw = padded_size(sizes, size_divisor)
        if any(h > pad_hw[0] or w > pad_hw[1] for h, w in sizes):
            raise PswinError(f"{what}: an output size exceeds the padded size {tuple(pad_hw)}")
        plan_t = torch.tensor(host, dtype=torch.int32, device=dev)
    Hp, Wp = int(pad_hw[0]), int(pad_hw[1])
    if Hp < 1 or Wp < 1:
        raise PswinError(f"{what}: the padded size must be positive, got {pad_hw}")
    if isinstance(rows, torch.Tensor):
        if rows.dtype != torch.int32 or rows.dim() != 3 or rows.shape[0] != B or rows.shape[1] < 1 or rows.shape[2] != 2 \
                or rows.device != dev or not rows.is_contiguous():
            raise PswinError(f"{what}: rows must be a contiguous int32 [B, Gmax, 2] tensor on the bitmaps' device")
        if not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or tuple(count.shape) != (B,) or count.device != dev \
                or not count.is_contiguous():
            raise PswinError(f"{what}: with a device rows tensor, count must be a contiguous int32 [B] tensor on the same device")
        rows_t, count_t = rows, count
    else:
        if count is not None or len(rows) != B:
            raise PswinError(f"{what}: host rows are one [n_i, 2] map per image ({B}), and carry their own count")
        max_gt = out.shape[1] if isinstance(out, torch.Tensor) and out.dim() == 4 else max(1, max(len(r) for r in rows))
        packed, counts = pack_rows(rows, max_gt)
        rows_t, count_t = torch.from_numpy(packed).to(dev), torch.from_numpy(counts).to(dev)
    Gmax = rows_t.shape[1]
    if not masks_addressable(B, Gin, Gmax, H, W, Hp, Wp):
        raise PswinError(f"{what}: B = {B}, Gin = {Gin}, Gmax = {Gmax}, {H} x {W} -> {Hp} x {Wp} is past what the kernel can index "
                         "(masks_addressable)")
    x = src.contiguous()
    if out is None:
        out = torch.empty(B, Gmax, Hp, Wp, device=dev, dtype=torch.uint8)
    else:
        _check_buffer(out, what, "out", torch.uint8, (B, Gmax, Hp, Wp), dev, (x, params, plan_t, rows_t, count_t))
    _lib.call("pswin_pano_masks", x, _lib.ptr(x), _lib.ptr(params), _lib.ptr(plan_t), _lib.ptr(rows_t), _lib.ptr(count_t), _lib.ptr(out),
              B, Gin, Gmax, H, W, Hp, Wp, algo_bytes=x.numel() + out.numel())
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the recipe
# ------------------------------------------------------------------------------------------------------------------------------

class PanoTrainTransform:
    """PanoStretch -> RollAug -> RandomFlip -> Resize -> Normalize -> Pad of the streetwin recipe, pixels on the device.

        x, boxes, labels, img_metas = PanoTrainTransform()(imgs_u8, boxes, labels)

    imgs_u8: uint8 [B, H, W, 3] BGR on the device, all of one size (group mixed sizes into separate calls); boxes: list of float32
    [n_i, 4]; labels: list of int64 [n_i].  x: float32 [B, 3, Hp, Wp], the backbone's input.

    auto_augment=STREETWIN_AUTO_AUGMENT puts the recipe's AutoAugment in the place of the Resize: per image either the Resize or
    Resize -> RandomCrop -> Resize (module docstring), both policies of a batch in one launch.  img_metas then also hold
    auto_augment_policy, crop ((y1, x1, y2, x2) in the first resize's image, or None), pano_ratio_v and pano_lr_noadj (crop width ==
    w1; None without a crop, where the reference leaves the key out); img_shape, scale, scale_factor (new / crop) and pad_shape
    describe the final resize, as mmdet leaves them."""

    def __init__(self, kxy=(2.0, 2.0), stretch_chance=1.0, roll_chance=1.0, clip01=True, flip_ratio=0.5, img_scales=TRAIN_RESIZE_SCALES,
                 mean=IMG_NORM_MEAN, std=IMG_NORM_STD, to_rgb=True, size_divisor=32, rng=np.random, auto_augment=None):
        self.kxy, self.stretch_chance, self.roll_chance, self.clip01 = tuple(kxy), stretch_chance, roll_chance, clip01
        self.flip_ratio, self.img_scales = flip_ratio, [tuple(s) for s in img_scales]
        self.mean, self.std, self.to_rgb, self.size_divisor, self.rng = mean, std, to_rgb, size_divisor, rng
        self.auto_augment = auto_augment
        self._norm = {}

    def draw(self, B, W):
        """Per image: the pano parameters, then the Resize scale (the reference's order)."""
        parts, scales = [], []
        for _ in range(B):
            parts.append(draw_pano_params(1, W, self.kxy, self.stretch_chance, self.roll_chance, self.flip_ratio, self.rng))
            scales.append(self.img_scales[self.rng.randint(len(self.img_scales))] if len(self.img_scales) > 1 else self.img_scales[0])
        params = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        return params, scales

    def draw_auto(self, B, H, W):
        """Per image: the pano parameters, then the AutoAugment draws (the reference's order)."""
        parts, aas = [], []
        for _ in range(B):
            parts.append(draw_pano_params(1, W, self.kxy, self.stretch_chance, self.roll_chance, self.flip_ratio, self.rng))
            aas.append(draw_auto_augment(H, W, self.auto_augment, self.rng, self.img_scales))
        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}, aas

    def _meta(self, params, i, H, W, nh, nw, fh, fw, scale, pad_hw, d):
        return dict(ori_shape=(H, W, 3), img_shape=(nh, nw, 3), pad_shape=(-(-nh // d) * d, -(-nw // d) * d, 3),
                    batch_input_shape=tuple(pad_hw), scale=scale,
                    scale_factor=np.array([nw / fw, nh / fh, nw / fw, nh / fh], np.float32),
                    flip=bool(params["flip"][i]), flip_direction="horizontal" if params["flip"][i] else None,
                    pano_stretch=(float(params["kx"][i]), float(params["ky"][i])) if params["stretch"][i] else None,
                    roll_dist=float(params["roll_dist"][i]) if params["roll"][i] else None, roll_shift=int(params["shift"][i]),
                    img_norm_cfg=dict(mean=np.array(self.mean, np.float32), std=np.array(self.std, np.float32),
                                      to_rgb=self.to_rgb))

    def _run(self, imgs_u8, boxes, labels):
        """The draws, the two launches and the host side of both recipes: (x, boxes, labels, metas) and what the mask launch needs
        (params, plan rows, pad_hw, the composed row maps)."""
        _check_images(imgs_u8, "PanoTrainTransform", (3,))
        B, H, W, _ = imgs_u8.shape
        if len(boxes) != B or len(labels) != B:
            raise PswinError(f"PanoTrainTransform: {B} images but {len(boxes)} box arrays and {len(labels)} label arrays")
        dev = imgs_u8.device
        d = self.size_divisor or 1
        if self.auto_augment is not None:
            params, aas = self.draw_auto(B, H, W)
            plan = [a["plan"] for a in aas]
        else:
            params, scales = self.draw(B, W)
            plan = [(0, 0, 0, 0, 0, 0) + rescale_size(H, W, s) for s in scales]
        pad_hw = padded_size([p[6:] for p in plan], self.size_divisor)
        if dev not in self._norm:
            self._norm[dev] = norm_tensor(self.mean, self.std, dev)
        warped = pano_warp(imgs_u8, params)
        if self.auto_augment is not None:
            x = resize_crop_resize_normalize_pad(warped, plan, to_rgb=self.to_rgb, size_divisor=self.size_divisor, pad_hw=pad_hw,
                                                 norm=self._norm[dev])
        else:
            x = resize_normalize_pad(warped, [p[6:] for p in plan], to_rgb=self.to_rgb, size_divisor=self.size_divisor, pad_hw=pad_hw,
                                     norm=self._norm[dev])
        boxes, labels, maps = transform_boxes(boxes, labels, H, W, params, self.clip01, row_map=True)
        metas = []
        for i in range(B):
            h1, w1, cy, cx, ch, cw, nh, nw = plan[i]
            if self.auto_augment is not None:
                a = aas[i]
                boxes[i], labels[i], maps[i] = auto_augment_boxes(boxes[i], labels[i], H, W, a, maps[i])
                fh, fw = (ch, cw) if a["policy"] else (H, W)               # what the final resize took in
                m = self._meta(params, i, H, W, nh, nw, fh, fw, a["scale"], pad_hw, d)
                m.update(auto_augment_policy=a["policy"], crop=a["crop"], pano_ratio_v=a["pano_ratio_v"], pano_lr_noadj=a["pano_lr_noadj"])
            else:
                boxes[i] = resize_boxes(boxes[i], H, W, nh, nw)
                m = self._meta(params, i, H, W, nh, nw, H, W, scales[i], pad_hw, d)
            metas.append(m)
        return (x, boxes, labels, metas), (params, plan, pad_hw, maps)

    def __call__(self, imgs_u8, boxes, labels):
        return self._run(imgs_u8, boxes, labels)[0]

    def with_targets(self, imgs_u8, boxes, labels, masks=None, out=None):
        """__call__ with the annotations as the detector takes them:

            x, targets, img_metas = PanoTrainTransform(...).with_targets(imgs_u8, boxes, labels, masks=None, out=None)

        The draws, x, the boxes, the labels and img_metas are those of __call__ under the same RNG state.  targets is a
        detector.PaddedTargets: boxes, labels and count filled by one copy each, masks (uint8 [B, Gmax, Hp, Wp], the padded input's
        resolution) by one launch of pswin_pano_masks (warp_resize_masks), every byte.  masks: a list of per-image [n_i, H, W] uint8
        arrays or tensors, one bitmap per input box, or one packed device tensor [B, Gin, H, W] (rows past an image's boxes are
        ignored), or a polygons.PolygonBatch of the images' size whose object k of image b belongs to box k (rasterised once by
        polygons_to_masks, then the packed-tensor route); None gives targets.masks = None, the Faster R-CNN form.  out: a PaddedTargets to write in place (its max_gt must
        hold the batch's rows and its masks have this batch's padded size); None allocates one with Gmax = the largest count, at
        least 1."""
        from .detector import PaddedTargets
        what = "PanoTrainTransform.with_targets"
        n_in = [int(np.asarray(b).reshape(-1, 4).shape[0]) for b in boxes]
        (x, boxes, labels, metas), (params, plan, pad_hw, maps) = self._run(imgs_u8, boxes, labels)
        B, H, W, _ = imgs_u8.shape
        dev = imgs_u8.device
        counts = [len(b) for b in boxes]
        if out is None:
            Gmax = max(1, max(counts))
            out = PaddedTargets(torch.empty(B, Gmax, 4, device=dev), torch.empty(B, Gmax, dtype=torch.long, device=dev),
                                torch.empty(B, dtype=torch.int32, device=dev),
                                None if masks is None else torch.empty(B, Gmax, pad_hw[0], pad_hw[1], dtype=torch.uint8, device=dev))
        else:
            if not isinstance(out, PaddedTargets):
                raise PswinError(f"{what}: out must be a PaddedTargets, got {type(out).__name__}")
            Gmax = out.boxes.shape[1] if out.boxes.dim() == 3 else -1
            if tuple(out.boxes.shape) != (B, Gmax, 4) or tuple(out.labels.shape) != (B, Gmax) or tuple(out.count.shape) != (B,):
                raise PswinError(f"{what}: out holds boxes {tuple(out.boxes.shape)}, labels {tuple(out.labels.shape)}, count "
                                 f"{tuple(out.count.shape)}; the batch has {B} images")
            if max(counts) > Gmax:
                raise PswinError(f"{what}: an image has {max(counts)} boxes, out holds max_gt = {Gmax}")
            if (masks is None) != (out.masks is None):
                raise PswinError(f"{what}: masks must be given exactly when out has a mask buffer")
            if masks is not None and tuple(out.masks.shape) != (B, Gmax) + tuple(pad_hw):
                raise PswinError(f"{what}: out.masks is {tuple(out.masks.shape)}, this batch needs {(B, Gmax) + tuple(pad_hw)}")
        if masks is not None:
            src = self._pack_masks(masks, n_in, B, H, W, dev, what)
            packed, _ = pack_rows(maps, Gmax)
        hb, hl = np.zeros((B, Gmax, 4), np.float32), np.zeros((B, Gmax), np.int64)
        for b, n in enumerate(counts):
            hb[b, :n], hl[b, :n] = boxes[b], labels[b]
        out.boxes.copy_(torch.from_numpy(hb))
        out.labels.copy_(torch.from_numpy(hl))
        out.count.copy_(torch.tensor(counts, dtype=torch.int32))
        out.list_counts = None
        if masks is not None:
            warp_resize_masks(src, params, plan, torch.from_numpy(packed).to(dev), out.count, pad_hw=pad_hw, out=out.masks)
        return x, out, metas

    @staticmethod
    def _pack_masks(masks, n_in, B, H, W, dev, what):
        """The source bitmaps as one device uint8 [B, Gin, H, W] tensor: a packed tensor as it is, a list padded with zero planes, a
        polygons.PolygonBatch rasterised once (polygons_to_masks: on the GPU two launches and no bitmap upload)."""
        from .polygons import PolygonBatch, polygons_to_masks
        if isinstance(masks, PolygonBatch):
            if masks.xy.device != dev or masks.B != B or (masks.height, masks.width) != (H, W) or masks.K < max(1, max(n_in)):
                raise PswinError(f"{what}: the PolygonBatch must hold {B} images of {H} x {W} on {dev} with K >= every image's boxes "
                                 f"({max(n_in)}); got B = {masks.B}, K = {masks.K}, {masks.height} x {masks.width} on {masks.xy.device}")
            return polygons_to_masks(masks)
        if isinstance(masks, torch.Tensor):
            if not masks.is_cuda or masks.device != dev or masks.dtype != torch.uint8 or masks.dim() != 4 or masks.shape[0] != B \
                    or tuple(masks.shape[2:]) != (H, W) or masks.shape[1] < max(1, max(n_in)):
                raise PswinError(f"{what}: packed masks must be a uint8 [B, Gin, {H}, {W}] tensor on {dev} with Gin >= every image's "
                                 f"boxes ({max(n_in)}); got {masks.dtype} {tuple(masks.shape)} on {masks.device}")
            return masks
        if len(masks) != B:
            raise PswinError(f"{what}: {B} images but {len(masks)} mask arrays")
        src = torch.zeros(B, max(1, max(n_in)), H, W, dtype=torch.uint8, device=dev)
        for b, m in enumerate(masks):
            m = torch.as_tensor(m)
            if m.dtype != torch.uint8 or tuple(m.shape) != (n_in[b], H, W):
                raise PswinError(f"{what}: image {b} needs uint8 masks of shape {(n_in[b], H, W)}, one per box; got {m.dtype} "
                                 f"{tuple(m.shape)}")
            if n_in[b]:
                src[b, :n_in[b]].copy_(m)
        return src


# ------------------------------------------------------------------------------------------------------------------------------
# test-time views (MultiScaleFlipAug)
# ------------------------------------------------------------------------------------------------------------------------------
def test_view_geometry(ori_hw, img_scales, flip=False):
    """The tta.View list of MultiScaleFlipAug(img_scale=img_scales, flip=flip) on H x W images (mmdet/datasets/pipelines/test_time_aug.py:
    for every scale the unflipped view, then the flipped one): img_hw = rescale_size(H, W, scale), scale_factor = (w / W, h / H, w / W,
    h / H) as float32 (Resize._resize_img)."""
    from .tta import View
    H, W = int(ori_hw[0]), int(ori_hw[1])
    views = []
    for scale in img_scales:
        h, w = rescale_size(H, W, scale)
        sf = (float(np.float32(w / W)), float(np.float32(h / H)))
        for f in ([False, True] if flip else [False]):
            views.append(View((h, w), sf + sf, f))
    return views


def test_views(imgs_u8, img_scales, flip=False, mean=IMG_NORM_MEAN, std=IMG_NORM_STD, to_rgb=True, size_divisor=32):
    """The V view batches of a uint8 [B, H, W, 3] batch and their tta.View: (list of V float32 [B, 3, Hp_v, Wp_v], list of V View), what
    model.aug_test takes.  Existing kernels only: a flipped view is pano_warp with nothing but the flip flag, then resize_normalize_pad to
    rescale_size -- the images of a batch share one size, so one View serves them all.

    PARITY: unpinned for the flipped views.  The reference resizes first and flips second (Resize, then RandomFlip); here the flip comes
    first.  With the project's own restatement of the resize (tests/_pano_ref.py resize_u8_f32) on random bytes the two orders give the same
    bytes at 64 x 128 -> 32 x 64, 64 x 128 -> 43 x 85 and 100 x 200 -> 64 x 128, and differ by one grey level in 2.7 % of the values at
    64 x 128 -> 96 x 192, 0.04 % at 128 x 256 -> 85 x 171 and 0.2 % at 512 x 1024 -> 400 x 800: the float32 source coordinate of a mirrored
    column is not the mirror of the column's.  The unflipped views are resize_normalize_pad as it is pinned elsewhere."""
    _check_images(imgs_u8, "test_views", (3,))
    B, H, W, _ = imgs_u8.shape
    views = test_view_geometry((H, W), img_scales, flip)
    flipped = None
    batches = []
    for v in views:
        src = imgs_u8
        if v.flip:
            if flipped is None:
                flipped = pano_warp(imgs_u8, make_pano_params([False] * B, [1.0] * B, [1.0] * B, None, [True] * B, W))
            src = flipped
        batches.append(resize_normalize_pad(src, [v.img_hw] * B, mean, std, to_rgb, size_divisor))
    return batches, views
