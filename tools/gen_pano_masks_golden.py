#!/usr/bin/env python3
"""Write tests/golden/pano_masks.npz: what the reference's RandomFlip -> AutoAugment (Resize | Resize -> RandomCrop -> Resize) -> Pad
returns for gt_masks (BitmapMasks) on small marker masks under fixed seeds.

Build machine only: it needs the reference tree (PSWIN_REFERENCE_ROOT, default /root/reference, as oracle/ref_loader.py).  It imports
mmdet/datasets/pipelines/{transforms,auto_augment,compose}.py and mmdet/core/mask/structures.py from where they lie and runs their
RandomFlip, AutoAugment, Resize, RandomCrop, Pad and BitmapMasks.  Everything else those files import is a stand-in, as in
tools/gen_pano_autoaug_golden.py; mmcv's image functions are numpy statements of their rules:
    imflip(horizontal)   img[:, ::-1]
    impad / impad_to_multiple   zeros of the new shape, the image in the top-left corner
    rescale_size         int(w * sf + 0.5), int(h * sf + 0.5), sf = min(long / max(h, w), short / min(h, w))
    imrescale / imresize with interpolation='nearest'   out[y, x] = in[nn(y, H, oh), nn(x, W, ow)],
                         nn(d, n_in, n_out) = min(int(floor(d * (1.0 / (n_out / n_in)))), n_in - 1): cv2.resize(INTER_NEAREST)'s rule
    imrescale with another interpolation (the image)    an image of the right size, no resampling
So the fixture pins the ORDER of the steps (flip first), which rows are kept, the crop arithmetic and every size to the reference;
it does NOT pin the resampling rule, which is the stand-in's (PARITY: unpinned).  Nothing under the reference root is written, and
the interpreter is left as it was found.

    python tools/gen_pano_masks_golden.py [--out tests/golden/pano_masks.npz]

The scales are the recipe's divided by ten (sources of 64x128, 49x98 and a portrait 96x64 give outputs of at most 80x133), so that
the fixture stays small and its test quick.  Contents: recorded results only.  Per source the marker masks (uint8, set bytes 1 / 255) and
boxes; per case the seed, the flip, the plan (h1, w1, cy, cx, ch, cw, oh, ow), the padded size, the input row of every returned mask
(the labels are the input row numbers) and the returned masks, bit-packed.
"""
import argparse
import importlib
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("PSWIN_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "pano_masks.npz")

TRAIN_SCALES = [(48, 133), (56, 133), (64, 133), (72, 133), (80, 133)]
FIRST_SCALES = [(40, 133), (50, 133), (60, 133)]
CROP_SIZE = (38, 60)
SOURCES = [(64, 128), (49, 98), (96, 64)]
PLAIN_SEEDS = 6                    # seeds 0 .. 5 of every source
SEARCH = 2000                      # seeds scanned for the cases with a wanted property


def policies():
    return [[dict(type="Resize", img_scale=TRAIN_SCALES, multiscale_mode="value", keep_ratio=True)],
            [dict(type="Resize", img_scale=FIRST_SCALES, multiscale_mode="value", keep_ratio=True),
             dict(type="RandomCrop", crop_type="absolute_range", crop_size=CROP_SIZE, allow_negative_crop=True),
             dict(type="Resize", img_scale=TRAIN_SCALES, multiscale_mode="value", override=True, keep_ratio=True)]]


def source(s, H, W):
    """Marker masks uint8 [n, H, W] (a filled box with a hole and a diagonal, bytes 1 or 255), their boxes and labels = row numbers."""
    f = [[0, 0.16, 0.16, 0.47], [0.78, 0.3, 1, 0.62], [0.3, 0.0, 0.55, 1.0], [0.45, 0.4, 0.5, 0.45], [0.1, 0.9, 0.9, 1.0],
         [0.0, 0.0, 1.0, 1.0], [0.02, 0.5, 0.12, 0.8]]
    b = np.round(np.array(f) * np.array([W, H, W, H])).astype(np.float32)
    m = np.zeros((len(b), H, W), np.uint8)
    for i, (x1, y1, x2, y2) in enumerate(b.astype(int)):
        m[i, y1:y2, x1:x2] = 255 if i % 2 else 1
        m[i, (y1 + y2) // 2, (x1 + x2) // 2] = 0
        for k in range(min(y2 - y1, x2 - x1)):
            m[i, y1 + k, x1 + k] = 0
    return m, b, np.arange(len(b), dtype=np.int64)


def _nn(d, n_in, n_out):
    return min(int(math.floor(d * (1.0 / (float(n_out) / float(n_in))))), n_in - 1)


def _resize_nearest(img, oh, ow):
    H, W = img.shape[:2]
    ys = [_nn(y, H, oh) for y in range(oh)]
    xs = [_nn(x, W, ow) for x in range(ow)]
    return np.ascontiguousarray(img[ys][:, xs])


def _rescale_size(old_size, scale, return_scale=False):
    w, h = old_size
    sf = min(max(scale) / max(h, w), min(scale) / min(h, w))
    new = (int(w * float(sf) + 0.5), int(h * float(sf) + 0.5))
    return (new, sf) if return_scale else new


def _imresize(img, size, return_scale=False, interpolation="bilinear", out=None, backend=None):
    ow, oh = size
    if interpolation == "nearest":
        res = _resize_nearest(img, oh, ow)
    else:
        res = np.broadcast_to(np.uint8(0), (oh, ow) + img.shape[2:])
        _imresize.image_calls.append((img.shape[:2], (oh, ow)))
    return (res, ow / img.shape[1], oh / img.shape[0]) if return_scale else res


_imresize.image_calls = []


def _imrescale(img, scale, return_scale=False, interpolation="bilinear", backend=None):
    new, sf = _rescale_size((img.shape[1], img.shape[0]), scale, return_scale=True)
    res = _imresize(img, new, interpolation=interpolation)
    return (res, sf) if return_scale else res


def _imflip(img, direction="horizontal"):
    assert direction == "horizontal"
    return np.flip(img, axis=1)


def _impad(img, *, shape=None, padding=None, pad_val=0, padding_mode="constant"):
    out = np.full(tuple(shape[:2]) + img.shape[2:], pad_val, img.dtype)
    out[:img.shape[0], :img.shape[1]] = img
    return out


def _impad_to_multiple(img, divisor, pad_val=0):
    return _impad(img, shape=(-(-img.shape[0] // divisor) * divisor, -(-img.shape[1] // divisor) * divisor), pad_val=pad_val)


def load_reference(root=REFERENCE_ROOT):
    """SimpleNamespace(AutoAugment, RandomFlip, Pad, BitmapMasks) of the reference, or None when its tree is not on this machine."""
    pipes = os.path.join(root, "mmdet", "datasets", "pipelines")
    maskdir = os.path.join(root, "mmdet", "core", "mask")
    if not os.path.isfile(os.path.join(pipes, "transforms.py")) or not os.path.isfile(os.path.join(maskdir, "structures.py")):
        return None

    def unused(*a, **k):
        raise NotImplementedError("stand-in: not used on the path the golden generator calls")

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        return m

    class Registry(dict):
        def register_module(self, *a, **k):
            def deco(cls):
                self[cls.__name__] = cls
                return cls
            return deco

    def build_from_cfg(cfg, registry, default_args=None):
        args = dict(cfg)
        return registry[args.pop("type")](**args)

    def is_list_of(seq, t):
        return isinstance(seq, list) and all(isinstance(v, t) for v in seq)

    registry = Registry()
    lzx = ["lzx", "lzx.lzx_augs", "lzx.yolo", "lzx.yolo.extensions"]
    names = ["mmcv", "mmcv.ops", "mmdet", "mmdet.core", "mmdet.core.evaluation", "mmdet.datasets", "pycocotools"] + lzx
    stubs = {n: module(n, __path__=[]) for n in names}
    stubs["mmcv"].__dict__.update(is_list_of=is_list_of, imrescale=_imrescale, imresize=_imresize, imflip=_imflip, impad=_impad,
                                  impad_to_multiple=_impad_to_multiple, rescale_size=_rescale_size)
    stubs["mmdet.core"].PolygonMasks = unused
    stubs["lzx"].coor_transition = module("lzx.coor_transition", xyxy2tlwh=unused, normlize01_xyxy=unused, unnormlize01_xyxy=unused)
    stubs.update({
        "cv2": module("cv2"),
        "pycocotools.mask": module("pycocotools.mask"),
        "mmcv.utils": module("mmcv.utils", build_from_cfg=build_from_cfg),
        "mmcv.parallel": module("mmcv.parallel", DataContainer=unused),
        "mmcv.ops.roi_align": module("mmcv.ops.roi_align", roi_align=unused),
        "mmdet.core.mask": module("mmdet.core.mask", __path__=[maskdir]),
        "mmdet.core.evaluation.bbox_overlaps": module("mmdet.core.evaluation.bbox_overlaps", bbox_overlaps=unused),
        "mmdet.datasets.builder": module("mmdet.datasets.builder", PIPELINES=registry),
        "mmdet.datasets.pipelines": module("mmdet.datasets.pipelines", __path__=[pipes]),
        "lzx.coor_transition": stubs["lzx"].coor_transition,
        "lzx.utils": module("lzx.utils", cv_show1=unused),
        "lzx.lzx_augs.basketball_transform": module("lzx.lzx_augs.basketball_transform", basketball_transition=unused, rec_img=unused),
        "lzx.yolo.extensions.xzaug": module("lzx.yolo.extensions.xzaug", xzaug_xywh=unused),
        "lzx.yolo.extensions.rollaug": module("lzx.yolo.extensions.rollaug", roll_aug=unused),
    })
    stubs["pycocotools"].mask = stubs["pycocotools.mask"]
    saved_flag, saved = sys.dont_write_bytecode, {n: sys.modules.get(n) for n in stubs}
    before = set(sys.modules)
    try:
        sys.dont_write_bytecode = True
        sys.modules.update(stubs)
        structures = importlib.import_module("mmdet.core.mask.structures")
        importlib.import_module("mmdet.datasets.pipelines.transforms")
        importlib.import_module("mmdet.datasets.pipelines.auto_augment")
        return types.SimpleNamespace(AutoAugment=registry["AutoAugment"], RandomFlip=registry["RandomFlip"], Pad=registry["Pad"],
                                     BitmapMasks=structures.BitmapMasks)
    except ImportError:
        return None
    finally:
        sys.dont_write_bytecode = saved_flag
        for n in set(sys.modules) - before:
            if n in stubs or n.startswith("mmdet.") or n.startswith("lzx."):
                del sys.modules[n]
        for n, m in saved.items():
            if m is not None:
                sys.modules[n] = m
            else:
                sys.modules.pop(n, None)


def make_pipeline(ref):
    return [ref.RandomFlip(flip_ratio=0.5), ref.AutoAugment(policies()), ref.Pad(size_divisor=32)]


def run_seeded(ref, masks, boxes, labels, seed, pipeline=None):
    """One image's annotations through the reference's RandomFlip -> AutoAugment -> Pad with the global np.random seeded."""
    pipeline = pipeline or make_pipeline(ref)
    H, W = masks.shape[1:]
    drawn, orig = [], np.random.randint

    def spy(*a, **k):
        drawn.append(int(orig(*a, **k)))
        return drawn[-1]

    res = dict(img=np.broadcast_to(np.uint8(0), (H, W, 3)), img_shape=(H, W, 3), ori_shape=(H, W, 3), gt_bboxes=boxes.copy(),
               gt_labels=labels.copy(), gt_masks=ref.BitmapMasks(masks.copy(), H, W), bbox_fields=["gt_bboxes"], mask_fields=["gt_masks"],
               img_fields=["img"])
    _imresize.image_calls.clear()
    np.random.seed(seed)
    res = pipeline[0](res)
    np.random.randint = spy
    try:
        res = pipeline[1](res)
    finally:
        np.random.randint = orig
    res = pipeline[2](res)
    calls = list(_imresize.image_calls)
    policy = len(calls) - 1                                    # one Resize or two
    oh, ow = calls[-1][1]
    if policy:
        (h1, w1), (ch, cw) = calls[0][1], calls[1][0]
        plan = (h1, w1, drawn[3], drawn[4], ch, cw, oh, ow)      # first scale, crop_h, crop_w, offset_h, offset_w, final scale
    else:
        plan = (0, 0, 0, 0, 0, 0, oh, ow)
    out = res["gt_masks"].masks
    hp, wp = res["pad_shape"][:2]
    assert out.shape == (len(res["gt_labels"]), hp, wp) and res["gt_masks"].height == hp and res["gt_masks"].width == wp
    return dict(seed=seed, policy=policy, flip=bool(res["flip"]), plan=plan, pad_hw=(int(hp), int(wp)),
                rows=res["gt_labels"].astype(np.int64), masks=(out != 0).astype(np.uint8))


WANTED = {
    "flip_crop": lambda r: r["policy"] == 1 and r["flip"] and r["plan"][3] > 0 and len(r["rows"]) > 0,
    "noflip_crop": lambda r: r["policy"] == 1 and not r["flip"] and r["plan"][2] > 0 and len(r["rows"]) > 0,
    "dropped": lambda r: r["policy"] == 1 and 0 < len(r["rows"]) < 7,
    "flip_plain": lambda r: r["policy"] == 0 and r["flip"],
    "noflip_plain": lambda r: r["policy"] == 0 and not r["flip"],
    "right": lambda r: r["policy"] == 1 and r["plan"][3] + r["plan"][5] == r["plan"][1],
}


def generate(ref):
    d, cases = {}, []
    pipeline = make_pipeline(ref)
    for s, (H, W) in enumerate(SOURCES):
        masks, boxes, labels = source(s, H, W)
        d[f"masks{s}"], d[f"boxes{s}"] = masks, boxes
        seeds, missing = list(range(PLAIN_SEEDS)), dict(WANTED)
        for seed in range(PLAIN_SEEDS, SEARCH):
            if not missing:
                break
            r = run_seeded(ref, masks, boxes, labels, seed, pipeline)
            hit = [k for k, f in missing.items() if f(r)]
            if hit:
                seeds.append(seed)
                for k in hit:
                    del missing[k]
        for seed in seeds:
            cases.append((s, run_seeded(ref, masks, boxes, labels, seed, pipeline)))
    d["src_hw"] = np.array(SOURCES, np.int64)
    d["train_scales"], d["first_scales"], d["crop_size"] = np.array(TRAIN_SCALES), np.array(FIRST_SCALES), np.array(CROP_SIZE)
    d["n_cases"] = np.array(len(cases))
    d["case_src"] = np.array([s for s, _ in cases], np.int64)
    d["case_seed"] = np.array([r["seed"] for _, r in cases], np.int64)
    d["case_flip"] = np.array([r["flip"] for _, r in cases], bool)
    d["case_plan"] = np.array([r["plan"] for _, r in cases], np.int64)
    d["case_pad_hw"] = np.array([r["pad_hw"] for _, r in cases], np.int64)
    d["case_n_rows"] = np.array([len(r["rows"]) for _, r in cases], np.int64)
    d["out_rows"] = np.concatenate([r["rows"] for _, r in cases])
    for i, (_, r) in enumerate(cases):
        d[f"out{i}"] = np.packbits(r["masks"].reshape(-1))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    ref = load_reference()
    if ref is None:
        print(f"reference not found under {REFERENCE_ROOT}", file=sys.stderr)
        return 1
    d = generate(ref)
    np.savez_compressed(a.out, **d)
    print(f"wrote {a.out}: {int(d['n_cases'])} cases, {int((d['case_plan'][:, 0] > 0).sum())} with a crop, {int(d['case_flip'].sum())} flipped, "
          f"{os.path.getsize(a.out) / 1024:.1f} KiB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
