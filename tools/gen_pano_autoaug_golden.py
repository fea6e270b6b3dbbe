#!/usr/bin/env python3
"""Write tests/golden/pano_autoaug.npz: what the reference's AutoAugment (Resize | Resize -> RandomCrop -> Resize) draws and returns.

Build machine only: it needs the reference tree (PSWIN_REFERENCE_ROOT, default /root/reference, as oracle/ref_loader.py).  It imports
mmdet/datasets/pipelines/{transforms,auto_augment,compose}.py from where they lie and runs their Resize, RandomCrop and AutoAugment
with the policies of configs/swin/faster_rcnn_panoswin_tiny_patch4_window7_mstrain_480800_adamw_1x_streetwin.py:65-89.  Everything
else those files import (cv2, mmcv, mmdet.core, the PIPELINES registry, lzx) is a stand-in: the registry and build_from_cfg are a
dict, and mmcv.imrescale returns an image of the right size without resampling (sizes, boxes and draws are what is recorded; the
pixels are checked on the device against the project's own statement).  Nothing under the reference root is written, and the
interpreter is left as it was found.

    python tools/gen_pano_autoaug_golden.py [--out tests/golden/pano_autoaug.npz]

Contents: recorded results only.  Four sources (512x1024, 64x128, 49x98 and a portrait 96x64: a crop as wide as the image, the
reference's pano_lr_noadj, cannot happen on a 2:1 panorama, whose first resize is wider than the largest crop) with boxes that
straddle crop edges or fall outside; per case the seed, the policy, every integer drawn, the plan (h1, w1, cy, cx, ch, cw, oh, ow),
the final img_shape, boxes and labels, pano_ratio_v, pano_lr_noadj (-1: the key is absent) and the next rand() of the stream.
Seeds: the first few per source, then the first seed found for each property the tests ask for (a crop touching each edge, every box
dropped, pano_lr_noadj).
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("PSWIN_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "pano_autoaug.npz")

TRAIN_SCALES = [(480, 1333), (512, 1333), (544, 1333), (576, 1333), (608, 1333), (640, 1333), (672, 1333), (704, 1333), (736, 1333),
                (768, 1333), (800, 1333)]
FIRST_SCALES = [(400, 1333), (500, 1333), (600, 1333)]
CROP_SIZE = (384, 600)
SOURCES = [(512, 1024), (64, 128), (49, 98), (96, 64)]
PLAIN_SEEDS = 8                    # seeds 0 .. 7 of every source
SEARCH = 4000                      # seeds scanned for the cases with a wanted property


def policies():
    return [[dict(type="Resize", img_scale=TRAIN_SCALES, multiscale_mode="value", keep_ratio=True)],
            [dict(type="Resize", img_scale=FIRST_SCALES, multiscale_mode="value", keep_ratio=True),
             dict(type="RandomCrop", crop_type="absolute_range", crop_size=CROP_SIZE, allow_negative_crop=True),
             dict(type="Resize", img_scale=TRAIN_SCALES, multiscale_mode="value", override=True, keep_ratio=True)]]


def source_boxes(s, H, W):
    """float32 x1 y1 x2 y2 pixels and int64 labels.  Source 2 keeps its boxes in the left fifth, so that most crops drop them all."""
    if s == 2:
        f = [[0, 0.1, 0.12, 0.5], [0.05, 0.55, 0.2, 0.95], [0.0, 0.0, 0.03, 0.05]]
    else:
        f = [[0, 0.16, 0.16, 0.47], [0.78, 0.3, 1, 0.62], [0.3, 0.0, 0.55, 1.0], [0.45, 0.4, 0.5, 0.45], [0.1, 0.9, 0.9, 1.0],
             [0.6, 0.02, 0.7, 0.1], [0.0, 0.0, 1.0, 1.0], [0.97, 0.45, 1.0, 0.55]]
    b = np.array(f) * np.array([W, H, W, H])
    return np.round(b).astype(np.float32), np.arange(len(f), dtype=np.int64)


def _rescale(img, scale, return_scale=False, interpolation="bilinear", backend=None):
    """Stand-in for mmcv.imrescale: the size rule of mmcv.rescale_size, no resampling (a zero image of the new size)."""
    h, w = img.shape[:2]
    sf = min(max(scale) / max(h, w), min(scale) / min(h, w))
    out = np.broadcast_to(np.uint8(0), (int(h * float(sf) + 0.5), int(w * float(sf) + 0.5)) + img.shape[2:])
    _rescale.calls.append((img.shape[:2], out.shape[:2]))
    return (out, sf) if return_scale else out


_rescale.calls = []


def load_reference(root=REFERENCE_ROOT):
    """SimpleNamespace(AutoAugment, Resize, RandomCrop) of the reference, or None when its tree is not on this machine."""
    pipes = os.path.join(root, "mmdet", "datasets", "pipelines")
    if not os.path.isfile(os.path.join(pipes, "transforms.py")):
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
    stubs = {n: module(n, __path__=[]) for n in ["mmcv", "mmdet", "mmdet.core", "mmdet.core.evaluation", "mmdet.datasets"] + lzx}
    stubs["mmcv"].__dict__.update(is_list_of=is_list_of, imrescale=_rescale, imresize=unused)
    stubs["mmdet.core"].PolygonMasks = unused
    stubs["lzx"].coor_transition = module("lzx.coor_transition", xyxy2tlwh=unused, normlize01_xyxy=unused, unnormlize01_xyxy=unused)
    stubs.update({
        "cv2": module("cv2"),
        "mmcv.utils": module("mmcv.utils", build_from_cfg=build_from_cfg),
        "mmcv.parallel": module("mmcv.parallel", DataContainer=unused),
        "mmdet.core.evaluation.bbox_overlaps": module("mmdet.core.evaluation.bbox_overlaps", bbox_overlaps=unused),
        "mmdet.datasets.builder": module("mmdet.datasets.builder", PIPELINES=registry),
        "mmdet.datasets.pipelines": module("mmdet.datasets.pipelines", __path__=[pipes]),
        "lzx.coor_transition": stubs["lzx"].coor_transition,
        "lzx.utils": module("lzx.utils", cv_show1=unused),
        "lzx.lzx_augs.basketball_transform": module("lzx.lzx_augs.basketball_transform", basketball_transition=unused, rec_img=unused),
        "lzx.yolo.extensions.xzaug": module("lzx.yolo.extensions.xzaug", xzaug_xywh=unused),
        "lzx.yolo.extensions.rollaug": module("lzx.yolo.extensions.rollaug", roll_aug=unused),
    })
    saved_flag, saved = sys.dont_write_bytecode, {n: sys.modules.get(n) for n in stubs}
    before = set(sys.modules)
    try:
        sys.dont_write_bytecode = True
        sys.modules.update(stubs)
        importlib.import_module("mmdet.datasets.pipelines.transforms")
        importlib.import_module("mmdet.datasets.pipelines.auto_augment")
        return types.SimpleNamespace(AutoAugment=registry["AutoAugment"], Resize=registry["Resize"], RandomCrop=registry["RandomCrop"])
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


def run_seeded(ref, H, W, boxes, labels, seed, aug=None):
    """One H x W image through the reference's AutoAugment with the global np.random seeded; returns a dict of recorded results."""
    aug = aug or ref.AutoAugment(policies())
    drawn, orig = [], np.random.randint

    def spy(*a, **k):
        drawn.append(int(orig(*a, **k)))
        return drawn[-1]

    res = dict(img=np.broadcast_to(np.uint8(0), (H, W, 3)), gt_bboxes=boxes.copy(), gt_labels=labels.copy(), bbox_fields=["gt_bboxes"],
               img_fields=["img"])
    _rescale.calls.clear()
    np.random.randint = spy
    try:
        np.random.seed(seed)
        res = aug(res)
        nxt = float(np.random.rand())
    finally:
        np.random.randint = orig
    calls = list(_rescale.calls)
    policy = len(calls) - 1                                    # one Resize or two
    oh, ow = calls[-1][1]
    if policy:
        (h1, w1), (ch, cw) = calls[0][1], calls[1][0]
        plan = (h1, w1, drawn[3], drawn[4], ch, cw, oh, ow)      # first scale, crop_h, crop_w, offset_h, offset_w, final scale
    else:
        plan = (0, 0, 0, 0, 0, 0, oh, ow)
    assert tuple(res["img_shape"][:2]) == (oh, ow) and res["img"].shape[:2] == (oh, ow)
    return dict(seed=seed, policy=policy, draws=[policy] + drawn, plan=plan, img_shape=tuple(res["img_shape"]),
                boxes=res["gt_bboxes"].astype(np.float32), labels=res["gt_labels"].astype(np.int64),
                ratio_v=[float(v) for v in res.get("pano_ratio_v", [0.0, 1.0])], has_ratio_v="pano_ratio_v" in res,
                lr_noadj=int(res["pano_lr_noadj"]) if "pano_lr_noadj" in res else -1, next_rand=nxt)


WANTED = {
    "top": lambda r: r["policy"] == 1 and r["plan"][2] == 0,
    "left": lambda r: r["policy"] == 1 and r["plan"][3] == 0,
    "bottom": lambda r: r["policy"] == 1 and r["plan"][2] + r["plan"][4] == r["plan"][0],
    "right": lambda r: r["policy"] == 1 and r["plan"][3] + r["plan"][5] == r["plan"][1],
    "all_dropped": lambda r: r["policy"] == 1 and len(r["boxes"]) == 0,
    "lr_noadj": lambda r: r["lr_noadj"] == 1,
    "inner": lambda r: r["policy"] == 1 and 0 < r["plan"][2] and r["plan"][2] + r["plan"][4] < r["plan"][0] and 0 < r["plan"][3],
}


def generate(ref):
    d, cases = {}, []
    aug = ref.AutoAugment(policies())
    for s, (H, W) in enumerate(SOURCES):
        boxes, labels = source_boxes(s, H, W)
        d[f"boxes{s}"], d[f"labels{s}"] = boxes, labels
        seeds, missing = list(range(PLAIN_SEEDS)), dict(WANTED)
        for seed in range(PLAIN_SEEDS, SEARCH):
            if not missing:
                break
            r = run_seeded(ref, H, W, boxes, labels, seed, aug)
            hit = [k for k, f in missing.items() if f(r)]
            if hit:
                seeds.append(seed)
                for k in hit:
                    del missing[k]
        for seed in seeds:
            cases.append((s, run_seeded(ref, H, W, boxes, labels, seed, aug)))
    n = len(cases)
    width = max(len(r["draws"]) for _, r in cases)
    d["src_hw"] = np.array(SOURCES, np.int64)
    d["train_scales"], d["first_scales"], d["crop_size"] = np.array(TRAIN_SCALES), np.array(FIRST_SCALES), np.array(CROP_SIZE)
    d["n_cases"] = np.array(n)
    d["case_src"] = np.array([s for s, _ in cases], np.int64)
    d["case_seed"] = np.array([r["seed"] for _, r in cases], np.int64)
    d["case_policy"] = np.array([r["policy"] for _, r in cases], np.int64)
    d["case_draws"] = np.array([r["draws"] + [-1] * (width - len(r["draws"])) for _, r in cases], np.int64)
    d["case_plan"] = np.array([r["plan"] for _, r in cases], np.int64)
    d["case_img_shape"] = np.array([r["img_shape"] for _, r in cases], np.int64)
    d["case_ratio_v"] = np.array([r["ratio_v"] for _, r in cases], np.float64)
    d["case_has_ratio_v"] = np.array([r["has_ratio_v"] for _, r in cases], bool)
    d["case_lr_noadj"] = np.array([r["lr_noadj"] for _, r in cases], np.int8)
    d["case_next_rand"] = np.array([r["next_rand"] for _, r in cases], np.float64)
    d["case_n_boxes"] = np.array([len(r["boxes"]) for _, r in cases], np.int64)          # rows of out_boxes / out_labels per case
    d["out_boxes"] = np.concatenate([r["boxes"].reshape(-1, 4) for _, r in cases])
    d["out_labels"] = np.concatenate([r["labels"] for _, r in cases])
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
    print(f"wrote {a.out}: {int(d['n_cases'])} cases, {int(d['case_policy'].sum())} with a crop, "
          f"{int((d['case_lr_noadj'] == 1).sum())} with pano_lr_noadj, {os.path.getsize(a.out) / 1024:.1f} KiB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
