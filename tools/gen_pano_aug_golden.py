#!/usr/bin/env python3
"""Write tests/golden/pano_aug.npz: reference outputs of PanoStretch -> RollAug -> RandomFlip for the pano augmentation tests.

Build machine only: it needs the reference tree (PSWIN_REFERENCE_ROOT, default /root/reference, as oracle/ref_loader.py) and scipy.
It imports lzx/yolo/extensions/{xzaug,rollaug,padding2}.py from where they lie, with stand-ins for cv2,
lzx.yolo.extensions.merge_bbs and lzx.yolo.utils.{general,metrics} (none of which the called functions use), and calls getAug /
_xzaug and roll_aug_raw (which applies merge_adjbox) directly.  The `__call__` glue of PanoStretch, RollAug (mmdet/datasets/pipelines/transforms.py:
992-1068) and mmdet's RandomFlip is restated below, because transforms.py needs mmcv and RollAug.__call__ uses np.float, which
NumPy >= 1.24 no longer has.  Nothing under the reference root is written.

    python tools/gen_pano_aug_golden.py [--out tests/golden/pano_aug.npz]

Contents: two smooth synthetic sources (64x128 and 49x98, odd H) with boxes that touch x = 0 and x = W (so the seam merge runs);
per case the parameters the reference drew or was given, its output image (stored as differences along x, encode_dx),
boxes and labels.  Cases: the 8 on/off combinations of
the three transforms (chances 0 or 1, seeded), a seeded run of consecutive images with chances 0.5, and hand-picked extremes
(kx, ky in {2, 1/2}, shift 0 and W-1, roll_dist close to 1, clip01 off).
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("PSWIN_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "pano_aug.npz")
KXY = (2.0, 2.0)

SOURCES = [(64, 128), (49, 98)]


def source_image(H, W, seed):
    """Smooth BGR panorama: a few low-frequency waves per channel plus a gentle ramp (compresses well, interpolates non-trivially)."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(3):
            fx, fy, ph = rng.randint(1, 4), rng.uniform(0.5, 2.5), rng.uniform(0, 2 * np.pi)
            img[..., c] += rng.uniform(20, 45) * np.sin(2 * np.pi * fx * x / W + ph) * np.cos(np.pi * fy * y / H + c)
        img[..., c] += 128 + 30 * (y / H - 0.5)
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


def source_boxes(H, W):
    """x1 y1 x2 y2 in pixels (float32, as mmdet's loader gives them) and int64 labels; boxes 0 / 3 touch x = 0, 1 / 2 touch x = W."""
    b = np.array([[0, 0.16 * H, 0.16 * W, 0.47 * H], [0.78 * W, 0.3 * H, W, 0.62 * H], [0.84 * W, 0.19 * H, W, 0.47 * H],
                  [0, 0.47 * H, 0.1 * W, 0.78 * H], [0.31 * W, 0.08 * H, 0.55 * W, 0.94 * H], [0.47 * W, 0.4 * H, 0.48 * W, 0.42 * H]])
    return np.round(b).astype(np.float32), np.array([1, 2, 3, 4, 0, 5], np.int64)


def encode_dx(img):
    """uint8 image -> its differences along x modulo 256 (the first column as is): smooth images then compress about 2x better.
    Decode with np.cumsum(dx, axis=1, dtype=np.int64) % 256."""
    prev = np.concatenate([np.zeros_like(img[:, :1]), img[:, :-1]], 1)
    return (img.astype(np.int16) - prev).astype(np.uint8)


def load_reference(root=REFERENCE_ROOT):
    """The reference's xzaug / rollaug / padding2 modules, or None when the reference tree is not on this machine.

    The interpreter is left as it was found: sys.path, sys.dont_write_bytecode and sys.modules lose the reference root, the
    stand-ins and the lzx modules again (the returned module objects keep working: their functions hold their own globals)."""
    ext = os.path.join(root, "lzx", "yolo", "extensions")
    if not os.path.isfile(os.path.join(ext, "xzaug.py")):
        return None
    try:
        import scipy.ndimage  # noqa: F401  (getAug resamples with map_coordinates)
        import PIL.Image  # noqa: F401
    except ImportError:
        return None
    import importlib

    def unused(*a, **k):
        raise NotImplementedError("stand-in: not used on the path the golden generator calls")

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        return m

    saved_path, saved_flag, saved_modules = list(sys.path), sys.dont_write_bytecode, set(sys.modules)
    stubs = {"lzx.yolo.extensions.merge_bbs": module("lzx.yolo.extensions.merge_bbs", read_txt_single=unused, rec_img=unused,
                                                     xyxy_mult_imgshape=unused),
             "lzx.yolo.utils": module("lzx.yolo.utils", __path__=[]),
             "lzx.yolo.utils.general": module("lzx.yolo.utils.general", xywh2xyxy=unused, xyxy2xywhn=unused, xywhn2xyxy=unused,
                                              xyxy2xywh=unused),
             "lzx.yolo.utils.metrics": module("lzx.yolo.utils.metrics", bbox_iou=unused)}
    if importlib.util.find_spec("cv2") is None:
        stubs["cv2"] = module("cv2")
    try:
        sys.dont_write_bytecode = True
        for name, m in stubs.items():
            sys.modules.setdefault(name, m)
        sys.path.insert(0, root)
        return types.SimpleNamespace(xzaug=importlib.import_module("lzx.yolo.extensions.xzaug"),
                                     rollaug=importlib.import_module("lzx.yolo.extensions.rollaug"),
                                     padding2=importlib.import_module("lzx.yolo.extensions.padding2"))
    finally:
        sys.path[:] = saved_path
        sys.dont_write_bytecode = saved_flag
        for name in set(sys.modules) - saved_modules:
            if name == "lzx" or name.startswith("lzx.") or (name in stubs and sys.modules[name] is stubs[name]):
                del sys.modules[name]


def _flip(img, boxes):
    """mmcv.imflip(direction='horizontal') and mmdet RandomFlip.bbox_flip."""
    W = img.shape[1]
    f = boxes.copy()
    f[..., 0::4] = W - boxes[..., 2::4]
    f[..., 2::4] = W - boxes[..., 0::4]
    return np.ascontiguousarray(img[:, ::-1]), f


def _roll_glue(ref, img, boxes, labels, clip01, roll_dist=None):
    """RollAug.__call__ (transforms.py:1040-1064) with np.float -> np.float64; roll_dist None draws inside roll_aug_raw."""
    H, W = img.shape[:2]
    lab = boxes.astype(np.float64)
    lab[:, [0, 2]] /= W
    lab[:, [1, 3]] /= H
    lab = np.concatenate([labels[:, None], lab], 1)
    img, lab, shift = ref.rollaug.roll_aug_raw(img, lab, roll_dist=roll_dist, is_xyxy=True, clip01=clip01)
    labels = lab[:, 0]
    lab = lab[:, 1:]
    lab[:, [0, 2]] *= W
    lab[:, [1, 3]] *= H
    return img, np.round(lab).astype(np.float32), np.round(labels).astype(np.int64), shift


def _stretch_glue(ref, img, boxes, labels, kx=None, ky=None):
    """PanoStretch.__call__ (transforms.py:1002-1026): xzaug_xywh(is_xyxy=True) draws kx, ky in _xzaug; explicit kx, ky go to getAug."""
    lab = np.concatenate([labels[:, None], boxes], 1)
    if kx is None:
        img, lab = ref.xzaug.xzaug_xywh(img, lab, is_xyxy=True, kxy=KXY)
    else:
        img, pts = ref.xzaug.getAug(img, kx, ky, lab[:, 1:].copy().reshape([-1, 2]))
        lab = np.concatenate([lab[:, :1], pts.reshape([-1, 4])], 1)
    return img, np.round(lab[:, 1:]).astype(np.float32), np.round(lab[:, 0]).astype(np.int64)


def run_seeded(ref, img, boxes, labels, seed, n, chances, clip01=True):
    """n consecutive images through the three transforms with the global np.random seeded once, recording what was drawn."""
    drawn = []
    orig = ref.xzaug.getAug

    def spy(im, kx, ky, pts):
        drawn[-1].update(kx=kx, ky=ky)
        return orig(im, kx, ky, pts)

    ref.xzaug.getAug = spy
    out = []
    try:
        np.random.seed(seed)
        for _ in range(n):
            drawn.append(dict(stretch=False, kx=1.0, ky=1.0, roll=False, roll_dist=0.0, shift=0, flip=False))
            im, b, l = img.copy(), boxes.copy(), labels.copy()
            if np.random.rand() < chances[0]:
                drawn[-1]["stretch"] = True
                im, b, l = _stretch_glue(ref, im, b, l)
            if np.random.rand() < chances[1]:
                st = np.random.get_state()
                r = np.random.rand()
                np.random.set_state(st)
                drawn[-1].update(roll=True, roll_dist=(int(r * 100000) % 100000) / 100000)
                im, b, l, shift = _roll_glue(ref, im, b, l, clip01)
                drawn[-1]["shift"] = shift
            cur = np.random.choice(["horizontal", None], p=[chances[2], 1 - chances[2]])
            if cur is not None:
                drawn[-1]["flip"] = True
                im, b = _flip(im, b)
            out.append((np.ascontiguousarray(im), b, l))
    finally:
        ref.xzaug.getAug = orig
    return out, drawn


def run_explicit(ref, img, boxes, labels, stretch, kx, ky, roll_dist, flip, clip01=True):
    """One image with given parameters (roll_dist None: no roll).  Returns (image, boxes, labels, shift)."""
    im, b, l, shift = img.copy(), boxes.copy(), labels.copy(), 0
    if stretch:
        im, b, l = _stretch_glue(ref, im, b, l, kx, ky)
    if roll_dist is not None:
        im, b, l, shift = _roll_glue(ref, im, b, l, clip01, roll_dist)
    if flip:
        im, b = _flip(im, b)
    return np.ascontiguousarray(im), b, l, shift


EXTREMES = [  # stretch, kx, ky, roll_dist, flip, clip01
    (True, 2.0, 0.5, 0.0, False, True),
    (True, 0.5, 2.0, 0.99999, True, True),
    (False, 1.0, 1.0, 0.9999999, False, True),
    (False, 1.0, 1.0, 0.3, True, True),
    (False, 1.0, 1.0, 0.3, False, False),
    (True, 1.7, 0.6, 0.25, True, True),
    (True, 2.0, 0.5, None, True, True),
    (True, 0.5, 0.5 * 4.0, 0.6, False, False),
]


def generate(ref):
    d = {}
    cases = []
    for s, (H, W) in enumerate(SOURCES):
        img = source_image(H, W, 11 + s)
        boxes, labels = source_boxes(H, W)
        d[f"src{s}"], d[f"boxes{s}"], d[f"labels{s}"] = img, boxes, labels
        for combo in range(8):
            chances = (float(combo >> 2 & 1), float(combo >> 1 & 1), float(combo & 1))
            seed = 100 + 10 * s + combo
            (res,), (p,) = run_seeded(ref, img, boxes, labels, seed, 1, chances)
            cases.append((s, seed, 0, chances, True, p, res))
        seed, chances = 7 + s, (0.5, 0.5, 0.5)
        outs, ps = run_seeded(ref, img, boxes, labels, seed, 5, chances)
        for j, (res, p) in enumerate(zip(outs, ps)):
            cases.append((s, seed, j, chances, True, p, res))
        for stretch, kx, ky, rd, flip, clip01 in EXTREMES:
            im, b, l, shift = run_explicit(ref, img, boxes, labels, stretch, kx, ky, rd, flip, clip01)
            p = dict(stretch=stretch, kx=kx if stretch else 1.0, ky=ky if stretch else 1.0, roll=rd is not None,
                     roll_dist=0.0 if rd is None else (int(rd * 100000) % 100000) / 100000, shift=shift, flip=flip)
            cases.append((s, -1, 0, (np.nan,) * 3, clip01, p, (im, b, l)))
    n = len(cases)
    d["case_src"] = np.array([c[0] for c in cases], np.int64)
    d["case_seed"] = np.array([c[1] for c in cases], np.int64)
    d["case_pos"] = np.array([c[2] for c in cases], np.int64)
    d["case_chances"] = np.array([c[3] for c in cases], np.float64)
    d["case_clip01"] = np.array([c[4] for c in cases], bool)
    for key, dt in (("stretch", bool), ("kx", np.float64), ("ky", np.float64), ("roll", bool), ("roll_dist", np.float64),
                    ("shift", np.int64), ("flip", bool)):
        d["case_" + key] = np.array([c[5][key] for c in cases], dt)
    for k, c in enumerate(cases):
        im, b, l = c[6]
        d[f"img_dx{k}"], d[f"out_boxes{k}"], d[f"out_labels{k}"] = encode_dx(im), b.astype(np.float32), l.astype(np.int64)
    d["n_cases"] = np.array(n)
    d["kxy"] = np.array(KXY)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    ref = load_reference()
    if ref is None:
        print(f"reference not found under {REFERENCE_ROOT} (or scipy / PIL missing)", file=sys.stderr)
        return 1
    d = generate(ref)
    np.savez_compressed(a.out, **d)
    combos = {(bool(s), bool(r), bool(f)) for s, r, f in zip(d["case_stretch"], d["case_roll"], d["case_flip"])}
    merged = sum(not np.array_equal(np.sort(d[f"out_labels{k}"]), d[f"labels{d['case_src'][k]}"][np.argsort(d[f"labels{d['case_src'][k]}"])])
                 for k in range(int(d["n_cases"])))
    print(f"wrote {a.out}: {int(d['n_cases'])} cases, {len(combos)} of 8 on/off combinations, {merged} with merged boxes, "
          f"{os.path.getsize(a.out) / 1024:.0f} KiB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
