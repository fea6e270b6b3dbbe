#!/usr/bin/env python3
"""Write tests/golden/aug_test.npz: what the reference's test-time-augmentation merges return for small fixed inputs.

Build machine only: it needs the reference tree (PSWIN_REFERENCE_ROOT, default /root/reference).  Two of the reference's files are imported
from where they lie, with empty stand-in packages around them so that no __init__.py of mmdet runs (the technique and the helpers of
tools/gen_detect_golden.py); no reference file is copied:

  (a) mmdet/core/bbox/transforms.py -- bbox_mapping and bbox_mapping_back on 24 boxes, unflipped and flipped, with the scale factors 1,
      0.5, 1.5 and (1333 / 2000, 800 / 1200) as float32 (dyadic and non-dyadic: the division's rounding is what is pinned).
  (b) mmdet/core/post_processing/merge_augs.py -- merge_aug_bboxes for V = 1, 2, 3, 4 and 6 views on the per-view boxes and scores that
      the definition's own first half yields (softmax and detector.decode_deltas_per_class, pinned by tests/golden/detect_post.npz);
      merge_aug_masks for N = 1, 2, 3 and 6 sources with mixed flips; merge_aug_proposals for V = 2 and 3 with max_per_img below and above
      the number of survivors, a flipped twin that maps back onto an identical box, and tied scores.
      mmcv.ops.nms is NOT in the reference tree: it is supplied by a stand-in written from its documented behaviour (the sequential rule
      in descending, stable score order; as tools/gen_detect_golden.py).  The NMS proper is therefore UNPINNED: only the reference's
      mapping back, concatenation, re-sort and cut are exercised.  mmcv.ConfigDict is a small attribute dict.

Nothing under the reference root is written (no bytecode either).  A case is written only if the CPU definition in
panoswintransformerobjectdetection_amd/tta.py reproduces it: bit for bit, except merge_aug_bboxes at V = 6, where torch's own summation
order is not the sequential one and each element must lie within (V - 1) * 2^-24 * sum|terms| / V plus one rounding of the result.

    python tools/gen_augtest_golden.py [--out tests/golden/aug_test.npz]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from gen_detect_golden import REFERENCE_ROOT, _greedy, _load_file, _module, _package, _with_stubs, write_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "aug_test.npz")
ABOUT = ("Reference results for tta.map_to_view / map_back / merge_aug_bboxes / merge_aug_masks / merge_aug_proposals "
         "(tools/gen_augtest_golden.py).  view_*: the geometry of the 8 views (hw, scale factor as float32, flip).  map_*: bbox_mapping and "
         "bbox_mapping_back of map_boxes in every view.  bbox_*: merge_aug_bboxes over the first V of the views listed in bbox_views_V, on "
         "the definition's own per-view softmax and decode of bbox_rois_V / bbox_cls / bbox_deltas; V <= 4 bit for bit, V = 6 in torch's "
         "own summation order.  mask_*: merge_aug_masks (np.mean) of sigmoid(mask_logits_q / 64) of the first N sources with mask_flips, "
         "the label's channel only.  prop_*: merge_aug_proposals with a STAND-IN for mmcv.ops.nms (not in the reference tree; the "
         "sequential rule in descending stable score order): the NMS proper is UNPINNED, only the reference's mapping back, "
         "concatenation, re-sort and cut are exercised.")
STDS = (0.1, 0.1, 0.2, 0.2)
F32 = np.float32
VIEWS = [((64, 128), (1.0, 1.0, 1.0, 1.0), False), ((64, 128), (1.0, 1.0, 1.0, 1.0), True),
         ((32, 64), (0.5, 0.5, 0.5, 0.5), False), ((32, 64), (0.5, 0.5, 0.5, 0.5), True),
         ((96, 192), (1.5, 1.5, 1.5, 1.5), False), ((96, 192), (1.5, 1.5, 1.5, 1.5), True),
         ((43, 85), (float(F32(1333 / 2000)), float(F32(800 / 1200)), float(F32(1333 / 2000)), float(F32(800 / 1200))), False),
         ((43, 85), (float(F32(1333 / 2000)), float(F32(800 / 1200)), float(F32(1333 / 2000)), float(F32(800 / 1200))), True)]


class ConfigDict(dict):
    """stand-in of mmcv.ConfigDict: a dict with attribute access, nested dicts converted"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        for key, v in list(self.items()):
            if isinstance(v, dict) and not isinstance(v, ConfigDict):
                self[key] = ConfigDict(v)

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = value


def nms_stand_in(boxes, scores, iou_threshold, offset=0):
    """mmcv.ops.nms as documented: (dets [k, 5] in descending score, inds [k])"""
    order = torch.sort(scores, descending=True, stable=True)[1]
    keep = order[_greedy(boxes[order], iou_threshold)]
    return torch.cat([boxes[keep], scores[keep, None]], -1), keep


def load_reference(root=REFERENCE_ROOT):
    """(transforms module, merge_augs module) of the reference, or None when its tree is not on this machine"""
    mmdet = os.path.join(root, "mmdet")
    f_tr = os.path.join(mmdet, "core", "bbox", "transforms.py")
    f_ma = os.path.join(mmdet, "core", "post_processing", "merge_augs.py")
    if not (os.path.isfile(f_tr) and os.path.isfile(f_ma)):
        return None
    tr = _with_stubs({}, lambda: _load_file(f_tr, "_pswin_ref_transforms"))
    mmcv = _package("mmcv", None)
    mmcv.ConfigDict = ConfigDict
    ma = _with_stubs({
        "mmcv": mmcv, "mmcv.ops": _module("mmcv.ops", nms=nms_stand_in),
        "mmdet": _package("mmdet", None), "mmdet.core": _package("mmdet.core", None),
        "mmdet.core.bbox": _module("mmdet.core.bbox", bbox_mapping_back=tr.bbox_mapping_back),
        "mmdet.core.post_processing": _package("mmdet.core.post_processing", os.path.join(mmdet, "core", "post_processing")),
    }, lambda: importlib.import_module("mmdet.core.post_processing.merge_augs"))
    return tr, ma


def refuse(what):
    raise SystemExit(f"refused: the CPU definition does not reproduce the reference: {what}")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(np.asarray(a, F32)), np.ascontiguousarray(np.asarray(b, F32))
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def meta(view):
    hw, sf, flip = view
    return dict(img_shape=(hw[0], hw[1], 3), scale_factor=np.array(sf, F32), flip=flip, flip_direction="horizontal")


def bbox_inputs(views, R=16, C=3, seed=41):
    """per view: rois in the view's pixels (multiples of 0.25), logits and deltas; one delta past the width clip, one box over the border"""
    g = torch.Generator().manual_seed(seed)
    rois, cls, deltas = [], [], []
    for hw, sf, flip in views:
        c = torch.rand(R, 2, generator=g) * torch.tensor([float(hw[1]), float(hw[0])])
        wh = torch.rand(R, 2, generator=g) * torch.tensor([hw[1] / 3.0, hw[0] / 3.0]) + 2
        r = torch.round(torch.cat([c - wh / 2, c + wh / 2], 1).clamp(min=0) * 4) / 4
        d = torch.randn(R, 4 * C, generator=g) * 2
        d[0, 2], d[1, 7] = 60.0, -60.0
        r[2] = torch.tensor([hw[1] - 6.0, hw[0] - 5.0, hw[1] - 1.0, hw[0] - 1.0])
        d[2, 0:4] = torch.tensor([4.0, 4.0, 3.0, 3.0])
        rois.append(r)
        cls.append(2 * torch.randn(R, C + 1, generator=g))
        deltas.append(d)
    return torch.stack(rois)[:, None], torch.stack(cls)[:, None], torch.stack(deltas)[:, None]      # [V, 1, R, .]


def bbox_bound(tta, det, rois, cls, deltas, views):
    """the V = 6 bound per element: (V - 1) * 2^-24 * sum|terms| / V + one rounding (half an ulp) of the result; (boxes, scores)"""
    V = len(views)
    tb = ts = 0
    for v in range(V):
        B, R, C = cls[v].shape[0], cls[v].shape[1], cls[v].shape[2] - 1
        ts = ts + torch.softmax(cls[v], -1).abs().double()
        bx = det.decode_deltas_per_class(rois[v].reshape(B * R, 4), deltas[v].reshape(B * R, 4 * C), STDS, views[v].img_hw)
        tb = tb + tta.map_back(bx, views[v]).reshape(B, R, 4 * C).abs().double()
    eps = 2.0 ** -24
    return (V - 1) * eps * tb / V + eps * tb / V, (V - 1) * eps * ts / V + eps * ts / V


def prop_inputs(V, seed):
    """aug_proposals of V views (views 0, 1 and 2 of VIEWS: identity, its flip, half scale) for one image: per view n_v <= P rows in the
    view's pixels.  Row 0 of view 1 is the flipped twin of row 0 of view 0; rows 3 and 4 of view 0 and row 2 of view 1 share one score."""
    g = torch.Generator().manual_seed(seed)
    P, ns = 24, [24, 17, 20][:V]
    props, scores = torch.zeros(V, 1, P, 4), torch.zeros(V, 1, P)
    for v in range(V):
        hw = VIEWS[v][0]
        c = torch.rand(P, 2, generator=g) * torch.tensor([float(hw[1]), float(hw[0])])
        wh = torch.rand(P, 2, generator=g) * torch.tensor([hw[1] / 2.5, hw[0] / 2.5]) + 3
        props[v, 0] = torch.round(torch.cat([c - wh / 2, c + wh / 2], 1).clamp(min=0) * 4) / 4
        scores[v, 0] = torch.sort(torch.rand(P, generator=g), descending=True)[0]
    props[0, 0, 0] = torch.tensor([10.0, 20.0, 50.0, 60.0])
    props[1, 0, 0] = torch.tensor([128 - 50.0, 20.0, 128 - 10.0, 60.0])
    scores[1, 0, 0] = scores[0, 0, 0] * 0.5 + 0.5
    scores[0, 0, 4] = scores[0, 0, 3]
    scores[1, 0, 2] = scores[0, 0, 3]
    return props, scores, torch.tensor(ns, dtype=torch.int32)[:, None]


def generate(ref):
    from panoswintransformerobjectdetection_amd import detector as det
    from panoswintransformerobjectdetection_amd import tta
    tr, ma = ref
    views = [tta.View(*v) for v in VIEWS]
    d = {"_about": np.array(ABOUT), "view_hw": np.array([v[0] for v in VIEWS], np.int64), "view_scale": np.array([v[1] for v in VIEWS], F32),
         "view_flip": np.array([v[2] for v in VIEWS], np.bool_)}
    # (a) the mappings
    g = torch.Generator().manual_seed(40)
    c = torch.rand(24, 2, generator=g) * torch.tensor([128.0, 64.0])
    wh = torch.rand(24, 2, generator=g) * 40 + 1
    boxes = torch.cat([c - wh / 2, c + wh / 2], 1).float()
    to, back = [], []
    for raw, view in zip(VIEWS, views):
        m = meta(raw)
        a = tr.bbox_mapping(boxes, m["img_shape"], m["scale_factor"], m["flip"], m["flip_direction"])
        b = tr.bbox_mapping_back(boxes, m["img_shape"], m["scale_factor"], m["flip"], m["flip_direction"])
        if not bits_equal(tta.map_to_view(boxes, view), a) or not bits_equal(tta.map_back(boxes, view), b):
            refuse(f"bbox_mapping / bbox_mapping_back in {view}")
        wide = boxes.reshape(6, 16)                                  # [..., 4 k] rows, as the merged [R, 4 C] boxes
        if not bits_equal(tta.map_back(wide, view), tr.bbox_mapping_back(wide, m["img_shape"], m["scale_factor"], m["flip"], m["flip_direction"])):
            refuse(f"bbox_mapping_back on [R, 4 C] rows in {view}")
        to.append(a.numpy())
        back.append(b.numpy())
    d.update(map_boxes=boxes.numpy(), map_to=np.stack(to), map_back=np.stack(back))
    # (b) merge_aug_bboxes
    for V, ids in ((1, [6]), (2, [0, 1]), (3, [0, 3, 4]), (4, [7, 2, 1, 4]), (6, [0, 1, 2, 3, 6, 7])):
        vs = [views[i] for i in ids]
        rois, cls, deltas = bbox_inputs([VIEWS[i] for i in ids], seed=41 + V)
        aug_b, aug_s = [], []
        for v in range(V):
            aug_s.append(torch.softmax(cls[v, 0], -1))
            aug_b.append(det.decode_deltas_per_class(rois[v, 0], deltas[v, 0], STDS, vs[v].img_hw))
        wb, wsc = ma.merge_aug_bboxes(aug_b, aug_s, [[meta(VIEWS[i])] for i in ids], None)
        mb, ms = tta.merge_aug_bboxes(rois, cls, deltas, STDS, vs)
        if V <= 4:
            if not bits_equal(mb[0], wb) or not bits_equal(ms[0], wsc):
                refuse(f"merge_aug_bboxes, V = {V}")
        else:
            bb, bs = bbox_bound(tta, det, rois, cls, deltas, vs)
            if bool(((mb[0].double() - wb.double()).abs() > bb[0]).any()) or bool(((ms[0].double() - wsc.double()).abs() > bs[0]).any()):
                refuse(f"merge_aug_bboxes, V = {V}: outside the bound of the two summation orders")
        d.update({f"bbox_views_{V}": np.array(ids, np.int64), f"bbox_rois_{V}": rois.numpy(), f"bbox_cls_{V}": cls.numpy(),
                  f"bbox_deltas_{V}": deltas.numpy(), f"bbox_merged_boxes_{V}": wb.numpy(), f"bbox_merged_scores_{V}": wsc.numpy()})
    # merge_aug_masks
    g = torch.Generator().manual_seed(47)
    n, C = 4, 2
    q = torch.round(3 * torch.randn(6, n, C, 28, 28, generator=g) * 64).to(torch.int16)
    labels = torch.randint(0, C, (1, n), generator=g)
    flips = [False, True, True, False, True, False]
    d.update(mask_logits_q=q.numpy(), mask_labels=labels.numpy(), mask_flips=np.array(flips, np.bool_))
    for N in (1, 2, 3, 6):
        logits = [q[s].float() / 64 for s in range(N)]
        metas = [[dict(flip=flips[s], flip_direction="horizontal")] for s in range(N)]
        want = ma.merge_aug_masks([l.sigmoid().cpu().numpy() for l in logits], metas, None)
        want = np.asarray(want)[np.arange(n), labels[0].numpy()]
        if want.dtype != F32 or not bits_equal(tta.merge_aug_masks(logits, flips[:N], labels), want):
            refuse(f"merge_aug_masks, N = {N}")
        d[f"mask_merged_{N}"] = want
    # merge_aug_proposals
    for V in (2, 3):
        props, scores, count = prop_inputs(V, 50 + V)
        vs = views[:V]
        aug = [torch.cat([props[v, 0, :int(count[v, 0])], scores[v, 0, :int(count[v, 0]), None]], 1) for v in range(V)]
        full = ma.merge_aug_proposals(aug, [meta(VIEWS[v]) for v in range(V)], ConfigDict(nms=dict(type="nms", iou_threshold=0.7), max_per_img=1000))
        n_keep = full.shape[0]
        if not 8 < n_keep < int(count.sum()):
            refuse(f"merge_aug_proposals, V = {V}: the case needs suppressed and surviving rows, got {n_keep} of {int(count.sum())}")
        d.update({f"prop_boxes_{V}": props.numpy(), f"prop_scores_{V}": scores.numpy(), f"prop_count_{V}": count.numpy(),
                  f"prop_max_per_img_{V}": np.array([n_keep - 5, n_keep, n_keep + 7], np.int64)})
        for i, m in enumerate((n_keep - 5, n_keep, n_keep + 7)):
            want = ma.merge_aug_proposals(aug, [meta(VIEWS[v]) for v in range(V)], ConfigDict(nms=dict(type="nms", iou_threshold=0.7), max_per_img=m))
            r, s, k = tta.merge_aug_proposals(props, scores, count, vs, 0.7, m)
            k = int(k[0])
            if k != want.shape[0] or not bits_equal(r[0, :k], want[:, :4]) or not bits_equal(s[0, :k], want[:, 4]) or r[0, k:].any() or s[0, k:].any():
                refuse(f"merge_aug_proposals, V = {V}, max_per_img = {m}")
            d[f"prop_merged_{V}_{i}"] = want.numpy()
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
    write_npz(a.out, d)
    print(f"wrote {a.out}: {len(d)} arrays, {os.path.getsize(a.out) / 1024:.1f} KiB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
