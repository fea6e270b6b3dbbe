#!/usr/bin/env python3
"""Time the detector's test-time post-processing: the HIP kernels against the definitions of detector.py run as torch ops on the same GPU.

    python tools/bench_detect.py [--reps 5] [--out profiles/detect_postprocess_bench.json]

Timing only; not part of bench.py.  The config's shapes (configs/_base_/models/mask_rcnn_swin_fpn.py): B = 8 images of 512 x 1024,
R = 1000 proposals, C = 80 classes, K = 100 detections per image.  Four rows, each with a `kernels` and a `torch` arm on the same inputs,
run in alternation (kernels, torch, kernels, ...), eager, timed with HIP events around one call:
    nms_typical   ops.multiclass_nms_batch / detector.detect_post on a score distribution with a few hundred candidates per image
    nms_worst     the same with every proposal above the threshold in every class and no box overlapping another of its class: all
                  R x C candidates survive (the torch arm is the definition's loop over classes and rows: one round)
    paste         ops.paste_masks / detector.paste_masks_batch, 100 detections per image
    heads_predict MiniMaskRCNN.heads_predict on random feature maps with the kernels, and with the definitions in their place
The torch arms read counts back to the host (the definitions have data-dependent shapes); that is part of what they cost.  Figures are
milliseconds per call, the median over the rounds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from panoswintransformerobjectdetection_amd import detector as det, ops  # noqa: E402

B, H, W, R, C, K = 8, 512, 1024, 1000, 80, 100
STDS = (0.1, 0.1, 0.2, 0.2)
DEV = "cuda:0"


def _time(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def _alternate(arms, reps):
    """arms: {name: (fn, rounds or None = reps)} -> {name: dict(rounds, median)}; one warm-up call each (not for an arm that is run for one
    round only: it takes a minute), then the arms in turn"""
    for fn, n in arms.values():
        if n is None:
            fn()
    times = {k: [] for k in arms}
    for i in range(reps):
        for k, (fn, n) in arms.items():
            if n is None or i < n:
                times[k].append(round(_time(fn), 3))
    return {k: dict(rounds=t, median=float(np.median(t))) for k, t in times.items()}


def nms_inputs(worst):
    g = torch.Generator().manual_seed(1)
    if worst:
        # 40 x 25 disjoint boxes, the same for every class.  80 classes cannot all be above 0.05 under one softmax (80 x 0.05 > 1), and the
        # kernels' contract is about candidates, not about the config's threshold: with score_thr = 0.002 and near-uniform logits every
        # (r, c) is a candidate, and every one survives
        gx, gy = torch.meshgrid(torch.arange(40.0), torch.arange(25.0), indexing="xy")
        x, y = gx.reshape(-1) * 25, gy.reshape(-1) * 20
        rois = torch.stack([x + 2, y + 2, x + 22, y + 18], 1)[None].repeat(B, 1, 1)
        deltas = torch.zeros(B, R, 4 * C)
        cls = torch.randn(B, R, C + 1, generator=g) * 0.3
        cls[:, :, C] = -4.0
        return rois, cls, deltas, 0.002
    c = torch.rand(B, R, 2, generator=g) * torch.tensor([W, H])
    wh = torch.rand(B, R, 2, generator=g) * torch.tensor([W / 4, H / 4]) + 8
    rois = torch.cat([c - wh / 2, c + wh / 2], -1).clamp(min=0)
    deltas = torch.randn(B, R, 4 * C, generator=g) * 0.5
    cls = torch.randn(B, R, C + 1, generator=g)
    cls[:, :, C] += 6.0                                                  # mostly background
    hot = torch.rand(B, R, generator=g) < 0.1
    cls[:, :, :8] += hot[:, :, None] * torch.rand(B, R, 8, generator=g) * 9
    return rois, cls, deltas, 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), shapes=dict(B=B, image=f"{H}x{W}", R=R, C=C, K=K), rounds=a.reps,
               unit="milliseconds per eager call (HIP events), median over the rounds; arms run in alternation")
    count = torch.full((B,), R, dtype=torch.int32, device=DEV)
    for name, worst in (("nms_typical", False), ("nms_worst", True)):
        rois, cls, deltas, thr = (t.to(DEV) if torch.is_tensor(t) else t for t in nms_inputs(worst))
        cls, deltas = cls.to(torch.bfloat16), deltas.to(torch.bfloat16)
        out = {}

        def kern():
            out["k"] = ops.multiclass_nms_batch(rois, count, cls, deltas, STDS, (H, W), None, thr, 0.5, K)

        def ref():
            out["t"] = det.detect_post(rois, count, cls, deltas, STDS, (H, W), None, thr, 0.5, K)

        r = _alternate({"kernels": (kern, None), "torch": (ref, 1 if worst else None)}, a.reps)
        cand = (torch.softmax(cls.float(), -1)[:, :, :C] > thr).sum((1, 2)).tolist()
        r.update(candidates_per_image=cand, detections=out["k"][3].tolist(), score_thr=thr,
                 same_selection=bool(torch.equal(out["k"][4], out["t"][4]) and torch.equal(out["k"][3], out["t"][3])))
        if worst:
            full = ops.multiclass_nms_batch(rois, count, cls, deltas, STDS, (H, W), None, thr, 0.5, 1024)
            r["survivors_at_least"] = full[3].tolist()
        res[name] = r
    # paste
    g = torch.Generator().manual_seed(2)
    logits = (3 * torch.randn(B * K, C, 28, 28, generator=g)).to(DEV, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, C, (B, K), generator=g).to(DEV)
    c = torch.rand(B, K, 2, generator=g) * torch.tensor([W, H])
    wh = torch.rand(B, K, 2, generator=g) * torch.tensor([W / 3, H / 3]) + 8
    boxes = torch.cat([c - wh / 2, c + wh / 2], -1).to(DEV)
    kcount = torch.full((B,), K, dtype=torch.int32, device=DEV)
    buf = torch.empty(B, K, H, W, dtype=torch.uint8, device=DEV)
    out = {}

    def kern_paste():
        out["k"] = ops.paste_masks(logits, labels, boxes, kcount, 0.5, (H, W), out=buf)

    def ref_paste():
        out["t"] = det.paste_masks_batch(logits, labels, boxes, kcount, 0.5, (H, W))

    r = _alternate({"kernels": (kern_paste, None), "torch": (ref_paste, None)}, a.reps)
    r.update(output_bytes=B * K * H * W, kernel_GBps=round(B * K * H * W / r["kernels"]["median"] / 1e6, 1),
             pixels_differing=int((out["k"] != out["t"]).sum()), pixels=B * K * H * W)
    res["paste"] = r
    del out, buf
    torch.cuda.empty_cache()
    # the whole heads_predict
    torch.manual_seed(0)
    m = det.MiniMaskRCNN(dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], ape=True), num_classes=C).to(DEV).eval()
    with torch.no_grad():
        m.bbox_head.cls.weight.mul_(300.0)
        m.bbox_head.cls.bias[C] += 16.0
    feats = [torch.randn(B, ch, H // s, W // s, device=DEV) for ch, s in zip(m.backbone.num_features, (4, 8, 16, 32))]
    out = {}

    def kern_heads():
        m.multiclass_nms, m.paste = det.multiclass_nms_batch, det.paste_masks_dispatch
        out["k"] = m.heads_predict(feats, (H, W))

    def ref_heads():
        m.multiclass_nms, m.paste = det.detect_post, det.paste_masks_batch
        out["t"] = m.heads_predict(feats, (H, W))

    r = _alternate({"kernels": (kern_heads, None), "torch": (ref_heads, None)}, a.reps)
    r.update(detections=out["k"].count.tolist())
    res["heads_predict"] = r
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
