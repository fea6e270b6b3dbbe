#!/usr/bin/env python3
"""Time test-time augmentation behind the backbone: tta.aug_heads_predict as a graph replay, each new kernel alone, and the torch
definitions of tta.py on the same GPU.

    python tools/bench_augtest.py [--reps 7] [--batches 1,8] [--views 2,6] [--out profiles/aug_test_bench.json]

Timing only; not part of bench.py.  The config's shapes: images of 512 x 1024, R = 1000 proposals, C = 80 classes, K = 100 detections per
image; V = 2 is (the image, its flip), V = 6 is 3 scales (0.75, 1, 1.25) x flip.  Per (B, V):
    aug_heads_predict   MiniMaskRCNN on random feature pyramids, captured once (graph.GraphedCallable) and replayed; beside it the same call
                        eager, and the per-view heads_predict replayed V times (what the views cost without any merge)
    merge_proposals, map_rois, merge_bboxes, nms_boxes, paste_masks_aug
                        one call of the ops wrapper (`kernels`) against the definition run as torch ops on the same inputs (`torch`), in
                        alternation, eager, HIP events around the call.  The definitions read counts back to the host and loop over rows
                        (data-dependent shapes); that is part of what they cost.  The torch arm of merge_proposals and nms_boxes runs for
                        two rounds only (seconds per call).
Figures are milliseconds per call: the median over the rounds, with every round kept (the spread is theirs)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from panoswintransformerobjectdetection_amd import detector as det, ops, tta  # noqa: E402
from panoswintransformerobjectdetection_amd.graph import GraphedCallable  # noqa: E402

H, W, R, C, K = 512, 1024, 1000, 80, 100
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
    """arms: {name: (fn, rounds or None = reps)} -> {name: dict(rounds, median)}; one warm-up call of every full arm, then the arms in turn"""
    for fn, n in arms.values():
        if n is None:
            fn()
    times = {k: [] for k in arms}
    for i in range(reps):
        for k, (fn, n) in arms.items():
            if n is None or i < n:
                times[k].append(round(_time(fn), 3))
    return {k: dict(rounds=t, median=float(np.median(t))) for k, t in times.items()}


def views_of(V):
    scales = [1.0] if V == 2 else [0.75, 1.0, 1.25]
    out = []
    for s in scales:
        h, w = int(H * s + 0.5), int(W * s + 0.5)
        sf = (float(np.float32(w / W)), float(np.float32(h / H)))
        out += [tta.View((h, w), sf + sf, False), tta.View((h, w), sf + sf, True)]
    return out


def kernel_rows(B, V, views, reps, g):
    res = {}
    # proposals of every view: boxes around shared centres, so that views overlap
    centres = torch.rand(B, 1, R, 2, generator=g) * torch.tensor([W - 40.0, H - 40.0]) + 20
    wh = torch.rand(B, 1, R, 2, generator=g) * torch.tensor([W / 5, H / 5]) + 8
    ori = (torch.cat([centres - wh / 2, centres + wh / 2], -1) + torch.randn(B, V, R, 4, generator=g) * 6).permute(1, 0, 2, 3).clamp(min=0)
    props = torch.stack([tta.map_to_view(ori[v], views[v]) for v in range(V)]).to(DEV).contiguous()
    scores = torch.sort(torch.rand(V, B, R, generator=g), -1, descending=True)[0].to(DEV)
    count = torch.randint(R // 2, R + 1, (V, B), generator=g).to(DEV, torch.int32)
    out = {}
    r = _alternate({"kernels": (lambda: out.__setitem__("k", ops.aug_merge_proposals(props, scores, count, views, 0.7, R)), None),
                    "torch": (lambda: out.__setitem__("t", tta.merge_aug_proposals(props, scores, count, views, 0.7, R)), 2)}, reps)
    r.update(candidates=count.sum(0).tolist(), survivors=out["k"][2].tolist(), launches=ops.aug_merge_proposals_launches(V, R, R),
             same_rows=bool(torch.equal(out["k"][0], out["t"][0]) and torch.equal(out["k"][2], out["t"][2])))
    res["merge_proposals"] = r
    rois, roi_count = out["k"][0], out["k"][2]
    r = _alternate({"kernels": (lambda: out.__setitem__("mk", ops.aug_map_rois(rois, views)), None),
                    "torch": (lambda: out.__setitem__("mt", torch.stack([tta.map_to_view(rois, v) for v in views])), None)}, reps)
    r.update(same_bits=bool(torch.equal(out["mk"], out["mt"])))
    res["map_rois"] = r
    rois_v = list(out["mk"].unbind(0))
    cls_v = [(torch.randn(B, R, C + 1, generator=g) + torch.tensor([0.0] * C + [6.0])).to(DEV, torch.bfloat16) for _ in range(V)]
    hot = (torch.rand(B, R, generator=g) < 0.1).to(DEV)
    for c in cls_v:
        c[:, :, :8] += (hot[:, :, None] * 8).to(torch.bfloat16)
    deltas_v = [(torch.randn(B, R, 4 * C, generator=g) * 0.5).to(DEV, torch.bfloat16) for _ in range(V)]
    r = _alternate({"kernels": (lambda: out.__setitem__("bk", ops.aug_merge_bboxes(rois_v, cls_v, deltas_v, STDS, views)), None),
                    "torch": (lambda: out.__setitem__("bt", tta.merge_aug_bboxes(rois_v, cls_v, deltas_v, STDS, views)), None)}, reps)
    nbytes = V * B * R * (16 + (C + 1) * 2 + 4 * C * 2) + B * R * (4 * C + C + 1) * 4
    r.update(bytes=nbytes, kernel_GBps=round(nbytes / r["kernels"]["median"] / 1e6, 1),
             max_box_difference_px=float((out["bk"][0] - out["bt"][0]).abs().max()), max_score_difference=float((out["bk"][1] - out["bt"][1]).abs().max()))
    res["merge_bboxes"] = r
    mb, ms = out["bk"]
    r = _alternate({"kernels": (lambda: out.__setitem__("nk", ops.multiclass_nms_boxes_batch(mb, ms, roi_count, 0.05, 0.5, K)), None),
                    "torch": (lambda: out.__setitem__("nt", tta.nms_merged(mb, ms, roi_count, 0.05, 0.5, K)), 2)}, reps)
    r.update(detections=out["nk"][3].tolist(), same_selection=bool(torch.equal(out["nk"][4], out["nt"][4]) and torch.equal(out["nk"][3], out["nt"][3])))
    res["nms_boxes"] = r
    boxes, _, labels, kcount, _ = out["nk"]
    logits = [(3 * torch.randn(B * K, C, 28, 28, generator=g)).to(DEV, torch.bfloat16).contiguous(memory_format=torch.channels_last) for _ in range(V)]
    flips = [v.flip for v in views]
    buf = torch.empty(B, K, H, W, dtype=torch.uint8, device=DEV)

    def torch_paste():
        prob = tta.merge_aug_masks(logits, flips, labels).reshape(B, K, 28, 28)
        o = torch.zeros(B, K, H, W, dtype=torch.uint8, device=DEV)
        for b, n in enumerate(kcount.tolist()):
            if n:
                o[b, :n] = det.paste_masks(prob[b, :n], boxes[b, :n], H, W, 0.5).to(torch.uint8)
        out["pt"] = o

    r = _alternate({"kernels": (lambda: out.__setitem__("pk", ops.paste_masks_aug(logits, flips, labels, boxes, kcount, 0.5, (H, W), out=buf)), None),
                    "torch": (torch_paste, None)}, reps)
    r.update(output_bytes=B * K * H * W, kernel_GBps=round(B * K * H * W / r["kernels"]["median"] / 1e6, 1),
             pixels_differing=int((out["pk"] != out["pt"]).sum()), pixels=B * K * H * W)
    res["paste_masks_aug"] = r
    return res


def heads_row(B, V, views, reps, g):
    torch.manual_seed(0)
    m = det.MiniMaskRCNN(dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], ape=True), num_classes=C).to(DEV).eval()
    with torch.no_grad():
        m.bbox_head.cls.weight.mul_(300.0)
        m.bbox_head.cls.bias[C] += 16.0
    feats_list = [[torch.randn(B, ch, -(-v.img_hw[0] // s), -(-v.img_hw[1] // s), generator=g).to(DEV) for ch, s in zip(m.backbone.num_features, (4, 8, 16, 32))]
                  for v in views]
    side = torch.cuda.Stream()
    state = {}

    def aug():
        state["aug"] = m.aug_heads_predict(feats_list, views, ori_hw=(H, W))
        return state["aug"].count

    def singles():
        state["one"] = [m.heads_predict(f, v.img_hw) for f, v in zip(feats_list, views)]
        return state["one"][0].count

    with torch.cuda.stream(side):
        g_aug = GraphedCallable(aug, warmup=2, stream=side, parameters=[])
        g_one = GraphedCallable(singles, warmup=2, stream=side, parameters=[])
        r = _alternate({"aug_replay": (g_aug, None), "views_simple_test_replay": (g_one, None), "aug_eager": (aug, None)}, reps)
    side.synchronize()
    r.update(detections=state["aug"].count.tolist(), merge_share_of_replay=round(1 - r["views_simple_test_replay"]["median"] / r["aug_replay"]["median"], 3))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--views", default="2,6")
    ap.add_argument("--skip-heads", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), shapes=dict(image=f"{H}x{W}", R=R, C=C, K=K), rounds=a.reps,
               unit="milliseconds per call (HIP events); median over the rounds, every round listed; arms run in alternation")
    for B in (int(v) for v in a.batches.split(",")):
        for V in (int(v) for v in a.views.split(",")):
            views = views_of(V)
            g = torch.Generator().manual_seed(10 * B + V)
            row = kernel_rows(B, V, views, a.reps, g)
            torch.cuda.empty_cache()
            row["aug_heads_predict"] = "not measured" if a.skip_heads else heads_row(B, V, views, a.reps, g)
            torch.cuda.empty_cache()
            res[f"B{B}_V{V}"] = row
            print(json.dumps({f"B{B}_V{V}": row}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
