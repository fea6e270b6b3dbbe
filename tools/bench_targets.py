#!/usr/bin/env python3
"""Time the detector's sampler, box targets and mask targets of a padded batch as hipGraph replays: the torch definitions run on the GPU
against the HIP kernels, and a captured padded MiniMaskRCNN.heads_loss (forward and backward of everything behind the backbone).

    python tools/bench_targets.py [--iters 50] [--reps 3] [--gmax 16 100] [--out profiles/targets_bench.json] [--label this]

Shapes: B = 8 images of 512 x 1024, PaddedTargets with Gmax = 16 and 100, 1-9 boxes per image (detector.synthetic_targets).
    rpn_targets   130,944 anchors, 128 + 256 slots          definition (detector.rpn_targets) | kernels (ops.rpn_targets)
    roi_targets   Gmax + 1,000 candidates, 128 + 384 slots  definition (detector.roi_targets) | kernels (ops.roi_targets)
    mask_targets  128 RoIs per image, 28 x 28 points        definition (detector.mask_targets) | kernels (ops.mask_targets)
    heads_loss    a captured step of the heads on PanoSwin-T feature maps (random), with the number of nodes of the captured graph
Each arm is captured once and replayed in turn, --reps rounds of --iters replays, in one process; figures are microseconds per replay
for the whole batch.  On a checkout that has no detector.rpn_targets only the heads_loss part runs: the tool is meant to be run on both
sides of a change to the heads."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from panoswintransformerobjectdetection_amd import detector as det  # noqa: E402

B, H, W, PROPOSALS = 8, 512, 1024, 1000
TCFG = dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], ape=True, drop_path_rate=0.0)
STDS = (0.1, 0.1, 0.2, 0.2)


def _capture(step, stream, keep_graph=False):
    with torch.cuda.stream(stream):
        for _ in range(2):
            step()
        stream.synchronize()
        g = torch.cuda.CUDAGraph(keep_graph=True) if keep_graph else torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            step()
        if keep_graph:
            g.instantiate()
    torch.cuda.synchronize()
    return g


def _node_count(g):
    """hipGraphGetNodes on the captured graph (a graph captured with keep_graph=True)"""
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_size_t(0)
    rc = hip.hipGraphGetNodes(ctypes.c_void_p(g.raw_cuda_graph()), None, ctypes.byref(n))
    return int(n.value) if rc == 0 else None


def _time(graphs, stream, iters, reps):
    times = {k: [] for k in graphs}
    with torch.cuda.stream(stream):
        for _ in range(reps):
            for k, gr in graphs.items():
                for _ in range(3):
                    gr.replay()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(iters):
                    gr.replay()
                e.record()
                stream.synchronize()
                times[k].append(round(s.elapsed_time(e) * 1e3 / iters, 1))
    return {k: dict(rounds=t, median=float(np.median(t)), spread=round(max(t) - min(t), 1)) for k, t in times.items()}


def _targets(Gmax, dev):
    tg = det.synthetic_targets(B, H, W, dev)
    T = det.PaddedTargets.allocate(B, Gmax, dev, mask_hw=(H, W))
    T.copy_from([t["boxes"] for t in tg], [t["labels"] for t in tg], [t["masks"] for t in tg])
    return T


def bench_ops(Gmax, side, a):
    from panoswintransformerobjectdetection_amd import ops
    dev = "cuda:0"
    T = _targets(Gmax, dev)
    shapes = [(H // s, W // s) for s in det.MiniMaskRCNN.STRIDES]
    anchors = torch.cat(det.make_anchors(shapes, det.MiniMaskRCNN.STRIDES, dev), 0)
    g = torch.Generator("cpu").manual_seed(0)
    c = torch.rand(B, PROPOSALS, 2, generator=g) * torch.tensor([W, H])
    wh = torch.rand(B, PROPOSALS, 2, generator=g) * torch.tensor([W / 3, H / 3]) + 4
    cand = torch.cat([T.boxes, torch.cat([c - wh / 2, c + wh / 2], -1).to(dev)], 1)
    inds_rpn = det.max_iou_assign_batch(anchors, T.boxes, T.count, 0.7, 0.3, 0.3, True)[0]
    inds_roi = det.max_iou_assign_batch(cand, T.boxes, T.count, 0.5, 0.5, 0.5, True, lead_gt=Gmax)[0]
    key_rpn, key_roi = torch.rand(inds_rpn.shape, device=dev), torch.rand(inds_roi.shape, device=dev)
    out = {}
    rois, _, _, pos_valid, gt_idx = ops.roi_targets(inds_roi, key_roi, cand, T.boxes, T.labels, 80, 128, 512, STDS)
    rois_p = rois[:, :128].contiguous()

    def arm(name, fn, *args):
        def step():
            out[name] = fn(*args)
        return step

    steps = {"rpn_targets_definition": arm("rd", det.rpn_targets, inds_rpn, key_rpn, anchors, T.boxes, 128, 256),
             "rpn_targets_kernels": arm("rk", ops.rpn_targets, inds_rpn, key_rpn, anchors, T.boxes, 128, 256),
             "roi_targets_definition": arm("od", det.roi_targets, inds_roi, key_roi, cand, T.boxes, T.labels, 80, 128, 512, STDS),
             "roi_targets_kernels": arm("ok", ops.roi_targets, inds_roi, key_roi, cand, T.boxes, T.labels, 80, 128, 512, STDS),
             "mask_targets_definition": arm("md", det.mask_targets, T.masks, rois_p, gt_idx, pos_valid, 28),
             "mask_targets_kernels": arm("mk", ops.mask_targets, T.masks, rois_p, gt_idx, pos_valid, 28)}
    graphs = {k: _capture(f, side) for k, f in steps.items()}
    with torch.cuda.stream(side):
        for gr in graphs.values():
            gr.replay()
        side.synchronize()
        differ = dict(rpn_idx=int((out["rd"][0] != out["rk"][0]).sum()), roi_labels=int((out["od"][1] != out["ok"][1]).sum()),
                      mask_points=int((out["md"] != out["mk"]).sum()))
    res = _time(graphs, side, a.iters, a.reps)
    res["entries_differing_from_the_definition_on_the_gpu"] = differ
    return res


def bench_heads(Gmax, side, a):
    dev = "cuda:0"
    with torch.cuda.stream(side):
        torch.manual_seed(0)
        m = det.MiniMaskRCNN(dict(TCFG, compute_dtype=torch.float32), num_classes=80).to(dev).train()
        heads = m.head_parameters()
        feats = [torch.randn(B, ch, H // s, W // s, device=dev) for ch, s in zip(m.backbone.num_features, (4, 8, 16, 32))]
        T = _targets(Gmax, dev)
        state = {}

        def step():
            for p in heads:
                p.grad = None
            ls = m.heads_loss(feats, T, (H, W))
            sum(ls.values()).backward()
            state["loss"] = torch.stack([ls[k] for k in sorted(ls)])

        g = _capture(step, side, keep_graph=True)
    res = _time({"heads_loss_padded": g}, side, max(a.iters // 5, 5), a.reps)
    res["heads_loss_padded"]["graph_nodes"] = _node_count(g)
    res["heads_loss_padded"]["losses"] = [round(v, 5) for v in state["loss"].tolist()]
    del g, m, feats, T
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gmax", type=int, nargs="+", default=[16, 100])
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = dict(label=a.label, device=torch.cuda.get_device_name(0), batch=B, image=f"{H}x{W}", iters_per_round=a.iters, rounds=a.reps,
               unit="microseconds per graph replay for the whole batch", has_target_ops=hasattr(det, "rpn_targets"))
    for Gmax in a.gmax:
        r = {}
        if res["has_target_ops"]:
            r.update(bench_ops(Gmax, side, a))
            torch.cuda.empty_cache()
        r.update(bench_heads(Gmax, side, a))
        res[f"Gmax_{Gmax}"] = r
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
