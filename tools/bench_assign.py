#!/usr/bin/env python3
"""Time the detector's target assignment as hipGraph replays: the per-image torch assigner against the batched HIP kernels.

    python tools/bench_assign.py [--iters 200] [--reps 5] [--out profiles/assign_bench.json]

Both stages of the BASELINE.json configs[2] shape (2 x 512 x 1024): the RPN stage assigns the 130,944 anchors of the five pyramid levels,
the RoI stage cat(gt, 1,000 proposals); the images carry 1-9 boxes (detector.synthetic_targets).
    torch    detector.max_iou_assign image by image on [G, 4] boxes (the list form of the targets: G is frozen into the capture)
    kernels  detector.max_iou_assign_batch on PaddedTargets buffers with Gmax = 16 (pswin_max_iou_assign: two launches per stage)
Each arm is captured once and replayed in turn (torch, kernels, torch, ...), --reps rounds of --iters replays, in one process; the
figure is microseconds per replay of one stage for the whole batch.  Before timing, the kernels' gt_inds are compared with the torch
arm's (on HIP tensors torch's max does not promise the lowest index among equal IoUs, so a mismatch is reported, not asserted)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from panoswintransformerobjectdetection_amd import detector as det  # noqa: E402

B, H, W, GMAX, PROPOSALS = 2, 512, 1024, 16, 1000


def _graph(step, stream):
    with torch.cuda.stream(stream):
        for _ in range(2):
            step()
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            step()
    torch.cuda.synchronize()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    tg = det.synthetic_targets(B, H, W, dev)
    T = det.PaddedTargets.allocate(B, GMAX, dev)
    T.copy_from([t["boxes"] for t in tg], [t["labels"] for t in tg])
    shapes = [(H // s, W // s) for s in det.MiniMaskRCNN.STRIDES]
    anchors = torch.cat(det.make_anchors(shapes, det.MiniMaskRCNN.STRIDES, dev), 0)
    g = torch.Generator("cpu").manual_seed(0)
    c = torch.rand(B, PROPOSALS, 2, generator=g) * torch.tensor([W, H])
    wh = torch.rand(B, PROPOSALS, 2, generator=g) * torch.tensor([W / 3, H / 3]) + 4
    props = torch.cat([c - wh / 2, c + wh / 2], -1).to(dev)
    cand_list = [torch.cat([t["boxes"], props[b]], 0) for b, t in enumerate(tg)]
    cand_pad = torch.cat([T.boxes, props], 1)
    stages = {"rpn": dict(N=int(anchors.shape[0]), thr=(0.7, 0.3, 0.3, True)), "roi": dict(N=PROPOSALS + GMAX, thr=(0.5, 0.5, 0.5, True))}
    out = {}

    def torch_rpn():
        out["torch_rpn"] = [det.max_iou_assign(anchors, t["boxes"], *stages["rpn"]["thr"]) for t in tg]

    def torch_roi():
        out["torch_roi"] = [det.max_iou_assign(cand_list[b], t["boxes"], *stages["roi"]["thr"]) for b, t in enumerate(tg)]

    def kern_rpn():
        out["kern_rpn"] = det.max_iou_assign_batch(anchors, T.boxes, T.count, *stages["rpn"]["thr"])[0]

    def kern_roi():
        out["kern_roi"] = det.max_iou_assign_batch(cand_pad, T.boxes, T.count, *stages["roi"]["thr"], lead_gt=GMAX)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    steps = {"torch_rpn": torch_rpn, "kernels_rpn": kern_rpn, "torch_roi": torch_roi, "kernels_roi": kern_roi}
    graphs = {k: _graph(f, side) for k, f in steps.items()}
    with torch.cuda.stream(side):
        for gr in graphs.values():
            gr.replay()
        side.synchronize()
        counts = T.count.tolist()
        mismatch = {"rpn": sum(int((out["kern_rpn"][b] != out["torch_rpn"][b]).sum()) for b in range(B)),
                    "roi": sum(int((torch.cat([out["kern_roi"][b, :n], out["kern_roi"][b, GMAX:]]) != out["torch_roi"][b]).sum())
                               for b, n in enumerate(counts))}
        times = {k: [] for k in graphs}
        for _ in range(a.reps):
            for k, gr in graphs.items():
                for _ in range(5):
                    gr.replay()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.iters):
                    gr.replay()
                e.record()
                side.synchronize()
                times[k].append(round(s.elapsed_time(e) * 1e3 / a.iters, 2))
    res = dict(device=torch.cuda.get_device_name(0), batch=B, image=f"{H}x{W}", boxes_per_image=counts, Gmax=GMAX,
               candidates={k: v["N"] for k, v in stages.items()}, iters_per_round=a.iters, rounds=a.reps,
               unit="microseconds per graph replay of one stage's assignment for the whole batch",
               gt_inds_differing_from_the_torch_arm=mismatch)
    for k, t in times.items():
        res[k] = dict(rounds=t, median=float(np.median(t)), spread=round(max(t) - min(t), 2))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
