#!/usr/bin/env python3
"""Time the RPN's proposal stage: the hook's kernel arm (ops.rpn_proposals -> pswin_rpn_proposals) against its definition arm
(detector.proposals_batch: MiniMaskRCNN._proposals image by image, as torch operators) on the same GPU and the same inputs.

    python tools/bench_proposals.py [--reps 20] [--out profiles/rpn_proposals_bench.json]

Timing only; not part of bench.py.  Shapes: B = 2 and B = 8 images of 512 x 1024 (levels 98,304 / 24,576 / 6,144 / 1,536 / 384), with the
training cfg (nms_pre 2000, 1000 per image) and with the test cfg (nms_pre 1000).  Logits are random normal rounded through bf16, deltas
random with std 0.1.  Both arms are captured once and timed as graph replays (HIP events around `inner` replays), in alternation
(kernels, definition, kernels, ...).  Figures are microseconds per replay, the median over the rounds; `graph_nodes` is the number of
nodes of each arm's captured graph (hipGraphGetNodes)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from panoswintransformerobjectdetection_amd import detector as det, ops  # noqa: E402

H, W = 512, 1024
STRIDES = (4, 8, 16, 32, 64)
DEV = "cuda:0"
CFGS = dict(train=dict(nms_pre=2000, max_per_img=1000, nms=0.7), test=dict(nms_pre=1000, max_per_img=1000, nms=0.7))


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        out = fn()
    g.instantiate()
    return g, out


def _replays(g, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(inner):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / inner


def _node_count(g):
    """hipGraphGetNodes on the captured graph (captured with keep_graph=True)"""
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_size_t(0)
    rc = hip.hipGraphGetNodes(ctypes.c_void_p(g.raw_cuda_graph()), None, ctypes.byref(n))
    return int(n.value) if rc == 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    anchors = det.make_anchors([(H // s, W // s) for s in STRIDES], STRIDES, DEV)
    sizes = [int(x.shape[0]) for x in anchors]
    A = sum(sizes)
    res = dict(device=torch.cuda.get_device_name(0), image=f"{H}x{W}", level_sizes=sizes, rounds=a.reps, replays_per_round=a.inner,
               unit="microseconds per graph replay of the proposal stage of the whole batch, median over the rounds; arms in alternation",
               rows={})
    for B in (2, 8):
        g = torch.Generator().manual_seed(B)
        cls = torch.randn(B, A, generator=g).bfloat16().float().to(DEV)
        reg = (torch.randn(B, A, 4, generator=g) * 0.1).to(DEV)
        for name, cfg in CFGS.items():
            assert ops.rpn_proposals_supported(sizes, B, cfg["nms_pre"], cfg["max_per_img"])
            gk, ok = _capture(lambda: det.proposals_batch_dispatch(cls, reg, anchors, cfg, (H, W)))
            gd, od = _capture(lambda: det.proposals_batch(cls, reg, anchors, cfg, (H, W)))
            gk.replay()
            gd.replay()
            torch.cuda.synchronize()
            times = dict(kernels=[], definition=[])
            for _ in range(a.reps):
                times["kernels"].append(round(_replays(gk, a.inner), 1))
                times["definition"].append(round(_replays(gd, a.inner), 1))
            row = {k: dict(rounds=t, median=float(np.median(t))) for k, t in times.items()}
            row["graph_nodes"] = dict(kernels=_node_count(gk), definition=_node_count(gd))
            row["launches_of_the_entry_point"] = ops.rpn_proposals_launches(sizes, cfg["nms_pre"], cfg["max_per_img"])
            row["survivors"] = ok[2].tolist()
            row["same_scores_and_count"] = bool(torch.equal(ok[1], od[1]) and torch.equal(ok[2], od[2]))
            row["max_box_difference_px"] = float((ok[0] - od[0]).abs().max())
            res["rows"][f"B{B}_{name}"] = row
            del gk, gd
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
