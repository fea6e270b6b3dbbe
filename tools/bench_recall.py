#!/usr/bin/env python3
"""Time RecallAccumulator.update (pswin_recall_match) against the torch definitions of evaluation.py on the same GPU and against
eval_recalls_lists on the host, read-back included.

    python tools/bench_recall.py [--iters 50] [--reps 5] [--out profiles/recall_bench.json]

Shapes: B = 8 images, R = 1000 proposals (all counted), Gmax = 32 and 100 boxes (Gmax - 4 counted), the default proposal numbers
(100, 300, 1000) and thresholds (0.5 .. 0.95).  A third of the proposals are jittered boxes, the rest are unrelated.
    kernel        one update captured once and replayed: --reps rounds of --iters replays
    definitions   proposal_round_ious + recall_hits on the device tensors, an eager call between two synchronisations (they read the counts
                  back and cannot be captured)
    host          Proposals.as_lists (the read-back) + eval_recalls_lists on the CPU, an eager call
The arms take turns inside every round.  Figures are microseconds; rounds, their median and spread (max - min)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_targets import _capture  # noqa: E402
from panoswintransformerobjectdetection_amd import evaluation as ev  # noqa: E402
from panoswintransformerobjectdetection_amd.detector import PaddedTargets, Proposals  # noqa: E402

B, R, H, W = 8, 1000, 512, 1024
DEV = "cuda:0"


def batch(G, seed=0):
    rng = np.random.RandomState(seed)
    xy = np.round(rng.uniform(0, [W - 200, H - 200], (B, G, 2)) * 4) / 4
    wh = np.round(rng.uniform(16, 200, (B, G, 2)) * 4) / 4
    gb = np.concatenate([xy, xy + wh], 2).astype(np.float32)
    src = rng.randint(0, G - 4, (B, R))
    near = np.take_along_axis(gb, src[:, :, None], 1) + np.round(rng.uniform(-12, 12, (B, R, 4)) * 4).astype(np.float32) / 4
    pxy = np.round(rng.uniform(0, [W - 100, H - 100], (B, R, 2)) * 4) / 4
    far = np.concatenate([pxy, pxy + np.round(rng.uniform(8, 100, (B, R, 2)) * 4) / 4], 2).astype(np.float32)
    pb = np.where(rng.rand(B, R, 1) < 0.33, near, far).astype(np.float32)
    pb[..., 2:] = np.maximum(pb[..., 2:], pb[..., :2] + 1)
    sc = np.sort(rng.uniform(0.01, 1, (B, R)).astype(np.float32), 1)[:, ::-1].copy()
    t = torch.as_tensor
    return (Proposals(t(pb).to(DEV), t(sc).to(DEV), torch.full((B,), R, dtype=torch.int32, device=DEV)),
            PaddedTargets(t(gb).to(DEV), torch.zeros(B, G, dtype=torch.long, device=DEV), torch.full((B,), G - 4, dtype=torch.int32, device=DEV)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recall_bench.json"))
    a = ap.parse_args()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    acc0 = ev.RecallAccumulator(device=DEV)
    res = dict(device=torch.cuda.get_device_name(0),
               shape=dict(B=B, R=R, Gmax=[32, 100], proposal_nums=list(acc0.proposal_nums), T=len(acc0.iou_thrs)),
               iters_per_round=a.iters, rounds=a.reps,
               unit="microseconds; kernel: per graph replay of one update; definitions and host: per eager call between two synchronisations; "
                    "spread = max - min over the rounds; the arms take turns inside every round")
    for G in (32, 100):
        props, gts = batch(G)
        acc = ev.RecallAccumulator(device=DEV)
        graph = _capture(lambda: acc.update(props, gts), side)

        def definitions():
            return ev.recall_hits(ev.proposal_round_ious(props, gts, acc.proposal_nums), acc.iou_thrs)

        def host():
            lists = props.as_lists()
            return ev.eval_recalls_lists([t["boxes"].cpu().numpy() for t in gts.as_lists()], lists, acc.proposal_nums, acc.iou_thrs)

        with torch.cuda.stream(side):
            acc.reset()
            rounds = acc.update(props, gts)
            side.synchronize()
        want_hits, want_num = definitions()
        same = bool(torch.equal(rounds.view(torch.int32), ev.proposal_round_ious(props, gts, acc.proposal_nums).view(torch.int32))) and \
            bool(torch.equal(acc.hits, want_hits)) and int(acc.num_gts) == want_num
        recalls = acc.summarize()
        times = dict(kernel=[], definitions=[], host=[])
        for _ in range(a.reps):
            with torch.cuda.stream(side):
                for _ in range(3):
                    graph.replay()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.iters):
                    graph.replay()
                e.record()
                side.synchronize()
            times["kernel"].append(round(s.elapsed_time(e) * 1e3 / a.iters, 1))
            for name, fn in (("definitions", definitions), ("host", host)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(round((time.perf_counter() - t0) * 1e6, 1))
        res[f"Gmax_{G}"] = dict({k: dict(rounds=v, median=float(np.median(v)), spread=round(max(v) - min(v), 1)) for k, v in times.items()},
                                kernel_equals_the_definitions=same, ar=[round(float(v), 6) for v in recalls["ar"]], num_gts=recalls["num_gts"])
        print(json.dumps({f"Gmax_{G}": res[f"Gmax_{G}"]}), flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
