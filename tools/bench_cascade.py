#!/usr/bin/env python3
"""Time the Cascade R-CNN pieces as hipGraph replays: the torch definitions run on the GPU against the HIP kernels, and a captured
MiniCascadeRCNN.heads_loss (forward and backward of everything behind the backbone).

    python tools/bench_cascade.py [--iters 50] [--reps 3] [--out profiles/cascade_bench.json] [--label this]

Shapes: B = 8 images of 512 x 1024, C = 80, bf16 logits and deltas (what the box head returns under autocast).
    refine_rois   R = 1000 RoIs per image                            definition (cascade.refine_rois) | kernel (ops.refine_rois)
    giou_rows     N = 8 * 512 rows, a quarter weighted, fwd + bwd    definition (cascade.giou_rows)   | kernels (ops.giou_rows)
    heads_loss    a captured step of the cascade heads on PanoSwin-T feature maps (random), with the node count of the captured graph
Each arm is captured once and replayed in turn, --reps rounds of --iters replays, in one process; figures are microseconds per replay for
the whole batch."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_targets import TCFG, _capture, _node_count, _targets, _time  # noqa: E402
from panoswintransformerobjectdetection_amd import cascade  # noqa: E402

B, H, W, R, N_TOT, C = 8, 512, 1024, 1000, 512, 80
STDS = (0.1, 0.1, 0.2, 0.2)


def _boxes(n, g):
    c = torch.rand(n, 2, generator=g) * torch.tensor([W, H])
    wh = torch.rand(n, 2, generator=g) * torch.tensor([W / 3, H / 3]) + 4
    return torch.cat([c - wh / 2, c + wh / 2], -1)


def bench_ops(side, a):
    from panoswintransformerobjectdetection_amd import ops
    dev = "cuda:0"
    g = torch.Generator("cpu").manual_seed(0)
    rois = _boxes(B * R, g).view(B, R, 4).to(dev)
    cls = torch.randn(B, R, C + 1, generator=g).to(dev, torch.bfloat16)
    deltas = torch.randn(B, R, 4 * C, generator=g).to(dev, torch.bfloat16)
    labels = torch.randint(0, C + 1, (B, R), generator=g).to(dev)
    N = B * N_TOT
    g_rois, g_target = _boxes(N, g).to(dev), _boxes(N, g).to(dev)
    g_deltas = torch.randn(N, 4 * C, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
    g_labels = torch.randint(0, C, (N,), generator=g).to(dev)
    g_weight = (torch.arange(N) % N_TOT < N_TOT // 4).float().to(dev)
    out = {}

    def refine(fn, name):
        def step():
            out[name] = fn(rois, cls, deltas, labels, STDS, (H, W))
        return step

    def giou(fn, name):
        def step():
            g_deltas.grad = None
            fn(g_rois, g_deltas, g_labels, g_weight, g_target, STDS).sum().backward()
            out[name] = g_deltas.grad
        return step

    steps = {"refine_rois_definition": refine(cascade.refine_rois, "rd"), "refine_rois_kernel": refine(ops.refine_rois, "rk"),
             "giou_rows_fwd_bwd_definition": giou(cascade.giou_rows, "gd"), "giou_rows_fwd_bwd_kernels": giou(ops.giou_rows, "gk")}
    graphs = {k: _capture(f, side) for k, f in steps.items()}
    with torch.cuda.stream(side):
        for gr in graphs.values():
            gr.replay()
        side.synchronize()
        differ = dict(refine_used=int((out["rd"][1] != out["rk"][1]).sum()))
    res = _time(graphs, side, a.iters, a.reps)
    res["entries_differing_from_the_definition_on_the_gpu"] = differ
    return res


def bench_heads(side, a, Gmax=16):
    dev = "cuda:0"
    with torch.cuda.stream(side):
        torch.manual_seed(0)
        m = cascade.MiniCascadeRCNN(dict(TCFG, compute_dtype=torch.float32), num_classes=C).to(dev).train()
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
    res = _time({"cascade_heads_loss_padded": g}, side, max(a.iters // 5, 5), a.reps)
    res["cascade_heads_loss_padded"]["graph_nodes"] = _node_count(g)
    res["cascade_heads_loss_padded"]["losses"] = [round(v, 5) for v in state["loss"].tolist()]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cascade_bench.json"))
    a = ap.parse_args()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = dict(label=a.label, device=torch.cuda.get_device_name(0), batch=B, image=f"{H}x{W}", classes=C, iters_per_round=a.iters, rounds=a.reps,
               unit="microseconds per graph replay for the whole batch")
    res.update(bench_ops(side, a))
    torch.cuda.empty_cache()
    res.update(bench_heads(side, a))
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
