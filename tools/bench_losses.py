#!/usr/bin/env python3
"""Time the detector's loss kernels as hipGraph replays against the torch expressions they replace, and a captured heads_loss + backward
of MiniMaskRCNN and MiniCascadeRCNN with the loss hooks on the kernels and on those expressions.

    python tools/bench_losses.py [--iters 50] [--reps 5] [--batches 2 8] [--models maskrcnn cascade] [--out profiles/losses_bench.json]
                                 [--bench-before FILE] [--bench-after FILE]

Shapes (the config's): B = 2 and 8 images of 512 x 1024, C = 80, bf16 logits and deltas as the heads return them under autocast, the mask
logits channels-last.  Per operation, forward + backward, the hook's whole loss (rows and the sum that remains):
    cls_loss    N = B * 512 rows of 81 logits             torch: F.cross_entropy(cls.float(), labels)    | kernels: ops.ce_rows
    box_loss    N = B * 512 rows of 320 deltas, 128 pos.  torch: two advanced indexings of reg.float()   | kernels: ops.l1_rows over all rows
    mask_loss   M = B * 128 maps of 80 x 28 x 28          torch: logits.float()[ar, labels], BCE, mean   | kernels: ops.mask_bce_rows
    rpn_loss    A = 130,944 anchors, 128 + 256 slots      torch: gather, BCE, abs, masked sums per image | kernels: ops.rpn_losses
"torch" is losses.*_loss_torch: the statements the models evaluated before the kernels (and still evaluate on the CPU).
Heads: one captured step (heads_loss + backward on PanoSwin-T feature maps, random) per model and arm, the peak of
torch.cuda.max_memory_allocated over an eager step of each arm, and the node count of each graph.
Every arm is captured once; the arms are replayed in turn, --reps rounds of --iters replays, in one process; figures are microseconds per
replay for the whole batch: rounds, their median and their spread (max - min).  --bench-before / --bench-after: files holding the JSON
line of `python bench.py --config maskrcnn` on the parent commit and on this one; they are copied into the result."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_targets import TCFG, _capture, _node_count, _time  # noqa: E402
from panoswintransformerobjectdetection_amd import cascade, losses  # noqa: E402
from panoswintransformerobjectdetection_amd import detector as det  # noqa: E402

H, W, C, N_TOT, N_POS, S_MASK = 512, 1024, 80, 512, 128, 28
A, RPN_POS, RPN_TOT = 130944, 128, 256
TORCH_HOOKS = dict(rpn_loss=losses.rpn_loss_torch, cls_loss=losses.cls_loss_torch, box_loss=losses.box_loss_torch, mask_loss=losses.mask_loss_torch)
DEV = "cuda:0"


def bench_ops(B, side, a):
    g = torch.Generator("cpu").manual_seed(B)
    leaf = lambda t: t.to(DEV).requires_grad_(True)                                             # noqa: E731
    cls = leaf(torch.randn(B * N_TOT, C + 1, generator=g).bfloat16())
    reg = leaf(torch.randn(B * N_TOT, 4 * C, generator=g).bfloat16())
    logits = leaf(torch.randn(B * N_POS, C, S_MASK, S_MASK, generator=g).bfloat16().contiguous(memory_format=torch.channels_last))
    pos_valid = (torch.rand(B, N_POS, generator=g) < 0.6).to(DEV)
    labels_b = torch.full((B, N_TOT), C)
    labels_b[:, :N_POS] = torch.randint(0, C, (B, N_POS), generator=g)
    labels_b[:, :N_POS][~pos_valid.cpu()] = C
    labels_b = labels_b.to(DEV)
    reg_t = torch.randn(B, N_POS, 4, generator=g).to(DEV) * pos_valid[:, :, None]
    pl = labels_b[:, :N_POS].reshape(-1).clamp(max=C - 1)
    mt = (torch.rand(B * N_POS, S_MASK, S_MASK, generator=g) > 0.5).float().to(DEV)
    pv = pos_valid.reshape(-1).float()
    cls_all, reg_all = leaf(torch.randn(B, A, generator=g)), leaf(torch.randn(B, A, 4, generator=g) * 0.1)
    idx = torch.stack([torch.randperm(A, generator=g)[:RPN_POS + RPN_TOT] for _ in range(B)]).to(DEV)
    rpn_pos = (torch.rand(B, RPN_POS, generator=g) < 0.3).to(DEV)
    valid = torch.cat([rpn_pos.float(), (torch.rand(B, RPN_TOT, generator=g) < 0.8).float().to(DEV)], 1)
    rpn_t = torch.randn(B, RPN_POS, 4, generator=g).to(DEV) * rpn_pos[:, :, None]
    calls = dict(cls_loss=((cls,), (cls, labels_b.reshape(-1))), box_loss=((reg,), (reg, labels_b, reg_t, pos_valid)),
                 mask_loss=((logits,), (logits, pl, mt, pv)), rpn_loss=((cls_all, reg_all), (cls_all, reg_all, idx, valid, rpn_pos, rpn_t)))
    out, steps = {}, {}
    for name, (leaves, args) in calls.items():
        for arm, hooks in (("torch", TORCH_HOOKS), ("kernels", losses.KERNEL_HOOKS)):
            def step(fn=hooks[name], leaves=leaves, args=args, key=f"{name}_{arm}"):
                for x in leaves:
                    x.grad = None
                res = fn(*args)
                (res if torch.is_tensor(res) else res[0] + res[1]).backward()
                out[key] = [x.grad for x in leaves]
            steps[f"{name}_fwd_bwd_{arm}"] = step
    graphs = {k: _capture(f, side) for k, f in steps.items()}
    with torch.cuda.stream(side):
        for gr in graphs.values():
            gr.replay()
        side.synchronize()
        # how far the two arms' gradients are apart, relative to the largest element (the torch arm rounds through a float copy)
        differ = {n: max(float((k.float() - t.float()).abs().max() / t.float().abs().max().clamp(min=1e-30))
                         for k, t in zip(out[f"{n}_kernels"], out[f"{n}_torch"])) for n in calls}
    res = _time(graphs, side, a.iters, a.reps)
    res["largest_gradient_difference_between_the_arms_relative"] = differ
    return res


def _targets(B, Gmax):
    tg = det.synthetic_targets(B, H, W, DEV)
    T = det.PaddedTargets.allocate(B, Gmax, DEV, mask_hw=(H, W))
    return T.copy_from([t["boxes"] for t in tg], [t["labels"] for t in tg], [t["masks"] for t in tg])


def bench_heads(model, B, side, a, Gmax=16):
    with torch.cuda.stream(side):
        torch.manual_seed(0)
        cls = det.MiniMaskRCNN if model == "maskrcnn" else cascade.MiniCascadeRCNN
        m = cls(dict(TCFG, compute_dtype=torch.float32), num_classes=C).to(DEV).train()
        heads = m.head_parameters()
        feats = [torch.randn(B, ch, H // s, W // s, device=DEV) for ch, s in zip(m.backbone.num_features, (4, 8, 16, 32))]
        T = _targets(B, Gmax)
        graphs, extra = {}, {}
        for arm, hooks in (("torch", TORCH_HOOKS), ("kernels", losses.KERNEL_HOOKS)):
            state = {}

            def step(hooks=hooks, state=state):
                for k, fn in hooks.items():
                    setattr(m, k, fn)
                for p in heads:
                    p.grad = None
                ls = m.heads_loss(feats, T, (H, W))
                sum(ls.values()).backward()
                state["loss"] = torch.stack([ls[k] for k in sorted(ls)])

            step()                                                                               # (library autotuning, caches)
            side.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step()
            side.synchronize()
            peak = torch.cuda.max_memory_allocated()
            key = f"{model}_heads_step_{arm}"
            graphs[key] = _capture(step, side, keep_graph=True)
            extra[key] = dict(graph_nodes=_node_count(graphs[key]), eager_step_peak_bytes=int(peak), eager_step_peak_over_resident_bytes=int(peak - base),
                              state=state)
    res = _time(graphs, side, max(a.iters // 5, 5), a.reps)
    for k, v in extra.items():
        v["losses_of_the_last_replay"] = [round(x, 5) for x in v.pop("state")["loss"].tolist()]
        res[k].update(v)
    del graphs, m, feats, T
    torch.cuda.empty_cache()
    return res


def _bench_line(path):
    if not path:
        return "not measured"
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip().startswith("{")]
    return json.loads(lines[-1]) if lines else "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--models", nargs="*", default=["maskrcnn", "cascade"])
    ap.add_argument("--label", default="this")
    ap.add_argument("--bench-before", default=None)
    ap.add_argument("--bench-after", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "losses_bench.json"))
    a = ap.parse_args()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = dict(label=a.label, device=torch.cuda.get_device_name(0), image=f"{H}x{W}", classes=C, iters_per_round=a.iters, rounds=a.reps,
               unit="microseconds per graph replay for the whole batch; spread = max - min over the rounds",
               torch_arm="losses.*_loss_torch: the statements the models evaluated before the kernels")
    res["bench_py_maskrcnn_before"] = _bench_line(a.bench_before)
    res["bench_py_maskrcnn_after"] = _bench_line(a.bench_after)

    def record(B, part):
        res.setdefault(f"batch_{B}", {}).update(part)
        print(json.dumps({f"batch_{B}": part}), flush=True)
        with open(a.out, "w") as f:                                                              # after every part: a run cut short keeps what it has
            json.dump(res, f, indent=1)

    for B in a.batches:
        record(B, bench_ops(B, side, a))
        torch.cuda.empty_cache()
    for B in a.batches:
        for model in a.models:
            record(B, bench_heads(model, B, side, a))
    return 0


if __name__ == "__main__":
    sys.exit(main())
