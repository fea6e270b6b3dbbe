"""Cost of the device training recipe of optim.FlatAdamW at the PanoSwin-T flat size, every variant captured into a hipGraph and
replayed (the way bench.py's step runs it):

  plain           FlatAdamW(paramwise_cfg)                                   1 launch   (pswin_adamw_flat_groups)
  schedule        + lr_config                                                2 launches (record, update)
  schedule_clip   + grad_clip                                                3 launches (sum of squares, record, update)
  schedule_guard  + grad_clip + skip_nonfinite                               3 launches

and the two new launches on their own (a graph holding only that launch).  Times are device events around `--replays` replays,
median of `--rounds`.  Writes profiles/optim_schedule_timing.json.

    python tools/bench_optim.py [--replays 200] [--rounds 5] [--out profiles/optim_schedule_timing.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from panoswintransformerobjectdetection_amd import SimplePanoSwinTransformer  # noqa: E402
from panoswintransformerobjectdetection_amd.dp import GradReducer  # noqa: E402
from panoswintransformerobjectdetection_amd.ops import call, ptr  # noqa: E402
from panoswintransformerobjectdetection_amd.optim import REFERENCE_PARAMWISE_CFG, FlatAdamW  # noqa: E402

TCFG = dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7, ape=True, drop_path_rate=0.0, pano_mode=True)
LR_CONFIG = dict(policy="step", warmup="linear", warmup_iters=500, warmup_ratio=0.001, step=[8, 11])
VARIANTS = {
    "plain": dict(),
    "schedule": dict(lr_config=LR_CONFIG, iters_per_epoch=1000),
    "schedule_clip": dict(lr_config=LR_CONFIG, iters_per_epoch=1000, grad_clip=dict(max_norm=35, norm_type=2)),
    "schedule_guard": dict(lr_config=LR_CONFIG, iters_per_epoch=1000, grad_clip=dict(max_norm=35, norm_type=2), skip_nonfinite=True),
}


def time_graph(fn, replays, rounds, stream):
    with torch.cuda.stream(stream):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        fn()
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(replays):
            g.replay()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / replays)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_schedule_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs an MI355X")
    torch.manual_seed(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = dict(workload="FlatAdamW.step captured in a hipGraph, PanoSwin-T flat buffer, reference paramwise_cfg, bf16 shadow",
               device=torch.cuda.get_device_name(0), replays=a.replays, rounds=a.rounds, variants={})
    with torch.cuda.stream(side):
        m = SimplePanoSwinTransformer(**TCFG, compute_dtype=torch.bfloat16)
        m.init_weights(None)
        m = m.cuda().train()
        red = GradReducer(m, pack=True)
        flat = red.flatten_parameters(m, torch.bfloat16)
        n = flat.numel()
        res["flat_elements"] = n
        red.flat.copy_(torch.randn(n, device="cuda") * 1e-3)
        master = flat.data.clone()
        for name, kw in VARIANTS.items():
            flat.data.copy_(master)
            opt = FlatAdamW(flat, lr=1e-4, betas=(0.9, 0.999), weight_decay=0.05, model=m, paramwise_cfg=REFERENCE_PARAMWISE_CFG, **kw)
            us, all_us = time_graph(opt.step, a.replays, a.rounds, side)
            res["variants"][name] = dict(us_per_step=round(us, 2), rounds_us=[round(x, 2) for x in all_us])
            if name == "schedule_guard":
                us, all_us = time_graph(lambda: call("pswin_grad_sumsq", flat, ptr(red.flat), n, ptr(opt._partials)), a.replays, a.rounds, side)
                res["grad_sumsq"] = dict(us=round(us, 2), rounds_us=[round(x, 2) for x in all_us], bytes=4 * n,
                                         tb_per_s=round(4 * n / (us * 1e-6) / 1e12, 3))
                st = opt.state[flat]
                grouped = opt.group_of is not None
                k = len(opt.group_mults) if grouped else 0
                mult = ctypes.addressof(opt._lr_mult_c) if grouped else None
                us, all_us = time_graph(lambda: call("pswin_adamw_record", flat, ptr(opt._partials), ctypes.addressof(opt._sched_c), 1e-4, k,
                                                     mult, 35.0, 1, ptr(st["step"]), ptr(st["iteration"]),
                                                     ptr(st["skipped"]), ptr(opt._record)), a.replays, a.rounds, side)
                res["adamw_record"] = dict(us=round(us, 2), rounds_us=[round(x, 2) for x in all_us])
            del opt
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    base = res["variants"]["plain"]["us_per_step"]
    for v in res["variants"].values():
        v["extra_us_vs_plain"] = round(v["us_per_step"] - base, 2)
        v["extra_pct_of_9p46ms_step"] = round(100 * (v["us_per_step"] - base) / 9460.0, 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
