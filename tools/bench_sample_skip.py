"""Sample skipping kernel by kernel: fc1 + GELU forward (pswin_gemm_nt_gelu_fwd), fc2's data gradient + GELU backward
(pswin_gemm_nt_gelu_bwd) and the two weight gradients of the Mlp on the ring kernel, at the Mlp shapes of PanoSwin-T stages 1-3
(batch 8), each with (a) no liveness argument, three times over (the run-to-run range), (b) an all-live factor vector, (c) one and two
dead samples of 8.  (b) must lie within (a)'s range; (c) shows what a dead sample saves -- for the tiled GEMM only because the live
tiles are compacted before they are dealt to the XCDs.  Each figure: microseconds per launch, 30 launches replayed from a hipGraph.
usage: python tools/bench_sample_skip.py [--json out.json]"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch

from panoswintransformerobjectdetection_amd import grad_queue, ops
from panoswintransformerobjectdetection_amd._lib import call, ptr

dev = "cuda:0"
BF = torch.bfloat16
B = 8
STAGES = [("stage 1", 64 * 128, 192), ("stage 2", 32 * 64, 384), ("stage 3", 16 * 32, 768)]


def t(fn, n=30):
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def scale(n_dead):
    s = torch.full((B,), 1.25, dtype=torch.float32, device=dev)
    if n_dead:
        s[torch.tensor([2, 5][:n_dead], device=dev)] = 0.0
    return s


def kernels(S, C):
    """name -> fn(live) for the Mlp of one stage"""
    M, Nh = B * S, 4 * C
    x = torch.randn(M, C, device=dev).to(BF)
    w1 = (torch.randn(Nh, C, device=dev) * 0.05).to(BF)
    w2t = (torch.randn(Nh, C, device=dev) * 0.05).to(BF)
    b1 = torch.zeros(Nh, device=dev)
    pre, h, g = (torch.zeros(M, Nh, dtype=BF, device=dev) for _ in range(3))
    dout = torch.randn(M, C, device=dev).to(BF)
    tf = ops.gemm_nt_tile(M, C, Nh, "pswin_gemm_nt_gelu_fwd", required=True)
    tb = ops.gemm_nt_tile(M, C, Nh, "pswin_gemm_nt_gelu_bwd", required=True)
    ws = torch.zeros(M // tb, Nh, device=dev)
    call("pswin_gemm_nt_gelu_fwd", x, ptr(x), ptr(w1), ptr(b1), ptr(pre), ptr(h), M, C, Nh, tf)
    sp = ops.grouped_wgrad_splits(M)
    p1 = torch.zeros(sp, Nh, C, dtype=BF if sp > 1 else torch.float32, device=dev)
    p2 = torch.zeros(sp, C, Nh, dtype=BF if sp > 1 else torch.float32, device=dev)

    def fwd(live):
        if live is None:
            call("pswin_gemm_nt_gelu_fwd", x, ptr(x), ptr(w1), ptr(b1), ptr(pre), ptr(h), M, C, Nh, tf)
        else:
            call("pswin_gemm_nt_gelu_fwd_live", x, ptr(x), ptr(w1), ptr(b1), ptr(pre), ptr(h), M, C, Nh, tf, ptr(live[0]), live[1])

    def bwd(live):
        if live is None:
            call("pswin_gemm_nt_gelu_bwd", x, ptr(dout), ptr(w2t), ptr(pre), ptr(b1), ptr(g), ptr(ws), M, C, Nh, tb)
        else:
            call("pswin_gemm_nt_gelu_bwd_live", x, ptr(dout), ptr(w2t), ptr(pre), ptr(b1), ptr(g), ptr(ws), M, C, Nh, tb, ptr(live[0]), live[1])

    def wgrads(live):                                     # dW1 and dW2 in one grouped launch, as at the end of a backward pass
        grad_queue._launch_wgrads([grad_queue.weight_grad(g, x, p1, None, sp, 0, 0, live), grad_queue.weight_grad(dout, h, p2, None, sp, 0, 0, live)])

    return {f"gelu_fwd tile {tf}": (fwd, S % tf == 0), f"gelu_bwd tile {tb}": (bwd, S % tb == 0), f"ring dW1+dW2 x{sp} splits": (wgrads, True)}


def main():
    rows = []
    print(f"{'':36s} |  null x3 (range)        | all live | 1 dead | 2 dead   (us per launch)")
    for name, S, C in STAGES:
        for kname, (fn, ok) in kernels(S, C).items():
            if not ok:
                continue
            null = [t(lambda: fn(None)) for _ in range(3)]
            vecs = [scale(nd) for nd in (0, 1, 2)]
            live = [t(lambda v=v: fn((v, S))) for v in vecs]
            rows.append(dict(stage=name, kernel=kname, null_us=null, all_live_us=live[0], one_dead_us=live[1], two_dead_us=live[2],
                             all_live_within_null_range=min(null) <= live[0] <= max(null)))
            print(f"{name + ' ' + kname:36s} | {null[0]:7.1f} {null[1]:7.1f} {null[2]:7.1f} | {live[0]:8.1f} | {live[1]:6.1f} | {live[2]:6.1f}", flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
