#!/usr/bin/env python3
"""Time the pano augmentation kernels (csrc/pswin_pano.hip) with device events at batch 8.

    python tools/bench_pano_aug.py [--iters 50] [--out profiles/pano_aug_bench.json] [--cpu-images 2]

For 512x1024 and 1024x2048 uint8 BGR sources and the Resize scales (480, 1333), (640, 1333), (800, 1333) it reports the median time
of pswin_pano_warp_u8 (every image stretched, rolled, half of them flipped) and of pswin_pano_resize_normalize_pad, and their
bandwidth by algorithmic bytes against the MI355X's 8 TB/s HBM peak:
    warp:   read + write of the uint8 images                          2 * B * H * W * 3
    resize: read of the uint8 images + write of the f32 [B,3,Hp,Wp]   B * H * W * 3 + B * 3 * Hp * Wp * 4
Beside it, labelled as such, the per-image time of the numpy float64 restatement of the warp (tests/_pano_ref.py) on one CPU core:
the cost of the stretch in a CPU data loader.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from panoswintransformerobjectdetection_amd import pano_aug as P  # noqa: E402

HBM_PEAK = 8.0e12


def _time(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return float(np.median([s.elapsed_time(e) for s, e in ev])) * 1e3       # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--cpu-images", type=int, default=2, help="images for the CPU restatement timing (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    B = a.batch
    rows = []
    for H, W in [(512, 1024), (1024, 2048)]:
        rng = np.random.RandomState(H)
        imgs = torch.from_numpy(rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).to(dev)
        params = P.draw_pano_params(B, W, rng=rng)
        params["stretch"][:] = True
        params["kx"][:] = rng.uniform(0.5, 2.0, B)
        params["ky"][:] = rng.uniform(0.5, 2.0, B)
        prm = P.params_tensor(params, dev)
        warped = torch.empty_like(imgs)
        t_warp = _time(lambda: P.pano_warp(imgs, prm, out=warped), a.iters)
        b_warp = 2 * imgs.numel()
        for s in (480, 640, 800):
            sizes = [P.rescale_size(H, W, (s, 1333))] * B
            Hp, Wp = P.padded_size(sizes, 32)
            hw = torch.tensor(sizes, dtype=torch.int32, device=dev)
            norm = P.norm_tensor(P.IMG_NORM_MEAN, P.IMG_NORM_STD, dev)
            x = torch.empty(B, 3, Hp, Wp, device=dev)
            t_rs = _time(lambda: P.resize_normalize_pad(warped, hw, pad_hw=(Hp, Wp), out=x, norm=norm), a.iters)
            b_rs = imgs.numel() + x.numel() * 4
            row = dict(src=f"{H}x{W}", batch=B, scale=s, out=f"{sizes[0][0]}x{sizes[0][1]}", padded=f"{Hp}x{Wp}",
                       warp_us=round(t_warp, 2), warp_GBps=round(b_warp / t_warp / 1e3, 1), warp_pct_of_8TBps=round(100 * b_warp / (t_warp * 1e-6) / HBM_PEAK, 1),
                       resize_us=round(t_rs, 2), resize_GBps=round(b_rs / t_rs / 1e3, 1), resize_pct_of_8TBps=round(100 * b_rs / (t_rs * 1e-6) / HBM_PEAK, 1),
                       both_us=round(t_warp + t_rs, 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
    cpu = {}
    if a.cpu_images > 0:
        import _pano_ref as R
        for H, W in [(512, 1024), (1024, 2048)]:
            img = np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)
            t0 = time.perf_counter()
            for i in range(a.cpu_images):
                R.warp(img, True, 1.5, 0.7, 100, i % 2 == 1)
            cpu[f"{H}x{W}"] = round((time.perf_counter() - t0) / a.cpu_images * 1e3, 1)
        print(json.dumps({"CPU_numpy_restatement_ms_per_image_one_core": cpu}), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), iters=a.iters, hbm_peak_TBps=HBM_PEAK / 1e12, rows=rows,
               cpu_numpy_restatement_ms_per_image=cpu)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
