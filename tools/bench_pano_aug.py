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

    python tools/bench_pano_aug.py --autoaug [--iters 200] [--reps 5] [--out profiles/pano_autoaug_bench.json]

times the recipe's AutoAugment stage on 8 x 512x1024 with a fixed plan, four images of each policy, as captured graphs replayed in turn
(a, b, c, a, b, c, ...; --reps rounds of --iters replays each) in one process:
    a  pswin_pano_resize_crop_resize_normalize_pad: one launch
    b  the same result from the plain resize kernel: one launch to h1 x w1 for the four cropped images, the uint8 image recovered and
       cropped in torch, one launch per crop (each has its own size), one launch for the four uncropped images
    c  pswin_pano_resize_normalize_pad on all eight images to the same output sizes: context only, it does no crop and one resize
It checks that a and b hold the same bits before it times them.
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


AUTOAUG_PLAN = [(0, 0, 0, 0, 0, 0) + P.rescale_size(512, 1024, (480, 1333)), (0, 0, 0, 0, 0, 0) + P.rescale_size(512, 1024, (608, 1333)),
                (0, 0, 0, 0, 0, 0) + P.rescale_size(512, 1024, (704, 1333)), (0, 0, 0, 0, 0, 0) + P.rescale_size(512, 1024, (800, 1333)),
                (400, 800, 5, 335, 392, 393) + P.rescale_size(392, 393, (480, 1333)),
                (500, 1000, 7, 547, 458, 453) + P.rescale_size(458, 453, (672, 1333)),
                (600, 1200, 16, 73, 573, 502) + P.rescale_size(573, 502, (736, 1333)),
                (600, 1200, 0, 600, 600, 600) + P.rescale_size(600, 600, (800, 1333))]


def _graph(step):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    torch.cuda.synchronize()
    return g


def autoaug(a):
    dev = "cuda:0"
    plans = AUTOAUG_PLAN
    B, H, W = len(plans), 512, 1024
    imgs = torch.from_numpy(np.random.RandomState(H).randint(0, 256, (B, H, W, 3)).astype(np.uint8)).to(dev)
    Hp, Wp = P.padded_size([p[6:] for p in plans], 32)
    norm = P.norm_tensor(P.IMG_NORM_MEAN, P.IMG_NORM_STD, dev)
    ident = P.norm_tensor((0, 0, 0), (1, 1, 1), dev)
    plan_t = torch.tensor(plans, dtype=torch.int32, device=dev)
    hw_all = torch.tensor([p[6:] for p in plans], dtype=torch.int32, device=dev)
    xa, xb, xc = (torch.empty(B, 3, Hp, Wp, device=dev) for _ in range(3))
    plain = [i for i, p in enumerate(plans) if p[0] == 0]
    crop = [i for i, p in enumerate(plans) if p[0]]
    assert plain == list(range(len(plain)))                    # the uncropped images lead the batch: x[:n] is one contiguous buffer
    hw_plain = hw_all[:len(plain)].contiguous()
    hw_first = torch.tensor([plans[i][:2] for i in crop], dtype=torch.int32, device=dev)
    hw_one = [hw_all[i:i + 1].contiguous() for i in crop]
    H1, W1 = max(plans[i][0] for i in crop), max(plans[i][1] for i in crop)
    first = torch.empty(len(crop), 3, H1, W1, device=dev)
    crop_imgs = imgs[crop[0]:].contiguous()

    def step_a():
        P.resize_crop_resize_normalize_pad(imgs, plan_t, pad_hw=(Hp, Wp), out=xa, norm=norm)

    def step_b():
        P.resize_normalize_pad(imgs[:len(plain)], hw_plain, pad_hw=(Hp, Wp), out=xb[:len(plain)], norm=norm)
        P.resize_normalize_pad(crop_imgs, hw_first, to_rgb=False, pad_hw=(H1, W1), out=first, norm=ident)
        for k, i in enumerate(crop):
            h1, w1, cy, cx, ch, cw = plans[i][:6]
            u8 = torch.round(first[k, :, cy:cy + ch, cx:cx + cw]).to(torch.uint8).permute(1, 2, 0).contiguous()
            P.resize_normalize_pad(u8[None], hw_one[k], pad_hw=(Hp, Wp), out=xb[i:i + 1], norm=norm)

    def step_c():
        P.resize_normalize_pad(imgs, hw_all, pad_hw=(Hp, Wp), out=xc, norm=norm)

    graphs = {"a_one_launch": _graph(step_a), "b_chain_of_plain_resizes": _graph(step_b), "c_plain_resize_only": _graph(step_c)}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    same = bool(torch.equal(xa, xb))
    times = {k: [] for k in graphs}
    for _ in range(a.reps):
        for k, g in graphs.items():
            for _ in range(5):
                g.replay()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                g.replay()
            e.record()
            torch.cuda.synchronize()
            times[k].append(round(s.elapsed_time(e) * 1e3 / a.iters, 2))
    res = dict(device=torch.cuda.get_device_name(0), batch=B, src=f"{H}x{W}", padded=f"{Hp}x{Wp}", plan=[list(p) for p in plans],
               iters_per_round=a.iters, rounds=a.reps, unit="microseconds per graph replay", a_equals_b_bit_for_bit=same,
               launches=dict(a_one_launch=1, b_chain_of_plain_resizes=2 + len(crop), c_plain_resize_only=1))
    for k, t in times.items():
        res[k] = dict(rounds=t, median=float(np.median(t)), spread=round(max(t) - min(t), 2))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--autoaug", action="store_true", help="time the AutoAugment stage: one launch against the chain of plain resizes")
    ap.add_argument("--reps", type=int, default=5, help="rounds of the --autoaug mode")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--cpu-images", type=int, default=2, help="images for the CPU restatement timing (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.autoaug:
        return autoaug(a)
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
