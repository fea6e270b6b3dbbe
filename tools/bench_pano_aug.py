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

    python tools/bench_pano_aug.py --masks [--iters 20] [--reps 5] [--out profiles/pano_masks_bench.json]

times pswin_pano_masks (B = 8, Gmax = Gin = 32, 512x1024 bitmaps, the plan above, counts from 0 to 32, every fifth row a merged pair),
with and without the stretch, against the definition restated as torch index ops on the same GPU, both as captured graphs replayed in
turn in one process.  It checks that both hold the same bits, and reports times, spreads and achieved bytes per second (the uint8
[B, Gmax, Hp, Wp] written; the same plus every source plane read once) beside pswin_pano_resize_normalize_pad's from
profiles/pano_aug_bench.json.
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


def _mask_geometry(H, W, stretch, kx, ky, shift, flip, plan, dev):
    """What the torch arm gathers with, worked out on the host OUTSIDE the timed step (the kernel works it out inside its launch): flat
    indices into a source plane for every pixel of oh x ow, and with the stretch the four taps and the float64 products of their weights."""
    sy, sx = P.mask_source_index(H, W, plan)
    xs = ((W - 1 - sx if flip else sx) - int(shift)) % W
    if not stretch:
        return dict(idx=torch.from_numpy((sy[:, None] * W + xs[None, :]).reshape(-1)).to(dev))
    u = ((xs.astype(np.float64) + 0.5) / W - 0.5) * 2 * np.pi
    v = ((sy.astype(np.float64) + 0.5) / H - 0.5) * np.pi
    su = np.sin(u)
    u0 = np.arctan2(su * kx / ky, np.cos(u))
    v0 = np.arctan(np.tan(v)[:, None] * np.sin(u0)[None, :] / su[None, :] * ky)
    ya, yb, wy0, wy1 = P._wrap_taps((v0 / np.pi + 0.5) * H - 0.5, H)
    xa, xb, wx0, wx1 = P._wrap_taps(((u0 / (2 * np.pi) + 0.5) * W - 0.5)[None, :], W)
    g = {}
    for name, (yi, wy) in (("0", (ya, wy0)), ("1", (yb, wy1))):
        for name2, (xi, wx) in (("0", (xa, wx0)), ("1", (xb, wx1))):
            g["i" + name + name2] = torch.from_numpy((yi * W + xi).reshape(-1)).to(dev)
            g["p" + name + name2] = torch.from_numpy((1.0 * wy * wx).reshape(-1)).to(dev)
    return g


def masks(a):
    """--masks: pswin_pano_masks against the definition restated as torch index ops on the same GPU, as captured graphs replayed in turn."""
    dev = "cuda:0"
    plans = AUTOAUG_PLAN
    B, H, W, G = len(plans), 512, 1024, 32
    Hp, Wp = P.padded_size([p[6:] for p in plans], 32)
    rng = np.random.RandomState(7)
    src_h = np.zeros((B, G, H, W), np.uint8)
    for b in range(B):
        for g in range(G):
            y0, x0 = rng.randint(0, H - 40), rng.randint(0, W - 40)
            src_h[b, g, y0:y0 + rng.randint(20, H // 2), x0:x0 + rng.randint(20, W // 2)] = 255 if g % 2 else 1
    src = torch.from_numpy(src_h).to(dev)
    counts = [32, 20, 8, 1, 0, 32, 15, 27]
    rows = []
    for b, n in enumerate(counts):
        m = np.stack([rng.permutation(G)[:n], np.full(n, -1)], 1).astype(np.int32).reshape(-1, 2)
        m[::5, 1] = (m[::5, 0] + 1) % G                                    # every fifth row a merged seam pair
        rows.append(m)
    packed, cnt = P.pack_rows(rows, G)
    rows_t, count_t = torch.from_numpy(packed).to(dev), torch.from_numpy(cnt).to(dev)
    plan_t = torch.tensor(plans, dtype=torch.int32, device=dev)
    res = dict(device=torch.cuda.get_device_name(0), batch=B, gmax=G, src=f"{H}x{W}", padded=f"{Hp}x{Wp}", plan=[list(p) for p in plans],
               counts=counts, iters_per_round=a.iters, rounds=a.reps, unit="microseconds per graph replay", hbm_peak_TBps=HBM_PEAK / 1e12,
               torch_arm="binarise, gather, blend, threshold, merge and pad as torch ops, image by image; its index and weight tensors are "
                         "built on the host outside the timed step",
               bytes=dict(dst_written=B * G * Hp * Wp, src_planes=B * G * H * W))
    ok = True
    for label, stretch in (("no_stretch", False), ("stretch", True)):
        params = P.draw_pano_params(B, W, stretch_chance=1.0 if stretch else 0.0, rng=np.random.RandomState(11))
        prm = P.params_tensor(params, dev)
        geo = [_mask_geometry(H, W, params["stretch"][b], params["kx"][b], params["ky"][b], params["shift"][b], params["flip"][b], plans[b],
                              dev) for b in range(B)]
        sel = [(torch.from_numpy(r[:, 0].astype(np.int64)).to(dev), torch.from_numpy(np.maximum(r[:, 1], 0).astype(np.int64)).to(dev),
                torch.from_numpy((r[:, 1] >= 0).astype(np.uint8)).to(dev)[:, None]) for r in rows]
        out_k = torch.empty(B, G, Hp, Wp, dtype=torch.uint8, device=dev)
        out_t = torch.empty(B, G, Hp, Wp, dtype=torch.uint8, device=dev)

        def step_kernel():
            P.warp_resize_masks(src, prm, plan_t, rows_t, count_t, pad_hw=(Hp, Wp), out=out_k)

        def step_torch():
            out_t.zero_()
            for b in range(B):
                n, (oh, ow) = counts[b], plans[b][6:]
                if n == 0:
                    continue
                g = geo[b]
                if "idx" in g:
                    flat = src[b].reshape(G, H * W)
                    w = (flat[:, g["idx"]] != 0).to(torch.uint8)
                else:
                    flat = (src[b].reshape(G, H * W) != 0).to(torch.float64)
                    t = 0.0 + flat[:, g["i00"]] * g["p00"]
                    t = t + flat[:, g["i01"]] * g["p01"]
                    t = t + flat[:, g["i10"]] * g["p10"]
                    t = t + flat[:, g["i11"]] * g["p11"]
                    w = torch.floor(t + 0.5).to(torch.uint8)
                a0, a1, has = sel[b]
                out_t[b, :n, :oh, :ow] = torch.maximum(w[a0], w[a1] * has).reshape(n, oh, ow)

        graphs = {"kernel_one_launch": _graph(step_kernel), "torch_index_ops": _graph(step_torch)}
        for g in graphs.values():
            g.replay()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_k, out_t))
        ok = ok and same
        times = {k: [] for k in graphs}
        for _ in range(a.reps):
            for k, g in graphs.items():
                for _ in range(3):
                    g.replay()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.iters):
                    g.replay()
                e.record()
                torch.cuda.synchronize()
                times[k].append(round(s.elapsed_time(e) * 1e3 / a.iters, 2))
        arm = dict(kernel_equals_torch_bit_for_bit=same, set_fraction=round(float(out_k.float().mean()), 4))
        for k, t in times.items():
            med = float(np.median(t))
            arm[k] = dict(rounds=t, median=med, spread=round(max(t) - min(t), 2))
        med = arm["kernel_one_launch"]["median"]
        arm["kernel_GBps_dst_written"] = round(B * G * Hp * Wp / med / 1e3, 1)
        arm["kernel_GBps_dst_and_src"] = round((B * G * Hp * Wp + B * G * H * W) / med / 1e3, 1)
        arm["kernel_pct_of_8TBps_dst_and_src"] = round(100 * (B * G * Hp * Wp + B * G * H * W) / (med * 1e-6) / HBM_PEAK, 1)
        arm["torch_over_kernel"] = round(arm["torch_index_ops"]["median"] / med, 2)
        res[label] = arm
        del graphs
    ref = os.path.join(ROOT, "profiles", "pano_aug_bench.json")
    if os.path.isfile(ref):
        with open(ref) as f:
            res["resize_normalize_pad_GBps_for_comparison"] = {f"{r['src']}@{r['scale']}": r["resize_GBps"] for r in json.load(f)["rows"]}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masks", action="store_true", help="time pswin_pano_masks against the definition as torch index ops")
    ap.add_argument("--autoaug", action="store_true", help="time the AutoAugment stage: one launch against the chain of plain resizes")
    ap.add_argument("--reps", type=int, default=5, help="rounds of the --autoaug mode")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--cpu-images", type=int, default=2, help="images for the CPU restatement timing (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.masks:
        return masks(a)
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
