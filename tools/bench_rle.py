#!/usr/bin/env python3
"""Time the run-length encoding of a batch's instance masks (csrc/pswin_rle.hip) against the mask paste alone and against the host path.

    python tools/bench_rle.py [--iters 50] [--reps 5] [--out profiles/rle_bench.json]

Shape: B = 8 images, K = 100 detections, C = 80 classes, 512 x 1024 masks (419 MB of bitmaps).  Logits: "blob" (a disc per detection, the
trained-model case) and "noise" (uniform noise, the random-initialisation worst case); the runs per column are reported.
    paste                  ops.paste_masks alone: the bitmaps
    paste_encode           ops.paste_masks + ops.rle_encode of the bitmaps
    paste_rle              ops.paste_masks_rle: the runs straight from the 28 x 28 logits, no bitmap
    host                   what there was before: Detections.masks.cpu() and rle.py's numpy definition mask by mask, an eager call between
                           two synchronisations -- NOT like for like with the replays: it pays a synchronisation and a 419 MB copy
    to_lists               RleMasks.to_lists(): the read-back of offsets and runs and the strings, eager
The three device arms are captured once each and replayed in turn, --reps rounds of --iters replays, in one process.  Figures are
microseconds; rounds, their median and spread (max - min).  "faster" may be said only where a difference exceeds both arms' spread."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_eval import _eager  # noqa: E402
from bench_targets import _capture, _time  # noqa: E402
from panoswintransformerobjectdetection_amd import ops, rle  # noqa: E402

B, K, C, H, W = 8, 100, 80, 512, 1024
DEV = "cuda:0"


def inputs(kind, seed=0):
    g = torch.Generator().manual_seed(seed)
    N = B * K
    if kind == "noise":
        lg = (torch.rand(N, C, 28, 28, generator=g) * 2 - 1) * 4
    else:
        yy, xx = torch.meshgrid(torch.arange(28.), torch.arange(28.), indexing="ij")
        r = ((yy - 13.5) ** 2 + (xx - 13.5) ** 2).sqrt()
        lg = (9.0 - r)[None, None] + torch.rand(N, C, 1, 1, generator=g) * 2
    xy = torch.rand(B, K, 2, generator=g) * torch.tensor([W - 64.0, H - 64.0])
    wh = 16 + torch.rand(B, K, 2, generator=g) * torch.tensor([384.0, 256.0])        # boxes of 16 .. 400 x 16 .. 272 pixels
    boxes = torch.cat([xy, xy + wh], 2)
    labels = torch.randint(0, C, (B, K), generator=g)
    count = torch.full((B,), K, dtype=torch.int32)
    lg = lg.to(torch.bfloat16).to(DEV).contiguous(memory_format=torch.channels_last)  # the mask head's own dtype and layout
    return lg, labels.to(DEV), boxes.to(DEV), count.to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_bench.json"))
    a = ap.parse_args()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = dict(device=torch.cuda.get_device_name(0), shape=dict(B=B, K=K, C=C, mask=f"{H}x{W}", logits="bf16 channels-last"),
               iters_per_round=a.iters, rounds=a.reps,
               unit="microseconds; paste, paste_encode, paste_rle: per graph replay; host and to_lists: per eager call between two "
                    "synchronisations (host is not like for like: it pays a synchronisation and the copy of the bitmaps); spread = max - "
                    "min over the rounds; the device arms take turns inside every round")
    for kind in ("blob", "noise"):
        lg, labels, boxes, count = inputs(kind)
        bitmaps = torch.empty(B, K, H, W, dtype=torch.uint8, device=DEV)
        enc_a, enc_b = (rle.RleMasks.allocate(B * K, H, W, DEV, None, B, K, count) for _ in range(2))

        def paste():
            ops.paste_masks(lg, labels, boxes, count, 0.5, (H, W), out=bitmaps)

        def paste_encode():
            ops.rle_encode(ops.paste_masks(lg, labels, boxes, count, 0.5, (H, W), out=bitmaps), count, out=enc_a)

        def paste_rle():
            ops.paste_masks_rle(lg, labels, boxes, count, 0.5, (H, W), out=enc_b)

        def host():
            m = bitmaps.cpu().numpy()
            n = count.tolist()
            return [[rle.rle_to_string(rle.rle_encode(m[b, k])) for k in range(n[b])] for b in range(B)]

        graphs = dict(paste=_capture(paste, side), paste_encode=_capture(paste_encode, side), paste_rle=_capture(paste_rle, side))
        torch.cuda.synchronize()
        total = int(enc_a.offsets[-1])
        same = bool(torch.equal(enc_a.offsets, enc_b.offsets) and torch.equal(enc_a.runs[:total].view(torch.int32), enc_b.runs[:total].view(torch.int32)))
        out = _time(graphs, side, a.iters, a.reps)
        out["to_lists"] = _eager(enc_b.to_lists, a.reps)
        out["host"] = _eager(host, max(1, a.reps // 2))
        lists = enc_b.to_lists()
        out["facts"] = dict(fused_runs_equal_the_bitmap_route=same, runs=total, capacity=enc_b.capacity,
                            runs_per_column=round(total / (B * K * W), 2), bitmap_bytes=B * K * H * W, run_bytes=4 * total,
                            strings_equal_the_host_path=bool([[d["counts"] for d in img] for img in lists] == host()))
        res[kind] = out
        print(json.dumps({kind: out}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        del graphs
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
