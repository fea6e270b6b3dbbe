#!/usr/bin/env python3
"""Time the rasterisation of a batch's polygon annotations on the device (csrc/pswin_poly.hip: pswin_poly_masks; the runs through pswin_rle_encode) against
what users do without it.

    python tools/bench_polygons.py [--iters 50] [--reps 5] [--out profiles/polygons_bench.json]

Shape: B = 8 images, K = 32 objects, 512 x 1024 masks (134 MB of bitmaps), one star polygon of 16 or of 256 vertices per object.
    poly_masks             polygons.polygons_to_masks: the bitmaps from the polygons on the device
    poly_rle               polygons.polygons_to_rle: the bitmaps into a scratch buffer, then rle.encode_masks of them
    upload                 the copy alone of bitmaps rasterised in advance, from pinned host memory: the best case of what users do today
    host                   polygons_to_masks_definition on the host plus that upload, an eager call between two synchronisations; the
                           definition is plain Python loops, far slower than pycocotools' C would be
The arms are NOT like for like: the first two read a few tens of kilobytes of vertices on the device, `upload` moves 134 MB over the
host link and rasterises nothing, `host` runs an interpreter.  The three device arms are captured once each and replayed in turn, --reps
rounds of --iters replays, in one process.  Figures are microseconds; rounds, their median and spread (max - min).  "faster" may be said
only where a difference exceeds both arms' spread."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_eval import _eager  # noqa: E402
from bench_targets import _capture, _time  # noqa: E402
from panoswintransformerobjectdetection_amd import polygons, rle  # noqa: E402

B, K, H, W = 8, 32, 512, 1024
DEV = "cuda:0"


def stars(n_vertices, seed=0):
    g = torch.Generator().manual_seed(seed)
    ann = []
    for _ in range(B):
        per = []
        for _ in range(K):
            cx, cy, r, ph = (float(v) for v in torch.rand(4, generator=g))
            cx, cy, r = cx * W, cy * H, 16 + r * 180
            part = []
            for i in range(n_vertices):
                rr = r if i % 2 == 0 else 0.45 * r
                a = ph + 2 * math.pi * i / n_vertices
                part += [cx + rr * math.cos(a), cy + rr * math.sin(a)]
            per.append([part])
        ann.append(per)
    return ann


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polygons_bench.json"))
    a = ap.parse_args()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = dict(device=torch.cuda.get_device_name(0), shape=dict(B=B, K=K, mask=f"{H}x{W}", parts_per_object=1),
               iters_per_round=a.iters, rounds=a.reps,
               unit="microseconds; poly_masks, poly_rle, upload: per graph replay; host: per eager call between two synchronisations; "
                    "spread = max - min over the rounds; the replayed arms take turns inside every round; the arms are not like for like "
                    "(see the tool's docstring)")
    for n in (16, 256):
        ann = stars(n)
        host_batch = polygons.PolygonBatch.from_lists(ann, H, W, "cpu", K=K)
        polys = polygons.PolygonBatch.from_lists(ann, H, W, DEV, K=K)
        bitmaps = torch.empty(B, K, H, W, dtype=torch.uint8, device=DEV)
        uploaded = torch.empty_like(bitmaps)
        enc = rle.RleMasks.allocate(B * K, H, W, DEV, None, B, K, polys.count)

        def poly_masks():
            polygons.polygons_to_masks(polys, out=bitmaps)

        def poly_rle():
            polygons.polygons_to_rle(polys, out=enc)

        graphs = dict(poly_masks=_capture(poly_masks, side), poly_rle=_capture(poly_rle, side))
        torch.cuda.synchronize()
        pinned = bitmaps.cpu().pin_memory()                                      # "rasterised in advance": the device's own answer

        def upload():
            uploaded.copy_(pinned, non_blocking=True)

        def host():
            uploaded.copy_(polygons.polygons_to_masks_definition(host_batch))

        graphs["upload"] = _capture(upload, side)
        out = _time(graphs, side, a.iters, a.reps)
        out["host"] = _eager(host, 1)
        torch.cuda.synchronize()
        via = rle.encode_masks(bitmaps, polys.count, capacity=enc.capacity)
        total = int(enc.offsets[-1])
        out["facts"] = dict(vertices_per_part=n, vertex_bytes=16 * B * K * n, bitmap_bytes=B * K * H * W, runs=total, run_bytes=4 * total,
                            foreground_fraction=round(float(bitmaps.float().mean()), 4),
                            masks_equal_the_host_definition=bool(torch.equal(bitmaps, uploaded)),
                            runs_equal_the_bitmap_route=bool(torch.equal(via.offsets, enc.offsets) and
                                                             torch.equal(via.runs[:total].view(torch.int32), enc.runs[:total].view(torch.int32))))
        res[f"star_{n}"] = out
        print(json.dumps({f"star_{n}": out}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        del graphs
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
