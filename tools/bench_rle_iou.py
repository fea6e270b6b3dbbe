#!/usr/bin/env python3
"""Time the mask metric from the masks' run-length encoding (csrc/pswin_rle_iou.hip) against the same metric from bitmaps.

    python tools/bench_rle_iou.py [--iters 50] [--reps 5] [--out profiles/rle_iou_bench.json]

Shape: B = 8 images, K = 100 detections, Gmax = 32 and 100 boxes, C = 80 classes, 512 x 1024 masks.  The detections' masks are the paste of
"blob" logits (a disc per detection, the trained-model case) or "noise" logits (the random-initialisation worst case); the boxes' masks
are blobs, their labels random, so about one pair in 80 is of one class.
    inter_rle / inter_bitmap         pswin_rle_inter_pairs on the runs against pswin_mask_inter_pairs on the bitmaps of the same masks
    update_rle / update_bitmap       CocoAccumulator.update(segm) from runs on both sides against the same call from bitmaps
    predict_rle / predict_bitmap     ops.paste_masks_rle + the update from runs against ops.paste_masks + the update from bitmaps
    peak memory                      torch's peak of allocated bytes over one eager predict_* call, the route's targets included, above
                                     what was allocated before (the logits, boxes and labels)
The six arms are captured once each and replayed in turn, --reps rounds of --iters replays, in one process.  Figures are microseconds;
rounds, their median and spread (max - min).  "faster" may be said only where a difference exceeds both arms' spread."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_rle import B, C, DEV, H, K, W, inputs  # noqa: E402
from bench_targets import _capture, _time  # noqa: E402
from panoswintransformerobjectdetection_amd import evaluation as ev  # noqa: E402
from panoswintransformerobjectdetection_amd import ops, rle  # noqa: E402
from panoswintransformerobjectdetection_amd.detector import Detections, PaddedTargets  # noqa: E402


def _peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del keep
    torch.cuda.empty_cache()
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_iou_bench.json"))
    a = ap.parse_args()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = dict(device=torch.cuda.get_device_name(0), shape=dict(B=B, K=K, C=C, mask=f"{H}x{W}", logits="bf16 channels-last"),
               iters_per_round=a.iters, rounds=a.reps,
               unit="microseconds per graph replay; spread = max - min over the rounds; the arms take turns inside every round; peak "
                    "memory in bytes")
    for kind in ("blob", "noise"):
        for G in (32, 100):
            lg, labels, boxes, count = inputs(kind)
            glg, glabels, gboxes, gcount = inputs("blob", seed=1)                          # the boxes' masks: blobs
            gl, gb = glabels[:, :G].contiguous(), gboxes[:, :G].contiguous()
            gc = torch.full((B,), G, dtype=torch.int32, device=DEV)
            glg = glg.reshape(B, K, C, 28, 28)[:, :G].reshape(B * G, C, 28, 28).contiguous(memory_format=torch.channels_last)
            scores = torch.linspace(0.99, 0.01, B * K, device=DEV).reshape(B, K).contiguous()
            source = torch.zeros(B, K, dtype=torch.int32, device=DEV)

            def targets(bitmaps):
                if bitmaps:
                    return PaddedTargets(gb, gl, gc, masks=ops.paste_masks(glg, gl, gb, gc, 0.5, (H, W)))
                return PaddedTargets(gb, gl, gc, rle=ops.paste_masks_rle(glg, gl, gb, gc, 0.5, (H, W)))

            def predict(bitmaps, acc, tg, out=None):
                if bitmaps:
                    d = Detections(boxes, scores, labels, count, source, masks=ops.paste_masks(lg, labels, boxes, count, 0.5, (H, W), out=out))
                else:
                    d = Detections(boxes, scores, labels, count, source, rle=ops.paste_masks_rle(lg, labels, boxes, count, 0.5, (H, W), out=out))
                return d, acc.update(d, tg)

            def route(bitmaps):
                tg = targets(bitmaps)
                return tg, predict(bitmaps, ev.CocoAccumulator(C, iou="segm", max_per_img=K, device=DEV), tg)

            for key in [k for k in ops._CACHE if k[0] == "rle_ws"]:                        # the encoder's workspace counts towards its route
                del ops._CACHE[key]
            peak = dict(rle=_peak(lambda: route(False)), bitmap=_peak(lambda: route(True)))
            t_rle, t_bit = targets(False), targets(True)
            bitmaps = ops.paste_masks(lg, labels, boxes, count, 0.5, (H, W))
            enc = ops.paste_masks_rle(lg, labels, boxes, count, 0.5, (H, W), out=rle.RleMasks.allocate(B * K, H, W, DEV, None, B, K, count))
            d_rle = Detections(boxes, scores, labels, count, source, rle=enc)
            d_bit = Detections(boxes, scores, labels, count, source, masks=bitmaps)
            out_rle = (torch.empty(B, K, G, dtype=torch.int32, device=DEV), torch.empty(B, K + G, dtype=torch.int32, device=DEV),
                       torch.zeros(1, dtype=torch.int32, device=DEV))
            out_bit = (torch.empty(B, K, G, dtype=torch.int32, device=DEV), torch.empty(B, K + G, dtype=torch.int32, device=DEV))
            ws = ev.rle_inter_workspace(B, K, G, enc.capacity, t_rle.rle.capacity, DEV)
            accs = {k: ev.CocoAccumulator(C, iou="segm", max_per_img=K, device=DEV) for k in ("ur", "ub", "pr", "pb")}
            flags = {}
            enc2 = rle.RleMasks.allocate(B * K, H, W, DEV, None, B, K, count)
            bitmaps2 = torch.empty_like(bitmaps)

            def upd(key, d, tg):
                flags[key] = accs[key].update(d, tg)

            def pre(key, bm, tg, out):
                flags[key] = predict(bm, accs[key], tg, out)[1]

            graphs = dict(inter_rle=_capture(lambda: ev.rle_inter_pairs_dispatch(d_rle, t_rle, out=out_rle, workspace=ws), side),
                          inter_bitmap=_capture(lambda: ev.mask_inter_pairs_dispatch(d_bit, t_bit, out=out_bit), side),
                          update_rle=_capture(lambda: upd("ur", d_rle, t_rle), side),
                          update_bitmap=_capture(lambda: upd("ub", d_bit, t_bit), side),
                          predict_rle=_capture(lambda: pre("pr", False, t_rle, enc2), side),
                          predict_bitmap=_capture(lambda: pre("pb", True, t_bit, bitmaps2), side))
            torch.cuda.synchronize()
            out = _time(graphs, side, a.iters, a.reps)                                     # (the flags exist only once a graph has been replayed)
            same = bool(torch.equal(out_rle[0], out_bit[0]) and torch.equal(out_rle[1], out_bit[1]) and torch.equal(flags["ur"], flags["ub"]) and
                        torch.equal(flags["pr"], flags["pb"]))
            pairs = int((out_rle[0] >= 0).sum())
            out["facts"] = dict(rle_results_equal_the_bitmap_route=same, rle_overflow=int(out_rle[2]), same_class_pairs=pairs,
                                pairs_that_meet=int((out_rle[0] > 0).sum()), det_runs=int(enc.offsets[-1]), det_capacity=enc.capacity,
                                gt_runs=int(t_rle.rle.offsets[-1]), gt_capacity=t_rle.rle.capacity, workspace_bytes=int(ws.numel()),
                                bitmap_bytes_read=(B * (K + G) + 2 * pairs) * H * W, images_scored=int(accs["ur"].cursor),
                                peak_memory=peak)
            res[f"{kind}_g{G}"] = out
            print(json.dumps({f"{kind}_g{G}": out}), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
            del graphs, accs, bitmaps, bitmaps2, enc, enc2, ws, t_rle, t_bit, d_rle, d_bit
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
