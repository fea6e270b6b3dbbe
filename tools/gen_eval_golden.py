#!/usr/bin/env python3
"""Write tests/golden/eval_map.npz: what the reference's eval_map and tpfp_default return for a small fixed data set.

Build machine only: it needs the reference tree (PSWIN_REFERENCE_ROOT, default /root/reference, as oracle/ref_loader.py).  Three of the
reference's files are imported from where they lie -- mmdet/core/evaluation/mean_ap.py, bbox_overlaps.py and class_names.py -- inside an
empty stand-in package, so that no __init__.py of mmdet runs, with three stand-ins for what the machine does not have: mmcv (print_log,
is_str), terminaltables.AsciiTable, and multiprocessing.Pool (a serial starmap).  Nothing under the reference root is written (no
bytecode either) and the interpreter is left as it was found.

The data set: 12 images, 4 classes, at most K = 16 detections per image, coordinates multiples of 0.25, scores distinct within a class
(asserted: the reference leaves equal scores to an unstable sort).  It holds ignored boxes on some images, two identical ground-truth
boxes in one image, detections whose best IoU is exactly 0.5 and exactly 0.75, an image without boxes, an image without detections and a
class (3) without ground truth anywhere.

Stored per case (iou_thr 0.5 / 0.75, without ranges and with scale_ranges = [(0, 8), (8, 1e5)]): tpfp_default's marks per image and class
(recoded 1 = tp, 2 = fp, 0 = neither, in the padded row layout of evaluation.padded_from_lists) and eval_map's ap, num_gts, num_dets,
recall and precision curves and mean_ap.  A case is written only if evaluation.eval_map_lists reproduces it: marks exactly, AP within one
float32 spacing, mean_ap within 1e-6 relative.  Fixed zip time stamps: a second run gives the same bytes.

    python tools/gen_eval_golden.py [--out tests/golden/eval_map.npz]
"""
import argparse
import importlib
import io
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("PSWIN_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "eval_map.npz")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ABOUT = ("Reference results of mmdet/core/evaluation/mean_ap.py (tools/gen_eval_golden.py) on 12 images, 4 classes, K = 16.  in_*: the data "
         "set in the padded layout of evaluation.padded_from_lists (detections class by class, ignored boxes behind the regular ones); "
         "<case>_marks uint8 [S, B, K]: tpfp_default per image and class, 1 = tp, 2 = fp, 0 = neither; <case>_ap f32 [S, C], _num_gts "
         "[S, C], _num_dets [C], _mean_ap f64 [S], _recall f64 / _precision f32 [S, sum of num_dets] (classes concatenated) from eval_map.  "
         "Cases: thr50 / thr75 (no ranges, S = 1), thr50_ranges / thr75_ranges (scale_ranges (0, 8), (8, 1e5)).")

NUM_IMAGES, NUM_CLASSES, K = 12, 4, 16
SCALE_RANGES = [(0, 8), (8, 1e5)]
CASES = {"thr50": (0.5, None), "thr75": (0.75, None), "thr50_ranges": (0.5, SCALE_RANGES), "thr75_ranges": (0.75, SCALE_RANGES)}


class _SerialPool:
    def __init__(self, *a, **k):
        pass

    def starmap(self, fn, args):
        return [fn(*a) for a in args]

    def close(self):
        pass


class _AsciiTable:
    def __init__(self, data):
        self.table = "\n".join(" | ".join(str(c) for c in row) for row in data)


def load_reference():
    """mean_ap.py of the reference as a module, Pool replaced by the serial stand-in; sys.modules and the bytecode flag as before"""
    evdir = os.path.join(REFERENCE_ROOT, "mmdet", "core", "evaluation")
    pkg = types.ModuleType("_pswin_ref_eval")
    pkg.__path__ = [evdir]
    mmcv = types.ModuleType("mmcv")
    mmcv.is_str = lambda x: isinstance(x, str)
    mmcv.utils = types.ModuleType("mmcv.utils")
    mmcv.utils.print_log = lambda msg, logger=None: None
    tt = types.ModuleType("terminaltables")
    tt.AsciiTable = _AsciiTable
    stubs = {"_pswin_ref_eval": pkg, "mmcv": mmcv, "mmcv.utils": mmcv.utils, "terminaltables": tt}
    saved_flag, saved = sys.dont_write_bytecode, {n: sys.modules.get(n) for n in stubs}
    before = set(sys.modules)
    try:
        sys.dont_write_bytecode = True
        sys.modules.update(stubs)
        mod = importlib.import_module("_pswin_ref_eval.mean_ap")
    finally:
        sys.dont_write_bytecode = saved_flag
        for n in set(sys.modules) - before:
            if n in stubs or n.startswith("_pswin_ref_eval"):
                del sys.modules[n]
        for n, m in saved.items():
            if m is not None:
                sys.modules[n] = m
    mod.Pool = _SerialPool
    return mod


def _q(v):
    return np.round(np.asarray(v, dtype=np.float64) * 4) / 4


def dataset():
    """(det_results, annotations) in eval_map's form"""
    rng = np.random.RandomState(20241019)
    gts = [[] for _ in range(NUM_IMAGES)]          # (box, label, ignored)
    dets = [[] for _ in range(NUM_IMAGES)]         # (box, label)
    for b in range(NUM_IMAGES):
        if b in (5, 9):                            # 5: no boxes at all (detections only); 9: filled by hand below
            continue
        for _ in range(rng.randint(2, 6)):
            x, y = _q(rng.uniform(0, 40, 2))
            w, h = _q(rng.uniform(2, 16, 2))
            gts[b].append(([x, y, x + w, y + h], int(rng.randint(0, 3)), bool(b % 3 == 0 and rng.rand() < 0.4)))
    for b in range(NUM_IMAGES):
        if b == 7:                                 # an image without detections
            continue
        for box, lab, _ in gts[b]:
            for _ in range(rng.randint(0, 3)):     # jittered copies of a box: matches, duplicates and near misses
                j = _q(rng.uniform(-2.5, 2.5, 4))
                d = [box[0] + j[0], box[1] + j[1], max(box[2] + j[2], box[0] + j[0] + 0.25), max(box[3] + j[3], box[1] + j[1] + 0.25)]
                dets[b].append((d, lab if rng.rand() < 0.85 else int(rng.randint(0, 4))))
        for _ in range(rng.randint(1, 4)):         # detections of nothing, small and large, class 3 among them
            x, y = _q(rng.uniform(0, 48, 2))
            w, h = _q(rng.uniform(1, 12, 2))
            dets[b].append(([x, y, x + w, y + h], int(rng.randint(0, 4))))
    # image 9 by hand: two identical boxes of class 0 and detections whose best IoU is exactly 0.5 and exactly 0.75
    gts[9] = [([0, 0, 8, 4], 0, False), ([0, 0, 8, 4], 0, False), ([20, 20, 28, 24], 1, False), ([40, 0, 48, 4], 1, False),
              ([40, 10, 48, 14], 2, True), ([40, 10, 48, 14], 2, False)]
    dets[9] = [([0, 0, 8, 4], 0), ([0, 0, 8, 3], 0), ([0, 0, 8, 2], 0), ([20, 20, 28, 22], 1), ([20, 20, 28, 23], 1), ([40, 0, 46, 4], 1),
               ([40, 10, 48, 14], 2), ([40, 10, 48, 13], 2), ([2, 2, 3, 3], 3)]
    total = sum(len(d) for d in dets)
    scores = (rng.permutation(total) + 1).astype(np.float32) / np.float32(total + 1)       # all distinct
    det_results, annotations, n = [], [], 0
    for b in range(NUM_IMAGES):
        dets[b] = dets[b][:K]
        per_class = [[] for _ in range(NUM_CLASSES)]
        for box, lab in dets[b]:
            per_class[lab].append(list(box) + [scores[n]])
            n += 1
        det_results.append([np.asarray(p, dtype=np.float32).reshape(-1, 5) for p in per_class])
        reg, ign = [g for g in gts[b] if not g[2]], [g for g in gts[b] if g[2]]
        annotations.append(dict(bboxes=np.asarray([g[0] for g in reg], dtype=np.float32).reshape(-1, 4),
                                labels=np.asarray([g[1] for g in reg], dtype=np.int64),
                                bboxes_ignore=np.asarray([g[0] for g in ign], dtype=np.float32).reshape(-1, 4),
                                labels_ignore=np.asarray([g[1] for g in ign], dtype=np.int64)))
    for c in range(NUM_CLASSES):
        s = np.concatenate([r[c][:, 4] for r in det_results])
        assert len(np.unique(s)) == len(s), f"class {c}: scores must be distinct"
    return det_results, annotations


def reference_case(ref, det_results, annotations, iou_thr, scale_ranges):
    """tpfp_default's marks in the padded row layout and eval_map's results"""
    S = 1 if scale_ranges is None else len(scale_ranges)
    area_ranges = None if scale_ranges is None else [(r[0] ** 2, r[1] ** 2) for r in scale_ranges]
    marks = np.zeros((S, NUM_IMAGES, K), dtype=np.uint8)
    for b in range(NUM_IMAGES):
        row = 0
        for c in range(NUM_CLASSES):
            cls_dets, cls_gts, cls_ign = ref.get_cls_results(det_results[b:b + 1], annotations[b:b + 1], c)
            tp, fp = ref.tpfp_default(cls_dets[0], cls_gts[0], cls_ign[0], iou_thr, area_ranges)
            assert not np.any((tp > 0) & (fp > 0))
            n = cls_dets[0].shape[0]
            marks[:, b, row:row + n] = (tp > 0) * 1 + (fp > 0) * 2
            row += n
    mean_ap, results = ref.eval_map(det_results, annotations, scale_ranges=scale_ranges, iou_thr=iou_thr, logger="silent")
    out = dict(marks=marks,
               ap=np.stack([np.reshape(r["ap"], -1) for r in results], 1).astype(np.float32),
               num_gts=np.stack([np.reshape(r["num_gts"], -1) for r in results], 1).astype(np.int64),
               num_dets=np.asarray([r["num_dets"] for r in results], dtype=np.int64),
               mean_ap=np.reshape(np.asarray(mean_ap, dtype=np.float64), -1),
               recall=np.concatenate([np.reshape(r["recall"], (S, -1)) for r in results], 1).astype(np.float64),
               precision=np.concatenate([np.reshape(r["precision"], (S, -1)) for r in results], 1).astype(np.float32))
    return out


def check_case(det_results, annotations, iou_thr, scale_ranges, want):
    """evaluation.eval_map_lists and match_pairs reproduce the case: marks exactly, AP within a float32 spacing, mAP within 1e-6"""
    from panoswintransformerobjectdetection_amd import evaluation as ev
    dets, gts, ignore, C = ev.padded_from_lists(det_results, annotations)
    area_ranges = None if scale_ranges is None else [(r[0] ** 2, r[1] ** 2) for r in scale_ranges]
    marks = ev.match_pairs(ev.box_iou_pairs(dets, gts), dets, gts, ignore, (iou_thr,), area_ranges, ev.box_areas(dets.boxes),
                           ev.box_areas(gts.boxes))[0].numpy()
    assert dets.labels.shape[1] <= K and np.array_equal(marks, want["marks"][:, :, :marks.shape[2]]), "marks differ from tpfp_default"
    mean_ap, results = ev.eval_map_lists(det_results, annotations, scale_ranges=scale_ranges, iou_thr=iou_thr)
    got = np.stack([np.reshape(r["ap"], -1) for r in results], 1)
    assert np.all(np.abs(got.astype(np.float64) - want["ap"]) <= np.spacing(want["ap"])), (got, want["ap"])
    assert np.array_equal(np.stack([np.reshape(r["num_gts"], -1) for r in results], 1), want["num_gts"])
    assert np.array_equal([r["num_dets"] for r in results], want["num_dets"])
    assert np.allclose(np.reshape(mean_ap, -1), want["mean_ap"], rtol=1e-6, atol=0)


def write_npz(path, arrays):
    """np.savez_compressed with fixed zip time stamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, np.asarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from panoswintransformerobjectdetection_amd import evaluation as ev
    ref = load_reference()
    det_results, annotations = dataset()
    dets, gts, ignore, _ = ev.padded_from_lists(det_results, annotations)
    pad = K - dets.labels.shape[1]
    assert pad >= 0
    arrays = {"about": np.array(ABOUT),
              "in_det_boxes": np.pad(dets.boxes.numpy(), ((0, 0), (0, pad), (0, 0))), "in_det_scores": np.pad(dets.scores.numpy(), ((0, 0), (0, pad))),
              "in_det_labels": np.pad(dets.labels.numpy(), ((0, 0), (0, pad))), "in_det_count": dets.count.numpy(),
              "in_gt_boxes": gts.boxes.numpy(), "in_gt_labels": gts.labels.numpy(), "in_gt_count": gts.count.numpy(),
              "in_gt_ignore": ignore.numpy(), "scale_ranges": np.asarray(SCALE_RANGES, dtype=np.float64)}
    for name, (thr, ranges) in CASES.items():
        want = reference_case(ref, det_results, annotations, thr, ranges)
        check_case(det_results, annotations, thr, ranges, want)
        for k, v in want.items():
            arrays[f"{name}_{k}"] = v
        print(f"{name}: mean_ap {want['mean_ap']}, ap {want['ap'].tolist()}, tp {int((want['marks'] == 1).sum())} fp {int((want['marks'] == 2).sum())}")
    on_thr = ev.box_iou_pairs(dets, gts).max(2)[0]
    assert (on_thr == 0.5).any() and (on_thr == 0.75).any(), "the set must hold best IoUs exactly on both thresholds"
    write_npz(a.out, arrays)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
