#!/usr/bin/env python3
"""Write tests/golden/recall.npz: what the reference's proposal recall (mmdet/core/evaluation/recall.py) returns for a small fixed data set.

Build machine only: it needs the reference tree (PSWIN_REFERENCE_ROOT, as tools/gen_eval_golden.py).  recall.py and bbox_overlaps.py are
imported from where they lie inside an empty stand-in package, with stand-ins for mmcv.utils.print_log and terminaltables.AsciiTable.
Nothing under the reference root is written (no bytecode either) and the interpreter is left as it was found.

HOW THE REFERENCE IS CALLED.  eval_recalls builds np.array() of the per-image IoU matrices, which current numpy refuses as soon as two
images differ in their counts.  So the reference's bbox_overlaps is called per image (on the proposals in descending score, cut at the
last proposal number, as eval_recalls cuts them) and its _recalls on an explicitly built object array; eval_recalls itself is called whole
on the images that share their counts, and both routes are asserted to agree there.

THE ROUNDS.  _recalls returns recalls only.  The greedy matching takes the largest IoU left in every round, so the values it records
never rise from one round to the next: the rounds ARE the recorded values in descending order.  They are recovered from the reference by
calling _recalls on one image and one proposal number with every value the image's IoU matrix holds (and 0 and -1) as a threshold: the
number of recorded values at or above each gives the multiset.  float32 values widened to float64 compare exactly.

The data set: 12 images, at most 8 boxes and 40 proposals, coordinates multiples of 0.25, distinct scores (asserted: the reference leaves
equal scores to an unstable sort), proposals stored in shuffled order.  Proposal numbers (1, 3, 10, 40, 100), the thresholds
np.arange(0.5, 0.96, 0.05).
    0, 1   pairs whose IoU is exactly 10/20 .. 14/20 and 15/20 .. 19/20
    2      no boxes, some proposals            3   five boxes, two proposals           4   duplicated boxes and duplicated proposals
    5      a box disjoint from every proposal  6   four boxes that all prefer one proposal
    7      three boxes, no proposal            8, 9  four boxes, 40 proposals (equal counts: the whole eval_recalls runs on them)
    10     one of its boxes is ignored (dropped before the reference sees it, as fast_eval_recall drops them)      11  random
A case is written only if evaluation.eval_recalls_lists and proposal_round_ious reproduce it exactly.  Fixed zip time stamps: a second
run gives the same bytes.

    python tools/gen_recall_golden.py [--out tests/golden/recall.npz]
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("PSWIN_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "recall.npz")
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

from gen_eval_golden import _AsciiTable, write_npz  # noqa: E402

ABOUT = ("Reference results of mmdet/core/evaluation/recall.py (tools/gen_recall_golden.py) on 12 images.  in_gt_boxes f32 [B, 8, 4], "
         "in_gt_count, in_gt_ignore bool [B, 8]; in_props f32 [B, 40, 5] (x1, y1, x2, y2, score; shuffled order, distinct scores), "
         "in_prop_count; proposal_nums [Kn], iou_thrs f64 [T].  ref_recalls f64 [Kn, T]: _recalls on all images; ref_ar f64 [Kn]: its mean "
         "over the thresholds; ref_rounds f32 [Kn, B, 8]: per (number, image) the IoU recorded in every round, recovered from _recalls, -2 "
         "past the image's regular boxes; equal_count_images: the images eval_recalls itself ran on.")

NUM_IMAGES, GMAX, PMAX = 12, 8, 40
PROPOSAL_NUMS = (1, 3, 10, 40, 100)
IOU_THRS = np.arange(0.5, 0.96, 0.05)


def load_reference():
    """recall.py of the reference as a module (its bbox_overlaps inside); sys.modules and the bytecode flag as before"""
    evdir = os.path.join(REFERENCE_ROOT, "mmdet", "core", "evaluation")
    pkg = types.ModuleType("_pswin_ref_recall")
    pkg.__path__ = [evdir]
    mmcv = types.ModuleType("mmcv")
    mmcv.utils = types.ModuleType("mmcv.utils")
    mmcv.utils.print_log = lambda msg, logger=None: None
    tt = types.ModuleType("terminaltables")
    tt.AsciiTable = _AsciiTable
    stubs = {"_pswin_ref_recall": pkg, "mmcv": mmcv, "mmcv.utils": mmcv.utils, "terminaltables": tt}
    saved_flag, saved = sys.dont_write_bytecode, {n: sys.modules.get(n) for n in stubs}
    before = set(sys.modules)
    try:
        sys.dont_write_bytecode = True
        sys.modules.update(stubs)
        mod = importlib.import_module("_pswin_ref_recall.recall")
    finally:
        sys.dont_write_bytecode = saved_flag
        for n in set(sys.modules) - before:
            if n in stubs or n.startswith("_pswin_ref_recall"):
                del sys.modules[n]
        for n, m in saved.items():
            if m is not None:
                sys.modules[n] = m
    return mod


def _q(v):
    return np.round(np.asarray(v, dtype=np.float64) * 4) / 4


def dataset():
    """(gts: per image [(box, ignored)], props: per image (k, 5) float32 in shuffled order)"""
    rng = np.random.RandomState(20241101)
    gts, props = [[] for _ in range(NUM_IMAGES)], [[] for _ in range(NUM_IMAGES)]
    for b, ks in ((0, range(10, 15)), (1, range(15, 20))):          # a 20 x 1 box and its first k columns: IoU k / 20
        for i, k in enumerate(ks):
            gts[b].append(([32 * i, 4 * i, 32 * i + 20, 4 * i + 1], False))
            props[b].append([32 * i, 4 * i, 32 * i + k, 4 * i + 1])
    props[2] = [[1, 1, 9, 9], [4, 4, 12, 20.5], [30, 2, 40, 8]]
    gts[3] = [([0, 0, 10, 10], False), ([20, 0, 30, 10], False), ([0, 20, 10, 30], False), ([20, 20, 30, 30], False), ([5, 5, 25, 25], False)]
    props[3] = [[1, 0, 10, 10], [6, 6, 24, 25]]
    gts[4] = [([0, 0, 8, 8], False), ([0, 0, 8, 8], False), ([20, 0, 28, 8], False), ([20, 0, 28, 8], False)]
    props[4] = [[0, 0, 8, 6], [0, 0, 8, 6], [0, 0, 8, 6], [20, 0, 28, 8], [20, 0, 26, 8], [20, 0, 26, 8]]
    gts[5] = [([100, 100, 110, 110], False), ([0, 0, 10, 10], False), ([20, 0, 30, 10], False)]
    props[5] = [[40, 40, 44, 44], [0, 0, 10, 9], [50, 50, 52, 52], [20, 0, 29, 10], [60, 0, 64, 4]]
    gts[6] = [([0, 0, 16, 16], False), ([0, 0, 16, 14], False), ([0, 0, 14, 16], False), ([2, 2, 16, 16], False)]
    props[6] = [[0, 0, 16, 16], [0, 0, 8, 8], [8, 8, 16, 16], [0, 0, 16, 4], [30, 30, 34, 34]]
    gts[7] = [([0, 0, 4, 4], False), ([8, 8, 12, 12.25], False), ([1, 1, 2, 2], False)]
    for b, ng, npr in ((8, 4, PMAX), (9, 4, PMAX), (10, 6, 17), (11, GMAX, 33)):
        for i in range(ng):
            x, y = _q(rng.uniform(0, 40, 2))
            w, h = _q(rng.uniform(3, 16, 2))
            gts[b].append(([x, y, x + w, y + h], b == 10 and i == 2))
        while len(props[b]) < npr:
            if rng.rand() < 0.7:                                   # a jittered copy of a box
                box = gts[b][rng.randint(ng)][0]
                j = _q(rng.uniform(-3, 3, 4))
                x1, y1 = box[0] + j[0], box[1] + j[1]
                props[b].append([x1, y1, max(box[2] + j[2], x1 + 0.25), max(box[3] + j[3], y1 + 0.25)])
            else:
                x, y = _q(rng.uniform(0, 48, 2))
                w, h = _q(rng.uniform(1, 12, 2))
                props[b].append([x, y, x + w, y + h])
    total = sum(len(p) for p in props)
    scores = (rng.permutation(total) + 1).astype(np.float32) / np.float32(total + 1)       # all distinct
    assert len(np.unique(scores)) == total
    out, at = [], 0
    for p in props:
        arr = np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1, 4), scores[at:at + len(p), None]], 1).astype(np.float32)
        at += len(p)
        out.append(arr)
    return gts, out


def reference_ious(ref, boxes, props):
    """per image the matrix eval_recalls hands to _recalls, from the reference's bbox_overlaps"""
    ious = []
    for g, p in zip(boxes, props):
        p = p[np.argsort(p[:, 4])[::-1]]                           # distinct scores: the reference's order
        n = min(p.shape[0], PROPOSAL_NUMS[-1])
        ious.append(np.zeros((0, p.shape[0]), dtype=np.float32) if g.shape[0] == 0 else ref.bbox_overlaps(g, p[:n, :4]))
    return ious


def _objects(mats):
    arr = np.empty(len(mats), dtype=object)
    for i, m in enumerate(mats):
        arr[i] = m
    return arr


def reference_rounds(ref, ious):
    """f32 [Kn, B, GMAX] recovered from _recalls, image by image and number by number (the module docstring says how)"""
    rounds = np.full((len(PROPOSAL_NUMS), len(ious), GMAX), -2.0, dtype=np.float32)
    for b, m in enumerate(ious):
        g = m.shape[0]
        if g == 0:
            continue
        cand = np.unique(np.concatenate([m.reshape(-1).astype(np.float64), [0.0, -1.0]]))[::-1]        # descending
        for k, num in enumerate(PROPOSAL_NUMS):
            at_least = np.rint(ref._recalls(_objects([m]), np.array([num]), cand)[0] * g).astype(int)
            assert at_least[-1] == g, "every recorded value is one of the candidates"
            vals = np.repeat(cand, np.diff(np.concatenate([[0], at_least])))
            rounds[k, b, :g] = vals.astype(np.float32)
    return rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch
    from panoswintransformerobjectdetection_amd import evaluation as ev
    from panoswintransformerobjectdetection_amd.detector import PaddedTargets, Proposals
    ref = load_reference()
    gts, props = dataset()
    regular = [np.asarray([g[0] for g in img if not g[1]], dtype=np.float32).reshape(-1, 4) for img in gts]
    nums, thrs = np.array(PROPOSAL_NUMS), IOU_THRS

    ious = reference_ious(ref, regular, props)
    recalls = ref._recalls(_objects(ious), nums, thrs)
    rounds = reference_rounds(ref, ious)
    equal = [b for b in range(NUM_IMAGES) if (regular[b].shape[0], props[b].shape[0]) == (regular[8].shape[0], props[8].shape[0])]
    assert len(equal) >= 2
    whole = ref.eval_recalls([regular[b] for b in equal], [props[b] for b in equal], PROPOSAL_NUMS, thrs)
    assert np.array_equal(whole, ref._recalls(_objects([ious[b] for b in equal]), nums, thrs)), "the two routes into the reference differ"

    # the definitions reproduce the case exactly, or nothing is written
    got = ev.eval_recalls_lists(regular, props, PROPOSAL_NUMS, thrs)
    assert got.dtype == np.float64 and np.array_equal(got, recalls), (got, recalls)
    B = NUM_IMAGES
    gt_boxes, gt_count = np.zeros((B, GMAX, 4), dtype=np.float32), np.zeros(B, dtype=np.int32)
    gt_ignore = np.zeros((B, GMAX), dtype=bool)
    in_props, prop_count = np.zeros((B, PMAX, 5), dtype=np.float32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        gt_count[b], prop_count[b] = len(gts[b]), props[b].shape[0]
        for i, (box, ign) in enumerate(gts[b]):
            gt_boxes[b, i], gt_ignore[b, i] = box, ign
        in_props[b, :prop_count[b]] = props[b]
    ordered = np.stack([p[np.argsort(-p[:, 4], kind="stable")] for p in in_props])          # the padding's score 0 sorts behind
    padded = Proposals(torch.from_numpy(ordered[:, :, :4].copy()), torch.from_numpy(ordered[:, :, 4].copy()), torch.from_numpy(prop_count))
    targets = PaddedTargets(torch.from_numpy(gt_boxes), torch.zeros(B, GMAX, dtype=torch.long), torch.from_numpy(gt_count))
    mine = ev.proposal_round_ious(padded, targets, PROPOSAL_NUMS, torch.from_numpy(gt_ignore))
    assert np.array_equal(mine.numpy().view(np.uint32), rounds.view(np.uint32)), "the rounds differ from the reference's"
    hits, num_gts = ev.recall_hits(mine, thrs)
    assert num_gts == sum(r.shape[0] for r in regular) and np.array_equal(hits.numpy() / float(num_gts), recalls)

    best = np.concatenate([m.max(1) for m in ious[:2]])
    assert sorted(best.tolist()) == [float(np.float32(k) / np.float32(20)) for k in range(10, 20)], "the ten exact fractions"
    assert gt_ignore.any() and (prop_count == 0).any() and ((gt_count > prop_count) & (prop_count > 0)).any()
    arrays = {"about": np.array(ABOUT), "in_gt_boxes": gt_boxes, "in_gt_count": gt_count, "in_gt_ignore": gt_ignore, "in_props": in_props,
              "in_prop_count": prop_count, "proposal_nums": nums.astype(np.int64), "iou_thrs": thrs.astype(np.float64),
              "ref_recalls": recalls.astype(np.float64), "ref_ar": recalls.mean(axis=1), "ref_rounds": rounds,
              "equal_count_images": np.asarray(equal, dtype=np.int64)}
    write_npz(a.out, arrays)
    print("recalls", recalls.tolist())
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
