#!/usr/bin/env python3
"""Write tests/golden/max_iou_assign_batch.npz: what the reference's MaxIoUAssigner returns for the boxes of tests/_assign_cases.py.

Build machine only: it needs the reference tree (PSWIN_REFERENCE_ROOT, default /root/reference, as oracle/ref_loader.py).  It imports
mmdet/core/bbox/assigners/max_iou_assigner.py (with its AssignResult, BboxOverlaps2D and the two builders) from where it lies.  The
packages around those files are empty stand-ins whose __path__ points at the reference's directories, so that no __init__.py of mmdet
runs, and mmcv.utils is a Registry / build_from_cfg stand-in.  Nothing under the reference root is written, and the interpreter is
left as it was found.

    python tools/gen_assign_golden.py [--out tests/golden/max_iou_assign_batch.npz]

Contents: data only.  cand f32 [N, 4], gt f32 [3, 9, 4] with count [0, 1, 9], thresholds [3, 4] (pos, neg, min_pos, match_low_quality);
per threshold set and image the reference's gt_inds / max_overlaps for the candidates alone ([3, 3, N]) and for cat(gt[:count], cand)
-- add_gt_as_proposals -- laid out as the padded batch form returns it ([3, 3, 9 + N]: rows count .. 8 are padding, -1).
A case is written only if detector.max_iou_assign on the CPU reproduces the reference's gt_inds exactly and its max_overlaps bit for
bit (box_iou's maximum)."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("PSWIN_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "max_iou_assign_batch.npz")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, GMAX, COUNTS = 3000, 9, (0, 1, 9)


def load_reference(root=REFERENCE_ROOT):
    """The reference's MaxIoUAssigner class, or None when its tree is not on this machine."""
    mmdet = os.path.join(root, "mmdet")
    if not os.path.isfile(os.path.join(mmdet, "core", "bbox", "assigners", "max_iou_assigner.py")):
        return None

    class Registry(dict):
        def __init__(self, name):
            super().__init__()
            self.name = name

        def register_module(self, *a, **k):
            def deco(cls):
                self[cls.__name__] = cls
                return cls
            return deco

    def build_from_cfg(cfg, registry, default_args=None):
        args = dict(default_args or {}, **cfg)
        return registry[args.pop("type")](**args)

    def package(name, *parts):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(mmdet, *parts)]
        return m

    stubs = {"mmcv": types.ModuleType("mmcv"), "mmcv.utils": types.ModuleType("mmcv.utils"),
             "mmdet": package("mmdet"), "mmdet.utils": package("mmdet.utils", "utils"), "mmdet.core": package("mmdet.core", "core"),
             "mmdet.core.bbox": package("mmdet.core.bbox", "core", "bbox"),
             "mmdet.core.bbox.assigners": package("mmdet.core.bbox.assigners", "core", "bbox", "assigners")}
    stubs["mmcv"].__path__ = []
    stubs["mmcv.utils"].__dict__.update(Registry=Registry, build_from_cfg=build_from_cfg)
    saved_flag, saved = sys.dont_write_bytecode, {n: sys.modules.get(n) for n in stubs}
    before = set(sys.modules)
    try:
        sys.dont_write_bytecode = True
        sys.modules.update(stubs)
        return importlib.import_module("mmdet.core.bbox.assigners.max_iou_assigner").MaxIoUAssigner
    except ImportError:
        return None
    finally:
        sys.dont_write_bytecode = saved_flag
        for n in set(sys.modules) - before:
            if n in stubs or n.startswith("mmdet.") or n.startswith("mmcv."):
                del sys.modules[n]
        for n, m in saved.items():
            if m is not None:
                sys.modules[n] = m
            else:
                sys.modules.pop(n, None)


def reference_assign(cls, cand, gt, thr):
    pos, neg, min_pos, low = thr
    r = cls(pos_iou_thr=pos, neg_iou_thr=neg, min_pos_iou=min_pos, match_low_quality=low, ignore_iof_thr=-1).assign(cand, gt)
    return r.gt_inds.long(), r.max_overlaps.float()


def checked(cls, cand, gt, thr):
    """The reference's (gt_inds, max_overlaps) for one image, refused unless the project's CPU statement reproduces both."""
    from panoswintransformerobjectdetection_amd.detector import box_iou, max_iou_assign
    inds, ovl = reference_assign(cls, cand, gt, thr)
    mine = max_iou_assign(cand, gt, *thr)
    best = box_iou(gt, cand).max(0)[0] if gt.shape[0] else torch.zeros(cand.shape[0])
    if not torch.equal(mine, inds):
        raise SystemExit(f"refused: detector.max_iou_assign differs from the reference in {int((mine != inds).sum())} gt_inds ({thr}, G={gt.shape[0]})")
    if not torch.equal(best.view(torch.int32), ovl.view(torch.int32)):
        raise SystemExit(f"refused: box_iou's maximum differs from the reference's max_overlaps in bits ({thr}, G={gt.shape[0]})")
    return inds.numpy(), ovl.numpy()


def generate(cls):
    import _assign_cases as ac
    gts = [ac.gt_boxes(g, seed=10 + g) for g in COUNTS]
    cand = ac.candidates(N, gts[-1], seed=1)
    gt, count = ac.padded_gt(gts, GMAX)
    T = len(ac.THRESHOLDS)
    d = dict(cand=cand, gt=gt, count=count, thresholds=np.asarray([[p, n, m, float(q)] for p, n, m, q in ac.THRESHOLDS], np.float64),
             gt_inds=np.zeros((T, len(COUNTS), N), np.int64), max_overlaps=np.zeros((T, len(COUNTS), N), np.float32),
             lead_gt_inds=np.full((T, len(COUNTS), GMAX + N), -1, np.int64), lead_max_overlaps=np.full((T, len(COUNTS), GMAX + N), -1, np.float32))
    c = torch.from_numpy(cand)
    for t, thr in enumerate(ac.THRESHOLDS):
        for b, g in enumerate(gts):
            g = torch.from_numpy(g)
            G = g.shape[0]
            d["gt_inds"][t, b], d["max_overlaps"][t, b] = checked(cls, c, g, thr)
            inds, ovl = checked(cls, torch.cat([g, c]), g, thr)
            d["lead_gt_inds"][t, b, :G], d["lead_max_overlaps"][t, b, :G] = inds[:G], ovl[:G]
            d["lead_gt_inds"][t, b, GMAX:], d["lead_max_overlaps"][t, b, GMAX:] = inds[G:], ovl[G:]
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    cls = load_reference()
    if cls is None:
        print(f"reference not found under {REFERENCE_ROOT}", file=sys.stderr)
        return 1
    d = generate(cls)
    np.savez_compressed(a.out, **d)
    gi = d["gt_inds"]
    print(f"wrote {a.out}: N = {N}, counts {COUNTS}, per threshold set positives {[(int((gi[t] > 0).sum())) for t in range(gi.shape[0])]}, "
          f"ignored {[(int((gi[t] < 0).sum())) for t in range(gi.shape[0])]}, exact 0.5 overlaps {int((d['max_overlaps'] == 0.5).sum())}, "
          f"{os.path.getsize(a.out) / 1024:.1f} KiB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
