#!/usr/bin/env python3
"""Write tests/golden/heads_list_form.npz: what MiniMaskRCNN's two target stages gave for LISTS of annotations on commit d875d97, the
last one whose list form had its own sampler, box encoding and mask sampling (image by image, unstable argsort, all gt bitmaps sampled).

    python tools/gen_heads_list_golden.py [--out tests/golden/heads_list_form.npz]

Since that commit a list is padded on entry and runs the definitions the padded form runs, so this script documents the inputs of the
file; run today it reproduces the file through the padded path, it does not regenerate the truth.  The inputs are those of
tests/_heads_list_case.py (CPU, float32): the `heads` fixture of tests/test_assign_batch.py with counts (3, 7), random RPN outputs and
feature maps from seeded generators, 1000 fixed proposals per image, and a rand_like stand-in whose keys are all distinct, so that no
outcome depends on a tie and the unstable and the stable sort agree.  The script runs the case twice and refuses to write unless the
two runs agree on every bit.

Contents: data only.  counts, seeds [rpn, fpn, proposals, keys], proposals f32 [2, 1000, 4]; loss_rpn_cls, loss_rpn_bbox
(_rpn_losses_and_proposals), loss_cls, loss_bbox, loss_mask (_roi_losses) as f32 scalars; rois_box f32 [2, 512, 4] and rois_mask f32
[2, 128, 4], the RoIs handed to the two roi_align calls."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "heads_list_form.npz")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import _heads_list_case as case
    m, tg = case.model(), case.targets()
    rpn_outs, fpn, proposals = case.inputs()
    first, second = (case.run(m, tg, rpn_outs, fpn, proposals) for _ in range(2))
    if not all(torch.equal(first[k], second[k]) for k in first):
        raise SystemExit(f"refused: two runs differ in {[k for k in first if not torch.equal(first[k], second[k])]}")
    d = {k: v.numpy() for k, v in first.items()}
    d.update(counts=np.asarray(case.COUNTS), proposals=torch.stack(proposals).numpy(),
             seeds=np.asarray([case.SEED_RPN, case.SEED_FPN, case.SEED_PROPOSALS, case.SEED_KEYS]))
    np.savez_compressed(a.out, **d)
    print(f"wrote {a.out}: " + ", ".join(f"{k} {float(first[k]):.9g}" for k in first if k.startswith("loss")) +
          f", {os.path.getsize(a.out) / 1024:.1f} KiB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
