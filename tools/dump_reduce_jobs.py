"""Print the grouped-reduction job list of one PanoSwin-T training step (rows, cols, dtype, blocks, MB)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from panoswintransformerobjectdetection_amd import SimplePanoSwinTransformer, grad_queue, ops

cfg = dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7, ape=True, drop_path_rate=0.2,
           pano_mode=True)
m = SimplePanoSwinTransformer(**cfg, compute_dtype=torch.bfloat16)
m.init_weights(None)
m = m.cuda().train()
x = torch.randn(8, 3, 512, 1024, device="cuda")
orig = grad_queue._launch_reductions


def spy(jobs):
    tot_b = tot_blk = 0
    for j in jobs:
        dt, rows, cols, ld = j.dtype, j.rows, j.cols, j.ld
        ve = 8 if dt == 1 else 4
        sh = 0 if rows <= 16 else (3 if rows <= 128 else 6)
        blocks = -(-(cols // ve) // (1024 >> sh))
        mb = rows * cols * (2 if dt == 1 else 4) / 1e6
        tot_b += mb
        tot_blk += blocks
        print(f"rows {rows:5d} cols {cols:8d} ld {ld:8d} {'bf16' if dt == 1 else 'f32 '} lanes {1 << sh:2d} blocks {blocks:5d} {mb:7.2f} MB")
    print(f"{len(jobs)} jobs, {tot_blk} blocks, {tot_b:.1f} MB")
    orig(jobs)


grad_queue._launch_reductions = spy
ops.set_deferred_reductions(True)
outs = m(x)
sum(o.float().mean() for o in outs).backward()
torch.cuda.synchronize()
