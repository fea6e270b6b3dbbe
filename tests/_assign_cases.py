"""Boxes for the target-assigner tests and for tools/gen_assign_golden.py: the cases in which an assigner can go wrong, at any size.

Ground truth (H x W = 256 x 512 image): integer boxes on an 8-pixel grid, an exact duplicate of the previous box, fractional boxes, a box
shifted by 8 pixels from an earlier one (equal IoUs with the grid candidates), a zero-area box and -- only with inverted=True, which the
reference's IoU does not clamp -- an inverted one.  Candidates: a copy of every gt (up to 16), the upper half of gt 0 (an IoU of exactly
0.5), zero-area and inverted boxes, then integer 32 x 32 / 64 x 32 boxes on the 8-pixel grid (ties between gts and between candidates)
alternating with fractional boxes.  The first candidate is always gt 0 itself, so N = 1 is a meaningful case."""
import numpy as np

H, W = 256, 512
THRESHOLDS = [(0.7, 0.3, 0.3, True), (0.5, 0.5, 0.5, True), (0.5, 0.5, 0.5, False)]      # (pos, neg, min_pos, match_low_quality) of the configs


def gt_boxes(G, seed, inverted=False):
    rng = np.random.RandomState(seed)
    out = []
    for g in range(G):
        kind = g % 6
        if g == 0:
            b = [16, 16, 80, 48]
        elif kind == 1:
            b = list(out[-1])                                       # a duplicate: the lowest index wins the argmax, the highest the low-quality loop
        elif kind == 3:
            p = out[g - 3]
            b = [p[0] + 8, p[1], p[2] + 8, p[3]]
        elif kind == 4:
            x, y = rng.randint(0, W), rng.randint(0, H - 40)
            b = [x, y, x, y + 40]                                   # zero area
        elif kind == 5 and inverted:
            x, y = rng.randint(40, W), rng.randint(0, H - 40)
            b = [x, y, x - 24, y + 40]
        elif kind in (2, 5):
            x, y = rng.uniform(0, W - 60), rng.uniform(0, H - 60)
            b = [x, y, x + rng.uniform(4, 60), y + rng.uniform(4, 60)]
        else:
            x, y = 8 * rng.randint(0, (W - 64) // 8), 8 * rng.randint(0, (H - 32) // 8)
            b = [x, y, x + 64, y + 32]
        out.append([float(v) for v in b])
    return np.asarray(out, np.float32).reshape(G, 4)


def candidates(N, gts, seed, inverted=False):
    rng = np.random.RandomState(seed)
    rows = [list(g) for g in gts[:16]]
    if len(gts):
        g = gts[0]
        rows.append([g[0], g[1], g[2], (g[1] + g[3]) / 2])          # half of gt 0: IoU exactly 0.5 for the 64 x 32 box
    rows += [[40, 40, 40, 90], [0, 0, 0, 0]]
    if inverted:
        rows += [[90, 30, 20, 60], [30, 90, 60, 20]]
    n = max(N - len(rows), 0)
    gx, gy = 8 * rng.randint(0, (W - 64) // 8, n), 8 * rng.randint(0, (H - 32) // 8, n)
    gw = np.where(rng.randint(0, 2, n) == 1, 64, 32)
    grid = np.stack([gx, gy, gx + gw, gy + 32], 1).astype(np.float32)
    fx, fy = rng.uniform(0, W - 80, n), rng.uniform(0, H - 80, n)
    frac = np.stack([fx, fy, fx + rng.uniform(2, 80, n), fy + rng.uniform(2, 80, n)], 1).astype(np.float32)
    rest = np.where((np.arange(n) % 2 == 0)[:, None], grid, frac)
    return np.concatenate([np.asarray(rows, np.float32).reshape(-1, 4), rest])[:N].copy()


def padded_gt(gt_list, Gmax):
    """[B, Gmax, 4] float32 (zeros past each image's count) and the int32 counts"""
    out = np.zeros((len(gt_list), Gmax, 4), np.float32)
    for b, g in enumerate(gt_list):
        out[b, :len(g)] = g
    return out, np.asarray([len(g) for g in gt_list], np.int32)
