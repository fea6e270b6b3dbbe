"""Cases of the run-length IoU tests (test_rle_iou.py on the CPU, test_rle_iou_gpu.py on the GPU): the intersection of two run-length
encoded masks restated as a two-pointer loop (the shape of pycocotools' rleIou inner loop, independent of the closed form in
panoswintransformerobjectdetection_amd/rle.py), the closed form with one planted defect each, a restatement of the two kernel passes of
csrc/pswin_rle_iou.hip in Python integers, and the builders of the batches both files use, so that the GPU cases can be rehearsed on the CPU."""
from bisect import bisect_left, bisect_right

import numpy as np
import torch

import _eval_cases
import _rle_cases as rc

M32 = 0xffffffff


# ---- the loop ----------------------------------------------------------------------------------------------------------------
def loop_area(c):
    return sum(int(v) for v in list(c)[1::2])


def loop_inter(a, b):
    """Walk both run lists at once: take the shorter remaining run, count it if both are foreground, move on in whichever list ran out.
    Runs of length 0 are stepped over one at a time, so they need no special case."""
    a, b = [int(v) for v in a], [int(v) for v in b]
    ia = ib = 0
    ca, cb = (a[0] if a else 0), (b[0] if b else 0)
    inter = 0
    while ia < len(a) and ib < len(b):
        if ca == 0:
            ia += 1
            ca = a[ia] if ia < len(a) else 0
            continue
        if cb == 0:
            ib += 1
            cb = b[ib] if ib < len(b) else 0
            continue
        c = min(ca, cb)
        if (ia & 1) and (ib & 1):
            inter += c
        ca -= c
        cb -= c
    return inter


def encode(mask):
    return rc.loop_encode(np.asarray(mask))


# ---- the closed form, and what it becomes with one planted defect -------------------------------------------------------------
# The rule as stated reads p[i - 1] only for odd i, so p[-1] itself is never read and "p[-1] taken as c[0]" alone changes nothing; its live
# neighbours are planted instead: the first foreground run started at p[-1] = 0 where p[0] = c[0] belongs ("first_start_is_p_minus_1"),
# and tables that are exclusive sums, every p[i] and f[i] standing one place late ("exclusive_tables").
# A LOWER bound in place of the upper one is no defect either: F is continuous and piecewise linear, the two bounds pick different pieces
# only at a breakpoint, where both pieces give the same value.  The tests assert that it changes nothing ("lower_bound" in HARMLESS).
DEFECTS = ("even_odd_swapped", "no_partial_run", "first_start_is_p_minus_1", "exclusive_tables", "area_from_even_counts", "row_major_position")
HARMLESS = ("lower_bound",)


def rule_tables(c, defect=None):
    p, f, sp, sf = [], [], 0, 0
    for i, v in enumerate(c):
        sp += int(v)
        if i & 1:
            sf += int(v)
        p.append(sp)
        f.append(sf)
    if defect == "exclusive_tables":
        p, f = [0] + p[:-1], [0] + f[:-1]
    return p, f


def rule_fg_below(p, f, x, defect=None):
    n = len(p)
    i = bisect_left(p, x) if defect == "lower_bound" else bisect_right(p, x)
    v = f[i - 1] if i else 0
    if (i & 1) and i < n and defect != "no_partial_run":
        v += x - (p[i - 1] if i else 0)
    return v


def rule_inter(cd, cg, defect=None):
    pd, _ = rule_tables(cd, defect)
    pg, fg = rule_tables(cg, defect)
    first = 1 if defect != "even_odd_swapped" else 2
    total = 0
    for i in range(first, len(cd), 2):
        before = pd[i - 1] if i else 0
        if i == 1 and defect == "first_start_is_p_minus_1":
            before = 0
        total += rule_fg_below(pg, fg, pd[i], defect) - rule_fg_below(pg, fg, before, defect)
    return total


def rule_area(c, defect=None):
    return sum(int(v) for v in list(c)[(0 if defect == "area_from_even_counts" else 1)::2])


def rule_of_masks(a, b, defect=None):
    """(inter, area of a) of two bitmaps by the closed form; "row_major_position" scans the first mask row by row"""
    a, b = np.asarray(a), np.asarray(b)
    ca = encode(a.reshape(-1).reshape(a.shape[1], a.shape[0]).T) if defect == "row_major_position" else encode(a)
    return rule_inter(ca, encode(b), defect), rule_area(ca, defect)


HAND = [                                                         # (counts a, counts b, inter): 10 positions each
    ([0, 3, 0, 2, 4, 0, 1], [2, 5, 3], 3),                       # zero-length runs inside: foreground 0 .. 4 against 2 .. 6
    ([0, 3, 0, 2, 4, 0, 1], [0, 3, 0, 2, 4, 0, 1], 5),
    ([10], [0, 10], 0),                                          # a mask of one run is empty
    ([0, 10], [0, 10], 10),
    ([0, 10], [3, 4, 3], 4),
    ([2, 3, 5], [5, 3, 2], 0),                                   # runs that touch end to start
    ([2, 3, 5], [4, 1, 0, 3, 2], 1),
    ([0, 1, 8, 1], [0, 1, 8, 1], 2),
    ([0, 0, 10], [0, 10], 0),
]


# ---- batches -----------------------------------------------------------------------------------------------------------------
def batch_definition(dm, dl, dc, gm, gl, gc):
    """(inter, areas) of evaluation.mask_inter_pairs' layout by the loop, from bitmaps [B, K, H, W] / [B, G, H, W] (numpy)"""
    B, K, G = dm.shape[0], dm.shape[1], gm.shape[1]
    inter, areas = np.full((B, K, G), -1, np.int32), np.zeros((B, K + G), np.int32)
    for b in range(B):
        nd, ng = max(0, min(int(dc[b]), K)), max(0, min(int(gc[b]), G))
        cd, cg = [encode(dm[b, k]) for k in range(nd)], [encode(gm[b, g]) for g in range(ng)]
        for k in range(nd):
            areas[b, k] = loop_area(cd[k])
        for g in range(ng):
            areas[b, K + g] = loop_area(cg[g])
        for k in range(nd):
            for g in range(ng):
                if dl[b, k] == gl[b, g]:
                    inter[b, k, g] = loop_inter(cd[k], cg[g])
    return inter, areas


def pattern_batch(H, W, shift=0):
    """All patterns as detections against all patterns as targets, B = 2: image 0 with every row counted, image 1 with the patterns in
    reverse, fewer detections and NO boxes.  Labels alternate over two classes (the targets' moved by `shift`), so every case has pairs
    of one class and pairs of two.  -> (det masks, det labels, det count, gt masks, gt labels, gt count) as tensors; K = G = the number
    of patterns"""
    pats = np.stack(list(rc.patterns(H, W).values()))
    N = pats.shape[0]
    dm = torch.from_numpy(np.stack([pats, pats[::-1].copy()]))
    gm = torch.from_numpy(np.stack([pats, pats]))
    dl = (torch.arange(N) & 1)[None, :].repeat(2, 1).long()
    gl = ((torch.arange(N) + shift) & 1)[None, :].repeat(2, 1).long()
    return dm, dl, torch.tensor([N, N - 5], dtype=torch.int32), gm, gl, torch.tensor([N, 0], dtype=torch.int32)


PATTERN_H, PATTERN_W = (1, 2, 64, 65, 130), (1, 17, 65)


def counts_with_runs(total, n_runs):
    """counts of n_runs >= 2 runs over `total` positions: [0, 1, 1, ..., 1, rest] -- a prefix of the scan that alternates from its first
    position on (what blanking the tail of a checkerboard leaves), or its complement's tail when n_runs is even"""
    c = [0] + [1] * (n_runs - 2)
    c.append(total - sum(c))
    assert len(c) == n_runs and c[-1] >= 1
    return c


def stage_masks(H, W, S):
    """Run counts around a staged table of S entries: S - 1, S, S + 1, 2 S + 5, the full checkerboard that starts with 1, and `ones`"""
    total = H * W
    full = encode(rc.patterns(H, W)["checker1"])
    out = [counts_with_runs(total, n) for n in (S - 1, S, S + 1, 2 * S + 5)] + [full, [0, total]]
    assert len(full) > 2 * S + 5
    return out


def lists_of(per_image_counts, H, W):
    """the input of RleMasks.from_lists for per-image lists of counts"""
    return [[dict(size=[H, W], counts=[int(v) for v in c]) for c in per] for per in per_image_counts]


def blob_masks(B, G, H, W, seed=0):
    """G filled discs and ellipses per image, uint8 [B, G, H, W], some empty, some over the border"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((B, G, H, W), np.uint8)
    for b in range(B):
        for g in range(G):
            if g % 11 == 10:
                continue
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            ry, rx = rng.uniform(2, H / 2), rng.uniform(2, W / 2)
            out[b, g] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0)
    return out


def scoring_case(seed=3, drop=0):
    """A batch with crowd flags and annotation areas, in every form the mask metric takes: name -> (Detections, PaddedTargets) on the CPU
    with runs on both sides, on one side, on both beside bitmaps, and bitmaps alone; all of the same masks.  drop: taken off every count"""
    from panoswintransformerobjectdetection_amd import rle
    from panoswintransformerobjectdetection_amd.detector import Detections, PaddedTargets
    dets, gts = _eval_cases.segm_case(2, 8, 5, 16, 24, seed=seed)
    dets.count, gts.count = (dets.count - drop).clamp(min=0), (gts.count - drop).clamp(min=0)
    for side in (dets, gts):                                                    # the containers' contract: zeros past the count
        for b, n in enumerate(side.count.tolist()):
            side.masks[b, n:] = 0
    dets.source = torch.zeros(2, 8, dtype=torch.int32)
    crowd = torch.zeros(2, 5, dtype=torch.bool)
    crowd[0, 1], crowd[1, 0] = True, True
    gt_area = torch.tensor([[10.0, 2000.0, 50.0, 120.0, 300.0], [64.0, 1.0, 5000.0, 90.0, 20.0]])
    de, ge = rle.encode_masks(dets.masks, dets.count), rle.encode_masks(gts.masks, gts.count)
    ge = rle.RleMasks.from_lists(ge.to_lists(), "cpu", K=5)                     # as annotations arrive
    D = lambda masks, enc: Detections(dets.boxes, dets.scores, dets.labels, dets.count, dets.source, masks, enc)
    T = lambda masks, enc: PaddedTargets(gts.boxes, gts.labels, gts.count, masks, enc)
    ways = dict(rle=(D(None, de), T(None, ge)), dets_rle=(D(None, de), T(gts.masks, None)), gts_rle=(D(dets.masks, None), T(None, ge)),
                both_given=(D(None, de), T(gts.masks, ge)), bitmaps=(D(dets.masks, None), T(gts.masks, None)))
    return ways, crowd, gt_area


# ---- the kernels' formulation, pass by pass (csrc/pswin_rle_iou.hip), in Python integers ----------------------------------------
def _whole(offsets, m, capacity):
    o0, o1 = int(offsets[m]), int(offsets[m + 1])
    return 0 <= o0 <= o1 <= capacity, o0, o1 - o0


def _ub(p, base, n, x):
    lo, hi = 0, n
    while lo < hi:
        mid = (lo + hi) >> 1
        if p[base + mid] <= x:
            lo = mid + 1
        else:
            hi = mid
    return lo


def _fg(p, f, base, n, x):
    i = _ub(p, base, n, x)
    v = f[base + i - 1] if i else 0
    if (i & 1) and i < n:
        v = (v + x - p[base + i - 1]) & M32
    return v


def _runs_against(pa, abase, m, pb, fb, bbase, nb, b0, b1):
    acc = 0
    for lane in range(64):
        for j in range(lane, m, 64):
            start, end = pa[abase + 2 * j], pa[abase + 2 * j + 1]
            if end <= b0 or start >= b1 or start == end:
                continue
            acc = (acc + _fg(pb, fb, bbase, nb, end) - _fg(pb, fb, bbase, nb, start)) & M32
    return acc


def emulate_kernel_passes(det, gt, B, K, G, threads=256, poison=None):
    """det / gt: dict(offsets, runs, capacity, labels [B][rows], count [B]) of Python lists.  Pass 1, a workgroup per mask: inclusive sums
    of the runs and of the odd-indexed runs in chunks of `threads` with a carry (uint32), written at the mask's own offsets; a mask inside
    its count that does not lie inside [0, capacity] is not read, has area 0 and sets overflow.  Pass 2, a workgroup per detection: per
    same-class box inside the counts, the lanes stride over the foreground runs of the mask with fewer runs and search the other's p twice.
    No entry at or past a capacity is touched: `poison` sits there (an int that would spoil any sum).
    -> (inter [B][K][G], areas [B][K + G], overflow)"""
    tables = []
    areas = [[0] * (K + G) for _ in range(B)]
    overflow = 0
    for side, rows, col in ((det, K, 0), (gt, G, K)):
        p, f = [poison] * side["capacity"], [poison] * side["capacity"]
        for b in range(B):
            live = max(0, min(int(side["count"][b]), rows))
            for r in range(live):
                ok, o0, n = _whole(side["offsets"], b * rows + r, side["capacity"])
                if not ok:
                    overflow = 1
                    continue
                cp = cf = 0
                for base in range(0, n, threads):
                    chunk = [int(v) for v in side["runs"][o0 + base:o0 + min(base + threads, n)]]
                    for t, c in enumerate(chunk):
                        cp = (cp + c) & M32
                        if (base + t) & 1:
                            cf = (cf + c) & M32
                        p[o0 + base + t], f[o0 + base + t] = cp, cf
                areas[b][col + r] = cf - (1 << 32) if cf >> 31 else cf
        tables.append((p, f))
    (pd, fd), (pg, fg) = tables
    inter = [[[-1] * G for _ in range(K)] for _ in range(B)]
    for b in range(B):
        nd_live, ng_live = max(0, min(int(det["count"][b]), K)), max(0, min(int(gt["count"][b]), G))
        for k in range(nd_live):
            d_ok, d0, nd = _whole(det["offsets"], b * K + k, det["capacity"])
            md = (nd >> 1) if d_ok else 0
            for g in range(ng_live):
                if det["labels"][b][k] != gt["labels"][b][g]:
                    continue
                acc = 0
                g_ok, g0, ng = _whole(gt["offsets"], b * G + g, gt["capacity"])
                if d_ok and g_ok:
                    mg = ng >> 1
                    if md and mg:
                        da, db, ga, gb = pd[d0], pd[d0 + 2 * md - 1], pg[g0], pg[g0 + 2 * mg - 1]
                        if da < gb and ga < db:
                            acc = _runs_against(pd, d0, md, pg, fg, g0, ng, ga, gb) if md <= mg else \
                                _runs_against(pg, g0, mg, pd, fd, d0, nd, da, db)
                inter[b][k][g] = acc - (1 << 32) if acc >> 31 else acc
    return inter, areas, overflow


def side_of(enc, labels, count):
    """an RleMasks on the CPU -> emulate_kernel_passes' dict"""
    return dict(offsets=enc.offsets.tolist(), runs=enc.runs[:enc.capacity].tolist(), capacity=enc.capacity, labels=labels.tolist(),
                count=count.tolist())
