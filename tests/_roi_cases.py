"""Shared by tests/test_roi_cases.py (CPU) and tests/test_roi_exact_gpu.py: inputs on which csrc/pswin_roi.hip can be held to its definition
BIT FOR BIT, the float64 statement of RoIAlign and of the greedy NMS rule, and the same statements with one defect at a time.

RoIAlign: box corners are chosen so that x * spatial_scale - 0.5, the bin size and the sample step are dyadic and every sample coordinate is a
multiple of 1/16 cell; a bin has a power-of-two number of samples; features and dout are small integers.  Then a bilinear weight is a
multiple of 2^-8, 1 / count is a power of two, every product and every partial sum of the kernels is an exactly representable f32, and
the result does not depend on the order of the additions -- not in the forward's lane groups and not in the backward's atomics.  A second,
small group has 3, 5, 6 and 7 samples per axis: there only 1 / count is rounded, and the bounds count those roundings.

NMS: integer boxes and dyadic thresholds; iou > thr is then the same verdict in f32 and in float64 (x -> fl(x) is monotone and thr is
representable), and the keep vectors must be equal.

A RoI is specified in cells of its level: the origin (x0, y0) is the box corner AFTER x * scale - offset, (bw, bh) the size of a bin."""
import collections
import functools
import math
import types

import torch
import torch.nn.functional as F

STRIDES = (4, 8, 16, 32)
IMG_H, IMG_W, B, CMAX = 128, 256, 2, 512
SIZES = tuple((IMG_H // s, IMG_W // s) for s in STRIDES)        # (H, W) of the levels: 32 x 64 .. 4 x 8
N_LEVELS = len(STRIDES)
FRAC = 4                         # sample coordinates of the exact cases are multiples of 2^-FRAC
PAIRS = ((torch.float32, 64), (torch.float32, 128), (torch.float32, 256),
         (torch.bfloat16, 64), (torch.bfloat16, 128), (torch.bfloat16, 256), (torch.bfloat16, 512))
UNSUPPORTED = ((torch.float32, 512), (torch.bfloat16, 192), (torch.bfloat16, 96), (torch.float32, 576))
CONFIGS = tuple((P, sr, aligned) for P in (7, 14, 2) for sr in (0, 2, 4) for aligned in (True, False))      # (P, sampling_ratio, aligned)

Roi = collections.namedtuple("Roi", "name b level x0 y0 bw bh box", defaults=(None,))


def name(dtype):
    return "bf16" if dtype == torch.bfloat16 else "f32"


def config_id(c):
    return f"P{c[0]}-sr{c[1]}-{'aligned' if c[2] else 'unaligned'}"


def lane_groups(dtype, C):
    """roi_align_fwd_kernel: 64 / (C / VEC) lane groups of a wave take different samples of a bin's row"""
    return 64 // (C // (8 if dtype == torch.bfloat16 else 4))


def clamp_level(l, n=N_LEVELS):
    return min(max(int(l), 0), n - 1)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pyramid():
    g = torch.Generator().manual_seed(20)
    return tuple(torch.randint(-8, 9, (B, CMAX, H, W), generator=g).float() for H, W in SIZES)


def pyramid(C):
    """integer features in [-8, 8] (bf16-exact), NCHW f32, the first C channels of one fixed CMAX-channel pyramid: the two images and
    all channels hold different values"""
    return [f[:, :C] for f in _pyramid()]


@functools.lru_cache(maxsize=None)
def _dout(R, P):
    g = torch.Generator().manual_seed(1000 * P + R)
    return torch.randint(-4, 5, (R, CMAX, P, P), generator=g).float()


def dout(R, C, P):
    """integer upstream gradients in [-4, 4], [R, C, P, P]"""
    return _dout(R, P)[:, :C]


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
ROI_DEFECTS = ("le_at_minus1", "ge_at_size", "no_clamp_at_size", "grid_floor", "no_half", "no_floor", "other_image", "level_unclamped",
               "count_axis")


def _axis(p, size, defect):
    """sample coordinates p [n] along an axis of `size` cells -> (valid, lo, hi, weight of hi, weight of lo).  A sample outside
    [-1, size] does not count; one inside is clamped to [0, size - 1] and read from the two cells around it."""
    low = (p <= -1.0) if defect == "le_at_minus1" else (p < -1.0)
    high = (p >= size) if defect == "ge_at_size" else (p > size)
    valid = ~(low | high)
    p = p.clamp(min=0)
    lo = p.floor().long()
    if defect == "no_clamp_at_size":             # rows / columns past the map read as 0 (the maps are padded with two of them)
        lo = lo.clamp(max=size)                  # (a sample that counts has lo <= size; the others are masked)
        return valid, lo, lo + 1, p - lo, 1 - (p - lo)
    top = lo >= size - 1
    lo = torch.where(top, torch.full_like(lo, size - 1), lo)
    hi = torch.where(top, lo, lo + 1)
    p = torch.where(top, lo.to(p.dtype), p)
    l = p - lo
    return valid, lo, hi, l, 1 - l


def roi_align(feats, strides, rois5, roi_level, P, sampling_ratio=0, aligned=True, dtype=torch.float64, defect=None):
    """RoIAlign over a pyramid as the header of csrc/pswin_roi.hip states it, evaluated in `dtype` (float64: the definition; float32: what
    the kernels compute, in another order of additions), differentiable in feats.  feats: NCHW maps; rois5 [R, 5] = (image, x1, y1, x2,
    y2) in image pixels; roi_level [R] is clamped to the pyramid; aligned = False floors the box's width and height at one cell.
    -> [R, C, P, P] in `dtype`.  defect: one of ROI_DEFECTS, for the sensitivity test."""
    n = len(feats)
    T = lambda v: torch.tensor(float(v), dtype=dtype, device=rois5.device)
    outs = []
    for r in range(rois5.shape[0]):
        l, b = int(roi_level[r]), int(rois5[r, 0])
        C = feats[0].shape[1]
        if defect == "level_unclamped" and not 0 <= l < n:          # a level that is no map of the pyramid: nothing to read
            outs.append(torch.zeros(C, P, P, dtype=dtype, device=rois5.device))
            continue
        l = clamp_level(l, n)
        if defect == "other_image":
            b = feats[l].shape[0] - 1 - b
        f = F.pad(feats[l][b].to(dtype), (0, 2, 0, 2))              # two rows and columns of zeros that only a defect reads
        H, W = feats[l].shape[2:]
        s, off = T(1.0 / strides[l]), T(0.5 if aligned and defect != "no_half" else 0.0)
        x1, y1, x2, y2 = [rois5[r, k].to(dtype) * s - off for k in range(1, 5)]
        rw, rh = x2 - x1, y2 - y1
        if not aligned and defect != "no_floor":
            rw, rh = torch.maximum(rw, T(1)), torch.maximum(rh, T(1))
        bh, bw = rh / P, rw / P
        rnd = math.floor if defect == "grid_floor" else math.ceil
        gh = sampling_ratio if sampling_ratio > 0 else max(int(rnd(float(bh))), 0)
        gw = sampling_ratio if sampling_ratio > 0 else max(int(rnd(float(bw))), 0)
        if gh * gw == 0:
            outs.append(f.new_zeros(C, P, P) + 0 * f.sum())         # (keeps every map in the graph)
            continue
        inv = T(1) / T(gh * gh if defect == "count_axis" else gh * gw)
        iy, ix = torch.arange(P * gh, device=f.device), torch.arange(P * gw, device=f.device)
        ys = y1 + (iy // gh).to(dtype) * bh + ((iy % gh).to(dtype) + 0.5) * (bh / gh)
        xs = x1 + (ix // gw).to(dtype) * bw + ((ix % gw).to(dtype) + 0.5) * (bw / gw)
        vy, yl, yh, ly, hy = _axis(ys, H, defect)
        vx, xl, xh, lx, hx = _axis(xs, W, defect)
        v = (f[:, yl][:, :, xl] * (hy[:, None] * hx[None]) + f[:, yl][:, :, xh] * (hy[:, None] * lx[None]) +
             f[:, yh][:, :, xl] * (ly[:, None] * hx[None]) + f[:, yh][:, :, xh] * (ly[:, None] * lx[None]))
        v = v * (vy[:, None] & vx[None]).to(dtype)
        outs.append(v.view(C, P, gh, P, gw).sum((2, 4)) * inv)
    return torch.stack(outs)


def adjoint(feats, strides, rois5, roi_level, P, sampling_ratio, aligned, dout, dtype=torch.float64, defect=None):
    """the gradients of sum(roi_align(...) * dout) with respect to the maps, by autograd one RoI at a time -> list of NCHW in `dtype`"""
    leaves = [f.detach().to(dtype).requires_grad_(True) for f in feats]
    for r in range(rois5.shape[0]):
        out = roi_align(leaves, strides, rois5[r:r + 1], roi_level[r:r + 1], P, sampling_ratio, aligned, dtype, defect)
        (out * dout[r:r + 1].to(dtype)).sum().backward()
    return [torch.zeros_like(f) if f.grad is None else f.grad for f in leaves]


# ---- the geometry of a RoI in plain Python (doubles; exact on dyadic operands) -------------------------------------------------------------
def geometry(box, level, P, sampling_ratio, aligned):
    """(x1, y1, x2, y2) in pixels on (clamped) level -> the grid of the RoI: H, W, origin x0, y0, bin bw, bh, samples per bin gw, gh"""
    l = clamp_level(level)
    s, off = 1.0 / STRIDES[l], 0.5 if aligned else 0.0
    x0, y0, x1, y1 = [float(v) * s - off for v in box]
    rw, rh = x1 - x0, y1 - y0
    if not aligned:
        rw, rh = max(rw, 1.0), max(rh, 1.0)
    bw, bh = rw / P, rh / P
    gw = sampling_ratio if sampling_ratio > 0 else max(math.ceil(bw), 0)
    gh = sampling_ratio if sampling_ratio > 0 else max(math.ceil(bh), 0)
    return types.SimpleNamespace(level=l, H=SIZES[l][0], W=SIZES[l][1], x0=x0, y0=y0, bw=bw, bh=bh, gw=gw, gh=gh)


def samples(start, step, count):
    return [start + (i + 0.5) * step for i in range(count)]


def axis_weights(start, step, count, size):
    """{cell: summed weight} of a bin's `count` samples start + (i + 0.5) step along an axis of `size` cells, from the definition; a
    touched cell of weight 0 (the upper neighbour of a sample on an integer coordinate) is listed with 0.0"""
    w = {}
    for p in samples(start, step, count):
        if p < -1.0 or p > size:
            continue
        p = max(p, 0.0)
        lo = int(math.floor(p))
        if lo >= size - 1:
            lo = hi = size - 1
            p = float(lo)
        else:
            hi = lo + 1
        w[lo] = w.get(lo, 0.0) + (1.0 - (p - lo))
        w[hi] = w.get(hi, 0.0) + (p - lo)
    return w


def footprint(start, step, count, size):
    """(first touched cell, last touched cell, number of cells between them inclusive) of a bin along one axis; (0, -1, 0) if no sample
    counts.  The backward kernel takes its one-atomic-per-cell path when both axes have at most 16."""
    w = axis_weights(start, step, count, size)
    return (min(w), max(w), max(w) - min(w) + 1) if w else (0, -1, 0)


def bins(case):
    """every bin of a case: (roi index, ph, pw, geometry, y start, x start, y step, x step)"""
    for r, (box, lvl) in enumerate(zip(case.rois[:, 1:].tolist(), case.level.tolist())):
        g = geometry(box, lvl, case.P, case.sr, case.aligned)
        for ph in range(case.P):
            for pw in range(case.P):
                yield (r, ph, pw, g, g.y0 + ph * g.bh, g.x0 + pw * g.bw, g.bh / g.gh if g.gh else 0.0, g.bw / g.gw if g.gw else 0.0)


# ---- the exact RoI cases -----------------------------------------------------------------------------------------------------------------
def _grid(b, sr):
    return sr if sr > 0 else max(math.ceil(b), 0)


def _origin(target, j, b, sr):
    """the origin that puts sample j (counted along the whole RoI) of bins of b cells exactly on `target`"""
    return target - (j + 0.5) * b / _grid(b, sr)


def _box(q, P, aligned):
    if q.box is not None:
        return q.box
    s, off = STRIDES[clamp_level(q.level)], 0.5 if aligned else 0.0
    return ((q.x0 + off) * s, (q.y0 + off) * s, (q.x0 + off + P * q.bw) * s, (q.y0 + off + P * q.bh) * s)


def _finish(specs, P, sr, aligned, pad_to, pad_level=2):
    k = 0
    while pad_to and len(specs) % 4 != pad_to:          # R = 1 or 3 (mod 4): R P P is no multiple of 16 for P = 7, 14 and 2
        specs.append(Roi(f"pad{k}", k % 2, pad_level, 1.0 + 2 * k, 0.5 + k, 1.0, 1.0))
        k += 1
    rois = torch.tensor([[float(q.b), *_box(q, P, aligned)] for q in specs], dtype=torch.float32)
    assert torch.equal(rois.double(), torch.tensor([[float(q.b), *_box(q, P, aligned)] for q in specs], dtype=torch.float64))
    level = torch.tensor([q.level for q in specs], dtype=torch.int32)
    return types.SimpleNamespace(rois=rois, level=level, names=[q.name for q in specs], P=P, sr=sr, aligned=aligned, specs=specs)


# bin sizes whose footprint is 16 / 17 cells along an axis, with the origin that makes it so: sampling_ratio -> {cells: (bin, origin)}
#   2: samples half a bin apart, on the same fraction: bin / 2 + 2 cells.  28 with an integer origin puts them on INTEGER coordinates 14
#      apart: of the 16 cells only two carry weight (the wr == 0 / w == 0 skips of the one-atomic-per-cell path)
#   4: 18 from 0.25: samples 2.5, 7, 11.5, 16 -> cells 2 .. 17;  20: samples 3.5 .. 18.5 -> cells 3 .. 19
#   0: a bin of 16 cells has a 16-sample grid one cell apart: 17 cells, the large-box regime of the detector's step; from -1 the first
#      sample (-0.5) is clamped onto cell 0: 16 cells
FOOTPRINTS = {2: {16: (28.0, 1.0), 17: (30.0, 0.5)}, 4: {16: (18.0, 0.25), 17: (20.0, 1.0)}, 0: {16: (16.0, -1.0), 17: (16.0, 1.0)}}


@functools.lru_cache(maxsize=None)
def exact_case(P, sr, aligned, skip_level=None):
    """The exact RoIs of one (P, sampling_ratio, aligned): rois [R, 5] f32, level int32 [R] as passed to the operator (-1 and
    N_LEVELS + 3 among them), names.  skip_level: without the RoIs of that level (its gradient map must stay 0)."""
    H0, W0 = SIZES[0]
    H3, W3 = SIZES[3]
    S = []
    # validity edges: the first sample of bin 1 exactly on -1 (the samples of bin 0 lie a step or more outside), the first sample of the
    # last bin exactly on H / W (the next one a step outside); 1.5-cell bins put samples into (-1, 0) and (H - 1, H)
    for i, b in enumerate((2.0, 1.5)):
        g = _grid(b, sr)
        lo = _origin(-1.0, g, b, sr)
        S.append(Roi(f"edge_lo_{b}", i, -1 if i else 0, lo, lo, b, b))
        S.append(Roi(f"edge_hi_{b}", 1 - i, 0, _origin(W0, g * (P - 1), b, sr), _origin(H0, g * (P - 1), b, sr), b, b))
    S.append(Roi("edge_lo_y_hi_x", 0, 0, _origin(W0, _grid(1.0, sr) * (P - 1), 1.0, sr), _origin(-1.0, _grid(1.0, sr), 1.0, sr), 1.0, 1.0))
    S.append(Roi("edge_hi_y_lo_x", 1, 0, _origin(-1.0, _grid(0.5, sr), 0.5, sr), _origin(H0, _grid(2.0, sr) * (P - 1), 2.0, sr), 0.5, 2.0))
    S.append(Roi("edge_coarsest", 1, N_LEVELS + 3, _origin(-1.0, _grid(1.0, sr), 1.0, sr), _origin(H3, _grid(1.0, sr), 1.0, sr), 1.0, 1.0))
    S.append(Roi("outside_right", 0, 1, SIZES[1][1] + 1.0, 2.0, 1.0, 1.0))
    S.append(Roi("outside_above", 1, 2, 3.0, -1.5 - P * 1.5, 2.0, 1.5))
    if aligned or P & (P - 1) == 0:        # aligned = False floors a degenerate box at one cell: a bin of 1 / P
        S.append(Roi("zero_area", 0, 1, 5.25, 3.5, 0.0, 0.0))
        S.append(Roi("inverted", 1, 1, 12.25, 9.5, -1.5, -1.0))
        S.append(Roi("inverted_x", 0, 2, 9.0, 1.25, -2.0, 1.5))
    if not aligned and P & (P - 1) == 0:   # narrower / flatter than one cell: only the floor makes the bins 1 / P
        s = STRIDES[0]
        S.append(Roi("narrow", 1, 0, None, None, None, None, (10.5 * s, 4.0 * s, 11.0 * s, (4.0 + 2.0 * P) * s)))
        S.append(Roi("flat", 0, 0, None, None, None, None, (20.0 * s, 7.25 * s, (20.0 + 1.5 * P) * s, 7.5 * s)))
    # both paths of the backward kernel: footprints of 16 and 17 cells, independently per axis, on one image and level (they overlap)
    fp = FOOTPRINTS[sr]
    for ny in (16, 17):
        for nx in (16, 17):
            S.append(Roi(f"footprint_{ny}x{nx}", 0, 0, fp[nx][1], fp[ny][1], fp[nx][0], fp[ny][0]))
    # a pile of RoIs on the same cells of image 1, level 1
    for k, (x0, y0, bw, bh) in enumerate(((6.125, 3.25, 1.0, 1.5), (6.5, 3.5, 1.5, 1.0), (7.0, 4.125, 2.0, 0.5), (5.875, 2.75, 0.5, 2.0),
                                          (6.25, 3.0, 1.0, 1.0))):
        S.append(Roi(f"pile{k}", 1, 1, x0, y0, bw, bh))
    # adaptive grid widths 1, 2, 4, 8, 16 (below, at and above the number of lane groups of every (dtype, C)), gh != gw, all levels
    for k, (bw, bh, lvl, x0, y0) in enumerate(((0.5, 2.0, 0, 30.125, 11.5), (1.0, 4.0, 1, -2.25, 1.0), (1.5, 0.5, 2, 4.75, 5.125),
                                               (2.0, 1.0, 3, -3.5, -1.25), (3.5, 1.5, 0, 41.0, 24.625), (4.0, 2.0, 1, 12.5, -5.0),
                                               (8.0, 1.0, 2, -9.0, 2.375), (8.0, 3.5, 0, 17.25, 3.0), (16.0, 2.0, 0, -20.0, 20.5),
                                               (16.0, 4.0, 1, 3.0, 0.875), (2.0, 8.0, 3, 1.5, -6.0), (4.0, 16.0, 2, 2.125, -30.0))):
        S.append(Roi(f"grid{k}", k % 2, lvl, x0, y0, bw, bh))
    if skip_level is not None:
        S = [q for q in S if clamp_level(q.level) != skip_level]
    return _finish(S, P, sr, aligned, 1 if len(S) % 4 != 3 else 3, 1 if skip_level == 2 else 2)


@functools.lru_cache(maxsize=None)
def mapped_case():
    """P = 7, adaptive grids, two RoIs per level whose size makes SingleRoIExtractor.map_roi_levels (finest_scale 56) choose that level:
    the operator is called WITHOUT roi_level.  level holds what the mapping must give."""
    S = []
    for l in range(N_LEVELS):
        S.append(Roi(f"mapped{l}a", l % 2, l, 1.25 - l, 0.5 - l, 3.5, 3.5))           # sqrt(area) = 98 * 2^l pixels
        S.append(Roi(f"mapped{l}b", 1 - l % 2, l, -0.75, 0.125, 2.0, 4.0))              # 79.2 * 2^l
    return _finish(S, 7, 0, True, 0)


# ---- 3, 5, 6 and 7 samples per axis: 1 / count is rounded ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inexact_case():
    """P = 7, adaptive grids, integer bins of 3, 5, 6 and 7 cells (a sample step of exactly 1), one RoI per (image, level): the sums
    are still exact, 1 / count and the product with it are rounded.  n_max: the most contributions (non-zero weights of different bins)
    one cell of a gradient map receives."""
    S = []
    for k, (bw, bh) in enumerate(((3.0, 5.0), (5.0, 3.0), (6.0, 7.0), (7.0, 6.0), (3.0, 3.0), (5.0, 7.0), (6.0, 5.0), (7.0, 3.0))):
        # (an integer origin puts the samples on half-integers: the cell on a bin boundary takes weight from both bins, on both axes 4)
        S.append(Roi(f"inexact{k}", k % 2, k // 2, (-2.0, 1.5, -0.5, 3.0)[k % 4], (1.0, -3.0, 2.0, -1.0)[k % 4], bw, bh))
    c = _finish(S, 7, 0, True, 0)
    hits = collections.Counter()
    for r, ph, pw, g, ys, xs, sy, sx in bins(c):
        wy, wx = axis_weights(ys, sy, g.gh, g.H), axis_weights(xs, sx, g.gw, g.W)
        for cy, a in wy.items():
            for cx, b in wx.items():
                if a * b != 0.0:
                    hits[(int(c.rois[r, 0]), g.level, cy, cx)] += 1
    c.n_max = max(hits.values())
    return c


FWD_REL = 1.5 * 2.0 ** -23       # |got - want| <= FWD_REL |want|: one rounding of 1 / count, one of the product with the exact sum


def bwd_bound(n_max, A):
    """|got - want| <= (3 + n_max) 2^-24 A, A the float64 adjoint of |dout|: dout / count is two roundings (1 / count, the product), the
    weight's product one, and each of the at most n_max additions to a cell loses at most 2^-24 of the sum of the magnitudes"""
    return (3 + n_max) * 2.0 ** -24 * A


def inside(got, want, tol):
    """got (f32 or bf16) against float64 want +- tol: a bf16 result is the rounding of an f32 inside the bound, and rounding is monotone"""
    want, tol = want.double(), tol.double() if torch.is_tensor(tol) else tol
    if got.dtype == torch.bfloat16:
        lo, hi = (want - tol).to(torch.bfloat16).double(), (want + tol).to(torch.bfloat16).double()
    else:
        lo, hi = want - tol, want + tol
    g = got.double()
    return bool(((g >= lo) & (g <= hi)).all())


# ---- greedy NMS --------------------------------------------------------------------------------------------------------------------------
NMS_DEFECTS = ("ge", "no_carry", "removed_suppresses")
NMS_N = 2048
THRESHOLDS = (0.5, 0.25)
MIXED_COUNTS = (2048, 2047, 1985, 64, 63, 1, 0)
PAIR_ROWS = {"exact": ((63, 64), (100, 116), (128, 191), (200, 264), (0, 2047)),          # row distances 1, 16, 63, 64, 2047
             "above": ((15, 16), (300, 316), (320, 383), (400, 464))}


def iou(a, b):
    """float64 IoU matrix as the kernel defines it: widths and heights clamped at 0, the union floored at 1e-6"""
    a, b = a.double(), b.double()
    area = lambda t: (t[:, 2] - t[:, 0]).clamp(min=0) * (t[:, 3] - t[:, 1]).clamp(min=0)
    iw = (torch.minimum(a[:, None, 2], b[None, :, 2]) - torch.maximum(a[:, None, 0], b[None, :, 0])).clamp(min=0)
    ih = (torch.minimum(a[:, None, 3], b[None, :, 3]) - torch.maximum(a[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = iw * ih
    return inter / (area(a)[:, None] + area(b)[None] - inter).clamp(min=1e-6)


def greedy(boxes, thr, defect=None):
    """keep[i] = no KEPT j < i with iou(i, j) > thr, row by row -> bool [n].  defect: one of NMS_DEFECTS."""
    n = boxes.shape[0]
    keep = torch.ones(n, dtype=torch.bool)
    if n == 0:
        return keep
    m = iou(boxes, boxes)
    hit = ((m >= thr) if defect == "ge" else (m > thr)).triu(1)
    if defect == "no_carry":                     # a row's mask reaches only its own 64-row word
        w = torch.arange(n) // 64
        hit &= w[:, None] == w[None]
    if defect == "removed_suppresses":
        return ~hit.any(0)
    for i in range(n):
        if keep[i]:
            keep &= ~hit[i]
    return keep


def _fillers(n):
    """n boxes that touch nothing: every row kept unless a planted box says otherwise"""
    i = torch.arange(n, dtype=torch.float32)
    return torch.stack([8 * i, torch.full_like(i, 100.0), 8 * i + 4, torch.full_like(i, 101.0)], 1)


def _chain(n, period, spacing):
    i = torch.arange(n)
    x = (spacing * (i % period) + i // period).float()
    return torch.stack([x, torch.zeros(n), x + 4, torch.ones(n)], 1)


@functools.lru_cache(maxsize=None)
def nms_case(which, thr=0.5):
    """NMS_N integer boxes in score order (f32 [n, 4]):
      threshold   fillers, and pairs (a, b) of boxes [x, 0, x + 4, 1] and [x, 0, x + w, 1] at the rows of PAIR_ROWS: w = 4 thr (IoU exactly
                  thr: b is kept) or 4 thr + 1 (one integer step above: b is removed)
      neighbour   box i = [i, 0, i + 4, 1]: IoU 3/5 with the next row, 1/3 with the one after
      stride64    x = 100 (i % 64) + i // 64: a row overlaps only the same bit of the neighbouring words
      stride16    x = 200 (i % 16) + i // 16: only the same row of the neighbouring 16-row batches
      far         fillers; row 2047 lies in row 0's box (IoU 3/4)
      degenerate  fillers; duplicated zero-area boxes (IoU 0: all kept), an inverted box, duplicated proper boxes (IoU 1)
      single      fillers (for the list of one box)"""
    b = _fillers(NMS_N)
    if which == "threshold":
        k = 0
        for kind, w in (("exact", 4 * thr), ("above", 4 * thr + 1)):
            for i, j in PAIR_ROWS[kind]:
                x = 16.0 * k
                b[i], b[j] = torch.tensor([x, 0., x + 4, 1.]), torch.tensor([x, 0., x + w, 1.])
                k += 1
    elif which == "neighbour":
        b = _chain(NMS_N, 1, 0)
    elif which == "stride64":
        b = _chain(NMS_N, 64, 100)
    elif which == "stride16":
        b = _chain(NMS_N, 16, 200)
    elif which == "far":
        b[0], b[NMS_N - 1] = torch.tensor([0., 0., 4., 1.]), torch.tensor([0., 0., 3., 1.])
    elif which == "degenerate":
        for i in (3, 4, 20, 62, 64, 700):
            b[i] = torch.tensor([5., 5., 5., 9.])                  # zero width, six times
        b[7] = torch.tensor([9., 2., 9., 2.])                       # a point, twice
        b[8] = b[7]
        b[10] = torch.tensor([30., 10., 26., 4.])                   # inverted
        b[11] = torch.tensor([24., 2., 32., 12.])                   # a proper box around it: IoU 0 with it
        b[12] = b[11]                                               # and its duplicates: IoU 1
        b[61] = b[11]
        b[1500] = b[11]
    else:
        assert which == "single"
    return b


CHAINS = ("threshold", "neighbour", "stride64", "stride16", "far", "degenerate")
MIXED = ("threshold", "neighbour", "stride64", "stride16", "degenerate", "single")          # a different chain in every non-empty list


def mixed_lists(thr):
    """lists of MIXED_COUNTS boxes for one launch: the leading rows of a different chain each"""
    return [nms_case(w, thr)[:n] for w, n in zip(MIXED + ("single",), MIXED_COUNTS)]


@functools.lru_cache(maxsize=None)
def nms_want(which, thr, n=NMS_N):
    return greedy(nms_case(which, thr)[:n], thr)
