"""tests/_roi_cases.py checked on the CPU before anything goes to a GPU: every property the exact RoIAlign and NMS cases claim (footprints of
16 and 17 cells, samples exactly on -1 and on H, grid widths around the number of lane groups, a bin count that is no multiple of 16,
power-of-two sample counts, the keep pattern of every NMS chain), that a float32 evaluation of the definition equals the float64 one bit
for bit on them, and that the same float32 evaluation with one defect at a time does not."""
import functools

import pytest
import torch

import _roi_cases as R
import _roi_ref

C_CPU = 4                        # channels are independent: the CPU checks run on the first four of the GPU tests' 512
pow2 = lambda n: n > 0 and n & (n - 1) == 0
config = pytest.mark.parametrize("cfg", R.CONFIGS, ids=R.config_id)


@functools.lru_cache(maxsize=None)
def _evaluated(cfg, dtype, defect=None, backward=True):
    P, sr, aligned = cfg
    c = R.exact_case(P, sr, aligned)
    feats = R.pyramid(C_CPU)
    out = R.roi_align(feats, R.STRIDES, c.rois, c.level, P, sr, aligned, dtype, defect)
    grads = R.adjoint(feats, R.STRIDES, c.rois, c.level, P, sr, aligned, R.dout(len(c.names), C_CPU, P), dtype, defect) if backward else None
    return out, grads


def _axis_samples(c):
    """per axis: [(coordinate, step, size of the axis)] of every sample of every RoI with a non-empty grid"""
    ys, xs = [], []
    for r, (box, lvl) in enumerate(zip(c.rois[:, 1:].tolist(), c.level.tolist())):
        g = R.geometry(box, lvl, c.P, c.sr, c.aligned)
        if g.gh * g.gw == 0:
            continue
        ys += [(p, g.bh / g.gh, g.H) for p in R.samples(g.y0, g.bh / g.gh, c.P * g.gh)]
        xs += [(p, g.bw / g.gw, g.W) for p in R.samples(g.x0, g.bw / g.gw, c.P * g.gw)]
    return ys, xs


@config
def test_exact_cases_are_what_they_claim(cfg):
    P, sr, aligned = cfg
    c = R.exact_case(P, sr, aligned)
    n = len(c.names)
    geo = [R.geometry(box, lvl, P, sr, aligned) for box, lvl in zip(c.rois[:, 1:].tolist(), c.level.tolist())]
    # the launch: a workgroup takes 16 bins, a wave 4
    assert (n * P * P) % 16 != 0 and (P != 7 or (n * P * P) % 4 != 0)
    # levels and images: all used, the level passed explicitly and out of range on both sides
    assert {R.clamp_level(l) for l in c.level.tolist()} == {0, 1, 2, 3} and {-1, R.N_LEVELS + 3} <= set(c.level.tolist())
    assert set(c.rois[:, 0].tolist()) == {0.0, 1.0}
    # dyadic geometry and power-of-two counts
    for g in geo:
        assert g.gh * g.gw == 0 or (pow2(g.gh) and pow2(g.gw)), (g.gh, g.gw)
    ys, xs = _axis_samples(c)
    assert all(float(p * 2 ** R.FRAC).is_integer() for p, _, _ in ys + xs)
    # validity edges, on both axes: a sample exactly on -1 and on the size (counted), one a grid step outside either (dropped), samples
    # in the clamp regions (-1, 0) and (size - 1, size)
    for axis in (ys, xs):
        at_lo = {s for p, s, _ in axis if p == -1.0}
        at_hi = {(s, size) for p, s, size in axis if p == size}
        assert at_lo and at_hi
        assert any(p == -1.0 - s for p, s, _ in axis if s in at_lo) and any(p == size + s for p, s, size in axis if (s, size) in at_hi)
        assert any(-1.0 < p < 0.0 for p, _, _ in axis) and any(size - 1 < p < size for p, _, size in axis)
    # degenerate boxes: an empty grid under sampling_ratio = 0, a zero or negative step under a fixed grid
    by = dict(zip(c.names, geo))
    if "zero_area" in by:
        z, inv = by["zero_area"], by["inverted"]
        if aligned:
            assert z.bw == z.bh == 0.0 and inv.bw < 0 and inv.bh < 0 and by["inverted_x"].bw < 0 < by["inverted_x"].bh
            assert (z.gh == z.gw == inv.gh == inv.gw == 0) if sr == 0 else (z.gh == inv.gw == sr)
        else:                                       # floored at one cell
            assert z.bw == z.bh == inv.bw == inv.bh == 1.0 / P
    else:
        assert not aligned and not pow2(P)          # a floored box has bins of 1 / P: dyadic for P = 2 only
    if "narrow" in by:
        box = c.rois[c.names.index("narrow"), 1:].tolist()
        assert (box[2] - box[0]) / R.STRIDES[0] < 1.0 and by["narrow"].bw == 1.0 / P and by["narrow"].bh == 2.0
        assert by["flat"].bh == 1.0 / P and by["flat"].bw == 1.5
    # footprints of the bins: both paths of the backward kernel, 16 and 17 independently per axis
    fps, thin, hits, big = {}, 0, {}, 0
    for r, ph, pw, g, y0, x0, sy, sx in R.bins(c):
        wy, wx = R.axis_weights(y0, sy, g.gh, g.H), R.axis_weights(x0, sx, g.gw, g.W)
        ny, nx = R.footprint(y0, sy, g.gh, g.H)[2], R.footprint(x0, sx, g.gw, g.W)[2]
        fps[(ny, nx)] = fps.get((ny, nx), 0) + 1
        if ny == 16 and nx == 16 and any(wy.get(k, 0.0) == 0.0 for k in range(min(wy) + 1, max(wy))):
            thin += 1
        if g.gh == g.gw == 16 and g.bh == g.bw == 16.0 and (ny, nx) == (17, 17):
            big += 1
        for cy, a in wy.items():
            for cx, b in wx.items():
                if a * b != 0.0:
                    hits.setdefault((int(c.rois[r, 0]), g.level, cy, cx), set()).add(r)
    wanted = {(16, 16), (16, 17), (17, 16), (17, 17)}
    print(R.config_id(cfg), f"R {n} bins {n * P * P}", "samples per bin (gh, gw):", sorted({(g.gh, g.gw) for g in geo}), "footprints (ny, nx): bins",
          {k: v for k, v in sorted(fps.items()) if max(k) >= 15}, f"16 x 16 with weightless interior rows: {thin}",
          f"most RoIs on one cell: {max(len(v) for v in hits.values())}")
    assert wanted <= set(fps), sorted(fps)
    assert any(max(k) <= 16 and min(k) >= 1 for k in fps) and any(max(k) > 16 for k in fps)
    assert max(len(v) for v in hits.values()) >= 4              # the atomics of different RoIs meet
    if sr == 2:
        assert thin >= 1
    if sr == 0:
        assert big >= 1
        widths = {g.gw for g in geo if g.gh * g.gw}
        assert {1, 2, 4, 8, 16} <= widths
        for dt, C in R.PAIRS:
            k = R.lane_groups(dt, C)
            assert k in widths and any(w > k for w in widths) and (k == 1 or any(w < k for w in widths)), (dt, C, k)
    assert {R.lane_groups(dt, C) for dt, C in R.PAIRS} == {1, 2, 4, 8}


@config
def test_float32_equals_float64_bit_for_bit(cfg):
    """forward and adjoint of the definition in float32 against float64 on the exact cases, and the room the sums have"""
    P, sr, aligned = cfg
    c = R.exact_case(P, sr, aligned)
    out64, g64 = _evaluated(cfg, torch.float64)
    out32, g32 = _evaluated(cfg, torch.float32)
    assert out32.dtype == torch.float32 and torch.equal(out32.double(), out64)
    for a, b in zip(g32, g64):
        assert a.dtype == torch.float32 and torch.equal(a.double(), b)
    # a term of the adjoint is a multiple of 2^-16 (weight 2^-8, 1 / count >= 2^-8): the sums are exact in any order below 2^8
    feats = R.pyramid(C_CPU)
    A = R.adjoint(feats, R.STRIDES, c.rois, c.level, P, sr, aligned, R.dout(len(c.names), C_CPU, P).abs())
    room = max(float(a.max()) for a in A)
    print(R.config_id(cfg), f"largest sum of |terms| of a gradient cell {room:.3f} (exact below 256), largest |out| {float(out64.abs().max()):.3f}")
    assert room < 2.0 ** (24 - 4 * R.FRAC) and all(float((a * 2.0 ** 16).frac().abs().max()) == 0.0 for a in g64)
    assert float(out64.abs().max()) > 0
    for name_ in ("outside_right", "outside_above") + (("zero_area", "inverted", "inverted_x") if sr == 0 and aligned else ()):
        assert float(out64[c.names.index(name_)].abs().max()) == 0.0, name_
    if sr > 0 and aligned:                          # every bin of a zero-area box reads the same point
        z = out64[c.names.index("zero_area")]
        assert float(z.abs().max()) > 0 and bool((z == z[:, :1, :1]).all())
    # bf16 cases: the inputs are bf16 numbers, and so is nothing else needed: the f32 result is exact, its bf16 rounding is the test's
    for t in feats + [R.dout(len(c.names), C_CPU, P)]:
        assert torch.equal(t.to(torch.bfloat16).float(), t)


def test_channels_and_images_differ():
    f = R.pyramid(R.CMAX)
    for t in f:
        assert not torch.equal(t[0], t[1]) and not torch.equal(t[:, 0], t[:, 64]) and float(t.abs().max()) == 8.0
    assert torch.equal(R.pyramid(64)[0], f[0][:, :64])


@pytest.mark.parametrize("defect", R.ROI_DEFECTS)
def test_every_roi_defect_is_seen(defect):
    """the float32 evaluation with one defect differs from the float64 definition on at least one exact case, forward"""
    order = sorted(R.CONFIGS, key=lambda c: (defect == "no_floor") == c[2])         # the floor exists only for aligned = False
    for cfg in order:
        want, _ = _evaluated(cfg, torch.float64)
        got, _ = _evaluated(cfg, torch.float32, defect, False)
        if not torch.equal(got.double(), want):
            c = R.exact_case(*cfg)
            rows = (got.double() != want).flatten(1).any(1).nonzero().flatten().tolist()
            print(defect, "seen on", R.config_id(cfg), [c.names[r] for r in rows][:6])
            return
    raise AssertionError(f"no exact case sees {defect}")


def test_mapped_case_takes_the_levels_the_extractor_assigns():
    c = R.mapped_case()
    assert torch.equal(_roi_ref.map_roi_levels(c.rois, R.N_LEVELS).int(), c.level) and set(c.level.tolist()) == {0, 1, 2, 3}
    feats = R.pyramid(C_CPU)
    a = R.roi_align(feats, R.STRIDES, c.rois, c.level, 7, 0, True, torch.float32)
    assert torch.equal(a.double(), R.roi_align(feats, R.STRIDES, c.rois, c.level, 7, 0, True))
    assert all(pow2(R.geometry(b, l, 7, 0, True).gw) for b, l in zip(c.rois[:, 1:].tolist(), c.level.tolist()))


def test_definition_is_the_plain_statement():
    """the float64 definition against tests/_roi_ref.py (float32, its own level mapping) on the mapped case"""
    c = R.mapped_case()
    feats = R.pyramid(C_CPU)
    want = R.roi_align(feats, R.STRIDES, c.rois, c.level, 7, 0, True)
    assert torch.equal(_roi_ref.roi_align_fpn(feats, R.STRIDES, c.rois, 7).double(), want)


def test_inexact_group_stays_inside_its_bounds():
    """3, 5, 6 and 7 samples per axis: the float32 evaluation against the float64 one, inside the two derived bounds"""
    c = R.inexact_case()
    grids = sorted({(g.gh, g.gw) for g in (R.geometry(b, l, 7, 0, True) for b, l in zip(c.rois[:, 1:].tolist(), c.level.tolist()))})
    print("inexact group: grids", grids, "n_max", c.n_max)
    assert {k for g in grids for k in g} == {3, 5, 6, 7} and c.n_max == 4         # a cell on the corner of four bins
    assert len({(int(b), int(l)) for b, l in zip(c.rois[:, 0], c.level)}) == len(c.names)           # one RoI per (image, level)
    feats, d = R.pyramid(C_CPU), R.dout(len(c.names), C_CPU, 7)
    arg = (feats, R.STRIDES, c.rois, c.level, 7, 0, True)
    want, got = R.roi_align(*arg), R.roi_align(*arg, torch.float32)
    assert not torch.equal(got.double(), want) and R.inside(got, want, R.FWD_REL * want.abs())
    A = R.adjoint(*arg, d.abs())
    for g, w, a in zip(R.adjoint(*arg, d, torch.float32), R.adjoint(*arg, d), A):
        assert R.inside(g, w, R.bwd_bound(c.n_max, a))
        assert not R.inside(g + 8 * R.bwd_bound(c.n_max, a).float().clamp(min=1e-6), w, R.bwd_bound(c.n_max, a))


# ---- NMS ---------------------------------------------------------------------------------------------------------------------------------
def _f32_verdicts(b, thr):
    """iou > thr with the kernel's f32 expressions"""
    area = (b[:, 2] - b[:, 0]).clamp(min=0) * (b[:, 3] - b[:, 1]).clamp(min=0)
    iw = (torch.minimum(b[:, None, 2], b[None, :, 2]) - torch.maximum(b[:, None, 0], b[None, :, 0])).clamp(min=0)
    ih = (torch.minimum(b[:, None, 3], b[None, :, 3]) - torch.maximum(b[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = iw * ih
    return inter / (area[:, None] + area[None] - inter).clamp(min=1e-6) > thr


@pytest.mark.parametrize("thr", R.THRESHOLDS)
def test_nms_chains_keep_what_they_claim(thr):
    i = torch.arange(R.NMS_N)
    for which in R.CHAINS:
        b = R.nms_case(which, thr)
        assert torch.equal(b, b.round()) and b.dtype == torch.float32
        assert torch.equal(_f32_verdicts(b, thr), R.iou(b, b) > thr)
    keep = R.nms_want("threshold", thr)
    m = R.iou(R.nms_case("threshold", thr), R.nms_case("threshold", thr))
    gone = set()
    for a, b in R.PAIR_ROWS["exact"]:
        assert float(m[a, b]) == thr and keep[a] and keep[b]
    for a, b in R.PAIR_ROWS["above"]:
        assert thr < float(m[a, b]) <= thr + 0.25 and keep[a] and not keep[b]
        gone.add(b)
    assert set((~keep).nonzero().flatten().tolist()) == gone
    assert sorted(b - a for a, b in R.PAIR_ROWS["exact"]) == [1, 16, 63, 64, 2047] and sorted(b - a for a, b in R.PAIR_ROWS["above"]) == [1, 16, 63, 64]
    assert (~R.nms_want("far", thr)).nonzero().flatten().tolist() == [R.NMS_N - 1]
    d = R.nms_want("degenerate", thr)
    assert (~d).nonzero().flatten().tolist() == [12, 61, 1500]
    if thr == 0.5:
        n = R.nms_case("neighbour")
        assert float(R.iou(n[:1], n[1:2])) == 3 / 5 and float(R.iou(n[:1], n[2:3])) == 1 / 3
        assert torch.equal(R.nms_want("neighbour", thr), i % 2 == 0)
        assert torch.equal(R.nms_want("stride64", thr), (i // 64) % 2 == 0)         # whole words alternate
        assert torch.equal(R.nms_want("stride16", thr), (i // 16) % 2 == 0)         # whole prefetch batches alternate
        for which, period in (("stride64", 64), ("stride16", 16)):
            a, b = (R.iou(R.nms_case(which), R.nms_case(which)) > thr).triu(1).nonzero(as_tuple=True)
            assert bool((b - a == period).all()) and len(a) == R.NMS_N - period      # the only links: to the same place one period on
    print(f"thr {thr}: kept", {w: int(R.nms_want(w, thr).sum()) for w in R.CHAINS})


@pytest.mark.parametrize("thr", R.THRESHOLDS)
def test_mixed_lists_hold_different_chains(thr):
    lists = R.mixed_lists(thr)
    assert tuple(len(b) for b in lists) == R.MIXED_COUNTS == (2048, 2047, 1985, 64, 63, 1, 0)
    want = [R.greedy(b, thr) for b in lists]
    for k in range(5):
        for j in range(k + 1, 5):
            n = min(len(lists[k]), len(lists[j]))
            assert not torch.equal(want[k][:n], want[j][:n])
    assert want[5].tolist() == [True] and want[6].shape == (0,)


@pytest.mark.parametrize("defect", R.NMS_DEFECTS)
def test_every_nms_defect_is_seen(defect):
    seen = [(w, thr) for thr in R.THRESHOLDS for w in R.CHAINS if not torch.equal(R.greedy(R.nms_case(w, thr), thr, defect), R.nms_want(w, thr))]
    print(defect, "seen on", seen)
    assert seen
