"""Detector inference behind the heads on the MI355X (csrc/pswin_detect.hip through ops.multiclass_nms_batch / ops.paste_masks and
MiniMaskRCNN.heads_predict) against the definitions of detector.py evaluated on the CPU.

SELECTION is compared exactly (which (proposal, class) pairs, in which order).  That is only meaningful for inputs on which float32 and
float64 arithmetic cannot disagree about an order or a threshold, so every test first asserts CONDITIONS on its inputs, on the CPU in
float64 (they are conditions on the inputs, not tolerances on the result):
  * no score within 1e-6 of score_thr;
  * candidate scores pairwise distinct, except within groups built from bit-equal logit rows.  "Distinct" in float64 is not enough for
    two float32 evaluations to agree on an order: F.softmax in float32 is a few ulp off (below: <= 2.7e-7 absolute), the kernel
    rounds the float64 value once.  The condition asserted is therefore a gap of at least SCORE_GAP = 1e-6 (8 float32 ulp of 1.0)
    between any two unequal candidate scores of an image -- stronger than pairwise distinct;
  * no same-class candidate pair with an IoU within 1e-4 of iou_thr, except exact duplicates;
  * the K-th and (K+1)-th survivors' scores differ (by SCORE_GAP, as above).

VALUES (boxes, scores) have no prescribed tolerance: with the float64 definition as the truth, the kernel's error may be at most 4 x the
float32 CPU definition's own error on the same inputs, plus one float32 ulp of the image size for boxes and of 1.0 for scores.
NOT YET MEASURED on an MI355X (no GPU machine could be had when the test was written; every run prints the figures).  A restatement of the
kernels' arithmetic on the CPU (softmax and the delta decoder in double, rounded once) gives, kernel / float32 CPU definition:
    boxes  R = 1000, 512 x 1024:  3.0e-05 / 5.2e-05 px      R = 70, 128 x 256:  7.4e-06 / 1.4e-05 px      with a scale factor: 1.4e-05 / 2.1e-05
    scores                      :  3.0e-08 / 2.7e-07

MASKS are compared outside the near-threshold set: pixels whose float reference value (the CPU definition's float image) lies within 1e-4
of mask_thr_binary are left out, at most 0.1 % of the pixels may be; all others must be equal."""
import functools
import os

import numpy as np
import pytest
import torch

from _util import TINY

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect_post.npz")
STDS = (0.1, 0.1, 0.2, 0.2)
SCORE_THR, IOU_THR, SCORE_GAP = 0.05, 0.5, 1e-6
ULP_ONE = float(np.spacing(np.float32(1.0)))


def _bf16_exact(t):
    return t.to(torch.bfloat16).float()


# ---- conditions -----------------------------------------------------------------------------------------------------------------------------
def check_conditions(rois, roi_count, cls, deltas, img_hw, scale, K):
    """the conditions of the module docstring for a batch, in float64: None, or the name of the first one violated"""
    from panoswintransformerobjectdetection_amd import detector as det
    B, R, C = cls.shape[0], cls.shape[1], cls.shape[2] - 1
    for b, n in enumerate(roi_count.tolist()):
        if n == 0:
            continue
        lg = cls[b, :n].double()
        sc = torch.softmax(lg, -1)[:, :C]
        if bool(((sc - SCORE_THR).abs() <= 1e-6).any()):
            return f"image {b}: a score within 1e-6 of score_thr"
        bx = det.decode_deltas_per_class(rois[b, :n].double(), deltas[b, :n].double(), STDS, img_hw).reshape(n, C, 4)
        if scale is not None:
            bx = bx / scale[b].double()
        rr, cc = torch.nonzero(sc > SCORE_THR, as_tuple=True)
        s = sc[rr, cc]
        order = torch.argsort(s)
        s, rr, cc = s[order], rr[order], cc[order]
        gap = s[1:] - s[:-1]
        same_rows = (lg[rr[1:]] == lg[rr[:-1]]).all(1) & (cc[1:] == cc[:-1])
        if bool(((gap < SCORE_GAP) & ~((gap == 0) & same_rows)).any()):
            return f"image {b}: two candidate scores closer than {SCORE_GAP} that do not come from bit-equal logit rows"
        for c in torch.unique(cc).tolist():
            bc = bx[rr[cc == c], c]
            if bc.shape[0] > 1:
                iou = det.box_iou(bc, bc)
                dup = (bc[:, None] == bc[None]).all(-1)
                if bool((((iou - IOU_THR).abs() <= 1e-4) & ~dup).any()):
                    return f"image {b}, class {c}: a candidate pair with an IoU within 1e-4 of iou_thr"
    more = det.detect_post(rois, roi_count, cls, deltas, STDS, img_hw, scale, SCORE_THR, IOU_THR, K + 1, dtype=torch.float64)
    for b in range(B):
        if int(more[3][b]) == K + 1 and float(more[1][b, K - 1] - more[1][b, K]) < SCORE_GAP:
            return f"image {b}: the K-th and (K+1)-th scores do not differ"
    return None


def compare_boxes_part(got, rois, roi_count, cls, deltas, img_hw, scale, K):
    """got = (boxes, scores, labels, count, source) of the kernels (CPU tensors) against the CPU definition: selection exact, values within
    4 x the float32 definition's own error + 1 ulp; returns the measured errors (kernel boxes, f32 boxes, kernel scores, f32 scores)"""
    from panoswintransformerobjectdetection_amd import detector as det
    want = det.detect_post(rois, roi_count, cls, deltas, STDS, img_hw, scale, SCORE_THR, IOU_THR, K)
    truth = det.detect_post(rois, roi_count, cls, deltas, STDS, img_hw, scale, SCORE_THR, IOU_THR, K, dtype=torch.float64)
    assert torch.equal(truth[3], want[3]) and torch.equal(truth[4], want[4]), "the float32 and float64 definitions select differently: conditions?"
    assert got[3].dtype == torch.int32 and got[4].dtype == torch.int32 and got[2].dtype == torch.int64
    assert got[3].tolist() == want[3].tolist()
    assert torch.equal(got[4], want[4]), "source (r * C + c, in order)"
    assert torch.equal(got[2], want[2]), "labels"
    for b, n in enumerate(want[3].tolist()):
        assert not got[0][b, n:].any() and not got[1][b, n:].any() and not got[2][b, n:].any() and not got[4][b, n:].any(), f"image {b}: rows past count"
    eb, eb32 = float((got[0].double() - truth[0]).abs().max()), float((want[0].double() - truth[0]).abs().max())
    es, es32 = float((got[1].double() - truth[1]).abs().max()), float((want[1].double() - truth[1]).abs().max())
    size = max(img_hw) if scale is None else max(img_hw) / float(scale.min())
    print(f"errors vs float64: boxes kernel {eb:.3e} / f32 definition {eb32:.3e} px; scores kernel {es:.3e} / f32 definition {es32:.3e}")
    assert eb <= 4 * eb32 + float(np.spacing(np.float32(size))), (eb, eb32)
    assert es <= 4 * es32 + ULP_ONE, (es, es32)
    return eb, eb32, es, es32


# ---- ops.multiclass_nms_batch ---------------------------------------------------------------------------------------------------------------
def _hot_logits(n, gen):
    """n distinct bf16-exact logits a > -2.9 with 2^-6 <= |a| <= 6: softmax([a, 0, -12, ...]) of neighbours differs by >= 3e-5"""
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    v = v[torch.isfinite(v) & (v.abs() >= 2.0 ** -6) & (v.abs() <= 6) & (v > -2.9)]
    return v[torch.randperm(v.numel(), generator=gen)[:n]]


def _spread_rois(n, H, W, gen):
    c = torch.rand(n, 2, generator=gen) * torch.tensor([W - 40.0, H - 40.0]) + 20
    wh = torch.rand(n, 2, generator=gen) * 30 + 10
    return torch.round(torch.cat([c - wh / 2, c + wh / 2], 1) * 4) / 4


@functools.lru_cache(maxsize=None)
def nms_case(R, C, K, H, W, seed):
    """The four images of the issue (CPU tensors; logits and deltas are bf16-exact, so the f32 and the bf16 run see the same numbers).  Every
    proposal has ONE class that can pass the threshold (logit a from _hot_logits, background 0, every other class -12)."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.full((4, R, C + 1), -12.0)
    cls[:, :, C] = 0.0
    rois = torch.stack([_spread_rois(R, H, W, g) for _ in range(4)])
    deltas = _bf16_exact(torch.randn(4, R, 4 * C, generator=g) * 0.5)
    hot = torch.randint(0, C, (4, R), generator=g)
    for b in range(4):
        cls[b, torch.arange(R), hot[b]] = _hot_logits(R, g)
    count = torch.tensor([0, R, R - 7, R], dtype=torch.int32)
    # image 1: every score below the threshold
    cls[1] = 0.0
    cls[1, :, C] = 8.0
    # image 2: more than K survivors; the rows past its count are confident and must never be read
    cls[2, R - 7:, 0], cls[2, R - 7:, 1:C] = 6.0, -12.0
    # image 3: every row passes in class 0; the highest scores are a chain of shifted boxes, then duplicates and a zero-width box
    a = torch.sort(_hot_logits(R, g), descending=True)[0]
    cls[3, :, :C] = -12.0
    cls[3, :, 0] = a[torch.randperm(R, generator=g)]
    n_chain = min(140, R // 2)
    order = torch.argsort(cls[3, :, 0], descending=True)
    chain = order[:n_chain]                                       # sorted positions 0 .. n_chain - 1: three 64-row chunks at R = 1000
    deltas[3, :, 0:4] = _bf16_exact(torch.randn(R, 4, generator=g) * 0.2)
    i = torch.arange(n_chain, dtype=torch.float32)
    rois[3, chain] = torch.stack([10 + i, torch.full_like(i, 50.0), 110 + i, torch.full_like(i, 150.0)], 1)      # IoU(i, j) = (100 - d) / (100 + d)
    deltas[3, chain, 0:4] = 0.0
    dup = order[n_chain:n_chain + 6]
    rois[3, dup] = torch.tensor([W - 60.0, 20.0, W - 20.0, 60.0])   # six exact duplicates with different scores ...
    deltas[3, dup, 0:4] = 0.0
    cls[3, dup[5]] = cls[3, dup[4]]                               # ... two of them with bit-equal logits
    zw = order[n_chain + 6]
    rois[3, zw] = torch.tensor([W - 100.0, 100.0, W - 100.0, 180.0])  # zero width
    deltas[3, zw, 0:4] = 0.0
    tie = order[n_chain + 7:n_chain + 9]
    cls[3, tie[1]] = cls[3, tie[0]]                               # a tie between two boxes that both survive
    return rois, count, cls, deltas


@functools.lru_cache(maxsize=None)
def _find_case(R, C, K, H, W):
    for seed in range(40):
        case = nms_case(R, C, K, H, W, seed)
        if check_conditions(*case, (H, W), None, K) is None:
            return case
    raise AssertionError("no seed below 40 gives inputs that meet the conditions")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R,C,K,H,W", [(1000, 80, 100, 512, 1024), (70, 3, 5, 128, 256)])
def test_multiclass_nms_batch_selects_what_the_definition_selects(ops, R, C, K, H, W, dtype):
    from panoswintransformerobjectdetection_amd import detector as det
    rois, count, cls, deltas = _find_case(R, C, K, H, W)
    assert check_conditions(rois, count, cls, deltas, (H, W), None, K) is None
    truth = det.detect_post(rois, count, cls, deltas, STDS, (H, W), None, SCORE_THR, IOU_THR, R * C, dtype=torch.float64)
    n3 = int((torch.softmax(cls[3].double(), -1)[:, 0] > SCORE_THR).sum())
    assert truth[3].tolist()[:2] == [0, 0] and int(truth[3][2]) > K and n3 == R            # truncation active; a class with all R rows
    got = ops.multiclass_nms_batch(rois.to(DEV), count.to(DEV), cls.to(DEV, dtype), deltas.to(DEV, dtype), STDS, (H, W), None, SCORE_THR, IOU_THR, K)
    torch.cuda.synchronize()
    compare_boxes_part([t.cpu() for t in got], rois, count, cls, deltas, (H, W), None, K)


def test_multiclass_nms_batch_with_a_scale_factor(ops):
    R, C, K, H, W = 70, 3, 5, 128, 256
    rois, count, cls, deltas = _find_case(R, C, K, H, W)
    scale = torch.tensor([[0.5, 0.5, 0.5, 0.5], [1.0, 1.0, 1.0, 1.0], [0.8, 0.75, 0.8, 0.75], [2.0, 2.0, 2.0, 2.0]])
    cond = check_conditions(rois, count, cls, deltas, (H, W), scale, K)
    assert cond is None, cond
    got = ops.multiclass_nms_batch(rois.to(DEV), count.to(DEV), cls.to(DEV), deltas.to(DEV), STDS, (H, W), scale.to(DEV), SCORE_THR, IOU_THR, K)
    torch.cuda.synchronize()
    compare_boxes_part([t.cpu() for t in got], rois, count, cls, deltas, (H, W), scale, K)


# ---- ops.paste_masks ------------------------------------------------------------------------------------------------------------------------
def compare_masks(got, ref_float, thr, count):
    """got uint8 [B, K, H, W] against the float reference [B, K, H, W] (zeros behind count): equal outside the near-threshold set"""
    near = (ref_float - thr).abs() <= 1e-4
    frac = float(near.float().mean())
    print(f"pixels within 1e-4 of the threshold: {frac:.5%}")
    assert frac <= 1e-3, frac
    want = ref_float >= thr
    for b, n in enumerate(count.tolist()):
        want[b, n:] = False
        assert not got[b, n:].any(), f"image {b}: rows past count"
    assert int(got.max()) <= 1
    assert torch.equal(got.bool() | near, want | near)
    return frac


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16_channels_last"])
@pytest.mark.parametrize("tag,H,W", [("plain", 64, 128), ("rescale", 64, 128), ("small", 37, 53)])
def test_paste_masks_against_the_reference_and_the_definition(ops, tag, H, W, dtype):
    from panoswintransformerobjectdetection_amd import detector as det
    g = np.load(GOLDEN)
    B, K, thr = 3, 12, float(g["paste_thr"])
    lg12 = torch.from_numpy(g["paste_logits_q"]).float() / 64
    lab12 = torch.from_numpy(g["paste_labels"])
    C = lg12.shape[1]
    gen = torch.Generator().manual_seed(31)
    logits = torch.cat([3 * torch.randn(K, C, 28, 28, generator=gen), lg12, lg12]).to(dtype)                # image 0 is never read
    labels = torch.stack([torch.randint(0, C, (K,), generator=gen), lab12, lab12])
    if tag == "small":
        bx = torch.from_numpy(g["paste_plain_boxes"]) * torch.tensor([W / 128, H / 64, W / 128, H / 64])
    else:
        bx = torch.from_numpy(g[f"paste_{tag}_boxes"])
    boxes = torch.stack([bx, bx, bx]).float()
    count = torch.tensor([0, 5, 12], dtype=torch.int32)
    ref = torch.zeros(B, K, H, W)
    for b, n in enumerate(count.tolist()):
        if n:
            prob = logits.float().view(B, K, C, 28, 28)[b, torch.arange(n), labels[b, :n]].sigmoid()
            ref[b, :n] = det.paste_masks(prob, boxes[b, :n], H, W, thr, return_float=True)
    if tag != "small" and dtype == torch.float32:                 # the reference's own float image, bit for bit (also tests/test_detect_post.py)
        assert np.array_equal(ref[2].numpy().view(np.int32), g[f"paste_{tag}_float"].view(np.int32))
    dl = logits.to(DEV)
    if dtype == torch.bfloat16:
        dl = dl.contiguous(memory_format=torch.channels_last)     # the mask head's layout: read in place through its strides
    out = torch.full((B, K, H, W), 255, dtype=torch.uint8, device=DEV)
    res = ops.paste_masks(dl, labels.to(DEV), boxes.to(DEV), count.to(DEV), thr, (H, W), out=out)
    torch.cuda.synchronize()
    assert res is out
    got = out.cpu()
    assert not got[0].any()
    compare_masks(got, ref, thr, count)
    if tag != "small" and dtype == torch.float32:                 # get_seg_masks' booleans, except the degenerate box's (see the fixture's _about)
        want = np.unpackbits(g[f"paste_{tag}_bool"])[:K * H * W].reshape(K, H, W).astype(bool)
        near = (ref[2] - thr).abs().numpy() <= 1e-4
        for i in range(K):
            if i not in set(g[f"paste_{tag}_region_only"].tolist()):
                assert np.array_equal(got[2, i].numpy().astype(bool) | near[i], want[i] | near[i]), i


# ---- heads_predict, captured once and replayed ----------------------------------------------------------------------------------------------
def test_one_captured_heads_predict_is_replayed_on_other_feature_maps():
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _replay_body(side)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


# The heads are initialised for training (std 0.01): every class score of every proposal is near 1 / 81.  Scaling fc_cls's weights spreads
# the logits, and a background bias then leaves of the order of a hundred candidates per image, with scores spread over (0.05, 1) -- few
# enough, and far enough apart, for the conditions of the comparison to hold (chosen on the CPU with the PyTorch RoIAlign stand-in).
FC_CLS_SCALE, BACKGROUND_BIAS = 300.0, 16.0


def _replay_body(side):
    from panoswintransformerobjectdetection_amd import detector as det
    from panoswintransformerobjectdetection_amd.graph import GraphedCallable
    B, H, W = 2, 128, 256
    torch.manual_seed(0)
    m = det.MiniMaskRCNN(dict(TINY, compute_dtype=torch.float32), num_classes=80).to(DEV).eval()
    with torch.no_grad():
        m.bbox_head.cls.weight.mul_(FC_CLS_SCALE)                 # so that every image yields detections (asserted below)
        m.bbox_head.cls.bias[m.num_classes] += BACKGROUND_BIAS
    K, C = m.test_cfg["rcnn"]["max_per_img"], m.num_classes
    gen = torch.Generator().manual_seed(7)
    sets = [[torch.randn(B, c, H // s, W // s, generator=gen) for c, s in zip(m.backbone.num_features, (4, 8, 16, 32))] for _ in range(3)]
    feats = [f.to(DEV) for f in sets[0]]
    state = {}

    def step():
        state["out"] = m.heads_predict(feats, (H, W), return_raw=True)
        return state["out"][0].count

    g = GraphedCallable(step, warmup=2, stream=side, parameters=[])
    for replay, fs in enumerate(sets[1:] + sets[:1]):             # other feature maps than the captured ones first
        for dst, src in zip(feats, fs):
            dst.copy_(src.to(DEV))
        g()
        side.synchronize()
        out, raw = state["out"]
        rois, roi_count, cls, deltas = raw["rois"].cpu(), raw["roi_count"].cpu(), raw["cls"].float().cpu(), raw["deltas"].float().cpu()
        R = rois.shape[1]
        assert tuple(cls.shape) == (B, R, C + 1) and tuple(raw["mask_logits"].shape) == (B * K, C, 28, 28)
        assert bool((roi_count > 0).all()) and bool((roi_count <= R).all())
        cond = check_conditions(rois, roi_count, cls, deltas, (H, W), None, K)
        if cond is not None:
            pytest.skip(f"replay {replay}: the inputs violate a condition of the comparison: {cond}")
        got = [t.cpu() for t in (out.boxes, out.scores, out.labels, out.count, out.source)]
        assert bool((got[3] > 0).all()), f"replay {replay}: an image without detections (FC_CLS_SCALE, BACKGROUND_BIAS)"
        print(f"replay {replay}: roi_count {roi_count.tolist()}, detections {got[3].tolist()}")
        compare_boxes_part(got, rois, roi_count, cls, deltas, (H, W), None, K)
        for b, n in enumerate(got[3].tolist()):
            assert bool((got[4][b, :n] // C < roi_count[b]).all()), "a detection from a proposal past roi_count"
        want = det.detect_post(rois, roi_count, cls, deltas, STDS, (H, W), None, SCORE_THR, IOU_THR, K)
        ml = raw["mask_logits"].float().cpu().view(B, K, C, 28, 28)
        ref = torch.zeros(B, K, H, W)
        for b, n in enumerate(want[3].tolist()):
            prob = ml[b, torch.arange(n), want[2][b, :n]].sigmoid()
            ref[b, :n] = det.paste_masks(prob, want[0][b, :n], H, W, 0.5, return_float=True)
        assert out.masks.dtype == torch.uint8 and tuple(out.masks.shape) == (B, K, H, W)
        compare_masks(out.masks.cpu(), ref, 0.5, want[3])
