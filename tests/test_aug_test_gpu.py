"""Test-time augmentation on the MI355X: the kernels of csrc/pswin_augtest.hip (through ops.aug_* / ops.multiclass_nms_boxes_batch /
ops.paste_masks_aug and aug_heads_predict) against the definitions of tta.py evaluated on the CPU.  Inputs: tests/_aug_cases.py.

Every kernel writes into NaN-filled (0xFF bytes) outputs and, where it has one, a NaN-filled workspace, and runs twice for identical bits.

  * merge_proposals, map_rois and the class-wise NMS on given boxes and scores are compared BIT FOR BIT.  For the two NMS stages that is
    meaningful only where float32 and float64 agree about `IoU > thr`, so each test first asserts on the CPU that no candidate pair lies
    within 1e-4 of the threshold except exact duplicates (conditions on the inputs, as tests/test_detect_post_gpu.py has them).
    The proposal merge sorts all V P composites of an image in ONE chunk (V P <= 8192), so there is no chunk boundary for ties to
    straddle; tied scores across views are in every case (scores lie on a 1 / 4096 grid), V P = 8192 included.
  * merge_bboxes: expf keeps it from being bit-exact.  E_kernel = max |kernel - float64 definition| must not exceed 4 x E_def =
    max |float32 CPU definition - float64 definition| on the same inputs, for boxes (pixels) and for scores; both are printed.
  * paste_masks_aug: equal to paste_masks(merge_aug_masks(...)) outside the pixels whose float value lies within 1e-4 of the threshold, at
    most 0.1 % of the pixels."""
import functools

import numpy as np
import pytest
import torch

import _aug_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IOU_RPN, SCORE_THR, IOU_THR = 0.7, 0.05, 0.5


def poisoned(shape, dtype):
    """a device tensor whose every byte is 0xFF: NaN as float, -1 as integer"""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(255)
    return t


def poison_workspaces(ops):
    for k, v in ops._CACHE.items():
        if isinstance(k, tuple) and k and k[0] in ("aug_proposals_ws", "detect_ws"):
            v.fill_(255)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- merge_proposals and map_rois -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _proposal_case(V, B, P, mode):
    """(props, scores, count, views) and whether they meet the conditions (checked once per case)"""
    case = cases.proposal_case(V, B, P, mode, IOU_RPN)
    return case + (cases.proposal_conditions(*case, IOU_RPN),)


@functools.lru_cache(maxsize=None)
def _proposal_reference(V, B, P, mode, max_per_img):
    from panoswintransformerobjectdetection_amd import tta
    props, scores, count, views, _ = _proposal_case(V, B, P, mode)
    return tta.merge_aug_proposals(props, scores, count, views, IOU_RPN, max_per_img)


def run_merge_proposals(ops, props, scores, count, views, iou_thr, max_per_img):
    V, B, P = props.shape[:3]
    Pm = min(max_per_img, V * P)
    d = [t.to(DEV) for t in (props, scores, count)]
    outs = []
    for rep in range(2):
        out = (poisoned((B, Pm, 4), torch.float32), poisoned((B, Pm), torch.float32), poisoned((B,), torch.int32))
        if rep == 0:                                              # the first call creates the workspace: poison it, then call again
            ops.aug_merge_proposals(*d, views, iou_thr, max_per_img)
        poison_workspaces(ops)
        ops.aug_merge_proposals(*d, views, iou_thr, max_per_img, out=out)
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in out])
    for a, b in zip(*outs):
        assert same_bits(a, b), "two calls differ"
    return outs[0]


@pytest.mark.parametrize("V,B,P,mode,max_per_img", [
    (1, 1, 1, "counts", 1000), (1, 3, 64, "counts", 1000), (2, 3, 65, "counts", 1000), (3, 1, 1000, "counts", 1000), (8, 3, 64, "counts", 1000),
    (2, 1, 1000, "counts", 1000), (8, 1, 1024, "full", 1000), (8, 1, 1024, "full", 8192), (3, 3, 65, "one_view_empty", 1000),
    (2, 3, 64, "all_empty", 1000), (8, 3, 1, "counts", 5)])
def test_merge_proposals_bit_for_bit(ops, V, B, P, mode, max_per_img):
    props, scores, count, views, cond = _proposal_case(V, B, P, mode)
    assert cond is None, cond
    want = _proposal_reference(V, B, P, mode, max_per_img)
    got = run_merge_proposals(ops, props, scores, count, views, IOU_RPN, max_per_img)
    print(f"V {V} B {B} P {P} {mode}: candidates {count.sum(0).tolist()}, survivors {want[2].tolist()} of at most {want[0].shape[1]}")
    assert got[2].tolist() == want[2].tolist()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    if mode == "all_empty":
        assert not got[0].any() and not got[1].any() and not got[2].any()
    assert ops.aug_merge_proposals_launches(V, P, max_per_img) == 3


def test_merge_proposals_cut_below_at_and_above_the_survivors(ops):
    from panoswintransformerobjectdetection_amd import tta
    props, scores, count, views, cond = _proposal_case(2, 3, 65, "counts")
    assert cond is None, cond
    n = [int(v) for v in _proposal_reference(2, 3, 65, "counts", 1000)[2]]
    assert min(n) > 8 and max(n) < 130                            # something is suppressed, something survives
    for m in (min(n) - 3, min(n), n[0], max(n), max(n) + 5):
        want = tta.merge_aug_proposals(props, scores, count, views, IOU_RPN, m)
        got = run_merge_proposals(ops, props, scores, count, views, IOU_RPN, m)
        assert got[2].tolist() == want[2].tolist() == [min(v, m) for v in n]
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])


def test_merge_proposals_chain_across_64_row_words(ops):
    """200 rows in a chain whose links reach 8 rows back: the verdict on the first rows of a 64-row word hangs on rows of the word before"""
    from panoswintransformerobjectdetection_amd import tta
    props, scores, count, views = cases.chain_case()
    assert cases.proposal_conditions(props, scores, count, views, IOU_RPN) is None
    want = tta.merge_aug_proposals(props, scores, count, views, IOU_RPN, 1000)
    kept = set(np.round((1.0 - want[1][0, :int(want[2][0])].double().numpy()) * 256).astype(int).tolist())      # chain positions
    assert kept == set(range(0, 200, 9)), sorted(kept)            # every ninth box survives: 63 -> 72 crosses a word, 126 -> 135 too
    got = run_merge_proposals(ops, props, scores, count, views, IOU_RPN, 1000)
    assert got[2].tolist() == want[2].tolist() and same_bits(got[0], want[0]) and same_bits(got[1], want[1])


@pytest.mark.parametrize("V,B,N", [(1, 1, 1), (3, 3, 65), (8, 2, 1000)])
def test_map_rois_bit_for_bit(ops, V, B, N):
    from panoswintransformerobjectdetection_amd import tta
    views = cases.views_for(V)
    boxes = torch.rand(B, N, 4, generator=torch.Generator().manual_seed(V + N)) * 300 - 20
    want = torch.stack([tta.map_to_view(boxes, v) for v in views])
    outs = []
    for _ in range(2):
        out = poisoned((V, B, N, 4), torch.float32)
        assert ops.aug_map_rois(boxes.to(DEV), views, out=out) is out
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], want)


# ---- class-wise NMS on given boxes and scores ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _merged_case(R, C):
    for seed in range(20):
        case = cases.merged_case(R, C, seed)
        if cases.merged_conditions(*case, SCORE_THR, IOU_THR) is None:
            return case
    raise AssertionError("no seed below 20 gives merged boxes that meet the conditions")


@pytest.mark.parametrize("R,C", [(1, 1), (70, 5), (1000, 80), (1000, 1), (70, 80)])
def test_nms_on_given_boxes_bit_for_bit(ops, R, C):
    from panoswintransformerobjectdetection_amd import tta
    boxes, scores, count = _merged_case(R, C)
    assert cases.merged_conditions(boxes, scores, count, SCORE_THR, IOU_THR) is None
    full = tta.nms_merged(boxes, scores, count, SCORE_THR, IOU_THR, R * C)
    n = [int(v) for v in full[3]]
    assert n[1] == 0 and (R == 1 or n[0] > 0)                     # one image with nothing above the threshold
    Ks = sorted({min(1024, max(1, k)) for k in (n[0] - 2, n[0], n[0] + 3)})    # below, at and above the survivors (K <= 1024)
    d = [t.to(DEV) for t in (boxes, scores, count)]
    for K in Ks:
        want = tta.nms_merged(boxes, scores, count, SCORE_THR, IOU_THR, K)
        outs = []
        for rep in range(2):
            out = (poisoned((3, K, 4), torch.float32), poisoned((3, K), torch.float32), poisoned((3, K), torch.int64), poisoned((3,), torch.int32),
                   poisoned((3, K), torch.int32))
            if rep == 0:
                ops.multiclass_nms_boxes_batch(*d, SCORE_THR, IOU_THR, K)
            poison_workspaces(ops)
            ops.multiclass_nms_boxes_batch(*d, SCORE_THR, IOU_THR, K, out=out)
            torch.cuda.synchronize()
            outs.append([t.cpu() for t in out])
        for a, b, w, name in zip(outs[0], outs[1], want, ("boxes", "scores", "labels", "count", "source")):
            assert same_bits(a, b), f"K {K}: two calls differ in {name}"
            assert same_bits(a, w), f"K {K}: {name}"
        assert bool((outs[0][4][2, :int(want[3][2])] // C < count[2]).all()), "a detection from a row past roi_count"


# ---- merge_bboxes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [1, 2, 6])
def test_merge_bboxes_within_four_times_the_definitions_own_error(ops, V, dtype):
    from panoswintransformerobjectdetection_amd import tta
    rois, cls, deltas, views = cases.bbox_case(V)
    assert any(v.flip for v in views) == (V > 1)
    truth = tta.merge_aug_bboxes(rois, cls, deltas, cases.STDS, views, dtype=torch.float64)
    want = tta.merge_aug_bboxes(rois, cls, deltas, cases.STDS, views)
    # the planted rows do what they are there for: a delta beyond the clip (row 0), a box clipped at its view's border (row 2)
    from panoswintransformerobjectdetection_amd import detector as det
    for v, view in enumerate(views):
        b0 = det.decode_deltas_per_class(rois[v][0], deltas[v][0], cases.STDS, view.img_hw)
        assert float(b0[2, 2]) == view.img_hw[1] and float(b0[2, 3]) == view.img_hw[0]
        assert float(deltas[v][0, 0, 2]) * cases.STDS[2] > abs(np.log(16 / 1000))
    d = ([r.to(DEV) for r in rois], [c.to(DEV, dtype) for c in cls], [x.to(DEV, dtype) for x in deltas])
    B, R, C = cls[0].shape[0], cls[0].shape[1], cls[0].shape[2] - 1
    outs = []
    for _ in range(2):
        out = (poisoned((B, R, 4 * C), torch.float32), poisoned((B, R, C + 1), torch.float32))
        ops.aug_merge_bboxes(*d, cases.STDS, views, out=out)
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in out])
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    eb, eb_def = float((outs[0][0].double() - truth[0]).abs().max()), float((want[0].double() - truth[0]).abs().max())
    es, es_def = float((outs[0][1].double() - truth[1]).abs().max()), float((want[1].double() - truth[1]).abs().max())
    print(f"V {V} {dtype}: boxes E_kernel {eb:.3e} / E_def {eb_def:.3e} px; scores E_kernel {es:.3e} / E_def {es_def:.3e}")
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    assert eb <= 4 * eb_def, (eb, eb_def)
    assert es <= 4 * es_def, (es, es_def)


# ---- paste_masks_aug ------------------------------------------------------------------------------------------------------------------------
def compare_masks(got, ref_float, thr, count):
    """got uint8 [B, K, H, W] against the float reference (zeros behind count): equal outside the near-threshold set (<= 0.1 % of the pixels)"""
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


def mask_reference(logits, flips, labels, boxes, count, H, W, thr):
    from panoswintransformerobjectdetection_amd import detector as det
    from panoswintransformerobjectdetection_amd import tta
    B, K = labels.shape
    prob = tta.merge_aug_masks(logits, flips, labels).reshape(B, K, 28, 28)
    ref = torch.zeros(B, K, H, W)
    for b, n in enumerate(count.tolist()):
        if n:
            ref[b, :n] = det.paste_masks(prob[b, :n], boxes[b, :n], H, W, thr, return_float=True)
    return ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32_nchw", "bf16_channels_last"])
@pytest.mark.parametrize("N,H,W", [(1, 64, 128), (2, 64, 128), (6, 37, 53), (24, 64, 128)])
def test_paste_masks_aug_against_the_definition(ops, N, H, W, dtype):
    logits, flips, labels, boxes, count = cases.mask_case(N)
    assert N == 1 or (any(flips) and not all(flips))
    if (H, W) != (64, 128):
        boxes = boxes * torch.tensor([W / 128, H / 64, W / 128, H / 64])
    logits = [l.to(dtype).float() for l in logits]                # what the kernel reads
    ref = mask_reference(logits, flips, labels, boxes, count, H, W, 0.5)
    dl = [l.to(DEV, dtype) for l in logits]
    if dtype == torch.bfloat16:                                   # the mask heads' layout, and one NCHW source among them
        dl = [l.contiguous(memory_format=torch.channels_last) if i != 1 else l for i, l in enumerate(dl)]
    B, K = labels.shape
    outs = []
    for _ in range(2):
        out = poisoned((B, K, H, W), torch.uint8)
        assert ops.paste_masks_aug(dl, flips, labels.to(DEV), boxes.to(DEV), count.to(DEV), 0.5, (H, W), out=out) is out
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    assert not outs[0][0].any()
    compare_masks(outs[0], ref, 0.5, count)


def test_paste_masks_aug_with_one_unflipped_source_is_paste_masks(ops):
    logits, flips, labels, boxes, count = cases.mask_case(1)
    assert flips == [False]
    d = [t.to(DEV) for t in (logits[0], labels, boxes, count)]
    a = ops.paste_masks_aug([d[0]], [False], d[1], d[2], d[3], 0.5, (64, 128))
    b = ops.paste_masks(*d, 0.5, (64, 128))
    assert torch.equal(a, b)


# ---- aug_heads_predict ------------------------------------------------------------------------------------------------------------------------
# The heads are initialised for training (std 0.01): every class score is near 1 / 81 and every mask logit near 0, the paste's threshold.
# Scaling the last layers' weights spreads them; MiniMaskRCNN's background bias is that of tests/test_detect_post_gpu.py (of the order of
# a hundred candidates per image).  The cascade's 4conv1f heads leave their logits near 0 whatever the last layer's scale, so it is built
# with 5 classes, as tests/_cascade_cases.py builds it: a uniform score of 1 / 6 passes the threshold, and every row is a candidate.
# Measured on an MI355X with MASK_LOGIT_SCALE = 100: 0.36 % of the pixels within 1e-4 of the threshold (1: 3.8 %); hence 1e4.
FC_CLS_SCALE, BACKGROUND_BIAS, MASK_LOGIT_SCALE = 300.0, 16.0, 1e4


class deterministic_convolutions:
    """The library's convolution kernels restricted to its deterministic ones, so that two calls on the same inputs can be compared for
    equality (the heads' convolutions are the library's; everything behind them is this project's and is deterministic by construction)"""

    def __enter__(self):
        self.was = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic = self.was
        return False


def _gpu_model(kind):
    from _util import TINY
    from panoswintransformerobjectdetection_amd import cascade
    from panoswintransformerobjectdetection_amd import detector as det
    torch.manual_seed(0)
    if kind == "mask_rcnn":
        m = det.MiniMaskRCNN(dict(TINY, compute_dtype=torch.float32), num_classes=80).to(DEV).eval()
        heads, mask_heads, bias = [m.bbox_head], [m.mask_head], BACKGROUND_BIAS
    else:
        m = cascade.MiniCascadeRCNN(dict(TINY, compute_dtype=torch.float32), num_classes=5).to(DEV).eval()
        heads, mask_heads, bias = list(m.bbox_heads), list(m.mask_heads), 0.0
    with torch.no_grad():
        for h in heads:
            h.cls.weight.mul_(FC_CLS_SCALE)
            h.cls.bias[m.num_classes] += bias
        for h in mask_heads:
            h.logits.weight.mul_(MASK_LOGIT_SCALE)
    return m


def _check_against_the_definitions(m, out, raw, views, ori_hw):
    from panoswintransformerobjectdetection_amd import tta
    cpu = lambda t: t.detach().float().cpu()                      # noqa: E731
    rcfg, cfg = m.test_cfg["rpn"], m.test_cfg["rcnn"]
    K, C = cfg["max_per_img"], m.num_classes
    props, pscores, pcount = cpu(raw["props"]), cpu(raw["prop_scores"]), raw["prop_count"].cpu()
    # the heads' own proposals are thousands of overlapping boxes: some pair always lies near the threshold.  The kernels evaluate the IoU
    # with the float32 operations of detector.box_iou, so they meet the float32 definition bit for bit all the same; the condition is
    # printed, not required
    print("proposal condition:", cases.proposal_conditions(props, pscores, pcount, views, rcfg["nms"]))
    rois, _, roi_count = tta.merge_aug_proposals(props, pscores, pcount, views, rcfg["nms"], rcfg["max_per_img"])
    assert same_bits(raw["rois"].cpu(), rois) and raw["roi_count"].cpu().tolist() == roi_count.tolist()
    assert int(roi_count.min()) > 0
    rois_v, cls_v, deltas_v = [cpu(t) for t in raw["rois_v"]], [cpu(t) for t in raw["cls_v"]], [cpu(t) for t in raw["deltas_v"]]
    truth = tta.merge_aug_bboxes(rois_v, cls_v, deltas_v, raw["stds"], views, dtype=torch.float64)
    want = tta.merge_aug_bboxes(rois_v, cls_v, deltas_v, raw["stds"], views)
    mb, ms = raw["merged_boxes"].cpu(), raw["merged_scores"].cpu()
    eb, eb_def = float((mb.double() - truth[0]).abs().max()), float((want[0].double() - truth[0]).abs().max())
    es, es_def = float((ms.double() - truth[1]).abs().max()), float((want[1].double() - truth[1]).abs().max())
    print(f"merged boxes E_kernel {eb:.3e} / E_def {eb_def:.3e} px; scores E_kernel {es:.3e} / E_def {es_def:.3e}")
    assert eb <= 4 * eb_def and es <= 4 * es_def
    print("merged-box condition:", cases.merged_conditions(mb, ms, roi_count, cfg["score_thr"], cfg["nms"]))
    sel = tta.nms_merged(mb, ms, roi_count, cfg["score_thr"], cfg["nms"], K)
    got = [t.cpu() for t in (out.boxes, out.scores, out.labels, out.count, out.source)]
    for a, w, name in zip(got, sel, ("boxes", "scores", "labels", "count", "source")):
        assert same_bits(a, w), name
    assert int(sel[3].min()) > 0, "an image without detections (FC_CLS_SCALE, BACKGROUND_BIAS)"
    logits = [cpu(l) for l in raw["mask_logits"]]
    ref = mask_reference(logits, raw["mask_flips"], sel[2], sel[0], sel[3], ori_hw[0], ori_hw[1], cfg["mask_thr_binary"])
    assert out.masks.dtype == torch.uint8 and tuple(out.masks.shape) == (sel[0].shape[0], K) + tuple(ori_hw)
    compare_masks(out.masks.cpu(), ref, cfg["mask_thr_binary"], sel[3])
    return roi_count.tolist()


def _views_and_sets(m, B, n_sets):
    from panoswintransformerobjectdetection_amd import tta
    H, W = 128, 256                                               # a 32 x 64 pyramid at stride 4
    views = [tta.View((H, W)), tta.View((H, W), 1.0, True), tta.View((H // 2, W // 2), 0.5, False)]
    sets = [[cases.pyramid(m, B, v.img_hw[0], v.img_hw[1], seed=100 * s + i) for i, v in enumerate(views)] for s in range(n_sets)]
    return (H, W), views, sets


@pytest.mark.parametrize("kind", ["mask_rcnn", "cascade"])
def test_aug_heads_predict_is_the_definitions_on_its_raw_tensors(kind):
    m = _gpu_model(kind)
    ori_hw, views, sets = _views_and_sets(m, 2, 1)
    feats_list = [[f.to(DEV) for f in fs] for fs in sets[0]]
    out, raw = m.aug_heads_predict(feats_list, views, ori_hw=ori_hw, return_raw=True)
    torch.cuda.synchronize()
    _check_against_the_definitions(m, out, raw, views, ori_hw)


@pytest.mark.parametrize("kind", ["mask_rcnn", "cascade"])
def test_a_single_identity_view_is_heads_predict(kind):
    from panoswintransformerobjectdetection_amd import tta
    m = _gpu_model(kind)
    ori_hw, views, sets = _views_and_sets(m, 2, 1)
    feats = [f.to(DEV) for f in sets[0][0]]
    with deterministic_convolutions():
        m.heads_predict(feats, ori_hw)                            # the first call of a shape lets the library pick its convolution kernels
        want = m.heads_predict(feats, ori_hw, scale_factor=torch.ones(2, 4, device=DEV), rescale=True, ori_hw=ori_hw)
        got = m.aug_heads_predict([feats], [tta.View(ori_hw)], ori_hw=ori_hw)
    torch.cuda.synchronize()
    assert int(want.count.sum()) > 0
    for name in ("boxes", "scores", "labels", "count", "source", "masks"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name


def test_one_captured_aug_heads_predict_is_replayed_on_other_feature_maps():
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), deterministic_convolutions():
        _replay_body(side)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def _replay_body(side):
    from panoswintransformerobjectdetection_amd.graph import GraphedCallable
    m = _gpu_model("mask_rcnn")
    ori_hw, views, sets = _views_and_sets(m, 2, 3)
    feats_list = [[f.to(DEV) for f in fs] for fs in sets[0]]
    state = {}

    def step():
        state["out"] = m.aug_heads_predict(feats_list, views, ori_hw=ori_hw, return_raw=True)
        return state["out"][0].count

    g = GraphedCallable(step, warmup=2, stream=side, parameters=[])
    seen = []
    for replay, fs in enumerate(sets[1:] + sets[:1]):             # other feature maps than the captured ones first
        for dst_v, src_v in zip(feats_list, fs):
            for dst, src in zip(dst_v, src_v):
                dst.copy_(src.to(DEV))
        g()
        side.synchronize()
        out, raw = state["out"]
        replayed = [t.clone() for t in (out.boxes, out.scores, out.labels, out.count, out.source, out.masks, raw["roi_count"], raw["prop_count"])]
        # the replayed merges are the eager merges of the replay's own raw tensors, bit for bit ...
        from panoswintransformerobjectdetection_amd import ops
        rcfg, cfg = m.test_cfg["rpn"], m.test_cfg["rcnn"]
        e_rois, _, e_count = ops.aug_merge_proposals(raw["props"], raw["prop_scores"], raw["prop_count"], views, rcfg["nms"], rcfg["max_per_img"])
        e_mb, e_ms = ops.aug_merge_bboxes(raw["rois_v"], raw["cls_v"], raw["deltas_v"], raw["stds"], views)
        e_sel = ops.multiclass_nms_boxes_batch(e_mb, e_ms, e_count, cfg["score_thr"], cfg["nms"], cfg["max_per_img"])
        e_masks = ops.paste_masks_aug(raw["mask_logits"], raw["mask_flips"], e_sel[2], e_sel[0], e_sel[3], cfg["mask_thr_binary"], ori_hw)
        side.synchronize()
        assert torch.equal(e_rois, raw["rois"]) and torch.equal(e_count, raw["roi_count"]) and torch.equal(e_mb, raw["merged_boxes"])
        for a, b, name in zip(replayed[:6], (e_sel[0], e_sel[1], e_sel[2], e_sel[3], e_sel[4], e_masks), ("boxes", "scores", "labels", "count",
                                                                                                          "source", "masks")):
            assert torch.equal(a, b), f"replay {replay}: {name} differs from the eager merges of the replay's raw tensors"
        # ... and the whole replay equals a whole eager call
        eager, eraw = m.aug_heads_predict(feats_list, views, ori_hw=ori_hw, return_raw=True)
        side.synchronize()
        for a, b, name in zip(replayed, (eager.boxes, eager.scores, eager.labels, eager.count, eager.source, eager.masks, eraw["roi_count"],
                                         eraw["prop_count"]), ("boxes", "scores", "labels", "count", "source", "masks", "roi_count", "prop_count")):
            assert torch.equal(a, b), f"replay {replay}: {name} differs from an eager call"
        assert int(replayed[3].min()) > 0
        seen.append((replayed[7].cpu().tolist(), replayed[6].cpu().tolist()))
        print(f"replay {replay}: proposal counts {seen[-1][0]}, merged {seen[-1][1]}, detections {replayed[3].tolist()}")
    assert seen[0] != seen[1], "the replays saw the same proposal counts: they would not show that the counts are read from the device"
