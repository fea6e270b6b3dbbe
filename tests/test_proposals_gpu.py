"""pswin_rpn_proposals (csrc/pswin_proposals.hip through ops.rpn_proposals and the MiniMaskRCNN.proposals hook) on the MI355X against
detector.proposals_batch on CPU tensors, evaluated with the sequential greedy NMS (tests/_proposals_cases.py).

EXACT.  With dw = dh = 0 the decode's exp is exactly 1 and every other operation is an IEEE float32 operation that the kernel restates in
the definition's order, so rois, scores and count must be torch.equal to the float32 reference over ALL P rows, the suppressed tail and
its order included.

WITH exp.  expf on the device and on the host may differ in the last place, so the boxes are compared with the float64 definition: the
kernel may err 4 x the float32 CPU definition's own error plus one float32 ulp of the image width (the rule of
tests/test_detect_post_gpu.py).  For that the float32 and the float64 evaluation must keep the same candidates: the test first asserts,
in float64, that no same-level pair of selected candidates has an IoU within 1e-5 of the threshold unless the two are duplicates.  The
float32 definition's own error on these inputs is about 1e-5 to 2e-5 px (printed)."""
import numpy as np
import pytest
import torch

import _proposals_cases as pc
from panoswintransformerobjectdetection_amd import detector as det
from panoswintransformerobjectdetection_amd._lib import PswinError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gpu(ops, cls, reg, anchors, cfg, img_hw):
    got = ops.rpn_proposals(cls.to(DEV), reg.to(DEV), [a.to(DEV) for a in anchors], cfg["nms_pre"], cfg["nms"], cfg["max_per_img"], img_hw)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in got)


def _assert_exact(got, want, P):
    rois, scores, count = got
    assert tuple(rois.shape) == tuple(want[0].shape) == (want[0].shape[0], P, 4) and count.dtype == torch.int32
    assert torch.equal(count, want[2]), (count, want[2])
    assert torch.equal(scores, want[1])
    assert torch.equal(rois, want[0])


# ---- 1: exact, any size ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_128x256():
    return pc.mixed_batch(128, 256, seed=0)          # levels 6144 / 1536 / 384 / 96 / 24


@pytest.mark.parametrize("max_per_img, P", [(1000, 1000), (2048, 2048)])
def test_exact_on_a_batch_with_ties_and_signed_zeros(ops, mixed_128x256, max_per_img, P):
    cls, reg, anchors = mixed_128x256
    cfg = pc.cfg_of(2000, max_per_img)
    want = pc.reference(cls, reg, anchors, cfg, (128, 256))
    if P == 2048:                                    # a suppressed tail whose order is checked
        assert bool((want[2] < P).all())
    got = _gpu(ops, cls, reg, anchors, cfg, (128, 256))
    _assert_exact(got, want, P)
    assert torch.equal(got[0][2], got[0][0]) and torch.equal(got[1][2], got[1][0]) and got[2][2] == got[2][0]      # -0.0 orders as +0.0


def test_exact_with_two_levels_cut_and_three_taken_whole(ops):
    H, W = 64, 128                                   # levels 1536 / 384 / 96 / 24 / 6
    cls, reg, anchors = pc.mixed_batch(H, W, seed=0)
    cfg = pc.cfg_of(200, 1000)
    want = pc.reference(cls, reg, anchors, cfg, (H, W))
    _assert_exact(_gpu(ops, cls, reg, anchors, cfg, (H, W)), want, 526)         # P = the sum of the k_l: every candidate comes out


def test_exact_where_both_trees_take_several_passes(ops):
    """1024 x 1024: the finest level has 196,608 scores (24 chunks of the workgroup's rows: four selection passes, both partial buffers
    written twice) and the concatenated candidates, 4 x 2000 + 768, exceed one chunk (two passes of the final order)"""
    H = W = 1024
    anchors = pc.anchors_of(H, W)
    sizes = [a.shape[0] for a in anchors]
    assert sizes[0] > 16 * ops.rpn_proposals_rows_per_workgroup() and sum(min(2000, n) for n in sizes) > ops.rpn_proposals_rows_per_workgroup()
    A = sum(sizes)
    cls, reg = pc.logits(2, A, seed=3), pc.deltas(2, A, 3, 0.1, 0.0)
    cfg = pc.cfg_of(2000, 1000)
    want = pc.reference(cls, reg, anchors, cfg, (H, W))
    _assert_exact(_gpu(ops, cls, reg, anchors, cfg, (H, W)), want, 1000)


# ---- 2: with exp -------------------------------------------------------------------------------------------------------------------------
def _assert_no_pair_at_the_threshold(cls, reg, anchors, cfg, img_hw):
    """in float64: no same-level pair of selected candidates has an IoU within 1e-5 of the threshold, unless the two are duplicates"""
    at = 0
    for a_l in anchors:
        n = a_l.shape[0]
        for b in range(cls.shape[0]):
            _, ti = det._topk_stable(cls[b, at:at + n], min(cfg["nms_pre"], n))
            bx = det.decode_deltas(a_l.double()[ti], reg[b, at:at + n].double()[ti], (1.0, 1.0, 1.0, 1.0), img_hw)
            near = (det.box_iou(bx, bx) - cfg["nms"]).abs() < 1e-5
            same = (bx[:, None] == bx[None]).all(-1)
            assert not bool((near & ~same).any())
        at += n


def _assert_as_the_definitions(got, cls, reg, anchors, cfg, img_hw, P, what):
    _assert_no_pair_at_the_threshold(cls, reg, anchors, cfg, img_hw)
    want32 = pc.reference(cls, reg, anchors, cfg, img_hw)
    want64 = pc.reference(cls, reg, anchors, cfg, img_hw, torch.float64)
    assert torch.equal(want32[2], want64[2]) and torch.equal(want32[1].double(), want64[1])       # both precisions select alike
    rois, scores, count = got
    assert tuple(rois.shape) == (cls.shape[0], P, 4)
    assert torch.equal(count, want32[2]) and torch.equal(scores, want32[1])                        # scores, count and the order: exact
    err = float((rois.double() - want64[0]).abs().max())
    err32 = float((want32[0].double() - want64[0]).abs().max())
    print(f"{what}: survivors {count.tolist()}, box error of the kernels {err:.3e} px, of the float32 definition {err32:.3e} px")
    assert err <= 4 * err32 + float(np.spacing(np.float32(img_hw[1]))), (err, err32)


def _exp_case(seed, std):
    H, W = 64, 128
    anchors = pc.anchors_of(H, W)
    A = sum(a.shape[0] for a in anchors)
    return pc.logits(2, A, seed), pc.deltas(2, A, seed, std, std), anchors, pc.cfg_of(200, 1000), (H, W)


@pytest.mark.parametrize("std, seed", [(0.3, 0), (0.05, 2)])      # seeds whose inputs meet the asserted condition (0.05: seeds 0 and 1 do not)
def test_with_exp_against_the_float64_definition(ops, std, seed):
    cls, reg, anchors, cfg, hw = _exp_case(seed, std)
    _assert_as_the_definitions(_gpu(ops, cls, reg, anchors, cfg, hw), cls, reg, anchors, cfg, hw, 526, f"std {std}")


# ---- 3: capture --------------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_follows_its_buffers(ops):
    cls0, reg0, anchors, cfg, hw = _exp_case(0, 0.3)
    cls1, reg1 = _exp_case(1, 0.3)[:2]
    dev_a = [a.to(DEV) for a in anchors]
    bc, br = cls0.to(DEV), reg0.to(DEV)
    call = lambda: ops.rpn_proposals(bc, br, dev_a, cfg["nms_pre"], cfg["nms"], cfg["max_per_img"], hw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                       # the workspace is allocated outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    bc.copy_(cls1.to(DEV))
    br.copy_(reg1.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = tuple(t.cpu() for t in out)
    eager = tuple(t.cpu() for t in call())
    assert all(torch.equal(r, e) for r, e in zip(replayed, eager))                                 # bit for bit
    _assert_as_the_definitions(replayed, cls1, reg1, anchors, cfg, hw, 526, "replay on another seed")


# ---- 4: limits ---------------------------------------------------------------------------------------------------------------------------
def test_beyond_the_limits_ops_raises_and_the_hook_falls_back(ops):
    H, W = 64, 128
    cls, reg, anchors = pc.mixed_batch(H, W, seed=2)
    cls, reg, dev_a = cls.to(DEV), reg.to(DEV), [a.to(DEV) for a in anchors]
    with pytest.raises(PswinError):
        ops.rpn_proposals(cls, reg, dev_a, 2049, pc.IOU_THR, 1000, (H, W))
    # nine levels: the three coarsest of the five split further
    nine = dev_a[:2] + [dev_a[2][:48], dev_a[2][48:], dev_a[3][:12], dev_a[3][12:], dev_a[4][:2], dev_a[4][2:4], dev_a[4][4:]]
    assert len(nine) == 9 and sum(a.shape[0] for a in nine) == cls.shape[1]
    with pytest.raises(PswinError):
        ops.rpn_proposals(cls, reg, nine, 200, pc.IOU_THR, 1000, (H, W))
    for a, cfg in ((dev_a, pc.cfg_of(2049, 1000)), (nine, pc.cfg_of(200, 1000))):
        got = det.MiniMaskRCNN.proposals(cls, reg, a, cfg, (H, W))
        per_image = [det.MiniMaskRCNN._proposals(cls[b], reg[b], a, cfg, (H, W)) for b in range(3)]
        assert torch.equal(got[0], torch.stack([p[0] for p in per_image])) and torch.equal(got[1], torch.stack([p[1] for p in per_image]))
        assert torch.equal(got[2], (got[1] > -1e4).sum(1).to(torch.int32)) and got[2].dtype == torch.int32
    # inside the limits the hook IS the kernel path
    inside = det.MiniMaskRCNN.proposals(cls, reg, dev_a, pc.cfg_of(200, 1000), (H, W))
    direct = ops.rpn_proposals(cls, reg, dev_a, 200, pc.IOU_THR, 1000, (H, W))
    assert all(torch.equal(i, d) for i, d in zip(inside, direct))
