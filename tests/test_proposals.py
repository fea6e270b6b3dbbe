"""detector.proposals_batch and the MiniMaskRCNN.proposals hook on the CPU: the batch definition is the stacked per-image one, both paths
of the detector call the hook once per batch with their own cfg, and a CPU tensor runs the definition.  The kernels behind the hook:
tests/test_proposals_gpu.py."""
import ctypes

import pytest
import torch

import _proposals_cases as pc
import _roi_ref
from panoswintransformerobjectdetection_amd import detector as det


def _model(seed=0):
    torch.manual_seed(seed)
    m = det.MiniMaskRCNN(dict(embed_dim=96, depths=[2, 2, 2, 2], num_heads=[3, 6, 12, 24], ape=True), num_classes=80).eval()
    m.roi_align = _roi_ref.roi_align_batched          # CPU: the PyTorch statement stands in for the HIP operator
    return m


@pytest.mark.parametrize("nms_pre, max_per_img, P", [(200, 1000, 526), (200, 300, 300), (2000, 1000, 1000)])
def test_proposals_batch_is_the_stacked_per_image_definition(nms_pre, max_per_img, P):
    H, W = 64, 128
    cls, reg, anchors = pc.mixed_batch(H, W, seed=0, std_xy=0.1, std_wh=0.3)
    cfg = pc.cfg_of(nms_pre, max_per_img)
    rois, scores, count = det.proposals_batch(cls, reg, anchors, cfg, (H, W))
    assert tuple(rois.shape) == (3, P, 4) and tuple(scores.shape) == (3, P) and tuple(count.shape) == (3,) and count.dtype == torch.int32
    for b in range(3):
        bx, sc = det.MiniMaskRCNN._proposals(cls[b], reg[b], anchors, cfg, (H, W))
        assert torch.equal(rois[b], bx) and torch.equal(scores[b], sc)
        n = int(count[b])
        assert n == int((sc > -1e4).sum()) and bool((sc[:n] > -1e4).all()) and bool((sc[n:] == -1e4).all())      # the survivors lead
    assert torch.equal(rois[2], rois[0]) and torch.equal(scores[2], scores[0])                     # -0.0 orders as +0.0
    if P == 526:                                                                                   # every candidate comes out: some are suppressed
        assert bool((count < P).all())


def test_the_dispatch_of_a_cpu_tensor_runs_the_definition(monkeypatch):
    H, W = 64, 128
    cls, reg, anchors = pc.mixed_batch(H, W, seed=1)
    cfg = pc.cfg_of(200, 1000)
    assert det.MiniMaskRCNN.proposals is det.proposals_batch_dispatch
    seen = []
    real = det.proposals_batch
    monkeypatch.setattr(det, "proposals_batch", lambda *a: seen.append(a) or real(*a))
    got = det.proposals_batch_dispatch(cls, reg, anchors, cfg, (H, W))
    assert len(seen) == 1
    want = real(cls, reg, anchors, cfg, (H, W))
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    from panoswintransformerobjectdetection_amd import ops
    via_ops = ops.rpn_proposals(cls, reg, anchors, 200, pc.IOU_THR, 1000, (H, W))                  # CPU tensors: the definition there too
    assert all(torch.equal(g, w) for g, w in zip(via_ops, want))


def test_both_paths_call_the_hook_once_per_batch_with_their_cfg():
    m = _model()
    B, H, W = 3, 64, 128
    torch.manual_seed(5)
    feats = [torch.randn(B, c, H // s, W // s) for c, s in zip((96, 192, 384, 768), (4, 8, 16, 32))]
    calls = []

    def recorder(cls_all, reg_all, anchors, cfg, img_hw):
        calls.append((tuple(cls_all.shape), tuple(reg_all.shape), len(anchors), cfg, tuple(img_hw)))
        return det.proposals_batch(cls_all, reg_all, anchors, cfg, img_hw)

    m.proposals = recorder
    with torch.no_grad():
        fpn = m.neck(feats)
        outs = m.rpn(fpn)
    anchors = det.make_anchors([f.shape[2:] for f in fpn], m.STRIDES, "cpu")
    A = sum(a.shape[0] for a in anchors)
    props = m._rpn_losses_and_proposals(outs, anchors, det.synthetic_targets(B, H, W, "cpu"), (H, W))[2]
    assert len(calls) == 1 and calls[0] == ((B, A), (B, A, 4), 5, m.rpn_cfg, (H, W)) and calls[0][3] is m.rpn_cfg
    assert isinstance(props, list) and len(props) == B                                             # still the per-image list
    cls_all, reg_all = m._rpn_flatten(outs)
    with torch.no_grad():
        for b in range(B):
            assert torch.equal(props[b], m._proposals(cls_all[b], reg_all[b], anchors, m.rpn_cfg, (H, W))[0])
    del calls[:]
    out, raw = m.heads_predict(feats, (H, W), return_raw=True)
    assert len(calls) == 1 and calls[0] == ((B, A), (B, A, 4), 5, m.test_cfg["rpn"], (H, W)) and calls[0][3] is m.test_cfg["rpn"]
    want = det.proposals_batch(cls_all, reg_all, anchors, m.test_cfg["rpn"], (H, W))
    assert torch.equal(raw["rois"], want[0]) and torch.equal(raw["roi_count"], want[2]) and raw["roi_count"].dtype == torch.int32


def test_the_entry_points_limits_without_a_gpu():
    """every check comes before the first launch: PSWIN_ERR_ARG (-1) on a CPU-only host; the predicate of ops mirrors the limits"""
    from panoswintransformerobjectdetection_amd import _lib, ops
    lib = _lib.load()
    ERR = -1
    rows = lib.pswin_rpn_proposals_rows_per_workgroup()
    assert rows >= 4 * 2048 and rows & (rows - 1) == 0

    def sizes(ns):
        arr = (ctypes.c_int * len(ns))(*ns)
        return arr, ctypes.cast(arr, ctypes.c_void_p)

    bench = [98304, 24576, 6144, 1536, 384]                        # 512 x 1024
    keep, p = sizes(bench)
    assert lib.pswin_rpn_proposals_workspace(p, 5, 8, 2000, 1000) > 0 and lib.pswin_rpn_proposals_workspace(p, 5, 8, 1000, 1000) > 0
    assert ops.rpn_proposals_supported(bench, 8, 2000, 1000) and ops.rpn_proposals_supported(bench, 2, 2048, 2048)
    # the launch count depends on the level sizes, nms_pre and P only: selection passes + the NMS's two + the final order's passes
    assert ops.rpn_proposals_launches(bench, 2000, 1000) == 3 + 2 + 1 and ops.rpn_proposals_launches(bench, 1000, 1000) == 3 + 2 + 1
    assert ops.rpn_proposals_launches([1536, 384, 96, 24, 6], 200, 1000) == 1 + 2 + 1
    for bad in ((p, 5, 8, 2049, 1000), (p, 5, 8, 0, 1000), (p, 5, 8, 2000, 0), (p, 5, 0, 2000, 1000), (p, 5, 410, 2000, 1000),
                (p, 0, 8, 2000, 1000), (None, 5, 8, 2000, 1000), (p, 5, 8, 2048, 2049), (p, 5, 2048, 100, 100)):
        assert lib.pswin_rpn_proposals_workspace(*bad) == ERR, bad[1:]
    assert not ops.rpn_proposals_supported(bench, 8, 2049, 1000) and not ops.rpn_proposals_supported(bench, 410, 2000, 1000)
    assert not ops.rpn_proposals_supported(bench, 8, 2048, 2049)
    nine, p9 = sizes([64] * 9)
    assert lib.pswin_rpn_proposals_workspace(p9, 9, 2, 100, 100) == ERR and lib.pswin_rpn_proposals_workspace(p9, 8, 2, 100, 100) > 0
    assert not ops.rpn_proposals_supported([64] * 9, 2, 100, 100)
    zero, pz = sizes([64, 0])
    assert lib.pswin_rpn_proposals_workspace(pz, 2, 2, 100, 100) == ERR
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15
    small, ps = sizes([96, 24])
    ok = [p16, p16, p16, ps, 2, 2, 50, ctypes.c_float(0.7), 60, 64, 128, p16, p16, p16, p16, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (11, None), (12, None), (13, None), (14, None), (1, p16 + 4), (2, p16 + 8),
                 (11, p16 + 4), (14, p16 + 8), (0, p16 + 2), (4, 9), (5, 0), (6, 2049), (7, ctypes.c_float(-0.1)), (8, 0), (9, 0), (10, 0)):
        bad = list(ok)
        bad[i] = v
        assert lib.pswin_rpn_proposals(*bad) == ERR, (i, v)
