"""Test-time augmentation on the CPU: the definitions of tta.py against the reference's own merge functions (tests/golden/aug_test.npz,
tools/gen_augtest_golden.py), the planted defects of tests/_aug_cases.py each caught by that fixture, aug_heads_predict on a tiny random
feature pyramid for both model classes with the PyTorch RoIAlign stand-in, pano_aug.test_views' geometry, and the argument checks of the
new entry points.  The kernels themselves: tests/test_aug_test_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import _aug_cases as cases


# ---- the definitions against the reference --------------------------------------------------------------------------------------------------
def test_the_definitions_reproduce_the_reference():
    """everything bit for bit, except merge_aug_bboxes at V = 6 (torch's own summation order): within the bound of _aug_cases.summation_bound"""
    from panoswintransformerobjectdetection_amd import tta
    assert cases.golden_failures(tta) == []


def test_the_fixture_says_what_is_unpinned():
    about = str(cases.golden()["_about"])
    assert "UNPINNED" in about and "STAND-IN" in about and "mmcv.ops.nms" in about


def test_the_second_statement_reproduces_the_reference_too():
    assert cases.golden_failures(cases.Restated()) == []


@pytest.mark.parametrize("defect", cases.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    bad = cases.golden_failures(cases.Restated(defect))
    print(defect, "->", bad)
    assert bad, f"the fixture does not notice: {defect}"


def test_map_back_inverts_map_to_view_on_dyadic_views():
    from panoswintransformerobjectdetection_amd import tta
    boxes = torch.round(torch.rand(50, 4, generator=torch.Generator().manual_seed(1)) * 400) / 4
    for view in (tta.View((64, 128), 0.5, True), tta.View((256, 512), 2.0, True), tta.View((128, 256), 1.0, False)):
        assert torch.equal(tta.map_back(tta.map_to_view(boxes, view), view), boxes)
    wide = boxes.reshape(10, 20)                                  # [R, 4 C] rows
    assert torch.equal(tta.map_back(wide, tta.View((64, 128), 0.5, True)).reshape(50, 4), tta.map_back(boxes, tta.View((64, 128), 0.5, True)))


def test_merge_aug_proposals_edges():
    """all views empty; one view empty; an exact duplicate across views is suppressed; max_per_img caps the rows; ties go to the smaller
    concatenated position"""
    from panoswintransformerobjectdetection_amd import tta
    views = [tta.View((64, 128), 1.0, False), tta.View((64, 128), 1.0, True)]
    props = torch.zeros(2, 1, 3, 4)
    props[0, 0] = torch.tensor([[10.0, 10, 30, 30], [60.0, 10, 80, 30], [10.0, 40, 30, 60]])
    props[1, 0] = tta.map_to_view(torch.tensor([[10.0, 10, 30, 30], [90.0, 40, 110, 60], [60.0, 40, 80, 60]]), views[1])
    scores = torch.tensor([[[0.9, 0.5, 0.5]], [[0.8, 0.5, 0.4]]])
    r, s, n = tta.merge_aug_proposals(props, scores, torch.zeros(2, 1, dtype=torch.int32), views, 0.7, 10)
    assert int(n) == 0 and tuple(r.shape) == (1, 6, 4) and not r.any() and not s.any()
    r, s, n = tta.merge_aug_proposals(props, scores, torch.tensor([[0], [3]], dtype=torch.int32), views, 0.7, 10)
    assert int(n) == 3 and s[0, :3].tolist() == pytest.approx([0.8, 0.5, 0.4]) and r[0, 0].tolist() == [10, 10, 30, 30]
    r, s, n = tta.merge_aug_proposals(props, scores, torch.tensor([[3], [3]], dtype=torch.int32), views, 0.7, 10)
    assert int(n) == 5 and s[0, :5].tolist() == pytest.approx([0.9, 0.5, 0.5, 0.5, 0.4])            # view 1's twin of row 0 is gone
    assert r[0, 1].tolist() == [60, 10, 80, 30] and r[0, 2].tolist() == [10, 40, 30, 60] and r[0, 3].tolist() == [90, 40, 110, 60]
    r2, s2, n2 = tta.merge_aug_proposals(props, scores, torch.tensor([[3], [3]], dtype=torch.int32), views, 0.7, 2)
    assert int(n2) == 2 and tuple(r2.shape) == (1, 2, 4) and torch.equal(r2[0], r[0, :2])


# ---- aug_heads_predict ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mask_rcnn", "cascade"])
def test_a_single_identity_view_is_heads_predict(kind):
    from panoswintransformerobjectdetection_amd import detector as det
    from panoswintransformerobjectdetection_amd import tta
    m = cases.cpu_model(kind)
    B, H, W = 2, 64, 128
    feats = cases.pyramid(m, B, H, W, seed=3)
    want = m.heads_predict(feats, (H, W), scale_factor=torch.ones(B, 4), rescale=True, ori_hw=(H, W))
    got = m.aug_heads_predict([feats], [tta.View((H, W))], ori_hw=(H, W))
    assert isinstance(got, det.Detections) and int(want.count.sum()) > 0
    for name in ("boxes", "scores", "labels", "count", "source", "masks"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name


@pytest.mark.parametrize("kind", ["mask_rcnn", "cascade"])
def test_aug_heads_predict_is_the_definitions_on_its_raw_tensors(kind):
    """three views (identity, its flip, half scale): shapes, dtypes, zeros past the count, and every merge applied to the raw tensors"""
    from panoswintransformerobjectdetection_amd import detector as det
    from panoswintransformerobjectdetection_amd import tta
    m = cases.cpu_model(kind)
    B, H, W = 2, 64, 128
    K, C = m.test_cfg["rcnn"]["max_per_img"], m.num_classes
    views = [tta.View((H, W)), tta.View((H, W), 1.0, True), tta.View((H // 2, W // 2), 0.5, False)]
    feats_list = [cases.pyramid(m, B, v.img_hw[0], v.img_hw[1], seed=5 + i) for i, v in enumerate(views)]
    out, raw = m.aug_heads_predict(feats_list, views, ori_hw=(H, W), return_raw=True)
    assert tuple(out.boxes.shape) == (B, K, 4) and tuple(out.masks.shape) == (B, K, H, W) and out.masks.dtype == torch.uint8
    assert out.count.dtype == torch.int32 and out.source.dtype == torch.int32 and out.labels.dtype == torch.long
    assert int(out.count.min()) > 0
    n_src = len(views) * (3 if kind == "cascade" else 1)
    assert len(raw["mask_logits"]) == n_src and raw["mask_flips"] == [v.flip for v in views for _ in range(n_src // len(views))]
    rcfg, cfg = m.test_cfg["rpn"], m.test_cfg["rcnn"]
    rois, _, roi_count = tta.merge_aug_proposals(raw["props"], raw["prop_scores"], raw["prop_count"], views, rcfg["nms"], rcfg["max_per_img"])
    assert torch.equal(rois, raw["rois"]) and torch.equal(roi_count, raw["roi_count"])
    assert int(roi_count.max()) <= rois.shape[1] <= rcfg["max_per_img"]
    for v, view in enumerate(views):
        first = raw["rois_v"][v] if kind == "mask_rcnn" else None
        if first is not None:
            assert torch.equal(first, tta.map_to_view(rois, view))
    bx, sc, lb, n, src = tta.aug_detect_post(raw["rois_v"], roi_count, raw["cls_v"], raw["deltas_v"], raw["stds"], views, cfg["score_thr"],
                                             cfg["nms"], K)
    assert torch.equal(bx, out.boxes) and torch.equal(sc, out.scores) and torch.equal(lb, out.labels) and torch.equal(n, out.count)
    assert torch.equal(src, out.source)
    prob = tta.merge_aug_masks(raw["mask_logits"], raw["mask_flips"], lb).reshape(B, K, 28, 28)
    for b, k in enumerate(n.tolist()):
        assert torch.equal(out.masks[b, :k].bool(), det.paste_masks(prob[b, :k], bx[b, :k], H, W, cfg["mask_thr_binary"]))
        assert not out.masks[b, k:].any() and not out.boxes[b, k:].any() and not out.scores[b, k:].any()
        assert bool((out.source[b, :k] // C < roi_count[b]).all())
        assert bool((out.boxes[b, :k, 0::2] <= W).all()) and bool((out.boxes[b, :k, 1::2] <= H).all())
    box_only = m.aug_heads_predict(feats_list, views, with_masks=False)
    assert box_only.masks is None and torch.equal(box_only.boxes, out.boxes)


def test_a_flipped_view_of_a_mirrored_pyramid_votes_for_the_same_boxes():
    """merge_aug_bboxes of (a view, the same view flipped with mirrored RoIs and mirrored x deltas) is the view's own result where no clip
    is active: the flip mapping, the decode and the un-flip cancel"""
    from panoswintransformerobjectdetection_amd import tta
    g = torch.Generator().manual_seed(9)
    H, W, R, C = 64, 128, 40, 3
    c = torch.rand(1, R, 2, generator=g) * torch.tensor([W - 60.0, H - 30.0]) + torch.tensor([30.0, 15.0])
    wh = torch.rand(1, R, 2, generator=g) * 16 + 4
    rois = torch.round(torch.cat([c - wh / 2, c + wh / 2], -1) * 4) / 4
    deltas = torch.round(torch.randn(1, R, 4 * C, generator=g) * 16) / 64
    cls = torch.randn(1, R, C + 1, generator=g)
    v0, v1 = tta.View((H, W)), tta.View((H, W), 1.0, True)
    mirrored = deltas.clone()
    mirrored[..., 0::4] = -deltas[..., 0::4]
    one = tta.merge_aug_bboxes([rois], [cls], [deltas], cases.STDS, [v0])
    two = tta.merge_aug_bboxes([rois, tta.map_to_view(rois, v1)], [cls, cls], [deltas, mirrored], cases.STDS, [v0, v1])
    assert torch.allclose(two[0], one[0], atol=1e-4, rtol=0) and torch.equal(two[1], one[1])


# ---- pano_aug.test_views --------------------------------------------------------------------------------------------------------------------
def test_test_views_geometry():
    from panoswintransformerobjectdetection_amd import pano_aug
    views = pano_aug.test_view_geometry((100, 200), [(256, 128), (400, 200)], flip=True)
    assert len(views) == 4 and [v.flip for v in views] == [False, True, False, True]
    for v in views:
        h, w = v.img_hw
        assert v.scale_factor == (float(np.float32(w / 200)), float(np.float32(h / 100)), float(np.float32(w / 200)), float(np.float32(h / 100)))
    assert views[0].img_hw == views[1].img_hw == pano_aug.rescale_size(100, 200, (256, 128))
    assert views[2].img_hw == pano_aug.rescale_size(100, 200, (400, 200))
    assert len(pano_aug.test_view_geometry((100, 200), [(256, 128)], flip=False)) == 1


# ---- the entry points' argument checks (no GPU needed: every check comes before the launch) --------------------------------------------------
def test_argument_errors_of_the_aug_entry_points_without_a_gpu():
    from panoswintransformerobjectdetection_amd import _lib
    lib = _lib.load()
    ERR = -1
    buf = (ctypes.c_char * 8192)()
    p16 = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15
    f = ctypes.c_float
    views = (_lib.AugView * 8)()
    for v in views:
        v.img_h, v.img_w, v.flip = 64, 128, 0
        v.scale[:] = [1.0, 1.0, 1.0, 1.0]
    vp = ctypes.cast(views, ctypes.c_void_p)
    assert lib.pswin_aug_merge_proposals_launches(2, 1000, 1000) == 3 and lib.pswin_aug_merge_proposals_launches(8, 1024, 1000) == 3
    assert lib.pswin_aug_merge_proposals_workspace(8, 1, 1024, 1000) > 0 and lib.pswin_aug_merge_proposals_workspace(2, 8, 1000, 1000) > 0
    for shape in ((9, 1, 100, 10), (8, 1, 1025, 10), (0, 1, 100, 10), (2, 0, 100, 10), (2, 1, 0, 10), (2, 1, 100, 0), (8, 256, 1024, 10)):
        assert lib.pswin_aug_merge_proposals_workspace(*shape) == ERR, shape
    ok = [p16, p16, p16, vp, 2, 1, 100, f(0.7), 50, p16, p16, p16, p16, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (9, None), (10, None), (11, None), (12, None), (4, 9), (4, 0), (6, 4097), (5, 0),
                 (7, f(-0.1)), (8, 0), (0, p16 + 4), (9, p16 + 8), (12, p16 + 4), (1, p16 + 2)):
        bad = list(ok); bad[i] = v
        assert lib.pswin_aug_merge_proposals(*bad) == ERR, (i, v)
    views[1].scale[0] = 0.0
    assert lib.pswin_aug_merge_proposals(*ok) == ERR                                               # a view with a zero scale factor
    views[1].scale[0] = 1.0
    views[1].img_w = 0
    assert lib.pswin_aug_map_rois(p16, vp, 2, 1, 10, p16, None) == ERR
    views[1].img_w = 128
    ok = [p16, vp, 2, 1, 10, p16, None]
    for i, v in ((0, None), (1, None), (5, None), (2, 0), (2, 9), (3, 0), (4, 0), (0, p16 + 4), (5, p16 + 8)):
        bad = list(ok); bad[i] = v
        assert lib.pswin_aug_map_rois(*bad) == ERR, (i, v)
    ptrs = ctypes.cast((ctypes.c_void_p * 8)(*[p16] * 8), ctypes.c_void_p)
    nulls = ctypes.cast((ctypes.c_void_p * 8)(p16, None, p16, p16, p16, p16, p16, p16), ctypes.c_void_p)
    std = ctypes.cast((ctypes.c_float * 4)(0.1, 0.1, 0.2, 0.2), ctypes.c_void_p)
    ok = [ptrs, ptrs, ptrs, 0, 1, std, vp, 2, 8, 1000, 80, p16, p16, None]
    for i, v in ((0, None), (1, None), (2, None), (5, None), (6, None), (11, None), (12, None), (3, 2), (4, 7), (7, 9), (7, 0), (8, 0), (9, 1025),
                 (10, 129), (11, p16 + 4), (1, nulls)):
        bad = list(ok); bad[i] = v
        assert lib.pswin_aug_merge_bboxes(*bad) == ERR, (i, v)
    ok = [p16, p16, 8, 1000, 80, f(0.05), p16, None]
    for i, v in ((0, None), (1, None), (6, None), (3, 1025), (4, 129), (2, 0), (5, f(-0.1)), (0, p16 + 2)):
        bad = list(ok); bad[i] = v
        assert lib.pswin_multiclass_nms_scores_boxes(*bad) == ERR, (i, v)
    ok = [p16, p16, p16, 8, 1000, 80, f(0.5), p16, p16, None]
    for i, v in ((0, None), (1, None), (2, None), (7, None), (8, None), (4, 1025), (5, 129), (3, 0), (6, f(-1.0)), (2, p16 + 4), (8, p16 + 8)):
        bad = list(ok); bad[i] = v
        assert lib.pswin_multiclass_nms_boxes(*bad) == ERR, (i, v)
    ok = [p16, p16, 80000, 100, p16, 8, 1000, 80, 100, p16, p16, p16, p16, p16, None]
    for i, v in ((0, None), (1, None), (4, None), (9, None), (10, None), (11, None), (12, None), (13, None), (8, 1025), (8, 0), (6, 1025), (7, 129),
                 (3, 0), (3, 80001), (2, 50), (9, p16 + 4)):
        bad = list(ok); bad[i] = v
        assert lib.pswin_multiclass_nms_select_boxes(*bad) == ERR, (i, v)
    src = _lib.AugMaskSources()
    src.count = 2
    for i in range(2):
        src.logits[i], src.stride_n[i], src.stride_c[i], src.stride_y[i], src.stride_x[i] = p16, 80 * 784, 784, 28, 1
    ok = [ctypes.byref(src), 1, p16, p16, p16, 8, 100, 80, 512, 1024, f(0.5), p16, None]
    for i, v in ((0, None), (2, None), (3, None), (4, None), (11, None), (1, 7), (6, 1025), (6, 0), (7, 129), (5, 0), (8, 0), (9, 0), (11, p16 + 1),
                 (3, p16 + 4)):
        bad = list(ok); bad[i] = v
        assert lib.pswin_paste_masks_aug(*bad) == ERR, (i, v)
    for count in (0, 25):
        src.count = count
        assert lib.pswin_paste_masks_aug(*ok) == ERR, count
    src.count = 2
    src.stride_x[1] = 0
    assert lib.pswin_paste_masks_aug(*ok) == ERR
    src.stride_x[1] = 1
    src.logits[1] = None
    assert lib.pswin_paste_masks_aug(*ok) == ERR
