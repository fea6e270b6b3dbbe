"""Mean average precision on the CPU: the definitions of panoswintransformerobjectdetection_amd/evaluation.py against the reference's own
results (tests/golden/eval_map.npz, tools/gen_eval_golden.py: tpfp_default and eval_map of mmdet/core/evaluation/mean_ap.py), the padded
form against the list form, the mask IoU against hand-made bitmaps, the accumulator, and the argument checks of the new entry points.
The kernels themselves: tests/test_eval_map_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from panoswintransformerobjectdetection_amd import evaluation as ev
from panoswintransformerobjectdetection_amd._lib import PswinError
from panoswintransformerobjectdetection_amd.detector import Detections, PaddedTargets

import _eval_cases as cases


@pytest.fixture(scope="module")
def golden():
    return cases.load_golden()


# ---- the definitions against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(cases.CASES))
def test_marks_reproduce_tpfp_default(golden, case):
    thr, ranged = cases.CASES[case]
    dets, gts, ignore = cases.golden_padded(golden)
    rng = cases.scale_ranges(golden, ranged)
    area_ranges = None if rng is None else [(a * a, b * b) for a, b in rng]
    marks = ev.match_pairs(ev.box_iou_pairs(dets, gts), dets, gts, ignore, (thr,), area_ranges, ev.box_areas(dets.boxes),
                           ev.box_areas(gts.boxes))
    assert marks.dtype == torch.uint8 and np.array_equal(marks[0].numpy(), golden[case + "_marks"])


def test_the_fixture_holds_the_cases_it_promises(golden):
    dets, gts, ignore = cases.golden_padded(golden)
    best = ev.box_iou_pairs(dets, gts).max(2)[0]
    assert (best == 0.5).any() and (best == 0.75).any()                         # detections exactly on both thresholds
    assert ignore.any() and (golden["in_gt_count"] == 0).any() and (golden["in_det_count"] == 0).any()
    assert (golden["thr50_num_gts"][0] == 0).tolist() == [False, False, False, True]       # class 3 has no ground truth
    same = [(gts.boxes[b, i] == gts.boxes[b, j]).all() and gts.labels[b, i] == gts.labels[b, j] and not ignore[b, i] and not ignore[b, j]
            for b in range(12) for i in range(int(gts.count[b])) for j in range(i)]
    assert any(same)                                                            # two identical regular boxes in one image
    for c in range(cases.NUM_CLASSES):
        s = dets.scores[(dets.labels == c) & (torch.arange(dets.labels.shape[1])[None] < dets.count[:, None])]
        assert s.unique().numel() == s.numel() and (s > 0).all()


@pytest.mark.parametrize("case", list(cases.CASES))
def test_eval_map_lists_reproduces_eval_map(golden, case):
    thr, ranged = cases.CASES[case]
    det_results, annotations = cases.golden_lists(golden)
    mean_ap, results = ev.eval_map_lists(det_results, annotations, scale_ranges=cases.scale_ranges(golden, ranged), iou_thr=thr)
    ref_ap = golden[case + "_ap"]
    got = np.stack([np.reshape(r["ap"], -1) for r in results], 1)
    assert got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref_ap.astype(np.float64))
    assert np.all(err <= np.spacing(ref_ap)), (got, ref_ap)                      # one float32 spacing of the reference's value
    assert np.array_equal(np.stack([np.reshape(r["num_gts"], -1) for r in results], 1), golden[case + "_num_gts"])
    assert np.array_equal([r["num_dets"] for r in results], golden[case + "_num_dets"])
    S = ref_ap.shape[0]
    assert np.array_equal(np.concatenate([np.reshape(r["recall"], (S, -1)) for r in results], 1), golden[case + "_recall"])
    assert np.array_equal(np.concatenate([np.reshape(r["precision"], (S, -1)) for r in results], 1), golden[case + "_precision"])
    ref_map = golden[case + "_mean_ap"]
    assert isinstance(mean_ap, list) == ranged
    assert np.all(np.abs(np.reshape(mean_ap, -1) - ref_map) <= 1e-6 * np.abs(ref_map))


def test_eval_map_lists_takes_what_detections_as_lists_produces(golden):
    dets, gts, ignore = cases.golden_padded(golden)
    det_results, annotations = cases.golden_lists(golden)
    want = ev.eval_map_lists(det_results, annotations, iou_thr=0.5)
    got = ev.eval_map_lists(dets.as_lists(), annotations, iou_thr=0.5, num_classes=cases.NUM_CLASSES)
    assert got[0] == want[0] and [r["ap"] for r in got[1]] == [r["ap"] for r in want[1]]
    with pytest.raises(PswinError):
        ev.eval_map_lists(dets.as_lists(), annotations)


# ---- the padded form against the list form ------------------------------------------------------------------------------------------------
def _lists_of(dets, gts, ignore, C):
    """the reference's form of a padded batch: regular boxes first, ignored ones behind them, whatever their positions were"""
    det_results, annotations, rows = [], [], []
    for b in range(dets.labels.shape[0]):
        n, m = int(dets.count[b]), int(gts.count[b])
        d = torch.cat([dets.boxes[b, :n], dets.scores[b, :n, None]], 1).numpy()
        lab = dets.labels[b, :n].numpy()
        det_results.append([d[lab == c] for c in range(C)])
        rows.append(np.concatenate([np.nonzero(lab == c)[0] for c in range(C)]) if n else np.zeros(0, np.int64))
        ig = ignore[b, :m].numpy()
        bx, lb = gts.boxes[b, :m].numpy(), gts.labels[b, :m].numpy()
        annotations.append(dict(bboxes=bx[~ig], labels=lb[~ig], bboxes_ignore=bx[ig], labels_ignore=lb[ig]))
    return det_results, annotations, rows


@pytest.mark.parametrize("Gmax", [5, 65])
@pytest.mark.parametrize("ranged", [False, True])
def test_match_pairs_on_the_padded_form_equals_the_list_form(Gmax, ranged):
    """Ignore flags in arbitrary positions, also in front of regular boxes that tie with them, and repeated scores: the list form moves the
    ignored boxes behind the regular ones and reorders the detections class by class, and the marks must not notice."""
    C, thrs = 4, (0.5, 0.75, 0.95)
    area_ranges = [(0.0, 1024.0), (1024.0, 1e10)] if ranged else None
    dets, gts, ignore = cases.pair_case(Gmax, K=40)
    tie = [(gts.boxes[b, i] == gts.boxes[b, j]).all() and ignore[b, j] and not ignore[b, i] and gts.labels[b, i] == gts.labels[b, j]
           for b in range(3) for i in range(int(gts.count[b])) for j in range(i)]
    assert any(tie)                                                       # an ignored box in front of an identical regular one
    marks = ev.match_pairs(ev.box_iou_pairs(dets, gts), dets, gts, ignore, thrs, area_ranges, ev.box_areas(dets.boxes), ev.box_areas(gts.boxes))
    det_results, annotations, rows = _lists_of(dets, gts, ignore, C)
    d2, g2, i2, _ = ev.padded_from_lists(det_results, annotations)
    marks2 = ev.match_pairs(ev.box_iou_pairs(d2, g2), d2, g2, i2, thrs, area_ranges, ev.box_areas(d2.boxes), ev.box_areas(g2.boxes))
    assert (marks == ev.MARK_TP).any() and (marks == ev.MARK_FP).any() and (marks[:, :, 1:] == ev.MARK_IGNORED).any()
    for b in range(3):
        n = int(dets.count[b])
        assert torch.equal(marks[:, :, b, :n][:, :, torch.as_tensor(rows[b], dtype=torch.long)], marks2[:, :, b, :n]), b
        assert not marks[:, :, b, n:].any()


# ---- mask IoU by hand ---------------------------------------------------------------------------------------------------------------------
def test_mask_iou_by_hand():
    H, W = 8, 16
    d, g = torch.zeros(1, 6, H, W, dtype=torch.uint8), torch.zeros(1, 6, H, W, dtype=torch.uint8)
    d[0, 0, :4], g[0, 0, 4:] = 1, 1                      # disjoint
    d[0, 1, 2:6, 3:9], g[0, 1, 2:6, 3:9] = 1, 1           # identical
    d[0, 2, :4, :8], g[0, 2, :8, :8] = 1, 1               # nested, exactly 1 / 2
    d[0, 3, :6, :8], g[0, 3, :8, :8] = 1, 1               # nested, exactly 3 / 4
    #      4: both empty
    d[0, 5, :2], g[0, 5, :2] = 200, 3                     # bytes other than 1 count as set
    lab = torch.arange(6)[None]
    dets = Detections(torch.zeros(1, 6, 4), torch.ones(1, 6), lab, torch.tensor([6], dtype=torch.int32), None, masks=d)
    gts = PaddedTargets(torch.zeros(1, 6, 4), lab.clone(), torch.tensor([6], dtype=torch.int32), masks=g)
    iou = ev.mask_iou_pairs(dets, gts)
    assert iou.dtype == torch.float32
    assert torch.equal(iou[0].diagonal(), torch.tensor([0.0, 1.0, 0.5, 0.75, 0.0, 1.0]))
    assert (iou[0][~torch.eye(6, dtype=torch.bool)] == -1).all()          # other classes
    da, ga = ev.mask_areas(dets, gts)
    assert da[0].tolist() == [64, 24, 32, 48, 0, 32] and ga[0].tolist() == [64, 24, 64, 64, 0, 32]
    gts.count[0] = 3
    assert torch.equal(ev.mask_iou_pairs(dets, gts)[0].diagonal(), torch.tensor([0.0, 1.0, 0.5, -1.0, -1.0, -1.0]))
    assert ev.mask_areas(dets, gts)[1][0].tolist() == [64, 24, 64, 0, 0, 0]


def test_average_precision_sorted_by_hand():
    m = torch.tensor([1, 2, 0, 1, 2, 2, 1], dtype=torch.uint8)
    # tp 1 1 1 2 2 2 3, fp 0 1 1 1 2 3 3: precision 1, 1/2, 1/2, 2/3, 1/2, 2/5, 1/2; monotone: 1, 2/3, 1/2 at the three recall steps
    want = np.float32((1 / 4 - 0) * 1.0 + (2 / 4 - 1 / 4) * np.float64(np.float32(2) / np.float32(3)) + (3 / 4 - 2 / 4) * 0.5)
    got = ev.average_precision_sorted(m, 4)
    assert got.dtype == torch.float32 and abs(float(got) - float(want)) <= np.spacing(want)
    assert float(ev.average_precision_sorted(m, 0)) == 0.0 and float(ev.average_precision_sorted(m[:0], 3)) == 0.0
    assert float(ev.average_precision_sorted(torch.full((5,), 2, dtype=torch.uint8), 3)) == 0.0
    assert float(ev.average_precision_sorted(torch.ones(5, dtype=torch.uint8), 5)) == 1.0


# ---- the accumulator on the CPU -----------------------------------------------------------------------------------------------------------
def _accumulate(golden, acc, batch=5):
    for lo in range(0, 12, batch):
        dets, gts, ignore = cases.golden_padded(golden, lo=lo, hi=lo + batch, pad_to=batch)
        acc.update(dets, gts, ignore)
    return acc


def test_accumulator_in_three_batches_equals_one_call_of_eval_map_lists(golden):
    rng = cases.scale_ranges(golden, True)
    acc = _accumulate(golden, ev.MapAccumulator(4, iou_thrs=(0.5, 0.75), scale_ranges=rng, capacity_images=15, max_per_img=16))
    assert int(acc.cursor) == 15                                       # 5 + 5 + (2 images and 3 of padding)
    out = acc.summarize()
    assert out["mean_ap"].shape == (2, 2) and out["ap"].shape == (2, 2, 4) and out["num_gts"].shape == (2, 4) and out["num_dets"].shape == (4,)
    det_results, annotations = cases.golden_lists(golden)
    for t, thr in enumerate((0.5, 0.75)):
        mean_ap, results = ev.eval_map_lists(det_results, annotations, scale_ranges=rng, iou_thr=thr)
        assert np.array_equal(out["ap"][t].numpy(), np.stack([r["ap"] for r in results], 1))
        assert np.array_equal(out["num_gts"].numpy(), np.stack([r["num_gts"] for r in results], 1))
        assert out["num_dets"].tolist() == [r["num_dets"] for r in results]
        assert np.allclose(out["mean_ap"][t].numpy(), mean_ap, rtol=1e-6, atol=0)
    plain = _accumulate(golden, ev.MapAccumulator(4, iou_thrs=(0.5,), capacity_images=15, max_per_img=16)).summarize()
    assert np.array_equal(plain["ap"][0, 0].numpy(), golden["thr50_ap"][0]) or \
        np.all(np.abs(plain["ap"][0, 0].numpy().astype(np.float64) - golden["thr50_ap"][0]) <= np.spacing(golden["thr50_ap"][0]))
    assert abs(float(plain["mean_ap"][0, 0]) - golden["thr50_mean_ap"][0]) <= 1e-6 * golden["thr50_mean_ap"][0]


def test_accumulator_takes_the_list_form_of_targets(golden):
    dets, gts, _ = cases.golden_padded(golden)
    a = ev.MapAccumulator(4, capacity_images=12, max_per_img=16)
    a.update(dets, gts)
    b = ev.MapAccumulator(4, capacity_images=12, max_per_img=16)
    b.update(dets, gts.as_lists())
    assert torch.equal(a.summarize()["ap"], b.summarize()["ap"])


def test_accumulator_overflow_raises_and_reset_clears(golden):
    acc = ev.MapAccumulator(4, capacity_images=10, max_per_img=16)
    _accumulate(golden, acc, batch=5)                                  # 15 image slots wanted
    assert int(acc.overflow) == 1
    with pytest.raises(PswinError):
        acc.summarize()
    acc.reset()
    assert int(acc.cursor) == 0 and int(acc.overflow) == 0 and not acc.num_gts.any() and not acc.rec_marks.any() and (acc.rec_label == 4).all()
    out = acc.summarize()
    assert not out["ap"].any() and not out["mean_ap"].any() and not out["num_dets"].any()
    dets, gts, ignore = cases.golden_padded(golden, lo=0, hi=10)
    acc.update(dets, gts, ignore)
    assert acc.summarize()["num_dets"].sum() == int(golden["in_det_count"][:10].sum())


def test_accumulator_rejects_what_it_cannot_score(golden):
    dets, gts, ignore = cases.golden_padded(golden)
    with pytest.raises(PswinError):
        ev.MapAccumulator(4, max_per_img=8).update(dets, gts)           # K of the detections
    with pytest.raises(PswinError):
        ev.MapAccumulator(4, max_per_img=16, iou="segm").update(dets, gts)      # no masks
    with pytest.raises(PswinError):
        ev.MapAccumulator(4, max_per_img=16).update(dets, gts, ignore[:, :2])
    with pytest.raises(PswinError):
        ev.MapAccumulator(4, iou="mask")
    with pytest.raises(PswinError):
        ev.MapAccumulator(4, iou_thrs=(0.0,))
    with pytest.raises(PswinError):
        ev.MapAccumulator(4, capacity_images=1 << 20, max_per_img=100)


def test_segm_accumulator_on_the_cpu_scores_identical_masks_as_hits():
    dets, gts = cases.segm_case(2, 8, 5, 16, 16)
    acc = ev.MapAccumulator(3, iou_thrs=(0.5, 1.0), capacity_images=2, max_per_img=8, iou="segm")
    marks = acc.update(dets, gts)
    iou = ev.mask_iou_pairs(dets, gts)
    assert (iou == 1).any() and (marks[1] == ev.MARK_TP).any()          # a true positive at threshold 1.0: an identical mask
    assert acc.summarize()["ap"].shape == (2, 1, 3)


# ---- the entry points' argument checks (no GPU needed: every check comes before the launch) --------------------------------------------------
def test_the_chunk_constant_is_the_library_s():
    from panoswintransformerobjectdetection_amd import _lib
    assert _lib.load().pswin_ap_segments_chunk() == ev.AP_CHUNK


def test_argument_errors_of_the_evaluation_entry_points_without_a_gpu():
    from panoswintransformerobjectdetection_amd import _lib
    lib = _lib.load()
    ERR = -1
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15
    thr = ctypes.cast((ctypes.c_float * 2)(0.5, 0.75), ctypes.c_void_p)
    bad_thr = ctypes.cast((ctypes.c_float * 2)(0.5, 1.5), ctypes.c_void_p)
    rng = ctypes.cast((ctypes.c_float * 4)(0.0, 64.0, 64.0, 1e10), ctypes.c_void_p)
    bad_rng = ctypes.cast((ctypes.c_float * 4)(0.0, 64.0, 64.0, 1.0), ctypes.c_void_p)
    # box IoU: every buffer but the two areas is required; shapes; alignment
    ok = [p16, p16, p16, p16, p16, p16, 8, 100, 32, p16, p16, p16, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (9, None), (6, 0), (6, 65536), (7, 0), (7, 1025), (8, 0),
                 (8, 1 << 22), (0, p16 + 4), (3, p16 + 8), (1, p16 + 4), (2, p16 + 2), (9, p16 + 2), (10, p16 + 1)):
        bad = list(ok); bad[i] = v
        assert lib.pswin_box_iou_pairs(*bad) == ERR, (i, v)
    # mask IoU: H W a multiple of 16, the workspace and both areas required
    assert lib.pswin_mask_iou_workspace(8, 100, 32) == 8 * 132 * 4
    for shape in ((0, 100, 32), (8, 0, 32), (8, 100, 0), (8, 1025, 32), (65536, 100, 32)):
        assert lib.pswin_mask_iou_workspace(*shape) == ERR, shape
    ok = [p16, p16, p16, p16, p16, p16, 2, 8, 5, 32, 48, p16, p16, p16, p16, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (11, None), (12, None), (13, None), (14, None), (6, 0), (7, 0),
                 (8, 0), (9, 0), (10, 0), (0, p16 + 8), (3, p16 + 4), (14, p16 + 2)):
        bad = list(ok); bad[i] = v
        assert lib.pswin_mask_iou_pairs(*bad) == ERR, (i, v)
    bad = list(ok); bad[9], bad[10] = 5, 5
    assert lib.pswin_mask_iou_pairs(*bad) == ERR                       # 25 pixels: no multiple of 16
    bad = list(ok); bad[9], bad[10] = 3, 8
    assert lib.pswin_mask_iou_pairs(*bad) == ERR                       # 24 pixels: a multiple of 8 only
    # match: buffers, T and S limits, thresholds in (0, 1], ordered ranges, ranges required when S > 1
    ok = [p16, p16, p16, p16, p16, p16, None, p16, p16, thr, 2, rng, 2, 8, 100, 32, 80, 5000, p16, p16, p16, p16, p16, p16, p16, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (7, None), (8, None), (9, None), (18, None), (19, None),
                 (20, None), (21, None), (22, None), (23, None), (24, None), (10, 0), (10, 17), (12, 0), (12, 9), (11, None), (13, 0), (14, 0),
                 (14, 1025), (15, 0), (16, 0), (17, 0), (9, bad_thr), (11, bad_rng), (0, p16 + 2), (2, p16 + 4), (18, p16 + 2), (20, p16 + 1),
                 (23, p16 + 2)):
        bad = list(ok); bad[i] = v
        assert lib.pswin_eval_match(*bad) == ERR, (i, v)
    # AP: buffers, limits, at most 2^24 records
    ok = [p16, p16, p16, 2, 2, 80, 500000, p16, None]
    for i, v in ((0, None), (1, None), (2, None), (7, None), (3, 0), (3, 17), (4, 0), (4, 9), (5, 0), (6, 0), (6, (1 << 24) + 1), (1, p16 + 2),
                 (7, p16 + 1)):
        bad = list(ok); bad[i] = v
        assert lib.pswin_ap_segments(*bad) == ERR, (i, v)
