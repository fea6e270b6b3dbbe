"""Proposal recall on the CPU: the definitions of panoswintransformerobjectdetection_amd/evaluation.py against the reference's own results
(tests/golden/recall.npz, tools/gen_recall_golden.py: _recalls and bbox_overlaps of mmdet/core/evaluation), against an independent numpy
restatement on random cases full of ties, the planted defects that the cases must expose, the accumulator, the RPN-only test path of the
detector and the argument checks of the entry point.  The kernel itself: tests/test_recall_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import _recall_cases as cases
import _roi_ref
from panoswintransformerobjectdetection_amd import detector as det
from panoswintransformerobjectdetection_amd import evaluation as ev
from panoswintransformerobjectdetection_amd._lib import PswinError


@pytest.fixture(scope="module")
def golden():
    return cases.load_golden()


# ---- the definitions against the reference ------------------------------------------------------------------------------------------------
def test_rounds_reproduce_the_reference_bit_for_bit(golden):
    props, gts, ignore = cases.golden_padded(golden)
    nums = golden["proposal_nums"].tolist()
    rounds = ev.proposal_round_ious(props, gts, nums, ignore)
    assert rounds.dtype == torch.float32 and tuple(rounds.shape) == (len(nums), 12, 8)
    for k in range(len(nums)):
        for b in range(12):
            assert cases.same_bits(rounds[k, b].numpy(), golden["ref_rounds"][k, b]), (nums[k], b, rounds[k, b], golden["ref_rounds"][k, b])


def test_recalls_and_ar_reproduce_the_reference(golden):
    props, gts, ignore = cases.golden_padded(golden)
    rounds = ev.proposal_round_ious(props, gts, golden["proposal_nums"].tolist(), ignore)
    hits, num_gts = ev.recall_hits(rounds, golden["iou_thrs"])
    assert hits.dtype == torch.int64 and isinstance(num_gts, int) and num_gts == int((golden["in_gt_count"] - golden["in_gt_ignore"].sum(1)).sum())
    recalls = hits.numpy() / float(num_gts)
    assert (recalls == golden["ref_recalls"]).all()
    assert (recalls.mean(axis=1) == golden["ref_ar"]).all()


def test_eval_recalls_lists_reproduces_the_reference(golden):
    gts, proposals = cases.golden_lists(golden)
    got = ev.eval_recalls_lists(gts, proposals, golden["proposal_nums"].tolist(), golden["iou_thrs"])
    assert got.dtype == np.float64 and (got == golden["ref_recalls"]).all()
    one = ev.eval_recalls_lists(gts, [p[:, :4][np.argsort(-p[:, 4], kind="stable")] for p in proposals], (3,), 0.5)       # (k, 4): taken in their order
    assert one.shape == (1, 1) and one[0, 0] == golden["ref_recalls"][1, 0]
    assert np.isnan(ev.eval_recalls_lists([None, np.zeros((0, 4))], [np.zeros((2, 5)), np.zeros((0, 5))], (1, 2), 0.5)).all()


def test_the_fixture_holds_the_cases_it_promises(golden):
    props, gts, ignore = cases.golden_padded(golden)
    gc, pc = golden["in_gt_count"], golden["in_prop_count"]
    assert (gc == 0).any() and (pc == 0).any() and ((gc > pc) & (pc > 0)).any() and ignore.any()
    assert golden["proposal_nums"].tolist() == [1, 3, 10, 40, 100] and golden["proposal_nums"][-1] > pc.max()
    assert (golden["iou_thrs"] == np.arange(0.5, 0.96, 0.05)).all()
    best = np.concatenate([cases.iou_matrix(gts.boxes[b, :gc[b]], props.boxes[b, :pc[b]]).max(1) for b in (0, 1)])
    assert sorted(best.tolist()) == [float(np.float32(k) / np.float32(20)) for k in range(10, 20)]
    dup = cases.iou_matrix(gts.boxes[4, :gc[4]], gts.boxes[4, :gc[4]])
    assert (dup == 1).sum() > gc[4]                                               # duplicated boxes
    assert (cases.iou_matrix(gts.boxes[5, :gc[5]], props.boxes[5, :pc[5]]) == 0).all(1).any()          # a box disjoint from everything
    m = cases.iou_matrix(gts.boxes[6, :gc[6]], props.boxes[6, :pc[6]])
    assert len(set(m.argmax(1).tolist())) == 1                                    # rows that all prefer one column
    for p in golden["in_props"]:
        s = p[:, 4][p[:, 4] > 0]
        assert len(np.unique(s)) == len(s)


def test_the_double_comparison_at_the_exact_fractions():
    props, gts, _ = cases.batch([cases.fractions()])
    rounds = ev.proposal_round_ious(props, gts, (10,))
    assert sorted(rounds[0, 0].tolist()) == [float(np.float32(k) / np.float32(20)) for k in range(10, 20)]
    hits, num = ev.recall_hits(rounds, cases.DEFAULT_THRS)
    missed_at_own = [k for k, t in zip(range(10, 20), cases.DEFAULT_THRS) if not np.float64(np.float32(k) / np.float32(20)) >= t]
    assert missed_at_own == [13, 14, 15, 18, 19] and num == 10
    want = [sum(np.float64(np.float32(k) / np.float32(20)) >= t for k in range(10, 20)) for t in cases.DEFAULT_THRS]
    assert hits[0].tolist() == want and want != list(range(10, 0, -1))           # a float32 comparison would count 10, 9, .. 1


# ---- against the restatement --------------------------------------------------------------------------------------------------------------
def test_definitions_equal_the_restatement_on_random_cases_with_ties():
    rng = np.random.RandomState(7)
    nums, ties = (1, 2, 5, 9), 0
    for trial in range(40):
        images = []
        for _ in range(8):
            g, n = rng.randint(0, 7), rng.randint(0, 10)
            rows, cols = cases.random_image(rng, g, n, span=8, integer=trial % 4 != 3)
            images.append((rows, cols, [i for i in range(g) if rng.rand() < 0.15]))
            m = cases.iou_matrix(rows, cols)
            ties += g > 0 and n > 1 and bool((np.sort(m, 1)[:, -1] == np.sort(m, 1)[:, -2]).any())
        props, gts, ignore = cases.batch(images, R=10, G=7, junk=float("nan"))
        props.count[0] += 5 * (trial % 2)                                         # a count above R is clamped
        rounds = ev.proposal_round_ious(props, gts, nums, ignore)
        want, want_hits, want_num = cases.restated(props, gts, ignore, nums, cases.DEFAULT_THRS)
        assert cases.same_bits(rounds.numpy(), want), trial
        hits, num = ev.recall_hits(rounds, cases.DEFAULT_THRS)
        assert hits.tolist() == want_hits.tolist() and num == want_num
    assert ties > 100                                                             # 320 images: ties are the rule


@pytest.mark.parametrize("defect", cases.DEFECTS)
def test_each_planted_defect_changes_its_case(defect):
    props, gts, ignore = cases.defect_batch()
    b = cases.DEFECTS.index(defect)
    good, good_hits, _ = cases.restated(props, gts, ignore, cases.DEFECT_NUMS, cases.DEFAULT_THRS)
    assert cases.same_bits(ev.proposal_round_ious(props, gts, cases.DEFECT_NUMS, ignore).numpy(), good)
    bad, bad_hits, _ = cases.restated(props, gts, ignore, cases.DEFECT_NUMS, cases.DEFAULT_THRS, defect)
    if defect == "f32_threshold":
        assert cases.same_bits(bad, good) and bad_hits.tolist() != good_hits.tolist()
    else:
        assert not cases.same_bits(bad[:, b], good[:, b])


# ---- the accumulator ----------------------------------------------------------------------------------------------------------------------
def test_accumulator_in_batches_equals_one_shot(golden):
    nums, thrs = golden["proposal_nums"].tolist(), golden["iou_thrs"]
    results = []
    for step in (1, 5, 12):
        acc = ev.RecallAccumulator(nums, thrs)
        for at in range(0, 12, step):
            props, gts, ignore = cases.golden_padded(golden, range(at, min(at + step, 12)))
            rounds = acc.update(props, gts, ignore)
            assert tuple(rounds.shape) == (5, props.count.numel(), 8)
        results.append(acc.summarize())
    for r in results:
        assert (r["recalls"] == golden["ref_recalls"]).all() and (r["ar"] == golden["ref_ar"]).all() and r["num_gts"] == results[0]["num_gts"]
        assert r["recalls"].dtype == np.float64
    acc.reset()
    assert not acc.hits.any() and not acc.num_gts.any() and np.isnan(acc.summarize()["recalls"]).all()


def test_accumulator_takes_the_list_form_and_checks_its_arguments():
    props, gts, _ = cases.batch([cases.DEFECT_IMAGES["highest_col"], cases.DEFECT_IMAGES["by_box"]])
    acc = ev.RecallAccumulator((1, 3), 0.5)
    as_lists = [dict(boxes=gts.boxes[b, :n], labels=gts.labels[b, :n]) for b, n in enumerate(gts.count.tolist())]
    assert torch.equal(acc.update(props, as_lists), ev.RecallAccumulator((1, 3), 0.5).update(props, gts))
    default = ev.RecallAccumulator()
    assert default.proposal_nums == (100, 300, 1000) and (default.iou_thrs == np.arange(0.5, 0.96, 0.05)).all()
    for bad in (dict(proposal_nums=()), dict(proposal_nums=(0,)), dict(iou_thrs=(0.0,)), dict(iou_thrs=(1.5,)), dict(iou_thrs=[0.5] * 17),
                dict(proposal_nums=range(1, 10))):
        with pytest.raises(PswinError):
            ev.RecallAccumulator(**bad)
    with pytest.raises(PswinError):
        acc.update(det.Proposals(props.boxes.double(), props.scores, props.count), gts)
    with pytest.raises(PswinError):
        acc.update(props, gts, ignore=torch.zeros(2, 9, dtype=torch.bool))
    assert ev.recall_supported(8, 1000, 100, 3, 10) and ev.recall_supported(1, 2048, 512, 8, 16)
    assert not ev.recall_supported(8, 2049, 100, 3, 10) and not ev.recall_supported(8, 1000, 513, 3, 10)
    assert not ev.recall_supported(8, 1000, 100, 9, 10) and not ev.recall_supported(8, 1000, 100, 3, 17)


def test_the_entry_point_refuses_bad_arguments_without_a_gpu():
    """every check comes before the first launch: PSWIN_ERR_ARG (-1) on a CPU-only host"""
    from panoswintransformerobjectdetection_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15
    nums, thrs = (ctypes.c_int * 8)(*[1, 3, 10, 40, 100, 300, 1000, 2000]), (ctypes.c_double * 16)(*np.linspace(0.25, 1.0, 16))
    ok = [p, p, p, p, None, nums, 3, thrs, 10, 8, 1000, 100, p, p, p, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (5, None), (7, None), (12, None), (13, None), (14, None), (0, p + 4), (2, p + 8),
                 (1, p + 2), (12, p + 2), (13, p + 4), (14, p + 4), (6, 0), (6, 9), (8, 0), (8, 17), (9, 0), (9, 65536), (10, 0), (10, 2049),
                 (11, 0), (11, 513), (5, (ctypes.c_int * 3)(1, 0, 5)), (5, (ctypes.c_int * 3)(1, -3, 5)),
                 (7, (ctypes.c_double * 10)(*([0.5] * 9 + [0.0]))), (7, (ctypes.c_double * 10)(*([0.5] * 9 + [1.25]))),
                 (7, (ctypes.c_double * 10)(*([0.5] * 9 + [float("nan")])))):
        bad = list(ok)
        bad[i] = v
        assert lib.pswin_recall_match(*bad) == -1, (i, v)


# ---- the RPN-only test path ---------------------------------------------------------------------------------------------------------------
def _model(kind="mask", seed=0):
    torch.manual_seed(seed)
    cfg = dict(embed_dim=96, depths=[2, 2, 2, 2], num_heads=[3, 6, 12, 24], ape=True)
    if kind == "cascade":
        from panoswintransformerobjectdetection_amd.cascade import MiniCascadeRCNN
        m = MiniCascadeRCNN(cfg, num_classes=80).eval()
    else:
        m = det.MiniMaskRCNN(cfg, num_classes=80).eval()
    m.roi_align = _roi_ref.roi_align_batched          # CPU: the PyTorch statement stands in for the HIP operator
    return m


def _feats(B, H, W, seed=5):
    torch.manual_seed(seed)
    return [torch.randn(B, c, H // s, W // s) for c, s in zip((96, 192, 384, 768), (4, 8, 16, 32))]


def test_proposals_as_lists():
    boxes = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4)
    scores = torch.tensor([[0.9, 0.5, 0.1], [0.8, 0.7, 0.6]])
    out = det.Proposals(boxes, scores, torch.tensor([2, 7], dtype=torch.int32)).as_lists()
    assert [o.shape for o in out] == [(2, 5), (3, 5)] and all(isinstance(o, np.ndarray) and o.dtype == np.float32 for o in out)
    assert np.array_equal(out[0], np.concatenate([boxes[0, :2].numpy(), scores[0, :2, None].numpy()], 1))
    assert np.array_equal(out[1][:, 4], scores[1].numpy())
    assert det.Proposals(boxes, scores, torch.zeros(2, dtype=torch.int32)).as_lists()[1].shape == (0, 5)


def test_heads_propose_is_the_per_image_proposals_under_the_test_cfg():
    m = _model()
    B, H, W = 2, 64, 128
    feats = _feats(B, H, W)
    props = m.heads_propose(feats, (H, W))
    assert isinstance(props, det.Proposals) and props.boxes.dtype == torch.float32 and props.count.dtype == torch.int32
    with torch.no_grad():
        fpn = m.neck(feats)
        cls_all, reg_all = m._rpn_flatten(m.rpn(fpn))
    anchors = det.make_anchors([f.shape[2:] for f in fpn], m.STRIDES, "cpu")
    for b in range(B):
        bx, sc = m._proposals(cls_all[b], reg_all[b], anchors, m.test_cfg["rpn"], (H, W))
        assert torch.equal(props.boxes[b], bx) and torch.equal(props.scores[b], sc) and int(props.count[b]) == int((sc > -1e4).sum())
    sf = torch.tensor([[0.5, 0.25, 0.5, 0.25], [2.0, 4.0, 2.0, 4.0]])
    big = m.heads_propose(feats, (H, W), scale_factor=sf, rescale=True)
    assert torch.equal(big.boxes, props.boxes / sf[:, None, :]) and torch.equal(big.scores, props.scores) and torch.equal(big.count, props.count)
    assert torch.equal(m.heads_propose(feats, (H, W), scale_factor=sf).boxes, props.boxes)          # rescale=False: as they are
    with pytest.raises(PswinError):
        m.heads_propose(feats, (H, W), rescale=True)
    lists = props.as_lists()
    assert [len(l) for l in lists] == props.count.tolist() and all((l[:-1, 4] >= l[1:, 4]).all() for l in lists)


@pytest.mark.parametrize("kind", ["mask", "cascade"])
def test_heads_predict_starts_from_the_same_proposals(kind):
    m = _model(kind)
    B, H, W = 2, 64, 128
    feats = _feats(B, H, W)
    calls = []
    m.proposals = lambda *a: calls.append(a[3]) or det.proposals_batch(*a)
    props = m.heads_propose(feats, (H, W))
    out, raw = m.heads_predict(feats, (H, W), with_masks=False, return_raw=True)
    assert len(calls) == 2 and calls[0] is m.test_cfg["rpn"] and calls[1] is m.test_cfg["rpn"]
    rois = raw["rois"][0] if isinstance(raw["rois"], list) else raw["rois"]
    assert torch.equal(rois, props.boxes) and torch.equal(raw["roi_count"], props.count)
    assert isinstance(out, det.Detections) and bool((props.count > 0).all())


def test_heads_propose_scored_by_the_accumulator():
    """(the backbone needs a GPU: simple_test_rpn is in tests/test_recall_gpu.py)"""
    m = _model()
    B, H, W = 2, 64, 128
    props = m.heads_propose(_feats(B, H, W, seed=3), (H, W))
    targets = det.synthetic_targets(B, H, W, "cpu")
    acc = ev.RecallAccumulator((1, 10, 100, 1000), device="cpu")
    acc.update(props, targets)
    gts = [t["boxes"].numpy() for t in targets]
    want = ev.eval_recalls_lists(gts, props.as_lists(), (1, 10, 100, 1000), cases.DEFAULT_THRS)
    got = acc.summarize()
    assert (got["recalls"] == want).all() and got["num_gts"] == sum(len(g) for g in gts) > 0
