"""pswin_sample_ranks / pswin_rpn_targets / pswin_roi_targets / pswin_mask_targets on the MI355X against their definitions on CPU tensors
(detector.sample_ranks, rpn_targets, roi_targets, mask_targets).

SELECTION is exact: both sides order the candidates by (float32 composed key, index), so the ranks must be torch.equal whatever the keys
tie like.  Integer, bool and gathered-box outputs of the two stages are exact for the same reason.  reg_t has a logf in it, the one
operation that may differ from the host: with the float64 definition as the truth, the kernel's largest error may be at most 4 x the
float32 CPU definition's own error plus one float32 ulp of the largest target (the rule of tests/test_detect_post_gpu.py).  MASK TARGETS
are thresholded bilinear samples: equal to the definition outside the points whose float64 value lies within 1e-4 of 0.5, a set that is
asserted to hold at most 1e-3 of the points."""
import numpy as np
import pytest
import torch

import _targets_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STDS = (0.1, 0.1, 0.2, 0.2)


def _rows():
    from panoswintransformerobjectdetection_amd import _lib
    return int(_lib.load().pswin_sample_rows_per_workgroup())


def _cpu(ts):
    return [t.cpu() for t in ts]


def _flat(out):
    return list(out["rpn"]) + list(out["roi"]) + [out["mask"]]


def _bits(t):
    return t.contiguous().view(torch.uint8)


# ---- selection ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pos,n_neg", [(1, 1), (128, 256), (128, 512)])
@pytest.mark.parametrize("n_index", range(5))
def test_sample_ranks_equal_the_definition(n_index, n_pos, n_neg):
    from panoswintransformerobjectdetection_amd import detector as det, ops
    R, k = _rows(), max(n_pos, n_neg)
    N = [k, R - 1, R, R + 1, 4 * R + 1][n_index]                      # the last one: three levels of the tree
    assert k <= N
    B, gen = 3, torch.Generator().manual_seed(100 * n_index + n_neg)
    for pop in tc.POPULATIONS:
        for kind in tc.KEY_KINDS:
            gt_inds, key = tc.population(pop, B, N, gen), tc.keys(kind, B, N, gen)
            if kind == "distinct":
                assert tc.composed_keys_distinct(gt_inds, key)
            want = det.sample_ranks(gt_inds, key, n_pos, n_neg)
            got = _cpu(ops.sample_ranks(gt_inds.to(DEV), key.to(DEV), n_pos, n_neg))
            for name, g, w in zip(("pos_rank", "neg_rank"), got, want):
                assert g.dtype == torch.long and torch.equal(g, w), (N, pop, kind, name, int((g != w).sum()))


# ---- the two stages ------------------------------------------------------------------------------------------------------------------------
def _reg_errors(got, want32, truth):
    ek, e32 = float((got.double() - truth).abs().max()), float((want32.double() - truth).abs().max())
    bound = 4 * e32 + float(np.spacing(np.float32(truth.abs().max())))
    print(f"reg_t errors vs float64: kernel {ek:.3e} / f32 definition {e32:.3e} (bound {bound:.3e})")
    assert ek <= bound, (ek, e32)


@pytest.mark.parametrize("Gmax", [1, 16])
def test_rpn_targets_equal_the_definition(Gmax):
    from panoswintransformerobjectdetection_amd import detector as det, ops
    n_pos_max, n_tot = 128, 256
    gt_inds, key, cand, gt, _, count = tc.stage_case(Gmax, _rows() + 52, False, seed=3)
    anchors = cand[0]
    assert count.tolist() == [Gmax, 0, 1]
    want = det.rpn_targets(gt_inds, key, anchors, gt, n_pos_max, n_tot)
    truth = det.rpn_targets(gt_inds, key, anchors.double(), gt.double(), n_pos_max, n_tot)
    assert all(torch.equal(a, b) for a, b in zip(want[:3], truth[:3])) and bool(want[2][0].any())
    got = _cpu(ops.rpn_targets(gt_inds.to(DEV), key.to(DEV), anchors.to(DEV), gt.to(DEV), n_pos_max, n_tot))
    for name, g, w in zip(("idx", "valid", "pos_valid"), got, want):
        assert g.dtype == w.dtype and torch.equal(g, w), name
    assert not got[3][~want[2]].any()
    _reg_errors(got[3], want[3], truth[3])


@pytest.mark.parametrize("Gmax", [1, 16])
def test_roi_targets_equal_the_definition(Gmax):
    from panoswintransformerobjectdetection_amd import detector as det, ops
    n_pos_max, n_tot, C = 128, 512, 80
    gt_inds, key, cand, gt, labels, count = tc.stage_case(Gmax, 1000, True, seed=4)                 # lead_gt = Gmax
    assert count.tolist() == [Gmax, 0, 1] and bool((gt_inds[1, :Gmax] == -1).all())
    want = det.roi_targets(gt_inds, key, cand, gt, labels, C, n_pos_max, n_tot, STDS)
    truth = det.roi_targets(gt_inds, key, cand.double(), gt.double(), labels, C, n_pos_max, n_tot, STDS)
    assert torch.equal(want[1], truth[1]) and torch.equal(want[3], truth[3]) and torch.equal(want[4], truth[4])
    got = _cpu(ops.roi_targets(gt_inds.to(DEV), key.to(DEV), cand.to(DEV), gt.to(DEV), labels.to(DEV), C, n_pos_max, n_tot, STDS))
    for i, name in ((0, "rois"), (1, "labels"), (3, "pos_valid"), (4, "gt_idx")):
        assert got[i].dtype == want[i].dtype and torch.equal(got[i], want[i]), name
    pad = torch.tensor(tc.SENTINEL)
    assert not bool((got[0] == pad).all(-1).any()) and not bool((got[1] == tc.SENTINEL_LABEL).any())
    assert not got[2][~want[3]].any()
    _reg_errors(got[2], want[2], truth[2])


# ---- mask targets --------------------------------------------------------------------------------------------------------------------------
def _check_masks(got, masks, rois, gt_idx, pos_valid, where):
    from panoswintransformerobjectdetection_amd import detector as det
    near, truth = tc.near_threshold(masks, rois, gt_idx, pos_valid)
    share = float(near.float().mean())
    want = det.mask_targets(masks, rois, gt_idx, pos_valid, 28)
    print(f"{where}: near-threshold share {share:.2e}; kernel differs from the f32 definition at {int((got != want).sum())} points, all near")
    assert share <= tc.NEAR_SHARE, share
    assert torch.equal(want[~near], truth[~near])
    assert got.dtype == torch.float32 and got.shape == want.shape and set(got.unique().tolist()) <= {0.0, 1.0}
    assert torch.equal(got[~near], want[~near]), int((got != want)[~near].sum())
    assert not got.view(-1, 28 * 28)[~pos_valid.reshape(-1)].any()


@pytest.mark.parametrize("H,W", [(37, 53), (128, 256)])
def test_mask_targets_equal_the_definition_outside_the_near_threshold_set(H, W):
    from panoswintransformerobjectdetection_amd import ops
    masks, rois, gt_idx, pos_valid, count = tc.mask_case(H, W)
    assert count.tolist() == [9, 1] and bool(masks[0, 9:].all()) and bool(masks[1, 1:].all())
    got = ops.mask_targets(masks.to(DEV), rois.to(DEV), gt_idx.to(DEV), pos_valid.to(DEV), 28).cpu()
    _check_masks(got, masks, rois, gt_idx, pos_valid, f"{H} x {W}")


# ---- one capture, replayed ------------------------------------------------------------------------------------------------------------------
def _replay_set(Gmax, counts, H, W, n_props, seed):
    """annotations, proposals, anchors' stand-ins, keys and bitmaps of one batch (CPU tensors)"""
    import _assign_cases as ac
    from panoswintransformerobjectdetection_amd.detector import synthetic_targets
    B = len(counts)
    tg = next(t for t in (synthetic_targets(B, H, W, "cpu", seed=s) for s in range(seed, seed + 400))
              if all(i["boxes"].shape[0] >= n for i, n in zip(t, counts)))
    gt, labels = torch.tensor(tc.SENTINEL).repeat(B, Gmax, 1), torch.full((B, Gmax), tc.SENTINEL_LABEL, dtype=torch.long)
    masks = torch.ones(B, Gmax, H, W, dtype=torch.uint8)
    for b, n in enumerate(counts):
        gt[b, :n], labels[b, :n], masks[b, :n] = tg[b]["boxes"][:n], tg[b]["labels"][:n], tg[b]["masks"][:n]
    big = max((tg[b]["boxes"][:n] for b, n in enumerate(counts)), key=len).numpy()
    props = torch.stack([torch.from_numpy(ac.candidates(n_props, tg[b]["boxes"][:n].numpy() if n else big, seed + b)) for b, n in enumerate(counts)])
    gen = torch.Generator().manual_seed(seed)
    return dict(gt=gt, labels=labels, masks=masks, count=torch.tensor(counts, dtype=torch.int32), props=props,
                key_rpn=tc.keys("distinct", B, n_props, gen), key_roi=tc.keys("eighths", B, Gmax + n_props, gen))


def test_one_capture_of_the_three_ops_follows_the_buffers_across_replays():
    """Assign, sample, encode and mask targets of both stages are captured ONCE; before each replay other boxes, counts (9 -> 1 -> 0 for
    image 0), bitmaps and keys are copied into the same buffers.  Every replay must equal the definitions for THAT replay's buffers, and
    a second replay on the same buffers must repeat the first bit for bit."""
    from panoswintransformerobjectdetection_amd import detector as det, ops
    from panoswintransformerobjectdetection_amd.graph import GraphedCallable
    Gmax, H, W, C, P, n_tot = 9, 128, 256, 80, 32, 128
    n_props = _rows() + 300
    sets = [_replay_set(Gmax, c, H, W, n_props, 40 + 50 * i) for i, c in enumerate([(9, 3), (1, 9), (0, 5)])]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        buf = {k: torch.zeros_like(v, device=DEV) for k, v in sets[0].items()}
        out = {}

        def step():
            # the RPN stage on the proposals of image 0 standing in for the shared anchors, then the RoI stage with the gt rows leading
            anchors = buf["props"][0]
            inds = ops.max_iou_assign_batch(anchors, buf["gt"], buf["count"], 0.7, 0.3, 0.3, True)[0]
            out["rpn"] = ops.rpn_targets(inds, buf["key_rpn"], anchors, buf["gt"], P, n_tot)
            cand = torch.cat([buf["gt"], buf["props"]], 1)
            inds = ops.max_iou_assign_batch(cand, buf["gt"], buf["count"], 0.5, 0.5, 0.5, True, lead_gt=Gmax)[0]
            out["roi"] = ops.roi_targets(inds, buf["key_roi"], cand, buf["gt"], buf["labels"], C, P, n_tot, STDS)
            rois, _, _, pos_valid, gt_idx = out["roi"]
            out["mask"] = ops.mask_targets(buf["masks"], rois[:, :P], gt_idx, pos_valid, 28)
            return out["mask"]

        for k, v in sets[2].items():
            buf[k].copy_(v)                                            # captured on the LAST set, replayed on the others first
        g = GraphedCallable(step, warmup=2, stream=side, parameters=[])
        for replay, s in enumerate(sets):
            for k, v in s.items():
                buf[k].copy_(v)
            g()
            side.synchronize()
            got = {k: _cpu(v) if isinstance(v, tuple) else v.cpu() for k, v in out.items()}
            g()
            side.synchronize()
            for a, c in zip(_flat(got), _flat({k: _cpu(v) if isinstance(v, tuple) else v.cpu() for k, v in out.items()})):
                assert torch.equal(_bits(a), _bits(c)), replay
            anchors = s["props"][0]
            inds = det.max_iou_assign_batch(anchors, s["gt"], s["count"], 0.7, 0.3, 0.3, True)[0]
            want = det.rpn_targets(inds, s["key_rpn"], anchors, s["gt"], P, n_tot)
            truth = det.rpn_targets(inds, s["key_rpn"], anchors.double(), s["gt"].double(), P, n_tot)
            for i in range(3):
                assert torch.equal(got["rpn"][i], want[i]), (replay, "rpn", i)
            _reg_errors(got["rpn"][3], want[3], truth[3])
            cand = torch.cat([s["gt"], s["props"]], 1)
            inds = det.max_iou_assign_batch(cand, s["gt"], s["count"], 0.5, 0.5, 0.5, True, lead_gt=Gmax)[0]
            want = det.roi_targets(inds, s["key_roi"], cand, s["gt"], s["labels"], C, P, n_tot, STDS)
            truth = det.roi_targets(inds, s["key_roi"], cand.double(), s["gt"].double(), s["labels"], C, P, n_tot, STDS)
            for i in (0, 1, 3, 4):
                assert torch.equal(got["roi"][i], want[i]), (replay, "roi", i)
            _reg_errors(got["roi"][2], want[2], truth[2])
            assert not bool((got["roi"][0] == torch.tensor(tc.SENTINEL)).all(-1).any()), replay
            if s["count"][0] > 0:
                assert bool(want[3][0].any()), replay                  # image 0 has positives whenever it has boxes
            _check_masks(got["mask"], s["masks"], want[0][:, :P], want[4], want[3], f"replay {replay}")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
