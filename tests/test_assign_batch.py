"""The target assigner for a padded batch (detector.max_iou_assign_batch, detector.PaddedTargets) on the CPU: the definition against
the reference's recorded results (tests/golden/max_iou_assign_batch.npz, written by tools/gen_assign_golden.py), the annotation buffers,
the argument checks of the C entry point, and MiniMaskRCNN.heads_loss on padded targets.  The kernels: tests/test_assign_batch_gpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from panoswintransformerobjectdetection_amd import detector as det
from panoswintransformerobjectdetection_amd._lib import PswinError

import _assign_cases as ac
import _roi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GMAX = 16
LIST_FORM_RTOL = 1e-6


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "max_iou_assign_batch.npz")))


def _padded(golden, Gmax=GMAX):
    gt = torch.zeros(3, Gmax, 4)
    gt[:, :golden["gt"].shape[1]] = torch.from_numpy(golden["gt"])
    return torch.from_numpy(golden["cand"]), gt, torch.from_numpy(golden["count"])


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_fixture_holds_the_cases_it_is_for(golden):
    assert golden["count"].tolist() == [0, 1, 9] and golden["cand"].shape == (3000, 4)
    assert [tuple(t) for t in golden["thresholds"].tolist()] == [(p, n, m, float(q)) for p, n, m, q in ac.THRESHOLDS]
    gt9 = golden["gt"][2]
    assert (gt9[0] == gt9[1]).all()                                                            # duplicate gt boxes
    assert (golden["max_overlaps"] == 0.5).any() and (golden["max_overlaps"] == 1.0).any()     # an exact threshold, a candidate equal to a gt
    assert ((gt9[:, 2] - gt9[:, 0]) * (gt9[:, 3] - gt9[:, 1]) == 0).any()                      # zero area
    assert (golden["gt_inds"][0] < 0).any() and (golden["gt_inds"][:, 2] > 0).any()


def test_definition_reproduces_the_reference_on_shared_candidates(golden):
    cand, gt, count = _padded(golden)
    for t, (pos, neg, min_pos, low) in enumerate(ac.THRESHOLDS):
        inds, best = det.max_iou_assign_batch(cand, gt, count, pos, neg, min_pos, low)
        assert inds.dtype == torch.long and tuple(inds.shape) == (3, cand.shape[0])
        assert torch.equal(inds, torch.from_numpy(golden["gt_inds"][t])), t
        assert _same_bits(best, torch.from_numpy(golden["max_overlaps"][t])), t


def test_definition_reproduces_the_reference_with_the_gt_rows_leading(golden):
    cand, gt, count = _padded(golden)
    G9 = golden["gt"].shape[1]
    cat = torch.cat([gt, cand[None].expand(3, -1, -1)], 1)                                     # add_gt_as_proposals on the padded rows
    for t, (pos, neg, min_pos, low) in enumerate(ac.THRESHOLDS):
        inds, best = det.max_iou_assign_batch(cat, gt, count, pos, neg, min_pos, low, lead_gt=GMAX)
        want_i, want_o = torch.from_numpy(golden["lead_gt_inds"][t]), torch.from_numpy(golden["lead_max_overlaps"][t])
        for b, G in enumerate(count.tolist()):
            assert torch.equal(inds[b, :G], want_i[b, :G]) and _same_bits(best[b, :G], want_o[b, :G]), (t, b)
            assert (inds[b, G:GMAX] == -1).all() and (best[b, G:GMAX] == -1).all(), (t, b)     # the padding rows
            assert torch.equal(inds[b, GMAX:], want_i[b, G9:]) and _same_bits(best[b, GMAX:], want_o[b, G9:]), (t, b)


def test_padded_targets_round_trip_reuse_their_buffers_and_refuse_too_many_boxes():
    tg = det.synthetic_targets(2, 32, 64, "cpu", seed=3)
    T = det.PaddedTargets.allocate(2, 12, "cpu", mask_hw=(32, 64))
    assert T.boxes.shape == (2, 12, 4) and T.labels.dtype == torch.long and T.count.dtype == torch.int32 and T.masks.dtype == torch.uint8
    ptrs = [t.data_ptr() for t in (T.boxes, T.labels, T.count, T.masks)]
    # lists of numpy arrays (what PanoTrainTransform returns), then lists of tensors with other counts
    T.copy_from([t["boxes"].numpy() for t in tg], [t["labels"].numpy() for t in tg], [t["masks"].numpy() for t in tg])
    for got, want in zip(T.as_lists(), tg):
        assert all(torch.equal(got[k], want[k]) for k in ("boxes", "labels", "masks"))
    assert T.count.tolist() == [t["boxes"].shape[0] for t in tg]
    tg2 = [{k: v[:1] for k, v in tg[1].items()}, {k: v[:0] for k, v in tg[0].items()}]
    T.copy_from([t["boxes"] for t in tg2], [t["labels"] for t in tg2], [t["masks"] for t in tg2])
    assert T.count.tolist() == [1, 0] and not T.boxes[0, 1:].any() and not T.boxes[1].any() and not T.masks[1].any() and not T.labels[1].any()
    for got, want in zip(T.as_lists(), tg2):
        assert all(torch.equal(got[k], want[k]) for k in ("boxes", "labels", "masks"))
    assert ptrs == [t.data_ptr() for t in (T.boxes, T.labels, T.count, T.masks)]
    with pytest.raises(PswinError):
        T.copy_from([np.zeros((13, 4), np.float32), np.zeros((0, 4), np.float32)], [np.zeros(13, np.int64), np.zeros(0, np.int64)],
                    [np.zeros((13, 32, 64), np.uint8), np.zeros((0, 32, 64), np.uint8)])
    F = det.PaddedTargets.allocate(2, 4, "cpu")                                                # Faster R-CNN: no masks
    F.copy_from([t["boxes"][:4] for t in tg], [t["labels"][:4] for t in tg])
    assert F.masks is None and set(F.as_lists()[0]) == {"boxes", "labels"}


def test_argument_errors_of_the_assigner_entry_point_without_a_gpu():
    """pswin_max_iou_assign validates before it touches the device: PSWIN_ERR_ARG (-1) on a CPU-only host."""
    from panoswintransformerobjectdetection_amd import _lib
    lib = _lib.load()
    ERR = -1
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15
    R = lib.pswin_max_iou_assign_rows_per_workgroup()
    assert R > 0 and R % 64 == 0
    assert lib.pswin_max_iou_assign_workspace(2, 3 * R + 37, 16) == 2 * 4 * 16 * 4          # one f32 per (image, workgroup, gt slot)
    assert lib.pswin_max_iou_assign_workspace(1, R, 256) == 256 * 4
    for B, N, G in ((0, 8, 4), (1, 0, 4), (1, 8, 0), (1, 8, 257)):
        assert lib.pswin_max_iou_assign_workspace(B, N, G) == ERR, (B, N, G)
    # cand, cand_per_image, gt, gt_count, B, N, Gmax, lead_gt, pos, neg, min_pos, match_low_quality, gt_inds, max_iou, workspace, stream
    ok = [p16, 0, p16, p16, 2, 100, 16, 0, 0.7, 0.3, 0.3, 1, p16, None, p16, None]
    for i, v in ((6, 0), (6, 257), (5, 0), (12, None), (7, 101), (4, 0), (0, None), (2, None), (3, None), (14, None), (7, -1), (1, 2),
                 (0, p16 + 4)):
        bad = list(ok)
        bad[i] = v
        assert lib.pswin_max_iou_assign(*bad) == ERR, (i, v)


# ------------------------------------------------------------------------------------------------------------------------
# MiniMaskRCNN.heads_loss on padded targets
# ------------------------------------------------------------------------------------------------------------------------
B, H, W = 2, 128, 256
SENTINEL = [1.25, 2.25, 250.25, 120.25]      # written into the padding rows: a box that would match half the image if it were ever read


def _keys(lead=0):
    """The samplers' random keys, the same in every call of a size; with lead > 0 the first `lead` keys of the RoI stage's calls (the
    gt rows of cat(gt, proposals), padding included) are the smallest, so a sampler that did not rank the padding last would draw it"""
    cache = {}

    def rand_like(t):
        n = t.numel()
        if n not in cache:
            k = torch.rand(n, generator=torch.Generator("cpu").manual_seed(1000 + n)) * 0.9 + 0.05
            if lead and n < 4000:                                                              # the RoI stage (the RPN ranks 8,184 anchors)
                k[:lead] = torch.arange(1, lead + 1) * 1e-4
            cache[n] = k
        return cache[n].view_as(t).to(t.dtype)
    return rand_like


@pytest.fixture(scope="module")
def heads():
    torch.manual_seed(0)
    m = det.MiniMaskRCNN(dict(embed_dim=96, depths=[2, 2, 2, 2], num_heads=[3, 6, 12, 24], ape=True), num_classes=80)
    m.roi_align = _roi_ref.roi_align_batched
    feats = [torch.randn(B, c, H // s, W // s) for c, s in zip((96, 192, 384, 768), (4, 8, 16, 32))]
    tg = next(t for t in (det.synthetic_targets(B, H, W, "cpu", seed=s) for s in range(100)) if min(i["boxes"].shape[0] for i in t) >= 7)
    return m, feats, tg


def _trim(tg, counts):
    return [{k: v[:n] for k, v in t.items()} for t, n in zip(tg, counts)]


def _pad(tg, Gmax, masks=True):
    T = det.PaddedTargets.allocate(B, Gmax, "cpu", mask_hw=(H, W) if masks else None)
    T.copy_from([t["boxes"] for t in tg], [t["labels"] for t in tg], [t["masks"] for t in tg] if masks else None)
    for b, n in enumerate(T.count.tolist()):
        T.boxes[b, n:] = torch.tensor(SENTINEL)
    return T


def _record_rois(m):
    seen = []

    def roi_align(feats, strides, rois, out_size, **kw):
        seen.append(rois.detach().clone())
        return _roi_ref.roi_align_batched(feats, strides, rois, out_size, **kw)
    m.roi_align = roi_align
    return seen


def test_heads_loss_on_padded_targets_equals_the_list_form_when_nothing_is_padded(heads):
    m, feats, tg = heads
    tg = _trim(tg, (5, 5))
    m.rand_like = _keys()
    try:
        with torch.no_grad():
            want = m.heads_loss(feats, tg, (H, W))
            got = m.heads_loss(feats, _pad(tg, 5), (H, W))
    finally:
        del m.rand_like
    assert set(got) == set(want) == {"loss_rpn_cls", "loss_rpn_bbox", "loss_cls", "loss_bbox", "loss_mask"}
    for k in want:
        assert torch.equal(got[k], want[k]), (k, float(got[k]), float(want[k]))


@pytest.mark.parametrize("masks", [True, False])
def test_heads_loss_with_padding_never_samples_a_padding_row(heads, masks):
    m, feats, tg = heads
    T = _pad(_trim(tg, (3, 7)), GMAX, masks)
    m.rand_like = _keys(lead=GMAX)
    seen = _record_rois(m)
    fs = [f.clone().requires_grad_(True) for f in feats]
    for p in m.parameters():
        p.grad = None
    try:
        losses = m.heads_loss(fs, T, (H, W))
        sum(losses.values()).backward()
    finally:
        del m.rand_like
        m.roi_align = _roi_ref.roi_align_batched
    want = {"loss_rpn_cls", "loss_rpn_bbox", "loss_cls", "loss_bbox"} | ({"loss_mask"} if masks else set())
    assert set(losses) == want and all(torch.isfinite(v) for v in losses.values())
    assert len(seen) == (2 if masks else 1) and seen[0].shape == (B, 512, 4)
    pad = torch.tensor(SENTINEL)
    for rois in seen:
        assert not (rois == pad).all(-1).any()
    # the valid gt rows hold the smallest keys, so they ARE drawn: the check above is not vacuous
    assert all((seen[0][b] == T.boxes[b, 0]).all(-1).any() for b in range(B))
    mask_ids = {id(p) for p in m.mask_head.parameters()}
    for k, p in m.named_parameters():
        if k.startswith("backbone."):
            continue
        if id(p) in mask_ids and not masks:
            assert p.grad is None, k
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert all(f.grad is not None and torch.isfinite(f.grad).all() for f in fs)


def test_list_targets_give_what_the_list_form_gave_before_it_was_padded_on_entry(heads):
    """Lists with ragged counts (3, 7) through both target stages against tests/golden/heads_list_form.npz, recorded by
    tools/gen_heads_list_golden.py on the last commit whose list form had a sampler, a box encoding and a mask sampling of its own.  The
    keys are all distinct (tests/_heads_list_case.py), so no outcome depends on a tie.  The RoIs handed to roi_align are copies of
    candidate rows: bit-equal.  The losses pass through float32 Linear layers and convolutions whose summation order belongs to the CPU
    and its BLAS.  Measured spread: on the recording machine that commit twice, and this code, give all five losses bit for bit; the
    same commit on a second machine (another CPU) gives four of them bit for bit and loss_cls 420.660187 against 420.660217, 7.25e-8
    relative (one float32 ulp), and this code gives there what that commit gives there.  LIST_FORM_RTOL = 1e-6 is 14 times that spread,
    8 float32 epsilons."""
    import _heads_list_case as case
    m, _, _ = heads
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "heads_list_form.npz")))
    assert tuple(gold["counts"]) == case.COUNTS
    assert gold["seeds"].tolist() == [case.SEED_RPN, case.SEED_FPN, case.SEED_PROPOSALS, case.SEED_KEYS]
    rpn_outs, fpn, proposals = case.inputs()
    assert torch.equal(torch.stack(proposals), torch.from_numpy(gold["proposals"]))
    got = case.run(m, case.targets(), rpn_outs, fpn, proposals)
    for k in ("rois_box", "rois_mask"):
        assert torch.equal(got[k], torch.from_numpy(gold[k])), k
    for k in ("loss_rpn_cls", "loss_rpn_bbox", "loss_cls", "loss_bbox", "loss_mask"):
        rel = abs(float(got[k]) - float(gold[k])) / abs(float(gold[k]))
        print(f"{k}: got {float(got[k]):.9g} recorded {float(gold[k]):.9g} relative difference {rel:.3g}")
        assert rel <= LIST_FORM_RTOL, (k, float(got[k]), float(gold[k]))
