"""COCO run-length encoding on the CPU: rle.py's vectorised definitions against the hand answers and against the plain-loop restatement of
pycocotools' C (tests/_rle_cases.py), the round trips, the container's layout and overflow contract, Detections.as_results against a
loop restatement of bbox2result + cls_segms + encode_mask_results, and the planted defects the cases must see.  Every comparison is
equality.  (pycocotools itself is not available: nothing here is pinned against it.)"""
import numpy as np
import pytest
import torch

import _rle_cases as rc
from panoswintransformerobjectdetection_amd import rle
from panoswintransformerobjectdetection_amd._lib import PswinError
from panoswintransformerobjectdetection_amd.detector import Detections

MASKS = rc.cpu_masks()


def test_hand_answers():
    for m, want in rc.HAND_ENCODE:
        got = rle.rle_encode(m)
        assert got.dtype == np.uint32 and got.tolist() == want
        assert rc.loop_encode(m) == want
    for cnts, want in rc.HAND_STRING:
        assert rle.rle_to_string(cnts) == want and rc.loop_to_string(cnts) == want
        assert rle.rle_from_string(want).tolist() == cnts and rc.loop_from_string(want) == cnts


def test_encode_equals_the_plain_loops_and_round_trips():
    for name, m in MASKS:
        got = rle.rle_encode(m).tolist()
        assert got == rc.loop_encode(m), name
        H, W = m.shape
        assert sum(got) == H * W, name
        assert np.array_equal(rle.rle_decode(got, H, W), (m != 0).astype(np.uint8)), name
        assert np.array_equal(rc.loop_decode(got, H, W), (m != 0).astype(np.uint8)), name
        assert rle.rle_area(got) == int((m != 0).sum()), name
        s = rle.rle_to_string(got)
        assert s == rc.loop_to_string(got), name
        assert rle.rle_from_string(s).tolist() == got, name
    assert rle.rle_encode(torch.from_numpy(MASKS[0][1])).tolist() == rc.loop_encode(MASKS[0][1])      # tensors are taken too


def test_the_checkerboard_has_the_most_runs():
    m = rc.patterns(7, 4)["checker1"]
    assert len(rle.rle_encode(m)) == 7 * 4 + 1


def test_strings_equal_the_plain_loops_and_round_trip():
    for cnts in rc.STRING_CASES:
        s = rle.rle_to_string(cnts)
        assert s == rc.loop_to_string(cnts), cnts
        assert rle.rle_from_string(s).tolist() == cnts and rc.loop_from_string(s) == cnts, cnts
        assert all(48 <= ch < 48 + 64 for ch in s)
    # the i > 2 rule: the run at i = 2 is written whole, those at i = 3 and 4 as differences
    assert rle.rle_to_string([5, 7, 5]) == b"575" and rle.rle_to_string([5, 7, 5, 7, 5]) == b"57500"
    assert rle.rle_to_string([5, 7, 5, 6, 9]) == rc.loop_to_string([5, 7, 5, 6, 9]) == b"575O4"
    with pytest.raises(PswinError):
        rle.rle_from_string(b"0T")                                                                       # ends inside a run
    with pytest.raises(PswinError):
        rle.rle_decode([1, 2], 2, 2)


def _batch(B=3, K=4, H=7, W=5, seed=3):
    g = np.random.default_rng(seed)
    masks = (g.random((B, K, H, W)) < 0.4).astype(np.uint8)
    masks[0, 1] = 0
    masks[1, 0] = 1
    return masks


def test_rle_masks_layout_counts_and_lists():
    masks = _batch()
    B, K, H, W = masks.shape
    count = torch.tensor([4, 0, 9], dtype=torch.int32)                          # full, none, above K (clamped)
    poisoned = masks.copy()
    poisoned[1] = 0xA5                                                          # rows past the count are not read
    enc = rle.encode_masks(torch.from_numpy(poisoned), count)
    truth = rc.batch_truth(masks, count.tolist())
    off = enc.offsets.tolist()
    assert off == np.concatenate([[0], np.cumsum([len(t) for t in truth])]).tolist()
    assert off[K] == off[2 * K]                                                 # flat across the image without detections
    assert enc.capacity == B * K * (30 * W + 1) and enc.runs.dtype == torch.uint32 and enc.offsets.dtype == torch.int64
    assert (enc.height, enc.width, enc.B, enc.K) == (H, W, B, K)
    for n, t in enumerate(truth):
        assert enc.runs[off[n]:off[n + 1]].tolist() == t, n
    lists = enc.to_lists()
    assert [len(l) for l in lists] == [4, 0, 4]
    for b in range(B):
        for k, d in enumerate(lists[b]):
            assert d == dict(size=[H, W], counts=rc.loop_to_string(truth[b * K + k]))
    # the [N, H, W] form: every mask is read, one "image"
    flat = rle.encode_masks(torch.from_numpy(masks.reshape(B * K, H, W)))
    assert [d["counts"] for d in flat.to_lists()[0]] == [rc.loop_to_string(rc.loop_encode(m)) for m in masks.reshape(B * K, H, W)]
    with pytest.raises(PswinError):
        rle.encode_masks(torch.from_numpy(masks.reshape(B * K, H, W)), count)   # count goes with the 4-d form
    with pytest.raises(PswinError):
        rle.encode_masks(torch.from_numpy(masks).float())


def test_overflow_contract_of_the_definition():
    masks = _batch()
    B, K, H, W = masks.shape
    count = torch.tensor([4, 2, 3], dtype=torch.int32)
    truth = rc.batch_truth(masks, count.tolist())
    total = sum(len(t) for t in truth)
    cap = total // 2
    out = rle.RleMasks(torch.empty(B * K + 1, dtype=torch.int64), torch.empty(total + 16, dtype=torch.uint32), H, W, capacity=cap)
    out.runs.view(torch.uint8).fill_(0xA5)
    enc = rle.encode_masks(torch.from_numpy(masks), count, out=out)
    assert enc is out and enc.capacity == cap
    off = enc.offsets.tolist()
    assert off[-1] == total and off == np.concatenate([[0], np.cumsum([len(t) for t in truth])]).tolist()
    whole = 0
    for n, t in enumerate(truth):
        if off[n + 1] <= cap:
            assert enc.runs[off[n]:off[n + 1]].tolist() == t
            whole += 1
    assert 0 < whole < B * K
    assert bool((enc.runs[cap:].view(torch.uint8) == 0xA5).all())               # nothing at or past capacity
    with pytest.raises(PswinError, match=f"{total}.*{cap}"):
        enc.to_lists()
    with pytest.raises(PswinError):
        rle.encode_masks(torch.from_numpy(masks), count, capacity=total + 17, out=out)   # more than the buffer holds
    assert rle.encode_masks(torch.from_numpy(masks), count, capacity=total).to_lists()


def _detections(with_masks=True, as_rle=False):
    masks = _batch(B=3, K=4, H=6, W=5, seed=5)
    g = torch.Generator().manual_seed(1)
    boxes, scores = torch.rand(3, 4, 4, generator=g) * 50, torch.rand(3, 4, generator=g)
    labels = torch.tensor([[2, 0, 2, 3], [0, 0, 0, 0], [3, 3, 1, 1]])           # class 1 of image 0 is empty; two rows of class 2
    count = torch.tensor([4, 0, 3], dtype=torch.int32)                          # image 1 has no detections
    m = torch.from_numpy(masks)
    det = Detections(boxes, scores, labels, count, torch.zeros(3, 4, dtype=torch.int32), m if with_masks and not as_rle else None,
                     rle.encode_masks(m, count) if as_rle else None)
    return det, masks


@pytest.mark.parametrize("as_rle", [False, True])
def test_as_results_equals_bbox2result_and_encoded_cls_segms(as_rle):
    det, masks = _detections(as_rle=as_rle)
    C = 5
    got = det.as_results(C)
    want = rc.results_truth(det.boxes.numpy(), det.scores.numpy(), det.labels.numpy(), det.count.tolist(), masks, C)
    assert len(got) == len(want) == 3
    for (gb, gs), (wb, ws) in zip(got, want):
        assert len(gb) == len(wb) == C and gs == ws
        for a, b in zip(gb, wb):
            assert a.dtype == np.float32 and a.shape == b.shape and np.array_equal(a, b)
    assert [len(s) for s in got[0][1]] == [1, 0, 2, 1, 0] and all(a.shape == (0, 5) for a in got[1][0])
    assert got[0][1][2][0]["counts"] == rc.loop_to_string(rc.loop_encode(masks[0, 0]))                 # row order inside a class list
    assert got[0][1][2][1]["counts"] == rc.loop_to_string(rc.loop_encode(masks[0, 2]))


def test_as_results_without_masks_is_the_bbox_half():
    det, _ = _detections(with_masks=False)
    got = det.as_results(5)
    assert all(isinstance(r, list) and len(r) == 5 and all(a.shape[1] == 5 for a in r) for r in got)
    assert [a.shape[0] for a in got[2]] == [0, 1, 0, 2, 0]


def test_paste_masks_rle_definition_is_paste_then_encode():
    from panoswintransformerobjectdetection_amd import detector
    lg, labels, boxes, count = rc.paste_inputs(2, 3, 4, 9, 11, "noise")
    enc = rle.paste_masks_rle(lg, labels, boxes, count, 0.5, (9, 11))
    masks = detector.paste_masks_batch(lg, labels, boxes, count, 0.5, (9, 11))
    truth = rc.batch_truth(masks.numpy(), count.tolist())
    off = enc.offsets.tolist()
    assert [enc.runs[off[n]:off[n + 1]].tolist() for n in range(6)] == truth and (enc.B, enc.K) == (2, 3)


def test_heads_predict_refuses_an_unknown_mask_format():
    from panoswintransformerobjectdetection_amd.detector import MiniMaskRCNN
    with pytest.raises(PswinError):
        MiniMaskRCNN._check_mask_format("polygons")


# ---- the cases see the planted defects ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.ENCODE_DEFECTS))
def test_encode_cases_see_the_planted_defect(name):
    bad = rc.ENCODE_DEFECTS[name]
    seen = [n for n, m in MASKS if list(bad(m)) != rle.rle_encode(m).tolist()]
    assert seen, name


@pytest.mark.parametrize("name", sorted(rc.STRING_DEFECTS))
def test_string_cases_see_the_planted_defect(name):
    bad = rc.STRING_DEFECTS[name]
    assert [c for c in rc.STRING_CASES if bad(c) != rle.rle_to_string(c)], name


def test_batch_case_sees_rows_past_the_count_encoded():
    masks = _batch()
    count = [4, 0, 9]
    bad = rc.BATCH_DEFECTS["rows_past_count"](masks, count)
    enc = rle.encode_masks(torch.from_numpy(masks), torch.tensor(count, dtype=torch.int32))
    off = enc.offsets.tolist()
    assert [enc.runs[off[n]:off[n + 1]].tolist() for n in range(12)] != bad
    assert len(rc.ENCODE_DEFECTS) + len(rc.STRING_DEFECTS) + len(rc.BATCH_DEFECTS) >= 8


# ---- the kernels' formulation (bit-planes, trans words, the two scans, guarded stores) restated on the CPU -----------------------
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (63, 2), (64, 3), (65, 17), (130, 5)])
def test_the_kernel_formulation_equals_the_definition(H, W):
    """csrc/pswin_rle.hip's passes in Python integers (tests/_rle_cases.py: emulate_kernel_passes) against rle.encode_masks: the
    formulation, not the HIP code, which tests/test_rle_gpu.py holds to the same definitions on the device"""
    pats = rc.patterns(H, W)
    masks = np.stack(list(pats.values()))
    N = masks.shape[0]
    live = np.ones(N, dtype=bool)
    live[3::5] = False
    want = [rc.loop_encode(m) if l else [] for m, l in zip(masks, live)]
    flat = [c for w in want for c in w]
    for capacity in (len(flat), max(1, len(flat) // 2)):
        offsets, runs = rc.emulate_kernel_passes(masks, live, capacity)
        assert offsets == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
        assert runs == flat[:capacity]
    offsets, runs = rc.emulate_kernel_passes(masks, live, len(flat) + 7)
    assert runs[len(flat):] == [0xA5A5A5A5] * 7                                      # nothing behind offsets[N]
    K = N
    enc = rle.encode_masks(torch.from_numpy(masks[None]), torch.tensor([K], dtype=torch.int32), capacity=N * (H * W + 1))
    all_live = rc.emulate_kernel_passes(masks, np.ones(N, dtype=bool), N * (H * W + 1))
    assert enc.offsets.tolist() == all_live[0] and enc.runs[:all_live[0][-1]].tolist() == all_live[1][:all_live[0][-1]]
