"""Instance masks through the device-side training augmentation, host side (no GPU): pano_aug.transform_masks_one against the
loop-written checker (_pano_masks_ref) bit for bit, closed forms, row provenance, with_targets' host logic with the launches stubbed,
six planted defects, and the reference's RandomFlip -> AutoAugment -> Pad on BitmapMasks (tests/golden/pano_masks.npz)."""
import os

import numpy as np
import pytest
import torch

import _pano_masks_ref as C
import _pano_ref as R
from panoswintransformerobjectdetection_amd import pano_aug as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pano_masks.npz")

# (H, W, n_in, (stretch, kx, ky, shift, flip), plan, rows, pad_hw)
CASES = [
    (24, 40, 3, (0, 1.0, 1.0, 0, False), (0, 0, 0, 0, 0, 0, 30, 50), [[0, -1], [2, 1], [1, -1]], (32, 52)),          # up-resize, merged row
    (24, 40, 3, (1, 1.4, 0.7, 13, True), (0, 0, 0, 0, 0, 0, 17, 29), [[2, -1], [0, -1]], (17, 29)),                    # shrink, all of the warp
    (24, 40, 2, (1, 0.6, 1.9, 39, False), (36, 60, 5, 7, 20, 31, 27, 43), [[1, 0]], (32, 64)),                        # crop, roll of W - 1
    (24, 40, 2, (0, 1.0, 1.0, 7, True), (12, 20, 3, 0, 9, 20, 33, 71), [[0, -1], [1, -1], [1, 0]], (37, 71)),         # shrink then enlarge
    (6, 8, 1, (0, 1.0, 1.0, 0, False), (0, 0, 0, 0, 0, 0, 34, 8), [[0, -1]], (34, 8)),                                 # the nn pair 6 -> 34
    (24, 40, 2, (1, 1.2, 1.1, 0, True), (0, 0, 0, 0, 0, 0, 24, 40), [[5, -1], [-7, 1], [-1, -1]], (24, 40)),          # rows outside [0, n_in)
]


def _one(src, prm, plan, rows, pad_hw):
    return P.transform_masks_one(src, prm[0], prm[1], prm[2], prm[3], prm[4], plan, rows, pad_hw)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_definition_equals_the_checker_bit_for_bit(case):
    H, W, n, prm, plan, rows, pad_hw = CASES[case]
    src = C.blobs(n, H, W, 10 + case)
    got = _one(src, prm, plan, rows, pad_hw)
    assert got.dtype == np.uint8 and got.shape == (len(rows),) + pad_hw and set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got, C.masks(src, *prm, plan, rows, pad_hw))
    assert got[:, plan[6]:].sum() == 0 and got[:, :, plan[7]:].sum() == 0
    if case < 5:
        assert 0 < got.sum() < got.size


def test_closed_forms():
    H, W = 12, 20
    src = C.blobs(3, H, W, 3)
    m = (src != 0).astype(np.uint8)
    ident, rows, off = (0, 0, 0, 0, 0, 0, H, W), [[0, -1], [1, -1], [2, -1]], (0, 1.0, 1.0, 0, False)
    assert np.array_equal(_one(src, off, ident, rows, (H, W)), m)                                                   # an identity plan
    assert np.array_equal(_one(src, (0, 1.0, 1.0, 0, True), ident, rows, (H, W)), m[:, :, ::-1])                     # flip alone
    assert np.array_equal(_one(src, (0, 1.0, 1.0, 7, False), ident, rows, (H, W)), np.roll(m, 7, axis=2))            # roll alone
    assert np.array_equal(_one(src, off, (0, 0, 0, 0, 0, 0, 2 * H, 2 * W), rows, (2 * H, 2 * W)), np.repeat(np.repeat(m, 2, 1), 2, 2))
    assert np.array_equal(_one(src, off, (0, 0, 0, 0, 0, 0, H // 2, W // 2), rows, (H // 2, W // 2)), m[:, ::2, ::2])  # exact 2:1 shrink
    assert np.array_equal(_one(src, off, (H, W, 3, 5, 7, 11, 7, 11), rows, (7, 11)), m[:, 3:10, 5:16])               # a crop alone
    assert np.array_equal(_one(src, off, ident, rows, (H + 5, W + 7)), np.pad(m, ((0, 0), (0, 5), (0, 7))))          # pad alone


def test_warped_plane_equals_the_image_warp_at_one_channel():
    src = C.blobs(2, 24, 40, 5)
    for a in range(2):
        want = R.warp((src[a] != 0).astype(np.uint8)[:, :, None], True, 1.7, 0.6, 11, True)[:, :, 0]
        assert np.array_equal(P.warp_plane01(src[a], True, 1.7, 0.6, 11, True), want)


# ---- row provenance ------------------------------------------------------------------------------------------------------------

SEAM = dict(H=64, W=128, roll_dist=0.25)


def _seam(boxes):
    b = np.array(boxes, np.float32)
    return P.transform_one(b, np.arange(len(b)), SEAM["H"], SEAM["W"], False, 1.0, 1.0, True, SEAM["roll_dist"], False, row_map=True)


def test_unpaired_rows_map_to_themselves_and_defaults_are_unchanged():
    boxes = np.array([[10, 10, 30, 40], [50, 5, 90, 60]], np.float32)
    b, l, m = _seam(boxes)
    assert np.array_equal(m, [[0, -1], [1, -1]]) and m.dtype == np.int32
    b2, l2 = P.transform_one(boxes, np.arange(2), 64, 128, False, 1.0, 1.0, True, 0.25, False)
    assert np.array_equal(b, b2) and np.array_equal(l, l2)
    params = P.make_pano_params([False], [1.0], [1.0], [0.25], [False], 128)
    assert len(P.transform_boxes([boxes], [np.arange(2)], 64, 128, params)) == 2
    assert np.array_equal(P.transform_boxes([boxes], [np.arange(2)], 64, 128, params, row_map=True)[2][0], m)
    e = P.transform_one(np.zeros((0, 4), np.float32), np.zeros(0, np.int64), 64, 128, True, 1.5, 0.8, True, 0.3, True, row_map=True)[2]
    assert e.shape == (0, 2) and e.dtype == np.int32


def test_a_seam_pair_merges_into_the_or_of_both_pieces():
    # row 0 starts at x = 0 (the left piece), row 1 ends at x = W (the right piece): one object cut by the panorama's border
    b, l, m = _seam([[0, 10, 20, 40], [100, 10, 128, 40], [40, 20, 60, 30]])
    assert np.array_equal(m, [[1, 0], [2, -1]]) and np.array_equal(l, [1, 2])
    assert np.array_equal(b[0], [4, 10, 52, 40])                                       # x1 of the right piece, x2 of the left one
    src = np.zeros((3, 64, 128), np.uint8)
    src[0, 10:40, 0:20], src[1, 10:40, 100:128], src[2, 20:30, 40:60] = 255, 1, 1
    got = P.transform_masks_one(src, False, 1.0, 1.0, 32, False, (0, 0, 0, 0, 0, 0, 64, 128), m, (64, 128))
    want = np.roll((src[0] | src[1]) != 0, 32, axis=1)
    assert np.array_equal(got[0], want) and got[0, 10:40, 4:52].all() and got[0].sum() == 30 * 48
    assert np.array_equal(got[1], np.roll(src[2], 32, axis=1))


def test_two_left_pieces_and_one_right_follow_the_last_left_partner():
    b, l, m = _seam([[0, 10, 20, 30], [100, 10, 128, 50], [0, 30, 36, 50]])
    assert np.array_equal(m, [[1, 2], [1, 2]])                                         # emitted once per pair, (j, left[-1]) both times
    assert np.array_equal(b, [[4, 10, 68, 50], [4, 10, 68, 50]])                       # the x2 of row 2, the last left partner


def _crop_aa():
    return dict(policy=1, plan=(64, 128, 8, 40, 40, 60, 40, 60))


def test_a_row_dropped_by_the_crop_takes_its_mask_with_it():
    boxes = np.array([[0, 0, 30, 30], [50, 10, 80, 40], [90, 20, 128, 60]], np.float32)
    b, l, m = P.auto_augment_boxes(boxes, np.arange(3), 64, 128, _crop_aa(), row_map=True)
    assert np.array_equal(l, [1, 2]) and np.array_equal(m, [[1, -1], [2, -1]])
    b2, l2 = P.auto_augment_boxes(boxes, np.arange(3), 64, 128, _crop_aa())
    assert np.array_equal(b, b2) and np.array_equal(l, l2)
    # composed with a seam merge in front: the merged row survives the crop with both of its sources
    tb, tl, tm = _seam([[0, 10, 20, 40], [100, 10, 128, 40], [110, 50, 120, 60]])
    assert np.array_equal(tm, [[1, 0], [2, -1]])                                      # row 2 moves to x = [14, 24]: left of the crop
    cb, cl, cm = P.auto_augment_boxes(tb, tl, 64, 128, _crop_aa(), tm)
    assert np.array_equal(cl, [1]) and np.array_equal(cm, [[1, 0]])
    assert np.array_equal(P.crop_boxes(tb, tl, 40, 8, 40, 60, row_map=True)[2], [[0, -1]])     # True: the identity in front
    with pytest.raises(P.PswinError):
        P.crop_boxes(tb, tl, 40, 8, 40, 60, row_map=tm[:1])


def test_an_image_left_without_rows_has_count_zero_and_a_zero_plane():
    boxes = np.array([[0, 0, 30, 60]], np.float32)
    b, l, m = P.auto_augment_boxes(boxes, np.zeros(1, np.int64), 64, 128, _crop_aa(), row_map=True)
    assert b.shape == (0, 4) and m.shape == (0, 2)
    packed, count = P.pack_rows([m, [[0, -1]]], 2)
    assert count.tolist() == [0, 1] and count.dtype == np.int32 and np.array_equal(packed[0], [[-1, -1], [-1, -1]])
    src = np.full((1, 64, 128), 255, np.uint8)
    assert P.transform_masks_one(src, False, 1.0, 1.0, 0, False, _crop_aa()["plan"], m, (40, 64)).shape == (0, 40, 64)
    assert not P.transform_masks_one(src, False, 1.0, 1.0, 0, False, _crop_aa()["plan"], packed[0], (40, 64)).any()
    with pytest.raises(P.PswinError):
        P.pack_rows([[[0, -1], [1, -1]]], 1)


def test_sizes_past_the_index_arithmetic_are_refused():
    assert P.masks_addressable(8, 100, 100, 512, 1024, 1344, 2688)        # 2.9e9 bytes: the plane bases are 64-bit
    assert not P.masks_addressable(1, 1, 1, 512, 1024, 46341, 46341)      # one output plane of 2^31 bytes and more
    assert not P.masks_addressable(1, 1, 1, 65536, 32768, 32, 64)         # one source plane of 2^31 bytes
    assert not P.masks_addressable(65536, 1, 1, 64, 128, 32, 64) and not P.masks_addressable(1, 1, 1, 64, 128, 16 * 65535 + 1, 2)


# ---- with_targets: the host logic, with the launches stubbed ----------------------------------------------------------------------

def _stub_launches(monkeypatch):
    calls = []
    monkeypatch.setattr(P, "_check_images", lambda *a, **k: None)
    monkeypatch.setattr(P, "norm_tensor", lambda *a, **k: None)
    monkeypatch.setattr(P, "pano_warp", lambda imgs, params, out=None: imgs)
    blank = lambda imgs, sizes, pad_hw=None, **k: torch.zeros(imgs.shape[0], 3, *pad_hw)
    monkeypatch.setattr(P, "resize_normalize_pad", blank)
    monkeypatch.setattr(P, "resize_crop_resize_normalize_pad", blank)

    def record(src, params, plan, rows, count=None, pad_hw=None, size_divisor=32, out=None):
        calls.append(dict(src=src, params=params, plan=plan, rows=rows, count=count, pad_hw=pad_hw, out=out))
        return out
    monkeypatch.setattr(P, "warp_resize_masks", record)
    return calls


def _batch():
    H, W = 64, 128
    boxes = [np.array([[0, 10, 30, 40], [100, 5, 128, 50]], np.float32), np.array([[20, 20, 60, 60]], np.float32),
             np.zeros((0, 4), np.float32), np.array([[40, 8, 90, 60], [2, 2, 6, 6], [0, 30, 128, 34]], np.float32)]
    labels = [np.array([1, 2], np.int64), np.array([3], np.int64), np.zeros(0, np.int64), np.array([4, 1, 0], np.int64)]
    masks = []
    for b in boxes:
        m = np.zeros((len(b), H, W), np.uint8)
        for i, (x1, y1, x2, y2) in enumerate(b.astype(int)):
            m[i, y1:y2, x1:x2] = 255
        masks.append(m)
    return torch.zeros(4, H, W, 3, dtype=torch.uint8), boxes, labels, masks


@pytest.mark.parametrize("auto", [False, True])
def test_with_targets_draws_and_returns_what_call_does(monkeypatch, auto):
    calls = _stub_launches(monkeypatch)
    imgs, boxes, labels, masks = _batch()
    kw = dict(auto_augment=P.STREETWIN_AUTO_AUGMENT) if auto else {}
    for seed in range(6):
        r1, r2 = np.random.RandomState(seed), np.random.RandomState(seed)
        x, b, l, metas = P.PanoTrainTransform(rng=r1, **kw)(imgs, [v.copy() for v in boxes], labels)
        x2, T, metas2 = P.PanoTrainTransform(rng=r2, **kw).with_targets(imgs, [v.copy() for v in boxes], labels, masks)
        assert r1.rand() == r2.rand()                                                  # the stream is in the same place
        assert x.shape == x2.shape and len(metas) == len(metas2)
        for m, m2 in zip(metas, metas2):
            assert m.keys() == m2.keys() and all(np.array_equal(m[k], m2[k]) for k in m if k != "img_norm_cfg")
        Gmax = max(1, max(len(v) for v in b))
        assert T.count.tolist() == [len(v) for v in b] and T.count.dtype == torch.int32
        assert tuple(T.boxes.shape) == (4, Gmax, 4) and T.labels.dtype == torch.long
        for i in range(4):
            n = len(b[i])
            assert np.array_equal(T.boxes[i, :n].numpy(), b[i]) and np.array_equal(T.labels[i, :n].numpy(), l[i])
            assert not T.boxes[i, n:].any() and not T.labels[i, n:].any()
        c = calls[-1]
        assert c["out"] is T.masks and tuple(T.masks.shape) == (4, Gmax) + tuple(x.shape[2:]) and T.masks.dtype == torch.uint8
        assert tuple(c["src"].shape) == (4, 3, 64, 128) and np.array_equal(c["src"][3].numpy(), masks[3]) and not c["src"][2].any()
        assert tuple(c["pad_hw"]) == tuple(x.shape[2:]) and [p[6:] for p in c["plan"]] == [m["img_shape"][:2] for m in metas]
        assert c["count"] is T.count and c["rows"].dtype == torch.int32 and tuple(c["rows"].shape) == (4, Gmax, 2)
        for i in range(4):
            assert (c["rows"][i, len(b[i]):] == -1).all() and (c["rows"][i, :len(b[i]), 0] >= 0).all()
    # without masks: the Faster R-CNN form, and no launch
    n = len(calls)
    _, T, _ = P.PanoTrainTransform(rng=np.random.RandomState(0), **kw).with_targets(imgs, boxes, labels)
    assert T.masks is None and len(calls) == n


def test_with_targets_writes_a_given_buffer_in_place_and_checks_it(monkeypatch):
    from panoswintransformerobjectdetection_amd.detector import PaddedTargets
    _stub_launches(monkeypatch)
    imgs, boxes, labels, masks = _batch()
    t = P.PanoTrainTransform(rng=np.random.RandomState(1), img_scales=[(64, 128)])
    out = PaddedTargets.allocate(4, 5, "cpu", mask_hw=(64, 128))
    out.boxes.fill_(7.0)
    x, T, _ = t.with_targets(imgs, boxes, labels, masks, out=out)
    assert T is out and tuple(x.shape) == (4, 3, 64, 128) and T.count.tolist()[2] == 0 and not T.boxes[2].any()
    for bad in (PaddedTargets.allocate(3, 5, "cpu", mask_hw=(64, 128)), PaddedTargets.allocate(4, 1, "cpu", mask_hw=(64, 128)),
                PaddedTargets.allocate(4, 5, "cpu", mask_hw=(64, 160)), PaddedTargets.allocate(4, 5, "cpu"), "targets"):
        with pytest.raises(P.PswinError):
            t.with_targets(imgs, boxes, labels, masks, out=bad)
    with pytest.raises(P.PswinError):
        t.with_targets(imgs, boxes, labels, None, out=out)                             # a mask buffer but no masks
    with pytest.raises(P.PswinError):
        t.with_targets(imgs, boxes, labels, masks[:3])
    with pytest.raises(P.PswinError):
        t.with_targets(imgs, boxes, labels, [m[:1] for m in masks])                    # one bitmap per box
    with pytest.raises(P.PswinError):
        t.with_targets(imgs, boxes, labels, [m.astype(np.float32) for m in masks])


# ---- planted defects ------------------------------------------------------------------------------------------------------------

def test_defect_ratio_written_as_n_in_over_n_out():
    """6 -> 34 at d = 17: 17 * (1 / (34 / 6)) = 2.9999999999999996 but 17 * (6 / 34) = 3.0 (found by a search over n_in < 200, n_out < 300:
    the first pair in that order)."""
    assert C.nn(17, 6, 34) == 2 and C.nn_ratio(17, 6, 34) == 3 and int(P.nn_index(17, 6, 34)) == 2
    H, W, n, prm, plan, rows, pad_hw = CASES[4]
    src = np.zeros((1, 6, 8), np.uint8)
    src[0, 3] = 1
    good = _one(src, prm, plan, rows, pad_hw)
    assert np.array_equal(good, C.masks(src, *prm, plan, rows, pad_hw))
    assert not np.array_equal(good, C.masks(src, *prm, plan, rows, pad_hw, nn=C.nn_ratio))


def test_defect_crop_offset_after_the_second_resize():
    H, W, n, prm, plan, rows, pad_hw = CASES[2]
    src = C.blobs(n, H, W, 12)
    assert not np.array_equal(_one(src, prm, plan, rows, pad_hw), C.masks(src, *prm, plan, rows, pad_hw, crop_late=True))


def test_defect_flip_before_roll():
    H, W, n, prm, plan, rows, pad_hw = CASES[1]
    src = C.blobs(n, H, W, 11)
    assert prm[3] and prm[4]
    assert not np.array_equal(_one(src, prm, plan, rows, pad_hw), C.masks(src, *prm, plan, rows, pad_hw, flip_first=True))


def test_defect_merge_as_and():
    H, W, n, prm, plan, rows, pad_hw = CASES[0]
    src = C.blobs(n, H, W, 10)
    assert not np.array_equal(_one(src, prm, plan, rows, pad_hw), C.masks(src, *prm, plan, rows, pad_hw, merge_and=True))


def test_defect_rows_not_remapped_after_the_crop():
    boxes = np.array([[0, 0, 30, 30], [50, 10, 80, 40]], np.float32)
    aa = _crop_aa()
    b, l, m = P.auto_augment_boxes(boxes, np.arange(2), 64, 128, aa, row_map=True)
    src = np.zeros((2, 64, 128), np.uint8)
    src[0, 0:30, 0:30], src[1, 10:40, 50:80] = 1, 1
    good = P.transform_masks_one(src, False, 1.0, 1.0, 0, False, aa["plan"], m, (40, 64))
    assert np.array_equal(good, C.masks(src, False, 1.0, 1.0, 0, False, aa["plan"], m, (40, 64)))
    stale = P._identity_map(2)[:len(m)]                                               # the first kept row read as input row 0
    assert not np.array_equal(good, C.masks(src, False, 1.0, 1.0, 0, False, aa["plan"], stale, (40, 64)))
    assert good[0, 2:32, 10:40].all() and good[0].sum() == 900                        # row 1's square, moved by the crop offset


def test_defect_strict_comparison_at_a_blend_of_exactly_one_half():
    plane = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]], np.uint8)
    refy, refx = np.array([[0.0, 0.5, 0.25]]), np.array([[0.5, 0.0, 0.5]])          # blends 0.5, 1.0, 0.5
    want = R.bilinear_wrap_u8(plane[:, :, None], refy, refx)[:, :, 0]
    assert np.array_equal(want, [[1, 1, 1]])
    assert np.array_equal(P.sample_plane01(plane.astype(np.float64), refy, refx), want)
    assert np.array_equal(C.sample_strict(plane, refy, refx), [[0, 1, 0]])


# ---- the reference's mask pipeline ----------------------------------------------------------------------------------------------

def test_definition_equals_the_recorded_reference_pipeline():
    """RandomFlip -> AutoAugment -> Pad of the reference on BitmapMasks, recorded by tools/gen_pano_masks_golden.py.  The fixture pins
    the order of the steps (flip first), which rows are kept, the crop arithmetic and every size; mmcv's resampling is stood in by the
    nearest rule itself, so the resampling rule is NOT pinned by it (PARITY: unpinned)."""
    g = np.load(GOLDEN)
    lo, seen = 0, set()
    for i in range(int(g["n_cases"])):
        src, plan = g[f"masks{int(g['case_src'][i])}"], tuple(int(v) for v in g["case_plan"][i])
        n, flip = int(g["case_n_rows"][i]), bool(g["case_flip"][i])
        keep = g["out_rows"][lo:lo + n]
        lo += n
        hp, wp = (int(v) for v in g["case_pad_hw"][i])
        want = np.unpackbits(g[f"out{i}"])[:n * hp * wp].reshape(n, hp, wp)
        assert (hp, wp) == P.padded_size([plan[6:]], 32)
        got = P.transform_masks_one(src, False, 1.0, 1.0, 0, flip, plan, np.stack([keep, np.full(n, -1)], 1), (hp, wp))
        assert np.array_equal(got, want), i
        seen.add((plan[0] > 0, flip, n < len(src)))
    assert lo == len(g["out_rows"]) and len(seen) == 6           # crop x flip with and without dropped rows, no crop x flip


def test_fresh_seeds_against_the_live_reference(monkeypatch):
    """The same comparison on seeds the fixture does not hold, where the reference tree is on the machine; the row maps come from the
    package's own box path (auto_augment_boxes) this time, so its row keeping is compared with the reference's too."""
    import sys
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import gen_pano_masks_golden as G
    path, modules = list(sys.path), dict(sys.modules)
    ref = G.load_reference()
    if ref is None:
        pytest.skip("the reference tree (PSWIN_REFERENCE_ROOT) is not on this machine")
    assert sys.path == path and dict(sys.modules) == modules                  # the interpreter is as it was: no stand-in left behind
    pipeline = G.make_pipeline(ref)
    for s, (H, W) in enumerate(G.SOURCES):
        masks, boxes, labels = G.source(s, H, W)
        for seed in range(5000, 5012):
            r = G.run_seeded(ref, masks, boxes, labels, seed, pipeline)
            fb = boxes.copy()
            if r["flip"]:
                fb[:, 0], fb[:, 2] = W - boxes[:, 2], W - boxes[:, 0]
            b, l, m = P.auto_augment_boxes(fb, labels, H, W, dict(policy=r["policy"], plan=r["plan"]), row_map=True)
            assert np.array_equal(l, r["rows"]) and np.array_equal(m[:, 0], r["rows"])
            got = P.transform_masks_one(masks, False, 1.0, 1.0, 0, r["flip"], r["plan"], m, r["pad_hw"])
            assert np.array_equal(got, r["masks"]), (s, seed)
