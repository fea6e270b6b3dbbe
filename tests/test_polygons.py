"""COCO polygons to masks on the CPU: the rule of panoswintransformerobjectdetection_amd/polygons.py (pycocotools' rleFrPoly restated;
PARITY: unpinned) against the independent column-by-column restatement of tests/_poly_cases.py, the facts the kernel relies on, planted
defects, the PolygonBatch container and its refusals, the wiring, and the C ABI's argument checks without a GPU."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _poly_cases as pc

N_RANDOM = 2400


def _mods():
    from panoswintransformerobjectdetection_amd import polygons, rle
    return polygons, rle


@functools.lru_cache(maxsize=None)
def _random():
    return pc.random_polygons(N_RANDOM, seed=0)


def _part_cases():
    return [(name, part, h, w) for name, parts, h, w in pc.NAMED for part in parts] + list(_random())


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_hand_answers():
    P, _ = _mods()
    for xy, h, w, want in pc.HAND:
        assert P.rle_from_polygon(xy, h, w).tolist() == want
        assert pc.restated_counts(xy, h, w) == want


def test_rule_equals_the_restatement_and_is_canonical():
    """On every named part and 2,400 seeded random polygons of the three families: == against the restatement (which is "toggle at the
    event positions, prefix XOR in scan order"), runs that sum to h w, and rle_encode(rle_decode(.)) returning them."""
    P, rle = _mods()
    seen = {f: 0 for f in pc.FAMILIES}
    sizes, dup, wrap, outside = set(), 0, 0, 0
    for name, xy, h, w in _part_cases():
        got = P.rle_from_polygon(xy, h, w)
        assert got.dtype == np.uint32
        assert got.tolist() == pc.restated_counts(xy, h, w), (name, xy, h, w)
        assert int(got.astype(np.int64).sum()) == h * w
        assert rle.rle_encode(rle.rle_decode(got, h, w)).tolist() == got.tolist(), (name, xy, h, w)
        if name in seen:
            seen[name] += 1
            sizes.add((h, w))
            ev = P.polygon_events(xy, h, w)
            dup += len(set(ev)) != len(ev)
            wrap += any(e % h == 0 and e > 0 for e in ev)
            a = np.asarray(xy).reshape(-1, 2)
            outside += bool((a[:, 0] < -2).any() or (a[:, 0] > w + 2).any() or (a[:, 1] < -2).any() or (a[:, 1] > h + 2).any())
    assert all(n == N_RANDOM // 3 for n in seen.values()) and N_RANDOM >= 2000
    assert sizes == {(h, w) for h in pc.RANDOM_H for w in pc.RANDOM_W}
    assert dup > 500 and wrap > 500 and outside > 500                      # duplicate positions, yd = h wraps, vertices 3 pixels outside


def test_every_image_column_holds_an_even_number_of_events():
    """What lets a kernel lane fill its column alone: the prefix XOR is 0 at the top of every column, and an event with yd = h is void."""
    for name, xy, h, w in _part_cases():
        for c, rows in pc.column_events(xy, h, w).items():
            if 0 <= c <= w - 1:
                assert len(rows) % 2 == 0, (name, xy, h, w, c)


def test_events_are_what_an_edge_s_ends_say():
    """An edge has an event in column c exactly when min(xs, xe) <= 5 c + 2 and 5 c + 3 <= max(xs, xe) (the kernel's test)."""
    P, _ = _mods()
    for name, xy, h, w in _part_cases()[:600]:
        k = len(xy) // 2
        X = [int(5.0 * float(xy[2 * j]) + 0.5) for j in range(k)]
        want = {}
        for j in range(k):
            lo, hi = min(X[j], X[(j + 1) % k]), max(X[j], X[(j + 1) % k])
            for c in range(w):
                if lo <= 5 * c + 2 and 5 * c + 3 <= hi:
                    want[c] = want.get(c, 0) + 1
        # a position x h + h is column x's event at yd = h, so the columns come from the restatement and the total from the rule
        cols = {c: len(r) for c, r in pc.column_events(xy, h, w).items() if 0 <= c <= w - 1}
        assert cols == want, (name, xy, h, w)
        assert len(P.polygon_events(xy, h, w)) == sum(want.values())


def test_named_objects_or_their_parts():
    P, _ = _mods()
    by_name = {}
    for name, parts, h, w in pc.NAMED:
        m = P.object_mask(parts, h, w)
        assert np.array_equal(m, pc.restated_object_mask(parts, h, w)), name
        by_name[name] = m
    assert not by_name["collinear"].any() and not by_name["collinear_horizontal"].any()
    for name in ("wholly_left", "wholly_right", "wholly_above", "wholly_below"):
        assert not by_name[name].any(), name
    assert by_name["covers_everything"].all() and by_name["one_pixel_image"].all()
    assert np.array_equal(by_name["hand_square"][1:4, 1:4], np.ones((3, 3), np.uint8)) and by_name["hand_square"].sum() == 9
    assert by_name["clamp_to_0_and_h"][:, 2:6].all() and by_name["clamp_to_0_and_h"].sum() == 8 * 4
    assert np.array_equal(by_name["same_part_twice"], P.object_mask([pc.NAMED_BY_NAME["same_part_twice"][0][0]], 8, 8))   # OR, not XOR
    assert by_name["parts_nested"].sum() == 64 and by_name["parts_overlapping"].sum() == 25 + 25 - 4
    assert by_name["parts_disjoint"].sum() == 18 and len(pc.NAMED_BY_NAME["five_parts"][0]) == 5
    assert np.array_equal(by_name["shared_events_cancel"], P.object_mask([[1, 1, 7, 1, 7, 5, 1, 5]], 8, 8))        # two halves of one box


@pytest.mark.parametrize("defect", pc.DEFECTS)
def test_planted_defects_change_an_answer(defect):
    """every wrong reading of the rule is noticed by a named case"""
    P, _ = _mods()
    hits = [name for name, parts, h, w in pc.NAMED
            if not np.array_equal(pc.restated_object_mask(parts, h, w, defect), P.object_mask(parts, h, w))]
    assert hits, defect


def test_the_branch_choice_at_dx_equal_dy_is_not_observable():
    """`>` for `>=` in the branch choice changes no answer, here or anywhere: at dx = dy the slope is exactly +-1, so both branches list
    the same points wherever u, v >= 0, and where they are negative (truncation makes int(z + 0.5) differ from z) the column is skipped
    (u < 2) and the row is clamped to 0 (v < 2).  So this reading of the rule cannot be told from the stated one by any case; the
    test records that instead of counting it among the planted defects."""
    for name, xy, h, w in _part_cases():
        assert pc.restated_counts(xy, h, w, "gt_for_ge") == pc.restated_counts(xy, h, w), (name, xy, h, w)


# ---- the container ----------------------------------------------------------------------------------------------------------------
ANN = [[[[1, 1, 4, 1, 4, 4, 1, 4]], [[0, 0, 3, 0, 3, 3], [5, 5, 8, 5, 8, 8, 5, 8.5]]], [], [[[2.5, 0, 4, 4, 0, 4]]]]


def test_polygon_batch_layout_and_flat_offsets():
    P, _ = _mods()
    pb = P.PolygonBatch.from_lists(ANN, 9, 10, "cpu")
    assert (pb.B, pb.K, pb.height, pb.width) == (3, 2, 9, 10) and pb.count.tolist() == [2, 0, 1]
    assert pb.xy.dtype == torch.float64 and tuple(pb.xy.shape) == (14, 2) and pb.part_offsets.dtype == torch.int32
    assert pb.part_offsets.tolist() == [0, 4, 7, 11, 14] and pb.obj_offsets.tolist() == [0, 1, 3, 3, 3, 4, 4]
    assert pb.xy[4:7].reshape(-1).tolist() == [0, 0, 3, 0, 3, 3] and pb.to_lists() == [[[[float(v) for v in p] for p in o] for o in per] for per in ANN]
    wide = P.PolygonBatch.from_lists(ANN, 9, 10, "cpu", K=4)
    assert wide.obj_offsets.tolist() == [0, 1, 3, 3, 3, 3, 3, 3, 3, 4, 4, 4, 4]
    empty = P.PolygonBatch.from_lists([[], []], 4, 4, "cpu")
    assert (empty.K, empty.max_parts, empty.max_vertices) == (1, 1, 1) and empty.obj_offsets.tolist() == [0, 0, 0]
    assert not P.polygons_to_masks(empty).any()
    # allocate + copy_from: the same contents in larger buffers, flat / zero tails, and a second batch over the first
    buf = P.PolygonBatch.allocate(3, 2, 6, 20, 9, 10, "cpu")
    assert buf.count.tolist() == [0, 0, 0] and not P.polygons_to_masks(buf).any()
    assert buf.copy_from(ANN) is buf
    assert buf.part_offsets.tolist() == [0, 4, 7, 11, 14, 14, 14] and buf.obj_offsets.tolist() == pb.obj_offsets.tolist()
    assert torch.equal(buf.xy[:14], pb.xy) and not buf.xy[14:].any() and buf.to_lists() == pb.to_lists()
    assert torch.equal(P.polygons_to_masks(buf), P.polygons_to_masks(pb))
    buf.copy_from([[], [[[0, 0, 9, 0, 9, 9]]], []])
    assert buf.count.tolist() == [0, 1, 0] and buf.obj_offsets.tolist() == [0, 0, 0, 1, 1, 1, 1] and buf.part_offsets.tolist() == [0, 3, 3, 3, 3, 3, 3]


def test_polygon_batch_refusals():
    P, _ = _mods()
    E = P.PswinError
    ok = [1, 1, 4, 1, 4, 4]
    for bad in ([1, 1, 4, 1], [1, 1, 4, 1, 4, 4, 2], [1, 1, 4, 1, 4, float("nan")], [1, 1, 4, 1, 4, float("inf")], [1, 1, 4, 1, 4, 2.0 ** 20 + 1],
                [-2.0 ** 20 - 1, 1, 4, 1, 4, 4]):
        with pytest.raises(E):
            P.PolygonBatch.from_lists([[[bad]]], 8, 8, "cpu")
        with pytest.raises(E):
            P.rle_from_polygon(bad, 8, 8)
    P.PolygonBatch.from_lists([[[[2.0 ** 20, 1, -2.0 ** 20, 1, 4, 4]]]], 8, 8, "cpu")                # the limit itself is taken
    with pytest.raises(E):
        P.PolygonBatch.from_lists([[[ok]], [[ok], [ok]]], 8, 8, "cpu", K=1)                         # more objects than K
    with pytest.raises(E):
        P.PolygonBatch.from_lists([[dict(size=[8, 8], counts=[64])]], 8, 8, "cpu")                  # a crowd's RLE
    with pytest.raises(E):
        P.PolygonBatch.from_lists([], 8, 8, "cpu")
    with pytest.raises(E):
        P.PolygonBatch.from_lists([[[ok]]], 0, 8, "cpu")
    with pytest.raises(E):
        P.PolygonBatch.allocate(1, 0, 1, 3, 8, 8, "cpu")
    buf = P.PolygonBatch.allocate(2, 1, 2, 7, 8, 8, "cpu")
    buf.copy_from([[[ok, ok]], []])
    before = [t.clone() for t in (buf.xy, buf.part_offsets, buf.obj_offsets, buf.count)]
    for bad in ([[[ok]]], [[[ok]], [[ok]], []], [[[ok], [ok]], []], [[[ok, ok, ok]], []], [[[ok + [5, 5, 6, 6], ok]], []], [[[ok[:4]]], []]):
        with pytest.raises(E):
            buf.copy_from(bad)                                                                      # images, K, parts, vertices, a short part
    assert all(torch.equal(a, b) for a, b in zip(before, (buf.xy, buf.part_offsets, buf.obj_offsets, buf.count)))   # refused: untouched
    with pytest.raises(E):
        P.polygons_to_masks(ANN)
    with pytest.raises(E):
        P.polygons_to_masks(buf, out=torch.zeros(2, 1, 8, 9, dtype=torch.uint8))
    with pytest.raises(E):
        P.polygons_to_rle(buf, capacity=0)
    assert P.poly_supported(8, 32, 512, 1024) and P.poly_supported(1, 1, 4096, 4096) and not P.poly_supported(1, 1, 4097, 8)
    assert not P.poly_supported(1, 1, 8, 4097) and not P.poly_supported(0, 1, 8, 8) and not P.poly_supported(1 << 16, 1 << 15, 8, 8)


# ---- wiring -------------------------------------------------------------------------------------------------------------------------
def test_definitions_of_a_batch_and_the_round_trip_through_lists():
    P, rle = _mods()
    pb = P.PolygonBatch.from_lists(ANN, 9, 10, "cpu", K=3)
    masks = P.polygons_to_masks(pb)
    assert masks.dtype == torch.uint8 and tuple(masks.shape) == (3, 3, 9, 10) and int(masks.max()) == 1
    for b, per in enumerate(ANN):
        for k in range(3):
            want = pc.restated_object_mask(per[k], 9, 10) if k < len(per) else np.zeros((9, 10), np.uint8)
            assert np.array_equal(masks[b, k].numpy(), want), (b, k)
    enc = P.polygons_to_rle(pb)
    assert (enc.B, enc.K, enc.height, enc.width) == (3, 3, 9, 10) and enc.count is pb.count
    via = rle.encode_masks(masks, pb.count)
    assert torch.equal(enc.offsets, via.offsets) and torch.equal(enc.runs[:int(enc.offsets[-1])], via.runs[:int(via.offsets[-1])])
    lists = enc.to_lists()
    assert [len(per) for per in lists] == [2, 0, 1]
    back = rle.RleMasks.from_lists(lists, "cpu", K=3)
    assert torch.equal(back.offsets, enc.offsets) and torch.equal(back.runs[:int(back.offsets[-1])], enc.runs[:int(enc.offsets[-1])])
    assert rle.rle_decode(rle.rle_from_string(lists[2][0]["counts"]), 9, 10).tolist() == masks[2, 0].tolist()
    # the overflow contract of the definition: offsets whole, to_lists raises
    total = int(enc.offsets[-1])
    short = P.polygons_to_rle(pb, capacity=total - 1)
    assert torch.equal(short.offsets, enc.offsets) and torch.equal(short.runs[:total - 1], enc.runs[:total - 1])
    with pytest.raises(P.PswinError):
        short.to_lists()
    out = rle.RleMasks.allocate(9, 9, 10, "cpu", total + 5)
    assert P.polygons_to_rle(pb, out=out) is out and (out.B, out.K) == (3, 3)


def test_with_targets_takes_a_polygon_batch(monkeypatch):
    """with_targets(masks=PolygonBatch) on CPU tensors, the launches stubbed as in tests/test_pano_masks.py: the source bitmaps it hands
    to the mask launch, and everything else, are those of the call with the rasterised bitmaps."""
    from panoswintransformerobjectdetection_amd import pano_aug as A
    P, _ = _mods()
    calls = []
    monkeypatch.setattr(A, "_check_images", lambda *a, **k: None)
    monkeypatch.setattr(A, "norm_tensor", lambda *a, **k: None)
    monkeypatch.setattr(A, "pano_warp", lambda imgs, params, out=None: imgs)
    blank = lambda imgs, sizes, pad_hw=None, **k: torch.zeros(imgs.shape[0], 3, *pad_hw)
    monkeypatch.setattr(A, "resize_normalize_pad", blank)
    monkeypatch.setattr(A, "resize_crop_resize_normalize_pad", blank)

    def record(src, params, plan, rows, count=None, pad_hw=None, size_divisor=32, out=None):
        calls.append(dict(src=src, rows=rows, plan=plan, pad_hw=pad_hw))
        return out
    monkeypatch.setattr(A, "warp_resize_masks", record)
    H, W = 64, 128
    boxes = [np.array([[0, 10, 30, 40], [100, 5, 128, 50]], np.float32), np.zeros((0, 4), np.float32), np.array([[40, 8, 90, 60]], np.float32)]
    labels = [np.array([1, 2], np.int64), np.zeros(0, np.int64), np.array([4], np.int64)]
    ann = [[[[0, 10, 30, 10, 30, 40, 0, 40]], [[100, 5, 128, 5, 128, 50], [101, 30, 120, 50, 100.5, 50]]], [], [[pc.star(16, 65, 34, 25, 11)]]]
    pb = P.PolygonBatch.from_lists(ann, H, W, "cpu", K=3)
    bitmaps = P.polygons_to_masks_definition(pb)
    imgs = torch.zeros(3, H, W, 3, dtype=torch.uint8)
    res = []
    for masks in (pb, [bitmaps[b, :len(boxes[b])].numpy() for b in range(3)]):
        rng = np.random.RandomState(3)
        x, T, metas = A.PanoTrainTransform(rng=rng).with_targets(imgs, [v.copy() for v in boxes], labels, masks)
        res.append((x, T, metas, rng.rand()))
    (x1, T1, m1, r1), (x2, T2, m2, r2) = res
    assert r1 == r2 and torch.equal(T1.boxes, T2.boxes) and torch.equal(T1.labels, T2.labels) and torch.equal(T1.count, T2.count)
    assert tuple(T1.masks.shape) == tuple(T2.masks.shape) and calls[0]["pad_hw"] == calls[1]["pad_hw"] and calls[0]["plan"] == calls[1]["plan"]
    assert torch.equal(calls[0]["rows"], calls[1]["rows"])
    assert torch.equal(calls[0]["src"][:, :2], calls[1]["src"]) and calls[0]["src"] is not bitmaps and torch.equal(calls[0]["src"], bitmaps)
    for bad in (P.PolygonBatch.from_lists(ann, H, W + 1, "cpu", K=3), P.PolygonBatch.from_lists(ann[:2], H, W, "cpu", K=3),
                P.PolygonBatch.from_lists([[], [], []], H, W, "cpu", K=1)):
        with pytest.raises(A.PswinError):
            A.PanoTrainTransform(rng=np.random.RandomState(3)).with_targets(imgs, [v.copy() for v in boxes], labels, bad)


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_touching_the_device():
    import os
    import re
    from panoswintransformerobjectdetection_amd import _poly_lib, build
    build.build_poly(force=False, verbose=False)
    lib = _poly_lib.load()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pswin_poly.h")).read()
    declared = sorted(set(re.findall(r"\bint\s+(pswin_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == _poly_lib.exported_symbols() and lib.pswin_poly_version() == _poly_lib.ABI_VERSION
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15
    #     xy   parts     objs       count      P  V  B  K  H  W   masks      ws          stream
    ok = [p16, p16 + 64, p16 + 128, p16 + 192, 4, 8, 1, 2, 8, 16, p16 + 256, p16 + 1024, None]
    bad = {"xy": (0, None), "xy align": (0, p16 + 8), "parts": (1, None), "parts align": (1, p16 + 66), "objs": (2, None),
           "objs align": (2, p16 + 130), "count": (3, None), "count align": (3, p16 + 193), "max_parts": (4, 0), "max_vertices": (5, 0),
           "B": (6, 0), "K": (7, 0), "K negative": (7, -1), "H": (8, 0), "H limit": (8, 4097), "W": (9, 0), "W limit": (9, 4097),
           "masks": (10, None), "workspace": (11, None), "workspace align": (11, p16 + 1032)}
    for name, (i, v) in bad.items():
        args = list(ok)
        args[i] = v
        assert lib.pswin_poly_masks(*args) == -1, name
    big = list(ok)
    big[6], big[7] = 1 << 16, 1 << 15                                           # B K = 2^31
    assert lib.pswin_poly_masks(*big) == -1
    nbytes = ctypes.c_longlong(-5)
    assert lib.pswin_poly_workspace(1, 2, 4097, 16, ctypes.byref(nbytes)) == -1 and lib.pswin_poly_workspace(1, 0, 8, 16, ctypes.byref(nbytes)) == -1
    assert lib.pswin_poly_workspace(1, 2, 8, 16, None) == -1 and nbytes.value == -5
    assert lib.pswin_poly_workspace(3, 2, 130, 17, ctypes.byref(nbytes)) == 0 and nbytes.value == 8 * 6 * 3 * 17
