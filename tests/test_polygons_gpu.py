"""COCO polygons to masks on the MI355X (csrc/pswin_poly.hip through polygons.polygons_to_masks / polygons_to_rle) against the definitions
of polygons.py computed once per batch on the CPU.  Every comparison is torch.equal: the rule has one answer.  Outputs are pre-filled
(masks with 0xFF, the run pool with 0xA5 and allocated longer than its capacity, offsets with -7) and the workspace with 0xFF before every
call; every call runs twice for identical bits.  The cases are those of tests/_poly_cases.py, which tests/test_polygons.py holds against
an independent restatement of the rule."""
import numpy as np
import pytest
import torch

import _poly_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 96


def _mods():
    from panoswintransformerobjectdetection_amd import polygons, rle
    return polygons, rle


def _on_device(pb):
    P, _ = _mods()
    return P.PolygonBatch(pb.xy.to(DEV), pb.part_offsets.to(DEV), pb.obj_offsets.to(DEV), pb.count.to(DEV), pb.height, pb.width, pb.B, pb.K)


def _poisoned_rle(N, H, W, capacity):
    _, rle = _mods()
    runs = torch.empty(capacity + GUARD, dtype=torch.uint32, device=DEV)
    runs.view(torch.uint8).fill_(0xA5)
    return rle.RleMasks(torch.full((N + 1,), -7, dtype=torch.int64, device=DEV), runs, H, W, capacity=capacity)


def _check_runs(enc, want, capacity):
    """enc (device) against the definition `want` (CPU, with room for every run) under `capacity`: offsets whole, the runs below the
    capacity, 0xA5 behind them"""
    assert torch.equal(enc.offsets.cpu(), want.offsets)
    total = int(want.offsets[-1])
    got = enc.runs.cpu()
    wrote = min(total, capacity)
    assert torch.equal(got[:wrote], want.runs[:wrote])
    assert bool((got[wrote:].view(torch.uint8) == 0xA5).all())
    return got


def _both_twice(ops, pb, capacity=None):
    """polygons_to_masks and polygons_to_rle of the CPU batch `pb` on the device, twice each, against the definitions; returns them"""
    P, rle = _mods()
    N, H, W = pb.B * pb.K, pb.height, pb.width
    want_masks = P.polygons_to_masks_definition(pb)
    want = P.polygons_to_rle_definition(pb, capacity=N * (H * W + 1))
    total = int(want.offsets[-1])
    cap = max(total, 1) if capacity is None else capacity
    d = _on_device(pb)
    ws, planes = ops._rle_workspace(N, H, W, torch.device(DEV)), P.poly_workspace(d)
    masks, runs = [], []
    for _ in range(2):
        out = torch.full((pb.B, pb.K, H, W), 0xFF, dtype=torch.uint8, device=DEV)
        planes.fill_(0xFF)
        got = P.polygons_to_masks(d, out=out)
        assert got is out
        torch.cuda.synchronize()
        assert torch.equal(got.cpu(), want_masks)
        masks.append(got)
        enc = _poisoned_rle(N, H, W, cap)
        ws.fill_(0xFF)
        planes.fill_(0xFF)
        P._scratch(d, "bitmaps", (pb.B, pb.K, H, W)).fill_(0xFF)
        assert P.polygons_to_rle(d, out=enc) is enc and (enc.B, enc.K) == (pb.B, pb.K) and enc.count is d.count
        torch.cuda.synchronize()
        runs.append(_check_runs(enc, want, cap))
    assert torch.equal(masks[0], masks[1]) and torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    if capacity is None:                                                         # the cross-check: the bitmap producer on these masks
        via = rle.encode_masks(masks[0], d.count, capacity=cap)
        torch.cuda.synchronize()
        assert torch.equal(via.offsets, enc.offsets) and torch.equal(via.runs[:total].view(torch.int32), enc.runs[:total].view(torch.int32))
    return d, masks[0], enc, want


def _scaled_star(n, H, W, phase=0.3):
    """n vertices (n edges) around the image's centre, reaching a little outside it"""
    return pc.star(n, W / 2.0, H / 2.0, 0.6 * max(W, H) + 1.0, 0.23 * min(W, H) + 0.4, phase)


def _shape_batch(H, W):
    """B = 3, K = 5: parts of 3, 64, 65, 256 and 257 edges, objects of 1, 3 and 5 parts (one part with vertices 3000 pixels away: long
    bisections), an image with count = 0, and rows past the counts that hold valid polygons which must not be rasterised"""
    P, _ = _mods()
    box = lambda x0, y0, x1, y1: [x0, y0, x1, y0, x1, y1, x0, y1]
    five = [box(W * i / 5.0 - 0.3, H * i / 7.0 - 1.0, W * (i + 1.6) / 5.0, H * (i + 3) / 7.0 + 0.2) for i in range(5)]
    full = [
        [[_scaled_star(3, H, W)], [_scaled_star(64, H, W)], [_scaled_star(65, H, W, 1.1)], [_scaled_star(256, H, W)], [_scaled_star(257, H, W, 0.7)]],
        [[box(-3, -3, W + 3, H + 3)], [_scaled_star(8, H, W)]],                                    # count = 0: neither is read
        [[_scaled_star(5, H, W), box(0.4, 0.4, W / 2.0, H / 2.0 + 0.6), [-3000.3, -2500.7, W * 0.4, H * 0.3, 2800.1, 3100.9]], five, [box(-3, -3, W + 3, H + 3)], [_scaled_star(7, H, W)]],
    ]
    pb = P.PolygonBatch.from_lists(full, H, W, "cpu", K=5)
    pb.count.copy_(torch.tensor([5, 0, 2], dtype=torch.int32))
    return pb


@pytest.mark.parametrize("H,W", [(1, 1), (63, 17), (64, 256), (65, 257), (130, 48), (130, 257), (64, 48), (1, 256), (63, 1), (65, 17)])
def test_shapes_where_the_kernels_change_path(ops, H, W):
    pb = _shape_batch(H, W)
    d, masks, enc, want = _both_twice(ops, pb)
    assert not masks[1].any() and not masks[2, 2:].any()                          # rows past a count: zeros, whatever their polygons say
    off = enc.offsets.cpu()
    assert int(off[5]) == int(off[10]) and int(off[12]) == int(off[15])           # rows past a count own no runs
    if H > 1 and W > 16:
        assert masks[0].any() and masks[2, 1].any()


def _groups():
    """every named case and 300 of the seeded random polygons, grouped by image size and cut into batches of B K = 1 .. 12 objects"""
    by_size = {}
    for name, parts, h, w in pc.NAMED:
        by_size.setdefault((h, w), []).append(parts)
    for fam, xy, h, w in pc.random_polygons(2400, seed=0)[:300]:
        by_size.setdefault((h, w), []).append([xy])
    out, n = [], 1
    for (h, w), objs in sorted(by_size.items()):
        while objs:
            out.append((h, w, objs[:n]))
            objs = objs[n:]
            n = n % 12 + 1
    return out


def test_named_and_random_cases_in_batches(ops):
    P, _ = _mods()
    sizes = set()
    for i, (h, w, objs) in enumerate(_groups()):
        K = 1 + i % 4
        per = [objs[j:j + K] for j in range(0, len(objs), K)]
        pb = P.PolygonBatch.from_lists(per, h, w, "cpu", K=K)
        sizes.add(pb.B * pb.K)
        _both_twice(ops, pb)
    assert min(sizes) == 1 and max(sizes) == 12 and len(sizes) >= 8


def test_overflow_keeps_offsets_whole_and_writes_nothing_past_the_capacity(ops):
    P, _ = _mods()
    pb = _shape_batch(65, 130)
    total = int(P.polygons_to_rle_definition(pb, capacity=15 * (65 * 130 + 1)).offsets[-1])
    d, _, enc, want = _both_twice(ops, pb, capacity=total - 1)
    assert enc.capacity == total - 1 and int(enc.offsets[-1]) == total
    with pytest.raises(P.PswinError, match=f"{total}.*{total - 1}"):
        enc.to_lists()


def test_one_capture_replayed_on_a_second_batch(ops):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _replay_body(side)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def _replay_body(side):
    from panoswintransformerobjectdetection_amd.graph import GraphedCallable
    P, rle = _mods()
    H, W, B, K = 65, 130, 2, 3
    first = [[[_scaled_star(64, H, W)], [_scaled_star(5, H, W), [1, 1, 40, 2, 30, 50]]], [[_scaled_star(257, H, W)]]]
    second = [[[[3, 3, 100, 8, 60, 60.5]]], [[_scaled_star(9, H, W)], [_scaled_star(300, H, W, 0.2)], [[0, 0, 20, 0, 20, 20, 0, 20], [10, 10, 129, 10, 129, 64]]]]
    buf = P.PolygonBatch.allocate(B, K, 8, 700, H, W, DEV)
    masks = torch.full((B, K, H, W), 0xFF, dtype=torch.uint8, device=DEV)
    enc = rle.RleMasks.allocate(B * K, H, W, DEV, B * K * (H * W + 1))
    buf.copy_from(first)

    def step():
        P.polygons_to_masks(buf, out=masks)
        P.polygons_to_rle(buf, out=enc)
        return enc.offsets

    g = GraphedCallable(step, warmup=2, stream=side, parameters=[])
    for ann in (second, first):                                                  # the other batch than the captured one first
        buf.copy_from(ann)
        masks.fill_(0xFF)
        enc.offsets.fill_(-7)
        g()
        side.synchronize()
        host = P.PolygonBatch.allocate(B, K, 8, 700, H, W, "cpu").copy_from(ann)
        want = P.polygons_to_rle_definition(host, capacity=enc.capacity)
        total = int(want.offsets[-1])
        assert torch.equal(masks.cpu(), P.polygons_to_masks_definition(host))
        assert torch.equal(enc.offsets.cpu(), want.offsets) and torch.equal(enc.runs[:total].cpu(), want.runs[:total])
        assert enc.to_lists() == want.to_lists()


# ---- wiring -------------------------------------------------------------------------------------------------------------------------
def test_with_targets_takes_a_polygon_batch_byte_for_byte(ops):
    from panoswintransformerobjectdetection_amd import pano_aug as A
    P, _ = _mods()
    B, h, w = 2, 64, 128
    rng = np.random.RandomState(5)
    imgs = torch.from_numpy(rng.randint(0, 256, (B, h, w, 3)).astype(np.uint8)).to(DEV)
    boxes = [np.array([[0, 10, 30, 50], [98, 10, 128, 50], [40, 20, 90, 60]], np.float32), np.array([[10, 5, 70, 40], [60, 30, 120, 62]], np.float32)]
    labels = [np.array([3, 3, 7], np.int64), np.array([1, 5], np.int64)]
    ann = [[[[0, 10, 30, 10, 30, 50, 0, 50]], [[98, 10, 128, 10, 128, 50], [99, 30, 120, 50, 98.5, 50]], [pc.star(16, 65, 40, 24, 12)]],
           [[[10, 5, 70, 5, 40, 40]], [pc.star(7, 90, 46, 29, 14)]]]
    pb = P.PolygonBatch.from_lists(ann, h, w, DEV, K=4)
    bitmaps = P.polygons_to_masks_definition(P.PolygonBatch.from_lists(ann, h, w, "cpu", K=4)).to(DEV)
    res = []
    for masks in (pb, bitmaps):
        t = A.PanoTrainTransform(img_scales=[(128, 256)], rng=np.random.RandomState(2))
        res.append(t.with_targets(imgs, [v.copy() for v in boxes], labels, masks))
    torch.cuda.synchronize()
    (x1, T1, _), (x2, T2, _) = res
    assert torch.equal(x1, x2) and torch.equal(T1.boxes, T2.boxes) and torch.equal(T1.labels, T2.labels) and torch.equal(T1.count, T2.count)
    assert T1.masks.any() and torch.equal(T1.masks, T2.masks)


def test_coco_accumulator_takes_polygon_ground_truth(ops):
    """CocoAccumulator(iou="segm") fed PaddedTargets(rle=polygons_to_rle(...)) gives the flags and curves of the bitmap route"""
    from panoswintransformerobjectdetection_amd import evaluation as ev
    from panoswintransformerobjectdetection_amd.detector import Detections, PaddedTargets
    P, _ = _mods()
    B, H, W, G, K, C = 2, 64, 80, 3, 4, 3
    box = lambda x0, y0, x1, y1: [x0, y0, x1, y0, x1, y1, x0, y1]
    gt_ann = [[[box(5, 5, 30, 40)], [pc.star(12, 55, 30, 22, 10)], [box(40, 2, 78, 20), box(60, 15, 79, 60)]], [[pc.star(9, 30, 30, 28, 9)], [box(50, 30, 75, 62)]]]
    det_ann = [[[box(6, 6, 31, 41)], [pc.star(12, 54, 31, 22, 10)], [box(0, 0, 20, 20)], [box(41, 2, 78, 21)]], [[box(49, 29, 75, 60)], [pc.star(9, 31, 30, 27, 9)]]]
    gts_p = P.PolygonBatch.from_lists(gt_ann, H, W, DEV, K=G)
    det_masks = P.polygons_to_masks(P.PolygonBatch.from_lists(det_ann, H, W, DEV, K=K))
    gt_labels = torch.tensor([[0, 1, 2], [1, 2, 0]], device=DEV)
    det_labels = torch.tensor([[0, 1, 0, 2], [2, 1, 0, 0]], device=DEV)
    det_count = torch.tensor([4, 2], dtype=torch.int32, device=DEV)
    scores = torch.linspace(0.9, 0.2, B * K, device=DEV).reshape(B, K)
    dets = Detections(torch.zeros(B, K, 4, device=DEV), scores, det_labels, det_count, torch.zeros(B, K, dtype=torch.int32, device=DEV), det_masks)
    zeros = torch.zeros(B, G, 4, device=DEV)
    ways = dict(polygons=PaddedTargets(zeros, gt_labels, gts_p.count, None, P.polygons_to_rle(gts_p)),
                bitmaps=PaddedTargets(zeros, gt_labels, gts_p.count, P.polygons_to_masks(gts_p)))
    got = {}
    for name, t in ways.items():
        acc = ev.CocoAccumulator(C, iou="segm", capacity_images=B, max_per_img=K, device=DEV)
        flags = acc.update(dets, t)
        e = acc.accumulate()
        assert int(acc.rle_overflow) == 0
        got[name] = (flags.cpu(), acc.rec_flags.cpu(), acc.num_gts.cpu(), torch.from_numpy(e["precision"]), torch.from_numpy(e["recall"]))
    assert (got["bitmaps"][0] & ev.FLAG_MATCHED).any()
    for a, b in zip(got["polygons"], got["bitmaps"]):
        assert torch.equal(a, b)
