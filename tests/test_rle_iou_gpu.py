"""Run-length IoU on the MI355X (csrc/pswin_rle_iou.hip through evaluation.rle_inter_pairs_dispatch, pair_iou_dispatch and both
accumulators) against the definitions of rle.py computed on the CPU.  Every comparison is equality.  In the kernel cases the outputs are
filled with the byte 0xA5 and the workspace with 0xFF before every call, and every case runs twice for identical bits.  The batches come
from tests/_rle_iou_cases.py, where tests/test_rle_iou.py rehearses them on a restatement of the kernels' passes."""
import ctypes

import numpy as np
import pytest
import torch

import _rle_cases as rc
import _rle_iou_cases as ric
from _util import TINY

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 96


def _mods():
    from panoswintransformerobjectdetection_amd import evaluation, rle
    return evaluation, rle


def _dets(labels, count, masks=None, enc=None, scores=None):
    from panoswintransformerobjectdetection_amd.detector import Detections
    B, K = labels.shape
    scores = torch.linspace(0.9, 0.1, B * K).reshape(B, K) if scores is None else scores
    t = lambda x: None if x is None else x.to(DEV)
    return Detections(torch.zeros(B, K, 4, device=DEV), t(scores), t(labels), t(count), torch.zeros(B, K, dtype=torch.int32, device=DEV), t(masks),
                      enc)


def _gts(labels, count, masks=None, enc=None):
    from panoswintransformerobjectdetection_amd.detector import PaddedTargets
    t = lambda x: None if x is None else x.to(DEV)
    return PaddedTargets(torch.zeros(labels.shape + (4,), device=DEV), t(labels), t(count), t(masks), enc)


def _to_dev(enc, capacity=None, guard=0, sentinel=None):
    """a CPU RleMasks on the device with `capacity` (default: what the batch needs), the pool `guard` elements longer and `sentinel` behind
    the capacity"""
    _, rle = _mods()
    cap = max(int(enc.offsets[-1]), 1) if capacity is None else capacity
    runs = torch.zeros(cap + guard, dtype=torch.int64)
    if sentinel is not None:
        runs[cap:] = sentinel
    n = min(cap, int(enc.offsets[-1]))
    runs[:n] = enc.runs[:n].to(torch.int64)
    runs = runs.to(torch.uint32).to(DEV)
    count = None if enc.count is None else enc.count.to(DEV)
    return rle.RleMasks(enc.offsets.to(DEV), runs, enc.height, enc.width, capacity=cap, B=enc.B, K=enc.K, count=count)


def _poisoned(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(0xA5)
    return t


def _inter_twice(de, dl, dc, ge, gl, gc):
    """pswin_rle_inter_pairs twice on poisoned outputs and a workspace of 0xFF -> (inter, areas, overflow) on the CPU"""
    ev, _ = _mods()
    (B, K), G = dl.shape, gl.shape[1]
    d, g = _dets(dl, dc, enc=de), _gts(gl, gc, enc=ge)
    res = []
    for _ in range(2):
        out = (_poisoned((B, K, G), torch.int32), _poisoned((B, K + G), torch.int32), torch.zeros(1, dtype=torch.int32, device=DEV))
        ws = ev.rle_inter_workspace(B, K, G, de.capacity, ge.capacity, DEV).fill_(0xFF)
        got = ev.rle_inter_pairs_dispatch(d, g, out=out, workspace=ws)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == out[0].data_ptr() and got[2].data_ptr() == out[2].data_ptr()
        res.append([t.cpu() for t in got])
    assert all(torch.equal(a, b) for a, b in zip(*res))
    return res[0]


def _iou_twice(de, dl, dc, ge, gl, gc):
    ev, _ = _mods()
    (B, K), G = dl.shape, gl.shape[1]
    d, g = _dets(dl, dc, enc=de), _gts(gl, gc, enc=ge)
    res = []
    for _ in range(2):
        out = (_poisoned((B, K, G), torch.float32), _poisoned((B, K), torch.float32), _poisoned((B, G), torch.float32))
        over = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = ev.pair_iou_dispatch(d, g, "segm", out=out, rle_overflow=over)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == out[0].data_ptr()
        res.append([t.cpu() for t in got] + [over.cpu()])
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*res))
    return res[0]


# ---- the kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", ric.PATTERN_H)
def test_all_patterns_against_all_patterns_equal_the_definition(ops, H):
    """K = G = 18, the number of patterns (one more than the 17 the kernels were specified at), B = 2, the second image with fewer
    detections and no boxes; labels alternate over two classes, the targets' once in step and once out of step with the detections'.
    hstripe1 has 63 / 64 / 65 foreground runs per column set at H = 130 / W = 1 and around; zeros has a table of one entry, ones of two."""
    _, rle = _mods()
    for W in ric.PATTERN_W:
        for shift in (0, 1):
            dm, dl, dc, gm, gl, gc = ric.pattern_batch(H, W, shift)
            room = dm.shape[0] * dm.shape[1] * (H * W + 1)
            de, ge = rle.encode_masks(dm, dc, capacity=room), rle.encode_masks(gm, gc, capacity=room)
            want = rle.inter_pairs_definition(de, dl, dc, ge, gl, gc)             # checked on the CPU before the device is asked
            assert (want[0][dl[:, :, None] == gl[:, None, :]] > 0).any() and (want[0] == -1).any() and want[2].tolist() == [0]
            got = _inter_twice(_to_dev(de), dl, dc, _to_dev(ge), gl, gc)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2].tolist() == [0], (H, W, shift)


def test_run_counts_around_the_staged_table(ops):
    """The pair kernel keeps a detection's table of up to S = pswin_rle_inter_stage() entries in LDS and searches a longer one in global
    memory: masks of S - 1, S, S + 1 and 2 S + 5 runs (a checkerboard's scan with its tail blanked), the whole 130 x 65 checkerboard that
    starts with 1 (8,387 runs) and `ones`, each against each, on either side"""
    from panoswintransformerobjectdetection_amd import _lib
    _, rle = _mods()
    S = _lib.load().pswin_rle_inter_stage()
    H, W = 130, 65
    per = ric.stage_masks(H, W, S)
    N = len(per)
    enc = rle.RleMasks.from_lists(ric.lists_of([per], H, W), "cpu")
    assert [int(v) for v in enc.offsets.diff()] == [S - 1, S, S + 1, 2 * S + 5, len(per[4]), 2]
    labels, count = torch.zeros(1, N, dtype=torch.long), torch.tensor([N], dtype=torch.int32)
    want = rle.inter_pairs_definition(enc, labels, count, enc, labels, count)
    assert torch.equal(want[0][0].diagonal(), want[1][0, :N]) and (want[0] > 0).all()
    got = _inter_twice(_to_dev(enc), labels, count, _to_dev(enc), labels, count)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2].tolist() == [0]


def test_one_realistic_batch_equals_the_bitmap_kernels_bit_for_bit(ops):
    """paste_masks_rle of 2 x 100 detections against 32 blobs per image: the integers against the definition, and iou / det_area / gt_area
    of pswin_rle_iou_pairs against pswin_mask_iou_pairs on the decoded bitmaps"""
    ev, rle = _mods()
    B, K, C, H, W, G = 2, 100, 3, 64, 96, 32
    lg, dl, boxes, dc = rc.paste_inputs(B, K, C, H, W)
    de = ops.paste_masks_rle(lg.to(DEV), dl.to(DEV), boxes.to(DEV), dc.to(DEV), 0.5, (H, W))
    gm = torch.from_numpy(ric.blob_masks(B, G, H, W))
    gl, gc = (torch.arange(B * G).reshape(B, G) * 5 % C).long(), torch.tensor([G, G - 12], dtype=torch.int32)
    ge = rle.encode_masks(gm.to(DEV), gc.to(DEV))
    torch.cuda.synchronize()
    host_d = rle.RleMasks(de.offsets.cpu(), de.runs.cpu(), H, W, de.capacity, B, K, dc)
    host_g = rle.RleMasks(ge.offsets.cpu(), ge.runs.cpu(), H, W, ge.capacity, B, G, gc)
    want = rle.inter_pairs_definition(host_d, dl, dc, host_g, gl, gc)
    assert (want[0] > 0).sum() > 50 and want[2].tolist() == [0]
    got = _inter_twice(de, dl, dc, ge, gl, gc)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2].tolist() == [0]
    counts = host_d.mask_counts()
    dm = torch.zeros(B, K, H, W, dtype=torch.uint8)
    for b in range(B):
        for k in range(int(dc[b])):
            dm[b, k] = torch.from_numpy(rle.rle_decode(counts[b * K + k], H, W))
    bit = [t.cpu() for t in ev.pair_iou_dispatch(_dets(dl, dc, dm), _gts(gl, gc, gm), "segm")]
    iou = _iou_twice(de, dl, dc, ge, gl, gc)
    for a, b in zip(iou[:3], bit):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert iou[3].tolist() == [0] and ((bit[0] > 0) & (bit[0] < 1)).any()


def test_a_pool_that_cuts_the_last_live_mask(ops):
    """The detections' pool is GUARD elements longer than its capacity and holds run lengths of 0xA5A5A5A5 behind it; the capacity ends
    inside the last live mask: the flag is 1, that mask is empty, every other result stands; with room the flag stays 0"""
    _, rle = _mods()
    H, W = 65, 17
    dm, dl, dc, gm, gl, gc = ric.pattern_batch(H, W)
    room = dm.shape[0] * dm.shape[1] * (H * W + 1)
    de, ge = rle.encode_masks(dm, dc, capacity=room), rle.encode_masks(gm, gc, capacity=room)
    total = int(de.offsets[-1])
    cut = rle.RleMasks(de.offsets, de.runs, H, W, capacity=total - 1, B=de.B, K=de.K, count=dc)
    want = rle.inter_pairs_definition(cut, dl, dc, ge, gl, gc)
    whole = rle.inter_pairs_definition(de, dl, dc, ge, gl, gc)
    last = int(dc[1]) - 1
    assert want[2].tolist() == [1] and int(want[1][1, last]) == 0 and int(whole[1][1, last]) > 0 and torch.equal(want[1][0], whole[1][0])
    assert torch.equal(want[0][0], whole[0][0]) and (whole[0][0] > 0).any()
    got = _inter_twice(_to_dev(de, total - 1, GUARD, 0xA5A5A5A5), dl, dc, _to_dev(ge), gl, gc)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2].tolist() == [1]
    got = _inter_twice(_to_dev(de, total, GUARD, 0xA5A5A5A5), dl, dc, _to_dev(ge), gl, gc)
    assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1]) and got[2].tolist() == [0]


def test_refused_arguments_return_the_error_code_and_touch_nothing(ops):
    from panoswintransformerobjectdetection_amd import _lib
    ev, rle = _mods()
    lib = _lib.load()
    B, K, G, H, W = 1, 2, 3, 4, 5
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    offs_d, offs_g = torch.zeros(B * K + 1, dtype=torch.int64, device=DEV), torch.zeros(B * G + 1, dtype=torch.int64, device=DEV)
    runs = torch.zeros(64, dtype=torch.uint32, device=DEV)
    labels, count = torch.zeros(8, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    inter, areas, over = _poisoned((B, K, G), torch.int32), _poisoned((B, K + G), torch.int32), _poisoned((1,), torch.int32)
    iou, da, ga = _poisoned((B, K, G), torch.float32), _poisoned((B, K), torch.float32), _poisoned((B, G), torch.float32)
    ws = ev.rle_inter_workspace(B, K, G, 64, 64, DEV).fill_(0xFF)
    head = [p(offs_d), p(runs), 64, p(labels), p(count), p(offs_g), p(runs), 64, p(labels), p(count), B, K, G, H, W]
    ok_inter = head + [p(inter), p(areas), p(over), p(ws), None]
    ok_iou = head + [p(iou), p(da), p(ga), p(over), p(ws), None]
    bad = {"det_offsets": (0, None), "det_runs": (1, None), "det capacity": (2, 0), "det_labels": (3, None), "det_count": (4, None),
           "gt_offsets": (5, None), "gt_runs": (6, None), "gt capacity": (7, 0), "gt_labels": (8, None), "gt_count": (9, None), "B": (10, 0),
           "K": (11, 0), "K max": (11, ev.COCO_MAX_K + 1), "G": (12, 0), "G max": (12, ev.COCO_MAX_G + 1), "H": (13, 0), "H W": (13, 1 << 29),
           "offsets align": (0, ctypes.c_void_p(offs_d.data_ptr() + 4)), "runs align": (1, ctypes.c_void_p(runs.data_ptr() + 2))}
    for name, (i, v) in bad.items():
        for fn, ok in ((lib.pswin_rle_inter_pairs, ok_inter), (lib.pswin_rle_iou_pairs, ok_iou)):
            args = list(ok)
            args[i] = v
            if name == "H W":
                args[14] = 4                                                    # 2^29 x 4 = 2^31 pixels
            assert fn(*args) == -1, name
    for i in (15, 16, 17, 18):                                                  # inter, areas, overflow, workspace
        args = list(ok_inter)
        args[i] = None
        assert lib.pswin_rle_inter_pairs(*args) == -1, i
    for i in (15, 16, 17, 18, 19):                                              # iou, det_area, gt_area, overflow, workspace
        args = list(ok_iou)
        args[i] = None
        assert lib.pswin_rle_iou_pairs(*args) == -1, i
    args = list(ok_inter)
    args[18] = ctypes.c_void_p(ws.data_ptr() + 8)
    assert lib.pswin_rle_inter_pairs(*args) == -1
    nbytes = ctypes.c_longlong(-5)
    assert lib.pswin_rle_inter_workspace(B, K, G, 0, 64, ctypes.byref(nbytes)) == -1 and lib.pswin_rle_inter_workspace(B, K, G, 64, 64, None) == -1
    assert lib.pswin_rle_inter_workspace(B, 1025, G, 64, 64, ctypes.byref(nbytes)) == -1 and nbytes.value == -5
    assert lib.pswin_rle_inter_workspace(B, K, G, 64, 64, ctypes.byref(nbytes)) == 0 and nbytes.value == ws.numel()
    torch.cuda.synchronize()
    for t in (inter, areas, over, iou, da, ga):
        assert bool((t.view(torch.uint8) == 0xA5).all())
    assert bool((ws == 0xFF).all())
    assert lib.pswin_rle_inter_pairs(*ok_inter) == 0                            # and the arguments that were varied are good ones
    torch.cuda.synchronize()
    assert bool((inter == -1).all()) and bool((areas == 0).all())


# ---- the accumulators -------------------------------------------------------------------------------------------------------------
def _case_on_device(pair):
    _, rle = _mods()
    d, t = pair
    enc = lambda e: None if e is None else _to_dev(e, e.capacity)
    return (_dets(d.labels, d.count, d.masks, enc(d.rle), d.scores), _gts(t.labels, t.count, t.masks, enc(t.rle)))


def test_accumulators_from_runs_equal_the_accumulators_from_bitmaps(ops):
    ev, _ = _mods()
    ways, crowd, gt_area = ric.scoring_case()
    kw = dict(area_ranges=((0.0, 1e10), (0.0, 60.0), (60.0, 200.0), (200.0, 1e10)), max_dets=(1, 3, 100))
    coco, voc = {}, {}
    for name, pair in ways.items():
        d, t = _case_on_device(pair)
        acc = ev.CocoAccumulator(3, iou="segm", capacity_images=2, max_per_img=8, device=DEV, **kw)
        flags = acc.update(d, t, crowd.to(DEV), gt_area.to(DEV))
        e = acc.accumulate()
        coco[name] = (flags.cpu(), acc.rec_flags.cpu(), acc.rec_rank.cpu(), acc.num_gts.cpu(), e["precision"], e["recall"])
        assert int(acc.rle_overflow) == 0
        m = ev.MapAccumulator(3, iou_thrs=(0.5, 0.75), scale_ranges=((0, 8), (8, 1000)), capacity_images=2, max_per_img=8, iou="segm", device=DEV)
        marks = m.update(d, t, crowd.to(DEV))
        voc[name] = (marks.cpu(), m.rec_marks.cpu(), m.num_gts.cpu(), m.summarize()["ap"])
    cpu = ev.CocoAccumulator(3, iou="segm", capacity_images=2, max_per_img=8, device="cpu", **kw)
    want_flags = cpu.update(*ways["rle"], crowd, gt_area)
    assert torch.equal(coco["rle"][0], want_flags) and (want_flags & ev.FLAG_MATCHED).any()
    for name in ways:
        for a, b in zip(coco[name], coco["bitmaps"]):
            assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)), name
        for a, b in zip(voc[name], voc["bitmaps"]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name


def test_a_captured_update_from_runs_follows_the_refilled_buffers(ops):
    """update from runs alone in a graph on one stream; the run pools, offsets, labels, scores and counts are then refilled with a second
    batch of other counts and other run totals inside the same capacities, and the replay's flags are the CPU definition's for it"""
    ev, rle = _mods()
    H, W, B, K, G = 16, 24, 2, 8, 5
    batches = []
    for seed, drop in ((3, 0), (11, 2)):
        ways, crowd, gt_area = ric.scoring_case(seed, drop)
        batches.append((ways["rle"], crowd, gt_area))
    (d0, t0), (d1, t1) = batches[0][0], batches[1][0]
    assert d0.count.tolist() != d1.count.tolist() and t0.count.tolist() != t1.count.tolist()
    assert int(d0.rle.offsets[-1]) != int(d1.rle.offsets[-1]) and int(t0.rle.offsets[-1]) != int(t1.rle.offsets[-1])
    cap_d = max(int(d0.rle.offsets[-1]), int(d1.rle.offsets[-1])) + 7
    cap_g = max(int(t0.rle.offsets[-1]), int(t1.rle.offsets[-1])) + 7
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        de, ge = _to_dev(d0.rle, cap_d), _to_dev(t0.rle, cap_g)
        dets, gts = _dets(d0.labels.clone(), d0.count.clone(), None, de, d0.scores.clone()), _gts(t0.labels.clone(), t0.count.clone(), None, ge)
        crowd, gt_area = batches[0][1].to(DEV), batches[0][2].to(DEV)
        acc = ev.CocoAccumulator(3, iou="segm", capacity_images=4, max_per_img=K, device=DEV)
        acc.update(dets, gts, crowd, gt_area)                                   # warm-up outside the capture
        acc.reset()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            flags = acc.update(dets, gts, crowd, gt_area)
        for (d, t), cr, ga in batches[::-1]:                                    # the other batch than the captured one first
            de.offsets.copy_(d.rle.offsets), ge.offsets.copy_(t.rle.offsets)
            de.runs.zero_(), ge.runs.zero_()
            de.runs[:int(d.rle.offsets[-1])].copy_(d.rle.runs[:int(d.rle.offsets[-1])])
            ge.runs[:int(t.rle.offsets[-1])].copy_(t.rle.runs[:int(t.rle.offsets[-1])])
            dets.labels.copy_(d.labels), dets.count.copy_(d.count), dets.scores.copy_(d.scores)
            gts.labels.copy_(t.labels), gts.count.copy_(t.count), crowd.copy_(cr), gt_area.copy_(ga)
            graph.replay()
            side.synchronize()
            cpu = ev.CocoAccumulator(3, iou="segm", capacity_images=4, max_per_img=K, device="cpu")
            want = cpu.update(d, t, cr, ga)
            assert torch.equal(flags.cpu(), want) and (want & ev.FLAG_MATCHED).any()
        assert int(acc.cursor) == 2 * B and int(acc.rle_overflow) == 0 and int(acc.overflow) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_end_to_end_runs_and_bitmaps_of_one_pass_score_alike(ops):
    """ONE heads_predict(mask_format="both") pass of the tiny detector (two passes over the same features do not agree on an MI355X:
    tests/test_rle_gpu.py): its detections with the runs alone and with the bitmaps alone, scored against the same targets"""
    from panoswintransformerobjectdetection_amd import detector as det
    ev, _ = _mods()
    B, H, W, G = 2, 128, 256, 6
    torch.manual_seed(0)
    m = det.MiniMaskRCNN(dict(TINY, compute_dtype=torch.float32), num_classes=80).to(DEV).eval()
    with torch.no_grad():
        m.bbox_head.cls.weight.mul_(300.0)                                      # as tests/test_rle_gpu.py: so that images yield detections
        m.bbox_head.cls.bias[m.num_classes] += 16.0
    gen = torch.Generator().manual_seed(7)
    feats = [torch.randn(B, c, H // s, W // s, generator=gen).to(DEV) for c, s in zip(m.backbone.num_features, (4, 8, 16, 32))]
    with torch.no_grad():
        both = m.heads_predict(feats, (H, W), mask_format="both")
    torch.cuda.synchronize()
    K, C = both.boxes.shape[1], m.num_classes
    assert both.masks is not None and both.rle is not None and bool((both.count > 0).all())
    n = [min(int(c), G) for c in both.count]
    gm = torch.from_numpy(ric.blob_masks(B, G, H, W, seed=1))
    gl = torch.zeros(B, G, dtype=torch.long)
    for b in range(B):                                                          # boxes of the detections' classes, three of them their masks
        gl[b, :n[b]] = both.labels[b, :n[b]].cpu()
        gm[b, :min(3, n[b])] = both.masks[b, :min(3, n[b])].cpu()
    gts = _gts(gl, torch.tensor(n, dtype=torch.int32), gm)
    crowd = torch.zeros(B, G, dtype=torch.bool, device=DEV)
    crowd[:, 1] = True
    res = []
    for masks, enc in ((None, both.rle), (both.masks, None)):
        d = det.Detections(both.boxes, both.scores, both.labels, both.count, both.source, masks, enc)
        acc = ev.CocoAccumulator(C, iou="segm", capacity_images=B, max_per_img=K, device=DEV)
        res.append((acc.update(d, gts, crowd).cpu(), acc.rec_flags.cpu(), acc.num_gts.cpu()))
        assert int(acc.rle_overflow) == 0
    assert all(torch.equal(a, b) for a, b in zip(*res)) and (res[0][0] & ev.FLAG_MATCHED).any()
