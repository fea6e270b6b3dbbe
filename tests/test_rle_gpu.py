"""COCO run-length encoding on the MI355X (csrc/pswin_rle.hip through ops.rle_encode / ops.paste_masks_rle and
MiniMaskRCNN.heads_predict(mask_format=...)) against the definitions of rle.py computed once on the CPU.  Every comparison is equality:
offsets and every run with torch.equal.  The run pool is filled with the byte 0xA5 and allocated longer than its capacity, and must still
hold 0xA5 from offsets[N] on and from the capacity on; the workspace is filled with 0xFF before every call; every case runs twice for
identical bits.  Capacities come from the CPU definition's total for the case."""
import ctypes

import numpy as np
import pytest
import torch

import _rle_cases as rc
from _util import TINY

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 96


def _rle():
    from panoswintransformerobjectdetection_amd import rle
    return rle


def _poisoned_out(n_masks, H, W, capacity):
    runs = torch.empty(capacity + GUARD, dtype=torch.uint32, device=DEV)
    runs.view(torch.uint8).fill_(0xA5)
    return _rle().RleMasks(torch.full((n_masks + 1,), -7, dtype=torch.int64, device=DEV), runs, H, W, capacity=capacity)


def _truth(masks, count):
    """the CPU definition with room for every run: (offsets int64 [N + 1], runs uint32 [total])"""
    N = masks.numel() // (masks.shape[-1] * masks.shape[-2])
    enc = _rle().encode_masks_definition(masks, count, capacity=N * (masks.shape[-1] * masks.shape[-2] + 1))
    return enc.offsets, enc.runs[:int(enc.offsets[-1])]


def _check(enc, offsets, runs, capacity):
    """enc (on the device) against the truth under `capacity`: offsets whole; the masks below the cut whole; 0xA5 behind"""
    torch.cuda.synchronize()
    assert torch.equal(enc.offsets.cpu(), offsets)
    total = int(offsets[-1])
    got = enc.runs.cpu()
    below = offsets[offsets <= capacity]
    cut = int(below[-1])                                                         # the end of the last mask that lies below capacity
    assert torch.equal(got[:cut], runs[:cut])
    wrote = min(total, capacity)
    assert torch.equal(got[cut:wrote], runs[cut:wrote])                          # (a mask across the cut is written up to the cut)
    assert bool((got[wrote:].view(torch.uint8) == 0xA5).all())
    return got


def _run_twice(fn, n_masks, H, W, offsets, runs, capacity, ops):
    res = []
    for _ in range(2):
        out = _poisoned_out(n_masks, H, W, capacity)
        ops._rle_workspace(n_masks, H, W, torch.device(DEV)).fill_(0xFF)
        enc = fn(out)
        assert enc is out
        res.append(_check(enc, offsets, runs, capacity))
    assert torch.equal(res[0].view(torch.int32), res[1].view(torch.int32))
    return enc


# ---- the bitmap producer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", rc.GPU_H)
def test_rle_encode_of_bitmaps_equals_the_definition(ops, H):
    for W in rc.GPU_W:
        pats = rc.patterns(H, W)
        m3 = torch.from_numpy(np.stack(list(pats.values())))                    # [N, H, W]
        N = m3.shape[0]
        offsets, runs = _truth(m3, None)
        assert int(offsets[-1]) >= N
        dm = m3.to(DEV)
        _run_twice(lambda out: ops.rle_encode(dm, out=out), N, H, W, offsets, runs, max(int(offsets[-1]), 1), ops)
        # [B, K, H, W] with counts 0, partial and above K (clamped); the rows past the count hold 0xA5 and own no runs
        K = N
        count = torch.tensor([0, K // 2, K + 5], dtype=torch.int32)
        m4 = torch.stack([m3, m3.flip(0), m3])
        offsets4, runs4 = _truth(m4, count)
        assert int(offsets4[K]) == 0 and int(offsets4[K + K // 2]) == int(offsets4[2 * K])
        poisoned = m4.clone()
        poisoned[0] = 0xA5
        poisoned[1, K // 2:] = 0xA5
        d4, dc = poisoned.to(DEV), count.to(DEV)
        enc = _run_twice(lambda out: ops.rle_encode(d4, dc, out=out), 3 * K, H, W, offsets4, runs4, max(int(offsets4[-1]), 1), ops)
        assert (enc.B, enc.K) == (3, K) and enc.count is not None


def test_rle_encode_to_lists_and_the_dispatch(ops):
    rle = _rle()
    H, W = 65, 17
    m = torch.from_numpy(np.stack(list(rc.patterns(H, W).values())))
    enc = rle.encode_masks(m.to(DEV))                                            # default capacity, fresh buffers
    want = rle.encode_masks(m)
    torch.cuda.synchronize()
    assert enc.capacity == m.shape[0] * (30 * W + 1)
    if int(want.offsets[-1]) <= want.capacity:
        assert enc.to_lists() == want.to_lists()
    big = rle.encode_masks(m.to(DEV), capacity=m.shape[0] * (H * W + 1))
    assert big.to_lists() == rle.encode_masks(m, capacity=m.shape[0] * (H * W + 1)).to_lists()
    assert [d["counts"] for d in big.to_lists()[0]] == [rc.loop_to_string(rc.loop_encode(x)) for x in m.numpy()]


# ---- the fused producer -------------------------------------------------------------------------------------------------------
THRS = (0.5, 1.0, 0.0, -1.0)
LOGITS = ("noise", "blob", 30.0, -30.0)
LAYOUTS = (("f32", torch.float32, False), ("f32_cl", torch.float32, True), ("bf16", torch.bfloat16, False), ("bf16_cl", torch.bfloat16, True))


@pytest.mark.parametrize("H,W", [(96, 160), (33, 47), (64, 64), (65, 130), (1, 1)])
def test_paste_masks_rle_equals_paste_then_encode(ops, H, W):
    rle = _rle()
    B, K, C = 2, 5, 4
    N = B * K
    seed = 0
    runs_per_column = []
    for kind in LOGITS:
        for tag, dtype, channels_last in LAYOUTS:
            for thr in THRS:
                lg, labels, boxes, count = rc.paste_inputs(B, K, C, H, W, kind, seed)
                seed += 1
                dl = lg.to(dtype).to(DEV)
                if channels_last:
                    dl = dl.contiguous(memory_format=torch.channels_last)
                dlab, dbox, dcnt = labels.to(DEV), boxes.to(DEV), count.to(DEV)
                bitmaps = ops.paste_masks(dl, dlab, dbox, dcnt, thr, (H, W))
                via = ops.rle_encode(bitmaps, dcnt, capacity=N * (H * W + 1))    # kernel against kernel: bit equality is the claim
                torch.cuda.synchronize()
                offsets = via.offsets.cpu()
                runs = via.runs.cpu()[:int(offsets[-1])]
                toff, truns = _truth(bitmaps.cpu(), count)                       # ... and the bitmap route against the definition
                assert torch.equal(offsets, toff) and torch.equal(runs, truns)
                _run_twice(lambda out: ops.paste_masks_rle(dl, dlab, dbox, dcnt, thr, (H, W), out=out), N, H, W, offsets, runs,
                           max(int(offsets[-1]), 1), ops)
                if kind == "noise" and thr == 0.5:
                    runs_per_column.append(int(offsets[-1]) / (int(count.sum()) * W))
                if (H, W) == (1, 1):                                             # the smallest case: also the CPU definition of the paste
                    want = rle.paste_masks_rle(lg.to(dtype), labels, boxes, count, thr, (H, W), capacity=N * 2)
                    assert torch.equal(offsets, want.offsets) and torch.equal(runs, want.runs[:int(want.offsets[-1])]), (kind, tag, thr)
    print(f"{H} x {W}: runs per column of a live mask, noise logits at thr 0.5: {np.mean(runs_per_column):.2f}")


# ---- overflow -------------------------------------------------------------------------------------------------------------------
def test_overflow_keeps_offsets_whole_and_the_guard_band_intact(ops):
    from panoswintransformerobjectdetection_amd._lib import PswinError
    H, W, B, K, C = 65, 130, 2, 5, 4
    lg, labels, boxes, count = rc.paste_inputs(B, K, C, H, W, "noise", 0)
    from panoswintransformerobjectdetection_amd import detector
    bitmaps = detector.paste_masks_batch(lg, labels, boxes, count, 0.5, (H, W))
    offsets, runs = _truth(bitmaps, count)                                       # the CPU definition's total sizes the pool
    cap = int(offsets[-1]) // 2
    whole = int((offsets[1:] <= cap).sum())
    assert 0 < whole < B * K
    db, dc = bitmaps.to(DEV), count.to(DEV)
    enc = _run_twice(lambda out: ops.rle_encode(db, dc, out=out), B * K, H, W, offsets, runs, cap, ops)
    with pytest.raises(PswinError, match=f"{int(offsets[-1])}.*{cap}"):
        enc.to_lists()
    # the fused producer: the pool is half of what the CPU definition needs for the bitmaps the paste kernel writes for these inputs
    dl, dlab, dbox = lg.to(DEV), labels.to(DEV), boxes.to(DEV)
    pasted = ops.paste_masks(dl, dlab, dbox, dc, 0.5, (H, W))
    voff, vruns = _truth(pasted.cpu(), count)
    vcap = int(voff[-1]) // 2
    assert 0 < int((voff[1:] <= vcap).sum()) < B * K
    enc = _run_twice(lambda out: ops.paste_masks_rle(dl, dlab, dbox, dc, 0.5, (H, W), out=out), B * K, H, W, voff, vruns, vcap, ops)
    with pytest.raises(PswinError, match=f"{int(voff[-1])}.*{vcap}"):
        enc.to_lists()


# ---- refused arguments ----------------------------------------------------------------------------------------------------------
def test_refused_arguments_return_the_error_code_and_touch_nothing(ops):
    from panoswintransformerobjectdetection_amd import _lib
    from panoswintransformerobjectdetection_amd._lib import PswinError
    lib = _lib.load()
    H, W, N = 8, 16, 3
    masks = torch.ones(N, H, W, dtype=torch.uint8, device=DEV)
    out = _poisoned_out(N, H, W, 64)
    ws = ops._rle_workspace(N, H, W, torch.device(DEV))
    ws.fill_(0xFF)
    count = torch.ones(1, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ok = [p(masks), None, N, 1, H, W, p(out.offsets), p(out.runs), 64, p(ws), None]
    bad = {"masks": (0, None), "N": (2, 0), "H": (4, 0), "W": (5, 65537), "offsets": (6, None), "offsets align": (6, ctypes.c_void_p(out.offsets.data_ptr() + 4)),
           "runs": (7, None), "runs align": (7, ctypes.c_void_p(out.runs.data_ptr() + 2)), "capacity": (8, 0), "workspace": (9, None),
           "workspace align": (9, ctypes.c_void_p(ws.data_ptr() + 8))}
    for name, (i, v) in bad.items():
        args = list(ok)
        args[i] = v
        assert lib.pswin_rle_encode(*args) == -1, name
    args = list(ok)
    args[1], args[3] = p(count), 2                                               # K must divide N
    assert lib.pswin_rle_encode(*args) == -1
    lg = torch.zeros(N, 2, 28, 28, device=DEV)
    labels, boxes = torch.zeros(1, N, dtype=torch.int64, device=DEV), torch.zeros(1, N, 4, device=DEV)
    okp = [p(lg), 0, 2 * 784, 784, 28, 1, p(labels), p(boxes), p(count), 1, N, 2, H, W, 0.5, p(out.offsets), p(out.runs), 64, p(ws), None]
    for name, (i, v) in {"logits": (0, None), "dtype": (1, 5), "stride": (2, 0), "count": (8, None), "K": (10, 1025), "C": (11, 129),
                         "H": (12, 65537), "capacity": (17, 0), "runs": (16, None)}.items():
        args = list(okp)
        args[i] = v
        assert lib.pswin_paste_masks_rle(*args) == -1, name
    nbytes = ctypes.c_longlong(-5)
    assert lib.pswin_rle_workspace(0, H, W, ctypes.byref(nbytes)) == -1 and lib.pswin_rle_workspace(N, 65536, 65536, ctypes.byref(nbytes)) == -1
    assert lib.pswin_rle_workspace(N, H, W, None) == -1 and nbytes.value == -5
    torch.cuda.synchronize()
    assert bool((out.runs.view(torch.uint8) == 0xA5).all()) and bool((out.offsets == -7).all()) and bool((ws == 0xFF).all())
    # the wrappers raise before the device is touched
    assert ops.rle_supported(800, 512, 1024, 100, 80) and not ops.rle_supported(1, 65536, 65536) and not ops.rle_supported(1, 65537, 1)
    assert not ops.rle_supported(10, 8, 8, 1025, 80) and not ops.rle_supported(10, 8, 8, 5, 129)
    with pytest.raises(PswinError):
        ops.rle_encode(masks.float())
    with pytest.raises(PswinError):
        ops.rle_encode(masks, out=_poisoned_out(N + 1, H, W, 64))
    with pytest.raises(PswinError):
        ops.rle_encode(masks, capacity=0)
    with pytest.raises(PswinError):
        ops.paste_masks_rle(torch.zeros(N, 129, 28, 28, device=DEV), labels, boxes, count, 0.5, (H, W))


# ---- heads_predict(mask_format=...) captured once and replayed ----------------------------------------------------------------------
FC_CLS_SCALE, BACKGROUND_BIAS = 300.0, 16.0                                      # as tests/test_detect_post_gpu.py: so that images yield detections


def _same_results(a, b):
    assert len(a) == len(b)
    for (ab, asg), (bb, bsg) in zip(a, b):
        assert len(ab) == len(bb) and all(np.array_equal(x, y) for x, y in zip(ab, bb))
        assert asg == bsg


def test_heads_predict_in_rle_format_is_captured_and_equals_the_bitmap_format(ops):
    """The three formats in one captured step, replayed on two inputs.  The formats are compared on the tensors of ONE forward pass (each
    format's results against the other format's hook applied to that pass's mask logits, labels, boxes and count), because two passes
    over the same features do not give the same detections, with or without this format: measured on an MI355X, two eager
    heads_predict(mask_format="bitmap") calls on these features differ in rois by up to 212 pixels, in cls by up to 9.8, in labels and in
    boxes (the RPN's convolutions are not reproducible from call to call, and near-tied proposals then change places), and a replay
    differs from an eager call in the same way."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _replay_body(side, ops)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def _replay_body(side, ops):
    from panoswintransformerobjectdetection_amd import detector as det
    from panoswintransformerobjectdetection_amd.graph import GraphedCallable
    B, H, W = 2, 128, 256
    torch.manual_seed(0)
    m = det.MiniMaskRCNN(dict(TINY, compute_dtype=torch.float32), num_classes=80).to(DEV).eval()
    with torch.no_grad():
        m.bbox_head.cls.weight.mul_(FC_CLS_SCALE)
        m.bbox_head.cls.bias[m.num_classes] += BACKGROUND_BIAS
    C = m.num_classes
    gen = torch.Generator().manual_seed(7)
    sets = [[torch.randn(B, c, H // s, W // s, generator=gen) for c, s in zip(m.backbone.num_features, (4, 8, 16, 32))] for _ in range(2)]
    feats = [f.to(DEV) for f in sets[0]]
    state = {}

    def step():
        state["rle"] = m.heads_predict(feats, (H, W), mask_format="rle", return_raw=True)
        state["bitmap"] = m.heads_predict(feats, (H, W), return_raw=True)
        state["both"] = m.heads_predict(feats, (H, W), mask_format="both")
        return state["rle"][0].count

    thr = m.test_cfg["rcnn"]["mask_thr_binary"]
    g = GraphedCallable(step, warmup=2, stream=side, parameters=[])
    for fs in sets[::-1]:                                                        # the other feature maps than the captured ones first
        for dst, src in zip(feats, fs):
            dst.copy_(src.to(DEV))
        g()
        side.synchronize()
        # "rle": no bitmap; its results equal those of the bitmap format's own hook (m.paste) on the tensors this pass pasted
        out, raw = state["rle"]
        assert out.masks is None and out.rle is not None and (out.rle.B, out.rle.K) == (B, out.boxes.shape[1])
        assert bool((out.count > 0).all()), "an image without detections (FC_CLS_SCALE, BACKGROUND_BIAS)"
        got = out.as_results(C)
        masks = m.paste(raw["mask_logits"], out.labels, out.boxes, out.count, thr, (H, W))
        _same_results(got, det.Detections(out.boxes, out.scores, out.labels, out.count, out.source, masks).as_results(C))
        # "bitmap", the default: no runs; its results (as_results encodes the bitmaps) equal those of the rle format's hook on its tensors
        plain, praw = state["bitmap"]
        assert plain.rle is None and plain.masks is not None and plain.masks.dtype == torch.uint8
        enc = m.paste_rle(praw["mask_logits"], plain.labels, plain.boxes, plain.count, thr, (H, W))
        _same_results(plain.as_results(C), det.Detections(plain.boxes, plain.scores, plain.labels, plain.count, plain.source, rle=enc).as_results(C))
        # "both" agrees with itself
        both = state["both"]
        assert both.masks is not None and both.rle is not None
        _same_results(both.as_results(C), det.Detections(both.boxes, both.scores, both.labels, both.count, both.source, both.masks).as_results(C))
        print(f"detections {out.count.tolist()}, runs {int(out.rle.offsets[-1])} of capacity {out.rle.capacity}")
