"""The evaluation kernels (csrc/pswin_eval.hip through panoswintransformerobjectdetection_amd/evaluation.py) against the definitions of the
same module on the same inputs: pair IoUs bit for bit, marks byte for byte, AP within one float32 spacing, the accumulator against the CPU
definition, a captured update against eager calls.  Every output buffer is pre-filled with a non-zero byte pattern, so that a row the
kernel did not write shows.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from panoswintransformerobjectdetection_amd import evaluation as ev
from panoswintransformerobjectdetection_amd._lib import PswinError

import _eval_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRS = (0.5, 0.75, 0.95)
RANGES = ((0.0, 32.0), (32.0, 65536.0))          # scale ranges: their squares 0, 1024 and 2^32 are exact in float32
K = 100


def _pattern(shape, dtype):
    """a buffer whose every byte is 0xA5"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV).view(dtype).reshape(shape)


def _spacing_ok(got, want):
    want = want.numpy() if torch.is_tensor(want) else want
    return np.all(np.abs(got.numpy().astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want).astype(np.float32)))


@pytest.fixture(scope="module")
def golden():
    return cases.load_golden()


# ---- pair IoU and match -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[1, 5, 64, 65, 130])
def pair(request):
    """one case per Gmax: the inputs and the definitions' results on the CPU, computed once"""
    Gmax = request.param
    dets, gts, ignore = cases.pair_case(Gmax, K=K)
    iou = ev.box_iou_pairs(dets, gts)
    da, ga = ev.box_areas(dets.boxes), ev.box_areas(gts.boxes)
    area_ranges = [(a * a, b * b) for a, b in RANGES]
    want = {False: ev.match_pairs(iou, dets, gts, ignore, THRS, None, da, ga), True: ev.match_pairs(iou, dets, gts, ignore, THRS, area_ranges, da, ga)}
    if Gmax >= 5:
        best = iou.max(2)[0]
        assert all((best == float(np.float32(t))).any() for t in THRS)                  # best IoUs exactly on every threshold
    return dict(Gmax=Gmax, dets=dets, gts=gts, ignore=ignore, iou=iou, da=da, ga=ga, marks=want, area_ranges=area_ranges)


def test_box_iou_pairs_bit_for_bit(pair):
    dets, gts = cases.to_device(pair["dets"], DEV), cases.to_device(pair["gts"], DEV)
    G = pair["Gmax"]
    out = (_pattern((3, K, G), torch.float32), _pattern((3, K), torch.float32), _pattern((3, G), torch.float32))
    iou, da, ga = ev.pair_iou_dispatch(dets, gts, "bbox", out=out)
    assert iou.data_ptr() == out[0].data_ptr()
    assert torch.equal(iou.cpu().view(torch.int32), pair["iou"].view(torch.int32))
    assert torch.equal(da.cpu().view(torch.int32), pair["da"].view(torch.int32)) and torch.equal(ga.cpu().view(torch.int32), pair["ga"].view(torch.int32))


@pytest.mark.parametrize("ranged", [False, True])
def test_match_byte_for_byte(pair, ranged):
    dets, gts, ignore = cases.to_device(pair["dets"], DEV), cases.to_device(pair["gts"], DEV), pair["ignore"].to(DEV)
    C, S = 4, 2 if ranged else 1
    acc = ev.MapAccumulator(C, iou_thrs=THRS, scale_ranges=RANGES if ranged else None, capacity_images=4, max_per_img=K, device=DEV)
    for buf in (acc.rec_score, acc.rec_label, acc.rec_marks):
        buf.copy_(_pattern(buf.shape, buf.dtype))
    acc.cursor.fill_(1)                                                          # the batch goes to slots 1 .. 3
    out = _pattern((len(THRS), S, 3, K), torch.uint8)
    marks = acc.update(dets, gts, ignore, out=out)
    want = pair["marks"][ranged]
    assert marks.data_ptr() == out.data_ptr() and torch.equal(marks.cpu(), want)
    assert int(acc.cursor) == 4 and int(acc.overflow) == 0
    # the records: slots 1 .. 3 hold the batch, slot 0 keeps the pattern
    assert torch.equal(acc.rec_marks[:, :, 1:].cpu(), want)
    live = torch.arange(K)[None] < pair["dets"].count[:, None]
    assert torch.equal(acc.rec_label[1:].cpu(), torch.where(live, pair["dets"].labels, C).to(torch.int32))
    assert torch.equal(acc.rec_score[1:].cpu(), torch.where(live, pair["dets"].scores, torch.zeros(())))
    assert (acc.rec_marks[:, :, 0] == 0xA5).all() and (acc.rec_score[0].view(torch.int32) == _pattern((1,), torch.int32)).all()
    gt_counts = ev.count_gts(pair["gts"], pair["ignore"], pair["ga"], pair["area_ranges"] if ranged else None, C).sum(0)
    assert torch.equal(acc.num_gts.cpu(), gt_counts)


def test_match_without_ignore_flags(pair):
    dets, gts = cases.to_device(pair["dets"], DEV), cases.to_device(pair["gts"], DEV)
    acc = ev.MapAccumulator(4, iou_thrs=THRS, capacity_images=3, max_per_img=K, device=DEV)
    marks = acc.update(dets, gts, out=_pattern((len(THRS), 1, 3, K), torch.uint8))
    assert torch.equal(marks.cpu(), ev.match_pairs(pair["iou"], pair["dets"], pair["gts"], None, THRS, None, pair["da"], pair["ga"]))


# ---- mask IoU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 8, 5, 32, 48), (2, 8, 5, 24, 40), (2, 4, 3, 512, 1024)])
def test_mask_iou_pairs_bit_for_bit(shape):
    B, Kk, G, H, W = shape
    d, g = cases.segm_case(B, Kk, G, H, W)
    dets, gts = cases.to_device(d, DEV), cases.to_device(g, DEV)
    want, (wda, wga) = ev.mask_iou_pairs(dets, gts).cpu(), ev.mask_areas(dets, gts)      # the definitions, on the same device
    assert (want > 0).any() and (want == 1).any() and (want == -1).any() and ((want > 0) & (want < 1)).any()
    out = (_pattern((B, Kk, G), torch.float32), _pattern((B, Kk), torch.float32), _pattern((B, G), torch.float32))
    iou, da, ga = ev.pair_iou_dispatch(dets, gts, "segm", out=out)
    assert torch.equal(iou.cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(da, wda) and torch.equal(ga, wga)


def test_mask_iou_pairs_rejects_a_size_that_is_no_multiple_of_16():
    d, g = cases.segm_case(1, 2, 2, 5, 5)
    with pytest.raises(PswinError):
        ev.pair_iou_dispatch(cases.to_device(d, DEV), cases.to_device(g, DEV), "segm")


# ---- AP segments --------------------------------------------------------------------------------------------------------------------------
def test_ap_segments_within_one_spacing_and_reproducible():
    marks, bounds, num_gts = cases.ap_case(ev.AP_CHUNK)
    want = ev.ap_segments(marks, bounds, num_gts)
    assert (want[:, :, -1] == 0).all() and (want[:, :, 0] == 0).all() and (want > 0).any()      # num_gts = 0; an empty segment
    assert float(want[0, 0, 3]) == pytest.approx(ev.AP_CHUNK / (ev.AP_CHUNK + 5), rel=1e-6)      # all tp: recall reaches n / (n + 5)
    m, b, n = marks.to(DEV), bounds.to(DEV), num_gts.to(DEV)
    first = ev.ap_segments_dispatch(m, b, n, out=_pattern(tuple(want.shape), torch.float32)).cpu()
    assert _spacing_ok(first, want), (first, want)
    second = ev.ap_segments_dispatch(m, b, n, out=_pattern(tuple(want.shape), torch.float32)).cpu()
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))


# ---- the accumulator ------------------------------------------------------------------------------------------------------------------------
def _batches(golden, device, batch=4):
    return [cases.golden_padded(golden, device=device, lo=lo, hi=lo + batch) for lo in range(0, 12, batch)]


@pytest.fixture(scope="module")
def cpu_result(golden):
    acc = ev.MapAccumulator(4, iou_thrs=(0.5, 0.75), scale_ranges=cases.scale_ranges(golden, True), capacity_images=12, max_per_img=16)
    for dets, gts, ignore in _batches(golden, "cpu"):
        acc.update(dets, gts, ignore)
    return acc, acc.summarize()


def _same_result(got, want):
    assert torch.equal(got["num_gts"], want["num_gts"]) and torch.equal(got["num_dets"], want["num_dets"])
    assert _spacing_ok(got["ap"], want["ap"]), (got["ap"], want["ap"])
    assert np.allclose(got["mean_ap"].numpy(), want["mean_ap"].numpy(), rtol=1e-6, atol=0)


def test_accumulator_bbox_on_the_fixture_in_batches_of_four(golden, cpu_result):
    acc = ev.MapAccumulator(4, iou_thrs=(0.5, 0.75), scale_ranges=cases.scale_ranges(golden, True), capacity_images=12, max_per_img=16, device=DEV)
    for dets, gts, ignore in _batches(golden, DEV):
        acc.update(dets, gts, ignore)
    cpu_acc, want = cpu_result
    assert torch.equal(acc.rec_marks.cpu(), cpu_acc.rec_marks) and torch.equal(acc.rec_label.cpu(), cpu_acc.rec_label)
    got = acc.summarize()
    _same_result(got, want)
    for t, name in enumerate(("thr50_ranges", "thr75_ranges")):                   # and the reference's own values
        assert _spacing_ok(got["ap"][t], golden[name + "_ap"])
        assert np.array_equal(got["num_gts"].numpy(), golden[name + "_num_gts"])


def test_accumulator_segm_against_the_cpu_definition():
    sets = [cases.segm_case(2, 8, 5, 32, 48, seed=s) for s in range(3)]
    cpu = ev.MapAccumulator(3, iou_thrs=THRS, capacity_images=6, max_per_img=8, iou="segm")
    gpu = ev.MapAccumulator(3, iou_thrs=THRS, capacity_images=6, max_per_img=8, iou="segm", device=DEV)
    for d, g in sets:
        want = cpu.update(d, g)
        got = gpu.update(cases.to_device(d, DEV), cases.to_device(g, DEV), out=_pattern(tuple(want.shape), torch.uint8))
        assert torch.equal(got.cpu(), want)
    assert (cpu.rec_marks == ev.MARK_TP).any() and (cpu.rec_marks == ev.MARK_FP).any()
    _same_result(gpu.summarize(), cpu.summarize())


def test_update_captured_once_and_replayed_over_three_batches(golden):
    batches = _batches(golden, DEV)
    eager = ev.MapAccumulator(4, iou_thrs=(0.5, 0.75), capacity_images=12, max_per_img=16, device=DEV)
    for dets, gts, ignore in batches:
        eager.update(dets, gts, ignore)
    acc = ev.MapAccumulator(4, iou_thrs=(0.5, 0.75), capacity_images=12, max_per_img=16, device=DEV)
    dets, gts, ignore = cases.golden_padded(golden, device=DEV, lo=0, hi=4)        # the static buffers
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        acc.update(dets, gts, ignore)                                             # warm-up outside the capture
        acc.reset()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            acc.update(dets, gts, ignore)
        for d, g, i in batches:
            for dst, src in ((dets.boxes, d.boxes), (dets.scores, d.scores), (dets.labels, d.labels), (dets.count, d.count), (gts.boxes, g.boxes),
                             (gts.labels, g.labels), (gts.count, g.count), (ignore, i)):
                dst.copy_(src)
            graph.replay()
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert int(acc.cursor) == 12
    for name in ("rec_score", "rec_label", "rec_marks", "num_gts", "overflow"):
        assert torch.equal(getattr(acc, name), getattr(eager, name)), name
    a, b = acc.summarize(), eager.summarize()
    assert torch.equal(a["ap"].view(torch.int32), b["ap"].view(torch.int32)) and torch.equal(a["mean_ap"], b["mean_ap"])


def test_overflow_keeps_the_first_records_and_summarize_raises(golden):
    batches = _batches(golden, DEV)
    acc = ev.MapAccumulator(4, capacity_images=8, max_per_img=16, device=DEV)
    for dets, gts, ignore in batches[:2]:
        acc.update(dets, gts, ignore)
    before = {n: getattr(acc, n).clone() for n in ("rec_score", "rec_label", "rec_marks", "num_gts")}
    assert int(acc.overflow) == 0
    acc.update(*batches[2])
    assert int(acc.overflow) == 1 and int(acc.cursor) == 12
    for n, v in before.items():
        assert torch.equal(getattr(acc, n), v), n
    with pytest.raises(PswinError):
        acc.summarize()
    assert acc.reset().summarize()["num_dets"].sum() == 0
