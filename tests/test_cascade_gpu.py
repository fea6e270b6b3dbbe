"""The Cascade R-CNN kernels on the MI355X (csrc/pswin_cascade.hip through ops.refine_rois / ops.giou_rows) and MiniCascadeRCNN's two
captured calls, against the definitions of cascade.py evaluated on the CPU.

INTEGERS (the class a RoI is regressed by, every stage's sampling) are compared exactly.

VALUES follow the rule the decode tests of tests/test_detect_post_gpu.py use: with the float64 definition as the truth, the kernel's largest
error may be at most 4 x the float32 CPU definition's own error on the same inputs, plus one float32 ulp of the largest value compared (the
largest coordinate for boxes, the largest row for the loss rows, the largest gradient element for the gradient).  A bf16 gradient is held
to that rule for the float32 value before it is rounded, plus half a bf16 ulp of the element.  Every comparison prints both errors.

Sizes sit on the kernels' own boundary: rows = pswin_cascade_rows_per_workgroup()."""
import ctypes

import pytest
import torch

import _cascade_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rows():
    from panoswintransformerobjectdetection_amd import ops
    return ops.cascade_rows_per_workgroup()


def _sizes():
    r = _rows()
    return (1, r - 1, r, r + 1, 1000)


def _within(got, f32, truth, what, half_bf16_ulp=False):
    """the module docstring's rule; got: the kernel's result, f32: the float32 CPU definition's, truth: the float64 definition's"""
    got, f32, truth = got.detach().double().cpu(), f32.detach().double().cpu(), truth.detach().double().cpu()
    e32 = float((f32 - truth).abs().max())
    slack = 4 * e32 + cases.ulp32(truth.abs().max())
    err = (got - truth).abs()
    bound = torch.full_like(err, slack)
    if half_bf16_ulp:                       # bf16 keeps 8 significant bits: half an ulp of v is 2^(e - 8) for 2^e <= |v| < 2^(e + 1)
        mag = truth.abs() + slack
        bound = bound + torch.where(mag > 0, torch.exp2(torch.floor(torch.log2(mag.clamp(min=2.0 ** -126))) - 8), torch.zeros_like(mag))
    print(f"{what}: kernel {float(err.max()):.3e} / f32 definition {e32:.3e} (largest value {float(truth.abs().max()):.3e})")
    assert bool((err <= bound).all()), (what, float(err.max()), e32, float((err - bound).max()))
    return float(err.max()), e32


# ---- ops.refine_rois -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 80, 128])
def test_refine_rois_picks_the_definitions_class_and_box(C, dtype):
    from panoswintransformerobjectdetection_amd import cascade, ops
    for R in _sizes():
        rois, cls, deltas, labels, stds, hw = cases.refine_case(2, R, C)
        for lab in (labels, None):
            new, used = ops.refine_rois(rois.to(DEV), cls.to(DEV, dtype), deltas.to(DEV, dtype), None if lab is None else lab.to(DEV), stds, hw)
            torch.cuda.synchronize()
            want, want_used = cascade.refine_rois(rois, cls, deltas, lab, stds, hw)              # bf16-exact values: the same numbers
            truth, _ = cascade.refine_rois(rois, cls, deltas, lab, stds, hw, dtype=torch.float64)
            assert used.dtype == torch.int64 and new.dtype == torch.float32 and tuple(new.shape) == (2, R, 4)
            assert torch.equal(used.cpu(), want_used), (R, C, lab is None)
            _within(new, want, truth, f"refine R={R} C={C} {'labels' if lab is not None else 'argmax'} boxes [px]")


# ---- ops.giou_rows ---------------------------------------------------------------------------------------------------------------------------
def _definition(case, dtype):
    rois, deltas, labels, weight, target, upstream, stds = case
    d = deltas.to(dtype).clone().requires_grad_(True)
    from panoswintransformerobjectdetection_amd import cascade
    rows = cascade.giou_rows(rois, d, labels, weight, target, stds, 1e-6, dtype=dtype)
    (rows * upstream.to(dtype)).sum().backward()
    return rows.detach(), d.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 80, 128])
def test_giou_rows_forward_and_backward(C, dtype):
    from panoswintransformerobjectdetection_amd import _lib, ops
    for N in _sizes():
        case = cases.giou_case(N, C)
        rois, deltas, labels, weight, target, upstream, stds = case
        dev = [t.to(DEV) for t in (rois, labels, weight, target, upstream)]

        def run():
            d = deltas.to(DEV, dtype).requires_grad_(True)
            rows = ops.giou_rows(dev[0], d, dev[1], dev[2], dev[3], stds, 1e-6)
            rows.backward(dev[4])
            torch.cuda.synchronize()
            return rows.detach(), d.grad, d
        rows, grad, d = run()
        rows2, grad2, _ = run()
        assert rows.dtype == torch.float32 and grad.dtype == dtype and tuple(grad.shape) == (N, 4 * C)
        assert torch.equal(rows.view(torch.int32), rows2.view(torch.int32)), "two calls on the same inputs"
        assert torch.equal(grad.view(torch.int16 if dtype == torch.bfloat16 else torch.int32), grad2.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
        want, want_grad = _definition(case, torch.float32)
        truth, truth_grad = _definition(case, torch.float64)
        _within(rows, want, truth, f"giou N={N} C={C} rows")
        _within(grad, want_grad, truth_grad, f"giou N={N} C={C} gradient", half_bf16_ulp=dtype == torch.bfloat16)
        # the entry point itself on a buffer full of NaN: every element is written, zeros outside the label's columns of weighted rows
        buf = torch.full((N, 4 * C), float("nan"), dtype=dtype, device=DEV)
        std4 = (ctypes.c_float * 4)(*stds)
        _lib.call("pswin_giou_rows_bwd", buf, _lib.ptr(dev[0]), _lib.ptr(d.detach()), _lib.dtype_code(buf), _lib.ptr(dev[1]), _lib.ptr(dev[2]),
                  _lib.ptr(dev[3]), _lib.ptr(dev[4]), N, C, ctypes.cast(std4, ctypes.c_void_p), ctypes.c_double(1e-6), _lib.ptr(buf))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(buf).all()), (N, C)
        assert torch.equal(buf, grad)
        mask = torch.zeros(N, C, 4, dtype=torch.bool)
        mask[torch.arange(N), labels.clamp(0, C - 1)] = (weight != 0)[:, None]
        assert not buf.cpu().float()[~mask.view(N, -1)].any(), (N, C)
        assert not rows.cpu()[weight == 0].any()


# ---- MiniCascadeRCNN: the stage hand-over ------------------------------------------------------------------------------------------------------
def _handover_chain(device):
    """the three stages' sampling and hand-over on fixed proposals, annotations, keys and BOX-HEAD OUTPUTS (no head runs): per stage the
    sample and the hand-over, as CPU tensors"""
    m = cases.tiny_model(device)
    m.rand_like = cases.layout_keys(8, device)
    T = cases.padded(cases.annotations((6, 0)), 8, device)
    g = torch.Generator().manual_seed(5)
    C = cases.NUM_CLASSES
    cand = torch.cat([T.boxes, torch.stack([cases._boxes(2000, g) for _ in range(cases.B)]).to(device)], 1)
    drop, out = None, []
    for i in range(3):
        s = m.stage_sample(i, cand, T, drop)
        cls = cases.bf16_exact(torch.round(torch.randn(cases.B * 512, C + 1, generator=g) * 4) / 4).to(device, torch.bfloat16)
        reg = cases.bf16_exact(torch.randn(cases.B * 512, 4 * C, generator=g)).to(device, torch.bfloat16)
        cand, drop, used = m.stage_handover(i, s, cls, reg, T, (cases.H, cases.W))
        with torch.no_grad():
            best = m.assign(cand, T.boxes, T.count, 0.5, 0.5, 0.5, False, lead_gt=8)[1]
        out.append({k: v.cpu() for k, v in dict(s, next_cand=cand, next_drop=drop, used=used, next_iou=best).items()})
    return out


def test_every_stages_sampling_equals_the_cpu_runs_on_the_same_box_head_outputs():
    """CONDITION on the inputs (asserted on the CPU run): no candidate's best IoU lies within 1e-5 of a stage's threshold, so that the
    refined boxes' last-ulp differences between the kernel and the CPU definition cannot move an assignment."""
    cpu, gpu = _handover_chain("cpu"), _handover_chain(DEV)
    for i, (a, b) in enumerate(zip(cpu, gpu)):
        thr = (0.6, 0.7, 0.7)[i]
        assert bool((((a["next_iou"] - thr).abs() > 1e-5) | (a["next_iou"] < 0)).all()), f"stage {i}: a best IoU within 1e-5 of {thr}"
        for k in ("labels", "pos_valid", "gt_idx", "pos_rank", "gt_inds", "used", "next_drop"):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (i, k)
        assert int(a["next_drop"][0].sum()) > 0
        err = float((a["next_cand"].double() - b["next_cand"].double()).abs().max())
        print(f"stage {i}: refined candidates differ by {err:.3e} px between the kernel and the float32 CPU definition")
        assert err <= 4 * cases.ulp32(cases.W)


# ---- MiniCascadeRCNN.heads_loss: one captured step -------------------------------------------------------------------------------------------
def test_one_captured_cascade_step_replays_bit_identically_and_follows_the_target_buffers():
    """heads_loss + backward on a PaddedTargets, captured once; every replay is run TWICE on the same buffers and must give the same bits,
    then the buffers take other annotations (other box counts, the image without boxes is now the other one) and the replay must follow them.

    The convolutions of the FPN, the RPN and the head stand-ins are MIOpen's, whose default bf16 solvers differ in the last bit from call to
    call (tools/debug_heads_determinism.py): with those, two replays of this very graph disagree -- seen on an MI355X
    before the mode below was set: loss_rpn_bbox by 23 ulp, and, because a few of the 2 x 512 sampled RoIs then change, s0.loss_cls
    1.8367 against 1.8363.  The test therefore runs under MIOpen's deterministic mode (torch.backends.cudnn.deterministic), which the
    project measured as bit-stable and does not adopt for training because of its cost; everything else in the step has to be
    bit-stable by itself."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _captured_step(side)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
    finally:
        torch.backends.cudnn.deterministic = prev


def _captured_step(side):
    from panoswintransformerobjectdetection_amd.graph import GraphedCallable
    GMAX = 8
    m = cases.tiny_model(DEV)                                   # narrow heads: the deterministic mode's convolution kernels are slow ones
    m.rand_like = cases.layout_keys(GMAX, DEV)
    heads = m.head_parameters()
    feats = cases.feature_maps(m, DEV)
    sets = [cases.annotations(c, seed) for c, seed in (((6, 0), 0), ((0, 8), 200))]            # captured on the first, replayed on the second
    T = cases.padded(sets[0], GMAX, DEV)
    state = {}

    def load(tg):
        T.copy_from([t["boxes"] for t in tg], [t["labels"] for t in tg], [t["masks"] for t in tg])

    def step():
        for p in heads:
            p.grad = None
        ls = m.heads_loss(feats, T, (cases.H, cases.W))
        sum(ls.values()).backward()
        state["names"] = sorted(ls)
        state["losses"] = torch.stack([ls[k] for k in state["names"]])
        return state["losses"]

    g = GraphedCallable(step, warmup=1, stream=side, parameters=heads)
    assert len(state["names"]) == 11
    seen = []
    for tg in sets:
        load(tg)
        g()
        side.synchronize()
        first = state["losses"].clone()
        grads_ok = all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in heads)
        g()
        side.synchronize()
        second = state["losses"].clone()
        print("replayed losses", dict(zip(state["names"], first.tolist())))
        assert bool(torch.isfinite(first).all()) and grads_ok
        assert torch.equal(first.view(torch.int32), second.view(torch.int32)), "two replays on the same buffers"
        seen.append(first)
    with torch.no_grad():
        want = m.heads_loss(feats, T, (cases.H, cases.W))                                        # eager, the last annotations and the same keys
    for k, v in zip(state["names"], seen[-1].tolist()):
        # the bound of the parent's replay test (tests/test_detector_padded_gpu.py) for an eager call against a captured one
        assert abs(v - float(want[k])) <= 2e-3 * max(abs(float(want[k])), 1e-3), (k, v, float(want[k]))
    assert not torch.equal(seen[0], seen[1])                                                     # the replay followed the buffers


# ---- MiniCascadeRCNN.heads_predict -----------------------------------------------------------------------------------------------------------
def test_heads_predict_is_the_post_processing_of_its_raw_tensors():
    from panoswintransformerobjectdetection_amd import cascade, ops
    m = cases.tiny_model(DEV, narrow=False).eval()
    feats = cases.feature_maps(m, DEV)
    hw = (cases.H, cases.W)
    out, raw = m.heads_predict(feats, hw, return_raw=True)
    torch.cuda.synchronize()
    assert len(raw["rois"]) == len(raw["cls"]) == len(raw["deltas"]) == len(raw["mask_logits"]) == 3
    B, R, C = raw["cls"][0].shape[0], raw["cls"][0].shape[1], cases.NUM_CLASSES
    # the last stage's RoIs are refine o refine of the first stage's, through the definition on the raw tensors
    cpu = lambda t: t.detach().cpu()                                                               # noqa: E731
    stds = [c["stds"] for c in m.rcnn_cfg]
    chain32, chain64 = cpu(raw["rois"][0]), cpu(raw["rois"][0]).double()
    for i in range(2):
        cls_i, reg_i = cpu(raw["cls"][i]).float(), cpu(raw["deltas"][i]).float()
        chain32, used32 = cascade.refine_rois(chain32, cls_i, reg_i, None, stds[i], hw)
        chain64, used64 = cascade.refine_rois(chain64, cls_i, reg_i, None, stds[i], hw, dtype=torch.float64)
        assert torch.equal(used32, used64)
    _within(raw["rois"][2], chain32, chain64, "heads_predict: the last stage's RoIs [px]")
    # the detections are the existing post-processing applied to the ensembles of the raw tensors
    K = m.test_cfg["rcnn"]["max_per_img"]
    cfg = m.test_cfg["rcnn"]
    boxes, scores, labels, count, source = ops.multiclass_nms_batch(raw["rois"][2], raw["roi_count"], cascade.ensemble_logits(raw["cls"]), raw["deltas"][2],
                                                                    stds[2], hw, None, cfg["score_thr"], cfg["nms"], K)
    masks = ops.paste_masks(cascade.ensemble_mask_logits(raw["mask_logits"], labels), torch.zeros_like(labels), boxes, count, cfg["mask_thr_binary"], hw)
    torch.cuda.synchronize()
    assert tuple(out.boxes.shape) == (B, K, 4) and tuple(out.masks.shape) == (B, K) + hw and out.masks.dtype == torch.uint8
    for name, a, b in (("boxes", out.boxes, boxes), ("scores", out.scores, scores), ("labels", out.labels, labels), ("count", out.count, count),
                       ("source", out.source, source), ("masks", out.masks, masks)):
        assert torch.equal(a, b), name
    assert int(out.count.sum()) > 0, "no detection at all: the comparison would be empty"
