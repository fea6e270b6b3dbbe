"""The loss kernels on the MI355X (csrc/pswin_losses.hip through ops.ce_rows / l1_rows / mask_bce_rows / rpn_losses) against the
definitions of losses.py evaluated on the CPU, and both models' heads_loss with the hooks on the kernels.

VALUES.  Kernel and float64 definition see the same (bf16-exact) inputs.  The bound is not a number fixed in advance: for every output
element it is max(4 e32, 4 ulp32(|value|)), e32 being the error of the float32 CPU definition against float64 on that element, computed
here (tests/_losses_cases.within); a bf16 gradient gets half a bf16 ulp of the float64 value on top.  The factor 4 is the margin this
project gives a kernel over the float32 formula elsewhere (tests/test_stem_chain_gpu.py).  Every comparison prints the kernel's largest
error beside the float32 definition's.

Every forward and backward is called twice on the same inputs and must return the same bits; every backward is also run through its
entry point on a buffer full of NaN, which must come back fully written and equal to the autograd result.

Sizes sit on the kernels' own boundaries: pswin_losses_rows_per_workgroup() rows, pswin_rpn_losses_chunk() anchors."""

import pytest
import torch

import _losses_cases as cases
from panoswintransformerobjectdetection_amd import losses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), what


def _sizes():
    from panoswintransformerobjectdetection_amd import ops
    assert ops.losses_rows_per_workgroup() == cases.ROWS
    return cases.row_sizes()


def _definition(fn, x, rest, upstream, dtype):
    """(rows, gradient of x) of a row definition evaluated in `dtype` on the CPU"""
    x = x.clone().requires_grad_(True)
    rows = fn(x, *rest, dtype=dtype)
    (rows * upstream.to(dtype)).sum().backward()
    return rows.detach(), x.grad


def _twice(fn, x_cpu, rest_dev, upstream_dev, dtype, memory_format=torch.contiguous_format):
    """the operator's rows and gradient, run twice on fresh leaves: identical bits; returns the first run and its leaf"""
    runs = []
    for _ in range(2):
        x = x_cpu.to(DEV, dtype, copy=True).contiguous(memory_format=memory_format).requires_grad_(True)
        rows = fn(x, *rest_dev)
        rows.backward(upstream_dev)
        torch.cuda.synchronize()
        runs.append((rows.detach(), x.grad, x))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])), "two forward calls on the same inputs"
    _same_bits(runs[0][1], runs[1][1], "two backward calls on the same inputs")
    return runs[0]


# ---- ce_rows -----------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("C1", [2, 6, 81, 129])
def test_ce_rows_forward_and_backward(C1, dtype):
    from panoswintransformerobjectdetection_amd import _lib, ops
    for N in _sizes():
        cls, labels, up = cases.ce_case(N, C1)
        lab_d, up_d = labels.to(DEV), up.to(DEV)
        rows, grad, x = _twice(ops.ce_rows, cls, (lab_d,), up_d, dtype)
        assert rows.dtype == torch.float32 and grad.dtype == dtype and tuple(grad.shape) == (N, C1)
        want, want_grad = _definition(losses.ce_rows, cls, (labels,), up, torch.float32)
        truth, truth_grad = _definition(losses.ce_rows, cls, (labels,), up, torch.float64)
        cases.within(rows, want, truth, f"ce_rows N={N} C+1={C1} rows")
        cases.within(grad, want_grad, truth_grad, f"ce_rows N={N} C+1={C1} gradient", bf16=dtype == torch.bfloat16)
        off = (labels < 0) | (labels >= C1)
        assert not rows.cpu()[off].any() and not grad.cpu()[off].any()
        if N >= 9:
            assert int(off.sum()) == 3 and float(rows[0]) == 0.0 and abs(float(rows[1]) - 160.0) < 1e-4
        buf = torch.full((N, C1), float("nan"), dtype=dtype, device=DEV)
        _lib.call("pswin_ce_rows_bwd", buf, _lib.ptr(x.detach()), _lib.dtype_code(buf), _lib.ptr(lab_d), _lib.ptr(up_d), N, C1 - 1, _lib.ptr(buf))
        torch.cuda.synchronize()
        _same_bits(buf, grad, "every element written")


# ---- l1_rows -----------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("C", [1, 5, 80, 128])
def test_l1_rows_forward_and_backward(C, dtype):
    from panoswintransformerobjectdetection_amd import _lib, ops
    for N in _sizes():
        reg, labels, weight, target, up = cases.l1_case(N, C)
        rest = [t.to(DEV) for t in (labels, weight, target)]
        up_d = up.to(DEV)
        rows, grad, x = _twice(ops.l1_rows, reg, rest, up_d, dtype)
        assert rows.dtype == torch.float32 and grad.dtype == dtype and tuple(grad.shape) == (N, 4 * C)
        want, _ = _definition(losses.l1_rows, reg, (labels, weight, target), up, torch.float32)
        truth, _ = _definition(losses.l1_rows, reg, (labels, weight, target), up, torch.float64)
        cases.within(rows, want, truth, f"l1_rows N={N} C={C} rows")
        # the gradient bit for bit: +-fl(weight * upstream) rounded to the dtype in the label's columns of a weighted row, +0 elsewhere
        lab = labels.clamp(0, C - 1)
        d = reg.view(N, C, 4)[torch.arange(N), lab] - target
        g = (weight * up)[:, None].expand(N, 4)
        vals = torch.where(d > 0, g, torch.where(d < 0, -g, torch.zeros(())))
        vals = torch.where((weight != 0)[:, None], vals, torch.zeros(()))
        full = torch.zeros(N, C, 4)
        full[torch.arange(N), lab] = vals
        _same_bits(grad.cpu(), full.view(N, 4 * C).to(dtype), f"l1_rows N={N} C={C} gradient")
        if N >= 9:
            assert float(vals[0, 1]) == 0.0 and float(vals[1, 3]) == 0.0 and not rows.cpu()[2:4].any()
        buf = torch.full((N, 4 * C), float("nan"), dtype=dtype, device=DEV)
        _lib.call("pswin_l1_rows_bwd", buf, _lib.ptr(x.detach()), _lib.dtype_code(buf), _lib.ptr(rest[0]), _lib.ptr(rest[1]), _lib.ptr(rest[2]),
                  _lib.ptr(up_d), N, C, _lib.ptr(buf))
        torch.cuda.synchronize()
        _same_bits(buf, grad, "every element written")


# ---- mask_bce_rows -----------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("memory", [torch.contiguous_format, torch.channels_last], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("S", [7, 28])
@pytest.mark.parametrize("C", [1, 5, 80])
def test_mask_bce_rows_forward_and_backward(C, S, memory, dtype):
    from panoswintransformerobjectdetection_amd import _lib, ops
    for M in (1, 3, 130):
        logits, labels, target, weight, up = cases.mask_case(M, C, S)
        rest = [t.to(DEV) for t in (labels, target, weight)]
        up_d = up.to(DEV)
        rows, grad, x = _twice(ops.mask_bce_rows, logits, rest, up_d, dtype, memory)
        assert rows.dtype == torch.float32 and grad.dtype == dtype and grad.shape == x.shape and grad.stride() == x.stride()
        want, want_grad, truth, truth_grad = _mask_reference(M, C, S)
        cases.within(rows, want, truth, f"mask_bce_rows M={M} C={C} S={S} rows")
        ar, lab = torch.arange(M), labels.clamp(0, C - 1)
        g = grad.cpu()
        cases.within(g[ar, lab], want_grad, truth_grad, f"mask_bce_rows M={M} C={C} S={S} gradient", bf16=dtype == torch.bfloat16)
        other = torch.ones(M, C, dtype=torch.bool)
        other[ar, lab] = False
        assert not g[other].any(), "every channel but the label's is exactly 0"
        dead = weight == 0
        assert not rows.cpu()[dead].any() and not g[dead].any()
        # the entry points themselves on buffers full of NaN: the forward leaves the label's channel (zeros in a weight-0 row), the backward
        # takes it and writes every element
        strides = ops._mask_strides(x.detach())
        picked = torch.full((M, S, S), float("nan"), device=DEV)
        rows2 = torch.full((M,), float("nan"), device=DEV)
        _lib.call("pswin_mask_bce_rows_fwd", picked, _lib.ptr(x.detach()), _lib.dtype_code(x), *strides, _lib.ptr(rest[0]), _lib.ptr(rest[1]),
                  _lib.ptr(rest[2]), M, C, S, _lib.ptr(rows2), _lib.ptr(picked))
        buf = torch.full((M, C, S, S), float("nan"), dtype=dtype, device=DEV).contiguous(memory_format=memory)
        _lib.call("pswin_mask_bce_rows_bwd", buf, _lib.ptr(picked), _lib.dtype_code(buf), *strides, _lib.ptr(rest[0]), _lib.ptr(rest[1]),
                  _lib.ptr(rest[2]), _lib.ptr(up_d), M, C, S, _lib.ptr(buf))
        torch.cuda.synchronize()
        want_picked = torch.where(dead[:, None, None], torch.zeros(()), logits[ar, lab])
        _same_bits(picked.cpu(), want_picked, "the label's channel as the forward read it")
        _same_bits(rows2, rows, "rows of the entry point")
        _same_bits(buf, grad, "every element written")


_MASK_REF = {}


def _mask_reference(M, C, S):
    """the CPU definition once per shape, shared by the layouts and dtypes: (rows32, grad32, rows64, grad64), the gradients as the label's
    channel [M, S, S] -- the definition's other channels are exactly 0, asserted here"""
    if (M, C, S) not in _MASK_REF:
        logits, labels, target, weight, up = cases.mask_case(M, C, S)
        out = []
        for dt in (torch.float32, torch.float64):
            rows, grad = _definition(losses.mask_bce_rows, logits, (labels, target, weight), up, dt)
            sel = grad[torch.arange(M), labels.clamp(0, C - 1)].clone()
            grad[torch.arange(M), labels.clamp(0, C - 1)] = 0
            assert not grad.any()
            out += [rows, sel]
        _MASK_REF[(M, C, S)] = tuple(out)
    return _MASK_REF[(M, C, S)]


# ---- rpn_losses --------------------------------------------------------------------------------------------------------------------------
def _rpn_definition(case, dtype):
    cls_all, reg_all, idx, valid, pos_valid, reg_t, up = case
    c, r = cls_all.clone().requires_grad_(True), reg_all.clone().requires_grad_(True)
    out = losses.rpn_losses(c, r, idx, valid, pos_valid, reg_t, dtype=dtype)
    (out * up.to(dtype)).sum().backward()
    return out.detach(), c.grad, r.grad


@pytest.mark.parametrize("A", [100, 4097, 20000])
def test_rpn_losses_forward_and_backward(A):
    from panoswintransformerobjectdetection_amd import _lib, ops
    assert ops.rpn_losses_chunk() == cases.CHUNK
    case = cases.rpn_case(A)
    cls_all, reg_all, idx, valid, pos_valid, reg_t, up = case
    dev = [t.to(DEV) for t in case]
    runs = []
    for _ in range(2):
        c, r = dev[0].clone().requires_grad_(True), dev[1].clone().requires_grad_(True)
        out = ops.rpn_losses(c, r, *dev[2:6])
        gc, gr = torch.autograd.grad(out, (c, r), dev[6])
        # the same backward into the SAME storage, filled with a sentinel first: every element must be written
        sent_c, sent_r, gc, gr = gc, gr, gc.clone(), gr.clone()
        sent_c.fill_(float("nan"))
        sent_r.fill_(float("nan"))
        _lib.call("pswin_rpn_losses_bwd", sent_c, _lib.ptr(dev[0]), _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]), _lib.ptr(dev[4].view(torch.uint8)),
                  _lib.ptr(dev[5]), _lib.ptr(dev[6]), cases.RPN_B, A, cases.RPN_S, cases.RPN_P, _lib.ptr(sent_c), _lib.ptr(sent_r))
        torch.cuda.synchronize()
        _same_bits(sent_c, gc, "grad_cls: every element written")
        _same_bits(sent_r, gr, "grad_reg: every element written")
        runs.append((out.detach(), gc, gr))
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b)), "two calls on the same inputs"
    out, gc, gr = runs[0]
    want, truth = _rpn_definition(case, torch.float32), _rpn_definition(case, torch.float64)
    for name, got, w, t in zip(("losses", "gradient of the scores", "gradient of the deltas"), (out, gc, gr), want, truth):
        cases.within(got, w, t, f"rpn_losses A={A} {name}")
    assert out[1].tolist() == [0.0, 0.0] and not gc[1].any() and not gr[1].any()                # the image without a valid slot
    assert torch.equal(gc.cpu() != 0, truth[1] != 0) and torch.equal(gr.cpu() != 0, truth[2] != 0)
    assert int((gc[0] != 0).sum()) == 15 and int((gc[2] != 0).sum()) == 22                       # an invalid repeat overwrote no valid anchor


# ---- all four in one captured graph ------------------------------------------------------------------------------------------------------
def test_the_four_losses_and_their_backward_replay_bit_identically_on_new_values():
    """One graph: the four operators forward and backward on static buffers (N = 65 rows, C = 5, M = 3 masks of 7 x 7 channels-last bf16,
    A = 4097 anchors).  Replayed on two sets of logits, labels and targets written into those buffers; every replay equals the eager call
    on the same values, bit for bit."""
    from panoswintransformerobjectdetection_amd import ops
    N, C, M, S, A = 65, 5, 3, 7, 4097

    def values(seed):
        cls, lab, up = cases.ce_case(N, C + 1, seed)
        reg, lab_r, w, tgt, up_r = cases.l1_case(N, C, seed)
        logits, lab_m, mt, wm, up_m = cases.mask_case(M, C, S, seed)
        return dict(cls=cls.bfloat16(), lab=lab, up=up, reg=reg.bfloat16(), lab_r=lab_r, w=w, tgt=tgt, up_r=up_r,
                    logits=logits.bfloat16().contiguous(memory_format=torch.channels_last), lab_m=lab_m, mt=mt, wm=wm, up_m=up_m,
                    **dict(zip(("cls_all", "reg_all", "idx", "valid", "pos_valid", "reg_t", "up_rpn"), cases.rpn_case(A, seed=seed))))

    leaves = ("cls", "reg", "logits", "cls_all", "reg_all")

    def run(buf):
        x = {k: buf[k].detach().requires_grad_(True) for k in leaves}
        outs = [ops.ce_rows(x["cls"], buf["lab"]), ops.l1_rows(x["reg"], buf["lab_r"], buf["w"], buf["tgt"]),
                ops.mask_bce_rows(x["logits"], buf["lab_m"], buf["mt"], buf["wm"]),
                ops.rpn_losses(x["cls_all"], x["reg_all"], buf["idx"], buf["valid"], buf["pos_valid"], buf["reg_t"])]
        ups = [buf["up"], buf["up_r"], buf["up_m"], buf["up_rpn"]]
        total = sum((o * u).sum() for o, u in zip(outs, ups))
        grads = torch.autograd.grad(total, [x[k] for k in leaves])
        return outs + list(grads)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        static = {k: v.to(DEV) for k, v in values(0).items()}
        for _ in range(2):
            run(static)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            held = run(static)
        seen = []
        for seed in (1, 2):
            fresh = {k: v.to(DEV) for k, v in values(seed).items()}
            for k, v in fresh.items():
                static[k].copy_(v)
            graph.replay()
            side.synchronize()
            replayed = [t.clone() for t in held]
            eager = run(fresh)
            side.synchronize()
            for i, (a, b) in enumerate(zip(replayed, eager)):
                _same_bits(a, b, f"seed {seed}: output {i} of the replay against the eager call")
            seen.append(replayed)
        assert not torch.equal(seen[0][0], seen[1][0])                                            # the replay followed the buffers
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


# ---- the models --------------------------------------------------------------------------------------------------------------------------
def test_minimaskrcnn_losses_with_the_kernels_agree_with_the_definitions_on_the_list_case():
    """The case of tests/_heads_list_case.py on the GPU, with its fixed sampler keys, once with the hooks on the kernels and once on the
    definitions.  The five losses agree within 2e-3 * max(|want|, 1e-3): the bound tests/test_detector_padded_gpu.py holds two
    evaluations of this step to (the heads' convolutions differ in the last bits from call to call)."""
    import _heads_list_case as lc
    from panoswintransformerobjectdetection_amd import detector as det
    m = lc.model().to(DEV)
    m.roi_align = det.roi_align
    keys = lc.permuted_keys()
    m.rand_like = lambda t: keys(t).to(t.device)
    tg = [{k: v.to(DEV) for k, v in t.items()} for t in lc.targets()]
    rpn_outs, fpn, proposals = lc.inputs()
    rpn_outs = [(c.to(DEV), r.to(DEV)) for c, r in rpn_outs]
    fpn, proposals = [f.to(DEV) for f in fpn], [p.to(DEV) for p in proposals]
    anchors = det.make_anchors(lc.LEVELS, m.STRIDES, DEV)

    def run(hooks):
        for k, fn in hooks.items():
            setattr(m, k, fn)
        with torch.no_grad():
            rpn_cls, rpn_reg, _ = m._rpn_losses_and_proposals(rpn_outs, anchors, tg, (lc.H, lc.W))
            with torch.autocast("cuda", dtype=torch.bfloat16):
                roi = m._roi_losses(fpn, proposals, tg, (lc.H, lc.W))
        torch.cuda.synchronize()
        return dict(zip(("loss_rpn_cls", "loss_rpn_bbox", "loss_cls", "loss_bbox", "loss_mask"), (float(v) for v in (rpn_cls, rpn_reg) + tuple(roi))))

    want, got = run(losses.DEFINITION_HOOKS), run(losses.KERNEL_HOOKS)
    for k in want:
        print(f"{k}: kernels {got[k]:.7g}, definitions {want[k]:.7g}")
        assert abs(got[k] - want[k]) <= 2e-3 * max(abs(want[k]), 1e-3), (k, got[k], want[k])


def test_minicascadercnn_heads_loss_with_the_kernels_is_finite_with_finite_gradients():
    import _cascade_cases as cc
    m = cc.tiny_model(DEV, narrow=False)
    m.rand_like = cc.layout_keys(8, DEV)
    T = cc.padded(cc.annotations((6, 0)), 8, DEV)
    ls = m.heads_loss(cc.feature_maps(m, DEV), T, (cc.H, cc.W))
    sum(ls.values()).backward()
    torch.cuda.synchronize()
    print({k: round(float(v), 6) for k, v in ls.items()})
    assert len(ls) == 11 and all(bool(torch.isfinite(v)) for v in ls.values())
    heads = m.head_parameters()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in heads)
    assert float(ls["s0.loss_mask"]) > 0 and float(ls["s0.loss_cls"]) > 0
