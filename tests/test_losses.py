"""The detector's loss rows (panoswintransformerobjectdetection_amd/losses.py) on the CPU: the row definitions composed as the models' hooks
compose them against the expressions the models evaluated before, the exact properties of the definitions, the argument checks of the
eight entry points of csrc/pswin_losses.hip on a host without a GPU, and the hooks of both models.  The GPU side is
tests/test_losses_gpu.py."""
import ctypes

import numpy as np
import torch

import _losses_cases as cases
from panoswintransformerobjectdetection_amd import losses

EPS32 = float(np.finfo(np.float32).eps)          # 2^-23: one ulp of 1.0; a float32 operation is off by at most half of it, relatively


def _leaves(d, names, dtype):
    return {k: (d[k].to(dtype).clone().requires_grad_(True) if k in names else d[k]) for k in d}


def _compare(new, old, leaves, terms, what):
    """new / old: callables on a dict of inputs returning a tuple of scalars.  Evaluated in float32 (new and old) and in float64 (old: the
    truth).  BOUND, from the formats: every scalar is a sum of at most `terms` non-negative float32 terms, each the result of a few
    float32 operations (an exp, a log, a few additions: under 8 roundings of half an ulp), divided once: both orders of evaluation are
    within (terms + 8) * 2^-24 of the truth relatively, so they differ from each other by at most twice that.  A gradient element is a
    product of under 8 float32 roundings (no sum: every element receives one contribution), relative to the largest element of its tensor
    plus the value bound for the softmax's row sum."""
    d = cases.heads_case()
    got, want, truth = {}, {}, {}
    for store, fn, dtype in ((got, new, torch.float32), (want, old, torch.float32), (truth, old, torch.float64)):
        x = _leaves(d, leaves, dtype)
        vals = fn(x)
        sum(v * (i + 1.5) for i, v in enumerate(vals)).backward()
        store["v"] = [float(v) for v in vals]
        store["g"] = {k: x[k].grad.double() for k in leaves}
    rel = 2 * (terms + 8) * EPS32 / 2
    for i, (a, b, t) in enumerate(zip(got["v"], want["v"], truth["v"])):
        print(f"{what}[{i}]: hooks' form {a:.9g}, the form before {b:.9g}, float64 {t:.12g}")
        assert abs(a - b) <= rel * abs(t) and abs(a - t) <= rel * abs(t) and abs(b - t) <= rel * abs(t), (what, i, a, b, t)
    for k in leaves:
        scale = float(truth["g"][k].abs().max())
        assert scale > 0, k
        for other in (want, truth):
            err = float((got["g"][k] - other["g"][k]).abs().max())
            print(f"{what}: gradient of {k} differs by {err:.3e} of {scale:.3e}")
            assert err <= rel * scale, (what, k, err, scale)
        assert torch.equal(got["g"][k] != 0, truth["g"][k] != 0), (what, k)          # the same elements receive a gradient


# ---- the compositions against the expressions before ---------------------------------------------------------------------------------
def test_cls_loss_of_rows_is_the_cross_entropy_before():
    _compare(lambda x: (losses.cls_loss_definition(x["cls"], x["labels_b"].reshape(-1)),),
             lambda x: (cases.cls_loss_before(x["cls"], x["labels_b"].reshape(-1)),), ("cls",), 48 * 6, "cls_loss")


def test_box_loss_of_all_rows_is_the_l1_on_the_positives_before():
    _compare(lambda x: (losses.box_loss_definition(x["reg"], x["labels_b"], x["reg_t"], x["pos_valid"]),),
             lambda x: (cases.box_loss_before(x["reg"], x["labels_b"], x["reg_t"], x["pos_valid"]),), ("reg",), 48 * 4, "box_loss")


def test_mask_loss_of_rows_is_the_bce_on_the_selected_channel_before():
    _compare(lambda x: (losses.mask_loss_definition(x["logits"], x["pl"], x["mt"], x["pv"]),),
             lambda x: (cases.mask_loss_before(x["logits"], x["pl"], x["mt"], x["pv"]),), ("logits",), 12 * 49, "mask_loss")


def test_rpn_loss_of_rows_is_the_two_rpn_losses_before():
    args = ("cls_all", "reg_all", "idx", "valid", "rpn_pos_valid", "rpn_reg_t")
    _compare(lambda x: losses.rpn_loss_definition(*(x[k] for k in args)), lambda x: cases.rpn_loss_before(*(x[k] for k in args)),
             ("cls_all", "reg_all"), 32 * 4, "rpn_loss")


def test_on_cpu_tensors_the_dispatch_functions_return_the_bits_of_the_expressions_before():
    d = cases.heads_case()
    assert torch.equal(losses.cls_loss_dispatch(d["cls"], d["labels_b"].reshape(-1)), cases.cls_loss_before(d["cls"], d["labels_b"].reshape(-1)))
    assert torch.equal(losses.box_loss_dispatch(d["reg"], d["labels_b"], d["reg_t"], d["pos_valid"]),
                       cases.box_loss_before(d["reg"], d["labels_b"], d["reg_t"], d["pos_valid"]))
    assert torch.equal(losses.mask_loss_dispatch(d["logits"], d["pl"], d["mt"], d["pv"]), cases.mask_loss_before(d["logits"], d["pl"], d["mt"], d["pv"]))
    args = [d[k] for k in ("cls_all", "reg_all", "idx", "valid", "rpn_pos_valid", "rpn_reg_t")]
    for a, b in zip(losses.rpn_loss_dispatch(*args), cases.rpn_loss_before(*args)):
        assert torch.equal(a, b)


# ---- exact properties of the definitions ---------------------------------------------------------------------------------------------
def _rows_and_grad(fn, x, *rest, upstream=None):
    x = x.clone().requires_grad_(True)
    rows = fn(x, *rest)
    (rows * (upstream if upstream is not None else 1.0)).sum().backward()
    return rows.detach(), x.grad


def test_ce_rows_zero_rows_for_labels_out_of_range_and_no_overflow():
    cls, labels, up = cases.ce_case(197, 81)
    rows, grad = _rows_and_grad(losses.ce_rows, cls, labels, upstream=up)
    assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(grad).all())
    for n in (6, 7, 8):                                                   # labels -1, C + 1 and 2^40
        assert float(rows[n]) == 0.0 and not grad[n].any()
    assert float(rows[0]) == 0.0                                          # the hot logit is the label: log(1 + 80 e^-160) rounds to 0
    assert abs(float(rows[1]) - 160.0) <= 160 * EPS32
    assert abs(float(rows[2]) - float(np.log(81.0))) <= 4 * EPS32 * float(np.log(81.0))          # all logits at 3e4: log(C + 1)
    assert bool((rows[[4, 5]] > 0).all()) and bool(grad[4].any()) and bool(grad[5].any())      # labels 0 and C are classes
    assert float(grad[4].sum().abs()) <= 81 * EPS32 * float(up[4])                              # a softmax row minus its one-hot sums to 0


def test_l1_rows_weight_zero_rows_and_the_sign_of_zero():
    reg, labels, weight, target, up = cases.l1_case(65, 5)
    rows, grad = _rows_and_grad(losses.l1_rows, reg, labels, weight, target, upstream=up)
    assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(grad).all())
    dead = weight == 0
    assert int(dead.sum()) >= 3 and not rows[dead].any() and not grad[dead].any()
    lab = labels.clamp(0, 4)
    assert float(grad[0, 4 * int(lab[0]) + 1]) == 0.0 and float(grad[1, 4 * int(lab[1]) + 3]) == 0.0        # reg == target there
    want = torch.sign(reg.view(65, 5, 4)[torch.arange(65), lab] - target) * (weight * up)[:, None]
    want[dead] = 0
    full = torch.zeros(65, 5, 4)
    full[torch.arange(65), lab] = want
    assert torch.equal(grad, full.view(65, 20))                           # +-fl(weight * upstream) in the label's columns, 0 elsewhere
    assert int(lab[4]) == 0 and int(lab[5]) == 4 and bool(grad[4, :4].all()) and bool(grad[5, 16:].all())   # clamped labels


def test_mask_bce_rows_weight_zero_rows_and_the_selected_channel():
    logits, labels, target, weight, up = cases.mask_case(130, 5, 7)
    assert bool(torch.isnan(logits[1]).all()) and float(weight[1]) == 0
    for mem in (torch.contiguous_format, torch.channels_last):
        rows, grad = _rows_and_grad(losses.mask_bce_rows, logits.contiguous(memory_format=mem), labels, target, weight, upstream=up)
        assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(grad).all())
        dead = weight == 0
        assert int(dead.sum()) >= 3 and not rows[dead].any() and not grad[dead].any()
        sel = torch.zeros(130, 5, dtype=torch.bool)
        sel[torch.arange(130), labels.clamp(0, 4)] = ~dead
        assert not grad[~sel].any() and float(grad[sel].ne(0).float().mean()) > 0.9    # (sigmoid(60) - 1 is 0 in float32)
        # sigmoid(0) - t = +-1/2 exactly where the logit is 0
        m = int(torch.nonzero(~dead)[0])
        c = int(labels[m].clamp(0, 4))
        assert float(logits[m, c, 0, 6]) == 0.0
        want = float((0.5 - target[m, 0, 6]) * (weight[m] * up[m]) / 49)
        assert abs(float(grad[m, c, 0, 6]) - want) <= 2 * EPS32 * abs(want)


def test_rpn_losses_of_an_image_without_valid_slots_and_skipped_slots():
    cls_all, reg_all, idx, valid, pos_valid, reg_t, up = cases.rpn_case(4097)
    c, r = cls_all.clone().requires_grad_(True), reg_all.clone().requires_grad_(True)
    out = losses.rpn_losses(c, r, idx, valid, pos_valid, reg_t)
    (out * up).sum().backward()
    assert tuple(out.shape) == (3, 2) and out[1].tolist() == [0.0, 0.0]            # avg = 1, zero losses
    assert not c.grad[1].any() and not r.grad[1].any()
    assert bool((out[0] > 0).all()) and bool((out[2] > 0).all())
    for b, n_cls, n_reg in ((0, 15, 5), (2, 22, 6)):                                # a gradient at the valid slots' anchors and nowhere else
        assert int((c.grad[b] != 0).sum()) == n_cls and int(r.grad[b].ne(0).any(1).sum()) == n_reg
        assert bool(c.grad[b][idx[b][valid[b] != 0]].ne(0).all())
    assert float(r.grad[0, idx[0, 1], 2]) == 0.0 and float(r.grad[2, idx[2, 0], 0]) == 0.0       # sign(0) = 0
    # the invalid slots hold NaN-free garbage today; whatever they hold, nothing changes
    poisoned = cls_all.clone()
    poisoned[1] = float("nan")                                                         # image 1 has no valid slot at all
    assert torch.equal(losses.rpn_losses(poisoned, reg_all, idx, valid, pos_valid, reg_t), out.detach())


# ---- the entry points' argument checks on a host without a GPU ---------------------------------------------------------------------------
def test_argument_errors_of_the_eight_entry_points_without_a_gpu():
    """Every entry point validates its arguments before it touches the device: a bad call returns PSWIN_ERR_ARG (-1) here, where no
    device exists.  (A good call is not made: it would launch.)"""
    from panoswintransformerobjectdetection_amd import _lib, ops
    lib = _lib.load()
    ERR = -1
    assert ops.losses_rows_per_workgroup() == cases.ROWS and ops.rpn_losses_chunk() == cases.CHUNK
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15

    def each_bad(fn, good, bads):
        for i, v in bads:
            args = list(good)
            args[i] = v
            assert getattr(lib, fn)(*args) == ERR, (fn, i, v)

    ce_f = [p, 1, p, 64, 80, p, None]
    each_bad("pswin_ce_rows_fwd", ce_f, [(0, None), (2, None), (5, None), (1, 2), (3, 0), (3, -1), (4, 0), (4, 129), (0, p + 1), (2, p + 4), (5, p + 2)])
    ce_b = [p, 0, p, p, 64, 80, p, None]
    each_bad("pswin_ce_rows_bwd", ce_b, [(0, None), (2, None), (3, None), (6, None), (4, -5), (5, 0), (5, 129), (0, p + 2), (6, p + 2), (3, p + 2)])
    l1_f = [p, 1, p, p, p, 64, 80, p, None]
    each_bad("pswin_l1_rows_fwd", l1_f, [(0, None), (2, None), (3, None), (4, None), (7, None), (1, -1), (5, 0), (6, 0), (6, 129), (0, p + 4),
                                         (4, p + 8), (5, 1 << 23)])
    l1_b = [p, 0, p, p, p, p, 64, 80, p, None]
    each_bad("pswin_l1_rows_bwd", l1_b, [(0, None), (5, None), (8, None), (6, -1), (7, 129), (8, p + 8), (0, p + 8), (4, p + 4)])
    mk_f = [p, 1, 80 * 784, 784, 28, 1, p, p, p, 16, 80, 28, p, p, None]
    each_bad("pswin_mask_bce_rows_fwd", mk_f, [(0, None), (6, None), (7, None), (8, None), (12, None), (9, 0), (10, 0), (10, 129), (11, 0), (11, 57),
                                               (2, 0), (5, -1), (0, p + 1), (1, 3), (13, p + 2)])
    mk_b = [p, 1, 80 * 784, 1, 28 * 80, 80, p, p, p, p, 16, 80, 28, p, None]
    each_bad("pswin_mask_bce_rows_bwd", mk_b, [(0, None), (9, None), (13, None), (12, 57), (11, 129), (10, -2), (3, 2), (2, 80 * 784 + 8), (4, 28),
                                               (13, p + 1)])
    rp_f = [p, p, p, p, p, p, 2, 1000, 24, 8, p, None]
    each_bad("pswin_rpn_losses_fwd", rp_f, [(0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (10, None), (6, 0), (7, 0), (8, 0),
                                            (9, 0), (9, 25), (1, p + 4), (5, p + 8), (2, p + 4), (7, -3), (7, 1 << 29)])
    rp_b = [p, p, p, p, p, p, p, 2, 1000, 24, 8, p, p, None]
    each_bad("pswin_rpn_losses_bwd", rp_b, [(6, None), (11, None), (12, None), (10, 25), (9, -1), (12, p + 4), (11, p + 2), (7, 70000)])


def test_the_python_wrappers_send_cpu_tensors_to_the_definitions():
    from panoswintransformerobjectdetection_amd import ops
    cls, labels, _ = cases.ce_case(9, 6)
    assert torch.equal(ops.ce_rows(cls, labels), losses.ce_rows(cls, labels))
    reg, labels, weight, target, _ = cases.l1_case(9, 5)
    assert torch.equal(ops.l1_rows(reg, labels, weight, target), losses.l1_rows(reg, labels, weight, target))
    logits, labels, target, weight, _ = cases.mask_case(3, 5, 7)
    assert torch.equal(ops.mask_bce_rows(logits, labels, target, weight), losses.mask_bce_rows(logits, labels, target, weight))
    args = cases.rpn_case(100)[:6]
    assert torch.equal(ops.rpn_losses(*args), losses.rpn_losses(*args))


def test_pswin_disable_knows_loss_kernels():
    """(in a process of its own: the switches are read once, at import)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import panoswintransformerobjectdetection_amd.ops as o; print(int(o.LOSS_KERNELS), int(o.GEMM_NT))"
    for value, want in (("loss_kernels", ["0", "1"]), ("gemm_nt", ["1", "0"])):
        env = dict(os.environ, PSWIN_DISABLE=value, PYTHONPATH=root)
        assert subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.split() == want


# ---- the hooks of both models --------------------------------------------------------------------------------------------------------
def _record(m, names=("rpn_loss", "cls_loss", "box_loss", "mask_loss")):
    calls = {k: 0 for k in names}
    for k in names:
        def hook(*a, _k=k, _fn=getattr(m, k)):
            calls[_k] += 1
            return _fn(*a)
        setattr(m, k, hook)
    return calls


def test_heads_loss_of_both_models_calls_every_hook_once_per_loss():
    import _cascade_cases as cc
    from panoswintransformerobjectdetection_amd import detector as det
    from _util import TINY
    feats_of = lambda m: cc.feature_maps(m)                                                    # noqa: E731
    T = cc.padded(cc.annotations((6, 0)), 8)
    torch.manual_seed(0)
    m = det.MiniMaskRCNN(dict(TINY, compute_dtype=torch.float32), num_classes=cc.NUM_CLASSES).train()
    m.roi_align, m.rand_like = cc.point_roi_align, cc.layout_keys(8)
    m.rpn_cfg = dict(m.rpn_cfg, nms_pre=2000, max_per_img=2000)                                # the proposals cc.layout_keys hands keys to
    calls = _record(m)
    with torch.no_grad():
        ls = m.heads_loss(feats_of(m), T, (cc.H, cc.W))
    assert set(ls) == {"loss_rpn_cls", "loss_rpn_bbox", "loss_cls", "loss_bbox", "loss_mask"} and all(np.isfinite(float(v)) for v in ls.values())
    assert calls == dict(rpn_loss=1, cls_loss=1, box_loss=1, mask_loss=1)
    c = cc.tiny_model()
    c.roi_align, c.rand_like = cc.point_roi_align, cc.layout_keys(8)
    calls = _record(c)
    with torch.no_grad():
        ls = c.heads_loss(feats_of(c), T, (cc.H, cc.W))
    assert len(ls) == 11 and all(np.isfinite(float(v)) for v in ls.values())
    assert calls == dict(rpn_loss=1, cls_loss=3, box_loss=0, mask_loss=3)                        # the cascade's box loss stays giou_rows
