"""tests/_bn_cases.py checked on the CPU before anything goes to a GPU: the ReLU condition of every case tests/test_bn_relu_gpu.py runs, the
hand-written float64 definition against nn.BatchNorm2d in float64 with autograd, a float32 mirror of the kernels' formulas inside every
bound at every case (the bounds are not too tight), and the same mirror with one defect at a time outside a bound (they are not too loose)."""
import functools

import pytest
import torch
import torch.nn as nn

import _bn_cases as B

F32, BF16 = torch.float32, torch.bfloat16
MOMENTUM = 0.1
BIG_CASES = [B.BIG[dt] + (dt, B.BIG_SEED) for dt in B.DTYPES]
ONE_ROW = [(B.MODE_C, 1, dt, 0) for dt in B.DTYPES]
MODE_CASES = [B.mode_shape(dt) + (dt, seed) for dt in B.DTYPES for seed in (2, 4, 6)]        # 4, 6: the later steps of the cumulative average
ALL = B.GRID + ONE_ROW + MODE_CASES + BIG_CASES


@functools.lru_cache(maxsize=2)
def _checked(v, batch, pre=True):
    C, M, dt, seed = v
    c = B.case(M, C, dt, seed, batch, plant=v in BIG_CASES, pre=pre)
    r, tol = B.case_reference(c, batch, MOMENTUM if batch else None, pre)
    return c, r, tol


@pytest.mark.parametrize("batch", [True, False], ids=["batch", "running"])
@pytest.mark.parametrize("v", ALL, ids=B.case_id)
def test_no_element_near_the_relu_boundary(v, batch):
    """smallest |p| / (allowed error of p) >= 8 with nothing excluded, the dead channel is dead, the planted channels are what they say"""
    c, r, tol = _checked(v, batch)
    factor = B.condition(c, r, tol)
    print(B.case_id(v), "batch" if batch else "running", f"factor {factor:.1f} moved {c.moved} in {c.passes} passes")
    assert factor >= 8.0
    if c.dtype == BF16:
        assert torch.equal(c.y, B.bf16_exact(c.y)) and torch.equal(c.dz, B.bf16_exact(c.dz))
    if batch and c.M > 1:
        assert float(r.var[0]) == 0.0 and float(r.mean[0]) == 1.5
        if c.C > 2:
            assert abs(float(r.mean[2])) > 20 / float(r.rstd[2])
    if c.C > 4:
        assert float(r.z[:, 4].max()) == 0.0 and float(c.gamma[3]) == 0.0 and int((c.gamma < 0).sum()) >= 2


@pytest.mark.parametrize("batch", [True, False], ids=["batch", "running"])
@pytest.mark.parametrize("v", MODE_CASES[::3], ids=B.case_id)
def test_without_pre_bias(v, batch):
    """the cases built for a call without pre_bias: the condition, and the mirror inside every bound"""
    c, r, tol = _checked(v, batch, False)
    assert float(c.pre_bias.abs().max()) == 0.0 and B.condition(c, r, tol) >= 8.0
    got = B.mirror(c, batch, MOMENTUM if batch else None, pre=False)
    q = B.ratios(got, r, tol)
    _report(f"mirror {B.case_id(v)} {'batch' if batch else 'running'} no pre_bias", q)
    assert all(x <= 1.0 for x in q.values()), q
    assert not B.exact_failures(got, c, batch)


@pytest.mark.parametrize("batch", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("v", [v for v in B.GRID + MODE_CASES if v[0] <= 96], ids=B.case_id)
def test_definition_is_batchnorm2d_in_float64(v, batch):
    """reference() against ReLU(nn.BatchNorm2d(...).double()(y + pre_bias)) and autograd, to 5e-8 of the largest value of each output"""
    c, r, _ = _checked(v, batch)
    bn = nn.BatchNorm2d(c.C, momentum=MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(c.gamma); bn.bias.copy_(c.beta); bn.running_mean.copy_(c.running_mean); bn.running_var.copy_(c.running_var)
    bn = bn.double().train(batch)
    assert bn.eps == B.EPS
    y = B.rows4(c.y.double()).clone().requires_grad_(True)
    pre = c.pre_bias.double().clone().requires_grad_(True)
    z = torch.relu(bn(y + pre.view(1, -1, 1, 1)))
    (z * B.rows4(c.dz.double())).sum().backward()
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(c.M, c.C)
    # the definition uses the f32 value of 1e-5 the kernel is handed (2.5e-8 off 1e-5: 1.3e-8 of rstd where the variance is 0)
    if batch:                  # a constant in front of batch statistics: autograd leaves rounding noise, the definition says 0
        assert float(r.dpre.abs().max()) == 0.0 and float(pre.grad.abs().max()) <= 1e-9 * float(y.grad.abs().sum())
        pre.grad.zero_()
    for got, want, what in ((r.z, rows(z), "z"), (r.dy, rows(y.grad), "dy"), (r.dgamma, bn.weight.grad, "dgamma"), (r.dbeta, bn.bias.grad, "dbeta"),
                            (r.dpre, pre.grad, "dpre"), (r.running_mean, bn.running_mean, "running_mean"),
                            (r.running_var, bn.running_var, "running_var")):
        scale = float(want.detach().abs().max())
        assert float((got - want.detach()).abs().max()) <= 5e-8 * scale, (what, float((got - want.detach()).abs().max()), scale)


def _report(what, q):
    print(what, " ".join(f"{k}={v:.3g}" for k, v in q.items()))


@pytest.mark.parametrize("batch", [True, False], ids=["batch", "running"])
@pytest.mark.parametrize("v", ALL, ids=B.case_id)
def test_float32_mirror_is_inside_every_bound(v, batch):
    c, r, tol = _checked(v, batch)
    got = B.mirror(c, batch, MOMENTUM if batch else None)
    q = B.ratios(got, r, tol)
    _report(f"mirror {B.case_id(v)} {'batch' if batch else 'running'}", q)
    assert set(q) >= {"z", "save_mean", "save_rstd", "dy", "dgamma", "dbeta"}
    assert all(x <= 1.0 for x in q.values()), q
    assert not B.exact_failures(got, c, batch)


# which cases a defect must be caught at: every one where it changes anything by more than rounding
MID = [v for v in B.GRID if v[0] <= 96 and v[1] > 2 * B.rpi(v[0], v[2])] + MODE_CASES
SMALL_AND_MID = [v for v in B.GRID if v[0] <= 96] + MODE_CASES
DEFECT_CASES = {
    "drop_last_row": SMALL_AND_MID + BIG_CASES,
    "double_sweep_row": MID + BIG_CASES,
    "mask_ge": [v for v in B.GRID if v[3] % 2 == 1 and v[0] <= 96] + BIG_CASES,
    "no_mgx": MID,
    "mean_m1": SMALL_AND_MID,
    "rv_biased": SMALL_AND_MID,
    "rm_no_pre": SMALL_AND_MID,
    "neg_gamma_mask": MID,
}


@pytest.mark.parametrize("defect", B.DEFECTS)
def test_a_defective_mirror_is_outside_a_bound(defect):
    assert DEFECT_CASES[defect]
    missed = []
    for v in DEFECT_CASES[defect]:
        c, r, tol = _checked(v, True)
        got = B.mirror(c, True, MOMENTUM, defect=defect)
        q = B.ratios(got, r, tol)
        worst = max(q, key=q.get)
        print(defect, B.case_id(v), f"{worst}={q[worst]:.3g}", B.exact_failures(got, c, True)[:1])
        if q[worst] <= 1.0 and not B.exact_failures(got, c, True):
            missed.append((B.case_id(v), q))
    assert not missed, missed
