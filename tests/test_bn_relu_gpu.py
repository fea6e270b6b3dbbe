"""The stand-alone BatchNorm2d + ReLU kernels (csrc/pswin_bn.hip: bn_reduce_kernel in both modes, bn_finalize, bn_eval_params, bn_scale_shift,
bn_relu_apply, bn_bwd_finalize, bn_relu_bwd_apply) against the float64 definition of tests/_bn_cases.py, inside its derived bounds, through
ops.batch_norm_relu on a real nn.BatchNorm2d with autograd and again through the entry points pswin_bn_relu_fwd / pswin_bn_relu_bwd.

Widths 8, 40, 64, 96 and C / VE == 256 (lane tails with idle threads, one group per row, one row per block step) at row counts around
the rows per block step and the first and the third block; one row; pre_bias or none, momentum 0.1 and the cumulative average,
track_running_stats=False; two shapes beyond one sweep of the capped reduce and apply grids.  The inputs plant a constant channel (variance
exactly 0), a constant 0.1 (the clamp), a mean at 30 sigma, gamma = 0, a dead channel and negative gammas; no element lies within 8 x
its allowed error of the ReLU's boundary (tests/test_bn_cases.py), so the masks agree and nothing is excluded from any comparison.

Every case runs three times: twice through autograd on fresh tensors (the same bits are required: the sums have a fixed order) and once
through the entry points with every output and the whole workspace filled with NaN beforehand (the same bits again, no NaN: every output
element is written and nothing is read from the workspace before it is written).

The apply grids' cap is reported by no entry point; this table is the record of it, as in tests/test_kernel_trips_gpu.py:
  APPLY_MAX_BLOCKS = 8192     pswin_bn.hip:213 apply_blocks(), 256 sixteen-byte groups per block and trip (:152, :187)
  MAX_BLOCKS       = 1024     pswin_bn.hip:21, asserted through pswin_bn_workspace(C) == (2 * 1024 + 6) * C

Measured on the MI355X: the kernels' largest error / bound per output, the largest over the cases of a row (n of them; the cumulative
average over its three steps), and the slowest case's wall time.  z and dy in bf16 sit at 1 because half a bf16 ulp is nearly all of
their bound and some element always lands next to a rounding tie; the sums' bounds count a worst case per addition, which random
rounding errors stay far below.  The float32 mirror of tests/test_bn_cases.py gives the same picture on the CPU (0.2 to 0.5 on the
statistics in training).  These figures are recorded (_util.record, "bn:<case>") and never affect a verdict.

  cases                                     n        z     mean     rstd run_mean  run_var       dy   dgamma    dbeta     dpre  slowest
  beyond one sweep             bf16 eval    1        1    0.928    0.303        -        -        1   0.0078 0.000109 0.000121  0.04 s
  beyond one sweep             bf16 train   1    0.998   0.0358   0.0322    0.115   0.0768    0.999  0.00377 0.000126        -  0.04 s
  beyond one sweep             f32  eval    1    0.478     0.95     0.22        -        -    0.342  0.00596 0.000275 0.000325  0.03 s
  beyond one sweep             f32  train   1   0.0406   0.0234   0.0342   0.0928   0.0882   0.0512  0.00309 0.000253        -  0.04 s
  cumulative average, 3 steps  bf16 train   1    0.997   0.0162   0.0369   0.0813   0.0863    0.998  0.00268  0.00142        -  0.02 s
  cumulative average, 3 steps  f32  train   1   0.0422   0.0331   0.0395    0.162   0.0972   0.0474  0.00431   0.0093        -  0.01 s
  no running statistics        bf16 eval    1    0.997   0.0162   0.0359        -        -    0.998  0.00268  7.5e-05        -  0.00 s
  no running statistics        bf16 train   1    0.997   0.0162   0.0359        -        -    0.998  0.00268  7.5e-05        -  0.00 s
  no running statistics        f32  eval    1   0.0422   0.0311   0.0395        -        -   0.0446  0.00349   0.0093        -  0.00 s
  no running statistics        f32  train   1   0.0422   0.0311   0.0395        -        -   0.0446  0.00349   0.0093        -  0.00 s
  one row                      bf16 eval    1    0.998    0.972     0.24        -        -    0.939     0.72        0        0  0.00 s
  one row                      bf16 train   1    0.792        0    0.349    0.266    0.214        0        0        0        -  0.00 s
  one row                      f32  eval    1    0.426    0.937    0.275        -        -    0.311    0.901        0        0  0.00 s
  one row                      f32  train   1    0.423        0    0.229    0.213    0.206        0        0        0        -  0.00 s
  pre_bias / none              bf16 eval    2        1    0.811    0.262        -        -        1   0.0104 7.32e-05 0.000687  0.00 s
  pre_bias / none              bf16 train   2    0.997   0.0162   0.0359    0.139   0.0952    0.998  0.00268  7.5e-05        -  0.00 s
  pre_bias / none              f32  eval    2    0.433    0.823    0.273        -        -    0.359   0.0141   0.0122   0.0161  0.00 s
  pre_bias / none              f32  train   2   0.0422   0.0311   0.0395    0.172   0.0728   0.0446  0.00349   0.0093        -  0.00 s
  widths and rows              bf16 eval   22        1        1    0.363        -        -        1    0.977 0.000968    0.002  0.01 s
  widths and rows              bf16 train  22        1    0.035    0.286    0.338    0.242    0.999    0.178 0.000826        -  0.01 s
  widths and rows              f32  eval   22    0.534    0.999    0.338        -        -    0.425    0.873    0.482    0.456  0.21 s
  widths and rows              f32  train  22    0.435    0.332    0.483    0.305    0.448    0.455    0.465     0.34        -  1.27 s
"""
import copy
import math
import time

import pytest
import torch
import torch.nn as nn

import _bn_cases as B
from _util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
BITS = ("z", "save_mean", "save_rstd", "running_mean", "running_var", "dy", "dgamma", "dbeta")


def _L():
    from panoswintransformerobjectdetection_amd import _lib
    return _lib


def _dev4(rows, dtype):
    """[M, C] CPU rows -> the [1, C, 1, M] channels-last tensor of `dtype` on the device"""
    return B.rows4(rows.to(DEV).to(dtype))


def _rows(t4):
    return t4.detach().permute(0, 2, 3, 1).reshape(-1, t4.shape[1])


def _module(c, momentum, track=True):
    bn = nn.BatchNorm2d(c.C, momentum=momentum, track_running_stats=track)
    with torch.no_grad():
        bn.weight.copy_(c.gamma); bn.bias.copy_(c.beta)
        if track:
            bn.running_mean.copy_(c.running_mean); bn.running_var.copy_(c.running_var); bn.num_batches_tracked.fill_(B.NBT0)
    return bn.to(DEV)


def _node(t):
    f = t.grad_fn
    assert type(f).__name__ == "_BatchNormReLUBackward", type(f).__name__
    return f


def _autograd(ops, c, bn, train, pre):
    """one forward and backward through ops.batch_norm_relu -> the outputs as [M, C] rows and [C] vectors (device tensors)"""
    y = _dev4(c.y, c.dtype).requires_grad_(True)
    pb = c.pre_bias.to(DEV).requires_grad_(True) if pre else None
    z = ops.batch_norm_relu(y, bn, train, pb)
    assert z.dtype == c.dtype and z.shape == y.shape and z.stride() == y.stride()
    _, _, _, mean, rstd = _node(z).saved_tensors
    z.backward(_dev4(c.dz, c.dtype))
    assert y.grad.dtype == c.dtype and bn.weight.grad.dtype == F32
    return dict(z=_rows(z), save_mean=mean.clone(), save_rstd=rstd.clone(), dy=_rows(y.grad), dgamma=bn.weight.grad.clone(),
                dbeta=bn.bias.grad.clone(), dpre=None if pb is None else pb.grad.clone(),
                running_mean=None if bn.running_mean is None else bn.running_mean.clone(),
                running_var=None if bn.running_var is None else bn.running_var.clone())


def _entry(c, batch, momentum, pre, rm, rv):
    """the same through pswin_bn_relu_fwd / pswin_bn_relu_bwd, every output and the workspace NaN beforehand; rm / rv: the running
    statistics to read or update (clones are used), or None"""
    L = _L()
    M, C = c.M, c.C
    nan = lambda *shape, dt=F32: torch.full(shape, float("nan"), dtype=dt, device=DEV)
    y, dz = _dev4(c.y, c.dtype), _dev4(c.dz, c.dtype)
    gamma, beta = c.gamma.to(DEV), c.beta.to(DEV)
    pb = c.pre_bias.to(DEV) if pre else None
    rm, rv = (None, None) if rm is None else (rm.clone(), rv.clone())
    z, dy = nan(M, C, dt=c.dtype), nan(M, C, dt=c.dtype)
    mean, rstd, dgamma, dbeta = nan(C), nan(C), nan(C), nan(C)
    n_ws = L.load().pswin_bn_workspace(C)
    ws = nan(n_ws)
    code = L.dtype_code(y)
    L.call("pswin_bn_relu_fwd", y, L.ptr(y), code, L.ptr(gamma), L.ptr(beta), L.ptr(pb), float(B.EPS), float(momentum), int(batch),
           L.ptr(rm), L.ptr(rv), L.ptr(z), L.ptr(mean), L.ptr(rstd), L.ptr(ws), M, C)
    ws2 = nan(n_ws)
    L.call("pswin_bn_relu_bwd", y, L.ptr(dz), L.ptr(y), code, L.ptr(gamma), L.ptr(beta), L.ptr(mean), L.ptr(rstd), int(batch),
           L.ptr(dy), L.ptr(dgamma), L.ptr(dbeta), L.ptr(ws2), M, C)
    return dict(z=z, save_mean=mean, save_rstd=rstd, dy=dy, dgamma=dgamma, dbeta=dbeta, running_mean=rm, running_var=rv)


class _Verdict:
    def __init__(self, name):
        self.name, self.t0, self.worst, self.bad = name, time.perf_counter(), {}, []

    def ratios(self, q, tag=""):
        for k, v in q.items():
            self.worst[k + tag] = max(self.worst.get(k + tag, 0.0), v) if v == v else float("inf")
            if not v <= 1.0:
                self.bad.append(f"{k}{tag}: error / bound = {v:.4g}")

    def check(self, ok, what):
        if not ok:
            self.bad.append(what)

    def done(self):
        torch.cuda.synchronize()
        secs = time.perf_counter() - self.t0
        print(f"bn:{self.name} seconds={secs:.2f} " + " ".join(f"{k}={v:.3g}" for k, v in self.worst.items()))
        record("bn:" + self.name, seconds=secs, **self.worst)
        assert not self.bad, "\n".join(self.bad)


def _ratio(err, bound):
    """largest err / bound; where the bound is 0 the error must be"""
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def _same_bits(v, a, b, what):
    for k in BITS:
        if a.get(k) is None and b.get(k) is None:
            continue
        v.check(a[k].shape == b[k].shape and torch.equal(a[k], b[k]), f"{k}: {what}")
        v.check(bool(torch.isfinite(b[k].float()).all()), f"{k}: not finite ({what})")


def _run(ops, v, c, train, momentum=0.1, pre=True, track=True, device="cpu", bn=None, step=0):
    """One case in one mode: autograd twice on fresh tensors, the entry points once, the first run against the float64 definition.
    bn: a module that carries its state from an earlier step (then the repeat runs use copies of it)."""
    batch = train or not track
    bn = _module(c, momentum, track) if bn is None else bn
    twin = copy.deepcopy(bn)
    old = None if not track else (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked))
    got = _autograd(ops, c, bn.train(train), train, pre)
    again = _autograd(ops, c, twin.train(train), train, pre)
    _same_bits(v, got, again, "two runs on the same inputs differ")
    update = train and track
    m = (momentum if momentum is not None else 1.0 / (old[2] + 1)) if update else 0.0
    ent = _entry(c, batch, m, pre, old[0] if track else None, old[1] if track else None)
    _same_bits(v, got, ent, "the entry points on NaN-filled outputs and workspace differ from the autograd path")
    # the float64 definition, anchored on the running statistics the kernel started from
    to = lambda t: t.to(device)
    r = B.reference(to(c.y), to(c.dz), to(c.gamma), to(c.beta), to(c.pre_bias) if pre else None, to(old[0]) if track else None,
                    to(old[1]) if track else None, batch, m if update else None)
    tol = B.bounds(r, c.dtype, to(c.gamma), to(c.beta))
    v.check(B.condition(c, r, tol) >= 8.0, "an element is near the ReLU boundary")
    cmp = {k: (None if t is None else to(t)) for k, t in got.items()}
    v.ratios(B.ratios(cmp, r, tol), f"@{step}" if step else "")
    for what in B.exact_failures(cmp, c, batch):
        v.check(False, what)
    if track:
        v.check(int(bn.num_batches_tracked) == old[2] + int(train), "num_batches_tracked")
        if not update:
            v.check(torch.equal(bn.running_mean, old[0]) and torch.equal(bn.running_var, old[1]), "eval mode wrote the running statistics")
    else:
        v.check(bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None, "buffers appeared")
    if pre:
        if batch:                                   # a constant in front of batch statistics: exactly zero
            v.check(got["dpre"].dtype == F32 and float(got["dpre"].abs().max()) == 0.0, "dpre is not exactly 0")
        else:
            # dpre = ops.colsum of the dy the kernel stored, against the float64 sum of those same values
            chain = _colsum_chain(c.M, c.C, c.dtype)
            dyk = got["dy"].double()
            err = (got["dpre"].double() - dyk.sum(0)).abs()
            bound = chain * B.U * dyk.abs().sum(0)
            v.ratios({"dpre": _ratio(err, bound)})
            # and against the definition's column sum: the bound of every dy element on top
            v.ratios({"dpre_def": _ratio((got["dpre"].double().cpu() - r.dpre.cpu()).abs(), bound.cpu() + tol["dy"].sum(0).cpu())})
    return got, r


def _sum_rows_chain(rows):
    """reduce_jobs_kernel (pswin_move.hip): up to 16 rows in one lane, up to 128 in 8 lanes and a chain of 8, more in 64 lanes and two
    chains of 8"""
    return rows if rows <= 16 else -(-rows // 8) + 8 if rows <= 128 else -(-rows // 64) + 16


def _colsum_chain(M, C, dtype):
    """the longest chain of f32 additions in ops.colsum of [M, C]: sum_rows up to 4096 rows; beyond, rowsum_partial_kernel (at least 8
    rows a lane, at most 2048 blocks, the rpi lanes of a block added one after the other) and sum_rows over the blocks' rows"""
    if M <= 4096:
        return _sum_rows_chain(M)
    r = B.rpi(C, dtype)
    blocks = min(-(-M // (8 * r)), 2048)
    return -(-M // (blocks * r)) + r + _sum_rows_chain(blocks)


def _name(v, train, extra=""):
    return f"{B.case_id(v)}:{'train' if train else 'eval'}{extra}"


# ---- widths and rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", B.GRID, ids=B.case_id)
def test_widths_and_rows(ops, case, train):
    C, M, dt, seed = case
    v = _Verdict(_name(case, train))
    _run(ops, v, B.case(M, C, dt, seed, train), train)
    v.done()


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dt", B.DTYPES, ids=B.name)
def test_one_row(ops, dt, train):
    """M = 1.  Eval: the definition.  Training: the kernel's stated choice, which is the definition with the biased variance 0 kept in
    the running update (no division by M - 1 = 0): z = relu(beta), rstd = 1 / sqrt(eps) -- to 3 ulps wherever y^2 is exact in f32
    (every bf16 value, the constant channel); an f32 y leaves var = fl(y^2) - y^2 >= 0 instead of 0, which the bound carries --,
    dy = 0 and a finite running variance moved towards 0."""
    case = (B.MODE_C, 1, dt, 0)
    c = B.case(1, B.MODE_C, dt, 0, train)
    v = _Verdict(_name(case, train))
    got, r = _run(ops, v, c, train)
    if train:
        want = 1.0 / math.sqrt(B.EPS32)
        assert float(r.var.abs().max()) == 0.0
        assert torch.equal(r.z.cpu()[0], torch.relu(c.beta.double()))
        rstd = got["save_rstd"].cpu().double()
        exact = torch.ones(c.C, dtype=torch.bool) if dt == BF16 else (c.y[0].double() ** 2 == (c.y[0] * c.y[0]).double())
        assert bool(exact[0]) and bool(((rstd - want).abs() <= 3 * B.ULP * want)[exact].all())
        assert float(got["dy"].float().abs().max()) == 0.0
        rv = got["running_var"].cpu()
        assert bool(torch.isfinite(rv).all()) and bool((rv <= c.running_var).all())
    v.done()


# ---- modes -------------------------------------------------------------------------------------------------------------------------------
def _mode_case(dt, train, seed=2, pre=True):
    C, M = B.mode_shape(dt)
    return (C, M, dt, seed), B.case(M, C, dt, seed, train, pre=pre)


@pytest.mark.parametrize("pre", [True, False], ids=["pre_bias", "no_pre_bias"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dt", B.DTYPES, ids=B.name)
def test_pre_bias_and_none(ops, dt, train, pre):
    """momentum 0.1 with and without the convolution bias in front: it only moves the running mean (training) or the mean (eval, where
    its gradient is the column sum of dy)"""
    case, c = _mode_case(dt, train, pre=pre)
    v = _Verdict(_name(case, train, ":pre" if pre else ":nopre"))
    _run(ops, v, c, train, pre=pre)
    v.done()


@pytest.mark.parametrize("dt", B.DTYPES, ids=B.name)
def test_cumulative_average_three_steps(ops, dt):
    """momentum=None: weight 1 / num_batches_tracked.  Three steps on one module, a new batch each, forward, backward and running
    statistics checked at every step (each step's definition starts from the running statistics the kernel held before it)."""
    C, M = B.mode_shape(dt)
    v = _Verdict(f"C{C}-M{M}-{B.name(dt)}:cumulative")
    bn = None
    for step in range(3):
        c = B.case(M, C, dt, 2 + 2 * step, True)
        if bn is None:
            bn = _module(c, None)
        with torch.no_grad():
            bn.weight.copy_(c.gamma); bn.bias.copy_(c.beta)
        bn.weight.grad = bn.bias.grad = None
        _run(ops, v, c, True, momentum=None, bn=bn, step=step + 1)
        assert int(bn.num_batches_tracked) == B.NBT0 + step + 1
    v.done()


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dt", B.DTYPES, ids=B.name)
def test_without_running_statistics(ops, dt, train):
    """track_running_stats=False: batch statistics in train() and in eval(), no buffers, an exactly zero dpre"""
    case, c = _mode_case(dt, True)
    v = _Verdict(_name(case, train, ":untracked"))
    _run(ops, v, c, train, track=False)
    v.done()


# ---- beyond one sweep of the capped grids ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dt", B.DTYPES, ids=B.name)
def test_beyond_one_sweep(ops, dt, train):
    """f32 C = 40 (10 groups a row) at 419,509 rows and bf16 C = 64 (8 groups a row) at 524,400: both apply kernels make a third trip
    and bn_reduce_kernel runs at its capped grid; rows at the seams of both grids carry 64 x the deviation and 64 x dz, so that one
    dropped or doubled row moves the sums far beyond their bound.  The float64 definition is evaluated on the device."""
    C, M = B.BIG[dt]
    n_vec = M * B.vpr(C, dt)
    assert _L().load().pswin_bn_workspace(C) == (2 * B.MAX_BLOCKS + 6) * C
    assert n_vec > 2 * B.APPLY_MAX_BLOCKS * B.THREADS and -(-n_vec // (B.APPLY_MAX_BLOCKS * B.THREADS)) == 3
    assert M > B.MAX_BLOCKS * B.rpi(C, dt) * 16 and B.reduce_blocks(M, C, dt) == B.MAX_BLOCKS
    case = (C, M, dt, B.BIG_SEED)
    c = B.case(M, C, dt, B.BIG_SEED, train, plant=True, device=DEV)
    rs, sa = B.reduce_sweep(M, C, dt), B.APPLY_MAX_BLOCKS * B.THREADS // B.vpr(C, dt)
    assert {0, M - 1, rs - 1, rs, (M - 1) // rs * rs, sa, 2 * sa} <= set(c.planted) and len(c.planted) >= 36
    v = _Verdict(_name(case, train))
    _run(ops, v, c, train, device=DEV)
    v.done()


# ---- rejections --------------------------------------------------------------------------------------------------------------------------
def _reject_entry(C, M, dt):
    """both entry points must return an error for this shape and leave every output as it was"""
    L = _L()
    nan = lambda *shape, d=F32: torch.full(shape, float("nan"), dtype=d, device=DEV)
    y = torch.zeros(M, C, dtype=dt, device=DEV)
    gamma, beta, rm, rv = torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    z, dy, mean, rstd, dgamma, dbeta = nan(M, C, d=dt), nan(M, C, d=dt), nan(C), nan(C), nan(C), nan(C)
    ws = nan((2 * B.MAX_BLOCKS + 6) * C)
    code = L.dtype_code(y)
    with pytest.raises(L.PswinError, match="invalid argument"):
        L.call("pswin_bn_relu_fwd", y, L.ptr(y), code, L.ptr(gamma), L.ptr(beta), None, 1e-5, 0.1, 1, L.ptr(rm), L.ptr(rv), L.ptr(z),
               L.ptr(mean), L.ptr(rstd), L.ptr(ws), M, C)
    with pytest.raises(L.PswinError, match="invalid argument"):
        L.call("pswin_bn_relu_bwd", y, L.ptr(y), L.ptr(y), code, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), 1, L.ptr(dy),
               L.ptr(dgamma), L.ptr(dbeta), L.ptr(ws), M, C)
    torch.cuda.synchronize()
    for t in (z, dy, mean, rstd, dgamma, dbeta, ws):
        assert bool(torch.isnan(t.float()).all())
    assert float(rm.abs().max()) == 0.0 and float((rv - 1).abs().max()) == 0.0


@pytest.mark.parametrize("C,dt", [(12, F32), (12, BF16), (1032, F32), (4, F32)], ids=["C12-f32", "C12-bf16", "C1032-f32", "C4-f32"])
def test_unsupported_widths_are_rejected(ops, C, dt):
    _reject_entry(C, 5, dt)
    bn = nn.BatchNorm2d(C).to(DEV)
    before = copy.deepcopy(bn.state_dict())
    y = B.rows4(torch.zeros(5, C, dtype=dt, device=DEV))
    with pytest.raises(_L().PswinError):
        ops.batch_norm_relu(y, bn, True)
    assert torch.equal(bn.running_mean, before["running_mean"]) and torch.equal(bn.running_var, before["running_var"])


def test_cpu_tensor_and_layout_are_rejected(ops):
    C = 8
    bn = nn.BatchNorm2d(C)
    with pytest.raises(_L().PswinError, match="CPU tensor"):
        ops.batch_norm_relu(B.rows4(torch.zeros(5, C)), bn, True)
    assert float(bn.running_mean.abs().max()) == 0.0
    bn = bn.to(DEV)
    with pytest.raises(AssertionError, match="channels-last"):
        ops.batch_norm_relu(torch.zeros(2, C, 3, 5, device=DEV), bn, True)          # NCHW-contiguous
    torch.cuda.synchronize()
    assert float(bn.running_mean.abs().max()) == 0.0 and float((bn.running_var - 1).abs().max()) == 0.0
