"""Shared by tests/test_bn_cases.py (CPU) and tests/test_bn_relu_gpu.py: the inputs, the float64 statement of ReLU(BatchNorm2d(y + pre_bias))
with its backward, the error bounds the kernels of csrc/pswin_bn.hip are held to, and a float32 mirror of the kernels' formulas.

Every bound counts correctly rounded f32 operations on the kernel's own order of operations (U = 2^-24 is the most one of them loses,
relative to its result; ULP = 2 U), with the count in a comment beside it.  None was taken from a kernel's output.  All functions work on
[M, C] rows and take tensors of any device, so the large cases are evaluated where their data lives."""
import functools
import math
import types

import torch

from _losses_cases import bf16_exact, half_ulp_bf16

U = 2.0 ** -24                   # unit roundoff of f32
ULP = 2.0 ** -23
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))        # the eps the kernels see (a float argument)
THREADS, MAX_BLOCKS, APPLY_MAX_BLOCKS = 256, 1024, 8192      # pswin_bn.hip: THREADS, MAX_BLOCKS, apply_blocks()
NBT0 = 3                         # num_batches_tracked before the first step
OUTPUTS = ("z", "save_mean", "save_rstd", "running_mean", "running_var", "dy", "dgamma", "dbeta")


# ---- the kernels' launch arithmetic ------------------------------------------------------------------------------------------------------
def ve(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def vpr(C, dtype):
    return C // ve(dtype)


def rpi(C, dtype):
    """rows per block step of bn_reduce_kernel"""
    return THREADS // vpr(C, dtype)


def reduce_blocks(M, C, dtype):
    """reduce_blocks() of pswin_bn.hip"""
    r = rpi(C, dtype)
    return max(1, min(MAX_BLOCKS, (M + 16 * r - 1) // (16 * r)))


def reduce_sweep(M, C, dtype):
    """rows one trip of bn_reduce_kernel's grid covers"""
    return reduce_blocks(M, C, dtype) * rpi(C, dtype)


def chain(M, C, dtype):
    """The longest chain of f32 additions behind a per-channel sum: a lane's trips over the rows, the rpi adds of the LDS merge, then
    colsum_kernel (pswin_common.hpp) over the blocks' partial rows: at most ceil(blocks / 64) adds in a row lane, 2 for its four
    accumulators, 2 for the 4-way merge and 16 for the last serial loop.  An addition to an accumulator that is still 0 is exact, so M rows
    never cost more than M roundings (M - 1 additions and the fused product of the first term)."""
    nb = reduce_blocks(M, C, dtype)
    trips = -(-M // (nb * rpi(C, dtype)))
    return min(trips + rpi(C, dtype) + -(-nb // 64) + 20, M)


def m_values(C, dtype):
    r = rpi(C, dtype)
    return (2, 37) if vpr(C, dtype) == THREADS else (2, r - 1, r + 1, 16 * r + 1, 3 * 16 * r + 5)


# the two cases beyond one sweep of the capped grids: dtype -> (C, M)
BIG = {torch.float32: (40, 419509), torch.bfloat16: (64, 524400)}


def planted_rows(M, C, dtype):
    """rows whose loss or doubling must move a sum beyond its bound: the first and the last row, and the last row of every sweep of the
    reduce grid and of the apply grid with the first row of the next"""
    rows = {0, M - 1}
    rs = reduce_sweep(M, C, dtype)
    sa = APPLY_MAX_BLOCKS * THREADS
    for k in range(1, -(-M // rs)):
        rows |= {k * rs - 1, k * rs}
    for k in range(1, -(-(M * vpr(C, dtype)) // sa)):
        rows |= {k * sa // vpr(C, dtype) - 1, k * sa // vpr(C, dtype), k * sa // vpr(C, dtype) + 1}
    return sorted(r for r in rows if 0 <= r < M)


# ---- the float64 definition --------------------------------------------------------------------------------------------------------------
def reference(y, dz, gamma, beta, pre_bias, running_mean, running_var, batch, momentum, eps=EPS32, backward=True):
    """ReLU(BatchNorm2d(y + pre_bias)) and its gradients in float64, by hand (nn.BatchNorm2d refuses one value per channel in training).
    y, dz: [M, C]; the rest [C] or None.  batch: statistics of the batch (train(), or no running statistics), else the running ones.
    momentum: None leaves the running statistics alone; otherwise they are updated with it (batch only).  pre_bias only moves the mean:
    statistics are stated for y, as the kernel sees it."""
    d = lambda t: None if t is None else t.double()
    y, gamma, beta, pre_bias, rm0, rv0 = d(y), d(gamma), d(beta), d(pre_bias), d(running_mean), d(running_var)
    M, C = y.shape
    r = types.SimpleNamespace(M=M, C=C, batch=batch)
    off = pre_bias if pre_bias is not None else torch.zeros_like(gamma)
    r.e_abs, r.ey2 = y.abs().mean(0), (y * y).mean(0)
    if batch:
        r.mean = y.mean(0)
        r.var = ((y - r.mean) ** 2).mean(0)                       # the biased variance; never below 0 in this form
    else:
        r.mean, r.var = rm0 - off, rv0
    r.rstd = 1.0 / torch.sqrt(r.var + eps)
    r.scale = gamma * r.rstd
    r.shift = beta - r.mean * r.scale
    xhat = (y - r.mean) * r.rstd
    r.p = xhat * gamma + beta
    r.z = r.p.clamp_min(0.0)
    r.dev_abs = (y - r.mean).abs()                                # elementwise: the bounds need it
    r.running_mean, r.running_var = rm0, rv0
    if batch and momentum is not None and rm0 is not None:
        unbiased = r.var * (M / (M - 1.0) if M > 1 else 1.0)
        r.running_mean = (1.0 - momentum) * rm0 + momentum * (r.mean + off)
        r.running_var = (1.0 - momentum) * rv0 + momentum * unbiased
        r.rm_terms = (1.0 - momentum) * rm0.abs() + momentum * (r.mean.abs() + off.abs())
        r.rv_terms = (1.0 - momentum) * rv0.abs() + momentum * unbiased
        r.momentum = momentum
    if backward:
        g = dz.double() * (r.p > 0)
        gx = g * xhat
        r.dbeta, r.dgamma = g.sum(0), gx.sum(0)
        r.sum_abs_g, r.sum_abs_gx = g.abs().sum(0), gx.abs().sum(0)
        r.mg, r.mgx = (r.dbeta / M, r.dgamma / M) if batch else (torch.zeros_like(gamma), torch.zeros_like(gamma))
        r.dy = r.scale * (g - r.mg - xhat * r.mgx)
        r.terms = g.abs() + r.mg.abs() + (xhat * r.mgx).abs()     # the magnitudes dy's bracket is rounded from
        r.xhat_abs = xhat.abs()
        r.dpre = torch.zeros_like(gamma) if batch else r.dy.sum(0)
    return r


# ---- the bounds --------------------------------------------------------------------------------------------------------------------------
def bounds(r, dtype, gamma, beta):
    """Allowed |kernel - reference| of every output of a case with reference r (float64 tensors on r's device).

    sums       a per-channel f32 sum over the rows: each addition loses at most U of the sum of the magnitudes, the longest chain is
               L = chain(M, C, dtype): e = L U, relative to sum |terms|
    batch statistics (bn_finalize_kernel, in double from the f32 sums):
      mean     e E|y|, and its f32 store: U |mean|
      var      = sumsq / M - mean^2: e E[y^2] + 2 |mean| e E|y|.  Relative to var + eps that is e kappa with
               kappa = (E[y^2] + 2 |mean| E|y|) / (var + eps), the conditioning of the formula (about 2700 for a mean at 30 sigma)
      rstd     = 1 / sqrt(var + eps) with the clamped var anywhere in max(var - d var, 0) .. var + d var (e kappa / 2 to first order; the
               interval itself is used, since one row of f32 data leaves var = fl(y^2) - y^2, which can exceed eps many times), and
               2 U for the f32 eps and the f32 store
    running statistics (bn_eval_params_kernel, f32): rstd = 1 / sqrtf(rv + eps): the sum U halved by the root, sqrtf and the division
               at most 2 U each: 5 U;  mean = rm - pre_bias: U |mean|
      scale    = gamma rstd: rstd's, + U
      p        the ReLU's argument fma(y, scale, shift), shift = beta - mean scale.  The scale's error meets y - mean, not y:
               |y - mean| |scale| rel(scale) + |scale| d mean + U |mean scale| (product) + U (|beta| + |mean scale|) (difference)
               + U |p| (fma); eval forms (mean gamma) rstd with one more product: + U |mean scale|, and y scale is not fused with it
               there: + U |y scale|
      z        p's, and half a bf16 ulp of the value where z is stored as bf16
    backward   g = dz [p > 0] is exact (the condition on the inputs).  xhat = fl(fl(y - mean) rstd): rstd d mean + |xhat| (rel(rstd)
               + 2 U)
      dbeta    e sum |g|
      dgamma   e sum |g xhat| + sum |g| d xhat  =  (e + rel(rstd) + 2 U) sum |g xhat| + rstd d mean sum |g|
      dy       = scale (g - mg - xhat mgx), mg = dbeta / M, mgx = dgamma / M (one f32 division each: U):
               |scale| (d mg + |xhat| d mgx + |mgx| d xhat + 2 U (|g| + |mg| + |xhat mgx|)) + |dy| (rel(scale) + U), and half a bf16 ulp
               where dy is bf16.  Eval: mg = mgx = 0 exactly and dy = scale g is one product.
    running    new = (1 - m) old + m stat, f32: the f32 momentum (U, both terms), 1 - m and its product (2 U), mean + bias, the
               momentum's product (2 U) or the double's f32 store and the product (2 U), the sum (U): at most 6 U = 3 ulps of
               (1 - m) |old| + m |stat|, plus m x the statistic's own error (the variance's times M / (M - 1))."""
    M, C = r.M, r.C
    e = chain(M, C, dtype) * U
    t = {}
    if r.batch:
        d_mean = e * r.e_abs + U * r.mean.abs()
        d_var = e * (r.ey2 + 2 * r.mean.abs() * r.e_abs)
        lo, hi = 1.0 / torch.sqrt(r.var + d_var + EPS32), 1.0 / torch.sqrt((r.var - d_var).clamp_min(0.0) + EPS32)
        rel_rstd = torch.maximum(r.rstd - lo, hi - r.rstd) / r.rstd + 2 * U
    else:
        d_mean = U * r.mean.abs()
        d_var = torch.zeros_like(r.var)
        rel_rstd = torch.full_like(r.var, 5 * U)
    rel_scale = rel_rstd + U
    t["save_mean"] = d_mean
    t["save_rstd"] = r.rstd * rel_rstd
    ms = (r.mean * r.scale).abs()
    d_p = r.dev_abs * r.scale.abs() * rel_scale + r.scale.abs() * d_mean + U * (beta.double().abs() + 2 * ms) + U * r.p.abs()
    if not r.batch:
        d_p = d_p + U * ms + U * (r.p - r.shift).abs()
    t["p"] = d_p
    t["z"] = d_p + (half_ulp_bf16(r.z + d_p) * (r.z + d_p > 0) if dtype == torch.bfloat16 else 0.0)
    if hasattr(r, "momentum"):
        f = M / (M - 1.0) if M > 1 else 1.0
        t["running_mean"] = 3 * ULP * r.rm_terms + r.momentum * d_mean
        t["running_var"] = 3 * ULP * r.rv_terms + r.momentum * f * d_var
    if hasattr(r, "dy"):
        d_xhat_rel = rel_rstd + 2 * U
        t["dbeta"] = e * r.sum_abs_g
        t["dgamma"] = (e + d_xhat_rel) * r.sum_abs_gx + r.rstd * d_mean * r.sum_abs_g
        if r.batch:
            d_mg = t["dbeta"] / M + U * r.mg.abs()
            d_mgx = t["dgamma"] / M + U * r.mgx.abs()
            d_xhat = r.rstd * d_mean + r.xhat_abs * d_xhat_rel
            inner = d_mg + r.xhat_abs * d_mgx + r.mgx.abs() * d_xhat + 2 * U * r.terms
            d_dy = r.scale.abs() * inner + r.dy.abs() * (rel_scale + U)
        else:
            d_dy = r.dy.abs() * (rel_scale + U)
        t["dy"] = d_dy + (half_ulp_bf16(r.dy.abs() + d_dy) * (r.dy.abs() + d_dy > 0) if dtype == torch.bfloat16 else 0.0)
    return t


def ratios(got, r, tol):
    """{output: largest |got - reference| / bound}; an element with a zero bound must be exact; NaN / inf never pass"""
    out = {}
    for k in OUTPUTS:
        if k not in got or got[k] is None or k not in tol:
            continue
        want = getattr(r, {"save_mean": "mean", "save_rstd": "rstd"}.get(k, k))
        g = got[k].double().to(want.device)
        assert g.shape == want.shape, (k, g.shape, want.shape)
        err = (g - want).abs()
        q = torch.where(err == 0, torch.zeros_like(err), err / tol[k])          # 0 / 0 -> 0, x / 0 -> inf
        out[k] = float(torch.where(torch.isfinite(g), q, torch.full_like(q, float("inf"))).max())
    return out


def exact_failures(got, case, batch):
    """The channels that are exact by construction -> list of what is not.  got holds [M, C] rows and [C] vectors."""
    bad = []
    C, beta = case.C, case.beta
    has = lambda k: k in got and got[k] is not None
    zero = lambda k, c: has(k) and not bool((got[k][..., c] == 0).all())
    if C > 3:                                       # gamma = 0: fma(y, 0, beta - mean 0) = beta, and dy = 0 (...) = 0
        want = torch.relu(beta[3]).to(got["z"].dtype)
        if not bool((got["z"][:, 3] == want.to(got["z"].device)).all()):
            bad.append("z of the gamma = 0 channel is not relu(beta)")
        if zero("dy", 3):
            bad.append("dy of the gamma = 0 channel is not 0")
        if float(beta[3]) == 0.0 and (zero("dbeta", 3) or zero("dgamma", 3)):
            bad.append("the gamma = 0, beta = 0 channel passes a gradient: the mask is not p > 0")
    if C > 4:
        for k in ("z", "dy", "dgamma", "dbeta"):
            if zero(k, 4):
                bad.append(f"{k} of the dead channel is not 0")
    if batch:                                       # constant 1.5: sum and sum of squares exact in f32, variance exactly 0
        want = 1.0 / math.sqrt(EPS32)
        if not abs(float(got["save_rstd"][0]) - want) <= 3 * ULP * want:
            bad.append(f"save_rstd of the constant channel {float(got['save_rstd'][0])} is not 1 / sqrt(eps)")
        if not float(got["save_mean"][0]) == 1.5:
            bad.append("save_mean of the constant channel is not 1.5")
        if float(beta[0]) < 0:                      # and p = beta < 0 everywhere: nothing passes the ReLU
            for k in ("z", "dy", "dgamma", "dbeta"):
                if zero(k, 0):
                    bad.append(f"{k} of the constant channel below the ReLU is not 0")
    return bad


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
SPECIAL = (0, 1, 3, 4)
MARGIN = 10.0                    # the inputs are built to 10 x the allowed error of p; the tests ask for 8


def condition(case, r, tol):
    """smallest |p| / (allowed error of p) over the elements of a case, the elements that are exactly 0 on both sides (the gamma = 0
    channel with beta = 0: fma(y, 0, 0 - mean 0) is 0 in any arithmetic) aside"""
    q = r.p.abs() / tol["p"]
    if case.C > 3 and float(case.beta[3]) == 0.0:
        assert bool((r.p[:, 3] == 0).all())
        q[:, 3] = float("inf")
    return float(q.min())


def settle(y, std, gamma, beta, pre_bias, rm, rv, dtype, batch, generic=None, device="cpu"):
    """Moves every element of the `generic` channels of y [M, C] whose |p| is below MARGIN x the allowed error of p a quarter of std
    away from 0, until none is left -> (y in float64 on `device`, elements moved, passes, the last reference)"""
    C = y.shape[1]
    generic = (torch.ones(C, dtype=torch.bool) if generic is None else generic).to(device)
    yd, stdd = y.double().to(device), std.double().to(device)
    par = [None if t is None else t.to(device) for t in (gamma, beta, pre_bias, rm, rv)]
    moved = 0
    for passes in range(60):
        r = reference(yd, None, *par, batch, None, backward=False)
        tol = bounds(r, dtype, par[0], par[1])
        frag = (r.p.abs() < MARGIN * tol["p"]) & generic
        n = int(frag.sum())
        if n == 0:
            return yd, moved, passes, r
        moved += n
        step = 0.25 * stdd * torch.sign(r.scale) * torch.where(r.p >= 0, 1.0, -1.0)
        yd = torch.where(frag, yd + step, yd)
        yd = (bf16_exact(yd.float()) if dtype == torch.bfloat16 else yd.float()).double()
    raise AssertionError("the ReLU condition did not converge")


@functools.lru_cache(maxsize=None)
def case(M, C, dtype, seed, batch=True, plant=False, device="cpu", pre=True):
    """The inputs of one case as CPU float32 tensors (bf16-exact y and dz when dtype is bf16), never written to afterwards:
    y, dz [M, C] rows; gamma, beta, pre_bias, running_mean, running_var [C].  Channels, as far as C goes:
      0  constant 1.5: sums exact in f32, variance exactly 0.  beta +0.5 (even seed) or -0.5 (odd seed: the ReLU passes nothing)
      1  constant 0.1: the f32 sums may leave a raw variance below 0 (the clamp)
      2  mean at 30 standard deviations
      3  gamma exactly 0; beta 0.375 (even seed) or 0 (odd seed: p is exactly 0, where `> 0` and `>= 0` differ)
      4  beta = -12: every p below 0, a dead channel
      every fifth: gamma negative;  the rest: |mean| of about one standard deviation, |gamma| in 0.5..1.5, |beta| in 0.1..0.4
    batch: the mode the ReLU condition is built for (batch or running statistics).  After generation every element of the other
    channels whose |p| is below MARGIN x the allowed error of p is moved a quarter of its channel's standard deviation away from 0,
    until none is left (the margin loop runs on `device`).  plant: the rows of planted_rows() carry 64 x the deviation from the mean
    in y (channels from 5 on) and 64 x dz.  pre=False: for a call without pre_bias (the running mean then tracks y alone)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * C + M % 1000 + (0 if dtype == torch.float32 else 500))
    q = bf16_exact if dtype == torch.bfloat16 else (lambda t: t)
    std = torch.rand(C, generator=g) * 1.5 + 0.5
    mean = torch.randn(C, generator=g) * std
    sign = lambda n: torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.arange(C) % 5 == 0, -1.0, 1.0)
    beta = (torch.rand(C, generator=g) * 0.3 + 0.1) * sign(C)
    pre_bias = torch.randn(C, generator=g) * 0.5 * (1.0 if pre else 0.0)
    if C > 2:
        mean[2] = 30.0 * std[2]
    y = torch.randn(M, C, generator=g) * std + mean
    dz = torch.randn(M, C, generator=g)
    rows = planted_rows(M, C, dtype) if plant else []
    if rows:
        idx = torch.tensor(rows)
        y[idx, 5:] = mean[5:] + 64.0 * (y[idx, 5:] - mean[5:])
        dz[idx] *= 64.0
    y[:, 0] = 1.5
    beta[0] = 0.5 if seed % 2 == 0 else -0.5
    if C > 1:
        y[:, 1] = 0.1
        beta[1] = 0.3
    if C > 3:
        gamma[3] = 0.0
        beta[3] = 0.375 if seed % 2 == 0 else 0.0
    if C > 4:
        beta[4] = -12.0
        y[:, 4] = (y[:, 4] - mean[4]).clamp(-4 * std[4], 4 * std[4]) + mean[4]
    y, dz = q(y), q(dz)
    # running statistics near the batch's, so that eval mode normalises the same data; the constant channels get a variance of 0.25
    bm, bv = y.double().mean(0), y.double().var(0, unbiased=False) if M > 1 else torch.zeros(C, dtype=torch.float64)
    rv = (bv * (0.8 + 0.4 * torch.rand(C, generator=g).double())).float()
    rm = (bm + pre_bias.double() + 0.1 * std.double() * torch.randn(C, generator=g).double()).float()
    if M == 1:
        rv = (std * std).float()
    rv[0], rm[0] = 0.25, 0.5 + pre_bias[0]
    if C > 1:
        rv[1], rm[1] = 0.25, -0.4 + pre_bias[1]
    c = types.SimpleNamespace(M=M, C=C, dtype=dtype, seed=seed, batch=batch, dz=dz, gamma=gamma, beta=beta, pre_bias=pre_bias,
                              running_mean=rm, running_var=rv, planted=rows, moved=0, passes=0)
    generic = torch.tensor([ch not in SPECIAL for ch in range(C)])
    yd, c.moved, c.passes, r = settle(y, std, gamma, beta, pre_bias if pre else None, rm, rv, dtype, batch, generic, device)
    c.y = yd.float().cpu()
    if C > 4:
        assert float(r.p[:, 4].max()) < -1.0            # dead in this mode
    return c


def rows4(t):
    """[M, C] rows -> the [1, C, 1, M] channels-last view the operator takes"""
    M, C = t.shape
    return t.view(1, 1, M, C).permute(0, 3, 1, 2)


def case_reference(c, batch, momentum, pre=True, device="cpu", track=True):
    """reference and bounds of a case on `device`"""
    to = lambda t: t.to(device)
    r = reference(to(c.y), to(c.dz), to(c.gamma), to(c.beta), to(c.pre_bias) if pre else None,
                  to(c.running_mean) if track else None, to(c.running_var) if track else None, batch, momentum if track else None)
    return r, bounds(r, c.dtype, to(c.gamma), to(c.beta))


# ---- a float32 mirror of the kernels' formulas ---------------------------------------------------------------------------------------------
DEFECTS = ("drop_last_row", "double_sweep_row", "mask_ge", "no_mgx", "mean_m1", "rv_biased", "rm_no_pre", "neg_gamma_mask")


def _fma(a, b, c):
    """f32 fma: the product of two f32 is exact in double"""
    return (a.double() * b.double() + c.double()).float()


def mirror(c, batch, momentum, pre=True, defect=None):
    """pswin_bn.hip's expressions in torch float32 on the CPU (double where bn_finalize_kernel uses it), the sums over rpi strided
    row lanes that are added one after the other -- not torch.sum's order over the rows, and not the kernel's.  defect: one of DEFECTS."""
    y, dz, gamma, beta = c.y, c.dz, c.gamma, c.beta
    M, C = y.shape
    off = c.pre_bias if pre else torch.zeros(C)
    lanes = rpi(C, c.dtype)
    sweep = reduce_sweep(M, C, c.dtype)

    def colsum(t):
        acc = torch.zeros(C)
        rows = t[:-1] if defect == "drop_last_row" else t
        for q in range(min(lanes, rows.shape[0])):
            acc = acc + rows[q::lanes].sum(0)
        if defect == "double_sweep_row" and sweep < M:
            acc = acc + t[sweep]
        return acc

    div = float(M - 1) if defect == "mean_m1" else float(M)
    out = {}
    rm, rv = c.running_mean.clone(), c.running_var.clone()
    if batch:
        m = colsum(y).double() / div
        var = (colsum(y * y).double() / div - m * m).clamp_min(0.0)
        rstd = (1.0 / torch.sqrt(var + EPS32)).float()
        mean = m.float()
        scale = gamma * rstd
        shift = beta - mean * scale
        if momentum is not None:
            mom = torch.tensor(momentum, dtype=torch.float32)
            tracked = mean + (torch.zeros(C) if defect == "rm_no_pre" else off)
            rm = (1.0 - mom) * rm + mom * tracked
            unb = var if (defect == "rv_biased" or M == 1) else var * M / (M - 1.0)
            rv = (1.0 - mom) * rv + mom * unb.float()
    else:
        rstd = 1.0 / torch.sqrt(rv + torch.tensor(EPS32))
        mean = rm - off
        scale = gamma * rstd
        shift = beta - mean * gamma * rstd
    p = _fma(y, scale, shift)
    store = (lambda t: t.to(torch.bfloat16)) if c.dtype == torch.bfloat16 else (lambda t: t)
    out.update(z=store(p.clamp_min(0.0)), save_mean=mean, save_rstd=rstd, running_mean=rm, running_var=rv)
    s_b = gamma * rstd                                            # bn_scale_shift_kernel
    pm = _fma(y, s_b.abs(), beta - mean * s_b.abs()) if defect == "neg_gamma_mask" else _fma(y, s_b, beta - mean * s_b)
    mask = pm >= 0 if defect == "mask_ge" else pm > 0
    gz = dz * mask
    xh = (y - mean) * rstd
    sg, sgx = colsum(gz), colsum(gz * xh)
    mg, mgx = (sg / div, sgx / div) if batch else (torch.zeros(C), torch.zeros(C))
    inner = gz - mg if defect == "no_mgx" else gz - mg - xh * mgx
    out.update(dy=store(s_b * inner), dgamma=sgx, dbeta=sg)
    return out


# ---- the cases both test files run -------------------------------------------------------------------------------------------------------
DTYPES = (torch.float32, torch.bfloat16)
WIDTHS = (8, 40, 64, 96)
WIDEST = {torch.float32: 1024, torch.bfloat16: 2048}            # C / VE == 256: one row per block step
MODE_C = 40
BIG_SEED = 1


def name(dtype):
    return "bf16" if dtype == torch.bfloat16 else "f32"


def grid():
    """(C, M, dtype, seed): every width at the row counts around its rows per block step; the seed (the index of M) alternates the
    two variants of channels 0 and 3"""
    return [(C, M, dt, i) for dt in DTYPES for C in WIDTHS + (WIDEST[dt],) for i, M in enumerate(m_values(C, dt))]


GRID = grid()


def mode_shape(dtype):
    return MODE_C, 16 * rpi(MODE_C, dtype) + 1


def case_id(v):
    C, M, dt, seed = v
    return f"C{C}-M{M}-{name(dt)}"
