"""The exact-row LayerNorm kernels (csrc/pswin_norm.hip: rows of 96, 192, 384, 768 elements, every load of a row in flight together)
through the wrappers of ops.py: (a) bit for bit against the generic kernels, forced with pswin_ln_rows_tune(1), and (b) against a
float64 reference of the same inputs on the CPU, with the tolerances tests/test_kernels_gpu.py uses for these kernels.  The widths 104
and 64 go through the same dispatch and stay on the generic kernels.  Shapes: 2 images of 9 x 11 tokens in 7 x 7 windows (99 tokens,
196 slots: pad slots, zero rows, a partial last block), 7 x 9 tokens for patch merging (quarters outside the image), 8 x 16 for the NCHW
forms, and one case per persistent backward kernel of 2.5 x (partial rows) x (rows per block) rows: some workgroups make three trips,
others two, and the last prefetch runs past the end.  Needs an MI355X."""
import pytest
import torch

from detfill import det_uniform

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
WIDTHS = [96, 192, 384, 768, 104, 64]
F32OUT = dict(rtol=1e-5, atol=2e-6)
BF16OUT = dict(rtol=1e-2, atol=1e-2)
DX_F32 = dict(rtol=1e-4, atol=1e-5)
DX_BF16 = dict(rtol=2e-2, atol=2e-2)


def _both_paths(run):
    """run() under the automatic dispatch and under the generic kernels: (fast, generic)"""
    from panoswintransformerobjectdetection_amd import _lib
    lib = _lib.load()
    res = []
    for mode in (0, 1):
        assert lib.pswin_ln_rows_tune(mode) == 0
        try:
            res.append(run())
            torch.cuda.synchronize()
        finally:
            assert lib.pswin_ln_rows_tune(0) == 0
    return res


def _check(fast, generic, ref, tols):
    """fast / generic / ref: dicts name -> tensor; tols: name -> allclose arguments, or "param" (rtol 1e-4, atol 1e-4 max |ref|)"""
    assert set(fast) == set(generic) == set(ref) == set(tols)
    for k in fast:
        assert torch.equal(fast[k], generic[k]), k
    for k, t in tols.items():
        got, want = fast[k].double().cpu(), ref[k].double()
        assert got.shape == want.shape, k
        if t == "param":
            t = dict(rtol=1e-4, atol=1e-4 * want.abs().max().item())
        assert torch.allclose(got, want, **t), (k, (got - want).abs().max().item())


def _ln64(x, gamma, beta):
    mu = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + EPS)
    return (x - mu) * rstd * gamma + beta, mu.squeeze(-1), rstd.squeeze(-1)


def _gather64(rows, wmap):
    """rows [B, S, C] through a slot -> token map (-1: zero row)"""
    idx = wmap.cpu().long()
    return rows[:, idx.clamp(min=0)] * (idx >= 0).double()[None, :, None]


def _leaf(t):
    return t.to(DEV).requires_grad_(True)


def _leaf64(t):
    return t.double().requires_grad_(True)


def _stats(y):
    return [t.detach() for t in y.grad_fn.saved_tensors[2:4]]


# ------------------------------------------------------------------------------------------------------------------------------
# layer_norm_gather: ln_fwd_kernel (MODE 0) and ln_bwd_kernel
# ------------------------------------------------------------------------------------------------------------------------------
def _gather_case(ops, C, B, S, wmap, inv, xdt, ydt, passthrough, res, add):
    tag = f"nr:g:{C}:{S}"
    x = (det_uniform((B, S, C), tag + "x", 2.0) + 0.3).to(xdt)
    gamma, beta = det_uniform((C,), tag + "g", 0.5, 1.0), det_uniform((C,), tag + "b", 0.5)
    rbias = det_uniform((C,), tag + "rb", 0.5) if res else None
    rscale = torch.tensor([1.25, 0.5][:B]) if res else None
    rows = det_uniform((S, C), tag + "r", 1.5) if add else None
    n_out = S if wmap is None else wmap.numel()
    gy = det_uniform((B, n_out, C), tag + "gy").to(ydt)
    gx = det_uniform((B, S, C), tag + "gx")

    def run():
        xd, gd, bd = _leaf(x), _leaf(gamma), _leaf(beta)
        rb = _leaf(rbias) if res else None
        rd = _leaf(rows) if add else None
        out = ops.layer_norm_gather(xd, gd, bd, EPS, wmap, inv, ydt, passthrough=passthrough, res_bias=rb,
                                    res_scale=None if rscale is None else rscale.to(DEV), add_rows=rd)
        y, x2 = out if passthrough else (out, None)
        mean, rstd = _stats(y)
        loss = (y.float() * gy.to(DEV).float()).sum()
        if passthrough:
            loss = loss + (x2 * gx.to(DEV)).sum()
        loss.backward()
        r = dict(y=y.detach(), mean=mean, rstd=rstd, dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad)
        if res:
            r["dres_sum"] = rb.grad
        return r

    fast, generic = _both_paths(run)
    xr, gr, br = _leaf64(x), _leaf64(gamma), _leaf64(beta)
    yr, mu, rstd = _ln64(xr, gr, br)
    if add:
        yr = yr + rows.double()
    if wmap is not None:
        yr = _gather64(yr, wmap)
    loss = (yr * gy.double()).sum() + ((xr * gx.double()).sum() if passthrough else 0.0)
    loss.backward()
    ref = dict(y=yr.detach(), mean=mu.detach(), rstd=rstd.detach(), dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)
    tols = dict(y=F32OUT if ydt == torch.float32 else BF16OUT, mean=F32OUT, rstd=F32OUT,
                dx=DX_F32 if xdt == torch.float32 else DX_BF16, dgamma="param", dbeta="param")
    if res:        # the bias of the branch x' + scale_b * (f(y) + bias): sum over the rows of scale_b * grad(x')
        ref["dres_sum"] = (gx.double() * rscale.double()[:, None, None]).sum((0, 1))
        tols["dres_sum"] = "param"
    _check(fast, generic, ref, tols)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("variant", ["map_shift", "map_noshift_shortcut", "plain_add", "plain_bf16"])
def test_layer_norm_gather_rows(ops, C, variant):
    B, H, W = 2, 9, 11
    wmap = inv = None
    if variant.startswith("map"):
        wmap, inv, nW = ops.window_maps(False, H, W, 3 if variant == "map_shift" else 0, DEV)
        assert nW * 49 == 196
    if variant == "map_shift":
        _gather_case(ops, C, B, H * W, wmap, inv, torch.float32, torch.float32, False, False, False)
    elif variant == "map_noshift_shortcut":     # shortcut gradient, its bias sums and scales: dres, RSUM, res_scale present
        _gather_case(ops, C, B, H * W, wmap, inv, torch.float32, torch.bfloat16, True, True, False)
    elif variant == "plain_add":
        _gather_case(ops, C, B, H * W, None, None, torch.float32, torch.float32, False, False, True)
    else:                                       # bf16 rows in: the forward kernel is the exact-row one, the backward the generic
        _gather_case(ops, C, B, H * W, None, None, torch.bfloat16, torch.float32, False, False, False)


# ------------------------------------------------------------------------------------------------------------------------------
# window_scatter_add + LayerNorm: ln_add_fwd_kernel; its backward is ln_bwd_kernel with the extra bf16 output
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("variant", ["windows_shift", "windows_noshift_bare", "join_out_map"])
def test_scatter_add_layer_norm_rows(ops, C, variant):
    B, H, W = 2, 9, 11
    S = H * W
    shift = 0 if variant == "windows_noshift_bare" else 3
    wmap, inv, nW = ops.window_maps(False, H, W, shift, DEV)
    pads = ops.window_pads(False, H, W, shift, DEV)
    n_slots = nW * 49
    bare = variant == "windows_noshift_bare"                    # no scale, no bias, no shortcut bias sums
    join = variant == "join_out_map"                            # token-order input, output through the map (with its zero rows)
    tag = f"nr:s:{C}:{variant}"
    win = det_uniform((B, S if join else n_slots, C), tag + "w", 2.0).to(torch.bfloat16)
    x = det_uniform((B, S, C), tag + "x", 2.0)
    gamma, beta = det_uniform((C,), tag + "g", 0.5, 1.0), det_uniform((C,), tag + "b", 0.5)
    pbias, fbias = det_uniform((C,), tag + "pb", 0.5), det_uniform((C,), tag + "fb", 0.5)
    s1 = None if bare else torch.tensor([0.75, 1.25])
    s2 = None if bare else torch.tensor([1.25, 0.5])
    gy = det_uniform((B, n_slots if join else S, C), tag + "gy").to(torch.bfloat16)
    gx = det_uniform((B, S, C), tag + "gx")
    ident = ops.identity_map(S, DEV)

    def run():
        wd, xd, gd, bd = _leaf(win), _leaf(x), _leaf(gamma), _leaf(beta)
        fb = None if bare else _leaf(fbias)
        kw = dict(res_bias=fb, res_scale=None if bare else s2.to(DEV))
        sc = None if bare else s1.to(DEV)
        pb = None if bare else pbias.to(DEV)
        if join:
            y, x1 = ops.scatter_add_layer_norm(wd, xd, ident, None, sc, pb, gd, bd, EPS, torch.bfloat16, out=(inv, n_slots, pads), **kw)
        else:
            y, x1 = ops.scatter_add_layer_norm(wd, xd, wmap, inv, sc, pb, gd, bd, EPS, torch.bfloat16, in_pads=pads, **kw)
        mean, rstd = _stats(y)
        ((y.float() * gy.to(DEV).float()).sum() + (x1 * gx.to(DEV)).sum()).backward()
        r = dict(y=y.detach(), x1=x1.detach(), mean=mean, rstd=rstd, dwin=wd.grad, dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad)
        if not bare:
            r["dres_sum"] = fb.grad
        return r

    fast, generic = _both_paths(run)
    wr, xr, gr, br = _leaf64(win.float()), _leaf64(x), _leaf64(gamma), _leaf64(beta)
    branch = wr if join else wr[:, inv.cpu().long()]
    if not bare:
        branch = (branch + pbias.double()) * s1.double()[:, None, None]
    x1r = xr + branch
    yr, mu, rstd = _ln64(x1r, gr, br)
    if join:
        yr = _gather64(yr, wmap)
    ((yr * gy.double()).sum() + (x1r * gx.double()).sum()).backward()
    ref = dict(y=yr.detach(), x1=x1r.detach(), mean=mu.detach(), rstd=rstd.detach(), dwin=wr.grad, dx=xr.grad, dgamma=gr.grad,
               dbeta=br.grad)
    tols = dict(y=BF16OUT, x1=F32OUT, mean=F32OUT, rstd=F32OUT, dwin=DX_BF16, dx=DX_F32, dgamma="param", dbeta="param")
    if not bare:
        ref["dres_sum"] = (gx.double() * s2.double()[:, None, None]).sum((0, 1))
        tols["dres_sum"] = "param"
    _check(fast, generic, ref, tols)
    if join:
        assert bool((fast["y"][:, pads.long()] == 0).all())
    else:
        assert bool((fast["dwin"][:, pads.long()] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------
# layer_norm_patch_merge: ln_fwd_kernel (MODE 1); merged widths 4 C_in, so 192, 384, 768 exact and 64 generic (96 and 104 are no
# multiple of 64 elements and cannot occur), 7 x 9 tokens: the last row and column of quarters lie outside the image
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C4", [192, 384, 768, 64])
@pytest.mark.parametrize("ydt", [torch.float32, torch.bfloat16])
def test_layer_norm_patch_merge_rows(ops, C4, ydt):
    B, H, W, C = 2, 7, 9, C4 // 4
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    tag = f"nr:pm:{C4}"
    x = det_uniform((B, H * W, C), tag + "x", 2.0) + 0.1
    gamma, beta = det_uniform((C4,), tag + "g", 0.5, 1.0), det_uniform((C4,), tag + "b", 0.5)
    gy = det_uniform((B, H2 * W2, C4), tag + "gy").to(ydt)

    def run():
        xd, gd, bd = _leaf(x), _leaf(gamma), _leaf(beta)
        y = ops.layer_norm_patch_merge(xd, gd, bd, EPS, H, W, ydt)
        mean, rstd = _stats(y)
        (y.float() * gy.to(DEV).float()).sum().backward()
        return dict(y=y.detach(), mean=mean, rstd=rstd, dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad)

    fast, generic = _both_paths(run)
    xr, gr, br = _leaf64(x), _leaf64(gamma), _leaf64(beta)
    img = torch.nn.functional.pad(xr.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
    cat = torch.cat([img[:, 0::2, 0::2], img[:, 1::2, 0::2], img[:, 0::2, 1::2], img[:, 1::2, 1::2]], -1).reshape(B, H2 * W2, C4)
    yr, mu, rstd = _ln64(cat, gr, br)
    (yr * gy.double()).sum().backward()
    ref = dict(y=yr.detach(), mean=mu.detach(), rstd=rstd.detach(), dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)
    tols = dict(y=F32OUT if ydt == torch.float32 else BF16OUT, mean=F32OUT, rstd=F32OUT, dx=DX_F32, dgamma="param", dbeta="param")
    _check(fast, generic, ref, tols)


# ------------------------------------------------------------------------------------------------------------------------------
# NCHW output norms: ln_nchw_fwd_kernel / ln_nchw_bwd_kernel, plain and with the fused closing residual add of a stage
# ------------------------------------------------------------------------------------------------------------------------------
def _nchw_case(ops, C, B, H, W, fused_add, passthrough):
    S = H * W
    tag = f"nr:n:{C}:{S}"
    x = det_uniform((B, S, C), tag + "x", 2.0) + 0.2
    gamma, beta = det_uniform((C,), tag + "g", 0.5, 1.0), det_uniform((C,), tag + "b", 0.5)
    ymlp = det_uniform((B, S, C), tag + "m", 2.0).to(torch.bfloat16)
    bias = det_uniform((C,), tag + "fb", 0.5)
    scale = torch.tensor([1.25, 0.5][:B])
    gy, gx = det_uniform((B, C, H, W), tag + "gy"), det_uniform((B, S, C), tag + "gx")
    assert ops._lib.load().pswin_ln_nchw_supported(S, C)

    def run():
        xd, gd, bd = _leaf(x), _leaf(gamma), _leaf(beta)
        r = {}
        if fused_add:
            md = _leaf(ymlp)
            assert ops.scatter_add_layer_norm_nchw_supported(md, xd)
            y, x2 = ops.scatter_add_layer_norm_nchw(md, xd, scale.to(DEV), bias.to(DEV), gd, bd, EPS, H, W)
            r["x1"] = x2.detach()
        else:
            out = ops.layer_norm_nchw(xd, gd, bd, EPS, H, W, passthrough=passthrough)
            y, x2 = out if passthrough else (out, None)
        mean, rstd = _stats(y)
        loss = (y * gy.to(DEV)).sum()
        if x2 is not None:
            loss = loss + (x2 * gx.to(DEV)).sum()
        loss.backward()
        r.update(y=y.detach(), mean=mean, rstd=rstd, dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad)
        if fused_add:
            r["dbranch"] = md.grad
        return r

    fast, generic = _both_paths(run)
    xr, gr, br = _leaf64(x), _leaf64(gamma), _leaf64(beta)
    tols = dict(y=F32OUT, mean=F32OUT, rstd=F32OUT, dx=DX_F32, dgamma="param", dbeta="param")
    if fused_add:
        mr = _leaf64(ymlp.float())
        x1r = xr + (mr + bias.double()) * scale.double()[:, None, None]
    else:
        x1r = xr
    yr, mu, rstd = _ln64(x1r, gr, br)
    yr = yr.view(B, H, W, C).permute(0, 3, 1, 2)
    loss = (yr * gy.double()).sum() + ((x1r * gx.double()).sum() if (fused_add or passthrough) else 0.0)
    loss.backward()
    ref = dict(y=yr.detach(), mean=mu.detach(), rstd=rstd.detach(), dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)
    if fused_add:
        ref.update(x1=x1r.detach(), dbranch=mr.grad)
        tols.update(x1=F32OUT, dbranch=DX_BF16)
    _check(fast, generic, ref, tols)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("variant", ["plain", "shortcut", "closing_add"])
def test_layer_norm_nchw_rows(ops, C, variant):
    _nchw_case(ops, C, 2, 8, 16, variant == "closing_add", variant == "shortcut")


# ------------------------------------------------------------------------------------------------------------------------------
# the persistent backward kernels beyond two sweeps of their grids
# ------------------------------------------------------------------------------------------------------------------------------
def _trip_rows(ops, C, rpb):
    lib = ops._lib.load()
    blocks = lib.pswin_ln_partial_rows(1 << 24, C)                 # the resident grid
    rows = blocks * rpb * 5 // 2
    assert lib.pswin_ln_partial_rows(rows, C) == blocks
    return rows


@pytest.mark.parametrize("C,rpb", [(96, 32), (768, 4)])
def test_layer_norm_gather_backward_makes_a_third_trip(ops, C, rpb):
    rows = _trip_rows(ops, C, rpb)
    assert rows % 2 == 0
    _gather_case(ops, C, 2, rows // 2, None, None, torch.float32, torch.bfloat16, True, True, False)


def test_layer_norm_nchw_backward_makes_a_third_trip(ops):
    rows = _trip_rows(ops, 768, 4)
    assert rows == 2 * 64 * 80
    _nchw_case(ops, 768, 2, 64, 80, True, False)
