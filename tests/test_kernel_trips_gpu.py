"""The persistent-grid kernels where a workgroup (or wave) makes a second and a third trip over its rows, tiles or windows: the
accumulators carried across trips, the double-buffer parity, the prefetch of the next trip's operands and the image index that changes
between the trips of one workgroup.  Every shape of tests/test_kernels_gpu.py fits into one sweep of these grids.  References are float64
restatements in plain torch on the device; every test asserts first that its shape really is beyond one sweep.  Needs an MI355X.

The measured worst error of every comparison as a fraction of its bound, the number of trips and the wall time of each case go to
the parity report (_util.record) under "trips:<case>"; they never affect a verdict."""
import math
import time

import pytest
import torch
import torch.nn.functional as F

import panoswin_oracle as po
from _util import record
from test_kernels_gpu import FUSED_CASES, _fused_moves_case
from test_lr_schedule import mmcv_lr
from test_optim_schedule_gpu import CFG, IPE, KW, _flat, _grads, _ref_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# One sweep of each capped grid, with the line of panoswintransformerobjectdetection_amd/csrc that sets it.  The LayerNorm and fc1_gelu
# grids are also reported by the library (pswin_ln_workspace, pswin_fc1_gelu_partial_rows) and asserted through it; the other three are
# reported by no entry point, so this table is the record of them.
LN_MAX_BLOCKS = 1024             # pswin_norm.hip:591 BWD_MAX_BLOCKS; bwd_blocks() :593; a block walks THREADS / L rows per trip
LN_THREADS = 256                 # pswin_norm.hip THREADS
SKINNY_MAX_GRID = 512            # pswin_gemm.hip:197 MAX_GRID, applied in launch() :207-208
SKINNY_WAVES = 4                 # pswin_gemm.hip:91 one 16 * RT-row tile per wave and trip (THREADS / 64 waves)
SKINNY_RT = {(96, 288): 2, (96, 96): 2, (96, 384): 1, (288, 96): 2, (384, 96): 2, (192, 192): 2}     # pswin_gemm.hip:521-526 (K, N) -> RT
FUSED_MAX_GRID = 256             # pswin_fused.hip:403 grid = min(nb, 256) bias windows, the trip loop :180
ADAMW_MAX_BLOCKS = 4096          # pswin_optim.hip:91 and :344 (256 * 16 blocks)
ADAMW_THREADS = 256              # pswin_optim.hip:99 / :352, one float4 granule per thread and trip
ADAMW_N = 4 * (2 * ADAMW_MAX_BLOCKS * ADAMW_THREADS + 777)

PANO_H, PANO_W, PANO_SHIFT = 45, 90, 3          # S = 4050: a multiple of no rows-per-block; the shift-3 pano map has padding slots


def _lib():
    from panoswintransformerobjectdetection_amd import _lib as L
    return L.load()


def _lanes(C):
    """lanes per row of the LayerNorm kernels: the smallest power of two in 2..64 with 16 L >= C"""
    L = 2
    while 16 * L < C and L < 64:
        L *= 2
    return L


def _ln_trips(rows, C):
    """asserts that `rows` rows of width C take the capped LayerNorm backward grid beyond two full trips -> the number of trips"""
    sweep = LN_MAX_BLOCKS * (LN_THREADS // _lanes(C))
    assert _lib().pswin_ln_workspace(rows, C) // (3 * C) == LN_MAX_BLOCKS
    assert rows > 2 * sweep
    return -(-rows // sweep)


def _uniform(shape, gen, scale=1.0, offset=0.0):
    return (torch.rand(shape, generator=gen, device=DEV) * 2.0 - 1.0) * scale + offset


class _Case:
    """Collects |got - ref| / (atol + rtol |ref|) (torch.allclose's form; NaN counts as a miss) of every comparison of a case, records
    them with the trips and the wall time, and fails at the end if any of them missed."""

    def __init__(self, name, trips):
        self.name, self.trips, self.t0, self.worst, self.bad = name, trips, time.perf_counter(), {}, []

    def ratio(self, key, value):
        self.worst[key] = max(self.worst.get(key, 0.0), value) if value == value else float("nan")
        if not value <= 1.0:
            self.bad.append(f"{key}: error / bound = {value:.4g}")

    def close(self, key, got, ref, rtol, atol):
        assert got.shape == ref.shape, (key, got.shape, ref.shape)
        got, ref = got.detach().to(DEV).double(), ref.detach().to(DEV).double()
        r = (got - ref).abs() / (atol + rtol * ref.abs())
        self.ratio(key, float(torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max()))

    def equal(self, key, a, b):
        if not torch.equal(a, b):
            self.bad.append(f"{key}: not bit-equal")

    def done(self):
        torch.cuda.synchronize()
        secs = time.perf_counter() - self.t0
        print(f"trips:{self.name} trips={self.trips} seconds={secs:.2f} " + " ".join(f"{k}={v:.3g}" for k, v in self.worst.items()))
        record("trips:" + self.name, trips=self.trips, seconds=secs, **self.worst)
        assert not self.bad, "\n".join(self.bad)


def _grad_bound(ref):
    """the project's form for a parameter gradient: rtol 1e-4, atol 1e-4 max|ref|"""
    return dict(rtol=1e-4, atol=1e-4 * ref.abs().max().item())


# ---- 1. LayerNorm backward over token rows (ln_bwd_kernel MODE 0) ------------------------------------------------------------------------
LN_PLAIN = [(96, 17, torch.float32, torch.bfloat16, True), (192, 9, torch.float32, torch.bfloat16, True),
            (384, 5, torch.float32, torch.bfloat16, True), (768, 3, torch.float32, torch.bfloat16, True),
            (768, 3, torch.bfloat16, torch.float32, True),
            (96, 17, torch.float32, torch.float32, False), (768, 3, torch.float32, torch.float32, False)]


def _ln_inputs(C, B, xdt, seed):
    gen = torch.Generator(DEV).manual_seed(seed)
    S = PANO_H * PANO_W
    x = _uniform((B, S, C), gen, 2.0, 0.3).to(xdt)
    gamma, beta = _uniform((C,), gen, 0.5, 1.0), _uniform((C,), gen, 0.5)
    return gen, S, x, gamma, beta


@pytest.mark.parametrize("C,B,xdt,ydt,use_map", LN_PLAIN)
def test_layer_norm_gather_beyond_one_sweep(ops, C, B, xdt, ydt, use_map):
    """ops.layer_norm_gather as in test_layer_norm_gather, against float64 F.layer_norm + po.gather_windows, at B x 45 x 90 tokens: two full
    trips of the 1024-block backward grid and a ragged third; image boundaries fall inside blocks and between the trips of a block."""
    gen, S, x, gamma, beta = _ln_inputs(C, B, xdt, 100 + C + B)
    case = _Case(f"ln_gather:C{C}:B{B}:{xdt}:{ydt}:map{int(use_map)}".replace("torch.", ""), _ln_trips(B * S, C))
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = F.layer_norm(xr, (C,), gr, br, 1e-5)
    wmap = inv = None
    if use_map:
        omap = po.pano_window_map(PANO_H, PANO_W, PANO_SHIFT)[0]
        assert int((omap < 0).sum()) > 0                                 # padding slots
        ref = po.gather_windows(ref, omap)
        wmap, inv, nW = ops.window_maps(True, PANO_H, PANO_W, PANO_SHIFT, DEV)
    xd = x.clone().requires_grad_(True)
    gd, bd = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    out = ops.layer_norm_gather(xd, gd, bd, 1e-5, wmap, inv, ydt)
    assert out.dtype == ydt and out.shape == ref.shape
    gout = _uniform(tuple(ref.shape), gen).to(ydt)
    (ref * gout.double()).sum().backward()
    out.backward(gout)
    case.close("out", out, ref, **(dict(rtol=1e-5, atol=2e-6) if ydt == torch.float32 else dict(rtol=1e-2, atol=1e-2)))
    case.close("dx", xd.grad, xr.grad, **(dict(rtol=1e-4, atol=1e-5) if xdt == torch.float32 else dict(rtol=2e-2, atol=2e-2)))
    case.close("dgamma", gd.grad, gr.grad, **_grad_bound(gr.grad))
    case.close("dbeta", bd.grad, br.grad, **_grad_bound(br.grad))
    case.done()


@pytest.mark.parametrize("C,B", [(96, 17), (768, 3)])
def test_layer_norm_gather_passthrough_sums_beyond_one_sweep(ops, C, B):
    """passthrough=True with res_bias and res_scale (the RSUM segment of ln_bwd_kernel and the shortcut gradient folded into dx) against
    float64: loss = <LN(x), gy> + <x, gx>, d res_bias = sum_b res_scale[b] sum_t gx[b, t, :].  Every image has a scale of its own and
    one of them is 0, so the sum taken with the image index of another trip is a different number."""
    gen, S, x, gamma, beta = _ln_inputs(C, B, torch.float32, 200 + C + B)
    case = _Case(f"ln_passthrough:C{C}:B{B}", _ln_trips(B * S, C))
    scale = torch.tensor([0.0 if b == B - 2 else 0.5 + 0.25 * b for b in range(B)], device=DEV)
    assert len(set(scale.tolist())) == B and 0.0 in scale.tolist()
    omap = po.pano_window_map(PANO_H, PANO_W, PANO_SHIFT)[0]
    wmap, inv, nW = ops.window_maps(True, PANO_H, PANO_W, PANO_SHIFT, DEV)
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = po.gather_windows(F.layer_norm(xr, (C,), gr, br, 1e-5), omap)
    gy, gx = _uniform(tuple(ref.shape), gen), _uniform((B, S, C), gen)
    ((ref * gy.double()).sum() + (xr * gx.double()).sum()).backward()
    ref_dbias = (scale.double()[:, None, None] * gx.double()).sum((0, 1))
    xd = x.clone().requires_grad_(True)
    gd, bd = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    biasd = torch.zeros(C, device=DEV, requires_grad=True)
    y, x2 = ops.layer_norm_gather(xd, gd, bd, 1e-5, wmap, inv, torch.float32, passthrough=True, res_bias=biasd, res_scale=scale)
    assert x2.data_ptr() == xd.data_ptr()
    ((y * gy).sum() + (x2 * gx).sum()).backward()
    case.close("out", y, ref, rtol=1e-5, atol=2e-6)
    case.close("dx", xd.grad, xr.grad, rtol=1e-4, atol=1e-5)
    case.close("dgamma", gd.grad, gr.grad, **_grad_bound(gr.grad))
    case.close("dbeta", bd.grad, br.grad, **_grad_bound(br.grad))
    case.close("dres_bias", biasd.grad, ref_dbias, **_grad_bound(ref_dbias))
    case.done()


# ---- 2. the EX forms: the backward kernel also writes the gathered branch gradient and the zero rows of the padding slots -------------------
@pytest.mark.parametrize("C,B", [(96, 17), (384, 5)])
def test_fused_moves_of_the_layer_norm_kernels_beyond_one_sweep(ops, C, B):
    """scatter_add_layer_norm(in_pads=...) and scatter_add_layer_norm(out=...) against the chain of separate kernels, bit for bit (the body
    of test_fused_moves_of_the_layer_norm_kernels_equal_the_separate_row_movers), where the EX stores and the loop over the padding
    slots run on later trips; test_layer_norm_gather_beyond_one_sweep holds the chain's backward kernel to float64 at these shapes."""
    S = PANO_H * PANO_W
    trips = _ln_trips(B * S, C)
    t0 = time.perf_counter()
    _fused_moves_case(ops, C, True, PANO_H, PANO_W, PANO_SHIFT, True, B)
    torch.cuda.synchronize()
    record(f"trips:ln_fused_moves:C{C}:B{B}", trips=trips, seconds=time.perf_counter() - t0, bit_equal=1)


# ---- 3. PatchMerging backward (ln_bwd_kernel MODE 1) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C,B", [(45, 90, 96, 17), (45, 90, 384, 9)])
@pytest.mark.parametrize("ydt", [torch.float32, torch.bfloat16])
def test_layer_norm_patch_merge_beyond_one_sweep(ops, H, W, C, B, ydt):
    """ops.layer_norm_patch_merge against float64, test_layer_norm_patch_merge's bounds: 17595 merged rows of width 384 (sweep 8192) and
    9315 rows of width 1536 (the wide-row instantiation <.., 64, 8>, sweep 4096); the odd H leaves zero quarters in the last merged
    row of every image."""
    rows = B * ((H + 1) // 2) * ((W + 1) // 2)
    case = _Case(f"ln_patch_merge:C{C}:B{B}:{ydt}".replace("torch.", ""), _ln_trips(rows, 4 * C))
    gen = torch.Generator(DEV).manual_seed(300 + C + B)
    x = _uniform((B, H * W, C), gen, 2.0, 0.1)
    gamma, beta = _uniform((4 * C,), gen, 0.5, 1.0), _uniform((4 * C,), gen, 0.5)
    pm = po.patch_merge_map(H, W).to(DEV)
    assert int((pm < 0).sum()) > 0
    xr, gr, br = [t.double().requires_grad_(True) for t in (x, gamma, beta)]
    gat = (xr[:, pm.clamp(min=0).reshape(-1), :] * (pm.reshape(-1) >= 0).double()[None, :, None]).reshape(B, -1, 4 * C)
    ref = F.layer_norm(gat, (4 * C,), gr, br, 1e-5)
    assert ref.shape[0] * ref.shape[1] == rows
    xd, gd, bd = [t.clone().requires_grad_(True) for t in (x, gamma, beta)]
    out = ops.layer_norm_patch_merge(xd, gd, bd, 1e-5, H, W, ydt)
    gout = _uniform(tuple(ref.shape), gen).to(ydt)
    (ref * gout.double()).sum().backward()
    out.backward(gout)
    case.close("out", out, ref, **(dict(rtol=1e-5, atol=2e-6) if ydt == torch.float32 else dict(rtol=1e-2, atol=1e-2)))
    case.close("dx", xd.grad, xr.grad, rtol=1e-4, atol=1e-5)
    case.close("dgamma", gd.grad, gr.grad, **_grad_bound(gr.grad))
    case.close("dbeta", bd.grad, br.grad, **_grad_bound(br.grad))
    case.done()


# ---- 4. the NCHW output norms (ln_nchw_bwd_kernel: the LDS tile reused across trips) --------------------------------------------------------
NCHW_SHAPES = [(48, 96, 768, 2), (48, 96, 96, 15)]          # S = 4608: a multiple of every rows-per-block (pswin_ln_nchw_supported)


@pytest.mark.parametrize("H,W,C,B", NCHW_SHAPES)
@pytest.mark.parametrize("passthrough", [False, True])
def test_layer_norm_nchw_beyond_one_sweep(ops, H, W, C, B, passthrough):
    """ops.layer_norm_nchw against float64 F.layer_norm + permute with test_layer_norm_nchw's bounds."""
    S = H * W
    case = _Case(f"ln_nchw:C{C}:B{B}:pass{int(passthrough)}", _ln_trips(B * S, C))
    assert _lib().pswin_ln_nchw_supported(S, C)
    gen = torch.Generator(DEV).manual_seed(400 + C + B)
    x = _uniform((B, S, C), gen, 2.0, 0.2)
    gamma, beta = _uniform((C,), gen, 0.5, 1.0), _uniform((C,), gen, 0.5)
    gy, gx = _uniform((B, C, H, W), gen), _uniform((B, S, C), gen)
    xr, gr, br = [t.double().requires_grad_(True) for t in (x, gamma, beta)]
    ref = F.layer_norm(xr, (C,), gr, br, 1e-5).view(B, H, W, C).permute(0, 3, 1, 2)
    ((ref * gy.double()).sum() + ((xr * gx.double()).sum() if passthrough else 0.0)).backward()
    xd, gd, bd = [t.clone().requires_grad_(True) for t in (x, gamma, beta)]
    out = ops.layer_norm_nchw(xd, gd, bd, 1e-5, H, W, passthrough=passthrough)
    y, x2 = out if passthrough else (out, None)
    assert y.shape == (B, C, H, W) and y.is_contiguous()
    ((y * gy).sum() + ((x2 * gx).sum() if passthrough else 0.0)).backward()
    case.close("out", y, ref, rtol=1e-5, atol=2e-6)
    case.close("dx", xd.grad, xr.grad, rtol=1e-4, atol=1e-5)
    case.close("dgamma", gd.grad, gr.grad, **_grad_bound(gr.grad))
    case.close("dbeta", bd.grad, br.grad, **_grad_bound(br.grad))
    case.done()


@pytest.mark.parametrize("H,W,C,B", NCHW_SHAPES)
def test_stage_end_residual_add_with_the_output_norm_beyond_one_sweep(ops, H, W, C, B):
    """ops.scatter_add_layer_norm_nchw against window_scatter_add followed by layer_norm_nchw, bit for bit, as in
    test_stage_end_residual_add_with_the_output_norm_equals_the_two_separate_ops, with a different scale for every image (one 0): the
    backward kernel's bf16(scale_b dx) store takes b from the trip's first row."""
    S = H * W
    trips = _ln_trips(B * S, C)
    case = _Case(f"ln_nchw_stage_end:C{C}:B{B}", trips)
    gen = torch.Generator(DEV).manual_seed(500 + C + B)
    y = torch.randn(B, S, C, device=DEV, generator=gen).to(torch.bfloat16)
    resid = torch.randn(B, S, C, device=DEV, generator=gen)
    scale = torch.tensor([0.0 if b == B - 1 else 1.25 - 0.0625 * b for b in range(B)], device=DEV)
    assert len(set(scale.tolist())) == B
    bias = torch.randn(C, device=DEV, generator=gen)
    gamma, beta = torch.rand(C, device=DEV, generator=gen) + 0.5, torch.randn(C, device=DEV, generator=gen)
    g_out, g_x = torch.randn(B, C, H, W, device=DEV, generator=gen), torch.randn(B, S, C, device=DEV, generator=gen)
    assert ops.scatter_add_layer_norm_nchw_supported(y, resid)
    ident = ops.identity_map(S, DEV)
    res = []
    for fused in (False, True):
        yd, rd = y.clone().requires_grad_(True), resid.clone().requires_grad_(True)
        gd, bd = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        if fused:
            out, x = ops.scatter_add_layer_norm_nchw(yd, rd, scale, bias, gd, bd, 1e-5, H, W)
        else:
            x0 = ops.window_scatter_add(yd, rd, ident, ident, scale, bias, True)
            out, x = ops.layer_norm_nchw(x0, gd, bd, 1e-5, H, W, passthrough=True)
        ((out * g_out).sum() + (x * g_x).sum()).backward()
        res.append((out.detach(), x.detach(), yd.grad, rd.grad, gd.grad, bd.grad))
    for name, a, b in zip(("out", "x", "dy", "dresid", "dgamma", "dbeta"), res[0], res[1]):
        case.equal(name, a, b)
    case.done()


# ---- 5. the streaming GEMM ------------------------------------------------------------------------------------------------------------
def _skinny_sweep(K, N):
    """rows the capped grid of skinny_gemm_kernel<K / 32, N / 16, RT> covers in one trip"""
    return SKINNY_MAX_GRID * SKINNY_WAVES * 16 * SKINNY_RT[(K, N)]


def _skinny_trips(M, K, N):
    ntiles = -(-M // (16 * SKINNY_RT[(K, N)]))
    assert (ntiles + SKINNY_WAVES - 1) // SKINNY_WAVES > SKINNY_MAX_GRID             # launch() caps the grid
    assert M > _skinny_sweep(K, N)
    return -(-ntiles // (SKINNY_MAX_GRID * SKINNY_WAVES))


@pytest.mark.parametrize("K,N", sorted(SKINNY_RT))
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("m_kind", ["sweep+1", "2sweep+5003"])
def test_skinny_gemm_beyond_one_sweep(ops, K, N, transposed, m_kind):
    """Every instantiation of skinny_gemm_kernel EPI 0 ((K, N): contraction and output width of the kernel) through ops.skinny_gemm, with
    the weight as nn.Linear holds it (y = x W^T + b) and as its transpose (y = x W, the data-gradient form), at M = sweep + 1 (exactly
    one wave takes a second tile, with one valid row) and M = 2 sweep + 5003, against the float64 product of the same bf16 operands.
    Bound: one bf16 rounding of the result is at most 2^-8 relative and the f32 accumulation over K <= 384 terms stays far below
    1e-5 sum|x||w|, so |y - ref| <= 2^-7 |ref| + 1e-5 (|x| @ |w|^T + |b|) elementwise, twice the rounding."""
    sweep = _skinny_sweep(K, N)
    assert sweep == (32768 if (K, N) == (96, 384) else 65536)
    M = sweep + 1 if m_kind == "sweep+1" else 2 * sweep + 5003
    case = _Case(f"skinny_gemm:K{K}:N{N}:t{int(transposed)}:M{M}", _skinny_trips(M, K, N))
    assert _lib().pswin_gemm_skinny_supported(K, N)
    g = torch.Generator(DEV).manual_seed(600 + K + N)
    x = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.1).to(torch.bfloat16)
    b = None if transposed else torch.randn(N, generator=g, device=DEV)
    assert ops.skinny_gemm_supported(x, N)
    if transposed:
        y = ops.skinny_gemm(x, w.t().contiguous(), None, transpose_w=True)
    else:
        y = ops.skinny_gemm(x, w, b)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    ref = x.double() @ w.double().t()
    mag = x.double().abs() @ w.double().abs().t()
    if b is not None:
        ref, mag = ref + b.double(), mag + b.double().abs()
    case.ratio("y", float(((y.double() - ref).abs() / (2.0 ** -7 * ref.abs() + 1e-5 * mag)).nan_to_num(nan=float("inf")).max()))
    tail = (y[sweep:].double() - ref[sweep:]).abs() / (2.0 ** -7 * ref[sweep:].abs() + 1e-5 * mag[sweep:])
    case.ratio("y_after_first_sweep", float(tail.nan_to_num(nan=float("inf")).max()))
    case.done()


@pytest.mark.parametrize("M", [32769, 70539])
def test_fc1_gelu_beyond_one_sweep(ops, M):
    """ops.fc1_gelu forward (EPI 1) and backward (EPI 2, whose per-workgroup bias-gradient partial is accumulated across the tiles of a
    workgroup) against float64 F.gelu(x W^T + b) and its autograd on the same bf16 operands, with test_fc1_gelu_fused's bounds."""
    K, N = 96, 384
    assert _lib().pswin_fc1_gelu_partial_rows(M) == SKINNY_MAX_GRID
    case = _Case(f"fc1_gelu:M{M}", _skinny_trips(M, K, N))
    g = torch.Generator(DEV).manual_seed(11)
    x = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    w = torch.randn(N, K, generator=g, device=DEV) * 0.15
    b = torch.randn(N, generator=g, device=DEV) * 0.3
    gh = torch.randn(M, N, generator=g, device=DEV).to(torch.bfloat16)
    xr = x.double().requires_grad_(True)
    wr = w.to(torch.bfloat16).double().requires_grad_(True)
    br = b.double().requires_grad_(True)
    ref = F.gelu(xr @ wr.t() + br)
    (ref * gh.double()).sum().backward()
    xd = x.clone().requires_grad_(True)
    wd, bd = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    assert ops.fc1_gelu_supported(xd, N)
    h = ops.fc1_gelu(xd, wd, bd)
    h.backward(gh)
    case.close("h", h, ref, rtol=1e-2, atol=1e-2)
    case.close("dx", xd.grad, xr.grad, rtol=2e-2, atol=2e-2)
    rel = lambda a, r: float((a.double() - r).norm() / r.norm())
    assert bool(torch.isfinite(bd.grad).all()) and bool(torch.isfinite(wd.grad).all())
    case.ratio("dw_rel_norm", rel(wd.grad, wr.grad) / 1e-2)
    case.ratio("db_rel_norm", rel(bd.grad, br.grad) / 1e-2)
    case.done()


# ---- 6. the fused C = 96 window attention: the cases live in test_kernels_gpu.FUSED_CASES -----------------------------------------------
@pytest.mark.parametrize("B,nW,pano,mask_kind,trips", [(1, 257, True, 0, 2), (2, 515, True, 3, 3), (9, 300, False, 0, 2),
                                                       (2, 150, False, 4, 2)])
def test_fused_window_attention_cases_beyond_one_sweep(B, nW, pano, mask_kind, trips):
    """The oracle and chain tests of the fused kernel run these cases; here: they are still in the list and still more bias windows than
    the 256 persistent workgroups (mask_kind 4: a mask per image, nb = B nW)."""
    assert (B, nW, pano, mask_kind) in FUSED_CASES
    nb = B * nW if mask_kind == 4 else nW
    assert nb > FUSED_MAX_GRID and -(-nb // FUSED_MAX_GRID) == trips


# ---- 7. FlatAdamW: the grid-stride step of adamw_flat_kernel and adamw_flat_sched_kernel --------------------------------------------------
def _adamw_trips(n):
    assert n % 4 == 0 and n // 4 > 2 * ADAMW_MAX_BLOCKS * ADAMW_THREADS
    return -(-(n // 4) // (ADAMW_MAX_BLOCKS * ADAMW_THREADS))


def test_flat_adamw_beyond_one_sweep(ops):
    """test_flat_adamw_matches_torch_adamw's form for two steps at 8.4 M parameters (two full trips of the 4096 x 256 grid and 777
    granules of a third), with its tolerances, against torch.optim.AdamW and against a float64 restatement of the update."""
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    n = ADAMW_N
    case = _Case("flat_adamw", _adamw_trips(n))
    gen = torch.Generator(DEV).manual_seed(7)
    p0 = torch.randn(n, device=DEV, generator=gen)
    ref = torch.nn.Parameter(p0.clone())
    mine = torch.nn.Parameter(p0.clone())
    lr, (b1, b2), eps, wd = 1e-2, (0.9, 0.999), 1e-8, 0.05
    kw = dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    o_ref = torch.optim.AdamW([ref], **kw)
    o_mine = FlatAdamW(mine, **kw)
    shadow = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    o_mine.lowp = shadow
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)
    for step in range(2):
        g = torch.randn(n, device=DEV, generator=gen) * (0.1 + step)
        ref.grad, mine.grad = g.clone(), g.clone()
        o_ref.step()
        o_mine.step()
        t = step + 1
        p64 = p64 - lr * wd * p64
        m64 = m64 + (1.0 - b1) * (g.double() - m64)
        v64 = b2 * v64 + (1.0 - b2) * g.double() * g.double()
        p64 = p64 - (lr / (1.0 - b1 ** t)) * m64 / (v64.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
        case.close("p_vs_torch", mine.data, ref.data, rtol=2e-6, atol=2e-7)
        case.close("p_vs_float64", mine.data, p64, rtol=2e-6, atol=2e-7)
        case.equal(f"bf16 shadow, step {step}", shadow, mine.data.to(torch.bfloat16))
    st = o_ref.state[ref]
    case.close("exp_avg_vs_torch", o_mine.exp_avg, st["exp_avg"], rtol=1e-5, atol=1e-6)
    case.close("exp_avg_sq_vs_torch", o_mine.exp_avg_sq, st["exp_avg_sq"], rtol=1e-5, atol=1e-8)
    case.close("exp_avg_vs_float64", o_mine.exp_avg, m64, rtol=1e-5, atol=1e-6)
    case.close("exp_avg_sq_vs_float64", o_mine.exp_avg_sq, v64, rtol=1e-5, atol=1e-8)
    assert float(o_mine.step_t) == 2.0
    case.done()


def test_scheduled_clipped_adamw_beyond_one_sweep(ops):
    """test_grad_clip_matches_clip_grad_norm_then_adamw's form and bounds for three steps at 8.4 M parameters (adamw_flat_sched_kernel)."""
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    n = ADAMW_N
    case = _Case("flat_adamw_sched", _adamw_trips(n))
    p = _flat(n, 3)
    ref = torch.nn.Parameter(p.data.clone())
    max_norm = 3000.0                                         # |g| ~ 2897 * (0.5, 1.5, 2.5): clipped on two steps of three
    opt = FlatAdamW(p, lr=1e-2, lr_config=CFG, iters_per_epoch=IPE, grad_clip=dict(max_norm=max_norm, norm_type=2), **KW)
    o_ref = torch.optim.AdamW([ref], lr=1e-2, **KW)
    clipped = []
    for i, g in enumerate(_grads(n, 3, 4)):
        p.grad = g.clone()
        total = _ref_step(o_ref, ref, g, mmcv_lr(CFG, 1e-2, i, IPE), max_norm)
        opt.step()
        want = float(g.double().norm())
        case.ratio("grad_norm_f32", abs(float(opt.grad_norm) - float(total)) / (1e-5 * float(total)))
        case.ratio("grad_norm_f64", abs(float(opt._record[8]) - want) / (1e-12 * want))
        case.equal(f"flat gradient, step {i}", p.grad, g)     # the flat gradient keeps the unclipped values
        clipped.append(float(total) > max_norm)
        case.close("p_vs_torch", p.data, ref.data, rtol=2e-6, atol=2e-7)
    assert any(clipped) and not all(clipped)
    case.done()
