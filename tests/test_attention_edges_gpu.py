"""The window-attention kernels (csrc/pswin_attn.hip: bf16 / f32 core; csrc/pswin_fused.hip: C = 96 qkv -> attention -> proj;
csrc/pswin_qkvattn.hip: C = 192 / 384 qkv -> attention) where the softmax has a known answer.  Needs an MI355X.
tests/test_attention_edges.py shows on the CPU that the float64 oracle meets every expectation used here.

A. One-hot rows (tests/_attn_edge_cases.py): the mask leaves one key per row, P is a 0 / 1 matrix, out[i] = v[sel(i)], dV = the
   selected dO rows, dQ = dK = 0.  Walks the row-max / row-sum reductions and the V / dO operand layouts through every (row, key) pair,
   and the TRANSPOSED mask tiles of the backward pass (the table is not symmetric).
B. Row offsets of +100 / -100 / 0 / +37.5 on all keys of a row: softmax is unchanged, so the kernel must agree with itself without them
   (and with the float64 oracle given the same offsets, or two equally wrong runs would agree).
C. The bf16 forward error on random input against a float64 model that rounds where the kernel rounds.

The kernels' arithmetic, from which the bounds below follow (line numbers of the kernel sources):
  * scores stay UNSCALED: s' = q.k + bias / scale in f32 (pswin_attn.hip:164, 203; pswin_fused.hip:311; pswin_qkvattn.hip:333), q is NOT
    multiplied by the scale before anything is rounded; p = exp2((s' - m') * scale * log2 e) with m' the row maximum (pswin_attn.hip:217-237).
  * bf16 rounding points, all round-to-nearest-even (`(__bf16)` casts and __builtin_convertvector, pswin_attn_frag.hpp:113,
    pswin_common.hpp:47):
      core kernel     P before P.V (pswin_attn.hip:252 pack_frag); the output o = (P.V) / l (pswin_attn.hip:260-261 -> pswin_attn_frag.hpp:236);
                      l is the f32 sum of the UNROUNDED p (pswin_attn.hip:239, 245).  q, k, v arrive as bf16.
      pswin_qkvattn   q, k after the Linear with its bias (:277-278), v (:285), P (:349), l = the sum of the ROUNDED p (a row of ones in the
                      P.V MFMA, :346-354), the attention rows (:357).
      pswin_fused     q, k (:216 through gemm_T), v (:269), P (:332), l = the sum of the rounded p (:329-337), the attention rows (:339),
                      the proj output (:375).
  * backward (pswin_attn.hip:397 / :660): p = exp2(s' * scale * log2 e - lse * log2 e) from the stored lse = m' * scale + log l; P and dS are
    rounded to bf16 for dV = dO^T P, dK = Q^T dS, dQ = dS K (:422-423 / :677-678), delta = sum_j p * dP in f32 from the unrounded p.
"""
import pytest
import torch

import _attn_edge_cases as ec
from _attn_edge_cases import DEV

pytestmark = pytest.mark.gpu

SCALE = 32 ** -0.5
CORE = [c + (h, p) for c in ec.CORE_ONEHOT for h in (1, 3) for p in (True, False)] + [ec.CORE_ONEHOT_LOOP + (3, True)]
DTYPES = [torch.float32, torch.bfloat16]


def _core_run(ops, x, alpha, beta, dist, mask, gout, heads, nb, dtype, chunks=None):
    """pswin_attn_fwd + pswin_attn_bwd on fused [rows, 3C] qkv rows -> out, dx = [dq | dk | dv], dalpha (None in planar mode), dbeta"""
    xd = x.to(DEV).to(dtype).requires_grad_(True)
    ad, bd = alpha.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    mt = None if mask is None else ops.Tiles(mask.reshape(-1, 49, 49).to(DEV), symmetric=False)
    out = ops.window_attention(xd, ad, bd, None if dist is None else dist.to(DEV), mt, heads, SCALE, nb, chunks=chunks)
    out.backward(gout.to(DEV).to(dtype))
    return (out.detach().float().cpu(), xd.grad.float().cpu(), None if ad.grad is None else ad.grad.float().cpu(), bd.grad.float().cpu())


def _device_module(ops, att, x, uv, mask, B, nW, pano, mask_kind, C):
    from panoswintransformerobjectdetection_amd.backbone import WindowAttention
    attd = WindowAttention(C, 7, C // 32)
    attd.load_state_dict(att.state_dict())
    attd = attd.to(DEV)
    uvd = uv.to(DEV)
    dist = ops.Tiles(ops.haversine_windows(uvd, uvd), symmetric=True) if pano else None
    mt = None if mask is None else ops.Tiles(mask.reshape(-1, 49, 49).to(DEV), symmetric=False)
    return attd, x.to(DEV).to(torch.bfloat16).view(-1, C), dist, mt, (B * nW if mask_kind == 4 else nW)


def _fused_forward(ops, attd, xd, dist, mt, nb, train):
    """what the fused kernel itself returns: proj_nobias(attention) at C = 96, the attention rows at C = 192 / 384; train = the mode that
    saves q, k, v and lse for a backward pass, otherwise the forward-only kernel variant"""
    f = ops.window_attention_fused if xd.shape[1] == 96 else ops.window_attention_qkv_fused
    if train:
        return f(xd.clone().requires_grad_(True), attd, dist, mt, nb).detach().float().cpu().double()
    with torch.no_grad():
        return f(xd, attd, dist, mt, nb).float().cpu().double()


def _fused_seed(C, B, nW, pano, mask_kind):
    return f"{B}{nW}{pano}{mask_kind}" if C == 96 else f"q{C}{B}{nW}{pano}{mask_kind}"       # the seeds of tests/test_kernels_gpu.py


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts if t is not None)


# ---- A. one-hot rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,n_rep,nW,chunks,heads,pano", CORE)
def test_core_kernel_selects_on_one_hot_rows(ops, family, n_rep, nW, chunks, heads, pano, dtype):
    """Input condition (float64, CPU): the 48 unselected keys of a row hold <= 1e-20 of its weight, and no single one more than 2^-134,
    half the smallest bf16 subnormal, so every unselected P entry rounds to bf16 zero.

    bf16 forward, out == v[sel] bit for bit: the selected score IS the row maximum, so p = exp2(fma(m', c, -(m' c))) = 1 + e with
    |e| <= 2^-24 |m' c| ln 2 ~ 1e-6 (c = scale * log2 e, |m' c| < 10), which rounds to the bf16 1.0; the MFMA then yields v exactly,
    l = 1 + e, and v / l rounds back to the bf16 value v (half a bf16 ulp is 2^-9 relative).
    bf16 backward: p = exp2(s' c - lse log2 e) = 1 + O(1e-6) rounds to 1.0 and the unselected ones to 0, so dV = dO^T P holds the dO row
    that selected the key, exactly (permutations), or the f32 sum of the 49 dO rows rounded once (column family: |err| <= 2^-8 |dv| for
    the rounding + 1e-5 sum|dO| for the f32 accumulation of 49 terms), and exactly 0 in every row that nobody selected.
    f32 forward, rtol 1e-6: v * p, * (1 / l) and their roundings are ~3 ulp = 2e-7; atol 1e-30 covers the unselected terms (truth <= 49 *
    e^-72 * |v|).  f32 dV, rtol 1e-4: p is recomputed from the stored lse, whose rounding is ~1e-6 relative in p.
    dQ, dK (truth 0 to 1e-20): <= 1e-3 max|dV|.  A wrong dS is of the order |dO| |v| |k|, a thousand times that; what a right kernel leaves
    is dS(sel) = p (1 - p) dP ~ 1e-6 |dP|.
    Table gradients (truth 0 to 1e-20; the oracle's own are 0, so an allclose with a tolerance relative to them could not be met by any f32
    arithmetic): <= 1e-3 of what a dS of the order of dP at the selected entries would leave in the table, per bin sum |dP(i, sel i)| (x d),
    computed in float64 (table_grad_scale); a right kernel leaves ~1e-6 of it."""
    bf = dtype == torch.bfloat16
    x, alpha, beta, dist, mask, gout, sel, kind = ec.core_onehot_case(family, n_rep, nW, heads, pano, bf)
    C, n = heads * 32, n_rep * nW
    qkv = x.view(n, 49, 3, C)
    _, p = ec.attention64(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], SCALE, ec.core_bias(alpha, beta, dist, heads, n_rep), mask, heads)
    rest, single = ec.unselected_weight(p, sel)
    assert rest <= 1e-20 and single < 2.0 ** -134
    rows = ec.selected_rows(sel, n)
    v = x[:, 2 * C:]
    out, dx, da, db = _core_run(ops, x, alpha, beta, dist, mask, gout, heads, n if kind == 4 else nW, dtype, chunks)
    assert _finite(out, dx, da, db)
    dv, dv_ref = dx[:, 2 * C:], torch.zeros(n * 49, C, dtype=torch.float64).index_add_(0, rows, gout.double())
    hit = torch.zeros(n * 49, dtype=torch.bool)
    hit[rows] = True
    ga, gb = ec.table_grad_scale(gout, v, sel, heads, dist)
    print(f"max|out - v[sel]| = {(out - v[rows]).abs().max().item():.3e}  max|dv - ref| = {(dv.double() - dv_ref).abs().max().item():.3e}  "
          f"max|dq, dk| / max|dv| = {dx[:, :2 * C].abs().max().item() / dv_ref.abs().max().item():.3e}  "
          f"max|dbeta| / scale = {db.abs().max().item() / gb:.3e}" + ("" if da is None else f"  max|dalpha| / scale = {da.abs().max().item() / ga:.3e}"))
    if bf:
        assert torch.equal(out, v[rows])
    else:
        assert torch.allclose(out, v[rows], rtol=1e-6, atol=1e-30)
    if family != "column":
        assert hit.all()
        if bf:
            assert torch.equal(dv[rows], gout)
        else:
            assert torch.allclose(dv[rows], gout, rtol=1e-4, atol=0)
    else:
        assert int(hit.sum()) == n
        acc = torch.zeros(n * 49, C, dtype=torch.float64).index_add_(0, rows, gout.double().abs())
        bound = (2.0 ** -8 if bf else 1e-4) * dv_ref.abs() + 1e-5 * acc
        assert ((dv.double() - dv_ref).abs() <= bound)[hit].all()
        if bf:
            assert (dv[~hit] == 0).all()
        else:
            assert dv[~hit].abs().max().item() <= 1e-29          # truth <= 49 * e^-72 * max|dO| = 3e-30
    assert dx[:, :2 * C].abs().max().item() <= 1e-3 * dv_ref.abs().max().item()
    assert db.abs().max().item() <= 1e-3 * gb
    if pano:
        assert da.abs().max().item() <= 1e-3 * ga
    else:
        assert da is None


@pytest.mark.parametrize("C", [96, 192, 384])
@pytest.mark.parametrize("family,B,nW,pano", ec.FUSED_ONEHOT)
def test_fused_kernels_select_on_one_hot_rows(ops, family, B, nW, pano, C):
    """v is computed inside the kernel, so the truth is float64: v64 = x Wv^T + b_v from the bf16-rounded x and weights of _fused_case.
    With P = 1.0 and l = 1.0 (the sum of the rounded weights) the attention row is the kernel's own bf16 v[sel]:
      C = 192 / 384 (the kernel returns the attention rows): |o - v64[sel]| <= 2^-8 |v64| (one bf16 rounding, worst case) + 1e-5 max|v64|
      (the f32 accumulation over C <= 384 terms).
      C = 96 (the kernel returns y = proj_nobias(o)): with y64 = v64[sel] Wp^T,  |y - y64| <= 2^-8 |y64| (rounding of y) + 2^-8 (|o64| |Wp|^T)
      (o's rounding, propagated in the worst case) + 1e-5 max|y64| (accumulation).
    Both in the training mode and in the forward-only mode (another kernel variant: nothing saved).
    Gradients against the float64 oracle module: y, dx and the parameter gradients at the tolerances of the fused kernels' oracle tests; the
    q and k rows of the qkv weight / bias gradients (truth 0) <= 1e-3 of the largest v-row entry; the table gradients as in the core test."""
    att, x, uv, mask, gout, sel, kind = ec.fused_onehot_case(family, B, nW, pano, C)
    n, heads = B * nW, C // 32
    _, _, p = ec.fused_model(att, x, uv, mask, pano, B)
    assert ec.unselected_weight(p, sel)[0] <= 1e-20
    rows = ec.selected_rows(sel, n)
    v64 = ec.fused_v64(att, x)
    o64 = v64[rows]
    wp = att.proj.weight.double()
    y64 = o64 @ wp.T
    attd, xd, dist, mt, nb = _device_module(ops, att, x, uv, mask, B, nW, pano, kind, C)
    for train in (True, False):
        got = _fused_forward(ops, attd, xd, dist, mt, nb, train)
        assert _finite(got)
        if C == 96:
            err, bound = (got - y64).abs(), 2.0 ** -8 * y64.abs() + 2.0 ** -8 * (o64.abs() @ wp.abs().T) + 1e-5 * y64.abs().max()
        else:
            err, bound = (got - o64).abs(), 2.0 ** -8 * o64.abs() + 1e-5 * v64.abs().max()
        print(f"train={train}: max(err / bound) = {(err / bound).max().item():.3f}")
        assert (err <= bound).all()
    y, dx, grads = ec._fused_run(ops, att, x, uv, mask, gout, B, nW, pano, kind, True, C)
    yo, dxo, go = ec.module_oracle(att, x, uv, ec.oracle_mask(mask, kind, B, nW), pano, gout, B)
    assert _finite(y, dx, *grads.values())
    close = lambda a, r, rt, at: torch.allclose(a.double().reshape(r.shape), r, rtol=rt, atol=at * r.abs().max().item())
    assert close(y, yo, 3e-2, 2e-2)
    assert close(dx, dxo, 5e-2, 3e-2)
    datt = gout.double().reshape(-1, C) @ wp                       # dO of the attention core
    ga, gb = ec.table_grad_scale(datt, v64, sel, heads, ec.po.haversine(uv.double(), uv.double()) if pano else None)
    for k, ref in go.items():
        if k == "proj.bias" or (k.endswith("alpha_table_Te") and not pano):
            continue
        assert k in grads, k
        if k.endswith("_table_Te"):
            s = ga if "alpha" in k else gb
            print(f"max|{k}.grad| / scale = {grads[k].abs().max().item() / s:.3e}")
            assert grads[k].abs().max().item() <= 1e-3 * s, k
        else:
            assert close(grads[k], ref, 5e-2, 3e-2), k
    for k in ("qkv.weight", "qkv.bias"):
        g = grads[k]
        print(f"{k}: max|q, k rows| / max|v rows| = {g[:2 * C].abs().max().item() / g[2 * C:].abs().max().item():.3e}")
        assert g[:2 * C].abs().max().item() <= 1e-3 * g[2 * C:].abs().max().item(), k


# ---- B. row offsets ----------------------------------------------------------------------------------------------------------------------
def _same(name, got, base, bf, forward):
    """f32: rtol 1e-4, atol 1e-4 max (the unscaled score near 100 / scale = 565 carries an f32 rounding of 3e-5, i.e. 5e-6 in the logit and
    in p).  bf16 forward: the perturbation can flip the rounding of a P entry or of the output, one bf16 ulp: |d| <= 2^-7 |y| + 2^-8 max|y|.
    bf16 gradients: the tolerance the fused kernels are held to against the three-kernel chain (rtol 2e-2, atol 1e-2 max)."""
    d, mx = (got - base).abs(), base.abs().max().item()
    if not bf:
        bound = 1e-4 * base.abs() + 1e-4 * mx
    elif forward:
        bound = 2.0 ** -7 * base.abs() + 2.0 ** -8 * mx
    else:
        bound = 2e-2 * base.abs() + 1e-2 * mx
    print(f"{name}: max(|with - without| / bound) = {(d / bound).max().item():.3f}")
    assert (d <= bound).all(), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_rep,nW,heads,pano,mask_kind", ec.CORE_RANDOM)
def test_core_kernel_is_unchanged_by_row_offsets(ops, n_rep, nW, heads, pano, mask_kind, dtype):
    """The run with the offsets against the run without them (_same), and against the float64 oracle given the same offset mask at the
    tolerances of test_window_attention_fwd_bwd.  Everything finite: rows at +100 overflow exp() without the right row maximum, rows at
    -100 on top of a -100 mask are the reference's fully masked rows."""
    bf = dtype == torch.bfloat16
    x, alpha, beta, dist, mask, gout = ec._attn_case(n_rep, nW, heads, pano, mask_kind, f"{n_rep}{nW}{heads}")
    if bf:
        x, gout = x.to(dtype).float(), gout.to(dtype).float()
    off = ec.row_offset_mask(mask, nW)
    nb = n_rep * nW if mask_kind == 4 else nW
    base = _core_run(ops, x, alpha, beta, dist, mask, gout, heads, nb, dtype)
    got = _core_run(ops, x, alpha, beta, dist, off, gout, heads, nb, dtype)
    d = lambda t: None if t is None else t.double()
    ref = ec._attn_oracle(d(x), d(alpha), d(beta), d(dist), off, d(gout), heads, n_rep, nW)
    assert _finite(*got)
    rt, at = (2e-5, 2e-5) if not bf else (3e-2, 3e-2)
    for i, name in enumerate(("out", "dx", "dalpha", "dbeta")):
        if got[i] is None:
            assert not pano and name == "dalpha" and base[i] is None
            continue
        _same(name, got[i], base[i], bf, i == 0)
        if i == 0:
            assert torch.allclose(got[i].double(), ref[i], rtol=rt, atol=at), name
        else:
            assert torch.allclose(got[i].double(), ref[i], rtol=rt * 5, atol=at * ref[i].abs().max().item()), name


@pytest.mark.parametrize("C,B,nW,pano,mask_kind", ec.FUSED_RANDOM)
def test_fused_kernels_are_unchanged_by_row_offsets(ops, C, B, nW, pano, mask_kind):
    """As for the core kernel: what the fused kernel returns (both modes) and the gradients of the chain around it, with against without the
    offsets (_same), and against the float64 oracle module given the same offset mask at the tolerances of the fused kernels' oracle tests."""
    att, x, uv, mask, gout = ec._fused_case(B, nW, pano, mask_kind, _fused_seed(C, B, nW, pano, mask_kind), C)
    off = ec.row_offset_mask(mask, nW)
    kind = mask_kind or 3
    a0 = _device_module(ops, att, x, uv, mask, B, nW, pano, mask_kind, C)
    a1 = _device_module(ops, att, x, uv, off, B, nW, pano, kind, C)
    for train in (True, False):
        k0, k1 = _fused_forward(ops, *a0, train), _fused_forward(ops, *a1, train)
        assert _finite(k1)
        _same(f"kernel output (train={train})", k1, k0, True, True)
    y0, dx0, g0 = ec._fused_run(ops, att, x, uv, mask, gout, B, nW, pano, mask_kind, True, C)
    y1, dx1, g1 = ec._fused_run(ops, att, x, uv, off, gout, B, nW, pano, kind, True, C)
    yo, dxo, go = ec.module_oracle(att, x, uv, off, pano, gout, B)
    assert _finite(y1, dx1, *g1.values())
    close = lambda a, r, rt, at: torch.allclose(a.double().reshape(r.shape), r, rtol=rt, atol=at * r.abs().max().item())
    assert close(y1, yo, 3e-2, 2e-2)
    assert close(dx1, dxo, 5e-2, 3e-2)
    _same("dx", dx1, dx0, True, False)
    assert g1.keys() == g0.keys()
    for k, ref in go.items():
        if k == "proj.bias" or (k.endswith("alpha_table_Te") and not pano):
            continue
        assert close(g1[k], ref, 5e-2, 3e-2), k
        _same(k, g1[k], g0[k], True, False)


# ---- C. the rounding model ---------------------------------------------------------------------------------------------------------------
def _judge(name, got, model, truth):
    """rms(K - T) <= 1.5 rms(E - T) and max|K - T| <= 3 max|E - T|: with the same rounding points the two errors are the same random
    variable up to the f32 accumulation order and exp2's last ulp; a maximum over 1e4 - 1e5 elements fluctuates more than an rms."""
    rk, re, mk, me = ec.err_stats(got, model, truth)
    print(f"{name}: rms(K - T) = {rk:.3e}, rms(E - T) = {re:.3e}, ratio {rk / re:.3f}; max|K - T| = {mk:.3e}, max|E - T| = {me:.3e}, ratio {mk / me:.3f}")
    assert re > 0
    assert rk <= 1.5 * re and mk <= 3 * me, name


@pytest.mark.parametrize("n_rep,nW,heads,pano,mask_kind", ec.CORE_RANDOM[:2])
def test_core_bf16_forward_error_is_what_its_rounding_points_explain(ops, n_rep, nW, heads, pano, mask_kind):
    """K = the bf16 core kernel's output, T = attention64 on the same bf16 q, k, v, E = attention64 rounding P and the output to bf16
    (the core kernel's two rounding points, see the module docstring; l from the unrounded p).
    Measured ratios rms(K - T) / rms(E - T), max|K - T| / max|E - T| on the MI355X: 1.000 and 1.000 in every case (rms(E - T) =
    3.6e-4 and 4.1e-4)."""
    x, alpha, beta, dist, mask, gout = ec._attn_case(n_rep, nW, heads, pano, mask_kind, f"{n_rep}{nW}{heads}")
    x, gout = x.to(torch.bfloat16).float(), gout.to(torch.bfloat16).float()
    C, n = heads * 32, n_rep * nW
    qkv = x.view(n, 49, 3, C)
    bias = ec.core_bias(alpha, beta, dist, heads, n_rep)
    t, _ = ec.attention64(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], SCALE, bias, mask, heads)
    e, _ = ec.attention64(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], SCALE, bias, mask, heads, ec.bf16_round)
    out = _core_run(ops, x, alpha, beta, dist, mask, gout, heads, nW, torch.bfloat16)[0]
    _judge("out", out.reshape(n, 49, C), e, t)


@pytest.mark.parametrize("C,B,nW,pano,mask_kind", ec.FUSED_MODEL)
def test_fused_bf16_forward_error_is_what_its_rounding_points_explain(ops, C, B, nW, pano, mask_kind):
    """K = what the fused kernel returns (C = 96: proj_nobias of the attention; C = 192 / 384: the attention rows), in both modes;
    T = fused_model in float64, E = fused_model rounding qkv, P, the attention rows and (C = 96) the proj output to bf16, l from the
    rounded p (see the module docstring).
    Measured ratios rms(K - T) / rms(E - T), max|K - T| / max|E - T| on the MI355X: 1.000 and 1.000 in every case and both modes
    (rms(E - T) = 2.4e-4 .. 2.9e-4)."""
    att, x, uv, mask, gout = ec._fused_case(B, nW, pano, mask_kind, _fused_seed(C, B, nW, pano, mask_kind), C)
    ot, yt, _ = ec.fused_model(att, x, uv, mask, pano, B)
    oe, ye, _ = ec.fused_model(att, x, uv, mask, pano, B, ec.bf16_round)
    args = _device_module(ops, att, x, uv, mask, B, nW, pano, mask_kind, C)
    for train in (True, False):
        got = _fused_forward(ops, *args, train)
        _judge(f"C={C} train={train}", got, ye if C == 96 else oe, yt if C == 96 else ot)
