"""The window-attention backward kernels (csrc/pswin_attn.hip: attn_bwd_pair_kernel for bf16, attn_bwd_kernel<PSWIN_F32, 3> for f32)
against the float64 model of tests/_attn_bwd_cases.py.  Needs an MI355X.  tests/test_attention_backward_cases.py shows on the CPU that
every expectation used here is sound: the exact class has one answer and sees a transposed tile, a swapped window or head and a wrong
window order; a float32 evaluation of the model passes the dense rules and four planted defects fail them.

A. Exact class: lse = 0 and operands that make every weight exactly 1 or 0, so that P is a 0 / 1 matrix of the test's choosing and all
   of dq, dk, dv, the raw dS-sum tiles and dalpha / dbeta are small integers (times the f32 scale, rounded once): torch.equal, in the
   three operand layouts the product uses (fused [rows, 3C], separate q / k / v, packed [n, heads, 3, 49, 32]).
   Device facts this rests on: exp2(+-0) == 1, exp2(x) == 0 for x < -4e4, MFMA with f32 accumulation is exact on small integers.
B. Dense softmax: random bf16-exact operands with lse = float32(logsumexp64); the bf16 dq, dk, dv by the rounding-model rule of
   tests/test_attention_edges_gpu.py (_judge), everything else by the float32-definition rule of tests/test_cascade_gpu.py (_within).
C. The contract of pswin_attn_bwd_ex: strided outputs between NaN sentinels, determinism, chunk invariance, neighbour isolation, and
   the log-sum-exp rows the forward kernel hands to it."""
import ctypes

import pytest
import torch

import _attn_bwd_cases as bc
import _attn_edge_cases as ec
from _attn_edge_cases import DEV
from test_attention_edges_gpu import _judge

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
EXACT = [(f,) + c for f in bc.FAMILIES for c in bc.EXACT]
LAYOUTS = ("fused", "separate", "packed")


def _tiles(ops, t):
    return None if t is None else ops.Tiles(t.to(DEV), symmetric=False)


def _backward(ops, monkeypatch, c, dtype, layout, chunks=None):
    """ops.attention_backward on the operands of a case in one of the three layouts -> dq, dk, dv [n * 49, C], the raw gsum tiles the
    kernel wrote (captured where ops hands them to the table-gradient stage), dalpha (None: planar), dbeta; all on the CPU"""
    seen = []
    real = ops.grad_queue.table_gradients
    monkeypatch.setattr(ops.grad_queue, "table_gradients", lambda gsum, *a: (seen.append(gsum), real(gsum, *a))[1])
    dev = lambda t: t.to(DEV).to(dtype).contiguous()
    C, heads = c.C, c.heads
    lse = c.lse.to(DEV).contiguous()
    alpha, beta = c.alpha.to(DEV).contiguous(), c.beta.to(DEV).contiguous()
    args = (lse, alpha if c.dist is not None else None, beta, _tiles(ops, c.dist), _tiles(ops, c.mask), dev(c.dout), heads, bc.SCALE,
            c.nb, chunks or c.chunks, True, (None, None))
    if layout == "separate":
        dq, dk, dv, da, db = ops.attention_backward(dev(c.q), dev(c.k), dev(c.v), *args)
    else:
        x = bc.packed_of(c.q, c.k, c.v, heads) if layout == "packed" else torch.cat([c.q, c.k, c.v], 1)
        dx, _, _, da, db = ops.attention_backward(dev(x), None, None, *args, packed=layout == "packed")
        dq, dk, dv = dx[:, :C], dx[:, C:2 * C], dx[:, 2 * C:]
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(seen) == 1
    cpu = lambda t: None if t is None else t.detach().float().cpu()
    return dict(dq=cpu(dq), dk=cpu(dk), dv=cpu(dv), gsum=cpu(seen[0]), dalpha=cpu(da), dbeta=cpu(db))


def _assert_exact(got, want, heads, what):
    for name in ("dq", "dk", "dv"):
        msg = bc.first_mismatch(got[name], want[name], heads)
        assert msg is None, f"{what} {name}: {msg}"
    for name in ("gsum", "dalpha", "dbeta"):
        assert (got[name] is None) == (want[name] is None), (what, name)
        if want[name] is not None:
            msg = bc.first_tile_mismatch(got[name], want[name])
            assert msg is None, f"{what} {name}: {msg}"


# ---- A. the exact class -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,n_rep,nW,heads,chunks,tables", EXACT)
def test_backward_is_exact_on_zero_one_weights(ops, monkeypatch, family, n_rep, nW, heads, chunks, tables, dtype):
    """dq, dk, dv, the raw gsum tiles, dalpha and dbeta equal the float64 model in value (torch.equal on the float64 copies: -0 == +0),
    in every layout, and the layouts agree with each other bit for bit.  A p that is not exactly 1 or 0 shows first in gsum, whose
    entries would then not be integers.  Measured on the MI355X: equal in all 64 cases, so exp2(+-0) == 1 and exp2(-43000 ..) == 0
    hold there for both kernels."""
    c = bc.exact_case(family, n_rep, nW, heads, chunks, tables)
    want = c.expected(dtype)
    runs = {}
    for layout in LAYOUTS:
        runs[layout] = _backward(ops, monkeypatch, c, dtype, layout)
        _assert_exact(runs[layout], want, heads, layout)
    for layout in LAYOUTS[1:]:
        for name, t in runs[layout].items():
            if t is not None:
                assert torch.equal(t.view(torch.int32), runs["fused"][name].view(torch.int32)), (layout, name)


# ---- B. the dense class -----------------------------------------------------------------------------------------------------------------------
def _within(name, got, f32, truth):
    err, e32, bound = bc.within32(got, f32, truth)
    print(f"{name}: max|K - T| = {err:.3e}, max|def32 - T| = {e32:.3e} (largest |T| {float(truth.abs().max()):.3e}), ratio {err / e32:.3f}, "
          f"of the bound {err / bound:.3f}")
    assert e32 > 0
    assert err <= bound, name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", bc.DENSE)
def test_backward_error_on_dense_softmax_is_what_its_rounding_points_explain(ops, monkeypatch, key, dtype):
    """K = the kernel given lse = float32(logsumexp64), T = backward64 in float64, E = backward64 rounding P, dS and the outputs to
    bf16, def32 = backward64 in float32; T, E and def32 receive the same f32 lse.
    bf16 dq, dk, dv: rms(K - T) <= 1.5 rms(E - T) and max|K - T| <= 3 max|E - T| (_judge, the margin of the forward test).
    gsum, dalpha, dbeta (both dtypes) and the f32 dq, dk, dv: max|K - T| <= 4 max|def32 - T| + ulp32(max|T|).
    Measured on the MI355X, over the four cases: bf16 dq, dk, dv at rms and max ratios of 1.000 and 1.000 (rms(E - T) = 1.9e-4 .. 3.2e-4);
    max|K - T| / max|def32 - T|: f32 dq 1.22 .. 1.59, dk 1.10 .. 1.52, dv 0.80 .. 1.32; gsum 1.49 .. 2.02 (f32) and 1.55 .. 1.83 (bf16),
    dalpha 2.06 and 2.20 (f32), 1.05 and 1.52 (bf16), dbeta 0.74 .. 1.22; the largest share of a bound 0.495 (f32 dalpha, batch loop)."""
    c = bc.dense_case(*key)
    got = _backward(ops, monkeypatch, c, dtype, "fused")
    assert all(bool(torch.isfinite(t).all()) for t in got.values() if t is not None)
    bf = dtype == torch.bfloat16
    for name in ("dq", "dk", "dv"):
        if bf:
            _judge(name, got[name], c.E[name], c.T[name])
        else:
            _within(name, got[name], c.D32[name], c.T[name])
    for name in ("gsum", "dalpha", "dbeta"):
        assert (got[name] is None) == (c.T[name] is None), name
        if c.T[name] is not None:
            _within(name, got[name], c.D32[name], c.T[name])


# ---- C. the contract of pswin_attn_bwd_ex ----------------------------------------------------------------------------------------------------
GUARD = 64


class _Raw:
    """One call of pswin_attn_bwd_ex through _lib.call on fused qkv rows with ld_out = C + 8, ld_dqkv = 3C + 8 and 64 guard rows behind
    every buffer; outputs, gaps and guard rows hold a NaN bit pattern beforehand."""

    def __init__(self, ops, c, dtype, chunks=None, dout=None):
        from panoswintransformerobjectdetection_amd import _lib
        C, n, heads = c.C, c.n, c.heads
        self.rows, self.C, self.chunks = n * bc.TOK, C, chunks or c.chunks
        nan = lambda *shape, dt=dtype: torch.full(shape, float("nan"), dtype=dt, device=DEV)
        qkv = nan(self.rows + GUARD, 3 * C)
        qkv[:self.rows] = torch.cat([c.q, c.k, c.v], 1).to(DEV).to(dtype)
        self.dout_buf = nan(self.rows + GUARD, C + 8)
        self.dout_buf[:self.rows, :C] = (c.dout if dout is None else dout).to(DEV).to(dtype)
        self.dx = nan(self.rows + GUARD, 3 * C + 8)
        self.gsum = nan(self.chunks * c.nb, heads, bc.PAD, bc.PAD, dt=torch.float32)
        lse = c.lse.to(DEV).contiguous()
        alpha, beta = c.alpha.to(DEV).contiguous(), c.beta.to(DEV).contiguous()
        dist, mask = _tiles(ops, c.dist), _tiles(ops, c.mask)
        es = qkv.element_size()
        p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off * es)
        _lib.call("pswin_attn_bwd_ex", qkv, p(qkv), p(qkv, C), p(qkv, 2 * C), 3 * C, bc.TOK * 3 * C, bc.HD,
                  _lib.ptr(None if dist is None else dist.bwd), 0 if dist is None else dist.n, _lib.ptr(alpha if dist is not None else None),
                  _lib.ptr(beta), _lib.ptr(None if mask is None else mask.bwd), 0 if mask is None else mask.n, p(self.dout_buf), C + 8,
                  _lib.ptr(lse), p(self.dx), p(self.dx, C), p(self.dx, 2 * C), 3 * C + 8, _lib.ptr(self.gsum), self.chunks, n, c.nb, heads,
                  bc.SCALE, _lib.dtype_code(qkv))
        torch.cuda.synchronize()
        self.dx, self.gsum, self.dout_buf = self.dx.cpu(), self.gsum.cpu(), self.dout_buf.cpu()

    def bits(self, t):
        return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)

    def real(self):
        C = self.C
        return {name: self.dx[:self.rows, i * C:(i + 1) * C].float() for i, name in enumerate(("dq", "dk", "dv"))}


CONTRACT = [("all", 2, 3, 3, 1, "window"), ("all", 4, 3, 2, 2, "window"), ("mask", 2, 3, 2, 2, "shared")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,n_rep,nW,heads,chunks,tables", CONTRACT)
def test_strided_outputs_between_sentinels_and_determinism(ops, family, n_rep, nW, heads, chunks, tables, dtype):
    """Every real element is written and equals part A's expectation; every gap column and guard row of the output, and the whole dO
    buffer, keeps its bit pattern; gsum is finite and zero beyond 49 in both directions; a second call returns identical bits."""
    c = bc.exact_case(family, n_rep, nW, heads, chunks, tables)
    want = c.expected(dtype)
    a, b = _Raw(ops, c, dtype), _Raw(ops, c, dtype)
    got = a.real()
    for name in ("dq", "dk", "dv"):
        msg = bc.first_mismatch(got[name], want[name], heads)
        assert msg is None, f"{name}: {msg}"
    sentinel = a.bits(torch.full((1,), float("nan"), dtype=dtype))[0]
    assert bool((a.bits(a.dx)[:a.rows, 3 * c.C:] == sentinel).all()), "gap columns of dq | dk | dv written"
    assert bool((a.bits(a.dx)[a.rows:] == sentinel).all()), "guard rows of dq | dk | dv written"
    assert bool((a.bits(a.dout_buf)[:a.rows, c.C:] == sentinel).all()) and bool((a.bits(a.dout_buf)[a.rows:] == sentinel).all())
    assert bool(torch.isfinite(a.gsum).all()), "gsum not fully written"
    assert bool((a.gsum[..., bc.TOK:, :] == 0).all()) and bool((a.gsum[..., :, bc.TOK:] == 0).all())
    msg = bc.first_tile_mismatch(a.gsum, want["gsum"])
    assert msg is None, f"gsum: {msg}"
    assert torch.equal(a.bits(a.dx), b.bits(b.dx)) and torch.equal(a.bits(a.gsum), b.bits(b.gsum))


@pytest.mark.parametrize("dtype", DTYPES)
def test_results_do_not_depend_on_the_chunking(ops, dtype):
    """n_rep = 4: chunks = 1, 2, 4 give bit-identical dq, dk, dv, and (exact class: integer sums) gsum tiles whose sum over the chunks
    is identical."""
    c = bc.exact_case("all", 4, 3, 2, 2, "window")
    runs = {ch: _Raw(ops, c, dtype, chunks=ch) for ch in (1, 2, 4)}
    for ch in (2, 4):
        assert torch.equal(runs[ch].bits(runs[ch].dx), runs[1].bits(runs[1].dx)), ch
        total = runs[ch].gsum.view(ch, c.nb, c.heads, bc.PAD, bc.PAD).sum(0)
        assert torch.equal(total, runs[1].gsum), ch
    assert torch.equal(runs[1].gsum.double(), c.expected(dtype)["gsum"].view(2, c.nb, c.heads, bc.PAD, bc.PAD).sum(0))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chunks", [1, 4])
def test_a_window_of_inf_and_nan_stays_in_its_window(ops, chunks, dtype):
    """inf / NaN in ONE window's dO: dq, dk, dv of every other window keep their bits (the rows 49..63 of a window's operand tiles lie in
    the next window's memory: the window_rsrc range has to keep them out), also inside the batch loop of one work item (chunks = 1)."""
    c = bc.exact_case("all", 4, 3, 2, 2, "window")
    w = 4
    dout = c.dout.clone()
    dout[w * bc.TOK:(w + 1) * bc.TOK] = torch.tensor([float("inf"), float("nan"), float("-inf"), float("nan")]).repeat(c.C // 4)
    base, hit = _Raw(ops, c, dtype, chunks=chunks), _Raw(ops, c, dtype, chunks=chunks, dout=dout)
    keep = torch.ones(base.dx.shape[0], dtype=torch.bool)
    keep[w * bc.TOK:(w + 1) * bc.TOK] = False
    assert torch.equal(hit.bits(hit.dx)[keep], base.bits(base.dx)[keep])
    assert not bool(torch.isfinite(hit.real()["dq"][w * bc.TOK:(w + 1) * bc.TOK]).any())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", bc.DENSE)
def test_forward_log_sum_exp_rows(ops, key, dtype):
    """The lse rows ops.window_attention saves for the backward pass, on the dense cases: max|K - T| <= 4 max|def32 - T| + ulp32(max|T|)
    against the float64 logsumexp of the scores (def32: float32 scores and float32 logsumexp), and +inf on rows 49..63 (which the
    backward kernels turn into p = 0).  Measured on the MI355X: max|K - T| = 4.9e-7 .. 6.1e-7 at |lse| <= 4.7, 1.04 .. 1.38 times the
    float32 definition's error, at most 0.271 of the bound."""
    c = bc.dense_case(*key)
    x = c.x.to(DEV).to(dtype).requires_grad_(True)
    out = ops.window_attention(x, c.alpha.to(DEV), c.beta.to(DEV), None if c.dist is None else c.dist.to(DEV), _tiles(ops, c.mask),
                               c.heads, bc.SCALE, c.nb, chunks=c.chunks)
    lse = out.grad_fn.saved_tensors[3].detach().cpu()
    assert lse.shape == (c.n, c.heads, bc.PAD) and lse.dtype == torch.float32
    assert bool(torch.isposinf(lse[..., bc.TOK:]).all())
    _within("lse", lse[..., :bc.TOK], c.lse32(), c.lse64)
