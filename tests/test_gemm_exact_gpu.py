"""The GEMM and GELU kernels bit for bit on operands with one right answer (tests/_gemm_exact_cases.py; tests/test_gemm_exact.py
checks on the CPU that every case used here meets its conditions).  Needs an MI355X.

  csrc/pswin_gemm_nt.hip   pswin_gemm_nt, _f32, _gelu_fwd, _gelu_bwd        dense / ties / select, saturated
  csrc/pswin_gemm_tn.hip   pswin_gemm_tn_ring, _bias, _jobs                 dense / ties, every slab and bias partial on its own
  csrc/pswin_gemm.hip      pswin_gemm_skinny, pswin_fc1_gelu_*, pswin_mlp0_*  dense / ties / select, saturated
  csrc/pswin_mlp.hip       pswin_bias_gelu_fwd, _bwd                        saturated; and the GELU itself over every finite bf16 value
                                                                            against float64

Every comparison is torch.equal on the values (-0 equals 0: the kernels produce v * 0 = -0) except the float64 GELU sweep.
A failure names the first wrong element, which for the `select` class is the (m, n) that fetched the wrong source element."""

import pytest
import torch
import torch.nn as nn

import _gemm_exact_cases as gc
from _util import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def _same(got, want, what):
    """torch.equal with the first differing element in the message"""
    want = want.to(got.device)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = (got != want) | (got != got)
    idx = tuple(int(i) for i in bad.nonzero()[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at {idx}: got {float(got[idx])!r}, want {float(want[idx])!r}")


def _dev(c, *keys):
    return [None if c[k] is None else c[k].to(DEV) for k in keys]


# ---------------------------------------------------------------------------------------------------------------------
# the tiled GEMM
# ---------------------------------------------------------------------------------------------------------------------
def _nt_run(ops, M, K, N, tiles, classes):
    for cls in classes:
        c = gc.nt_case(cls, M, K, N)
        x, w, b = _dev(c, "x", "w", "bias")
        for bias in ((None, b) if b is not None else (None,)):
            want = c["want"] + (0.0 if bias is None else c["bias"].double())
            want32, want16 = want.float(), gc.rne_bf16(want)
            for tile in tiles:
                what = f"{cls} M={M} K={K} N={N} tile={tile} bias={bias is not None} {gc.nt_form(M, K, N, tile)}"
                y16 = ops.gemm_nt(x, w, bias, tile)
                _same(y16, want16, "pswin_gemm_nt " + what)
                if tile != 96:
                    y32 = ops.gemm_nt(x, w, bias, tile, out_f32=True)
                    _same(y32, want32, "pswin_gemm_nt_f32 " + what)
                    _same(y16, y32.to(BF16), "bf16 result against the f32 result rounded " + what)


@pytest.mark.parametrize("K", gc.NT_K)
@pytest.mark.parametrize("N", gc.NT_N)
def test_tiled_gemm_is_exact(ops, K, N):
    """pswin_gemm_nt (tile_m 64, 96, 128) and pswin_gemm_nt_f32 (64, 128), with and without bias, M in {64 .. 333}: a partial last row
    tile for every tile height and tile counts that are no multiples of 8 (the XCD dealing).  All these launches have at most
    6 x 4 = 24 tiles, so by the launcher's rule (launch_nt: tiles <= 256 and K / 64 >= 3) K = 64 and 128 run the two-stage loop with one and
    two k-steps, K = 192 (the smallest count that takes it), 256 and 3072 the four-stage loop with counted waits."""
    for M in gc.NT_M:
        _nt_run(ops, M, K, N, (64, 96, 128), gc.NT_CLASSES)


@pytest.mark.parametrize("M,K,N,tile", gc.NT_DEEP)
def test_tiled_gemm_two_stage_loop_with_a_long_contraction_is_exact(ops, M, K, N, tile):
    """More than 256 tiles (264 of 64 rows at M = 4161, 260 of 128 rows at M = 8200; N = 768): the launcher's rule then picks the
    two-stage loop although K / 64 >= 3 -- 3 and 48 k-steps through the two LDS stages, a last row tile of 1 and 8 rows."""
    assert gc.nt_form(M, K, N, tile) == "two-stage"
    _nt_run(ops, M, K, N, (tile,), ("dense", "ties", "select_x"))


# ---------------------------------------------------------------------------------------------------------------------
# the tiled GEMM's GELU forms and the autograd nodes on them
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", gc.MLP_NT)
@pytest.mark.parametrize("tile", [64, 128])
def test_tiled_gemm_gelu_epilogues_are_exact_where_the_gelu_is_saturated(ops, M, C, tile):
    """pswin_gemm_nt_gelu_fwd: pre = the exact product, h = relu(pre + b1).  pswin_gemm_nt_gelu_bwd: dpre = (dout W2) [v > 0] and EVERY
    row of the per-tile workspace = the integer column sum over exactly that tile's rows (a row past M counted, or a sum written to the
    neighbouring tile's row, shows here and not in the total).  K = C = 192: 3 k-steps, four-stage loop; C = 768 (12 k-steps): the same."""
    from panoswintransformerobjectdetection_amd import _lib
    c = gc.mlp_case(M, C)
    N = c["N"]
    x, w1, b1, w2, dout = _dev(c, "x", "w1", "b1", "w2", "dout")
    pre = torch.full((M, N), float("nan"), dtype=BF16, device=DEV)
    h = torch.full_like(pre, float("nan"))
    ops.call("pswin_gemm_nt_gelu_fwd", x, ops.ptr(x), ops.ptr(w1), ops.ptr(b1), ops.ptr(pre), ops.ptr(h), M, C, N, tile)
    _same(pre, c["pre"].to(BF16), "pre")
    _same(h, c["h"].to(BF16), "h")
    rows = _lib.load().pswin_gemm_nt_partial_rows(M, tile)
    assert rows == -(-M // tile)
    wt = w2.t().contiguous()
    dpre = torch.full_like(pre, float("nan"))
    ws = torch.full((rows, N), float("nan"), dtype=F32, device=DEV)
    ops.call("pswin_gemm_nt_gelu_bwd", dout, ops.ptr(dout), ops.ptr(wt), ops.ptr(pre), ops.ptr(b1), ops.ptr(dpre), ops.ptr(ws), M, C, N, tile)
    _same(dpre, c["dpre"].to(BF16), "dpre")
    _same(ws, gc.tile_sums(c["dpre"], tile).float(), "per-tile column sums")


def _mlp_modules(c):
    fc1, fc2 = nn.Linear(c["C"], c["N"]).to(DEV), nn.Linear(c["N"], c["C"]).to(DEV)
    with torch.no_grad():
        fc1.weight.copy_(c["w1"].float()); fc1.bias.copy_(c["b1"]); fc2.weight.copy_(c["w2"].float())
    for lin, w in ((fc1, c["w1"]), (fc2, c["w2"])):
        wb = w.to(DEV)
        lin.__dict__["_lowp"] = (wb, None)
        lin.__dict__["_lowp_t"] = wb.t().contiguous()
    return fc1, fc2


def _wgrad_want(ops, exact, M, N, K):
    """A weight gradient dy^T x of M rows as ops.weight_gradient returns it: from the ring kernel (one split at these M: the f32 sum
    itself) where ops.gemm_tn_ring_splits takes the shape, else from the library's bf16 GEMM: the RNE of the exact sum, as f32"""
    sp = ops.gemm_tn_ring_splits(M, N, K)
    assert sp in (0, 1)
    return exact.float() if sp else gc.rne_bf16(exact).float()


@pytest.mark.parametrize("M,C", gc.MLP_NT + (gc.MLP_NT_RING,))
def test_mlp_autograd_nodes_give_the_exact_integer_chain(ops, M, C):
    """ops.mlp_fused and ops.bias_gelu_linear (fc1 on pswin_gemm_nt for the latter) on the saturated Mlp: the output and every gradient
    equal the integer chain, rounded once to bf16 where a result leaves as bf16 (out, dx) -- every intermediate is exact in bf16, so it
    does not matter where a kernel rounds.  At M = 577 the two weight gradients run on the ring kernel (one split, f32), below 512 rows
    on the library GEMM, which returns bf16."""
    c = gc.mlp_case(M, C)
    N = c["N"]
    fc1, fc2 = _mlp_modules(c)
    x, dout = _dev(c, "x", "dout")
    assert ops.mlp_fused_supported(x, N) and (ops.gemm_tn_ring_splits(M, N, C) == 1) == (M >= 512)
    for path in ("mlp_fused", "bias_gelu_linear"):
        for p in (*fc1.parameters(), *fc2.parameters()):
            p.grad = None
        xx = x.clone().requires_grad_(True)
        if path == "mlp_fused":
            out = ops.mlp_fused(xx, fc1, fc2)
        else:
            out = ops.bias_gelu_linear(ops.linear(xx, fc1, BF16, use_bias=False), fc1.bias, fc2)
        out.backward(dout)
        torch.cuda.synchronize()
        _same(out.detach(), gc.rne_bf16(c["out"]), path + " out")
        _same(xx.grad, gc.rne_bf16(c["dx"]), path + " dx")
        _same(fc1.bias.grad, c["db1"].float(), path + " db1")
        _same(fc1.weight.grad, _wgrad_want(ops, c["dw1"], M, N, C), path + " dW1")
        _same(fc2.weight.grad, _wgrad_want(ops, c["dw2"], M, C, N), path + " dW2")


# ---------------------------------------------------------------------------------------------------------------------
# the ring weight-gradient kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", gc.TN_SHAPES)
def test_ring_weight_gradient_slabs_are_exact(ops, N, K):
    """pswin_gemm_tn_ring (bf16 slabs) and pswin_gemm_tn_ring_bias (f32 slabs + bias partials) for M in {64 .. 4033} and splits in
    {1, 2, 3, M / 64}: EACH slab part[s] = dy[lo:hi]^T x[lo:hi] with lo, hi from the launcher's rows_per_split rule (a split past M:
    zeros; M = 130 in two splits: a split of two rows; M / 64 splits: two slabs each), each bias partial the column sum of its rows,
    the zero_cols range exact zeros.  (192, 192), (384, 576): 192 x 192 tiles, three stages; K = 96 with N = 48 .. 384: one 96 x 384
    tile, two stages, the widths 64, 80, 208, 368 leave a wave's 48 columns partly filled; (96, 384): one 384 x 96 tile."""
    from panoswintransformerobjectdetection_amd import _lib
    lib = _lib.load()
    for M in gc.TN_M:
        assert lib.pswin_gemm_tn_ring_supported(M, N, K) == 1
        for sp in gc.tn_splits(M):
            for cls in ("dense", "ties"):
                c = gc.tn_case(cls, M, N, K, sp)
                dy, x = _dev(c, "dy", "x")
                what = f"{cls} M={M} N={N} K={K} splits={sp}"
                part, dbp = ops.gemm_tn_ring(dy, x, sp, F32, bias_sums=True, zero_cols=c["zero_cols"])
                _same(part, c["want"].float(), "f32 slabs " + what)
                _same(dbp, c["want_db"].float(), "bias partials " + what)
                _same(ops.gemm_tn_ring(dy, x, sp, BF16), gc.rne_bf16(c["want"]), "bf16 slabs " + what)


def test_ring_weight_gradients_in_one_grouped_launch_are_exact(ops):
    """pswin_gemm_tn_ring_jobs through grad_queue._launch_wgrads: eight jobs of the three geometries listed in a shuffled order, f32
    and bf16 slabs, with and without bias partials, against the same expected values as the single launches."""
    from panoswintransformerobjectdetection_amd import grad_queue
    jobs, wants = [], []
    for i in gc.TN_GROUP_ORDER:
        M, N, K, sp, cls, bf, with_bias = gc.TN_GROUP[i]
        c = gc.tn_case(cls, M, N, K, sp)
        dy, x = _dev(c, "dy", "x")
        part = torch.full((sp, N, K), float("nan"), dtype=BF16 if bf else F32, device=DEV)
        dbp = torch.full((sp, N), float("nan"), dtype=F32, device=DEV) if with_bias else None
        zc = c["zero_cols"] if with_bias else (0, 0)
        jobs.append(grad_queue.WeightGrad(dy, x, part, dbp, M, N, K, sp, zc[0], zc[1]))
        wants.append((gc.rne_bf16(c["want"]) if bf else c["want"].float(), c["want_db"].float()))
    grad_queue._launch_wgrads(jobs)
    torch.cuda.synchronize()
    for j, (want, want_db) in zip(jobs, wants):
        what = f"M={j.M} N={j.N} K={j.K} splits={j.splits}"
        _same(j.partial, want, "slabs " + what)
        if j.dbias_partial is not None:
            _same(j.dbias_partial, want_db, "bias partials " + what)


# ---------------------------------------------------------------------------------------------------------------------
# the streaming kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", gc.SKINNY_KN)
def test_streaming_gemm_is_exact(ops, K, N):
    """pswin_gemm_skinny for its six shapes at M in {16, 63, 64, 333} (the entry point takes any M > 0): the weight as [N, K] and,
    transposed while it is staged, as [K, N] -- the six shapes are closed under the swap, so each one is the transposed form of a
    supported Linear."""
    from panoswintransformerobjectdetection_amd import _lib
    assert _lib.load().pswin_gemm_skinny_supported(N, K) == 1
    for M in gc.STREAM_M:
        for cls in gc.NT_CLASSES:
            c = gc.nt_case(cls, M, K, N)
            x, w, b = _dev(c, "x", "w", "bias")
            for bias in ((None, b) if b is not None else (None,)):
                want = gc.rne_bf16(c["want"] + (0.0 if bias is None else c["bias"].double()))
                what = f"{cls} M={M} K={K} N={N} bias={bias is not None}"
                _same(ops.skinny_gemm(x, w, bias), want, "weight [N, K] " + what)
                _same(ops.skinny_gemm(x, w.t().contiguous(), bias, transpose_w=True), want, "weight [K, N] " + what)


@pytest.mark.parametrize("M", gc.STREAM_M)
def test_stage0_mlp_kernels_are_exact_where_the_gelu_is_saturated(ops, M):
    """pswin_fc1_gelu_fwd / _bwd and pswin_mlp0_fwd / _bwd (C = 96, hidden = 384): h, y, g, the bias gradient and EVERY workspace row --
    the column sums over the 64 (fc1_gelu_bwd: 4 waves x 16 rows) or 128 (mlp0_bwd: 8 waves) rows of each workgroup -- and the mlp0_bwd run
    without a workspace."""
    from panoswintransformerobjectdetection_amd import _lib
    lib = _lib.load()
    C, Hd = 96, 384
    c = gc.mlp_case(M, C)
    x, w1, b1, w2, dout = _dev(c, "x", "w1", "b1", "w2", "dout")
    nan16 = lambda *s: torch.full(s, float("nan"), dtype=BF16, device=DEV)
    nan32 = lambda *s: torch.full(s, float("nan"), dtype=F32, device=DEV)
    h = nan16(M, Hd)
    ops.call("pswin_fc1_gelu_fwd", x, ops.ptr(x), ops.ptr(w1), ops.ptr(b1), ops.ptr(h), M, C, Hd)
    _same(h, c["h"].to(BF16), "fc1_gelu_fwd h")
    # fc1 + GELU backward: the pre-activation recomputed, dy = dh [v > 0]
    dh = c["dh"].to(BF16).to(DEV)
    rows = lib.pswin_fc1_gelu_partial_rows(M)
    assert rows == -(-M // gc.FC1_BWD_ROWS)
    dy, db = nan16(M, Hd), nan32(Hd)
    ws = nan32(lib.pswin_fc1_gelu_workspace(Hd) // Hd, Hd)
    ops.call("pswin_fc1_gelu_bwd", x, ops.ptr(x), ops.ptr(w1), ops.ptr(b1), ops.ptr(dh), ops.ptr(dy), ops.ptr(db), ops.ptr(ws), M, C, Hd)
    _same(dy, c["dpre"].to(BF16), "fc1_gelu_bwd dy")
    _same(db, c["db1"].float(), "fc1_gelu_bwd dbias")
    _same(ws[:rows], gc.tile_sums(c["dpre"], gc.FC1_BWD_ROWS).float(), "fc1_gelu_bwd workspace rows")
    # both products in one pass
    hh, yy = nan16(M, Hd), nan16(M, C)
    ops.call("pswin_mlp0_fwd", x, ops.ptr(x), ops.ptr(w1), ops.ptr(b1), ops.ptr(w2), ops.ptr(hh), ops.ptr(yy), M, C, Hd)
    _same(hh, c["h"].to(BF16), "mlp0_fwd h")
    _same(yy, gc.rne_bf16(c["out"]), "mlp0_fwd y")
    rows = lib.pswin_mlp0_bwd_partial_rows(M)
    assert rows == -(-M // gc.MLP0_BWD_ROWS)
    g, db, ws = nan16(M, Hd), nan32(Hd), nan32(rows, Hd)
    ops.call("pswin_mlp0_bwd", x, ops.ptr(x), ops.ptr(w1), ops.ptr(b1), ops.ptr(dout), ops.ptr(w2), ops.ptr(g), ops.ptr(db), ops.ptr(ws), M, C, Hd)
    _same(g, c["dpre"].to(BF16), "mlp0_bwd g")
    _same(db, c["db1"].float(), "mlp0_bwd dbias1")
    _same(ws, gc.tile_sums(c["dpre"], gc.MLP0_BWD_ROWS).float(), "mlp0_bwd workspace rows")
    g2 = nan16(M, Hd)
    ops.call("pswin_mlp0_bwd", x, ops.ptr(x), ops.ptr(w1), ops.ptr(b1), ops.ptr(dout), ops.ptr(w2), ops.ptr(g2), None, None, M, C, Hd)
    _same(g2, c["dpre"].to(BF16), "mlp0_bwd g without a workspace")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("N", gc.BIAS_GELU_N)
def test_bias_gelu_is_exact_where_the_gelu_is_saturated(ops, dtype, N):
    """pswin_bias_gelu_fwd / _bwd on y + bias = 16 * odd, M in {1, 5, 333}: h = relu, dy = dh [v > 0], the bias gradient and the sum of
    the workspace rows the exact integer column sums."""
    from panoswintransformerobjectdetection_amd import _lib
    lib = _lib.load()
    for M in gc.BIAS_GELU_M:
        c = gc.bias_gelu_case(M, N)
        y, b, dh = c["y"].to(dtype).to(DEV), c["b"].to(DEV), c["dh"].to(dtype).to(DEV)
        h = torch.full_like(y, float("nan"))
        ops.call("pswin_bias_gelu_fwd", y, ops.ptr(y), ops.dtype_code(y), ops.ptr(b), ops.ptr(h), M, N)
        _same(h, c["h"].to(dtype), f"h M={M}")
        dy, db = torch.full_like(y, float("nan")), torch.full((N,), float("nan"), dtype=F32, device=DEV)
        rows = lib.pswin_bias_gelu_partial_rows(M, N, ops.dtype_code(y))
        ws = torch.full((lib.pswin_bias_gelu_workspace(M, N) // N, N), float("nan"), dtype=F32, device=DEV)
        assert 1 <= rows <= ws.shape[0]
        ops.call("pswin_bias_gelu_bwd", y, ops.ptr(dh), ops.ptr(y), ops.dtype_code(y), ops.ptr(b), ops.ptr(dy), ops.ptr(db), ops.ptr(ws), M, N)
        _same(dy, c["dy"].to(dtype), f"dy M={M}")
        _same(db, c["db"].float(), f"dbias M={M}")
        _same(ws[:rows].sum(0), c["db"].float(), f"workspace rows M={M}")


# ---------------------------------------------------------------------------------------------------------------------
# the GELU itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gelu_over_every_finite_bf16_value_against_float64(ops, dtype):
    """pswin_bias_gelu_fwd / _bwd on all 65 280 finite bf16 values ([8160, 8], zero bias, dh = 1) against float64 v Phi(v) and its
    derivative, for |v| < 1e18.  f32: |h - ref| <= 5e-7 |v| + 2^-23 |ref|, |g - ref| <= 5.4e-7 -- twice the maxima of the float32 CPU
    model of csrc/pswin_gelu.hpp (tests/test_gemm_exact.py), the factor for the hardware reciprocal and exp2.  bf16 results: plus one
    bf16 rounding, 2^-8 |ref|, and no less than 2^-134, half a step of the bf16 subnormals (|ref| < 2^-126 has no relative bound: the
    correctly rounded gelu(3 * 2^-133) is off by a third).  The measured maxima and their ratio to the model's are recorded."""
    v = gc.all_finite_bf16()
    y = v.view(8160, 8).to(dtype).to(DEV)
    zero, one = torch.zeros(8, device=DEV), torch.ones_like(y)
    h, g = torch.full_like(y, float("nan")), torch.full_like(y, float("nan"))
    ws = torch.empty(ops._lib.load().pswin_bias_gelu_workspace(8160, 8), dtype=F32, device=DEV)
    ops.call("pswin_bias_gelu_fwd", y, ops.ptr(y), ops.dtype_code(y), ops.ptr(zero), ops.ptr(h), 8160, 8)
    ops.call("pswin_bias_gelu_bwd", y, ops.ptr(one), ops.ptr(y), ops.dtype_code(y), ops.ptr(zero), ops.ptr(g), None, ops.ptr(ws), 8160, 8)
    h, g = h.float().cpu().reshape(-1), g.float().cpu().reshape(-1)
    ref, refg = gc.gelu_ref64(v)
    ok = v.double().abs() < gc.GELU_SWEEP_LIMIT
    lowp = dtype == BF16
    round16 = torch.clamp(2.0 ** -8 * ref.abs(), min=2.0 ** -134) if lowp else 0.0
    round16g = 2.0 ** -8 * refg.abs() if lowp else 0.0
    eh, eg = (h.double() - ref).abs(), (g.double() - refg).abs()
    bh = gc.GELU_FWD_REL * v.double().abs() + 2.0 ** -23 * ref.abs() + round16
    bg = gc.GELU_GRAD_ABS + round16g
    fwd, grad = gc.gelu_errors(h, g, v)
    mf, mg = gc.gelu_errors(*gc.gelu_model_f32(v), v)
    worst_h, worst_g = int((eh - bh)[ok].argmax()), int((eg - bg)[ok].argmax())
    print(f"gelu sweep {dtype}: max |h - ref| / |v| = {fwd:.4g} (model {mf:.4g}), max |g - ref| = {grad:.4g} (model {mg:.4g}); "
          f"nearest the bound: h at v = {float(v[ok][worst_h])!r}, g at v = {float(v[ok][worst_g])!r}")
    over = dict(fwd_err_over_bound=float((eh / bh)[ok & (v != 0)].max()), grad_err_over_bound=float((eg / bg)[ok].max()))
    if lowp:                                             # dominated by the bf16 rounding of the result: only the distance to the bound
        record("gelu_sweep_bf16", **over)
    else:
        record("gelu_sweep_f32", fwd_err_over_abs_v=fwd, grad_abs_err=grad, model_fwd=mf, model_grad=mg, fwd_over_model=fwd / mf,
               grad_over_model=grad / mg, **over)
    assert bool(torch.isfinite(h[ok]).all()) and bool(torch.isfinite(g[ok]).all())
    assert bool((eh <= bh)[ok].all()), (float(v[ok][worst_h]), float(eh[ok][worst_h]), float(bh[ok][worst_h]))
    assert bool((eg <= bg)[ok].all()), (float(v[ok][worst_g]), float(eg[ok][worst_g]), float(bg[ok][worst_g]))
