"""The expectations of tests/test_attention_edges_gpu.py for the reference alone, on the CPU: before a kernel is judged against "the
selected V row", "unchanged by a row offset" or "no worse than its rounding points", the oracle itself has to meet them.

One-hot rows: the condition (the 48 unselected keys of every row hold at most 1e-20 of the weight in float64: logits spread over a few
units against a -100 mask give e^-72 at the very most) is a property of the INPUTS; then the oracle's output is v[sel], its dV the selected
dO rows and its dQ, dK vanish.  Row offsets: the float64 oracle does not see them.  Rounding model: it differs from the truth."""
import pytest
import torch

import _attn_edge_cases as ec

CORE = [c + (h, p) for c in ec.CORE_ONEHOT for h in (1, 3) for p in (True, False)] + [ec.CORE_ONEHOT_LOOP + (3, True)]


@pytest.mark.parametrize("family,n_rep,nW,chunks,heads,pano", CORE)
def test_one_hot_rows_select_for_the_core_oracle(family, n_rep, nW, chunks, heads, pano):
    x, alpha, beta, dist, mask, gout, sel, kind = ec.core_onehot_case(family, n_rep, nW, heads, pano, False)
    C, n = heads * 32, n_rep * nW
    qkv = x.view(n, 49, 3, C)
    _, p = ec.attention64(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], 32 ** -0.5, ec.core_bias(alpha, beta, dist, heads, n_rep), mask, heads)
    rest, single = ec.unselected_weight(p, sel)
    print(f"unselected weight of a row <= {rest:.3e}, of a key <= {single:.3e}")
    assert rest <= 1e-20
    assert single < 2.0 ** -134                                  # rounds to bf16 zero (half the smallest bf16 subnormal)
    rows = ec.selected_rows(sel, n)
    om = ec.oracle_mask(mask, kind, n_rep, nW)
    for dt, tol in ((torch.float64, 1e-15), (torch.float32, 1e-6)):
        c = lambda t: None if t is None else t.to(dt)
        out, dx, _, _ = ec._attn_oracle(c(x), c(alpha), c(beta), c(dist), om, c(gout), heads, n_rep, nW)
        v = c(x)[:, 2 * C:]
        assert ((out - v[rows]).abs() <= tol * v[rows].abs()).all()
        dv_exp = torch.zeros(n * 49, C, dtype=dt).index_add_(0, rows, c(gout))
        assert torch.allclose(dx[:, 2 * C:], dv_exp, rtol=10 * tol, atol=10 * tol)
        if family != "column":
            assert torch.allclose(dx[:, 2 * C:][rows], c(gout), rtol=tol, atol=0)
        if dt == torch.float64:
            assert dx[:, :2 * C].abs().max().item() < 1e-18


@pytest.mark.parametrize("C", [96, 192, 384])
@pytest.mark.parametrize("family,B,nW,pano", ec.FUSED_ONEHOT)
def test_one_hot_rows_select_for_the_oracle_module(family, B, nW, pano, C):
    att, x, uv, mask, gout, sel, kind = ec.fused_onehot_case(family, B, nW, pano, C)
    n = B * nW
    o, y, p = ec.fused_model(att, x, uv, mask, pano, B)
    rest, single = ec.unselected_weight(p, sel)
    print(f"unselected weight of a row <= {rest:.3e}, of a key <= {single:.3e}")
    assert rest <= 1e-20
    rows = ec.selected_rows(sel, n)
    v64 = ec.fused_v64(att, x)
    assert ((o - v64[rows]).abs() <= 1e-15 * v64[rows].abs()).all()
    yo, dx, grads = ec.module_oracle(att, x, uv, ec.oracle_mask(mask, kind, B, nW), pano, gout, B)
    y64 = v64[rows] @ att.proj.weight.double().T
    assert torch.allclose(yo.reshape(-1, C), y64, rtol=1e-12, atol=1e-13)
    assert torch.allclose(y, y64, rtol=1e-12, atol=1e-13)
    gw, gb = grads["qkv.weight"], grads["qkv.bias"]
    assert gw[:2 * C].abs().max().item() < 1e-18 and gb[:2 * C].abs().max().item() < 1e-18
    assert gw[2 * C:].abs().max().item() > 0.1
    # float32: the module the GPU tests' gradients are compared with selects as well
    with torch.no_grad():
        y32 = att(x, uv.repeat(B, 1, 1), ec.oracle_mask(mask, kind, B, nW), pano) - att.proj.bias
    assert torch.allclose(y32.reshape(-1, C).double(), y64, rtol=1e-4, atol=1e-5 * y64.abs().max().item())


@pytest.mark.parametrize("n_rep,nW,heads,pano,mask_kind", ec.CORE_RANDOM)
def test_row_offsets_do_not_change_the_core_oracle(n_rep, nW, heads, pano, mask_kind):
    x, alpha, beta, dist, mask, gout = ec._attn_case(n_rep, nW, heads, pano, mask_kind, f"{n_rep}{nW}{heads}")
    d = lambda t: None if t is None else t.double()
    off = ec.row_offset_mask(mask, nW)
    assert off.max().item() >= 100.0 and off.min().item() <= -100.0
    a = ec._attn_oracle(d(x), d(alpha), d(beta), d(dist), mask, d(gout), heads, n_rep, nW)
    b = ec._attn_oracle(d(x), d(alpha), d(beta), d(dist), off, d(gout), heads, n_rep, nW)
    for s, t in zip(a, b):
        if s is not None:
            assert torch.allclose(t, s, rtol=1e-12, atol=1e-12 * s.abs().max().item())


@pytest.mark.parametrize("C,B,nW,pano,mask_kind", ec.FUSED_RANDOM)
def test_row_offsets_do_not_change_the_oracle_module(C, B, nW, pano, mask_kind):
    seed = f"{B}{nW}{pano}{mask_kind}" if C == 96 else f"q{C}{B}{nW}{pano}{mask_kind}"
    att, x, uv, mask, gout = ec._fused_case(B, nW, pano, mask_kind, seed, C)
    y0, dx0, g0 = ec.module_oracle(att, x, uv, mask, pano, gout, B)
    y1, dx1, g1 = ec.module_oracle(att, x, uv, ec.row_offset_mask(mask, nW), pano, gout, B)
    assert torch.allclose(y1, y0, rtol=1e-12, atol=1e-12 * y0.abs().max().item())
    assert torch.allclose(dx1, dx0, rtol=1e-12, atol=1e-12 * dx0.abs().max().item())
    assert g1.keys() == g0.keys()
    for k in g0:
        assert torch.allclose(g1[k], g0[k], rtol=1e-12, atol=1e-12 * g0[k].abs().max().item()), k


@pytest.mark.parametrize("n_rep,nW,heads,pano,mask_kind", ec.CORE_RANDOM[:2])
def test_the_core_rounding_model_differs_from_the_truth(n_rep, nW, heads, pano, mask_kind):
    x, alpha, beta, dist, mask, gout = ec._attn_case(n_rep, nW, heads, pano, mask_kind, f"{n_rep}{nW}{heads}")
    x = x.to(torch.bfloat16).float()
    C, n = heads * 32, n_rep * nW
    qkv = x.view(n, 49, 3, C)
    bias = ec.core_bias(alpha, beta, dist, heads, n_rep)
    t, _ = ec.attention64(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], 32 ** -0.5, bias, mask, heads)
    e, _ = ec.attention64(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], 32 ** -0.5, bias, mask, heads, ec.bf16_round)
    d = lambda v: None if v is None else v.double()
    ref = ec._attn_oracle(d(x), d(alpha), d(beta), d(dist), mask, d(gout), heads, n_rep, nW)[0]
    assert torch.allclose(t.reshape(-1, C), ref, rtol=1e-12, atol=1e-13)          # attention64 without roundings IS the oracle
    _, rms, _, mx = ec.err_stats(t, e, t)
    print(f"rms(E - T) = {rms:.3e}, max|E - T| = {mx:.3e}, max|T| = {t.abs().max().item():.3e}")
    assert rms > 0
    assert mx <= 2.0 ** -7 * t.abs().max().item()            # and by no more than bf16 roundings can explain


@pytest.mark.parametrize("C,B,nW,pano,mask_kind", ec.FUSED_MODEL)
def test_the_fused_rounding_model_differs_from_the_truth(C, B, nW, pano, mask_kind):
    seed = f"{B}{nW}{pano}{mask_kind}" if C == 96 else f"q{C}{B}{nW}{pano}{mask_kind}"
    att, x, uv, mask, gout = ec._fused_case(B, nW, pano, mask_kind, seed, C)
    ot, yt, _ = ec.fused_model(att, x, uv, mask, pano, B)
    oe, ye, _ = ec.fused_model(att, x, uv, mask, pano, B, ec.bf16_round)
    yo, _, _ = ec.module_oracle(att, x, uv, mask, pano, gout, B)
    assert torch.allclose(yt, yo.reshape(-1, C), rtol=1e-12, atol=1e-13)          # fused_model without roundings IS the oracle module
    for name, t, e in (("attention rows", ot, oe), ("proj output", yt, ye)):
        _, rms, _, mx = ec.err_stats(t, e, t)
        print(f"{name}: rms(E - T) = {rms:.3e}, max|E - T| = {mx:.3e}, max|T| = {t.abs().max().item():.3e}")
        assert rms > 0
