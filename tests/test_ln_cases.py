"""tests/_ln_cases.py checked on the CPU before anything goes to a GPU: the conditions the exact assertions rest on, the hand-written float64
definition against torch.nn.functional.layer_norm and autograd in float64 on every row mover, the float32 mirror of the kernels' formulas
inside every bound at every case (the bounds are not too tight), and the same mirror with one planted defect at a time outside a bound
or breaking an exact assertion, at C = 96 and C = 768 (they are not too loose).  The last test prints which assertion caught each defect."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _ln_cases as L

N_SLOTS = 196                    # 9 x 11 tokens in 7 x 7 windows
S_WIN = L.WINDOW_HW[0] * L.WINDOW_HW[1]


def _maps(C):
    return L.synthetic_map(S_WIN, N_SLOTS, C), L.synthetic_map(S_WIN, N_SLOTS, C + 1)


def _all_cases():
    out = {}
    for C in L.WIDTHS:
        wmap, omap = _maps(C)
        for i, S in enumerate(L.token_counts(C)):
            out.update({f"gather-C{C}-S{S}-{k}": c for k, c in L.gather_variants(C, S, i).items()})
        out.update({f"gather-C{C}-{k}": c for k, c in L.gather_variants(C, S_WIN, 4, wmap).items()})
        out.update({f"scatter-C{C}-{k}": c for k, c in L.scatter_variants(C, S_WIN, 5, wmap, omap).items()})
        if L.nchw_supported(L.NCHW_HW[0] * L.NCHW_HW[1], C):
            out.update({f"nchw-C{C}-{k}": c for k, c in L.nchw_variants(C, 6).items()})
    out.update({f"merge-C{C4}": L.merge_case(C4, 7) for C4 in L.MERGE_WIDTHS})
    C, rows = 96, L.BWD_MAX_BLOCKS * L.rpb(96) * 5 // 2                      # one case beyond one sweep of the backward grid
    out[f"gather-C{C}-sweeps"] = L.Case("gather", C, 2, rows // 2, 8, shortcut=True, res=True, extra=L.sweep_seams(rows, C))
    return out


CASES = _all_cases()


@functools.lru_cache(maxsize=4)
def _ref(name):
    return CASES[name].reference()


def test_launch_arithmetic():
    assert [L.pick_lanes(C) for C in (32, 64, 96, 104, 192, 384, 768, 1024, 1536)] == [2, 4, 8, 8, 16, 32, 64, 64, 64]
    assert [L.lane_chunks(C) for C in (32, 64, 96, 104, 192, 384, 768, 1024, 1536)] == [4, 4, 3, 4, 3, 3, 3, 4, 6]
    assert [C for C in range(8, 2049, 8) if L.exact_rows(C)] == list(L.EXACT_WIDTHS)
    assert L.chunk_slots(1536) == 8 and L.chunk_slots(104) == 4 and L.chunk_slots(96) == 3 and L.chunk_slots(64, True) == 4
    assert L.bwd_blocks(10 ** 6, 96) == 1024 and L.bwd_blocks(65, 96) == 3
    assert all(L.nchw_supported(128, C) for C in L.WIDTHS)
    assert len(L.DEFECTS) == 12 and len(CASES) > 150


@pytest.mark.parametrize("name", list(CASES))
def test_conditions_of_the_exact_assertions(name):
    c = CASES[name]
    assert not c.conditions()
    for m in (c.wmap, c.in_map, c.out_map):
        if m is not None:
            assert int((m >= 0).sum()) == c.S and torch.equal(m[L.invert(m, c.S)], torch.arange(c.S))
    x = c.ln_input()
    kinds = {k: x[row] for row, k in c.plan.items()}
    if c.win is None and c.kind != "merge" and c.xdt == L.F32:
        for row, k in c.plan.items():
            v = x[row].double()
            if k in ("const13", "const37", "zeros"):
                assert float(v.var(unbiased=False)) == 0.0
            if k in ("mean30", "mean1000"):
                assert abs(float(v.mean())) > (25 if k == "mean30" else 800) * float(v.std())
            if k == "tiny":
                assert float(v.var()) < 1e-3 * L.EPS
    assert kinds
    assert float(c.gamma[1]) == 0.0 and float(c.gamma[2]) == 16.0 and int((c.gamma < 0).sum()) >= 2


def _soft_slots(t, wmap):
    if wmap is None:
        return t
    return t[:, wmap.clamp(min=0)] * (wmap >= 0).double()[None, :, None]


@pytest.mark.parametrize("name", [n for n in CASES if "sweeps" not in n and ("-S" not in n or "C104" in n or "C96" in n)])
def test_definition_is_layer_norm_in_float64(name):
    """Case.reference() against F.layer_norm in float64 with autograd through the same row movers, to 5e-8 of the largest value"""
    c = CASES[name]
    want, _ = _ref(name)
    B, S, C = c.B, c.S, c.C
    leaf = lambda t: None if t is None else t.double().clone().requires_grad_(True)
    x, gamma, beta, win, add = leaf(c.x), leaf(c.gamma), leaf(c.beta), leaf(c.win), leaf(c.add)
    x1 = x
    if win is not None:
        br = win if c.in_map is None else win[:, L.invert(c.in_map, S)]
        br = br if c.bias is None else br + c.bias.double()
        br = br if c.scale is None else br * c.scale.double()[:, None, None]
        x1 = x + br
        exact = x1.detach()
        # LayerNorm is stated on the float32 x1 the operator returns (and saves for its backward pass): the same point, same gradient
        x1 = x1 + (c.ln_input().view(B, S, C).double() - exact).detach()
    rows = L.merge(x1, c.H, c.W) if c.kind == "merge" else x1
    y = F.layer_norm(rows, (C,), gamma, beta, L.EPS32)
    if add is not None:
        y = y + add
    y = L.nchw(y, c.H, c.W) if c.kind == "nchw" else _soft_slots(y, c.wmap if c.kind == "gather" else c.out_map)
    loss = (y * c.dy.double()).sum()
    if c.dres is not None:
        loss = loss + (x1 * c.dres.double()).sum()
    loss.backward()
    got = dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, mean=rows.detach().mean(-1),
               rstd=1.0 / torch.sqrt(rows.detach().var(-1, unbiased=False) + L.EPS32))
    if win is not None:
        got["x1"], got["dwin" if c.kind == "scatter" else "dbranch"] = exact, win.grad
    if add is not None:
        got["dadd"] = add.grad
    if c.res_scale is not None:
        got["dres_sum"] = (c.dres.double() * c.res_scale.double()[:, None, None]).sum((0, 1))
    for k, v in got.items():
        scale = float(want[k].abs().max())
        assert v.shape == want[k].shape and float((v - want[k]).abs().max()) <= 5e-8 * scale, (k, float((v - want[k]).abs().max()), scale)


@pytest.mark.parametrize("name", list(CASES))
def test_float32_mirror_is_inside_every_bound(name):
    c = CASES[name]
    q, bad = c.judge(L.mirror(c), _ref(name))
    print(name, " ".join(f"{k}={v:.3g}" for k, v in q.items()))
    assert {"y", "mean", "rstd", "dx", "dgamma", "dbeta"} <= set(q)
    assert all(v <= 1.0 for v in q.values()), q
    assert not bad, bad


# the cases a defect is planted in, at C = 96 and C = 768 (patch merging: the merged widths of 96 and 192 input channels)
def _defect_cases(defect):
    if defect == "outside_quarters_skipped":
        return ["merge-C384", "merge-C768"]
    if defect in ("pad_beta", "stats_at_slot"):
        return [f"gather-C{C}-map_shortcut" for C in (96, 768)]
    return [f"gather-C{C}-S{L.token_counts(C)[-1]}-{'bf16x' if defect == 'bf16_truncation' else 'shortcut'}" for C in (96, 768)] + \
           ([f"scatter-C{C}-windows" for C in (96, 768)] if defect == "bf16_truncation" else [])


@pytest.mark.parametrize("defect", L.DEFECTS)
def test_a_planted_defect_is_caught(defect):
    missed = []
    for name in _defect_cases(defect):
        c = CASES[name]
        q, bad = c.judge(L.mirror(c, defect), _ref(name))
        over = {k: v for k, v in q.items() if not v <= 1.0}
        print(f"{defect:26s} {name:28s} caught by: " + "; ".join([f"bound of {k} (error / bound = {v:.3g})" for k, v in over.items()] + bad))
        if not over and not bad:
            missed.append((name, q))
    assert not missed, missed
    if defect == "bf16_truncation":             # a whole bf16 ulp is twice the bound of a bf16 output; the exact casts must notice it as well
        for name in _defect_cases(defect):
            c = CASES[name]
            _, bad = c.judge(L.mirror(c, defect), _ref(name))
            assert any("nearest-even" in b for b in bad), bad
