"""tests/_stem_exact_cases.py can tell a wrong stem kernel from a right one (CPU only): every case meets the conditions it asserts,
the float64 restatement agrees with a second formulation (autograd and the definitions), and every planted defect of the
restatement changes at least one compared output at every shape where it can apply.  The per-defect counts are printed."""
import pytest
import torch
import torch.nn.functional as F

import _stem_exact_cases as sc

SMALL = sc.SMALL_SHAPES


@pytest.mark.parametrize("B,H,W", SMALL)
@pytest.mark.parametrize("cls", ["dense", "ties"])
def test_conditions(cls, B, H, W):
    c = sc.case(cls, B, H, W)              # asserts its conditions while it builds
    print(cls, (B, H, W), {k: round(v, 4) for k, v in c.info.items()})
    for st in "ABCDE":
        for k in sc.compared(cls, st, (B, H, W)):
            assert bool(torch.isfinite(c.out[k].double()).all()), k


@pytest.mark.parametrize("B,H,W", SMALL)
def test_select_conditions(B, H, W):
    sub = sc.select_case(B, H, W)          # asserts that every compared output is a bit copy
    assert set(sub) == {"conv2", "conv3_fwd", "conv3_bwd_data", "conv3_wgrad", "conv2_wgrad"}
    tok = sub["conv3_fwd"].out["tok"]
    assert bool((tok.double() >= 0).all()) and float((tok.double() > 0).double().mean()) > 0.2
    assert float((sub["conv3_bwd_data"].out["dy2"].double() != 0).double().mean()) > 0.2


def test_thin_conditions_and_trip_counts():
    c = sc.case("thin", *sc.TRIP_SHAPE)
    n = sc.launch_counts(*sc.TRIP_SHAPE)
    assert n["tiles16"] == 270 > n["grid16"] == 256 and n["tiles8"] == 540 > n["grid8"] == 512 and n["M"] == 8640 and n["per"] == 3
    g = sc.launch_counts(*sc.GROUP_SHAPE)
    assert g["M"] == 32896 and g["groups"] == 257 > g["grid_groups"] == 256
    print("thin", sc.TRIP_SHAPE, {k: round(v, 4) for k, v in c.info.items()}, {k: v for k, v in c.out.items() if k.startswith("bound")})
    # the tiled restatement of the second-trip tiles is the plain one; with the previous trip's input window it is not
    assert torch.equal(sc._tiled_y2(c.ops, c.out["y2_exact"], 256, False), c.out["y2_exact"])
    mixed = sc.restate(c.ops, "B", mut="prefetch_mix")
    d = sc.differing(mixed["y2"], c.out["y2"]), sc.differing(mixed["sums2"], c.out["sums2"])
    print("mutant prefetch_mix", sc.TRIP_SHAPE, "thin: y2, sums2 differ in", d)
    assert d[0] > 0 and d[1] > 0


def test_group_case_conditions():
    c = sc.case_groups(*sc.GROUP_SHAPE)
    print("thin", sc.GROUP_SHAPE, c.info)
    assert c.out["dy2"].shape == (1, 64, 512, 1028) and bool(torch.isfinite(c.out["sums3"]).all())


def test_restatement_against_autograd():
    """second formulation on one small shape: weight and data gradients from torch.autograd.grad of float64 losses, the masks, sums
    and G from their definitions with explicit tap loops"""
    B, H, W = 1, 20, 36
    c = sc.case("dense", B, H, W)
    ops, out = c.ops, c.out
    x, n = ops["x"], B * H * W
    # conv1 by explicit taps
    xp = F.pad(x, (1, 1, 1, 1))
    y1 = torch.zeros(B, 32, H, W, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            y1 += torch.einsum("oc,bchw->bohw", ops["w1"][:, :, ky, kx], xp[:, :, ky:ky + H, kx:kx + W])
    assert torch.equal(y1, out["y1"])
    a1 = torch.relu(y1 * sc._ch(ops["scale1"]) + sc._ch(ops["shift1"])).requires_grad_(True)
    w2, w3 = ops["w2"].clone().requires_grad_(True), ops["w3"].clone().requires_grad_(True)
    y2 = F.conv2d(a1, w2, padding=1)
    assert torch.equal(y2.detach(), out["y2_exact"]) and torch.equal(y2.detach(), out["y2"].double())
    dw2, da1 = torch.autograd.grad((y2 * ops["dy2_in"]).sum(), (w2, a1))
    assert torch.equal(dw2, out["dw2"])
    g1 = da1 * ((y1 * sc._ch(ops["scale1"]) + sc._ch(ops["shift1"])) > 0)
    yh1 = y1 * sc._ch(ops["a1c"]) + sc._ch(ops["b1c"])
    assert torch.equal(g1.sum((0, 2, 3)), out["sg1"]) and torch.equal((g1 * yh1).sum((0, 2, 3)), out["sgy1"])
    x4p = F.pad(torch.cat([x, torch.ones(B, 1, H, W, dtype=torch.float64)], 1), (1, 1, 1, 1))
    G, XX = torch.zeros(32, 48, dtype=torch.float64), torch.zeros(48, 48, dtype=torch.float64)
    for tap in range(9):
        win = x4p[:, :, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W]
        G[:, 4 * tap:4 * tap + 4] = torch.einsum("bohw,bchw->oc", g1, win)
        for tap2 in range(9):
            win2 = x4p[:, :, tap2 // 3:tap2 // 3 + H, tap2 % 3:tap2 % 3 + W]
            XX[4 * tap:4 * tap + 4, 4 * tap2:4 * tap2 + 4] = torch.einsum("bchw,bdhw->cd", win, win2)
    assert torch.equal(G, out["G"])                       # g1 fits bf16 in `dense`
    assert torch.equal(torch.cat([y1.sum((0, 2, 3)), (y1 * y1).sum((0, 2, 3)), XX.reshape(-1)]), out["sums1"])
    assert float(XX[19, 19]) == n
    # conv3 and its gradients
    y2b = out["y2"].double()
    z2 = y2b * sc._ch(ops["scale2"]) + sc._ch(ops["shift2"])
    a2 = torch.relu(z2).requires_grad_(True)
    tok = (F.conv2d(a2, w3, stride=4) + sc._ch(ops["bias3"])).permute(0, 2, 3, 1).reshape(-1, 96)
    assert torch.equal(tok.detach(), out["tok_exact"])
    dw3, da2 = torch.autograd.grad((tok * ops["dtok"]).sum(), (w3, a2))
    assert torch.equal(dw3, out["dw3"])
    g2 = da2 * (z2 > 0)
    sg, sgy = g2.sum((0, 2, 3)), (g2 * (y2b * sc._ch(ops["a2c"]) + sc._ch(ops["b2c"]))).sum((0, 2, 3))
    assert torch.equal(torch.cat([sg, sgy]), out["sums3"])
    dy2 = sc._ch(ops["k1"]) * g2 - sc._ch(ops["P"]) * y2b - sc._ch(ops["Q"])
    assert torch.equal(dy2, out["dy2"].double())


def _mutant_count(cls, shape, mut):
    c = sc.case(cls, *shape)
    ops = dict(c.ops, y2=c.out["y2"].double())
    stages = sc.MUTANT_STAGES[mut]
    got = sc.restate(ops if set(stages) <= set("CD") else c.ops, stages, mut=mut, sums=cls != "ties")
    return sum(sc.differing(got[k], c.out[k]) for st in stages for k in sc.compared(cls, st, shape))


def _applies(mut, shape):
    n = sc.launch_counts(*shape)
    if mut == "drop_tail":
        return n["M"] % 16 != 0
    if mut == "prefetch_mix":
        return n["tiles16"] > n["grid16"]
    if mut == "sums2_rounded":
        return shape[0] * shape[1] * shape[2] <= 4096       # where `ties` still compares an exact statistic of a y2 that rounds
    return True


@pytest.mark.parametrize("mut", [m for m in sc.MUTANTS if m != "prefetch_mix"])       # (prefetch_mix: test_thin_conditions_and_trip_counts)
def test_mutants_are_seen(mut):
    for shape in SMALL:
        if not _applies(mut, shape):
            continue
        counts = {cls: _mutant_count(cls, shape, mut) for cls in ("dense", "ties")}
        print("mutant", mut, shape, counts)
        assert sum(counts.values()) > 0, (mut, shape)
    assert any(_applies(mut, s) for s in SMALL)
