"""tests/_optim_cases.py checked on the CPU before anything goes to a GPU: every operand class meets its own conditions, every f32
constant is safe against the device's pow, the float32 mirror lies inside every derived bound of the float64 definition (and, on the
training class, inside the tolerance the older tests grant torch.optim.AdamW), every planted defect changes a bit on a class other than
`training`, and the record model is optim.scheduled_lr / mmcv_lr."""
import functools
import math

import numpy as np
import pytest
import torch

import _optim_cases as O
from test_lr_schedule import mmcv_lr

F = np.float32
N = 4 * 9216                     # 9216 granules: every tie exponent, every combination of the extremes, runs of 257 granules
LR_MULTS = [a for a, _ in O.GROUP_MULTS]
DECAY_MULTS = [b for _, b in O.GROUP_MULTS]
COEF = F(0.37)
OLD_RTOL, OLD_ATOL = 2e-6, 2e-7  # tests/test_kernels_gpu.py, test_optim_schedule_gpu.py, test_kernel_trips_gpu.py


def _t_of(name):
    return 2 if name == "eps_regime" else 10


@functools.lru_cache(maxsize=None)
def _setup(name, warm=True):
    """a class on the scheduled, grouped path: eight groups in runs of 3 granules, a clip coefficient that is no power of two"""
    h = O.hyper(name)
    p, g, m, v = O.operands(name, 0, N, warm=warm)
    for a in (p, g, m, v):
        a.setflags(write=False)
    return h, (p, g, m, v), O.group_lrs(h["lr"]), O.group_map(N // 4, 3)


def _mirror(name, defect=None, t=None, warm=True):
    h, ops, lrs, gmap = _setup(name, warm)
    c = O.constants(lrs, t or _t_of(name), h["b1"], h["b2"], h["eps"], h["wd"], DECAY_MULTS, LR_MULTS, defect=defect)
    return O.mirror_update(*ops, c, group_of=gmap, coef=COEF, defect=defect)


def _definition(name, t=None, warm=True):
    h, ops, lrs, gmap = _setup(name, warm)
    return O.definition(*ops, lrs, t or _t_of(name), h["b1"], h["b2"], h["eps"], h["wd"], DECAY_MULTS, gmap, coef=float(COEF))


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("name", O.CLASSES)
def test_every_class_meets_its_conditions(name, warm):
    for n in (4, 1024, 1028, N):
        p, g, m, v = O.operands(name, 3, n, warm=warm)
        for t in ((1, 2) if name == "eps_regime" else (1, 10)):
            rep = O.check_class(name, p, g, m, v, t)
        print(name, "warm" if warm else "cold", n, " ".join(f"{k}={x:.3f}" for k, x in rep.items()))
    if name == "training":
        assert bool(m.any()) == warm and bool(v.any()) == warm


def test_every_constant_is_safe_against_the_device_pow():
    """no f32 constant of a launch the GPU tests make moves when pow is off by 16 double ulps; a t that fails would be replaced"""
    used = []
    for h in (O.RECIPE, dict(O.RECIPE, wd=0.0)):
        for lrs in (O.group_lrs(h["lr"]), O.group_lrs(h["lr"], ((1.0, 1.0),)), O.group_lrs(1e-3), O.group_lrs(1e-2)):
            for t in O.T_VALUES + (3, 4, 5, 6, 11, 12, 13, 14):
                safe = O.safe_t(t, lrs, h["b1"], h["b2"], h["eps"], h["wd"], DECAY_MULTS)
                used.append((t, safe))
    moved = sorted({x for x in used if x[0] != x[1]})
    print("t replaced:", moved or "none")
    assert not moved                                         # T_VALUES are used as they are: a replacement has to be made there


WORST = {}                       # quantity -> (largest measured / bound so far, where)


@pytest.mark.parametrize("name", O.CLASSES)
def test_the_mirror_is_adamw_within_every_derived_bound(name):
    for warm in (False, True):
        for t in ((1, 2) if name == "eps_regime" else (1, 10, 6931)):
            r = _definition(name, t, warm)
            q = O.ratios(_mirror(name, None, t, warm), r, O.bounds(r))
            print(f"mirror/bound {name} {'warm' if warm else 'cold'} t={t}", " ".join(f"{k}={x:.3g}" for k, x in q.items()),
                  f"overflow={int(r.overflow.sum())}")
            assert all(x <= 1.0 for x in q.values()), (name, warm, t, q)
            for k, x in q.items():
                if x > WORST.get(k, (-1.0, ""))[0]:
                    WORST[k] = (x, f"{name} {'warm' if warm else 'cold'} t={t}")
            if name == "isolate_step":                       # no weight to hide behind: the bound is relative to the step
                tol = O.bounds(r)
                live = r.S != 0
                rel = tol["p"][live] / np.abs(r.S[live])     # about 20 roundings of the step; more only where m nearly cancels
                print(f"  bound / |step|: median {float(np.median(rel)):.3g} max {float(rel.max()):.3g}")
                assert float(np.median(rel)) < 40 * O.U


def test_largest_mirror_ratio_over_all_classes():
    """the one line the documents quote: the largest measured / bound of every quantity over all classes, states and step counts"""
    WORST.clear()
    for name in O.CLASSES:
        test_the_mirror_is_adamw_within_every_derived_bound(name)
    print("largest mirror/bound over all classes:", " ".join(f"{k}={x:.3f} ({w})" for k, (x, w) in WORST.items()))
    assert set(WORST) == {"p", "m", "v", "shadow"} and all(x <= 1.0 for x, _ in WORST.values())


def test_the_mirror_is_torch_adamw_within_the_older_tolerance():
    """five chained steps of the plain path on `training` against torch.optim.AdamW (CPU, float32) at the older tests' tolerance, and
    against the float64 definition's bounds: the new definition and the old one are the same optimizer"""
    h = O.RECIPE
    p, g, m, v = O.operands("training", 5, 4 * 4099)
    ref = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.AdamW([ref], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    for t in range(1, 6):
        g = O.operands("training", 5 + t, p.size)[1]
        out = O.mirror_update(p, g, m, v, O.constants(h["lr"], t, h["b1"], h["b2"], h["eps"], h["wd"]))
        ref.grad = torch.from_numpy(g.copy())
        opt.step()
        got, want = torch.from_numpy(out["p"]), ref.detach()
        print(f"step {t}: mirror - torch {float((got - want).abs().max()):.3g}")
        assert torch.allclose(got, want, rtol=OLD_RTOL, atol=OLD_ATOL)
        st = opt.state[ref]
        # m: gam(4) W1 |g - m| + U |m| with |g|, |m| < 6e-3;  v: gam(8) v (_optim_cases.bounds), torch's own roundings as many again
        assert torch.allclose(torch.from_numpy(out["m"]), st["exp_avg"], rtol=2 * O.U, atol=8 * O.U * 0.1 * 1.2e-2)
        assert torch.allclose(torch.from_numpy(out["v"]), st["exp_avg_sq"], rtol=16 * O.U, atol=0)
        p, m, v = out["p"], out["m"], out["v"]


def _changed(a, b):
    return {k: O.same_bits(a[k], b[k])[0] for k in ("p", "m", "v", "shadow", "g")}


@pytest.mark.parametrize("defect", O.UPDATE_DEFECTS)
def test_a_defective_update_changes_a_bit(defect):
    seen = {}
    for name in O.CLASSES:
        for warm in (False, True):
            d = _changed(_mirror(name, defect, warm=warm), _mirror(name, None, warm=warm))
            if any(d.values()):
                seen[f"{name}/{'warm' if warm else 'cold'}"] = {k: x for k, x in d.items() if x}
    print(defect, "seen by", seen)
    classes = {k.split("/")[0] for k in seen}
    assert classes and classes != {"training"}, (defect, seen)


def test_which_defects_the_older_tolerance_lets_through():
    """the parameter of a defective mirror against the definition at rtol 2e-6, atol 2e-7, which is all the older tests ask of it"""
    r = _definition("training")
    passed = []
    for defect in O.UPDATE_DEFECTS:
        got = _mirror("training", defect)["p"].astype(np.float64)
        with np.errstate(all="ignore"):
            ok = bool((np.abs(got - r.p) <= OLD_ATOL + OLD_RTOL * np.abs(r.p)).all())
        if ok:
            passed.append(defect)
    print("the older tolerance on `training` lets through:", passed)
    print("and catches:", [d for d in O.UPDATE_DEFECTS if d not in passed])
    # decay after the step moves p by lr wd |step| <= 5e-6 x 2e-4: far inside atol.  (The eps placement shows on `training` only
    # through the elements whose gradient was tiny or zero in every warm-up step, about one in a thousand.)
    assert "decay_after_step" in passed
    older = _older_operands()
    print("and on the older tests' own operands (randn weights and gradients, lr 1e-2, t = 1):", older)
    assert "betas_f32" in older and "w2_gg" in older and "no_lerp" in older


def _older_operands():
    rng = np.random.default_rng(11)
    n = 4 * 20000
    p, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    z = np.zeros(n, dtype=np.float32)
    h = dict(O.RECIPE, lr=1e-2)
    r = O.definition(p, g, z, z, h["lr"], 1, h["b1"], h["b2"], h["eps"], h["wd"])
    passed = []
    for defect in ("decay_after_step", "eps_inside", "betas_f32", "no_lerp", "w2_gg", "bias_t_minus_1"):
        got = O.mirror_update(p, g, z, z, O.constants(h["lr"], 1, h["b1"], h["b2"], h["eps"], h["wd"], defect=defect), defect=defect)
        with np.errstate(all="ignore"):
            if bool((np.abs(got["p"].astype(np.float64) - r.p) <= OLD_ATOL + OLD_RTOL * np.abs(r.p)).all()):
                passed.append(defect)
    return passed


@pytest.mark.parametrize("defect", O.SUMSQ_DEFECTS)
def test_a_defective_partial_range_changes_a_partial(defect):
    for n4 in O.SUMSQ_N4[:4] + (5 * 1024 + 3,):
        g = O.integer_gradient(n4, 4 * n4)
        g[3::4] = np.where(g[3::4] == 0, F(1.0), g[3::4])    # no granule sums to 0: its loss or doubling shows
        diff = int((O.partial_sums(g, defect) != O.partial_sums(g)).sum())
        print(defect, f"n4={n4}: {diff} partials differ")
        assert diff >= 1 or (defect == "partial_overlap" and n4 == 1)           # one granule has no neighbour to run into
    ranges = O.partial_ranges(1025)
    assert ranges[0] == (0, 2) and ranges[512] == (1024, 1025) and ranges[513] == (1025, 1025) and ranges[1023] == (1025, 1025)
    for n4 in O.SUMSQ_N4:                                    # the ranges tile [0, n4) in order
        rs = O.partial_ranges(n4)
        assert rs[0][0] == 0 and max(hi for _, hi in rs) == n4 and all(a[1] == b[0] or b[0] == n4 for a, b in zip(rs, rs[1:]))


def test_defective_records_differ_where_it_matters():
    sched = _parse(O.FIXED)
    base = dict(sched=sched, lr=1e-4, lr_mults=None, skip_nonfinite=True, step=4, iteration=9, skipped=1)
    # a norm beyond the f32 maximum: the guard must decide on the double
    big = O.record_model(4.0 * 3e38 ** 2, max_norm=1.0, **base)
    bad = O.record_model(4.0 * 3e38 ** 2, max_norm=1.0, defect="guard_on_norm_f", **base)
    assert big["applied"] == 1 and np.isinf(big["norm_f"]) and 0 < big["coef"] < 1e-38 and bad["applied"] == 0
    assert big["step_after"] == 5 and bad["step_after"] == 4 and bad["skipped_after"] == 2
    # the 1e-6 of clip_grad_norm_ decides whether max_norm == norm clips
    a = O.record_model(0.5 ** 2, max_norm=0.5, **base)
    b = O.record_model(0.5 ** 2, max_norm=0.5, defect="coef_no_1e6", **base)
    assert a["coef"] == F(0.5 / (0.5 + 1e-6)) and a["coef"] < 1 and b["coef"] == 1
    print("coef_no_1e6 seen by record/max_norm=norm; guard_on_norm_f seen by record/norm beyond f32")
    for bad_sum in (math.inf, math.nan):
        r = O.record_model(bad_sum, max_norm=1.0, **base)
        assert r["applied"] == 0 and r["t"] == 4 and r["skipped_after"] == 2 and r["iteration_after"] == 10
    assert O.record_model(math.nan, max_norm=1.0, **dict(base, skip_nonfinite=False))["coef"] != \
        O.record_model(math.nan, max_norm=1.0, **dict(base, skip_nonfinite=False))["coef"]           # NaN, as torch's clamp gives
    assert O.record_model(math.inf, max_norm=1.0, **dict(base, skip_nonfinite=False))["coef"] == 0


def _parse(cfg, ipe=None):
    from panoswintransformerobjectdetection_amd.optim import parse_lr_config
    return parse_lr_config(cfg, ipe)


@pytest.mark.parametrize("cfg", [O.FIXED, O.SCHED_NO_POW, O.SCHED_CONSTANT, O.SCHED_POW], ids=["fixed", "no_pow", "constant", "pow"])
def test_the_record_model_is_the_schedule_for_all_eight_groups(cfg):
    from panoswintransformerobjectdetection_amd.optim import scheduled_lr
    sched = _parse(cfg)
    for i in list(range(0, 45)) + [999, 1000, 2000, 5000]:
        r = O.record_model(None, sched, 1e-4, LR_MULTS, 0.0, False, i, i, 0)
        for k, a in enumerate(LR_MULTS):
            base = 1e-4 * float(F(a))
            assert r["lr"][k] == scheduled_lr(sched, base, i) == mmcv_lr(cfg, base, i), (i, k)
        assert r["lr_base"] == F(r["lr"][0]) and r["norm"] == 0.0 and r["coef"] == 1 and r["applied"] == 1
        assert (r["t"], r["iteration"], r["iteration_after"]) == (i + 1, i, i + 1)


def test_record_sum_and_partial_bound():
    """the record's tree is exact on integers, and the bound of a partial counts the additions of the longest chain"""
    part = np.arange(1024, dtype=np.float64) ** 2
    assert O.record_sum(part) == float(part.sum())
    assert O.partial_bound(1) == pytest.approx(12 * 2.0 ** -53) and O.partial_bound(1024 * 1024 + 1024) == pytest.approx(28 * 2.0 ** -53)
    g = (np.random.default_rng(1).standard_normal(4 * 5000) * 1e3).astype(np.float32)
    a, b = O.partial_sums(g), O.partial_sums(g, exact=True)
    assert (np.abs(a - b) <= O.partial_bound(5000) * b).all()
