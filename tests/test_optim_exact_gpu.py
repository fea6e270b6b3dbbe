"""csrc/pswin_optim.hip bit for bit: the AdamW update kernels (plain, grouped, scheduled, scheduled and grouped) and the bf16 shadow against
the float32 mirror of tests/_optim_cases.py, pswin_grad_sumsq's 1024 partials against the documented ranges, pswin_adamw_record against
its model in Python doubles, the non-finite guard at the elements a range or a loop could miss, and the arguments the entry points refuse.

p, m, v and the shadow are compared as bit patterns (a NaN with any NaN, see _optim_cases.same_bits).  FlatAdamW.step() drives the plain
and the scheduled path; eight groups on a bare buffer, a record with a pow in its schedule and the refused arguments go through the entry
points themselves."""
import ctypes
import functools
import math
import types

import numpy as np
import pytest
import torch

import _optim_cases as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
LR_MULTS = [a for a, _ in O.GROUP_MULTS]
DECAY_MULTS = [b for _, b in O.GROUP_MULTS]
PATHS = ("plain", "groups", "sched", "sched_groups")
ITER = 7                         # the iteration the scheduled cases run: inside SCHED_NO_POW's linear warmup
SENTINEL = 0x1234                # bf16 bits a shadow holds before the step


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)             # (a copy: the cached operands are read-only)


def _np(t):
    return t.detach().cpu().numpy()


def _bits16(t):
    return None if t is None else _np(t.view(torch.int16)).view(np.uint16)


def _shadow(n, mode, p=None):
    """the bf16 buffer of a case: "16" (16-byte aligned, sentinel-filled), "nan" (NaN-filled), "8" (8- but not 16-byte aligned: all the
    header promises), "keep" (RNE of p: what a frozen group must leave), None (no shadow)"""
    if mode is None:
        return None
    if mode == "keep":
        return _dev(O.bf16_rne(p).view(np.int16)).view(torch.bfloat16)
    base = torch.full((n + 4,), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    if mode == "nan":
        base.fill_(float("nan"))
    s = base[4:] if mode == "8" else base[:n]
    assert s.data_ptr() % 16 == (8 if mode == "8" else 0)
    return s


@functools.lru_cache(maxsize=8)
def _operands(name, n, warm=False, seed=0):
    ops = O.operands(name, seed, n, warm=warm)
    for a in ops:
        a.setflags(write=False)
    return ops


@functools.lru_cache(maxsize=None)
def _schedule(key):
    """(the host struct, optim.parse_lr_config's dict) of a schedule, built as FlatAdamW builds it"""
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    cfg = {"fixed": O.FIXED, "no_pow": O.SCHED_NO_POW, "constant": O.SCHED_CONSTANT, "pow": O.SCHED_POW}[key]
    opt = FlatAdamW(torch.nn.Parameter(torch.zeros(4, device=DEV)), lr_config=cfg)
    return opt._sched_c, opt.sched, cfg


def _record(t):
    from panoswintransformerobjectdetection_amd._lib import StepRecord
    r = StepRecord.from_buffer_copy(_np(t).tobytes())
    return types.SimpleNamespace(lr=np.array(list(r.lr), dtype=np.float64), norm=float(r.norm), lr_base=F(r.lr_base), norm_f=F(r.norm_f),
                                 coef=F(r.coef), t=F(r.t), applied=int(r.applied), iteration=int(r.iteration))


def _floats(n, x):
    return (ctypes.c_float * n)(*x)


def run(ops, h, t, path, gmap=None, shadow="16", max_norm=0.0, skip=False, sched="no_pow", iteration=ITER, steps=1, grads=None):
    """One step (or `steps` chained ones on the gradients `grads`) of a path from the state `ops` with Adam's step count preset so
    that the kernel sees t -> every buffer afterwards as numpy, the record of the last step, and the device partials."""
    from panoswintransformerobjectdetection_amd._lib import call, ptr
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    p, g, m, v = ops
    n = p.size
    sh = _shadow(n, shadow, p)
    G = _dev(g)
    out = types.SimpleNamespace(rec=None, partials=None, states=[])
    b1, b2, eps, wd, lr = h["b1"], h["b2"], h["eps"], h["wd"], h["lr"]

    def state(P, M, V, step):
        torch.cuda.synchronize()
        return dict(p=_np(P), m=_np(M), v=_np(V), g=_np(G), shadow=_bits16(sh), step=float(step))

    if path in ("plain", "sched"):
        P = torch.nn.Parameter(_dev(p))
        kw = dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        if path == "sched":
            kw.update(lr_config=_schedule(sched)[2], grad_clip=dict(max_norm=max_norm) if max_norm > 0 else None, skip_nonfinite=skip)
        opt = FlatAdamW(P, **kw)
        opt.exp_avg.copy_(_dev(m))
        opt.exp_avg_sq.copy_(_dev(v))
        opt.step_t.fill_(t - 1)
        if path == "sched":
            opt.iteration.fill_(iteration)
        opt.lowp = sh
        P.grad = G
        for s in range(steps):
            if grads is not None:
                G.copy_(_dev(grads[s]))
            opt.step()
            out.states.append(state(P.data, opt.exp_avg, opt.exp_avg_sq, opt.step_t))
            if path == "sched":
                out.rec = _record(opt._record)
                out.states[-1]["rec"] = out.rec
        if path == "sched":
            out.partials = None if opt._partials is None else _np(opt._partials)
            out.iteration, out.skipped = float(opt.iteration), float(opt.skipped)
    else:
        assert steps == 1
        P, M, V = _dev(p), _dev(m), _dev(v)
        GM = _dev(gmap)
        lr_c, dc_c = _floats(8, LR_MULTS), _floats(8, DECAY_MULTS)
        if path == "groups":
            step = torch.tensor(float(t), dtype=torch.float32, device=DEV)
            call("pswin_adamw_flat_groups", P, ptr(P), ptr(G), ptr(M), ptr(V), ptr(sh), n, ptr(GM), 8, ctypes.addressof(lr_c),
                 ctypes.addressof(dc_c), lr, b1, b2, eps, wd, ptr(step))
        else:
            step = torch.tensor(float(t - 1), dtype=torch.float32, device=DEV)
            it = torch.tensor(float(iteration), dtype=torch.float32, device=DEV)
            skipped = torch.zeros((), dtype=torch.float32, device=DEV)
            rec = torch.zeros(12, dtype=torch.float64, device=DEV)
            partials = None
            if max_norm > 0 or skip:
                partials = torch.full((O.PARTIALS,), float("nan"), dtype=torch.float64, device=DEV)
                call("pswin_grad_sumsq", G, ptr(G), n, ptr(partials))
            call("pswin_adamw_record", G, ptr(partials), ctypes.addressof(_schedule(sched)[0]), lr, 8, ctypes.addressof(lr_c), max_norm,
                 int(skip), ptr(step), ptr(it), ptr(skipped), ptr(rec))
            call("pswin_adamw_flat_sched", P, ptr(P), ptr(G), ptr(M), ptr(V), ptr(sh), n, ptr(GM), 8, ctypes.addressof(dc_c), b1, b2, eps,
                 wd, ptr(rec))
            torch.cuda.synchronize()
            out.rec = _record(rec)
            out.partials = None if partials is None else _np(partials)
            out.iteration, out.skipped = float(it), float(skipped)
        out.states.append(state(P, M, V, step))
    out.__dict__.update(out.states[-1])
    return out


def expect(ops, h, t, path, gmap=None, rec=None):
    """the mirror's step: the plain paths from the hyper-parameters, the scheduled ones from the lr, t and coefficient the record holds
    (the record itself is judged against its model by check_record)"""
    grouped = gmap is not None
    if path in ("plain", "groups"):
        lrs, coef = (O.group_lrs(h["lr"]) if grouped else h["lr"]), None
    else:
        if not rec.applied:
            p, g, m, v = ops
            return dict(p=p, g=g, m=m, v=v, shadow=None)
        lrs, coef, t = (rec.lr if grouped else rec.lr[0]), rec.coef, float(rec.t)
    dms = DECAY_MULTS if grouped else None
    assert O.safe_constants(lrs, t, h["b1"], h["b2"], h["eps"], h["wd"], dms), ("a constant of this case depends on the device's pow", t)
    return O.mirror_update(*ops, O.constants(lrs, t, h["b1"], h["b2"], h["eps"], h["wd"], dms), group_of=gmap, coef=coef)


def judge(got, want, what, keys=("p", "m", "v", "shadow", "g")):
    bad = []
    for k in keys:
        if want[k] is None or got[k] is None:
            continue
        n, i = O.same_bits(got[k], want[k])
        if n:
            bad.append(f"{k}: {n} of {want[k].size} elements differ, the first at {i}: kernel {got[k][i]!r} mirror {want[k][i]!r}")
    assert not bad, (what, bad)


def check_record(rec, out, sched, lr, lr_mults, max_norm, skip, t_before, it_before, skipped_before, sumsq, exact_lr=True, norm=None):
    """every field of the record and the three counters against the model, as bit patterns"""
    w = O.record_model(sumsq, _schedule(sched)[1], lr, lr_mults, max_norm, skip, t_before, it_before, skipped_before, norm=norm)
    d64 = lambda x: np.float64(x).view(np.int64)
    d32 = lambda x: np.float32(x).view(np.int32)
    nan = lambda a, b: math.isnan(float(a)) and math.isnan(float(b))
    assert d64(rec.norm) == d64(w["norm"]) or nan(rec.norm, w["norm"]), (rec.norm, w["norm"])
    for k in ("norm_f", "coef", "t"):
        assert d32(getattr(rec, k)) == d32(w[k]) or nan(getattr(rec, k), w[k]), (k, getattr(rec, k), w[k])
    assert (rec.applied, rec.iteration) == (w["applied"], w["iteration"])
    assert (out.step, out.iteration, out.skipped) == (float(w["step_after"]), float(w["iteration_after"]), float(w["skipped_after"]))
    for k in range(O.MAX_GROUPS):
        if exact_lr:
            assert d64(rec.lr[k]) == d64(w["lr"][k]), (k, rec.lr[k], w["lr"][k])
        else:                                               # a pow on the way: the OpenCL bound of a double pow, 16 ulps
            assert O.f64_ulps(rec.lr[k], w["lr"][k]) <= 16, (k, rec.lr[k], w["lr"][k])
    assert d32(rec.lr_base) == d32(F(rec.lr[0]))
    return w


def _clip(g, share=0.37):
    """a max_norm that clips g to about `share`"""
    return share * math.sqrt(float((g.astype(np.float64) ** 2).sum()))


def _case(name, n, path, t, warm=False, shadow="16", run_len=3, clip=True):
    """run a case twice from the same state, compare the two runs and the mirror"""
    h = O.hyper(name)
    ops = _operands(name, n, warm)
    gmap = O.group_map(n // 4, run_len) if "groups" in path else None
    max_norm = _clip(ops[1]) if clip and path.startswith("sched") and name in ("training", "isolate_step", "eps_regime") else 0.0
    a = run(ops, h, t, path, gmap, shadow, max_norm)
    b = run(ops, h, t, path, gmap, shadow, max_norm)
    what = f"{name} n={n} {path} t={t}"
    judge(b.__dict__, a.__dict__, what + ": the second run differs from the first")
    want = expect(ops, h, t, path, gmap, a.rec)
    judge(a.__dict__, want, what)
    assert a.step == t
    if a.rec is not None:
        lr_mults = LR_MULTS if gmap is not None else None
        if a.partials is None:
            assert check_record(a.rec, a, "no_pow", h["lr"], lr_mults, 0.0, False, t - 1, ITER, 0, None)["coef"] == 1
        else:                    # random gradients: the norm is the partials' sum, the coefficient comes from the RECORDED norm
            check_record(a.rec, a, "no_pow", h["lr"], lr_mults, max_norm, False, t - 1, ITER, 0, None, norm=a.rec.norm)
            # the record's own tree over the partials, then a double sqrt, which IEEE 754 rounds correctly on either side
            assert a.rec.norm == math.sqrt(O.record_sum(a.partials)) and 0 < float(a.rec.coef) < 1
    return a, want


SMALL = [(name, n, path) for name in O.CLASSES for n, paths in ((4, ("plain", "sched_groups")), (1024, ("groups", "sched")), (1028, PATHS))
         for path in paths]
MID = [(name, 4 * 100003, path) for name in O.CLASSES for path in ("plain", "sched_groups")]
BIG = [("training", O.SIZES[3], path) for path in PATHS] + [("extremes", O.SIZES[3], "groups")]
RUNS = {4: 1, 1024: 1, 1028: 3, 4 * 100003: 257, O.SIZES[3]: 1}


def _t_of(name, i):
    return (1, 2)[i % 2] if name == "eps_regime" else O.T_VALUES[i % len(O.T_VALUES)]


@pytest.mark.parametrize("i,case", list(enumerate(SMALL + MID + BIG)), ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_update_equals_the_mirror_bit_for_bit(ops, i, case):
    name, n, path = case
    _case(name, n, path, _t_of(name, i), warm=(i % 2 == 1 and n < 10 ** 6), run_len=RUNS[n])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("t", O.T_VALUES)
def test_update_at_a_preset_step_count(ops, path, t):
    _case("training", 1028, path, t, warm=True)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shadow", ["nan", None, "8"])
def test_update_with_the_shadow_nan_filled_absent_or_8_byte_aligned(ops, path, shadow):
    a, _ = _case("training", 1028, path, 10, warm=True, shadow=shadow)
    if shadow is not None:
        assert not np.isnan(O.bf16_value(a.shadow)).any()


@pytest.mark.parametrize("path", ["plain", "sched"])
def test_five_chained_steps(ops, path):
    """the kernel's own state feeds its next step, the mirror's feeds the mirror: equal after every step"""
    h = O.hyper("training")
    n = 4 * 5003
    ops0 = _operands("training", n)
    grads = [O.operands("training", 20 + s, n)[1] for s in range(5)]
    max_norm = _clip(grads[0], 0.8) if path == "sched" else 0.0           # clips some of the five steps' gradients, not all
    out = run(ops0, h, 1, path, max_norm=max_norm, steps=5, grads=grads)
    p, _, m, v = ops0
    coefs = []
    for s in range(5):
        got = out.states[s]
        want = expect((p, grads[s], m, v), h, s + 1, path, rec=got.get("rec"))
        judge(got, want, f"{path} step {s + 1}")
        p, m, v = want["p"], want["m"], want["v"]
        if path == "sched":
            assert got["rec"].t == s + 1 and got["rec"].iteration == ITER + s
            coefs.append(float(got["rec"].coef))
    print(path, "clip coefficients of the five steps:", coefs)


# ---- groups ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["groups", "sched_groups"])
@pytest.mark.parametrize("run_len", [1, 3, 257])
def test_eight_groups_and_a_frozen_one(ops, path, run_len):
    """group ids in runs of 1, 3 and 257 granules, the last granule unlike its neighbour; the (0, 0) group keeps p and the shadow"""
    h = O.hyper("training")
    n = 4 * 4099
    o = _operands("training", n, True)
    gmap = O.group_map(n // 4, run_len)
    assert gmap[-1] != gmap[-2] and len(set(gmap.tolist())) == 8
    a = run(o, h, 10, path, gmap, shadow="keep", max_norm=_clip(o[1]) if path == "sched_groups" else 0.0)
    judge(a.__dict__, expect(o, h, 10, path, gmap, a.rec), f"{path} runs of {run_len}")
    frozen = np.repeat(gmap == 1, 4)
    assert O.GROUP_MULTS[1] == (0.0, 0.0) and frozen.sum() >= 4
    assert O.same_bits(a.p[frozen], o[0][frozen])[0] == 0 and O.same_bits(a.shadow[frozen], O.bf16_rne(o[0])[frozen])[0] == 0
    live = frozen & (o[1] != 0)
    assert (a.m[live] != o[2][live]).mean() > 0.99 and (a.v[live] != o[3][live]).mean() > 0.99     # a frozen group's moments still move
    assert (a.p[~frozen] != o[0][~frozen]).mean() > 0.5


@pytest.mark.parametrize("sched,i", [("fixed", 3), ("no_pow", 0), ("no_pow", 17), ("no_pow", 39), ("no_pow", 40), ("constant", 0), ("constant", 39), ("constant", 40), ("pow", 0), ("pow", 5),
                                     ("pow", 39), ("pow", 41)])
def test_recorded_lr_of_all_eight_groups(ops, sched, i):
    """rec.lr[k] = the host's double where the schedule has no pow on the way (gamma^0, the linear and the constant warmup), within 16 double ulps
    where it has.  lr_at takes the multiplier the device takes: the f32 value."""
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    h = O.hyper("training")
    o = _operands("training", 1028)
    a = run(o, h, 3, "sched_groups", O.group_map(257, 1), sched=sched, iteration=i)
    check_record(a.rec, a, sched, h["lr"], LR_MULTS, 0.0, False, 2, i, 0, None, exact_lr=sched != "pow")
    host = FlatAdamW(torch.nn.Parameter(torch.zeros(4, device=DEV)), lr=h["lr"], lr_config=_schedule(sched)[2])
    for k, mult in enumerate(LR_MULTS):
        want = host.lr_at(i, float(F(mult)))
        assert a.rec.lr[k] == want if sched != "pow" else O.f64_ulps(a.rec.lr[k], want) <= 16, (k, a.rec.lr[k], want)
    judge(a.__dict__, expect(o, h, 3, "sched_groups", O.group_map(257, 1), a.rec), f"{sched} i={i}")


class _Odd(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        for name, k in (("a_one", 1), ("norm_three", 3), ("b_five", 5), ("table_64", 64), ("norm_65", 65), ("c_130", 130)):
            self.register_parameter(name, torch.nn.Parameter(torch.randn(k, generator=g) * 0.02))


@pytest.mark.parametrize("scheduled", [False, True], ids=["plain", "scheduled"])
def test_flattened_module_with_custom_keys(ops, scheduled):
    """GradReducer.flatten_parameters on parameters of 1, 3, 5, 64, 65 and 130 elements: the group map against one derived from the
    offsets alone, three steps against the mirror, and the alignment gaps still bit-zero in p, m, v and the shadow"""
    from panoswintransformerobjectdetection_amd.dp import GradReducer
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    h = O.hyper("training")
    keys = {"norm": dict(decay_mult=0.0), "table": dict(lr_mult=0.1, decay_mult=0.5), "c_130": dict(lr_mult=2.0, decay_mult=3.0)}
    mults = {"a_one": (1.0, 1.0), "norm_three": (1.0, 0.0), "b_five": (1.0, 1.0), "table_64": (0.1, 0.5), "norm_65": (1.0, 0.0), "c_130": (2.0, 3.0)}
    model = _Odd().to(DEV)
    red = GradReducer(model, pack=True)
    flat = red.flatten_parameters(model)
    n = flat.numel()
    kw = dict(lr_config=O.SCHED_NO_POW, grad_clip=dict(max_norm=1e-3)) if scheduled else {}
    opt = FlatAdamW(flat, lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"], model=model,
                    paramwise_cfg=dict(custom_keys=keys), prefix="", **kw)
    opt.lowp = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    # the map from the offsets alone: groups are numbered in the order the parameters introduce their pair, (1, 1) first
    pairs, gmap, gap = [(1.0, 1.0)], np.zeros(n // 4, dtype=np.uint8), np.ones(n, dtype=bool)
    for name, p in model.named_parameters():
        off = (p.data_ptr() - flat.data_ptr()) // 4
        assert off % 64 == 0 and 0 <= off and off + p.numel() <= n
        if mults[name] not in pairs:
            pairs.append(mults[name])
        gmap[off // 4:-(-(off + p.numel()) // 4)] = pairs.index(mults[name])
        gap[off:off + p.numel()] = False
    assert np.array_equal(_np(opt.group_of), gmap) and opt.group_mults == pairs and len(pairs) == 4 and gap.sum() == n - 268
    lrs = O.group_lrs(h["lr"], pairs)
    dms = [b for _, b in pairs] + [1.0] * (8 - len(pairs))
    p, m, v = _np(flat.data).copy(), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    for s in range(3):
        g = np.where(gap, F(0), O.operands("training", 40 + s, n)[1]).astype(np.float32)
        red.flat.copy_(_dev(g))
        opt.step()
        torch.cuda.synchronize()
        got = dict(p=_np(flat.data), m=_np(opt.exp_avg), v=_np(opt.exp_avg_sq), shadow=_bits16(opt.lowp), g=_np(red.flat))
        if scheduled:
            rec = _record(opt._record)
            for k, (a, _) in enumerate(pairs):
                assert rec.lr[k] == opt.lr_at(s, float(F(a)))
            assert 0 < float(rec.coef) < 1
            c = O.constants(rec.lr, float(rec.t), h["b1"], h["b2"], h["eps"], h["wd"], dms)
            want = O.mirror_update(p, g, m, v, c, group_of=gmap, coef=rec.coef)
        else:
            want = O.mirror_update(p, g, m, v, O.constants(lrs, s + 1, h["b1"], h["b2"], h["eps"], h["wd"], dms), group_of=gmap)
        judge(got, want, f"flattened module step {s + 1}")
        for k in ("p", "m", "v", "shadow"):
            assert not got[k][gap].view(np.uint32 if k != "shadow" else np.uint16).any(), k        # +0 bits, after weight decay too
        p, m, v = want["p"], want["m"], want["v"]


@functools.lru_cache(maxsize=None)
def _kernel_ratios(name):
    h = O.hyper(name)
    n = 4 * 9216
    t = 2 if name == "eps_regime" else 10
    o = _operands(name, n, True)
    gmap = O.group_map(n // 4, 3)
    a = run(o, h, t, "groups", gmap)
    r = O.definition(*o, O.group_lrs(h["lr"]), t, h["b1"], h["b2"], h["eps"], h["wd"], DECAY_MULTS, gmap)
    tol = O.bounds(r, clipped=False)
    return O.ratios(a.__dict__, r, tol), O.ratios(expect(o, h, t, "groups", gmap), r, tol)


@pytest.mark.parametrize("name", O.CLASSES)
def test_kernel_against_the_float64_definition(ops, name):
    """the kernel's own distance to the float64 definition over the derived bound, beside the mirror's (equal bits give equal figures)"""
    qk, qm = _kernel_ratios(name)
    print(f"{name}: kernel/bound", " ".join(f"{k}={x:.3g}" for k, x in qk.items()), "| mirror/bound", " ".join(f"{k}={x:.3g}" for k, x in qm.items()))
    assert all(x <= 1.0 for x in qk.values()), qk


def test_largest_kernel_ratio_over_all_classes(ops):
    """the one line the documents quote"""
    worst = {k: max((_kernel_ratios(name)[0][k], name) for name in O.CLASSES) for k in ("p", "m", "v", "shadow")}
    print("largest kernel/bound over all classes:", " ".join(f"{k}={x:.3f} ({w})" for k, (x, w) in worst.items()))
    assert all(x <= 1.0 for x, _ in worst.values())


# ---- pswin_grad_sumsq --------------------------------------------------------------------------------------------------------------
def _sumsq(g):
    from panoswintransformerobjectdetection_amd._lib import call, ptr
    G = _dev(g)
    partials = torch.full((O.PARTIALS,), float("nan"), dtype=torch.float64, device=DEV)
    call("pswin_grad_sumsq", G, ptr(G), g.size, ptr(partials))
    torch.cuda.synchronize()
    return _np(partials)


@pytest.mark.parametrize("n4", O.SUMSQ_N4)
def test_every_partial_is_its_documented_range_sum(ops, n4):
    """integer gradients: every sum is exact in double, so each of the 1024 NaN-prefilled partials must EQUAL its range's sum"""
    g = O.integer_gradient(n4, 4 * n4)
    g[-1], g[0] = F(63.0), F(-64.0)
    got, want = _sumsq(g), O.partial_sums(g)
    bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, (n4, bad[:8], got[bad[:8]], want[bad[:8]])
    assert (want[[lo == hi for lo, hi in O.partial_ranges(n4)]] == 0).all() and float(want.sum()) == float((g.astype(np.float64) ** 2).sum())


@pytest.mark.parametrize("n4", [1025, 768 * 1024 + 1])
def test_partials_of_random_gradients_within_their_additions(ops, n4):
    g = (np.random.default_rng(n4).standard_normal(4 * n4) * 1e3).astype(np.float32)
    got, want = _sumsq(g), O.partial_sums(g, exact=True)
    q = np.abs(got - want) / np.where(want > 0, O.partial_bound(n4) * want, 1.0)
    print(f"n4={n4}: worst partial error / bound {float(q.max()):.3g}")
    assert (q <= 1.0).all() and (got[want == 0].view(np.int64) == 0).all()


def test_partials_stay_finite_where_an_f32_sum_would_not(ops):
    n4 = 5 * 1024 + 3
    g = O.integer_gradient(7, 4 * n4)
    for lo, hi in O.partial_ranges(n4):
        if hi > lo:
            g[4 * lo + (lo % 4)] = F(3e38) * (F(-1) if lo % 2 else F(1))
    got, want = _sumsq(g), O.partial_sums(g, exact=True)
    assert np.isfinite(got).all() and (want[want > 0] > 8e76).all()
    assert (np.abs(got - want) <= O.partial_bound(n4) * want).all()


# ---- pswin_adamw_record ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [6, 10, 11])
def test_record_on_a_norm_that_is_exact(ops, k):
    """constant gradients c over n = 4^k elements: norm = c 2^k exactly; every field and counter against the model, as bits, for
    max_norm at, beside, below and above the norm"""
    from panoswintransformerobjectdetection_amd._lib import call, ptr
    n = 4 ** k
    lr_c = _floats(8, LR_MULTS)
    for c in (2.0 ** -7, 3 * 2.0 ** -9):
        norm = c * 2.0 ** k
        G = torch.full((n,), c, dtype=torch.float32, device=DEV)
        partials = torch.full((O.PARTIALS,), float("nan"), dtype=torch.float64, device=DEV)
        call("pswin_grad_sumsq", G, ptr(G), n, ptr(partials))
        sumsq = O.record_sum(_np(partials))
        assert sumsq == norm * norm
        edge = norm + 1e-6
        seen = set()
        for j, max_norm in enumerate((norm, edge, math.nextafter(edge, 0.0), math.nextafter(edge, math.inf), norm / 2, 2 * norm, 0.0, -1.0)):
            step = torch.tensor(float(j), dtype=torch.float32, device=DEV)
            it = torch.tensor(float(ITER + j), dtype=torch.float32, device=DEV)
            skipped = torch.tensor(2.0, dtype=torch.float32, device=DEV)
            rec = torch.zeros(12, dtype=torch.float64, device=DEV)
            call("pswin_adamw_record", G, ptr(partials), ctypes.addressof(_schedule("no_pow")[0]), 1e-4, 8, ctypes.addressof(lr_c), max_norm, 1,
                 ptr(step), ptr(it), ptr(skipped), ptr(rec))
            torch.cuda.synchronize()
            out = types.SimpleNamespace(step=float(step), iteration=float(it), skipped=float(skipped))
            w = check_record(_record(rec), out, "no_pow", 1e-4, LR_MULTS, max_norm, True, j, ITER + j, 2, sumsq)
            assert w["norm"] == norm and w["applied"] == 1
            seen.add(float(w["coef"]))
        assert 1.0 in seen and len(seen) >= 3 and min(seen) < 0.51


def test_record_of_a_norm_beyond_the_f32_range(ops):
    """norm 6e38: finite in double, inf in f32.  The step is applied, norm_f is +inf, the coefficient tiny and finite, the update the
    mirror's"""
    h = O.hyper("training")
    n = 4 * 4099
    p, g, m, v = _operands("training", n, True)
    g = g.copy()
    g[[5, 4098, 9000, n - 1]] = F(3e38)
    a = run((p, g, m, v), h, 4, "sched", max_norm=1.0, skip=True)
    sumsq = O.record_sum(a.partials)
    assert math.isfinite(sumsq) and a.rec.applied == 1 and np.isposinf(a.rec.norm_f) and 0 < float(a.rec.coef) < 1e-38 and a.rec.t == 4
    assert abs(a.rec.norm - 6e38) < 1e-6 * 6e38
    assert a.rec.coef.view(np.int32) == F(1.0 / (a.rec.norm + 1e-6)).view(np.int32)
    assert (a.iteration, a.skipped, a.step) == (ITER + 1, 0, 4)
    judge(a.__dict__, expect((p, g, m, v), h, 4, "sched", rec=a.rec), "norm beyond f32")
    assert (a.m != m).any()


# ---- the non-finite guard ----------------------------------------------------------------------------------------------------------
N4_TAIL = 1024 * 1024 + 1024     # chunk 1025: granule 1024 of a range is read by the tail loop alone, and by thread 0
N4_SHORT = 1025                  # chunk 2: range 512 is one granule long and the last that is not empty
BAD = (math.inf, -math.inf, math.nan)


def _guard_positions(n4):
    rs = [r for r in O.partial_ranges(n4) if r[1] > r[0]]
    pos = {"first": 0, "last": 4 * n4 - 1, "end_of_range_0": 4 * rs[0][1] - 1, "start_of_last_range": 4 * rs[-1][0]}
    if n4 == N4_TAIL:
        pos["tail_loop_only"] = 4 * (5 * 1025 + 1024) + 2
    else:
        assert rs[-1][1] - rs[-1][0] == 1 and len(rs) == 513
        pos["one_granule_range"] = 4 * rs[-1][0] + 1
    return pos


@pytest.mark.parametrize("n4", [N4_SHORT, N4_TAIL])
def test_one_nonfinite_element_anywhere_skips_the_step(ops, n4):
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    h = O.hyper("training")
    n = 4 * n4
    p, g, m, v = _operands("training", n)
    P = torch.nn.Parameter(_dev(p))
    opt = FlatAdamW(P, lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"], grad_clip=dict(max_norm=1.0), skip_nonfinite=True)
    opt.exp_avg.copy_(_dev(m))
    opt.exp_avg_sq.copy_(_dev(v))
    opt.step_t.fill_(3)
    opt.lowp = _shadow(n, "16")
    G = _dev(g)
    P.grad = G
    before = [t.clone() for t in (P.data.view(torch.int32), opt.exp_avg.view(torch.int32), opt.exp_avg_sq.view(torch.int32),
                                  opt.lowp.view(torch.int16))]
    runs = 0
    for where, j in _guard_positions(n4).items():
        for bad in BAD:
            keep = float(G[j])
            G[j] = bad
            opt.step()
            G[j] = keep
            runs += 1
            rec = _record(opt._record)
            assert rec.applied == 0 and rec.t == 3 and not math.isfinite(rec.norm), (where, bad, rec)
            assert (float(opt.step_t), float(opt.skipped), float(opt.iteration)) == (3, runs, runs), (where, bad)
            now = (P.data.view(torch.int32), opt.exp_avg.view(torch.int32), opt.exp_avg_sq.view(torch.int32), opt.lowp.view(torch.int16))
            assert all(torch.equal(a, b) for a, b in zip(before, now)), (where, bad)
    opt.step()                                               # and the clean gradient is applied
    assert _record(opt._record).applied == 1 and float(opt.step_t) == 4 and float(opt.skipped) == runs


@pytest.mark.parametrize("bad", BAD, ids=["inf", "-inf", "nan"])
def test_without_the_guard_the_same_gradients_give_what_the_mirror_gives(ops, bad):
    """an inf makes the norm inf and the coefficient 0 (inf 0 = NaN at that element alone), a NaN makes both NaN (every element)"""
    h = O.hyper("training")
    p, g, m, v = _operands("training", 4 * N4_SHORT, True)
    for where, j in _guard_positions(N4_SHORT).items():
        gb = g.copy()
        gb[j] = bad
        a = run((p, gb, m, v), h, 5, "sched", max_norm=1.0, skip=False)
        assert a.rec.applied == 1 and a.rec.t == 5 and (math.isnan(a.rec.coef) if math.isnan(bad) else a.rec.coef == 0)
        want = expect((p, gb, m, v), h, 5, "sched", rec=a.rec)
        judge(a.__dict__, want, f"{where} {bad}")
        assert int(np.isnan(a.p).sum()) == (p.size if math.isnan(bad) else 1)


def test_without_the_guard_an_inf_that_only_the_tail_loop_reads(ops):
    h = O.hyper("training")
    p, g, m, v = _operands("training", 4 * N4_TAIL)
    gb = g.copy()
    gb[_guard_positions(N4_TAIL)["tail_loop_only"]] = F(math.inf)
    a = run((p, gb, m, v), h, 5, "sched", max_norm=1.0, skip=False)
    assert a.rec.applied == 1 and a.rec.t == 5 and a.rec.coef == 0 and math.isinf(a.rec.norm)
    judge(a.__dict__, expect((p, gb, m, v), h, 5, "sched", rec=a.rec), "tail_loop_only inf")
    assert int(np.isnan(a.p).sum()) == 1


# ---- refused arguments -------------------------------------------------------------------------------------------------------------
def test_refused_arguments_touch_nothing(ops):
    from panoswintransformerobjectdetection_amd._lib import LrSchedule, PswinError, call, ptr
    n = 64
    bufs = {k: torch.full((n + 4,), 7.25, dtype=torch.float32, device=DEV) for k in ("p", "g", "m", "v", "step", "it", "skipped")}
    bufs["shadow"] = torch.full((n + 4,), 7.25, dtype=torch.bfloat16, device=DEV)
    bufs["partials"] = torch.full((O.PARTIALS,), 7.25, dtype=torch.float64, device=DEV)
    bufs["rec"] = torch.full((12,), 7.25, dtype=torch.float64, device=DEV)
    bufs["gmap"] = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    b = types.SimpleNamespace(**{k: ptr(t) for k, t in bufs.items()})
    ok8, neg = _floats(9, [1.0] * 9), _floats(8, [1.0, -0.5] + [1.0] * 6)
    a8, aneg = ctypes.addressof(ok8), ctypes.addressof(neg)
    sched = ctypes.addressof(_schedule("no_pow")[0])
    desc = LrSchedule(policy=1, n_milestones=2, gamma=0.1)
    desc.milestones[0], desc.milestones[1] = 5, 3
    hyp = (1e-4, 0.9, 0.999, 1e-8, 0.05)
    flat = lambda **k: ("pswin_adamw_flat", (k.get("p", b.p), b.g, b.m, b.v, b.shadow, k.get("n", n), k.get("lr", 1e-4), k.get("b1", 0.9), 0.999,
                                             1e-8, 0.05, b.step))
    groups = lambda k, lrm: ("pswin_adamw_flat_groups", (b.p, b.g, b.m, b.v, b.shadow, n, b.gmap, k, lrm, a8) + hyp + (b.step,))
    record = lambda s, max_norm, partials: ("pswin_adamw_record", (partials, s, 1e-4, 0, None, max_norm, 0, b.step, b.it, b.skipped, b.rec))
    refused = {
        "n % 4 != 0": flat(n=62),
        "a misaligned p": flat(p=ctypes.c_void_p(bufs["p"].data_ptr() + 4)),
        "beta1 = 1": flat(b1=1.0),
        "lr < 0": flat(lr=-1e-4),
        "n_groups = 9": groups(9, a8),
        "a negative multiplier": groups(8, aneg),
        "max_norm = NaN": record(sched, math.nan, b.partials),
        "partials = NULL with max_norm > 0": record(sched, 1.0, None),
        "descending milestones": record(ctypes.addressof(desc), 0.0, None),
        "a negative decay multiplier (scheduled)": ("pswin_adamw_flat_sched", (b.p, b.g, b.m, b.v, b.shadow, n, b.gmap, 8, aneg, 0.9, 0.999, 1e-8,
                                                                             0.05, b.rec)),
    }
    for what, (name, args) in refused.items():
        with pytest.raises(PswinError, match="invalid argument"):
            call(name, bufs["p"], *args)
        torch.cuda.synchronize()
        for k, t in bufs.items():
            assert bool((t == (7 if k == "gmap" else 7.25)).all()), (what, k)
    # and the same calls with the offending argument put right are accepted (on buffers of their own)
    good = {k: torch.zeros_like(t) for k, t in bufs.items()}
    one = torch.ones((), device=DEV)
    call("pswin_adamw_flat", good["p"], ptr(good["p"]), ptr(good["g"]), ptr(good["m"]), ptr(good["v"]), ptr(good["shadow"]), n, *hyp, ptr(one))
    torch.cuda.synchronize()
