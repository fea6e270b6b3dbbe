"""The device lr schedule of optim.FlatAdamW (lr_config / grad_clip / skip_nonfinite) on the host side: FlatAdamW.lr_at against an
independent restatement of mmcv's LrUpdaterHook rules (mmcv 1.2.4 - 1.4.0: StepLrUpdaterHook.get_lr, LrUpdaterHook.get_warmup_lr),
the reference configs' anchors, the keys that are refused, and the argument checks of the new C entry points.  No GPU."""
import ctypes

import pytest
import torch

from panoswintransformerobjectdetection_amd import _lib
from panoswintransformerobjectdetection_amd._lib import PswinError
from panoswintransformerobjectdetection_amd.optim import FlatAdamW, parse_grad_clip, parse_lr_config, scheduled_lr

SCHEDULE_1X = dict(policy="step", warmup="linear", warmup_iters=500, warmup_ratio=0.001, step=[8, 11])     # configs/_base_/schedules/schedule_1x.py
SCHEDULE_3X = dict(SCHEDULE_1X, step=[27, 33])                                                            # configs/swin/*_3x_coco.py
SCHEDULE_STREET = dict(SCHEDULE_1X, step=[8 * 30, 11 * 30])                                               # the PanoSwin street config


def mmcv_lr(cfg, base, it, iters_per_epoch=None):
    """Restated from mmcv's hooks: the lr that runner.iter == it runs with."""
    by_epoch = cfg.get("by_epoch", True)
    if cfg["policy"] == "fixed":
        regular = base
    else:
        progress = it // iters_per_epoch if by_epoch else it
        step = cfg["step"]
        if isinstance(step, int):
            n = progress // step
        else:
            n = len(step)
            for j, s in enumerate(step):
                if progress < s:
                    n = j
                    break
        regular = base * cfg.get("gamma", 0.1) ** n
        if cfg.get("min_lr") is not None:
            regular = max(regular, cfg["min_lr"])
    warmup = cfg.get("warmup")
    if warmup is None:
        return regular
    w_iters = cfg["warmup_iters"] * (iters_per_epoch if cfg.get("warmup_by_epoch", False) else 1)
    if it >= w_iters:
        return regular
    ratio = cfg.get("warmup_ratio", 0.1)
    if warmup == "constant":
        return regular * ratio
    if warmup == "linear":
        k = (1 - it / w_iters) * (1 - ratio)
        return regular * (1 - k)
    return regular * ratio ** (1 - it / w_iters)


def lr_at(cfg, it, lr=1e-4, iters_per_epoch=None):
    return scheduled_lr(parse_lr_config(cfg, iters_per_epoch), lr, it)


def _check(cfg, ipe, iters, lr=1e-4):
    for it in iters:
        want = mmcv_lr(cfg, lr, it, ipe)
        got = lr_at(cfg, it, lr, ipe)
        assert got == pytest.approx(want, rel=1e-15, abs=0), (cfg, it)


@pytest.mark.parametrize("cfg", [SCHEDULE_1X, SCHEDULE_3X, SCHEDULE_STREET], ids=["1x", "3x", "street"])
@pytest.mark.parametrize("by_epoch", [True, False])
def test_reference_schedules_match_the_restated_rules(cfg, by_epoch):
    cfg = dict(cfg, by_epoch=by_epoch)
    ipe = 1000
    last = (cfg["step"][-1] + 2) * (ipe if by_epoch else 1)
    iters = list(range(0, 600)) + list(range(0, last, 97)) + [s * (ipe if by_epoch else 1) + d for s in cfg["step"] for d in (-1, 0, 1)]
    _check(cfg, ipe, iters)


@pytest.mark.parametrize("warmup", ["constant", "linear", "exp", None])
@pytest.mark.parametrize("warmup_by_epoch", [False, True])
def test_every_warmup_kind(warmup, warmup_by_epoch):
    cfg = dict(policy="step", warmup=warmup, warmup_iters=2 if warmup_by_epoch else 50, warmup_ratio=0.01, step=[3, 5],
               warmup_by_epoch=warmup_by_epoch)
    if warmup is None:
        del cfg["warmup_iters"], cfg["warmup_ratio"]
    _check(cfg, 37, range(0, 37 * 7))


def test_fixed_policy_int_step_min_lr_and_gamma():
    _check(dict(policy="fixed", warmup="exp", warmup_iters=20, warmup_ratio=0.1), None, range(40))
    _check(dict(policy="step", step=3, gamma=0.5, by_epoch=False), None, range(40))
    _check(dict(policy="step", step=[2, 4, 6], gamma=0.1, min_lr=3e-7, by_epoch=True), 5, range(60))
    _check(dict(policy="Step", step=[2], by_epoch=False, warmup="linear", warmup_iters=3, warmup_ratio=1.0), None, range(10))


def test_anchors_of_the_1x_schedule():
    ipe = 1000
    assert lr_at(SCHEDULE_1X, 0, iters_per_epoch=ipe) == pytest.approx(1e-4 * 0.001, rel=1e-14)
    assert lr_at(SCHEDULE_1X, 250, iters_per_epoch=ipe) == pytest.approx(1e-4 * 0.5005, rel=1e-14)
    assert lr_at(SCHEDULE_1X, 499, iters_per_epoch=ipe) == pytest.approx(1e-4 * (1 - 0.999 / 500), rel=1e-14)
    assert lr_at(SCHEDULE_1X, 500, iters_per_epoch=ipe) == 1e-4
    assert lr_at(SCHEDULE_1X, 8 * ipe - 1, iters_per_epoch=ipe) == 1e-4
    assert lr_at(SCHEDULE_1X, 8 * ipe, iters_per_epoch=ipe) == pytest.approx(1e-5, rel=1e-14)
    assert lr_at(SCHEDULE_1X, 11 * ipe - 1, iters_per_epoch=ipe) == pytest.approx(1e-5, rel=1e-14)
    assert lr_at(SCHEDULE_1X, 11 * ipe, iters_per_epoch=ipe) == pytest.approx(1e-6, rel=1e-14)


@pytest.mark.parametrize("cfg, word", [
    (dict(policy="CosineAnnealing", min_lr=0), "CosineAnnealing"),
    (dict(policy="poly", power=0.9), "power"),
    (dict(policy="Poly"), "Poly"),
    (dict(policy="step", step=[8, 11], warmup="cosine", warmup_iters=5), "cosine"),
    (dict(policy="step", step=[8, 11], warmup_iters=5, by_epoch=True, cyclic_times=2), "cyclic_times"),
    (dict(policy="step", step=[11, 8], by_epoch=False), "step"),
    (dict(policy="step", step=[8, 11]), "iters_per_epoch"),
])
def test_unsupported_lr_config_raises(cfg, word):
    with pytest.raises(PswinError, match=word):
        parse_lr_config(cfg, None)


def test_unsupported_grad_clip_raises():
    assert parse_grad_clip(dict(max_norm=35, norm_type=2)) == 35.0
    assert parse_grad_clip(None) == 0.0
    for bad, word in ((dict(max_norm=35, norm_type=1), "norm_type"), (dict(max_norm=35, norm_type=float("inf")), "norm_type"),
                      (dict(max_norm=-1), "max_norm"), (dict(max_norm=1, error_if_nonfinite=True), "error_if_nonfinite")):
        with pytest.raises(PswinError, match=word):
            parse_grad_clip(bad)


def test_flat_adamw_refuses_an_unsupported_recipe_before_touching_a_device():
    p = torch.nn.Parameter(torch.zeros(16))
    with pytest.raises(PswinError):                      # (a CPU buffer is refused first; the recipe check must not mask that)
        FlatAdamW(p, lr_config=SCHEDULE_1X, iters_per_epoch=10)


def _sched(**kw):
    s = _lib.LrSchedule(policy=1, warmup=2, warmup_iters=500, by_epoch=1, iters_per_epoch=100, n_milestones=2, step_every=0, has_min_lr=0,
                        warmup_ratio=0.001, gamma=0.1, min_lr=0.0)
    s.milestones[0], s.milestones[1] = 8, 11
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_argument_errors_of_the_schedule_entry_points_without_a_gpu():
    """Every bad call returns PSWIN_ERR_ARG (-1) before anything is launched (only rejected calls are made: no device here)."""
    lib = _lib.load()
    ERR = -1
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15
    assert ctypes.sizeof(_lib.LrSchedule) == 88 and ctypes.sizeof(_lib.StepRecord) == 96
    # pswin_grad_sumsq(g, n, partials, stream)
    assert lib.pswin_grad_sumsq(None, 1024, p16, None) == ERR
    assert lib.pswin_grad_sumsq(p16, 1022, p16, None) == ERR
    assert lib.pswin_grad_sumsq(p16, 0, p16, None) == ERR
    assert lib.pswin_grad_sumsq(p16 + 4, 1024, p16, None) == ERR
    assert lib.pswin_grad_sumsq(p16, 1024, None, None) == ERR
    assert lib.pswin_grad_sumsq(p16, 1024, p16 + 4, None) == ERR
    # pswin_adamw_record(partials, sched, lr, n_groups, lr_mult, max_norm, skip_nonfinite, step, iteration, skipped, record, stream)
    mult = (ctypes.c_float * 2)(1.0, 0.1)
    good_sched = _sched()
    ok = [p16, ctypes.addressof(good_sched), 1e-4, 2, ctypes.addressof(mult), 35.0, 1, p16, p16 + 4, p16 + 8, p16 + 64, None]
    keep = []
    for i, v in ((0, None),                      # clipping needs the partial sums
                 (1, None), (2, -1e-4), (3, 0), (3, 9), (4, None), (5, float("nan")), (7, None), (8, None), (9, None), (10, None),
                 (10, p16 + 4)):
        bad = list(ok); bad[i] = v
        if i == 4:
            bad[3] = 2                           # lr_mult NULL takes 0 or 1 groups only
        assert lib.pswin_adamw_record(*bad) == ERR, (i, v)
    bad = list(ok); bad[0] = None; bad[5] = 0.0      # no partials: the guard needs them too
    assert lib.pswin_adamw_record(*bad) == ERR
    bad_mult = (ctypes.c_float * 2)(1.0, -0.5)
    bad = list(ok); bad[4] = ctypes.addressof(bad_mult)
    assert lib.pswin_adamw_record(*bad) == ERR
    for field, v in (("policy", 2), ("warmup", 4), ("warmup_iters", 0), ("warmup_ratio", 1.5), ("iters_per_epoch", 0),
                     ("n_milestones", 9), ("step_every", -1), ("gamma", -0.1), ("gamma", float("nan"))):
        s = _sched(**{field: v})
        keep.append(s)
        bad = list(ok); bad[1] = ctypes.addressof(s)
        assert lib.pswin_adamw_record(*bad) == ERR, field
    s = _sched()
    s.milestones[0], s.milestones[1] = 11, 8                                  # milestones ascending
    bad = list(ok); bad[1] = ctypes.addressof(s)
    assert lib.pswin_adamw_record(*bad) == ERR
    s = _sched(has_min_lr=1, min_lr=-1.0)
    bad = list(ok); bad[1] = ctypes.addressof(s)
    assert lib.pswin_adamw_record(*bad) == ERR
    # pswin_adamw_flat_sched(p, g, m, v, p_bf16, n, group_of, n_groups, decay_mult, b1, b2, eps, wd, record, stream)
    dmult = (ctypes.c_float * 2)(1.0, 0.0)
    ok = [p16, p16, p16, p16, None, 1024, p16, 2, ctypes.addressof(dmult), 0.9, 0.999, 1e-8, 0.05, p16, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (13, None), (5, 1022), (5, 0), (0, p16 + 4), (4, p16 + 2), (13, p16 + 4),
                 (7, 0), (7, 9), (8, None), (9, 1.0), (10, -0.1), (11, -1.0)):
        bad = list(ok); bad[i] = v
        assert lib.pswin_adamw_flat_sched(*bad) == ERR, (i, v)
    bad = list(ok); bad[6] = None                                              # one group: n_groups 0
    assert lib.pswin_adamw_flat_sched(*bad) == ERR
    bad_d = (ctypes.c_float * 2)(1.0, -1.0)
    bad = list(ok); bad[8] = ctypes.addressof(bad_d)
    assert lib.pswin_adamw_flat_sched(*bad) == ERR
