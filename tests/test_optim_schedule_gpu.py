"""optim.FlatAdamW with the reference configs' training recipe on the device: lr_config (mmcv's LrUpdaterHook), grad_clip (mmcv's
OptimizerHook -> clip_grad_norm_) and the non-finite guard, eager and inside a captured hipGraph, against torch.optim.AdamW driven by
the restated schedule (tests/test_lr_schedule.py:mmcv_lr)."""
import io

import numpy as np
import pytest
import torch

from test_lr_schedule import mmcv_lr

pytestmark = pytest.mark.gpu
DEV = "cuda"
KW = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
# warmup over 5 iterations, decays at epochs 4 and 9 (iterations 12 and 27 with 3 iterations per epoch)
CFG = dict(policy="step", warmup="linear", warmup_iters=5, warmup_ratio=0.001, step=[4, 9])
IPE = 3


def f32(x):
    return float(np.float32(x))


def _flat(n, seed):
    g = torch.Generator(DEV).manual_seed(seed)
    return torch.nn.Parameter(torch.randn(n, device=DEV, generator=g))


def _grads(n, k, seed, scale=1.0):
    g = torch.Generator(DEV).manual_seed(seed)
    return [torch.randn(n, device=DEV, generator=g) * scale * (0.5 + (i % 3)) for i in range(k)]


def _ref_step(o_ref, ref, g, lr, max_norm=None):
    ref.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_([ref], max_norm) if max_norm else None
    o_ref.param_groups[0]["lr"] = lr
    o_ref.step()
    return total


def test_device_lr_record_follows_the_schedule(ops):
    from panoswintransformerobjectdetection_amd._lib import StepRecord
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    n = 4096
    p = _flat(n, 1)
    opt = FlatAdamW(p, lr=1e-3, lr_config=CFG, iters_per_epoch=IPE, **KW)
    for i, g in enumerate(_grads(n, 40, 2)):
        p.grad = g
        opt.step()
        rec = opt._record.cpu().numpy().view(np.uint8)
        lr_d = rec[:64].view(np.float64)[0]
        want = opt.lr_at(i)
        assert want == mmcv_lr(CFG, 1e-3, i, IPE)
        assert f32(lr_d) == f32(want) and float(opt.lr_tensor) == f32(want), (i, lr_d, want)
        t = rec[StepRecord.t.offset:StepRecord.t.offset + 4].view(np.float32)[0]
        it = rec[StepRecord.iteration.offset:StepRecord.iteration.offset + 4].view(np.int32)[0]
        assert (t, it) == (i + 1, i)
        assert float(opt.iteration) == i + 1 and float(opt.step_t) == i + 1 and float(opt.skipped) == 0
        assert float(opt.grad_norm) == 0.0                   # (no clipping, no guard: no sum of squares)
    assert f32(opt.lr_at(39)) == f32(1e-5)


def test_scheduled_parameter_groups_match_torch_adamw(ops):
    from panoswintransformerobjectdetection_amd import SimplePanoSwinTransformer
    from panoswintransformerobjectdetection_amd.dp import GradReducer
    from panoswintransformerobjectdetection_amd.optim import REFERENCE_PARAMWISE_CFG, FlatAdamW, paramwise_groups
    cfg = dict(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], ape=True, drop_path_rate=0.0)
    pw = dict(custom_keys=dict(REFERENCE_PARAMWISE_CFG["custom_keys"], **{"abs_encoder": dict(lr_mult=0.1, decay_mult=0.5)}))
    sched = dict(policy="step", warmup="linear", warmup_iters=4, warmup_ratio=0.001, step=[2, 3])
    torch.manual_seed(5)
    m = SimplePanoSwinTransformer(**cfg, compute_dtype=torch.bfloat16)
    m.init_weights(None)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn_like(p) * 0.5)
    m = m.to(DEV)
    named = list(m.named_parameters())
    ref_params = {k: torch.nn.Parameter(p.detach().clone()) for k, p in named}
    groups = {}
    for name, lr_mult, decay_mult in paramwise_groups(named, pw, "backbone"):
        groups.setdefault((lr_mult, decay_mult), []).append(ref_params[name])
    lr = 1e-2
    o_ref = torch.optim.AdamW([dict(params=ps, lr=lr * a, weight_decay=KW["weight_decay"] * b, lr_mult=a) for (a, b), ps in groups.items()],
                              betas=KW["betas"], eps=KW["eps"])
    red = GradReducer(m, pack=True)
    flat = red.flatten_parameters(m, torch.bfloat16)
    o_mine = FlatAdamW(flat, model=m, paramwise_cfg=pw, lr=lr, lr_config=sched, iters_per_epoch=4, **KW)
    for i in range(15):
        red.flat.copy_(torch.randn_like(red.flat) * (0.1 + i % 4))
        for k, p in named:
            ref_params[k].grad = p._grad_slot.view_as(p).clone()
        for grp in o_ref.param_groups:
            grp["lr"] = mmcv_lr(sched, lr * grp["lr_mult"], i, 4)
        o_ref.step()
        o_mine.step()
        for k, p in named:
            assert torch.allclose(p.data, ref_params[k].data, rtol=2e-6, atol=2e-7), (i, k, (p.data - ref_params[k].data).abs().max())
    assert torch.equal(m.__dict__["_flat_pair"][1], flat.data.to(torch.bfloat16))
    assert o_mine.param_groups[0]["lr"] == lr                # the base lr (mmcv's initial_lr) stays in the group


def test_grad_clip_matches_clip_grad_norm_then_adamw(ops):
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    n = 4 * 100003
    p = _flat(n, 3)
    ref = torch.nn.Parameter(p.data.clone())
    max_norm = 700.0                                          # |g| ~ 632 * (0.5, 1.5, 2.5): clipped on two steps of three
    opt = FlatAdamW(p, lr=1e-2, lr_config=CFG, iters_per_epoch=IPE, grad_clip=dict(max_norm=max_norm, norm_type=2), **KW)
    o_ref = torch.optim.AdamW([ref], lr=1e-2, **KW)
    clipped = []
    for i, g in enumerate(_grads(n, 9, 4)):
        p.grad = g.clone()
        total = _ref_step(o_ref, ref, g, mmcv_lr(CFG, 1e-2, i, IPE), max_norm)
        opt.step()
        want = float(g.double().norm())
        assert abs(float(opt.grad_norm) - float(total)) <= 1e-5 * float(total), (i, float(opt.grad_norm), float(total))
        assert abs(float(opt._record[8]) - want) <= 1e-12 * want
        assert torch.equal(p.grad, g)                        # the flat gradient keeps the unclipped values
        clipped.append(float(total) > max_norm)
        assert torch.allclose(p.data, ref.data, rtol=2e-6, atol=2e-7), (i, (p.data - ref.data).abs().max())
    assert any(clipped) and not all(clipped)


def _capture(fn, warmup=2):
    from panoswintransformerobjectdetection_amd.graph import GraphedCallable
    return GraphedCallable(fn, warmup=warmup, parameters=[])


def test_captured_steps_follow_the_schedule(ops):
    """The whole point: a replayed FlatAdamW.step() picks up the lr of the iteration it runs, without the host."""
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    n = 4 * 20000
    p = _flat(n, 5)
    ref = torch.nn.Parameter(p.data.clone())
    opt = FlatAdamW(p, lr=1e-2, lr_config=CFG, iters_per_epoch=IPE, **KW)
    o_ref = torch.optim.AdamW([ref], lr=1e-2, **KW)
    gs = _grads(n, 20, 6)
    src = torch.zeros(n, device=DEV)
    p.grad = torch.zeros(n, device=DEV)
    it = 0
    for j in range(2):                                        # eager steps
        p.grad.copy_(gs[j])
        opt.step()
        _ref_step(o_ref, ref, gs[j], mmcv_lr(CFG, 1e-2, it, IPE))
        it += 1

    def fn():
        p.grad.copy_(src)
        opt.step()

    src.copy_(gs[2])
    g = _capture(fn)                                          # the two warm-up passes are real iterations
    for _ in range(2):
        _ref_step(o_ref, ref, gs[2], mmcv_lr(CFG, 1e-2, it, IPE))
        it += 1
    torch.cuda.synchronize()
    assert torch.allclose(p.data, ref.data, rtol=2e-6, atol=2e-7)
    for j in range(3, 20):
        src.copy_(gs[j])
        g()
        lr = mmcv_lr(CFG, 1e-2, it, IPE)
        _ref_step(o_ref, ref, gs[j], lr)
        torch.cuda.synchronize()
        assert float(opt.lr_tensor) == f32(lr), (it, float(opt.lr_tensor), lr)
        assert float(opt.iteration) == it + 1
        assert torch.allclose(p.data, ref.data, rtol=2e-6, atol=2e-7), (it, (p.data - ref.data).abs().max())
        it += 1
    assert it == 21 and f32(mmcv_lr(CFG, 1e-2, 20, IPE)) == f32(1e-3)


def test_nonfinite_gradient_skips_the_step_and_the_schedule_moves_on(ops):
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    n = 4 * 5000
    p = _flat(n, 7)
    ref = torch.nn.Parameter(p.data.clone())
    opt = FlatAdamW(p, lr=1e-2, lr_config=CFG, iters_per_epoch=IPE, skip_nonfinite=True, **KW)
    shadow = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    opt.lowp = shadow
    o_ref = torch.optim.AdamW([ref], lr=1e-2, **KW)
    gs = _grads(n, 8, 8)
    bad_at = 4
    gs[bad_at][17] = float("inf")
    gs[bad_at][4711] = float("nan")
    for i, g in enumerate(gs):
        p.grad = g.clone()
        before = [t.clone() for t in (p.data, opt.exp_avg, opt.exp_avg_sq, shadow, opt.step_t)]
        opt.step()
        torch.cuda.synchronize()
        if i == bad_at:
            for a, b in zip(before, (p.data, opt.exp_avg, opt.exp_avg_sq, shadow, opt.step_t)):
                assert torch.equal(a, b)
            assert not np.isfinite(float(opt.grad_norm))
        else:
            _ref_step(o_ref, ref, g, mmcv_lr(CFG, 1e-2, i, IPE))  # the reference skips the bad iteration, its lr moves on
            assert torch.allclose(p.data, ref.data, rtol=2e-6, atol=2e-7), (i, (p.data - ref.data).abs().max())
            assert torch.equal(shadow, p.data.to(torch.bfloat16))
        assert float(opt.iteration) == i + 1
        assert float(opt.skipped) == (1.0 if i >= bad_at else 0.0)
        assert float(opt.step_t) == (i if i >= bad_at else i + 1)


def test_grad_norm_is_bit_identical_across_replays(ops):
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    n = 4 * (1 << 22) + 4 * 321                               # 16.8 M elements: every one of the 1024 partial ranges is long
    p = _flat(n, 9)
    opt = FlatAdamW(p, lr=1e-4, grad_clip=dict(max_norm=1.0), **KW)
    p.grad = torch.randn(n, device=DEV, generator=torch.Generator(DEV).manual_seed(10))
    opt.step()
    eager = opt._record[8].clone()
    g = _capture(lambda: opt.step())
    norms = []
    for _ in range(2):
        g()
        torch.cuda.synchronize()
        norms.append(opt._record[8].clone())
    assert torch.equal(norms[0], norms[1]) and torch.equal(norms[0], eager)
    want = p.grad.double().square().sum().sqrt()
    assert abs(float(norms[0]) - float(want)) <= 1e-6 * float(want)
    assert float(opt.grad_norm) == f32(float(norms[0]))


def test_state_dict_round_trip_in_the_middle_of_warmup(ops):
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    n = 4 * 3000
    gs = _grads(n, 10, 11, scale=30.0)
    kw = dict(lr=1e-2, lr_config=dict(CFG, warmup_iters=8), iters_per_epoch=IPE, grad_clip=dict(max_norm=100.0), skip_nonfinite=True, **KW)
    a = _flat(n, 12)
    b = torch.nn.Parameter(a.data.clone())
    oa = FlatAdamW(a, **kw)
    for g in gs:
        a.grad = g.clone()
        oa.step()
    ob = FlatAdamW(b, **kw)
    for g in gs[:4]:
        b.grad = g.clone()
        ob.step()
    buf = io.BytesIO()
    torch.save(ob.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf)
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "iteration", "skipped"}
    assert sd["param_groups"][0]["lr_config"] == kw["lr_config"] and sd["param_groups"][0]["grad_clip"] == kw["grad_clip"]
    b2 = torch.nn.Parameter(b.data.clone())
    ob2 = FlatAdamW(b2, **kw)
    ob2.load_state_dict(sd)
    assert float(ob2.iteration) == 4.0
    for g in gs[4:]:
        b2.grad = g.clone()
        ob2.step()
    assert torch.equal(a.data, b2.data) and torch.equal(oa.exp_avg_sq, ob2.exp_avg_sq)
    assert float(ob2.lr_tensor) == float(oa.lr_tensor)
    # a state dict without the counters (torch.optim.AdamW's): iteration = step
    c = torch.nn.Parameter(a.data.clone())
    oc = torch.optim.AdamW([c], lr=1e-2, capturable=True, **KW)
    for g in gs[:3]:
        c.grad = g.clone()
        oc.step()
    od = FlatAdamW(torch.nn.Parameter(c.data.clone()), **kw)
    od.load_state_dict(oc.state_dict())
    assert float(od.iteration) == 3.0 and float(od.skipped) == 0.0 and od.param_groups[0]["lr_config"] == kw["lr_config"]


def test_capturable_torch_adamw_reads_lr_tensor_in_the_same_graph(ops):
    """The detector's head parameters under torch.optim.AdamW(lr=opt.lr_tensor, capturable=True), stepped after FlatAdamW in one graph."""
    from panoswintransformerobjectdetection_amd.optim import FlatAdamW
    n, nh = 4 * 4000, 3000
    p = _flat(n, 13)
    q = _flat(nh, 14)
    qref = torch.nn.Parameter(q.data.clone())
    opt = FlatAdamW(p, lr=1e-2, lr_config=CFG, iters_per_epoch=IPE, **KW)
    head = torch.optim.AdamW([q], lr=opt.lr_tensor, capturable=True, foreach=True, **KW)
    assert head.param_groups[0]["lr"] is opt.lr_tensor                # torch keeps the tensor itself, no copy
    o_ref = torch.optim.AdamW([qref], lr=1e-2, **KW)
    src, srcq = torch.zeros(n, device=DEV), torch.zeros(nh, device=DEV)
    p.grad, q.grad = torch.zeros(n, device=DEV), torch.zeros(nh, device=DEV)
    gq = _grads(nh, 16, 15)

    def fn():
        p.grad.copy_(src)
        q.grad.copy_(srcq)
        opt.step()
        head.step()

    srcq.copy_(gq[0])
    g = _capture(fn)
    it = 0
    for _ in range(2):
        _ref_step(o_ref, qref, gq[0], f32(mmcv_lr(CFG, 1e-2, it, IPE)))
        it += 1
    for j in range(1, 16):
        srcq.copy_(gq[j])
        g()
        _ref_step(o_ref, qref, gq[j], f32(mmcv_lr(CFG, 1e-2, it, IPE)))
        torch.cuda.synchronize()
        assert torch.allclose(q.data, qref.data, rtol=1e-5, atol=1e-6), (it, (q.data - qref.data).abs().max())
        it += 1
    assert head.param_groups[0]["lr"].data_ptr() == opt.lr_tensor.data_ptr()


def test_captured_tiny_panoswin_with_schedule_and_clipping_matches_eager_torch(ops):
    """End to end: TINY PanoSwin, bf16, GradReducer's flat buffer, FlatAdamW with lr_config + grad_clip + the reference paramwise_cfg,
    captured on one stream and replayed 8 times, against an eager copy stepped by torch.optim.AdamW after clip_grad_norm_, at the bounds
    of test_backbone_gpu.py::test_training_steps_with_the_flat_hip_adamw_match_torch_adamw: no element further apart than 2 lr per step
    (here the sum of the scheduled lr of the steps taken), < 2 % of the elements apart by more than 1e-5 after its 3 steps.  Those are
    Adam's sign noise on near-zero gradients, whose share grows with every step at full lr: after all 10 steps it is bounded by 6 %
    (measured 5.0 %; 0.8 % after 3 steps), while the gradient norms of the two runs agree to 1e-3."""
    from _util import TINY
    from panoswintransformerobjectdetection_amd import SimplePanoSwinTransformer
    from panoswintransformerobjectdetection_amd.dp import GradReducer
    from panoswintransformerobjectdetection_amd.graph import GraphedCallable
    from panoswintransformerobjectdetection_amd.optim import REFERENCE_PARAMWISE_CFG, FlatAdamW, paramwise_groups
    lr, ipe = 1e-3, 2
    sched = dict(policy="step", warmup="linear", warmup_iters=4, warmup_ratio=0.001, step=[3, 4])
    x = torch.randn(2, 3, 128, 256, device=DEV, generator=torch.Generator(DEV).manual_seed(3))

    def build():
        torch.manual_seed(0)
        m = SimplePanoSwinTransformer(**TINY, window_size=7, pano_mode=True, compute_dtype=torch.bfloat16)
        m.init_weights(None)
        return m.to(DEV).train()

    def loss_of(m, ws):
        return sum(o.float().flatten() @ w for o, w in zip(m(x), ws))

    r = build()                                               # the eager reference; its first gradient sets max_norm (clipping active early)
    with torch.no_grad():
        ws = [torch.linspace(-1, 1, o.numel(), device=DEV) / o.numel() for o in r(x)]
    loss_of(r, ws).backward()
    max_norm = 0.5 * float(torch.cat([p.grad.flatten() for p in r.parameters() if p.grad is not None]).double().norm())
    torch.cuda.synchronize()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m = build()
        red = GradReducer(m, pack=True)
        flat = red.flatten_parameters(m, torch.bfloat16)
        opt = FlatAdamW(flat, model=m, paramwise_cfg=REFERENCE_PARAMWISE_CFG, lr=lr, lr_config=sched, iters_per_epoch=ipe,
                        grad_clip=dict(max_norm=max_norm), **KW)
        gaps = torch.ones(flat.numel(), dtype=torch.bool, device=DEV)
        for p in m.parameters():
            gaps[p._grad_slot.storage_offset():p._grad_slot.storage_offset() + p.numel()] = False
        assert int(gaps.sum()) > 0

        def step():
            red.zero_grad()
            loss = loss_of(m, ws)
            loss.backward()
            red.pack_grads()
            red.finish()
            opt.step()
            return loss.detach()

        g = GraphedCallable(step, warmup=2, stream=side, parameters=[m])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    # eager reference: the same model stepped by torch.optim.AdamW (per-parameter groups) after clip_grad_norm_, one step per
    # warm-up pass / replay of the captured step
    named = list(r.named_parameters())
    groups = {}
    for name, lr_mult, decay_mult in paramwise_groups(named, REFERENCE_PARAMWISE_CFG, "backbone"):
        groups.setdefault((lr_mult, decay_mult), []).append(dict(named)[name])
    o_ref = torch.optim.AdamW([dict(params=ps, lr=lr * a, weight_decay=KW["weight_decay"] * b, lr_mult=a) for (a, b), ps in groups.items()],
                              betas=KW["betas"], eps=KW["eps"])

    def ref_step(i):
        o_ref.zero_grad()
        loss_of(r, ws).backward()
        total = torch.nn.utils.clip_grad_norm_([p for _, p in named if p.grad is not None], max_norm)
        for grp in o_ref.param_groups:
            grp["lr"] = mmcv_lr(sched, lr * grp["lr_mult"], i, ipe)
        o_ref.step()
        return float(total)

    def diff():
        return torch.cat([(p.data - q.data).abs().flatten() for p, (_, q) in zip(m.parameters(), named)])

    norms = [ref_step(0), ref_step(1)]
    lr_sum = mmcv_lr(sched, lr, 0, ipe) + mmcv_lr(sched, lr, 1, ipe)
    for i in range(2, 10):
        with torch.cuda.stream(side):
            g()
            side.synchronize()
            assert not bool(red.flat[gaps].any())             # the alignment gaps of the flat gradient stay zero
            mine = float(opt.grad_norm)
        norms.append(ref_step(i))
        assert abs(mine - norms[-1]) <= 1e-3 * norms[-1], (i, mine, norms[-1])
        assert float(opt.lr_tensor) == f32(mmcv_lr(sched, lr, i, ipe))
        lr_sum += mmcv_lr(sched, lr, i, ipe)
        d = diff()
        assert float(d.max()) <= 2 * lr_sum * 1.01, (i, float(d.max()), lr_sum)
        if i == 2:
            assert float((d > 1e-5).float().mean()) < 0.02, (i, (d > 1e-5).float().mean())
    with torch.cuda.stream(side):
        outs = [o.detach().float().clone() for o in m(x)]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert float(opt.iteration) == 10.0
    assert any(v > max_norm for v in norms)                  # clipping was active
    with torch.no_grad():
        ref_outs = [o.float() for o in r(x)]
    d = diff()
    assert float((d > 1e-5).float().mean()) < 0.06, (d > 1e-5).float().mean()
    for a, b in zip(outs, ref_outs):
        assert torch.allclose(a, b, rtol=2e-2, atol=2e-2), (a - b).abs().max()
