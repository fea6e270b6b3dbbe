"""Sample skipping under per-sample DropPath on the GPU: the ring kernel's live slabs, the tiled GEMM's live-tile compaction, the Mlp
node on poisoned buffers, and a two-stage model with the switch on and off, eager and captured.

"Equal" below means numerically equal element by element (a zero may differ in sign; a NaN equals nothing): skipping removes exact-zero
terms from f32 sums and whole tiles whose result is multiplied by zero afterwards, so nothing else may change."""
import pytest
import torch

from panoswintransformerobjectdetection_amd import _lib, grad_queue, ops
from panoswintransformerobjectdetection_amd._lib import call, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


def patterns(B):
    """scale vectors: none dead, first dead, last dead, an interior one dead, all but one dead, all dead"""
    keep = 1.25
    out = {"none": [keep] * B, "first": [0.0] + [keep] * (B - 1), "last": [keep] * (B - 1) + [0.0],
           "interior": [keep if b != B // 2 else 0.0 for b in range(B)], "all_but_one": [0.0 if b != 1 else keep for b in range(B)],
           "all": [0.0] * B}
    return {k: torch.tensor(v, dtype=torch.float32, device=DEV) for k, v in out.items()}


def rows_mask(scale, rps):
    return (scale == 0).repeat_interleave(rps)


def equal(a, b):
    return bool((a == b).all())


def bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def rand(shape, seed, dtype=BF):
    return (torch.randn(*shape, device=DEV, generator=torch.Generator(DEV).manual_seed(seed)) * 0.5).to(dtype)


# ---- weight gradient: the ring kernel -----------------------------------------------------------------------------------------

def run_wgrad(dy, x, splits, live, bias=True):
    M, N = dy.shape
    K = x.shape[1]
    part = torch.full((splits, N, K), 7.0, dtype=BF if splits > 1 else torch.float32, device=DEV)
    dbp = torch.full((splits, N), 7.0, dtype=torch.float32, device=DEV) if bias else None
    grad_queue._launch_wgrads([grad_queue.weight_grad(dy, x, part, dbp, splits, 0, 0, live)])
    dw = ops.sum_rows(part, splits, N * K).view(N, K) if splits > 1 else part.view(N, K)
    return part, dbp, dw


RING_CASES = [(64, 1), (64, 2), (128, 1), (128, 2), (192, 1), (192, 2), (192, 3), (98, 1), (98, 2)]


@pytest.mark.parametrize("rps,splits", RING_CASES)
def test_ring_kernel_leaves_out_the_slabs_of_dead_samples(rps, splits):
    """N = K = 192, B = 4: dy has exact zeros in dead rows; partial tiles, bias partials and the reduced dW equal the job without liveness.
    192 rows per sample with 3 splits puts the split boundaries inside samples; 98 rows per sample (two windows) is not slab-aligned, so
    slabs straddle samples and are kept.  Aligned cases run again with NaN in the dead rows of BOTH operands."""
    B, N, K = 4, 192, 192
    M = B * rps
    dy0, x0 = rand((M, N), 1), rand((M, K), 2)
    for name, scale in patterns(B).items():
        dead = rows_mask(scale, rps)
        dy = dy0.clone()
        dy[dead] = 0
        want = run_wgrad(dy, x0, splits, None)
        got = run_wgrad(dy, x0, splits, (scale, rps))
        for w, g, what in zip(want, got, ("partial", "bias partial", "dW")):
            assert equal(w, g), (name, what)
        if name == "all":
            assert equal(got[2], torch.zeros_like(got[2])) and equal(got[1], torch.zeros_like(got[1]))
        if rps % 64 == 0:
            dyp, xp = dy.clone(), x0.clone()
            dyp[dead] = float("nan")
            xp[dead] = float("nan")
            poisoned = run_wgrad(dyp, xp, splits, (scale, rps))
            for w, g, what in zip(want, poisoned, ("partial", "bias partial", "dW")):
                assert equal(w, g), (name, what, "poisoned")


def test_ring_kernel_grouped_launch_mixes_jobs_with_and_without_liveness():
    B, rps, N, K = 4, 128, 192, 192
    M = B * rps
    scale = patterns(B)["interior"]
    dead = rows_mask(scale, rps)
    dy_a, x_a, dy_b, x_b = rand((M, N), 3), rand((M, K), 4), rand((M, 2 * N), 5), rand((M, K), 6)
    dy_a[dead] = 0
    want_a, want_b = run_wgrad(dy_a, x_a, 2, None), run_wgrad(dy_b, x_b, 1, None)
    xp = x_a.clone()
    xp[dead] = float("nan")                                   # job a skips its dead slabs; job b (no liveness) contracts every row
    pa = torch.full((2, N, K), 7.0, dtype=BF, device=DEV)
    da = torch.full((2, N), 7.0, dtype=torch.float32, device=DEV)
    pb = torch.full((1, 2 * N, K), 7.0, dtype=torch.float32, device=DEV)
    db = torch.full((1, 2 * N), 7.0, dtype=torch.float32, device=DEV)
    grad_queue._launch_wgrads([grad_queue.weight_grad(dy_a, xp, pa, da, 2, 0, 0, (scale, rps)),
                               grad_queue.weight_grad(dy_b, x_b, pb, db, 1, 0, 0, None)])
    assert equal(pa, want_a[0]) and equal(da, want_a[1]) and equal(pb, want_b[0]) and equal(db, want_b[1])


def test_ring_kernel_rejects_liveness_it_cannot_index():
    lib = _lib.load()
    M, N, K = 8192, 192, 192
    dy, x = torch.zeros(M, N, dtype=BF, device=DEV), torch.zeros(M, K, dtype=BF, device=DEV)
    part = torch.zeros(1, N, K, dtype=torch.float32, device=DEV)
    s = torch.ones(4, device=DEV)
    import ctypes
    arr = (_lib.TnJob * 1)()
    grad_queue.weight_grad(dy, x, part, None, 1, 0, 0, (s, 2048)).fill(arr[0])       # 8,192 rows in one range: 128 slabs > 64
    assert lib.pswin_gemm_tn_ring_jobs(ctypes.cast(arr, ctypes.c_void_p), 1, None) == -1
    grad_queue.weight_grad(dy, x, part, None, 2, 0, 0, (s, 2000)).fill(arr[0])       # rows are not whole samples
    assert lib.pswin_gemm_tn_ring_jobs(ctypes.cast(arr, ctypes.c_void_p), 1, None) == -1


# ---- tiled GEMM: live-tile compaction ---------------------------------------------------------------------------------------

def nt_plain(x, w, bias, tile, live):
    M, K = x.shape
    N = w.shape[0]
    y = torch.full((M, N), 7.0, dtype=BF, device=DEV)
    if live is None:
        call("pswin_gemm_nt", x, ptr(x), ptr(w), ptr(bias), ptr(y), M, K, N, tile)
    else:
        call("pswin_gemm_nt_live", x, ptr(x), ptr(w), ptr(bias), ptr(y), M, K, N, tile, ptr(live[0]), live[1])
    return (y,)


def nt_gelu_fwd(x, w, bias, tile, live):
    M, K = x.shape
    N = w.shape[0]
    pre, h = torch.full((M, N), 7.0, dtype=BF, device=DEV), torch.full((M, N), 7.0, dtype=BF, device=DEV)
    if live is None:
        call("pswin_gemm_nt_gelu_fwd", x, ptr(x), ptr(w), ptr(bias), ptr(pre), ptr(h), M, K, N, tile)
    else:
        call("pswin_gemm_nt_gelu_fwd_live", x, ptr(x), ptr(w), ptr(bias), ptr(pre), ptr(h), M, K, N, tile, ptr(live[0]), live[1])
    return pre, h


def nt_gelu_bwd(dy, wt, pre, bias, tile, live):
    M, K = dy.shape
    N = wt.shape[0]
    g = torch.full((M, N), 7.0, dtype=BF, device=DEV)
    part = torch.full((M // tile, N), 7.0, dtype=torch.float32, device=DEV)
    if live is None:
        call("pswin_gemm_nt_gelu_bwd", dy, ptr(dy), ptr(wt), ptr(pre), ptr(bias), ptr(g), ptr(part), M, K, N, tile)
    else:
        call("pswin_gemm_nt_gelu_bwd_live", dy, ptr(dy), ptr(wt), ptr(pre), ptr(bias), ptr(g), ptr(part), M, K, N, tile, ptr(live[0]), live[1])
    return g, part


# K = 192: three k-steps, the four-stage form (every shape here has <= 256 tiles); K = 128: two k-steps, the two-stage form
NT_CASES = [(B, rps, tile, K) for B in (3, 5) for rps, tile in ((128, 128), (256, 128), (64, 64)) for K in (192, 128)]


@pytest.mark.parametrize("B,rps,tile,K", NT_CASES)
def test_tiled_gemm_computes_live_tiles_and_settles_dead_ones(B, rps, tile, K):
    """N = 384 (two column tiles): tiles per sample 1 and 2, tiles_live not a multiple of 8 (the remainder branch of the XCD deal) and
    tiles_live = 0.  Outputs are pre-filled with a sentinel; the dead rows of the row operands hold NaN in the launch with liveness."""
    N, M = 384, B * rps
    x0, w, bias = rand((M, K), 11), rand((N, K), 12), rand((N,), 13, torch.float32)
    pre0 = rand((M, N), 14)
    base = nt_plain(x0, w, bias, tile, None) + nt_gelu_fwd(x0, w, bias, tile, None) + nt_gelu_bwd(x0, w, pre0, bias, tile, None)
    sent = torch.tensor(7.0, device=DEV)
    for name, scale in patterns(B).items():
        dead = rows_mask(scale, rps)
        dead_tiles = dead[::tile]
        live = (scale, rps)
        x, pre = x0.clone(), pre0.clone()
        x[dead] = float("nan")
        pre[dead] = float("nan")
        y, p, h, g, part = nt_plain(x, w, bias, tile, live) + nt_gelu_fwd(x, w, bias, tile, live) + nt_gelu_bwd(x, w, pre, bias, tile, live)
        for got, want, what in zip((y, p, h, g), base[:4], ("y", "pre", "h", "g")):
            assert equal(got[~dead], want[~dead]), (name, what)
        assert equal(y[dead], torch.zeros_like(y[dead])), name                          # EPI 0: zeros for the row kernels that follow
        for t, what in ((p, "pre"), (h, "h"), (g, "g")):
            assert equal(t[dead].float(), sent), (name, what)                           # unwritten: still the sentinel
        assert equal(part[~dead_tiles], base[4][~dead_tiles]) and equal(part[dead_tiles], torch.zeros_like(part[dead_tiles])), name
        if name == "none":                                                              # all live: bit-equal to the null-pointer launch
            for got, want in zip((y, p, h, g, part), base):
                assert torch.equal(bits(got), bits(want))


def test_tiled_gemm_rejects_tiles_that_straddle_samples():
    lib = _lib.load()
    M, K, N = 4 * 192, 192, 384
    x, w, y = torch.zeros(M, K, dtype=BF, device=DEV), torch.zeros(N, K, dtype=BF, device=DEV), torch.zeros(M, N, dtype=BF, device=DEV)
    s = torch.ones(4, device=DEV)
    assert lib.pswin_gemm_nt_live(ptr(x), ptr(w), None, ptr(y), M, K, N, 128, ptr(s), 192, None) == -1     # 192 % 128 != 0
    assert lib.pswin_gemm_nt_live(ptr(x), ptr(w), None, ptr(y), M, K, N, 64, ptr(s), 512, None) == -1      # 768 rows are not whole samples


# ---- the Mlp node ----------------------------------------------------------------------------------------------------------

def mlp_chain(x, w1, w1t, w2, w2t, b1, dout, live, poison):
    """The six products of _MlpFused through the C-ABI wrappers on buffers of the test's own (NaN-filled with `poison`)."""
    M, C = x.shape
    Nh = w1.shape[0]
    fill = float("nan") if poison else 0.0
    pre, h, g = (torch.full((M, Nh), fill, dtype=BF, device=DEV) for _ in range(3))
    out, dx = torch.full((M, C), fill, dtype=BF, device=DEV), torch.full((M, C), fill, dtype=BF, device=DEV)
    ws = torch.full((M // 64, Nh), fill, dtype=torch.float32, device=DEV)
    sfx, extra = ("", ()) if live is None else ("_live", (ptr(live[0]), live[1]))
    call("pswin_gemm_nt_gelu_fwd" + sfx, x, ptr(x), ptr(w1), ptr(b1), ptr(pre), ptr(h), M, C, Nh, 64, *extra)
    call("pswin_gemm_nt" + sfx, x, ptr(h), ptr(w2), None, ptr(out), M, Nh, C, 64, *extra)
    call("pswin_gemm_nt_gelu_bwd" + sfx, x, ptr(dout), ptr(w2t), ptr(pre), ptr(b1), ptr(g), ptr(ws), M, C, Nh, 64, *extra)
    call("pswin_gemm_nt" + sfx, x, ptr(g), ptr(w1t), None, ptr(dx), M, Nh, C, 64, *extra)
    _, _, dw2 = run_wgrad(dout, h, 1, live, bias=False)
    _, _, dw1 = run_wgrad(g, x, 1, live, bias=False)
    db1 = ops.sum_rows(ws, M // 64, Nh)
    return out, dx, dw1, db1, dw2


def test_mlp_products_on_poisoned_buffers():
    """M = 4 x 256, C = 192: pre, h and d(pre) start as NaN and stay NaN for dead samples; out, dx, dW1, db1, dW2 equal the unskipped
    chain fed the same dout (zeros in dead rows), with zeros in the dead rows of out and dx."""
    B, rps, C, Nh = 4, 256, 192, 768
    M = B * rps
    x, w1, w2, b1 = rand((M, C), 21), rand((Nh, C), 22) * 0.2, rand((C, Nh), 23) * 0.2, rand((Nh,), 24, torch.float32)
    w1t, w2t = w1.t().contiguous(), w2.t().contiguous()
    dout0 = rand((M, C), 25)
    assert ops.mlp_sample_skip(M, C, Nh, rps).fwd
    for name, scale in patterns(B).items():
        dead = rows_mask(scale, rps)
        dout = dout0.clone()
        dout[dead] = 0
        want = mlp_chain(x, w1, w1t, w2, w2t, b1, dout, None, False)
        got = mlp_chain(x, w1, w1t, w2, w2t, b1, dout, (scale, rps), True)
        # the unskipped chain computes out for dead samples (the row kernel multiplies it by zero afterwards); skipped: zeros
        assert equal(got[0][~dead], want[0][~dead]) and equal(got[0][dead], torch.zeros_like(got[0][dead])), name
        assert equal(got[1], want[1]) and equal(got[1][dead], torch.zeros_like(got[1][dead])), name
        for w, g_, what in zip(want[2:], got[2:], ("dW1", "db1", "dW2")):
            assert equal(w, g_), (name, what)


def test_mlp_node_with_the_switch_on_and_off(monkeypatch):
    B, rps, C, Nh = 4, 256, 192, 768
    M = B * rps
    fc1, fc2 = torch.nn.Linear(C, Nh).to(DEV), torch.nn.Linear(Nh, C).to(DEV)
    for lin in (fc1, fc2):
        lin.__dict__["_lowp"] = (lin.weight.detach().to(BF), None)
        lin.__dict__["_lowp_t"] = lin.weight.detach().to(BF).t().contiguous()
    x0 = rand((M, C), 31)
    dout0 = rand((M, C), 32)
    for name, scale in patterns(B).items():
        dead = rows_mask(scale, rps)
        res = {}
        for on in (True, False):
            monkeypatch.setattr(ops, "SAMPLE_SKIP", on)
            x = x0.clone().requires_grad_(True)
            for p in (*fc1.parameters(), *fc2.parameters()):
                p.grad = None
            out = ops.mlp_fused(x, fc1, fc2, scale, rps)
            dout = dout0.clone()
            dout[dead] = 0
            out.backward(dout)
            res[on] = (out.detach(), x.grad, fc1.weight.grad, fc1.bias.grad, fc2.weight.grad)
        assert equal(res[True][0][~dead], res[False][0][~dead]) and equal(res[True][0][dead], torch.zeros_like(res[True][0][dead])), name
        for a, b, what in zip(res[True][1:], res[False][1:], ("dx", "dW1", "db1", "dW2")):
            assert equal(a, b), (name, what)


# ---- model level --------------------------------------------------------------------------------------------------------------

CFG = dict(embed_dim=96, depths=[2, 2], num_heads=[3, 6], ape=True, drop_path_rate=0.5, out_indices=(0, 1))
SHAPE = (4, 3, 128, 256)                  # stage 1: 16 x 32 = 512 tokens per sample, C = 192: the tiled GEMMs and the ring kernel run


def _model():
    from panoswintransformerobjectdetection_amd import SimplePanoSwinTransformer
    torch.manual_seed(0)
    m = SimplePanoSwinTransformer(**CFG, window_size=7, pano_mode=True, compute_dtype=BF)
    m.init_weights(None)
    return m.to(DEV).train()


def _record_draws(m, store):
    """every DropPath draw of m lands in `store` (a list of [blocks, 2, B] stacks per pass, copied: also inside a captured graph)"""
    draw = m._draw_drop_path

    def wrapped(x):
        out = draw(x)
        store.append([s.clone() for s in out])
        return out
    m._draw_drop_path = wrapped


def _step(m, x, ws):
    for p in m.parameters():
        p.grad = None
    outs = m(x)
    loss = sum(o.float().flatten() @ w for o, w in zip(outs, ws))
    loss.backward()
    return [o.detach() for o in outs]


def _weights(m, x):
    with torch.no_grad():
        return [torch.linspace(-1, 1, o.numel(), device=DEV) / o.numel() ** 0.5 for o in m(x)]


def _assert_some_dead_some_live(draws):
    flat = torch.cat([s.reshape(-1) for step in draws for s in step])
    assert bool((flat == 0).any()) and bool((flat != 0).any())
    stage1 = torch.cat([step[1].reshape(-1) for step in draws])                    # where the Mlp and the weight gradients skip
    assert bool((stage1 == 0).any()) and bool((stage1 != 0).any())


def test_model_steps_are_equal_with_the_switch_on_and_off(monkeypatch):
    """Three steps of a two-stage model (B = 4, drop_path_rate 0.5) from the same seeds: same masks, equal outputs, equal parameter gradients."""
    assert ops.mlp_sample_skip(4 * 512, 192, 768, 512).fwd                         # stage 1 of this model skips in the forward pass
    m = _model()
    x = rand(SHAPE, 41, torch.float32)
    ws = _weights(m, x)
    prev = ops.set_deferred_reductions(ops.deferred_reductions_available())       # the grouped end-of-pass launch where torch has the hooks
    try:
        runs = {}
        for on in (True, False):
            monkeypatch.setattr(ops, "SAMPLE_SKIP", on)
            draws, steps = [], []
            _record_draws(m, draws)
            for i in range(3):
                torch.manual_seed(100 + i)
                outs = _step(m, x, ws)
                torch.cuda.synchronize()
                steps.append((outs, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
            del m._draw_drop_path
            runs[on] = (draws, steps)
    finally:
        ops.set_deferred_reductions(prev)
    _assert_some_dead_some_live(runs[True][0])
    for da, db in zip(runs[True][0], runs[False][0]):
        assert all(torch.equal(a, b) for a, b in zip(da, db))                      # the same seed gives the same masks
    for i, ((oa, ga), (ob, gb)) in enumerate(zip(runs[True][1], runs[False][1])):
        assert all(equal(a, b) for a, b in zip(oa, ob)), i
        assert ga.keys() == gb.keys()
        for n in ga:
            assert equal(ga[n], gb[n]), (i, n)


def test_captured_step_replays_equal_eager_steps_on_the_same_masks():
    """The step captured once and replayed three times (the masks are drawn inside the graph, the skipping follows them on the device)
    against eager steps that are handed each replay's masks."""
    from panoswintransformerobjectdetection_amd.graph import GraphedCallable
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m = _model()
        x = rand(SHAPE, 42, torch.float32)
        ws = _weights(m, x)
        draws = []
        _record_draws(m, draws)
        g = GraphedCallable(lambda: _step(m, x, ws), warmup=2, stream=side, parameters=[m])
        static_draw = draws[-1]                                                    # the capture's copies: refilled by every replay
        replays = []
        for _ in range(3):
            outs = g()
            side.synchronize()
            replays.append(([s.clone() for s in static_draw], [o.clone() for o in outs],
                            {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
        del m._draw_drop_path
        _assert_some_dead_some_live([r[0] for r in replays])
        for i, (masks, outs, grads) in enumerate(replays):
            m._draw_drop_path = lambda _x, masks=masks: masks
            want = _step(m, x, ws)
            side.synchronize()
            assert all(equal(a, b) for a, b in zip(outs, want)), i
            for n, p in m.named_parameters():
                if p.grad is not None:
                    assert equal(grads[n], p.grad), (i, n)
        del m._draw_drop_path
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
