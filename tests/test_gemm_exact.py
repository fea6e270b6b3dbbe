"""tests/_gemm_exact_cases.py on the CPU: every case tests/test_gemm_exact_gpu.py runs meets its class's conditions (sums below 2^24,
the tie and rounding shares, the 8-bit condition, no zero pre-activation), and a plain torch evaluation of the same operation gives
the builder's expected value -- the two ways of writing the expectation agree.  Also the float32 model of csrc/pswin_gelu.hpp from
which the bounds of the GPU sweep over every finite bf16 value are taken."""
import pytest
import torch
import torch.nn.functional as F

import _gemm_exact_cases as gc

BF16 = torch.bfloat16


def _plain_nt(case, with_bias):
    y = case["x"].float() @ case["w"].float().t()
    return y + case["bias"] if with_bias and case["bias"] is not None else y


@pytest.mark.parametrize("K", gc.NT_K)
@pytest.mark.parametrize("N", gc.NT_N)
def test_tiled_gemm_cases(K, N):
    for M in gc.NT_M:
        for cls in gc.NT_CLASSES:
            case = gc.nt_case(cls, M, K, N)
            for with_bias in (False, True):
                gc.nt_conditions(cls, case, with_bias)
                want = case["want"] + (case["bias"].double() if with_bias and case["bias"] is not None else 0.0)
                assert torch.equal(_plain_nt(case, with_bias).double(), want), (cls, M)
            if cls == "select_x":                      # each output names its source element
                assert torch.equal(case["want"][5], case["w"].double()[:, gc.walk(5, K)])
            if cls == "select_w":
                assert torch.equal(case["want"][:, 5], case["x"].double()[:, gc.walk(5, K)])
        assert set(int(gc.walk(m, K)) for m in range(max(M, K))) == set(range(K)) or M < K     # 7 is coprime to every K here


@pytest.mark.parametrize("M,K,N,tile_m", gc.NT_DEEP)
def test_tiled_gemm_cases_above_the_four_stage_threshold(M, K, N, tile_m):
    assert gc.nt_form(M, K, N, tile_m) == "two-stage" and K // 64 >= 3 and -(-M // tile_m) * (N // 192) > 256
    for cls in ("dense", "ties", "select_x"):
        case = gc.nt_case(cls, M, K, N)
        gc.nt_conditions(cls, case, True)
        assert torch.equal(_plain_nt(case, False).double(), case["want"]), cls


def test_the_launcher_rule_puts_the_small_shapes_where_the_docstrings_say():
    for tile_m in (64, 96, 128):
        for M in gc.NT_M:
            for N in gc.NT_N:
                assert all(gc.nt_form(M, K, N, tile_m) == "two-stage" for K in (64, 128))
                assert all(gc.nt_form(M, K, N, tile_m) == "four-stage" for K in (192, 256, 3072))


@pytest.mark.parametrize("K,N", gc.SKINNY_KN)
def test_streaming_gemm_cases(K, N):
    for M in gc.STREAM_M:
        for cls in gc.NT_CLASSES:
            case = gc.nt_case(cls, M, K, N)
            gc.nt_conditions(cls, case, True)
            assert torch.equal(_plain_nt(case, True).double(), case["want"] + (0.0 if case["bias"] is None else case["bias"].double()))
    # the transposed-weight form of shape (K, N) serves the Linear of shape (N, K): the six shapes are closed under the swap, so each has both
    assert (N, K) in gc.SKINNY_KN


@pytest.mark.parametrize("N,K", gc.TN_SHAPES)
def test_ring_cases(N, K):
    assert gc.tn_geom(N, K) == (0 if K >= 192 and N >= 192 else 1 if K == 96 else 2)
    for M in gc.TN_M:
        assert gc.tn_splits(M)[0] == 1 and gc.tn_splits(M)[-1] == max(1, M // 64)
        for sp in gc.tn_splits(M):
            for cls in ("dense", "ties"):
                case = gc.tn_case(cls, M, N, K, sp)
                gc.tn_conditions(cls, case)
                dy, x = case["dy"].float(), case["x"].float()
                assert torch.equal((dy.t() @ x).double(), case["want"].sum(0))              # the splits partition the rows
                lo, hi = case["ranges"][-1]
                assert torch.equal((dy[lo:hi].t() @ x[lo:hi]).double(), case["want"][-1])
                db = dy.sum(0).double()
                db[case["zero_cols"][0]:case["zero_cols"][1]] = 0
                assert torch.equal(db, case["want_db"].sum(0))
    # the cases hold a split with fewer than three slabs and one that begins past M
    assert gc.tn_rows_per_split(130, 2) == 128 and gc.tn_ranges(130, 2)[1] == (128, 130)
    assert gc.tn_ranges(333, 5)[3] == (333, 333) and gc.tn_ranges(4033, 63)[32] == (4033, 4033) and gc.tn_ranges(1000, 15)[8] == (1000, 1000)


def test_ring_group_cases():
    assert sorted(gc.TN_GROUP_ORDER) == list(range(len(gc.TN_GROUP))) and {gc.tn_geom(j[1], j[2]) for j in gc.TN_GROUP} == {0, 1, 2}
    for M, N, K, sp, cls, _, _ in gc.TN_GROUP:
        assert 1 <= sp <= M // 64
        gc.tn_conditions(cls, gc.tn_case(cls, M, N, K, sp))


def _saturated_gelu(v):
    """F.gelu's value where it is saturated: v for v >= 15, -0 for v <= -15 (and what the float64 definition gives to 1e-40)"""
    assert float(v.abs().min()) >= 15
    h = torch.where(v > 0, v, torch.zeros_like(v))
    assert float((F.gelu(v.double()) - h.double()).abs().max()) < 1e-40
    return h


@pytest.mark.parametrize("M,C", gc.MLP_NT + (gc.MLP_NT_RING,) + tuple((M, 96) for M in gc.STREAM_M))
def test_saturated_mlp_cases(M, C):
    c = gc.mlp_case(M, C)
    gc.mlp_conditions(c)
    # the torch definition with F.gelu replaced by its saturated value, autograd for the gradients
    x = c["x"].double().requires_grad_(True)
    w1, w2 = c["w1"].double().requires_grad_(True), c["w2"].double().requires_grad_(True)
    b1 = c["b1"].double().requires_grad_(True)
    pre = x @ w1.t()
    v = pre + b1
    h = v * (_saturated_gelu(v.detach()) != 0).double()            # d gelu / dv = [v > 0] where saturated
    out = h @ w2.t()
    out.backward(c["dout"].double())
    assert torch.equal(pre.detach(), c["pre"]) and torch.equal(h.detach(), c["h"]) and torch.equal(out.detach(), c["out"])
    assert torch.equal(h.detach(), _saturated_gelu(v.detach()))
    assert torch.equal(x.grad, c["dx"]) and torch.equal(w1.grad, c["dw1"]) and torch.equal(b1.grad, c["db1"]) and torch.equal(w2.grad, c["dw2"])
    for rows in (64, 128):
        ts = gc.tile_sums(c["dpre"], rows)
        assert ts.shape[0] == -(-M // rows) and torch.equal(ts.sum(0), c["db1"])
    # the kernels' own float32 formula is saturated on these pre-activations: exactly v or (-)0, exactly 1 or 0
    gl, gr = gc.gelu_model_f32(c["v"].float().reshape(-1))
    assert torch.equal(gl.double(), c["h"].reshape(-1)) and torch.equal(gr.double(), (c["v"] > 0).double().reshape(-1))


@pytest.mark.parametrize("N", gc.BIAS_GELU_N)
@pytest.mark.parametrize("M", gc.BIAS_GELU_M)
def test_saturated_bias_gelu_cases(M, N):
    c = gc.bias_gelu_case(M, N)
    v = c["v"]
    assert bool(((v / 16) % 2 == 1).all()) and float(v.abs().max()) <= 240
    for k in ("y", "dh", "v", "h", "dy"):
        assert bool(gc.fits_bf16(c[k]).all())
    assert torch.equal(c["h"], _saturated_gelu(c["y"] + c["b"].double())) and torch.equal(c["db"], c["dy"].sum(0))
    gl, gr = gc.gelu_model_f32(v.float().reshape(-1))
    assert torch.equal(gl.double(), c["h"].reshape(-1)) and torch.equal(gr.double() * c["dh"].reshape(-1), c["dy"].reshape(-1))


def test_bit_helpers():
    t = torch.tensor([0.0, 1.0, 255.0, 256.0, 257.0, 511.0, 512.0, 514.0, 516.0, 1026.0, -257.0, 3.0 * 2 ** 20])
    assert gc.fits_bf16(t).tolist() == [True, True, True, True, False, False, True, False, True, False, False, True]
    assert gc.is_tie(t).tolist() == [False, False, False, False, True, True, False, True, False, False, True, False]
    # RNE on ties: to the even neighbour, both ways
    assert gc.rne_bf16(torch.tensor([257.0, 259.0, 514.0, 518.0, -257.0])).tolist() == [256.0, 260.0, 512.0, 520.0, -256.0]
    r = gc.random_bf16(gc.gen(1), (4096,)).double()
    assert bool(torch.isfinite(r).all()) and float(r.abs().min()) >= 2.0 ** -20 and float(r.abs().max()) < 2.0 ** 21
    assert bool((r < 0).any()) and bool((r > 0).any())


def test_gelu_model_error_is_where_the_gpu_bounds_come_from():
    v = gc.all_finite_bf16()
    assert v.numel() == 65280 == 8160 * 8
    gl, gr = gc.gelu_model_f32(v)
    fwd, grad = gc.gelu_errors(gl, gr, v)
    assert fwd <= gc.MODEL_FWD_REL and grad <= gc.MODEL_GRAD_ABS, (fwd, grad)
    assert gc.GELU_FWD_REL == 2 * gc.MODEL_FWD_REL and gc.GELU_GRAD_ABS == 2 * gc.MODEL_GRAD_ABS
    # saturation, exactly: the values the `saturated` class rests on
    s = torch.tensor([14.0, -14.0, 15.0, -15.0, 16.0, -16.0, 48.0, -240.0, 0.0])
    gl, gr = gc.gelu_model_f32(s)
    assert gl[2:].tolist() == [15.0, 0.0, 16.0, 0.0, 48.0, 0.0, 0.0] and gr[2:8].tolist() == [1.0, 0.0, 1.0, 0.0, 1.0, 0.0]
