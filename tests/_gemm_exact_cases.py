"""Operands on which the GEMM and GELU kernels have ONE right answer, and that answer (CPU only; tests/test_gemm_exact.py checks
the conditions below, tests/test_gemm_exact_gpu.py runs the kernels).

The kernels multiply bf16 and accumulate in f32.  With small-integer operands every partial sum is an integer below 2^24 in any
summation order, so the correct f32 result is one exact number and the correct bf16 result is its round-to-nearest-even.  Classes:

  dense      activations in {-1, 0, 1}, weights in {-2 .. 2}, bias an f32 integer in [-8, 8]
  ties       the same with the weights of every other contraction index scaled by 2^s: the product is 2^s A + B with two independent
             small integers, so that many outputs exceed 256 and a good share of them are exact bf16 ties (an odd integer in
             [256, 512) and its analogues in higher binades) -- what tells RNE from half-away and from truncation.  (Scaling ALL
             weights by 2^s would shift every output by s bits and change no rounding.)
  select     one operand one-hot per row at a position that walks the contraction, the other arbitrary finite bf16 bit patterns of
             magnitude 2^-20 .. 2^20: every output is a bit copy of one operand element
  saturated  for everything with a GELU: pre-activations 16 * odd with |v| <= 240.  In the kernels' formula (csrc/pswin_gelu.hpp)
             exp2(-v^2 * 0.7213) is below 2^-150 for |v| >= 15, i.e. 0 in any rounding, so gelu(v) is exactly v or -0 and gelu'(v)
             exactly 1 or 0; every intermediate has at most 8 significant bits, so no bf16 rounding anywhere changes a value

Everything is built from a seeded torch.Generator; expected values are float64 (exact for these integers).
"""
import math

import numpy as np
import torch

BF16 = torch.bfloat16
LIMIT = float(2 ** 24)


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def ints(g, shape, lo, hi):
    """float64 integers uniform in [lo, hi]"""
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def rne_bf16(t):
    """the round-to-nearest-even bf16 of exact values below 2^24 (f32 holds them exactly, torch's cast rounds to nearest even)"""
    return t.float().to(BF16)


def odd_part(t):
    """|v| with its trailing zero bits removed (0 for 0), int64: the integer's significant bits"""
    v = t.abs().to(torch.int64)
    low = (v & -v).clamp_min(1)
    return v // low


def fits_bf16(t):
    """at most 8 significant bits: exact in bf16"""
    return odd_part(t) < 256


def is_tie(t):
    """exactly 9 significant bits: halfway between two bf16 values"""
    o = odd_part(t)
    return (o >= 256) & (o < 512)


def sums_bounded(a, b):
    """max over outputs of sum_k |a[m, k]| |b[n, k]|: every partial sum of a . b^T, in any order, is bounded by it"""
    return float((a.abs().double() @ b.abs().double().t()).max())


def tie_scale(n_contract):
    """s for the `ties` class: half of the contraction carries 2^s; 2^s times the standard deviation of that half's sum
    (sqrt(n / 2 * 4 / 3) for {-1, 0, 1} x {-2 .. 2}) is about 400, so that most outputs lie in [256, 1024)"""
    std = math.sqrt(max(n_contract, 2) / 2 * 4 / 3)
    return max(0, round(math.log2(400.0 / std)))


def random_bf16(g, shape):
    """arbitrary finite non-zero bf16 bit patterns: random sign and mantissa, exponent 2^-20 .. 2^20"""
    sign = torch.randint(0, 2, shape, generator=g)
    expo = torch.randint(127 - 20, 127 + 20 + 1, shape, generator=g)
    mant = torch.randint(0, 128, shape, generator=g)
    bits = (sign << 15) | (expo << 7) | mant
    return (bits - (sign << 16)).to(torch.int16).view(BF16)           # the 16-bit pattern as a signed int16


def walk(i, K):
    """the one-hot position of row i"""
    return (7 * i + 3) % K


# ---------------------------------------------------------------------------------------------------------------------
# y[M, N] = x[M, K] . w[N, K]^T (+ bias): the tiled GEMM and the streaming GEMM
# ---------------------------------------------------------------------------------------------------------------------
NT_CLASSES = ("dense", "ties", "select_x", "select_w")


def nt_case(cls, M, K, N, seed=0):
    """-> dict(x bf16 [M, K], w bf16 [N, K], bias f32 [N] or None, want float64 [M, N] WITHOUT bias, scale).
    select_x: x one-hot, y[m, n] = w[n, walk(m)];  select_w: w one-hot, y[m, n] = x[m, walk(n)]; neither takes a bias."""
    g = gen(1000003 * seed + 7919 * M + 31 * K + N + NT_CLASSES.index(cls))
    if cls in ("dense", "ties"):
        x = ints(g, (M, K), -1, 1)
        w = ints(g, (N, K), -2, 2)
        s = tie_scale(K) if cls == "ties" else 0
        if s:
            w[:, 0::2] *= 2.0 ** s
        bias = ints(g, (N,), -8, 8)
        assert sums_bounded(x, w) + 8 < LIMIT
        want = x @ w.t()
        return dict(x=x.to(BF16), w=w.to(BF16), bias=bias.float(), want=want, scale=s)
    if cls == "select_x":
        w = random_bf16(g, (N, K))
        pos = walk(torch.arange(M), K)
        x = torch.zeros(M, K, dtype=BF16)
        x[torch.arange(M), pos] = 1.0
        return dict(x=x, w=w, bias=None, want=w.double()[:, pos].t().contiguous(), scale=0)
    assert cls == "select_w"
    x = random_bf16(g, (M, K))
    pos = walk(torch.arange(N), K)
    w = torch.zeros(N, K, dtype=BF16)
    w[torch.arange(N), pos] = 1.0
    return dict(x=x, w=w, bias=None, want=x.double()[:, pos].contiguous(), scale=0)


def nt_conditions(cls, case, with_bias):
    """the class's own conditions on a built case (asserts); -> (tie outputs, share of outputs that need rounding)"""
    want = case["want"] + (case["bias"].double() if with_bias and case["bias"] is not None else 0.0)
    assert bool(torch.isfinite(want).all())
    if cls.startswith("select"):
        assert bool((want != 0).all()) and bool((want.float().to(BF16).double() == want).all())      # bit copies of bf16 values
        assert float(want.abs().min()) >= 2.0 ** -20 and float(want.abs().max()) < 2.0 ** 21
        return 0, 0.0
    assert bool((want == want.round()).all()) and float(want.abs().max()) < LIMIT
    ties, share = int(is_tie(want).sum()), float((~fits_bf16(want)).double().mean())
    if cls == "ties":
        assert ties >= 64 and share >= 0.10, (ties, share)
    return ties, share


# the tiled GEMM's launcher rule (csrc/pswin_gemm_nt.hip: launch_nt, DEEP_TILES = 256, BN = 192, BK = 64), written out so that every
# test can say which loop its shape runs
def nt_form(M, K, N, tile_m):
    tiles = -(-M // tile_m) * (N // 192)
    return "four-stage" if (tiles <= 256 and K // 64 >= 3) else "two-stage"


NT_M = (64, 65, 127, 129, 191, 193, 333)
NT_K = (64, 128, 192, 256, 3072)
NT_N = (192, 768)
# (M, K, N, tile_m): more than 256 tiles (264, 264, 260), so the two-stage loop runs with K / 64 >= 3
NT_DEEP = ((4161, 192, 768, 64), (4161, 3072, 768, 64), (8200, 192, 768, 128))

SKINNY_KN = ((96, 288), (96, 96), (96, 384), (288, 96), (384, 96), (192, 192))
STREAM_M = (16, 63, 64, 333)


# ---------------------------------------------------------------------------------------------------------------------
# part[s] = dy[rows of split s]^T . x[rows of split s]: the ring weight-gradient kernel
# ---------------------------------------------------------------------------------------------------------------------
TN_SHAPES = ((192, 192), (384, 576), (48, 96), (64, 96), (80, 96), (208, 96), (368, 96), (384, 96), (96, 384))      # (N, K)
TN_M = (64, 65, 130, 333, 1000, 4033)


def tn_geom(N, K):
    """ring_geom of csrc/pswin_gemm_tn.hip"""
    if N >= 192 and K >= 192 and N % 192 == 0 and K % 192 == 0:
        return 0
    if K == 96 and 48 <= N <= 384 and N % 16 == 0:
        return 1
    if K == 384 and N == 96:
        return 2
    return -1


def tn_splits(M):
    """{1, 2, 3, M // 64} as far as the entry point accepts them (1 <= splits <= M / 64)"""
    return sorted({s for s in (1, 2, 3, M // 64) if 1 <= s <= M // 64})


def tn_rows_per_split(M, splits):
    """launch_tn_jobs: ceil(M / splits) rounded up to whole 64-row slabs"""
    return -(-(-(-M // splits)) // 64) * 64


def tn_ranges(M, splits):
    rows = tn_rows_per_split(M, splits)
    return [(min(s * rows, M), min((s + 1) * rows, M)) for s in range(splits)]


def tn_zero_cols(N):
    return (N // 3 // 16 * 16, 2 * (N // 3) // 16 * 16)


def tn_case(cls, M, N, K, splits, seed=0):
    """-> dict(dy bf16 [M, N] in {-1, 0, 1}, x bf16 [M, K], want float64 [splits, N, K], want_db float64 [splits, N] with the
    tn_zero_cols range zeroed, ranges, scale).  ties: every other ROW of x (the contraction index) carries 2^s."""
    g = gen(1000003 * seed + 7919 * M + 31 * K + N + 131 * splits + (cls == "ties"))
    dy = ints(g, (M, N), -1, 1)
    x = ints(g, (M, K), -2, 2)
    ranges = tn_ranges(M, splits)
    s = tie_scale(min(tn_rows_per_split(M, splits), M)) if cls == "ties" else 0
    if s:
        x[0::2] *= 2.0 ** s
    assert float(x.abs().max()) * M < LIMIT
    want = torch.zeros(splits, N, K, dtype=torch.float64)
    want_db = torch.zeros(splits, N, dtype=torch.float64)
    zlo, zhi = tn_zero_cols(N)
    for i, (lo, hi) in enumerate(ranges):
        if hi > lo:
            want[i] = dy[lo:hi].t() @ x[lo:hi]
            want_db[i] = dy[lo:hi].sum(0)
    want_db[:, zlo:zhi] = 0
    return dict(dy=dy.to(BF16), x=x.to(BF16), want=want, want_db=want_db, ranges=ranges, scale=s, zero_cols=(zlo, zhi))


def tn_conditions(cls, case):
    want = case["want"]
    assert bool((want == want.round()).all()) and float(want.abs().max()) < LIMIT
    live = torch.tensor([hi > lo for lo, hi in case["ranges"]])
    assert bool((want[~live] == 0).all())
    ties, share = int(is_tie(want).sum()), float((~fits_bf16(want[live])).double().mean())
    if cls == "ties":
        assert ties >= 64 and share >= 0.10, (ties, share)
    return ties, share


# (M, N, K, splits, class, bf16 slabs, bias sums) of the grouped launch: the three geometries, ragged M, a split past M, both slab types
TN_GROUP = ((1000, 384, 576, 15, "ties", True, True), (333, 192, 192, 3, "dense", False, False), (4033, 208, 96, 63, "ties", True, True),
            (130, 64, 96, 2, "dense", False, True), (1000, 96, 384, 3, "ties", True, False), (65, 368, 96, 1, "dense", False, True),
            (333, 80, 96, 5, "ties", False, True), (64, 192, 192, 1, "dense", True, False))
TN_GROUP_ORDER = (5, 2, 7, 0, 3, 6, 1, 4)           # the order the jobs are listed in


# ---------------------------------------------------------------------------------------------------------------------
# The Mlp with a saturated GELU: fc1 -> bias + GELU -> fc2 and all its gradients
# ---------------------------------------------------------------------------------------------------------------------
MLP_NT = ((65, 192), (333, 192), (200, 768))          # (M, C), hidden = 4 C: the tiled GEMM's GELU forms
MLP_NT_RING = (577, 192)                              # one more for the autograd nodes: M >= 512, their weight gradients run on the ring kernel


def mlp_case(M, C, seed=0):
    """Operands and the exact integer chain of out = relu-saturated-gelu(x W1^T + b1) W2^T with upstream gradient dout:
    x [M, C] (at most three +-1 per row at walking positions), w1 [4C, C] in 32 {-2 .. 2}, b1 f32 in 16 {-3, -1, 1, 3},
    w2 [C, 4C] in {-1, 0, 1}, dout [M, C] in {-1, 0, 1}; float64: pre (without bias), v = pre + b1, h, out, dh, dpre, db1, dw1, dw2, dx."""
    N = 4 * C
    g = gen(1000003 * seed + 7919 * M + C)
    x = torch.zeros(M, C, dtype=torch.float64)
    rows = torch.arange(M)
    for a, b in ((7, 3), (11, 5), (13, 1)):
        x[rows, (a * rows + b) % C] = ints(g, (M,), -1, 1)          # (a later position may overwrite an earlier one: still <= 3 non-zeros)
    w1 = 32.0 * ints(g, (N, C), -2, 2)
    b1 = 16.0 * (2.0 * ints(g, (N,), -2, 1) + 1.0)
    w2 = ints(g, (C, N), -1, 1)
    dout = ints(g, (M, C), -1, 1)
    pre = x @ w1.t()
    v = pre + b1
    on = (v > 0).double()
    h = v * on
    out = h @ w2.t()
    dh = dout @ w2
    dpre = dh * on
    c = dict(M=M, C=C, N=N, x=x.to(BF16), w1=w1.to(BF16), b1=b1.float(), w2=w2.to(BF16), dout=dout.to(BF16),
             pre=pre, v=v, h=h, out=out, dh=dh, dpre=dpre, db1=dpre.sum(0), dw1=dpre.t() @ x, dw2=dout.t() @ h, dx=dpre @ w1)
    assert max(sums_bounded(h, w2), sums_bounded(dpre, w1.t()), sums_bounded(dpre.t(), x.t()), sums_bounded(dout.t(), h.t())) < LIMIT
    return c


def mlp_conditions(c):
    """every pre-activation is 16 * odd with 16 <= |v| <= 240, and no intermediate needs more than 8 significant bits"""
    v = c["v"]
    assert bool(((v / 16) % 2 == 1).all()) and float(v.abs().min()) >= 16 and float(v.abs().max()) <= 240
    assert int((c["x"] != 0).sum(1).max()) <= 3
    for k in ("pre", "v", "h", "dh", "dpre"):
        assert bool(fits_bf16(c[k]).all()), k
    for k in ("out", "db1", "dw1", "dw2", "dx"):
        assert float(c[k].abs().max()) < LIMIT


def tile_sums(t, rows_per_tile):
    """float64 [ceil(M / rows_per_tile), N]: the column sums over exactly the rows [r t, min(r (t + 1), M)) of each tile"""
    M = t.shape[0]
    return torch.stack([t[lo:min(lo + rows_per_tile, M)].sum(0) for lo in range(0, M, rows_per_tile)])


# the streaming kernels' row blocks (csrc/pswin_gemm.hip): a workgroup of pswin_fc1_gelu_bwd owns 4 waves x 16 rows, one of
# pswin_mlp0_bwd 8 waves x 16 rows, each ONE trip at these M (grids far below MAX_GRID / M0_MAX_GRID)
FC1_BWD_ROWS, MLP0_BWD_ROWS = 64, 128

BIAS_GELU_N = (8, 96, 3072)
BIAS_GELU_M = (1, 5, 333)


def bias_gelu_case(M, N, seed=0):
    """y [M, N] in 32 {-3 .. 3}, bias f32 in 16 {-3, -1, 1, 3}, dh in {-3 .. 3}: y + bias = 16 * odd; float64 v, h, dy, db"""
    g = gen(1000003 * seed + 7919 * M + N)
    y = 32.0 * ints(g, (M, N), -3, 3)
    b = 16.0 * (2.0 * ints(g, (N,), -2, 1) + 1.0)
    dh = ints(g, (M, N), -3, 3)
    v = y + b
    on = (v > 0).double()
    return dict(y=y, b=b.float(), dh=dh, v=v, h=v * on, dy=dh * on, db=(dh * on).sum(0))


# ---------------------------------------------------------------------------------------------------------------------
# The GELU itself over every finite bf16 value
# ---------------------------------------------------------------------------------------------------------------------
def all_finite_bf16():
    """the 65 280 finite bf16 values in bit order, as f32"""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    v = bits.view(BF16).float()
    return v[torch.isfinite(v)]


def gelu_ref64(v):
    """float64 v Phi(v) and its derivative"""
    x = v.double()
    cdf = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
    return x * cdf, cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_model_f32(v):
    """csrc/pswin_gelu.hpp evaluated in float32 on the CPU with IEEE division and libm exp2 (f32 results below 2^-126 flushed):
    -> (gelu, gelu') as float32 tensors.  The kernel differs by its 1-ulp hardware reciprocal and exp2."""
    f = np.float32
    x = v.numpy().astype(f)
    with np.errstate(all="ignore"):
        z = np.abs(x) * f(0.70710678118654752440)
        t = (f(1.0) / (f(0.3275911) * z + f(1.0))).astype(f)
        E = np.exp2((x * x * f(-0.72134752044448170368)).astype(f)).astype(f)
        E = np.where(np.abs(E) < f(2.0 ** -126), f(0), E)
        p = f(1.061405429) * t + f(-1.453152027)
        p = p * t + f(1.421413741)
        p = p * t + f(-0.284496736)
        p = p * t + f(0.254829592)
        tail = f(0.5) * p * t * E
        cdf = np.where(x >= 0, f(1.0) - tail, tail).astype(f)
        gl = (x * cdf).astype(f)
        gr = (x * f(0.39894228040143267794) * E + cdf).astype(f)
    return torch.from_numpy(gl), torch.from_numpy(gr)


GELU_SWEEP_LIMIT = 1e18                     # |v| below it: v * v stays finite in f32
# forward: |h - ref| <= GELU_FWD_REL |v| + 2^-23 |ref|;  gradient: |g - ref| <= GELU_GRAD_ABS.  Twice the f32 CPU model's own maxima
# (MODEL_*: 0.75e-7 of it is Abramowitz-Stegun 7.1.26, the rest f32 rounding), the factor for the hardware reciprocal and exp2
GELU_FWD_REL, GELU_GRAD_ABS = 5e-7, 5.4e-7
MODEL_FWD_REL, MODEL_GRAD_ABS = 2.5e-7, 2.7e-7


def gelu_errors(h, g, v):
    """(max |h - ref| / |v|, max |g - ref|) over the sweep's checked values (0 < |v| < GELU_SWEEP_LIMIT), float64"""
    ref, refg = gelu_ref64(v)
    ok = (v.double().abs() < GELU_SWEEP_LIMIT) & (v != 0)
    return float(((h.double() - ref).abs()[ok] / v.double().abs()[ok]).max()), float((g.double() - refg).abs()[ok].max())
