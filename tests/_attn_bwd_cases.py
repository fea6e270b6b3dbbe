"""Inputs, float64 model and rules for the window-attention backward tests (tests/test_attention_backward_cases.py on the CPU,
tests/test_attention_backward_gpu.py on the MI355X).

The backward kernels of csrc/pswin_attn.hip (bf16: attn_bwd_pair_kernel, two waves per (window, head); f32: attn_bwd_kernel<PSWIN_F32, 3>)
take the forward pass's log-sum-exp rows as an INPUT and recompute the weights from them (pswin_attn.hip:388-408, :652-671):

    s'    = q.k + bias / scale                 (f32, the MFMA's C operand is the bias)
    p     = exp2(fma(s', scale * log2 e, -lse * log2 e))
    dP    = dO.V^T
    delta = sum_j p * dP                       (f32, from the UNROUNDED p)
    dS    = p * (dP - delta)
    dV    = rnd(P)^T.dO      dK = (rnd(dS)^T.Q) * scale      dQ = (rnd(dS).K) * scale         (rnd: bf16 in the bf16 kernel)
    gsum  = sum over the windows of a work item of dS, unrounded, stored as a transposed [key j][query i] 64 x 64 tile

backward64 states these formulas once.  Two classes of input follow from them.

The exact class.  The test supplies lse = 0 for the 49 real rows and operands for which every s' is exactly 0 or hugely negative: q has
its four +-1 entries in head dims 0..15, k in dims 16..31, so q.k = 0 exactly while neither is zero, and bias is 0 or a sum of -30000s.
Then p = exp2(+-0) = 1 or exp2(-43000 ..) = 0: the weight matrix P is an ARBITRARY 0 / 1 matrix the test chose (no softmax: rows sum to
0 .. 49), every intermediate is a small integer (|dP| <= 4, |delta| <= 196, |dS| <= 200: exact in bf16 and f32, whatever the order of the
additions), and the only roundings are the final `* scale` (one f32 multiply of an integer below 2^24) and the bf16 store.  The float64
model reproduces both, so dq, dk, dv, the raw gsum tiles and the table gradients have ONE right answer each.  P comes from four
families, each through another transposed fetch of the backward bias build (bias_fetch<true>, bias_lookup<true>):
    mask   planar, beta = 0, non-symmetric mask tiles of 0 / -30000 with one all-zero and one all-one row of P planted per tile
    beta   planar, no mask, beta[idx, h] in {0, -30000}, another pattern per head
    dist   pano, non-symmetric distance tiles of 0 / 1, alpha[idx, h] in {0, -30000}, beta = 0
    all    the three together

The dense class: random bf16-exact q, k, v, dO with lse = float32(logsumexp64(scores)); judged against the float64 truth T by the error
of a rounding model E (bf16 dq, dk, dv) or of the float32 evaluation of the same formulas (everything else), see `within32`."""
import math

import numpy as np
import torch

import _attn_edge_cases as ec
import panoswin_oracle as po
from _cascade_cases import ulp32
from detfill import det_uniform

TOK, PAD, HD, NBINS = 49, 64, 32, 169
OFF = -30000.0
SCALE = 32 ** -0.5
SCALE32 = float(np.float32(SCALE))                  # the operand the kernels receive (`float scale`)
FAMILIES = ("mask", "beta", "dist", "all")
# (n_rep, nW, heads, chunks, tables): n = n_rep * nW windows; tables = "window": nb = nW bias windows with a mask / distance tile each,
# "each": nb = n (per-window tables, one image per work item), "shared": nb = nW with ONE mask tile and ONE distance tile (wb % n_mask)
EXACT = [(1, 1, 1, 1, "window"), (2, 3, 3, 1, "window"), (4, 3, 2, 2, "window"), (4, 1, 1, 4, "window"), (3, 2, 4, 1, "window"),
         (2, 3, 2, 1, "each"), (2, 3, 2, 2, "shared"), (1, 2, 6, 1, "window")]       # the last: C = 192, a width the fused forward saves packed
# the dense cases (n_rep, nW, heads, pano, mask_kind, chunks): ec.CORE_RANDOM with one work item per window, and one with a batch loop
DENSE = [c + (1 if c[4] == 4 else c[0],) for c in ec.CORE_RANDOM] + [(4, 3, 2, True, 3, 1)]     # (a per-window mask: nb = n, one image each)


def rel_index():
    """[49, 49] long: the table bin of the pair (query i, key j)"""
    return po.relative_position_index(7)


def f32_round(t):
    return t.to(torch.float32).to(torch.float64)


def heads_first(t, heads):
    """[n * 49, heads * 32] or [n, 49, heads * 32] -> [n, heads, 49, 32]"""
    return t.reshape(-1, TOK, heads, HD).permute(0, 2, 1, 3)


def rows_of(t):
    """[n, heads, 49, 32] -> [n * 49, heads * 32]"""
    n, heads = t.shape[:2]
    return t.permute(0, 2, 1, 3).reshape(n * TOK, heads * HD)


def packed_of(q, k, v, heads):
    """three [n * 49, C] -> [n, heads, 3, 49, 32]: what the fused forward kernels save"""
    return torch.stack([heads_first(t, heads) for t in (q, k, v)], 2).contiguous()


# ---- the formulas -----------------------------------------------------------------------------------------------------------------------------
def backward64(q, k, v, dout, bias_over_scale, lse, scale, rnd=None, dtype=torch.float64, mutant=None):
    """q, k, v, dout [n, heads, 49, 32]; bias_over_scale broadcastable to [n, heads, 49, 49]; lse [n, heads, 49] -> (dq, dk, dv, dS).
    rnd = None: the truth; rnd = ec.bf16_round: the bf16 kernel's rounding points (P and dS as MFMA operands, the three outputs);
    dtype = float32: the float32 definition.  mutant: a planted defect, for the CPU tests only."""
    c = lambda t: t.to(dtype)
    r = (lambda t: t) if rnd is None else (lambda t: rnd(t).to(dtype))
    q, k, v, dout, lse = c(q), c(k), c(v), c(dout), c(lse)
    s = q @ k.transpose(-2, -1) + c(bias_over_scale)
    p = torch.exp(s * scale - lse[..., None])
    dp = dout @ v.transpose(-2, -1)
    delta = ((r(p) if mutant == "delta_from_rounded_p" else p) * dp).sum(-1, keepdim=True)
    if mutant == "delta_shifted":
        delta = delta.roll(1, -2)
    ds = p * (dp - delta)
    dsr = r(ds)
    dv = r(p).transpose(-2, -1) @ dout
    dk = dsr.transpose(-2, -1) @ q
    if mutant != "dk_unscaled":
        dk = dk * scale
    dq = ((dsr.transpose(-2, -1) if mutant == "ds_not_transposed" else dsr) @ k) * scale
    return r(dq), r(dk), r(dv), ds


def table_grads(ds, dist, n_tiles):
    """ds [n, heads, 49, 49], dist [n_tiles, 49, 49] or None (window w uses tile w % n_tiles: the bias window is w % nb and nb is a
    multiple of n_tiles) -> (dalpha or None, dbeta) [169, heads] in ds's dtype: dbeta[idx, h] = sum dS, dalpha[idx, h] = sum dS * dist"""
    n, heads = ds.shape[:2]
    idx = rel_index().reshape(-1)
    per_pair = lambda t: t.sum(0).reshape(heads, TOK * TOK).T.contiguous()
    dbeta = torch.zeros(NBINS, heads, dtype=ds.dtype).index_add_(0, idx, per_pair(ds))
    if dist is None:
        return None, dbeta
    d = dist.to(ds.dtype)[torch.arange(n) % n_tiles][:, None]
    return torch.zeros(NBINS, heads, dtype=ds.dtype).index_add_(0, idx, per_pair(ds * d)), dbeta


def gsum_expected(ds, n_rep, nW, chunks, interleaved=False):
    """ds [n_rep * nW, heads, 49, 49] -> [chunks * nW, heads, 64, 64]: per work item (chunk, bias window wb, head) the sum of dS over its
    n_rep / chunks windows, window (chunk * reps_per_chunk + r) * nW + wb (pswin_attn.hip:359 / :631), as a transposed [j][i] tile that
    is zero beyond 49.  nW = the number of bias windows, n_rep = windows per bias window.  interleaved: the WRONG window order
    (r * chunks + chunk), for the CPU tests."""
    assert n_rep % chunks == 0 and ds.shape[0] == n_rep * nW
    heads, rpc = ds.shape[1], n_rep // chunks
    out = torch.zeros(chunks * nW, heads, PAD, PAD, dtype=ds.dtype)
    for chunk in range(chunks):
        for r in range(rpc):
            rep = r * chunks + chunk if interleaved else chunk * rpc + r
            for wb in range(nW):
                out[chunk * nW + wb, :, :TOK, :TOK] += ds[rep * nW + wb].transpose(-2, -1)
    return out


# ---- the exact class --------------------------------------------------------------------------------------------------------------------------
def _signed4(rows, lo, hi, tag):
    """[rows, 32] float32 with four +-1 entries per row, all in columns lo .. hi - 1"""
    u = det_uniform((rows, hi - lo), tag)
    pos = u.abs().topk(4, dim=1).indices
    return torch.zeros(rows, HD).scatter_(1, pos + lo, torch.sign(u.gather(1, pos)))


def _off_where(cond):
    return torch.where(cond, torch.tensor(OFF), torch.tensor(0.0))


class ExactCase:
    """Operands of one exact case as the kernels take them (float32 tensors holding bf16-exact values; rows [n * 49, C]) and the 0 / 1
    matrix P [n, heads, 49, 49] they encode."""

    def __init__(self, family, n_rep, nW, heads, chunks, tables):
        assert family in FAMILIES and n_rep % chunks == 0
        tag = f"bwd:{family}:{n_rep}:{nW}:{heads}:{chunks}:{tables}"
        self.family, self.heads, self.C = family, heads, heads * HD
        self.n = n = n_rep * nW
        self.nb = nb = n if tables == "each" else nW
        self.reps, self.chunks = n // nb, chunks
        assert self.reps % chunks == 0
        self.n_tiles = {"window": nb, "each": nb, "shared": 1}[tables]
        rows = n * TOK * heads
        as_rows = lambda t: t.reshape(n * TOK, heads * HD)
        self.q, self.k = as_rows(_signed4(rows, 0, 16, tag + ":q")), as_rows(_signed4(rows, 16, 32, tag + ":k"))
        self.v, self.dout = as_rows(_signed4(rows, 0, 32, tag + ":v")), as_rows(_signed4(rows, 0, 32, tag + ":g"))
        self.lse = torch.cat([torch.zeros(n, heads, TOK), torch.full((n, heads, PAD - TOK), math.inf)], -1)
        # how often a factor switches a pair off: so that more than half of P is 1 in every family
        cut = {"mask": 0.3, "beta": 0.3, "dist": 0.0, "all": 0.7}[family]
        self.alpha, self.beta = torch.zeros(NBINS, heads), torch.zeros(NBINS, heads)
        self.mask = self.dist = None
        if family in ("mask", "all"):
            self.mask = _off_where(det_uniform((self.n_tiles, TOK, TOK), tag + ":m") > cut)
            for t in range(self.n_tiles):
                self.mask[t, (5 + t) % TOK] = OFF                  # an all-zero row of P
                if family == "mask":
                    self.mask[t, (17 + 3 * t) % TOK] = 0.0          # an all-one row of P
        if family in ("beta", "all"):
            self.beta = _off_where(det_uniform((NBINS, heads), tag + ":b") > cut)
        if family in ("dist", "all"):
            self.dist = (det_uniform((self.n_tiles, TOK, TOK), tag + ":d") > 0.0).float()
            self.alpha = _off_where(det_uniform((NBINS, heads), tag + ":a") > (cut if family == "all" else 0.0))
        self.P = (self.bias() == 0).double()

    def bias(self, mask=None, dist=None):
        """[n, heads, 49, 49] float64: (dist * alpha[idx] + beta[idx]) + mask of each window's bias window (tile wb % n_tiles)"""
        mask, dist = (self.mask if mask is None else mask), (self.dist if dist is None else dist)
        idx = rel_index().reshape(-1)
        tile = (torch.arange(self.n) % self.nb) % self.n_tiles
        b = self.beta.double()[idx].reshape(TOK, TOK, self.heads).permute(2, 0, 1)[None].expand(self.n, -1, -1, -1)
        if dist is not None:
            a = self.alpha.double()[idx].reshape(TOK, TOK, self.heads).permute(2, 0, 1)
            b = dist.double()[tile][:, None] * a[None] + b
        if mask is not None:
            b = b + mask.double()[tile][:, None]
        return b

    def expected(self, dtype, bias=None, operands=None, dist=None):
        """what the kernel of `dtype` must return: dq, dk, dv [n * 49, C], gsum [chunks * nb, heads, 64, 64], dalpha (None: planar), dbeta,
        all float64 holding values of `dtype`, and dS.  bias / operands / dist: replacements, for the CPU tests."""
        bias = self.bias() if bias is None else bias
        q, k, v, dout = [heads_first(t, self.heads) for t in (operands or (self.q, self.k, self.v, self.dout))]
        rnd = ec.bf16_round if dtype == torch.bfloat16 else f32_round
        dq, dk, dv, ds = backward64(q, k, v, dout, bias / SCALE32, self.lse[..., :TOK], SCALE32, rnd)
        dist = self.dist if dist is None else dist
        dalpha, dbeta = table_grads(ds, dist, self.n_tiles)
        return dict(dq=rows_of(dq), dk=rows_of(dk), dv=rows_of(dv), gsum=gsum_expected(ds, self.reps, self.nb, self.chunks),
                    dalpha=dalpha, dbeta=dbeta, ds=ds)


def exact_case(family, n_rep, nW, heads, chunks, tables):
    return ExactCase(family, n_rep, nW, heads, chunks, tables)


def first_mismatch(got, want, heads):
    """None, or a message naming the first wrong (window, head, row, column) of a [n * 49, heads * 32] result"""
    got, want = got.double().cpu(), want.double().cpu()
    bad = (got != want) & ~(got.isnan() & want.isnan())
    if not bool(bad.any()):
        return None
    r, col = [int(x) for x in bad.nonzero()[0]]
    return (f"{int(bad.sum())} of {bad.numel()} wrong, first at window {r // TOK}, head {col // HD}, row {r % TOK}, column {col % HD}: "
            f"got {got[r, col].item()!r}, expected {want[r, col].item()!r}")


def first_tile_mismatch(got, want):
    """the same for gsum tiles [items, heads, 64, 64] (stored [key j][query i]) and the [169, heads] tables"""
    got, want = got.double().cpu(), want.double().cpu()
    bad = (got != want) | got.isnan()
    if not bool(bad.any()):
        return None
    at = tuple(int(x) for x in bad.nonzero()[0])
    return f"{int(bad.sum())} of {bad.numel()} wrong, first at {at}: got {got[at].item()!r}, expected {want[at].item()!r}"


# ---- the dense class --------------------------------------------------------------------------------------------------------------------------
class DenseCase:
    """Random bf16-exact q, k, v, dO (ec._attn_case) with the tables, distances and masks of the forward tests; lse = float32 of the
    float64 log-sum-exp of the scores, which T, the rounding model, the float32 definition and the kernel all receive."""

    def __init__(self, n_rep, nW, heads, pano, mask_kind, chunks):
        x, self.alpha, self.beta, self.dist, mask, gout = ec._attn_case(n_rep, nW, heads, pano, mask_kind, f"{n_rep}{nW}{heads}")
        self.heads, self.C, self.n, self.chunks = heads, heads * HD, n_rep * nW, chunks
        C = self.C
        self.nb = self.n if mask_kind == 4 else nW
        self.reps = self.n // self.nb
        assert self.reps % chunks == 0
        self.x =x.to(torch.bfloat16).float()
        self.q, self.k, self.v = [self.x[:, i * C:(i + 1) * C].contiguous() for i in range(3)]
        self.dout = gout.to(torch.bfloat16).float()
        self.mask = None if mask is None else mask.reshape(-1, TOK, TOK)
        bias = ec.core_bias(self.alpha, self.beta, self.dist, heads, n_rep)               # [1 | n, heads, 49, 49]
        if self.mask is not None:
            bias = bias + self.mask.double().repeat(self.n // self.mask.shape[0], 1, 1)[:, None]
        self.bias = bias.expand(self.n, -1, -1, -1)
        qh, kh = heads_first(self.q, heads).double(), heads_first(self.k, heads).double()
        self.scores = (qh @ kh.transpose(-2, -1)) * SCALE32 + self.bias
        self.lse64 = torch.logsumexp(self.scores, -1)
        self.lse = torch.cat([self.lse64.float(), torch.full((self.n, heads, PAD - TOK), math.inf)], -1)

    def evaluate(self, rnd=None, dtype=torch.float64, mutant=None):
        """-> dq, dk, dv [n * 49, C], gsum, dalpha (None: planar), dbeta in `dtype`"""
        ops = [heads_first(t, self.heads) for t in (self.q, self.k, self.v, self.dout)]
        dq, dk, dv, ds = backward64(*ops, self.bias / SCALE32, self.lse[..., :TOK], SCALE32, rnd, dtype, mutant)
        dalpha, dbeta = table_grads(ds, self.dist, 1 if self.dist is None else self.dist.shape[0])
        return dict(dq=rows_of(dq), dk=rows_of(dk), dv=rows_of(dv), gsum=gsum_expected(ds, self.reps, self.nb, self.chunks),
                    dalpha=dalpha, dbeta=dbeta)

    def lse32(self):
        """the float32 definition of the forward's log-sum-exp rows: float32 scores, float32 logsumexp"""
        qh, kh = heads_first(self.q, self.heads), heads_first(self.k, self.heads)
        return torch.logsumexp((qh @ kh.transpose(-2, -1)) * SCALE32 + self.bias.float(), -1)


_DENSE = {}


def dense_case(*key):
    """built once per process and shared, with its three evaluations: T (float64), E (float64 with the bf16 rounding points) and the
    float32 definition.  Read only."""
    if key not in _DENSE:
        c = DenseCase(*key)
        c.T, c.E, c.D32 = c.evaluate(), c.evaluate(ec.bf16_round), c.evaluate(dtype=torch.float32)
        _DENSE[key] = c
    return _DENSE[key]


def within32(got, f32, truth):
    """the rule of tests/test_cascade_gpu.py::_within: max|K - T| <= 4 max|def32 - T| + ulp32(max|T|), K = the kernel's result, def32 =
    the float32 evaluation of the same formulas, T = the float64 one (all given the same f32 lse).  -> (max|K - T|, max|def32 - T|, bound)"""
    got, f32, truth = got.detach().double().cpu(), f32.detach().double().cpu(), truth.detach().double().cpu()
    e32 = float((f32 - truth).abs().max())
    return float((got - truth).abs().max()), e32, 4 * e32 + ulp32(truth.abs().max())
