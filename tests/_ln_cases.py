"""Shared by tests/test_ln_cases.py (CPU) and tests/test_ln_edges_gpu.py: the launch arithmetic of csrc/pswin_norm.hip, the float64 statement
of LayerNorm with its backward and its row movers, the inputs, the error bounds the kernels are held to, the assertions that have one
right answer, and a float32 mirror of the kernels' formulas that can carry one planted defect.

Every bound counts correctly rounded f32 operations along the kernel's own order (U = 2^-24 is the most one of them loses, relative to its
result; n of them in a chain lose at most g(n) = n U / (1 - n U) of the sum of the magnitudes added), with the count in a comment beside
it.  None was taken from a kernel's output.  The library is built with -ffp-contract=off, so no product is fused with an addition.

ASSUMPTION (rsqrtf): the HIP math documentation (docs/reference/math_api of the HIP repository: "rsqrtf, 1 ULP") is not shipped with the
ROCm installation this was written against -- no file under its share/doc/hip or include/hip states an accuracy --, so the figure is
taken from memory of that table: rsqrtf is within 1 ulp of 1 / sqrt(x), that is within 2^-23 of it relatively (RSQRT_REL).

All functions take tensors of any device, so the cases beyond one sweep are evaluated where their data lives.  LayerNorm itself is stated
on [R, C] rows; each operator is a way to lay rows out (Case.ln_input, Case.row_ops, Case.layout)."""
import math
import types

import torch
import torch.nn.functional as F

from _losses_cases import half_ulp_bf16

F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24                   # unit roundoff of f32
ULP = 2.0 ** -23
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))        # the eps the kernels see (a float argument)
RSQRT_REL = ULP                  # see ASSUMPTION above


def g(n):
    """n chained roundings, relative to the sum of the magnitudes"""
    return n * U / (1.0 - n * U)


# ---- the kernels' launch arithmetic (line numbers of panoswintransformerobjectdetection_amd/csrc/pswin_norm.hip) ---------------------------
THREADS = 256                    # :23
BWD_MAX_BLOCKS = 1024            # :1040


def pick_lanes(C):
    """pick_lanes() :1029-1033: the lanes of a row, the smallest power of two in 2..64 with 16 L >= C"""
    L = 2
    while L * 16 < C and L < 64:
        L *= 2
    return L


def rpb(C):
    """rows per block, RPB = THREADS / L (:176, :235, :460)"""
    return THREADS // pick_lanes(C)


def wide_row(C):
    """wide_row() :1034: rows wider than 1024 elements take 8 chunk slots per lane (launch_fwd :1097, launch_bwd :1133)"""
    return C > 1024


def chunk_slots(C, backward=False):
    """the NCH a kernel is instantiated with: 8 for a wide row; forward 4 (:1104), 3 in the exact-row kernels (:235); backward 3 where
    C / 4 <= 3 L, else 4 (:1151)"""
    if wide_row(C):
        return 8
    if exact_rows(C) or (backward and C // 4 <= 3 * pick_lanes(C)):
        return 3
    return 4


def lane_chunks(C):
    """the chunk slots of a lane that lie in the row (in_row() :44-47): 3 or 4, up to 8 for a wide row; the others add nothing"""
    n = -(-(C // 4) // pick_lanes(C))
    assert n <= chunk_slots(C, True)
    return n


def exact_rows(C):
    """exact_rows() :1066: C == 12 L with L = 8..64 (96, 192, 384, 768) under pswin_ln_rows_tune(0)"""
    L = pick_lanes(C)
    return L >= 8 and C == 12 * L


def bwd_exact_rows(C, S):
    """launch_bwd :1117: the exact-row backward kernel also needs S >= RPB (a block's rows in at most two images)"""
    return exact_rows(C) and S >= rpb(C)


def bwd_blocks(rows, C):
    """bwd_blocks() :1042-1046: the persistent grid of the backward kernels, one partial row per block"""
    return min(-(-rows // rpb(C)), BWD_MAX_BLOCKS)


def row_chain(C):
    """the longest chain of f32 additions behind a row sum (row_stats :51-66, bwd_chunk :85-86, row_sum :29-37): per chunk of a lane the
    two levels of (a + b) + (c + d) and the addition to the lane's accumulator, then log2 L steps across the lanes"""
    return 3 * lane_chunks(C) + int(math.log2(pick_lanes(C)))


def colsum_seg_chain(R):
    """colsum_seg_kernel :994-1021 over R partial rows: a row lane's two accumulators take every 128th row each (ceil(R / 128) additions),
    their sum (1), the 4-way merge of the 64 row lanes (2) and the serial loop over the last 16 (16)"""
    return -(-R // 128) + 1 + 2 + 16


def sum_rows_chain(R):
    """reduce_jobs_kernel (pswin_move.hip), which the autograd wrappers sum the partial rows with: up to 16 rows in one lane, up to 128
    in 8 lanes and a chain of 8, more in 64 lanes and two chains of 8"""
    return R if R <= 16 else -(-R // 8) + 8 if R <= 128 else -(-R // 64) + 16


def col_chain(rows, C):
    """the longest chain behind a dgamma / dbeta / dres_sum column: a row group's trips over its rows (:471), the RPB row groups of a
    block added one after the other (bwd_partials :569-572), then the partial rows of the blocks by either reduction"""
    nb = bwd_blocks(rows, C)
    trips = -(-rows // (nb * rpb(C)))
    return trips + rpb(C) + max(colsum_seg_chain(nb), sum_rows_chain(nb))


# ---- the float64 definition: the row movers ------------------------------------------------------------------------------------------------
def invert(wmap, S):
    """slot -> token map (-1: a zero row) -> token -> slot"""
    inv = torch.full((S,), -1, dtype=torch.long, device=wmap.device)
    real = wmap >= 0
    inv[wmap[real]] = torch.nonzero(real).flatten()
    assert bool((inv >= 0).all())
    return inv


def to_slots(t, wmap, pad=None):
    """t [B, S, ...] rows per token -> [B, n_out, ...] rows per slot; a slot without a token is a zero row (pad: a defect's value)"""
    if wmap is None:
        return t
    out = t[:, wmap.clamp(min=0)].clone()
    out[:, wmap < 0] = 0 if pad is None else pad.to(out.dtype)
    return out


def merge(x, H, W):
    """PatchMerging's 2 x 2 gather: [B, H W, C] -> [B, ceil(H / 2) ceil(W / 2), 4 C], quarters (0,0) (1,0) (0,1) (1,1), zeros outside"""
    B, _, C = x.shape
    img = F.pad(x.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
    cat = torch.cat([img[:, 0::2, 0::2], img[:, 1::2, 0::2], img[:, 0::2, 1::2], img[:, 1::2, 1::2]], -1)
    return cat.reshape(B, -1, 4 * C)


def unmerge(d, H, W):
    """the adjoint of merge(): every token lies in one quarter of one merged row; what falls outside the image is dropped"""
    B, _, C4 = d.shape
    C, H2, W2 = C4 // 4, (H + 1) // 2, (W + 1) // 2
    d = d.view(B, H2, W2, 4, C)
    img = d.new_zeros(B, 2 * H2, 2 * W2, C)
    img[:, 0::2, 0::2], img[:, 1::2, 0::2], img[:, 0::2, 1::2], img[:, 1::2, 1::2] = d[..., 0, :], d[..., 1, :], d[..., 2, :], d[..., 3, :]
    return img[:, :H, :W].reshape(B, H * W, C)


def nchw(t, H, W):
    B, S, C = t.shape
    return t.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def from_nchw(t):
    B, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B, H * W, C)


def branch64(resid, win, scale, bias):
    """x1 = resid + scale_b * (win + bias) in float64; an absent scale or bias is left out"""
    v = win.double()
    if bias is not None:
        v = v + bias.double()
    if scale is not None:
        v = v * scale.double()[:, None, None]
    return resid.double() + v


def branch32(resid, win, scale, bias):
    """the same in float32 in branch_add's order (:72-76): three correctly rounded operations with one right answer"""
    v = win.float()
    if bias is not None:
        v = v + bias
    if scale is not None:
        v = v * scale[:, None, None]
    return v + resid


# ---- the float64 definition: LayerNorm on rows ---------------------------------------------------------------------------------------------
def ln_forward(x, gamma, beta, add=None, eps=EPS32):
    """y = (x - mean) * rstd * gamma + beta (+ add) with the biased variance; x [R, C], add [R, C] or None"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    r = types.SimpleNamespace(C=x.shape[-1], x=x)
    r.mean = x.mean(-1)
    r.mean_abs = x.abs().mean(-1)
    dev = x - r.mean[:, None]
    r.var = (dev * dev).mean(-1)
    r.rstd = 1.0 / torch.sqrt(r.var + eps)
    r.xhat = dev * r.rstd[:, None]
    r.y0 = r.xhat * gamma + beta
    r.y = r.y0 if add is None else r.y0 + add.double()
    r.has_add = add is not None
    return r


def ln_backward(r, dy, gamma, dres=None, row_scale=None):
    """dx = (g - mean(g) - xhat mean(g xhat)) rstd (+ dres), g = dy gamma; dgamma = sum dy xhat; dbeta = sum dy;
    dres_sum = sum row_scale dres (row_scale [R]: res_scale of the row's image)"""
    dy, gamma = dy.double(), gamma.double()
    k = types.SimpleNamespace(dy=dy)
    k.g = dy * gamma
    k.mg, k.mgx = k.g.mean(-1), (k.g * r.xhat).mean(-1)
    k.dx0 = (k.g - k.mg[:, None] - r.xhat * k.mgx[:, None]) * r.rstd[:, None]
    k.dx = k.dx0 if dres is None else k.dx0 + dres.double()
    k.has_dres = dres is not None
    k.dgamma, k.dbeta = (dy * r.xhat).sum(0), dy.sum(0)
    k.dres_sum = None
    if dres is not None and row_scale is not None:
        k.sres = dres.double() * row_scale.double()[:, None]
        k.dres_sum = k.sres.sum(0)
    return k


# ---- the bounds ----------------------------------------------------------------------------------------------------------------------------
def forward_bounds(r, gamma, beta):
    """Allowed |kernel - float64| of mean, rstd [R] and y [R, C] (f32 stores), with what the backward bounds need.

    mean     row_sum(s) / C: n = row_chain(C) additions, g(n) of sum |x| / C, and the division: U |mean|
    var      the second pass sees the computed mean mu = mean + d, |d| <= d_mean, and sum (x - mu)^2 / C = var + d^2 exactly.  Each term:
             x - mu (U), its square (that error twice and the product: 3 U in all), n additions, the division: g(n + 4) (var + d^2),
             plus d^2 itself
    rstd     rsqrtf(var + eps) with the computed var anywhere in var -+ d_var (the interval itself, as tests/_bn_cases.py: on a constant
             row d_var exceeds eps many times over only in relative terms, the interval stays exact), the addition of eps (U of the
             argument, at most U of the result), rsqrtf (RSQRT_REL); the f32 store is the value itself
    xhat     fl(fl(x - mu) rstd): rstd d_mean -- the term that leaves a constant row of 3.7 with 7.5e-5 instead of 0 -- and
             (|xhat| + rstd d_mean) (rel(rstd) + 2 U) for rstd's error, the difference and the product
    y        ln_affine (:68): fl(fl(xhat gamma) + beta): |gamma| d_xhat + U |xhat gamma| + U |y0|; an added row: + U |y|"""
    n = row_chain(r.C)
    t = types.SimpleNamespace()
    t.mean = g(n) * r.mean_abs + U * r.mean.abs()                                    # n additions, 1 division
    d2 = t.mean * t.mean
    d_var = g(n + 4) * (r.var + d2) + d2                                             # 1 difference, 3 for the square, n additions, 1 division
    lo, hi = 1.0 / torch.sqrt(r.var + d_var + EPS32), 1.0 / torch.sqrt((r.var - d_var).clamp_min(0.0) + EPS32)
    t.rel_rstd = torch.maximum(r.rstd - lo, hi - r.rstd) / r.rstd + U + RSQRT_REL    # the interval, + eps, rsqrtf
    t.rstd = r.rstd * t.rel_rstd
    slip = (r.rstd * t.mean)[:, None]
    t.xhat = slip + (r.xhat.abs() + slip) * (t.rel_rstd[:, None] + 2 * U)            # the mean's error; rstd's, 1 difference, 1 product
    ga = gamma.double().abs()
    t.y = ga * t.xhat + U * (r.xhat * gamma.double()).abs() + U * r.y0.abs()         # 1 product, 1 addition
    if r.has_add:
        t.y = t.y + U * r.y.abs()                                                    # 1 more addition
    return t


def backward_bounds(r, k, t, gamma, rows):
    """Allowed |kernel - float64| of dx [R, C] and of the column sums [C]; t: forward_bounds (the backward kernels read the stored mean
    and rstd and form xhat as the forward pass did); rows: the rows the launch walks (for the chain of a column).

    g        dy gamma: U |g|
    s1       row_sum(g) / C: each term's U, n additions, the division: (g(n) + U) mean |g| + U |s1|
    s2       row_sum(g xhat) / C: mean(|g| d_xhat), each product's 2 U (g's and its own), n additions, the division
    dx       bwd_dx (:88): ((g - s1) - xhat s2) rstd: d_g + d_s1 + |xhat| d_s2 + |s2| d_xhat + U |xhat s2| (product), the two
             differences U (|g| + |s1|) and U (|g| + |s1| + |xhat s2|); times rstd; |dx0| (rel(rstd) + U) for rstd and the last
             product; a shortcut gradient: + U |dx|
    dgamma   sum over the rows of dy xhat: sum |dy| d_xhat, each product's U, and e = g(col_chain) of sum |dy xhat|
    dbeta    e sum |dy|;  dres_sum: each product res_scale dres (U) and e of sum |res_scale dres|"""
    n = row_chain(r.C)
    ag = k.g.abs()
    d_s1 = (g(n) + U) * ag.mean(-1) + U * k.mg.abs()                                 # 1 product a term, n additions, 1 division
    d_s2 = (ag * t.xhat).mean(-1) + (g(n) + 2 * U) * (k.g * r.xhat).abs().mean(-1) + U * k.mgx.abs()     # 2 products a term, n, 1
    xm = (r.xhat * k.mgx[:, None]).abs()
    inner = (U * ag + d_s1[:, None] + r.xhat.abs() * d_s2[:, None] + k.mgx.abs()[:, None] * t.xhat + U * xm      # operands; 1 product
             + U * (ag + k.mg.abs()[:, None]) + U * (ag + k.mg.abs()[:, None] + xm))                             # 2 differences
    b = types.SimpleNamespace()
    b.dx = r.rstd[:, None] * inner + k.dx0.abs() * (t.rel_rstd[:, None] + U)         # rstd's own error, 1 product
    if k.has_dres:
        b.dx = b.dx + U * k.dx.abs()                                                 # 1 addition
    e = g(col_chain(rows, r.C))
    b.dgamma = (k.dy.abs() * t.xhat).sum(0) + (e + U) * (k.dy * r.xhat).abs().sum(0)     # 1 product a term, the chain
    b.dbeta = e * k.dy.abs().sum(0)                                                  # the chain
    b.dres_sum = None if k.dres_sum is None else (e + U) * k.sres.abs().sum(0)       # 1 product a term, the chain
    return b


def with_bf16(value, bound):
    """a bf16 store adds half a bf16 ulp of the value (of the largest value the bound admits); an exact zero stays exact"""
    top = value.abs() + bound
    return bound + half_ulp_bf16(top) * (top > 0)


def ratio(got, want, bound):
    """largest |got - want| / bound; an element with a zero bound must be exact; NaN / inf never pass"""
    gd = got.double().to(want.device)
    assert gd.shape == want.shape, (gd.shape, want.shape)
    if gd.numel() == 0:
        return 0.0
    err = (gd - want).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(torch.where(torch.isfinite(gd), q, torch.full_like(q, float("inf"))).max())


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------------
KINDS = ("const13", "const37", "mean30", "mean1000", "tiny", "big", "zeros")
CONST13 = 2.625                  # 5 significant bits: every partial sum of up to 2048 of them is exact in f32 whatever the order
SIGMA = 2.0 / math.sqrt(3.0)     # the standard deviation of the benign rows, uniform in +-2
INT_MAX = 4                      # |dy|, |dres| <= 4, integers
SCALES = (0.0, 0.5, 1.25)        # the dyadic per-sample scales


def significant_bits(v):
    m, _ = math.frexp(abs(v))
    n = 0
    while m != int(m):
        m, n = m * 2, n + 1
    return n


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def uniform(shape, gen, scale=1.0, offset=0.0):
    return (torch.rand(shape, generator=gen) * 2.0 - 1.0) * scale + offset


def integers(shape, gen):
    return torch.randint(-INT_MAX, INT_MAX + 1, shape, generator=gen).float()


def affine_params(C, gen):
    """gamma in +-[0.5, 1.5] (every fifth channel negative) with channel 1 exactly 0 and channel 2 at 16; beta in +-0.5"""
    gamma = uniform((C,), gen, 0.5, 1.0) * torch.where(torch.arange(C) % 5 == 0, -1.0, 1.0)
    gamma[1], gamma[2] = 0.0, 16.0
    return gamma, uniform((C,), gen, 0.5)


def plan_rows(B, S, C, seed, maps=(), extra=()):
    """{LN row: kind}: the first and last two tokens of every image and a middle one, the first and last row of the last row block,
    `extra` (the seams of a sweep), the kinds in turn; and at every slot map a token of zeros in front of a pad slot with an exactly
    summable constant behind one (the other way round in the second image)"""
    R = B * S
    rows = [b * S + t for b in range(B) for t in (0, 1, S // 2, S - 2, S - 1) if 0 <= t < S]
    rows += [(R - 1) // rpb(C) * rpb(C), R - 1] + [int(e) for e in extra if 0 <= e < R]
    special = {}
    for m in maps:
        if m is None:
            continue
        pad = m < 0
        before = torch.nonzero(pad[1:] & ~pad[:-1]).flatten()          # slot s real, s + 1 a pad
        after = torch.nonzero(pad[:-1] & ~pad[1:]).flatten() + 1       # slot s real, s - 1 a pad
        if len(before) and len(after):
            tz, tc = int(m[before[0]]), int(m[after[-1]])
            if tz != tc:
                for b in range(B):
                    special[b * S + tz], special[b * S + tc] = ("zeros", "const13") if b % 2 == 0 else ("const13", "zeros")
    plan = {row: KINDS[(i + seed) % len(KINDS)] for i, row in enumerate(sorted(set(rows) - set(special)))}
    plan.update(special)
    return plan


def plant(x2d, plan, gen):
    """writes the planted rows into x2d [R, C] (benign rows: uniform(+-2) + 0.3, as the older tests)"""
    C = x2d.shape[1]
    for row, kind in plan.items():
        base = uniform((C,), gen, 2.0)
        x2d[row] = {"const13": torch.full((C,), CONST13), "const37": torch.full((C,), 3.7), "mean30": base + 30.0 * SIGMA,
                    "mean1000": base + 1000.0 * SIGMA, "tiny": base * 5e-5, "big": base * 5e3, "zeros": torch.zeros(C)}[kind]
    return x2d


class Case:
    """One operator call.  Inputs are CPU float32 tensors (holding bf16 values where the operand is bf16), never written to afterwards.
    kind "gather":  layer_norm_gather          x [B, S, C] (xdt), wmap (slot -> token) or None, add [S, C], dres / res_scale (passthrough)
         "scatter": scatter_add_layer_norm     win (bf16) [B, n_in, C] by in_map or in token order, resid, scale, bias; y through out_map
         "merge":   layer_norm_patch_merge     x [B, H W, C / 4]
         "nchw":    layer_norm_nchw, or with win: scatter_add_layer_norm_nchw
    C is always the width LayerNorm sees, S the tokens of an image, rows the rows LayerNorm walks."""

    def __init__(self, kind, C, B, S, seed, xdt=F32, wmap=None, in_map=None, out_map=None, add=False, shortcut=False, res=False,
                 bare=False, branch=False, H=0, W=0, extra=(), name=None):
        gen = _gen(C, B, S, seed, len(kind))
        self.kind, self.C, self.B, self.S, self.seed, self.xdt, self.H, self.W = kind, C, B, S, seed, xdt, H, W
        self.wmap, self.in_map, self.out_map, self.bare = wmap, in_map, out_map, bare
        self.name = name or f"{kind}-C{C}-S{S}"
        q = (lambda t: t.to(BF16).float()) if xdt == BF16 else (lambda t: t)
        self.gamma, self.beta = affine_params(C, gen)
        self.rows = B * S
        Cin = C
        if kind == "merge":
            Cin, self.S2 = C // 4, ((H + 1) // 2) * ((W + 1) // 2)
            self.rows = B * self.S2
        ymap = wmap if kind == "gather" else out_map
        if kind == "merge":                              # planted on the merged rows: every token of the 2 x 2 inside the image
            self.plan, tokens, W2 = plan_rows(B, self.S2, C, seed, extra=extra), {}, (W + 1) // 2
            for row, what in self.plan.items():
                b, (i, j) = row // self.S2, divmod(row % self.S2, W2)
                tokens.update({b * S + yy * W + xx: what for yy in (2 * i, 2 * i + 1) for xx in (2 * j, 2 * j + 1) if yy < H and xx < W})
        else:
            self.plan = tokens = plan_rows(B, S, C, seed, (wmap, in_map, out_map), extra)
        x = q(plant(uniform((B * S, Cin), gen, 2.0, 0.3), tokens, gen)).view(B, S, Cin)
        self.x = x                                       # gather / merge / nchw: the input; scatter and a branch: the shortcut (resid)
        self.scale = self.bias = self.win = self.res_scale = self.dres = self.add = None
        if kind == "scatter" or branch:
            n_in = S if in_map is None else in_map.numel()
            self.win = uniform((B, n_in, C), gen, 2.0).to(BF16).float()
            tok = torch.tensor(sorted(self.plan))        # a planted row stays what it is where the branch adds nothing to it
            b_of, t_of = tok // S, tok % S
            self.win[b_of, t_of if in_map is None else invert(in_map, S)[t_of]] = 0.0
            if not bare:
                self.scale, self.bias = torch.tensor([1.25, 0.0, 0.5][:B]), uniform((C,), gen, 0.5)
            shortcut, res = True, kind == "scatter" and not bare
        if add:
            self.add = uniform((S, C), gen, 1.5)
        n_y = S if ymap is None else ymap.numel()
        self.dy = integers((B, C, H, W) if kind == "nchw" else (B, self.S2 if kind == "merge" else n_y, C), gen)
        if shortcut:
            self.dres = integers((B, S, C), gen)
        if res:
            self.res_scale = torch.tensor([0.0, 0.5, 1.25][:B])

    # -- the rows LayerNorm sees ---------------------------------------------------------------------------------------------------------
    def ln_input(self):
        """f32 [rows, C]: x itself, the merged rows, or x1 in float32 (three operations with one right answer)"""
        if self.win is not None:
            win = self.win if self.in_map is None else self.win[:, invert(self.in_map, self.S)]
            return branch32(self.x, win, self.scale, self.bias).reshape(-1, self.C)
        if self.kind == "merge":
            return merge(self.x, self.H, self.W).reshape(-1, self.C)
        return self.x.reshape(-1, self.C)

    def inside(self):
        """merge: which elements of a merged row lie in the image"""
        return merge(torch.ones_like(self.x), self.H, self.W).reshape(-1, self.C) > 0 if self.kind == "merge" else None

    def row_ops(self):
        """(add, dy, dres, row_scale) as [rows, C] / [rows] operands of the row definition"""
        B, S, C = self.B, self.S, self.C
        ymap = self.wmap if self.kind == "gather" else self.out_map
        dy = from_nchw(self.dy) if self.kind == "nchw" else self.dy if ymap is None else self.dy[:, invert(ymap, S)]
        add = None if self.add is None else self.add.expand(B, S, C).reshape(-1, C)
        dres = None if self.dres is None else self.dres.reshape(-1, C)
        rs = None if self.res_scale is None else self.res_scale.repeat_interleave(S)
        return add, dy.reshape(-1, C), dres, rs

    # -- rows -> the operator's outputs ---------------------------------------------------------------------------------------------------
    def layout(self, d, defect=None):
        """d: y, mean, rstd, dx, dgamma, dbeta, dres_sum (and y_bf16, dx_bf16) on rows -> the operator's outputs.  The same function lays
        out the definition, the bounds and the mirror; defect: "pad_beta" or "stats_at_slot"."""
        B, S, C = self.B, self.S, self.C
        ymap = self.wmap if self.kind == "gather" else self.out_map
        out = {k: d[k] for k in ("dgamma", "dbeta", "dres_sum") if d.get(k) is not None}
        for k in ("y", "y_bf16"):
            if d.get(k) is None:
                continue
            if self.kind == "merge":
                out[k] = d[k].view(B, self.S2, C)
            elif self.kind == "nchw":
                out[k] = nchw(d[k].view(B, S, C), self.H, self.W)
            else:
                out[k] = to_slots(d[k].view(B, S, C), ymap, self.beta if defect == "pad_beta" and torch.is_floating_point(d[k]) else None)
        for k in ("mean", "rstd"):
            out[k] = d[k].view(B, -1)
            if defect == "stats_at_slot" and ymap is not None:       # written at the slot a row went to instead of at its token
                wrong = out[k].clone()
                slots = torch.nonzero((ymap >= 0) & (torch.arange(ymap.numel()) < S)).flatten()
                wrong[:, slots] = out[k][:, ymap[slots]]
                out[k] = wrong
        for k in ("dx", "dx_bf16"):
            if d.get(k) is not None:
                out[k] = unmerge(d[k].view(B, self.S2, C), self.H, self.W) if self.kind == "merge" else d[k].view(B, S, C)
        return out

    # -- the definition and the bounds ---------------------------------------------------------------------------------------------------
    def reference(self, device="cpu"):
        """(want, bound): {output: float64 tensor} in the operator's layout.  bf16 outputs have entries of their own (<name>_bf16, dwin,
        dbranch) with half a bf16 ulp on top."""
        to = lambda t: None if t is None else t.to(device)
        x = to(self.ln_input())
        add, dy, dres, rs = (to(t) for t in self.row_ops())
        gamma, beta = to(self.gamma), to(self.beta)
        r = ln_forward(x, gamma, beta, add)
        t = forward_bounds(r, gamma, beta)
        k = ln_backward(r, dy, gamma, dres, rs)
        b = backward_bounds(r, k, t, gamma, self.rows)
        want = dict(y=r.y, mean=r.mean, rstd=r.rstd, dx=k.dx, dgamma=k.dgamma, dbeta=k.dbeta, dres_sum=k.dres_sum)
        bound = dict(y=t.y, mean=t.mean, rstd=t.rstd, dx=b.dx, dgamma=b.dgamma, dbeta=b.dbeta, dres_sum=b.dres_sum)
        want.update(y_bf16=r.y, dx_bf16=k.dx)
        bound.update(y_bf16=with_bf16(r.y, t.y), dx_bf16=with_bf16(k.dx, b.dx))
        self._to_device(device)
        want, bound = self.layout(want), self.layout(bound)
        if self.win is not None:
            B, S, C = self.B, self.S, self.C
            win = to(self.win) if self.in_map is None else to(self.win)[:, invert(to(self.in_map), S)]
            want["x1"] = branch64(to(self.x), win, to(self.scale), to(self.bias))
            # x1: the sum win + bias (U), its product with the scale (U), the sum with the shortcut (U)
            inner = win.double() if self.bias is None else win.double() + to(self.bias).double()
            sc = torch.ones(B, dtype=torch.float64, device=device) if self.scale is None else to(self.scale).double()
            bound["x1"] = 2 * U * (inner * sc[:, None, None]).abs() + U * want["x1"].abs()
            # the branch gradient bf16(scale_b dx): dx's bound, the product (U), the bf16 store
            dw, bw = want["dx"] * sc[:, None, None], bound["dx"] * sc.abs()[:, None, None]
            bw = with_bf16(dw, bw + U * dw.abs())
            key = "dwin" if self.kind == "scatter" else "dbranch"
            want[key], bound[key] = to_slots(dw, to(self.in_map)), to_slots(bw, to(self.in_map))
        if self.add is not None:                             # the added rows' gradient: the sum of dy over the images, B - 1 additions
            want["dadd"] = to(self.dy).double().sum(0)
            bound["dadd"] = g(self.B - 1) * to(self.dy).double().abs().sum(0)
        self._to_device("cpu")
        return want, bound

    def _to_device(self, device):
        for k in ("wmap", "in_map", "out_map"):
            if getattr(self, k) is not None:
                setattr(self, k, getattr(self, k).to(device))

    # -- the assertions with one right answer ---------------------------------------------------------------------------------------------
    def exact_failures(self, got):
        """got: the operator's outputs as CPU tensors -> the list of exact assertions that do not hold"""
        bad = []
        B, S, C = self.B, self.S, self.C
        x = self.ln_input()
        add, dy, dres, rs = self.row_ops()
        eq = lambda a, b: a.shape == b.shape and torch.equal(a, b)
        # 1. y from the statistics the kernel stored, in ln_affine's order
        mu, rstd = got["mean"].reshape(-1, 1), got["rstd"].reshape(-1, 1)
        y = ((x - mu) * rstd) * self.gamma + self.beta
        if add is not None:
            y = y + add
        if not eq(got["y"], self.layout(dict(y=y, mean=mu, rstd=rstd))["y"]):
            bad.append("y is not ((x - mean) * rstd) * gamma + beta (+ add) of the stored statistics")
        # 2. every bf16 output is the round-to-nearest-even cast of its f32 counterpart
        if "y_bf16" in got and not eq(got["y_bf16"], got["y"].to(BF16)):
            bad.append("the bf16 y is not the nearest-even cast of the f32 y")
        if "dx_bf16" in got and not eq(got["dx_bf16"], got["dx"].to(BF16)):
            bad.append("the bf16 dx is not the nearest-even cast of the f32 dx")
        for key in ("dwin", "dbranch"):
            if key in got:
                sc = got["dx"] if self.scale is None else got["dx"] * self.scale[:, None, None]
                if not eq(got[key], to_slots(sc.to(BF16), self.in_map)):
                    bad.append(f"{key} is not the nearest-even cast of scale_b * dx (zero rows at the pad slots)")
        # 3. sums of integers: one answer whatever the order
        sums = dict(dbeta=dy.double().sum(0))
        if dres is not None and rs is not None:
            sums["dres_sum"] = (dres.double() * rs.double()[:, None]).sum(0)
        if self.add is not None:
            sums["dadd"] = self.dy.double().sum(0)
        for key, want in sums.items():
            if not eq(got[key].double(), want):
                bad.append(f"{key} is not the exact sum")
        # 4. x1 in float32, a constant row that sums exactly and a token of zeros give beta (+ add), the gamma = 0 channel gives beta
        if self.win is not None and not eq(got["x1"], x.view(B, S, C)):
            bad.append("x1 is not fl(fl(fl(win + bias) * scale) + resid)")
        flat = x[:, :1]
        const = ((x == flat).all(1) & (flat[:, 0].abs() * 2 ** 8 == (flat[:, 0].abs() * 2 ** 8).round()) & (flat[:, 0].abs() < 16)).view(-1, 1)
        sure = const.expand(-1, C).clone()
        sure[:, 1] = True
        plain = self.beta.expand(x.shape[0], C) if add is None else self.beta + add
        lay = lambda t: self.layout(dict(y=t, mean=mu, rstd=rstd))["y"]
        if not torch.equal(got["y"][lay(sure)], lay(plain.contiguous())[lay(sure)]):
            bad.append("y of an exactly summable constant row, of a token of zeros or of the gamma = 0 channel is not beta (+ add)")
        ymap = self.wmap if self.kind == "gather" else self.out_map
        if ymap is not None and bool((got["y"][:, ymap < 0] != 0).any()):
            bad.append("y of a pad slot is not 0")
        return bad

    def judge(self, got, ref=None, device="cpu"):
        """({output: largest error / bound}, [exact assertions that fail]); every key of `got` must have a bound"""
        want, bound = ref or self.reference(device)
        q = {k: ratio(v, want[k], bound[k]) for k, v in got.items()}
        return q, self.exact_failures({k: v.cpu() for k, v in got.items()})

    def conditions(self):
        """what the exact assertions rest on -> list of violations"""
        bad = []
        if significant_bits(CONST13) > 13 or CONST13 * MAX_WIDTH >= 2 ** 24 * 2 ** -3:      # the sums are multiples of 2^-3
            bad.append("the constant is not exactly summable")
        for t in (self.dy, self.dres):
            if t is not None and not (bool((t == t.round()).all()) and float(t.abs().max()) <= INT_MAX):
                bad.append("a gradient is not a small integer")
        if self.rows * INT_MAX * max(SCALES) >= 2 ** 24 / 4:           # quarters: the scales are multiples of 0.25
            bad.append("a partial sum can reach 2^24")
        for s in (self.scale, self.res_scale):
            if s is not None and not all(float(v) in SCALES for v in s):
                bad.append("a scale is not dyadic")
        kinds = set(self.plan.values())
        if self.win is None and self.rows >= 14 and kinds != set(KINDS):
            bad.append(f"kinds missing: {set(KINDS) - kinds}")
        if self.xdt == BF16 and not torch.equal(self.x, self.x.to(BF16).float()):
            bad.append("x is not bf16")
        return bad


MAX_WIDTH = 2048                 # MAX_C :1035


# ---- a float32 mirror of the kernels' formulas ---------------------------------------------------------------------------------------------
DEFECTS = ("unbiased_variance", "no_eps", "one_pass_variance", "bf16_truncation", "no_mean_g", "no_mean_g_xhat", "pad_beta",
           "zero_token_zero", "outside_quarters_skipped", "stats_at_slot", "drop_block_last_row", "res_scale_ignored")


def _row_sum32(t, C):
    """row_sum of per-chunk (a + b) + (c + d) in the kernel's order: a lane's chunks one after the other, then the tree over the lanes"""
    L, n = pick_lanes(C), lane_chunks(C)
    R = t.shape[0]
    ch = t.view(R, C // 4, 4)
    c = (ch[..., 0] + ch[..., 1]) + (ch[..., 2] + ch[..., 3])
    c = F.pad(c, (0, n * L - C // 4)).view(R, n, L)
    s = torch.zeros(R, L)
    for i in range(n):
        s = s + c[:, i]
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2]
    return s[:, 0]


def _bf16_store(t, defect):
    if defect == "bf16_truncation":
        return (t.contiguous().view(torch.int32) & -65536).view(F32).to(BF16)
    return t.to(BF16)


def mirror(c, defect=None):
    """row_stats, ln_affine, bwd_chunk and bwd_dx (:51-88) in torch float32 on the CPU, the column sums over RPB strided row groups that
    are added one after the other -> the operator's outputs, the bf16 ones beside their f32 counterparts.  defect: one of DEFECTS."""
    C = c.C
    x = c.ln_input()
    add, dy, dres, rs = c.row_ops()
    gamma, beta = c.gamma, c.beta
    fC = float(C)
    if defect == "outside_quarters_skipped":
        inside = c.inside()
        cnt = inside.sum(1).float()
        mu = _row_sum32(x, C) / cnt
        d = (x - mu[:, None]) * inside
        var = _row_sum32(d * d, C) / cnt
    else:
        mu = _row_sum32(x, C) / fC
        d = x - mu[:, None]
        if defect == "one_pass_variance":
            var = (_row_sum32(x * x, C) / fC - mu * mu).clamp_min(0.0)
        else:
            var = _row_sum32(d * d, C) / (fC - 1.0 if defect == "unbiased_variance" else fC)
    rstd = torch.rsqrt(var + (0.0 if defect == "no_eps" else torch.tensor(EPS32)))
    xh = d * rstd[:, None] if defect == "outside_quarters_skipped" else (x - mu[:, None]) * rstd[:, None]
    y = xh * gamma + beta
    if defect == "zero_token_zero":
        y = y * (x != 0).any(1, keepdim=True)
    if add is not None:
        y = y + add
    gg = dy * gamma
    s1 = torch.zeros_like(mu) if defect == "no_mean_g" else _row_sum32(gg, C) / fC
    s2 = torch.zeros_like(mu) if defect == "no_mean_g_xhat" else _row_sum32(gg * xh, C) / fC
    dx = (gg - s1[:, None] - xh * s2[:, None]) * rstd[:, None]
    if dres is not None:
        dx = dx + dres
    lanes = rpb(C)

    def colsum(t):
        keep = t
        if defect == "drop_block_last_row":
            last = min(lanes, t.shape[0]) - 1                       # the last row group of the first block
            keep = torch.cat([t[:last], torch.zeros_like(t[last:last + 1]), t[last + 1:]])
        acc = torch.zeros(C)
        for q in range(min(lanes, keep.shape[0])):
            acc = acc + keep[q::lanes].sum(0)
        return acc

    rows = dict(y=y, y_bf16=_bf16_store(y, defect), mean=mu, rstd=rstd, dx=dx, dgamma=colsum(dy * xh), dbeta=colsum(dy))
    if c.xdt == BF16:
        rows["dx_bf16"] = _bf16_store(dx, defect)
    if dres is not None and rs is not None:
        rows["dres_sum"] = colsum(dres if defect == "res_scale_ignored" else dres * rs[:, None])
    out = c.layout(rows, defect)
    if c.win is not None:
        out["x1"] = x.view(c.B, c.S, C)
        sc = out["dx"] if c.scale is None else out["dx"] * c.scale[:, None, None]
        out["dwin" if c.kind == "scatter" else "dbranch"] = to_slots(_bf16_store(sc, defect), c.in_map)
    if c.add is not None:
        out["dadd"] = c.dy.sum(0)
    if c.kind == "nchw":
        out.pop("y_bf16")
    return out


# ---- the cases both test files run ---------------------------------------------------------------------------------------------------------
EXACT_WIDTHS = (96, 192, 384, 768)
GENERIC_WIDTHS = (32, 64, 104, 1024)
WIDTHS = EXACT_WIDTHS + GENERIC_WIDTHS
MERGE_WIDTHS = (64, 192, 384, 768, 1536)
MERGE_HW = (7, 9)
NCHW_HW = (8, 16)
WINDOW_HW = (9, 11)


def token_counts(C):
    """tokens per image around the rows per block: S >= RPB switches the exact-row backward kernel on"""
    r = rpb(C)
    return tuple(s for s in (r - 1, r, r + 1, 2 * r + 3) if s >= 2)


def synthetic_map(S, n_out, seed):
    """a slot -> token map as the window maps are: every token once, n_out - S pad slots in between (for the CPU tests)"""
    gen = _gen(S, n_out, seed)
    wmap = torch.full((n_out,), -1, dtype=torch.long)
    wmap[torch.randperm(n_out, generator=gen)[:S].sort().values] = torch.randperm(S, generator=gen)
    return wmap


def gather_variants(C, S, seed, wmap=None):
    """the calls of layer_norm_gather one shape is run with: name -> Case"""
    if wmap is not None:
        return {"map_shortcut": Case("gather", C, 2, S, seed, wmap=wmap, shortcut=True, res=True),
                "map_bf16x": Case("gather", C, 2, S, seed + 1, xdt=BF16, wmap=wmap)}
    return {"shortcut": Case("gather", C, 2, S, seed, shortcut=True, res=True),
            "add": Case("gather", C, 2, S, seed + 1, add=True),
            "bf16x": Case("gather", C, 2, S, seed + 2, xdt=BF16)}


def scatter_variants(C, S, seed, wmap, out_map):
    """windows in (scale with a zero sample, bias), bare (neither), join (token order in, y through the out map)"""
    return {"windows": Case("scatter", C, 2, S, seed, in_map=wmap),
            "bare": Case("scatter", C, 2, S, seed + 1, in_map=wmap, bare=True),
            "join": Case("scatter", C, 2, S, seed + 2, out_map=out_map)}


def merge_case(C4, seed):
    H, W = MERGE_HW
    return Case("merge", C4, 2, H * W, seed, H=H, W=W)


def nchw_variants(C, seed):
    H, W = NCHW_HW
    return {"plain": Case("nchw", C, 2, H * W, seed, H=H, W=W),
            "shortcut": Case("nchw", C, 2, H * W, seed + 1, H=H, W=W, shortcut=True),
            "closing_add": Case("nchw", C, 2, H * W, seed + 2, H=H, W=W, branch=True)}


def nchw_supported(S, C):
    """pswin_ln_nchw_supported :1340-1345"""
    return 8 <= C <= 1024 and C % 8 == 0 and rpb(C) >= 4 and S % rpb(C) == 0


def sweep_seams(rows, C):
    """the last row of every sweep of the capped backward grid and the first of the next"""
    sweep = BWD_MAX_BLOCKS * rpb(C)
    return [k * sweep + d for k in range(1, -(-rows // sweep)) for d in (-1, 0)]
