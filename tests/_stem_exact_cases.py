"""Operands on which the tile kernels of the fused PatchEmbed stem (csrc/pswin_stem.hip, csrc/pswin_stem_tiles.inc) have ONE right
answer, and that answer from a plain float64 restatement of the stem (CPU only; tests/test_stem_exact.py checks the conditions and
the planted defects below, tests/test_stem_exact_gpu.py runs the kernels).

All operands are bf16 and every MFMA accumulates in f32.  If all terms of a sum are multiples of one 2^-k and the sum of their
magnitudes stays below 2^(24-k), every partial sum in any order is exact: the f32 result is one number and a bf16 store is its
round-to-nearest-even (the argument of tests/_gemm_exact_cases.py, whose helpers are used here).  BatchNorm scales are +-1 or
another power of two and shifts small dyadic numbers, so that z = fma(y, scale, shift) is exact too and z == 0 is a legitimate input
(activation 0, mask off).  Classes:

  dense   x in {-2..2}, w1 in {-1, 0, 1}, scale1 = +-1 (every fifth channel negative), shift1 an integer in [-3, 3], w2 and w3 in
          {-1, 0, 1} (densities W2_DENSE, 0.25), scale2 = +-1, shift2 an integer chosen per channel at the most frequent value of
          scale2 y2 that leaves 10 % of the channel on either side (a half-integer on every eighth channel where |z2| < 127), bias3 an
          f32 integer, d tokens in {-2..2}, backward coefficients from {+-1, +-0.5, +-2} and small integers.  Every stored bf16 value
          except the tokens has at most 8 significant bits, so no store rounds; the tokens (a 1024-term contraction of a2 up to ~100)
          exceed 8 bits under these ranges and are compared with the RNE of their exact f32 value like everywhere else.
  ties    dense, with w2 of every other input channel, the d tokens of every other output channel and the conv2-backward dy2 of
          every other channel scaled by 2^TIE_S, scale2 = +-2^-TIE_S and a thin w3: a good share of y2, of the tokens and of dy2 are
          exact bf16 ties, which tells RNE from truncation and from half-away rounding.  The sums leave the exactness bound; only the
          element-wise outputs (y2, tokens, dy2 and G, which takes rne_bf16(g1)) are compared, and the plain sum of y2 up to 4096
          pixels, where it is still exact.
  thin    for the shapes beyond one sweep of the grids: x in {-1, 0, 1}, w1 at density 0.5, W2_THIN balanced taps of w2 per output
          channel, d tokens and w3 at density 0.25, so that every sum stays exact over 1.4e5 .. 5.3e5 pixels.
  select  one operand one-hot at a position that walks (tap, channel) with the output index, the other arbitrary finite bf16 bit
          patterns (or the dense a1): every output is a bit copy and a failure names the tap.

`case` asserts the exact-sum bound of every quantity that is compared bit for bit, fits_bf16 of every value the class expects
unrounded, and the shares the classes exist for (ties: >= 5 % exact ties in y2, tokens, dy2; dense: >= 1 % of z1 and of z2 exactly
0 and >= 10 % on either side).  `restate(ops, stages, mut)` also carries the planted defects ("mutants": switches on this
restatement, never on a kernel) that tests/test_stem_exact.py must see.

Layouts here are PyTorch's: images [B, C, H, W], weights nn.Conv2d's; stored activations are given as bf16, exact values as
float64.  The sign of a zero is not part of any expectation."""
import functools

import torch
import torch.nn.functional as F

from _gemm_exact_cases import BF16, LIMIT, fits_bf16, gen, ints, is_tie, random_bf16, rne_bf16, walk

C1, C2, C3, NSLOT = 32, 64, 96, 48
SMALL_SHAPES = [(1, 4, 4), (1, 16, 32), (1, 20, 36), (2, 24, 40), (3, 52, 100)]
TRIP_SHAPE = (3, 144, 320)              # beyond one sweep of every tile kernel's grid, conv3_wgrad with per = 3
GROUP_SHAPE = (1, 512, 1028)            # 257 token groups: conv3_bwd_stats / conv3_bwd_data make a second trip
CLASSES = ("dense", "ties", "thin", "select")
W2_DENSE = 0.12                         # 0.25 puts sigma(y2) at 38: z2 == 0 on < 1 % and sum y2^2 past 2^24 at (3, 52, 100)
W2_DENSE_LARGE = 0.04                   # (3, 52, 100): sum y2^2 over 15600 pixels must stay below 2^24 on the channel with the largest mean
W2_THIN = 6                             # the same over 138240 pixels: 6 taps per output channel (density 0.02), three +1 and three -1, so
                                        # that the channel means of y2, which dominate sum y2^2 at random signs, vanish
TIE_S = 4                               # half of conv2's ~35 terms carries 2^4: 16 x sigma 18 puts y2 in [256, 1024); 11-16 % of y2 are ties
TIE_W3 = 0.03
MUTANTS = ("a1_halo", "mask1_ge", "mask2_ge", "trunc_y2", "trunc_tok", "trunc_dy2", "sums2_rounded", "transpose2", "transpose3",
           "drop_tail", "prefetch_mix")
# the stages a mutant changes; every backward stage takes the EXPECTED upstream tensors, as the GPU tests hand them to the kernels
MUTANT_STAGES = {"a1_halo": "BE", "mask1_ge": "E", "mask2_ge": "D", "trunc_y2": "B", "trunc_tok": "C", "trunc_dy2": "D",
                 "sums2_rounded": "B", "transpose2": "BE", "transpose3": "CD", "drop_tail": "CD", "prefetch_mix": "B"}


def launch_counts(B, H, W):
    """the launch rules of csrc/pswin_stem.hip, written out (grid_for :721, the entry points :750-867)"""
    t16, t8 = B * -(-H // 16) * -(-W // 32), B * -(-H // 8) * -(-W // 32)
    M = B * (H // 4) * (W // 4)
    nsteps = -(-M // 32)
    splits = min(nsteps, 128)
    per = -(-nsteps // splits)
    return dict(tiles16=t16, grid16=min(t16, 256), tiles8=t8, grid8=min(t8, 512), M=M, groups=-(-M // 128),
                grid_groups=min(-(-M // 128), 256), conv3_fwd_wgs=-(-M // 512), per=per, splits=-(-nsteps // per))


def _sparse(g, shape, density, hi=1):
    """float64 integers in {-hi..hi} \\ {0} at the given density, 0 elsewhere"""
    mag = torch.randint(1, hi + 1, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return mag * sign * (torch.rand(shape, generator=g) < density).double()


def _balanced(g, shape, k):
    """per output channel k weights of +-1 at random positions, as many +1 as -1"""
    n = shape[1] * shape[2] * shape[3]
    w = torch.zeros(shape[0], n, dtype=torch.float64)
    for o in range(shape[0]):
        pos = torch.randperm(n, generator=g)[:k]
        w[o, pos[:k // 2]], w[o, pos[k // 2:]] = 1.0, -1.0
    return w.view(shape)


def _pick(g, n, values):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), (n,), generator=g)]


def _ch(v):
    return v[None, :, None, None]


def trunc_bf16(t):
    """f32 -> bf16 by dropping the low 16 bits (a planted defect)"""
    return (t.float().view(torch.int32) & -65536).view(torch.float32).to(BF16)


def patches48(x):
    """[B, 3, H, W] -> [n, 48]: the zero-padded 3x3 patches of (x, ones), slot = tap * 4 + channel, slots 36..47 zero"""
    B, _, H, W = x.shape
    x4 = torch.cat([x, torch.ones(B, 1, H, W, dtype=x.dtype)], 1)
    p = F.unfold(x4, 3, padding=1).view(B, 4, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 36)
    return torch.cat([p, torch.zeros(B * H * W, 12, dtype=x.dtype)], 1)


def _pad_a1(a1, halo):
    """a1 with its one-pixel halo: zeros (conv2 zero-pads a1, not x), or a per-channel value (the a1_halo defect)"""
    p = F.pad(a1, (1, 1, 1, 1))
    if halo is not None:
        m = F.pad(torch.zeros_like(a1[:, :1]), (1, 1, 1, 1), value=1.0)
        p = p + m * _ch(halo)
    return p


def _exact(abs_sum, k=0):
    """the exactness bound for terms that are multiples of 2^-k"""
    return float(abs_sum) < LIMIT / 2 ** k


def _tiled_y2(ops, y2, grid, mix):
    """y2 of the tiles a 256-workgroup grid reaches on its second trip, tile by tile from the 20 x 36 input window as
    stem_conv2_fwd_kernel does; mix: the window is the one of tile t - grid (the prefetch that was never replaced)"""
    x, w1, w2 = ops["x"], ops["w1"], ops["w2"]
    B, _, H, W = x.shape
    nty, ntx = -(-H // 16), -(-W // 32)
    xp = F.pad(x, (2, 2 + 32, 2, 2 + 16))
    out = y2.clone()
    for t in range(grid, B * nty * ntx):
        b, r = divmod(t, nty * ntx)
        y0, x0 = 16 * (r // ntx), 32 * (r % ntx)
        sb, sr = divmod(t - grid if mix else t, nty * ntx)
        sy0, sx0 = 16 * (sr // ntx), 32 * (sr % ntx)
        win = xp[sb:sb + 1, :, sy0:sy0 + 20, sx0:sx0 + 36]
        a1 = rne_bf16(torch.relu(F.conv2d(win, w1) * _ch(ops["scale1"]) + _ch(ops["shift1"]))).double()
        gy, gx = torch.arange(y0 - 1, y0 + 17), torch.arange(x0 - 1, x0 + 33)
        inside = ((gy >= 0) & (gy < H))[:, None] & ((gx >= 0) & (gx < W))[None, :]
        tile = F.conv2d(a1 * inside.double(), w2)
        h, w = min(16, H - y0), min(32, W - x0)
        out[b, :, y0:y0 + h, x0:x0 + w] = tile[0, :, :h, :w]
    return out


def restate(ops, stages="ABCDE", mut=None, sums=True):
    """The stem in float64.  Stages: A conv1 statistics, B conv2 forward, C conv3 forward, D conv3 backward (statistics, data,
    weights), E conv2 backward (weights, data).  C and D take ops["y2"] if present, else the y2 of stage B; E takes ops["dy2_in"].
    sums = False leaves out what the `ties` class does not compare.  mut: one of MUTANTS."""
    o = {}
    x, w1, w2, w3 = ops.get("x"), ops.get("w1"), ops.get("w2"), ops.get("w3")
    dt = ops.get("dtype", torch.float64)
    if mut == "transpose2":
        w2 = w2.transpose(2, 3)
    if mut == "transpose3":
        w3 = w3.transpose(2, 3)
    if set(stages) & set("ABE"):
        y1 = F.conv2d(x, w1, padding=1)
        z1 = y1 * _ch(ops["scale1"]) + _ch(ops["shift1"])
        a1 = rne_bf16(torch.relu(z1)).double()
        o.update(y1=y1, z1=z1, a1=a1)
        halo = torch.relu(ops["shift1"]) if mut == "a1_halo" else None
    if "A" in stages:
        xp = patches48(x)
        o["sums1"] = torch.cat([y1.sum((0, 2, 3)), (y1 * y1).sum((0, 2, 3)), (xp.t() @ xp).reshape(-1)])
        o["bound_sums1"] = max(float(F.conv2d(x.abs(), w1.abs(), padding=1).sum((0, 2, 3)).max()), float((y1 * y1).sum((0, 2, 3)).max()),
                               float((xp.abs().t() @ xp.abs()).max()))
    if "B" in stages:
        y2 = F.conv2d(_pad_a1(a1, halo), w2)
        if mut == "prefetch_mix":
            y2 = _tiled_y2(ops, y2, 256, True)
        o["y2_exact"] = y2
        o["y2"] = trunc_bf16(y2) if mut == "trunc_y2" else rne_bf16(y2)
        s = o["y2"].double() if mut == "sums2_rounded" else y2
        o["sums2"] = torch.cat([s.sum((0, 2, 3)), (s * s).sum((0, 2, 3))])
        o["sums2_sum"] = o["sums2"][:C2]
        absy = F.conv2d(a1, w2.abs(), padding=1)
        o["bound_sums2_sum"] = float(absy.sum((0, 2, 3)).max())
        o["bound_y2"] = float(absy.max())
        o["bound_sums2"] = max(float(absy.sum((0, 2, 3)).max()), float((y2 * y2).sum((0, 2, 3)).max()))
    if set(stages) & set("CD"):
        y2b = (ops["y2"] if "y2" in ops else o["y2"]).to(dt)
        B, _, H, W = y2b.shape
        M = B * (H // 4) * (W // 4)
        tail = M % 16 if mut == "drop_tail" else 0
        z2 = y2b * _ch(ops["scale2"]).to(dt) + _ch(ops["shift2"]).to(dt)
        a2 = rne_bf16(torch.relu(z2)).to(dt)
        o.update(z2=z2, a2=a2)
    if "C" in stages:
        tok = F.conv2d(a2, w3, stride=4) + _ch(ops["bias3"])
        o["bound_tok"] = float((F.conv2d(a2, w3.abs(), stride=4) + _ch(ops["bias3"]).abs()).max())
        tok = tok.permute(0, 2, 3, 1).reshape(M, C3)
        o["tok_exact"] = tok
        o["tok"] = trunc_bf16(tok) if mut == "trunc_tok" else rne_bf16(tok)
        if tail:
            o["tok"][M - tail:] = float("nan")              # never written
    if "D" in stages:
        dtok = ops["dtok"].to(dt).clone()
        if tail:
            dtok[M - tail:] = 0
        dimg = dtok.view(B, H // 4, W // 4, C3).permute(0, 3, 1, 2)
        w3d = w3.to(dt)
        on = (z2 >= 0) if mut == "mask2_ge" else (z2 > 0)
        g2 = F.conv_transpose2d(dimg, w3d, stride=4) * on.to(dt)
        o["g2"] = g2
        k1, P, Q = (_ch(ops[k]).to(dt) for k in ("k1", "P", "Q"))
        dy2 = k1 * g2 - (P * y2b + Q)
        o["dy2_exact"] = dy2
        o["dy2"] = trunc_bf16(dy2) if mut == "trunc_dy2" else rne_bf16(dy2)
        if tail:                                            # the pixels of the dropped tokens are never written
            px = torch.zeros(M, dtype=torch.bool)
            px[M - tail:] = True
            px = px.view(B, 1, H // 4, 1, W // 4, 1).expand(B, C2, H // 4, 4, W // 4, 4).reshape(B, C2, H, W)
            o["dy2"] = torch.where(px, torch.full_like(o["dy2"], float("nan")), o["dy2"])
        if sums:
            sg = g2.sum((0, 2, 3), dtype=torch.float64)
            sgy = (g2 * y2b).sum((0, 2, 3), dtype=torch.float64)
            o["sums3"] = torch.cat([sg, ops["a2c"] * sgy + ops["b2c"] * sg])
            ag = g2.abs().sum((0, 2, 3), dtype=torch.float64)
            agy = (g2 * y2b).abs().sum((0, 2, 3), dtype=torch.float64)
            o["bound_sums3"] = float(torch.maximum(torch.maximum(ag, agy), ops["a2c"].abs() * agy + ops["b2c"].abs() * ag).max())
            o["dw3"] = torch.nn.grad.conv2d_weight(a2, w3.shape, dimg, stride=4).double()
            if mut == "transpose3":
                o["dw3"] = o["dw3"].transpose(2, 3)
            o["bound_dw3"] = float(torch.nn.grad.conv2d_weight(a2, w3.shape, dimg.abs(), stride=4).max())
    if "E" in stages:
        dy = ops["dy2_in"].double()
        a1p = _pad_a1(a1, halo)
        dw2 = torch.nn.grad.conv2d_weight(a1p, w2.shape, dy)
        o["dw2"] = dw2.transpose(2, 3) if mut == "transpose2" else dw2
        o["bound_dw2"] = float(torch.nn.grad.conv2d_weight(a1p, w2.shape, dy.abs()).max())
        on = (z1 >= 0) if mut == "mask1_ge" else (z1 > 0)
        g1 = F.conv_transpose2d(dy, w2, padding=1) * on.double()
        o["g1"] = g1
        yh1 = y1 * _ch(ops["a1c"]) + _ch(ops["b1c"])
        n = g1.shape[0] * g1.shape[2] * g1.shape[3]
        g1r = rne_bf16(g1).double().permute(0, 2, 3, 1).reshape(n, C1)
        xp = patches48(x)
        o["sg1"], o["sgy1"], o["G"] = g1.sum((0, 2, 3)), (g1 * yh1).sum((0, 2, 3)), g1r.t() @ xp
        o["bound_g1"] = float(F.conv_transpose2d(dy.abs(), w2.abs(), padding=1).max())
        o["bound_out5"] = max(float(g1.abs().sum((0, 2, 3)).max()), float((g1 * yh1).abs().sum((0, 2, 3)).max()))
        o["bound_G"] = float((g1r.abs().t() @ xp.abs()).max())
    return o


# what each stage's kernels return and the tests compare, per class (`ties`: element-wise outputs only)
STAGE_OUTPUTS = {"A": ("sums1",), "B": ("y2", "sums2"), "C": ("tok",), "D": ("sums3", "dy2", "dw3"), "E": ("dw2", "sg1", "sgy1", "G")}
TIES_OUTPUTS = ("y2", "tok", "dy2", "G")


def compared(cls, stage, shape):
    """`ties` also keeps the plain sum of y2 where it is still exact (up to 4096 pixels): the only place where y2 rounds AND a
    statistic is exact, i.e. where statistics taken from the rounded y2 would show"""
    if cls != "ties":
        return STAGE_OUTPUTS[stage]
    extra = ("sums2_sum",) if stage == "B" and shape[0] * shape[1] * shape[2] <= 4096 else ()
    return tuple(k for k in STAGE_OUTPUTS[stage] if k in TIES_OUTPUTS) + extra


def _shift2(y2b, scale2, g, half_ok):
    """per channel: minus the most frequent value of scale2 y2 that leaves >= 10 % of the channel on either side (the median's
    neighbourhood if none does), so that z2 == 0 is as frequent as the operands allow; + 0.5 on every eighth channel if it fits"""
    zs = (y2b * _ch(scale2)).permute(1, 0, 2, 3).reshape(C2, -1)
    sh = torch.zeros(C2, dtype=torch.float64)
    for c in range(C2):
        vals, cnt = torch.unique(zs[c], return_counts=True)
        below = torch.cumsum(cnt, 0) - cnt
        above = cnt.sum() - below - cnt
        ok = (below * 10 >= cnt.sum()) & (above * 10 >= cnt.sum())
        if bool(ok.any()):
            sh[c] = -vals[torch.argmax(cnt * ok)]
        else:
            sh[c] = -zs[c].median()
        if half_ok and c % 8 == 5 and float((zs[c] + sh[c]).abs().max()) < 127:
            sh[c] += 0.5
    return sh


def _operands(cls, B, H, W, seed):
    g = gen(1000003 * seed + 7919 * B + 31 * H + W + 101 * CLASSES.index(cls))
    thin, ties = cls == "thin", cls == "ties"
    M = B * (H // 4) * (W // 4)
    ops = dict(cls=cls)
    ops["x"] = _sparse(g, (B, 3, H, W), 0.66) if thin else ints(g, (B, 3, H, W), -2, 2)
    ops["w1"] = _sparse(g, (C1, 3, 3, 3), 0.5 if thin else 0.66)
    ops["scale1"] = torch.where(torch.arange(C1) % 5 == 0, -1.0, 1.0).double()
    ops["shift1"] = ints(g, (C1,), -3, 3)
    if thin:
        ops["w2"] = _balanced(g, (C2, C1, 3, 3), W2_THIN)
    else:
        ops["w2"] = _sparse(g, (C2, C1, 3, 3), W2_DENSE if ties or B * H * W <= 4096 else W2_DENSE_LARGE)
    if ties:
        ops["w2"][:, 0::2] *= 2.0 ** TIE_S
    ops["scale2"] = (torch.randint(0, 2, (C2,), generator=g).double() * 2 - 1) * (2.0 ** -TIE_S if ties else 1.0)
    ops["w3"] = _sparse(g, (C3, C2, 4, 4), TIE_W3 if ties else 0.25)
    ops["bias3"] = ints(g, (C3,), -8, 8)
    ops["dtok"] = _sparse(g, (M, C3), 0.25, 2) if thin else ints(g, (M, C3), -2, 2)
    ops["dy2_in"] = _sparse(g, (B, C2, H, W), 0.25 if thin else 0.5)
    if ties:
        ops["dtok"][:, 0::2] *= 2.0 ** TIE_S
        ops["dy2_in"][:, 0::2] *= 2.0 ** (TIE_S + 2 if B * H * W <= 4096 else TIE_S)       # (G over 15600 pixels stays below 2^24)
    # backward coefficients: (a, b) of yhat = a y + b, and (k1, P, Q) of dy2 = k1 g2 - P y2 - Q; pairs that keep dy2 in 8 bits
    ops["a1c"], ops["b1c"] = _pick(g, C1, [1, -1, 0.5, -0.5, 2, -2]), _pick(g, C1, [0, 1, -1, 2, -3, 0.5])
    ops["a2c"], ops["b2c"] = _pick(g, C2, [1, -1, 0.5, -0.5, 2, -2]), _pick(g, C2, [0, 1, -1, 2, -3, 0.5])
    pairs = torch.tensor([[1, 1], [-1, 1], [1, -1], [0.5, 0.5], [-0.5, 0.5], [0.5, -0.5], [2, 1], [-2, -1], [1, 0], [0.5, 0.25]],
                         dtype=torch.float64)[torch.randint(0, 10, (C2,), generator=g)]
    ops["k1"], ops["P"] = pairs[:, 0].clone(), pairs[:, 1].clone()
    ops["Q"] = _pick(g, C2, [1, -1, 2, -2, 3, 0.5, -0.5, 0])
    return ops, g


def _conditions(cls, ops, o, info):
    """asserts on a built dense / ties / thin case; fills info with the shares"""
    exact = cls != "ties"
    if "sums1" in o:
        assert _exact(o["bound_sums1"]), o["bound_sums1"]
    if "a1" in o:
        assert bool(fits_bf16(o["a1"]).all()) and bool((o["a1"] == torch.relu(o["z1"])).all())
    if "y2_exact" in o:
        assert _exact(o["bound_y2"])
        assert not exact or _exact(o["bound_sums2"]), o["bound_sums2"]
        assert not exact or bool(fits_bf16(o["y2_exact"]).all())
        assert exact or o["y2_exact"].numel() > 4096 * C2 or _exact(o["bound_sums2_sum"]), o["bound_sums2_sum"]
        info["y2_ties"] = float(is_tie(o["y2_exact"]).double().mean())
        info["y2_max"] = float(o["y2_exact"].abs().max())
    if "a2" in o:
        k = TIE_S + 1 if cls == "ties" else 1
        assert exact is False or bool((o["a2"] == torch.relu(o["z2"])).all())         # a2 itself rounds in `ties` (in the kernel too)
        assert bool(fits_bf16(o["a2"] * 2 ** k).all())
    if "tok_exact" in o:
        k = TIE_S + 1 if cls == "ties" else 1
        assert _exact(o["bound_tok"], k), o["bound_tok"]
        info["tok_ties"] = float(is_tie(o["tok_exact"] * 2 ** k).double().mean())
    if "dy2_exact" in o:
        assert _exact(float((ops["k1"].abs().max() * o["g2"].abs().max()) + 2 * 2.0 ** 16), 2)
        assert not exact or bool(fits_bf16(o["dy2_exact"] * 4).all())
        info["dy2_ties"] = float(is_tie(o["dy2_exact"] * 4).double().mean())
    if "sums3" in o and exact:
        assert _exact(o["bound_sums3"], 1), o["bound_sums3"]
        assert _exact(o["bound_dw3"], 1), o["bound_dw3"]
    if "dw2" in o:
        assert not exact or _exact(o["bound_dw2"]), o["bound_dw2"]
        assert _exact(o["bound_g1"]) and _exact(o["bound_G"]), (o["bound_g1"], o["bound_G"])
        assert not exact or (_exact(o["bound_out5"], 1) and bool(fits_bf16(o["g1"]).all())), o["bound_out5"]
        info["g1_ties"] = float(is_tie(o["g1"]).double().mean())
    if cls == "dense":
        for k in ("z1", "z2"):
            z = o[k]
            info[k + "_zero"], info[k + "_pos"], info[k + "_neg"] = (float((z == 0).double().mean()), float((z > 0).double().mean()),
                                                                     float((z < 0).double().mean()))
            assert info[k + "_zero"] >= 0.01 and info[k + "_pos"] >= 0.10 and info[k + "_neg"] >= 0.10, (k, info)
    if cls == "ties":
        assert min(info["y2_ties"], info["tok_ties"], info["dy2_ties"]) >= 0.05, info


class Case:
    def __init__(self, cls, shape, ops, out, info):
        self.cls, self.shape, self.ops, self.out, self.info = cls, shape, ops, out, info


@functools.lru_cache(maxsize=12)
def case(cls, B, H, W, seed=0):
    """-> Case: .ops the operands (float64; exact in bf16, or in f32 for x, bias3 and the prm rows), .out every expected output
    of restate() (bf16 for the stored activations, float64 for the sums and gradients), .info the shares reached"""
    assert cls in ("dense", "ties", "thin")
    ops, g = _operands(cls, B, H, W, seed)
    out = restate(ops, "ABE", sums=cls != "ties")
    ops["shift2"] = _shift2(out["y2"].double(), ops["scale2"], g, cls != "ties")
    if cls == "ties":
        ops["shift2"] = ops["shift2"].round()
    out.update(restate(dict(ops, y2=out["y2"].double()), "CD", sums=cls != "ties"))
    info = {}
    _conditions(cls, ops, out, info)
    return Case(cls, (B, H, W), ops, out, info)


@functools.lru_cache(maxsize=1)
def case_groups(B, H, W, seed=0):
    """`thin` for conv3_bwd_stats / conv3_bwd_data alone: y2 is generated directly (small integers).  float32 holds every
    element-wise value here exactly (integers and halves far below 2^24) and the sums are taken in float64."""
    ops, g = {}, gen(1000003 * seed + 7919 * B + 31 * H + W + 5)
    M = B * (H // 4) * (W // 4)
    ops.update(cls="thin", dtype=torch.float32)
    ops["y2"] = torch.randint(-6, 7, (B, C2, H, W), generator=g).float()
    ops["scale2"] = torch.randint(0, 2, (C2,), generator=g).double() * 2 - 1
    ops["shift2"] = ints(g, (C2,), -3, 3)
    ops["w3"] = _sparse(g, (C3, C2, 4, 4), 0.25).float()
    ops["dtok"] = _sparse(g, (M, C3), 0.25, 2).float()
    ops["a2c"], ops["b2c"] = _pick(g, C2, [1, -1, 0.5, -0.5]), _pick(g, C2, [0, 1, -1, 2, -3, 0.5])
    ops["k1"], ops["P"] = _pick(g, C2, [1, -1, 0.5, 2]), _pick(g, C2, [1, -1, 0.5, 0])
    ops["Q"] = _pick(g, C2, [1, -1, 2, -2, 3, 0.5, -0.5, 0])
    out = {}
    y2b = ops["y2"]
    z2 = y2b * _ch(ops["scale2"]).float() + _ch(ops["shift2"]).float()
    dimg = ops["dtok"].view(B, H // 4, W // 4, C3).permute(0, 3, 1, 2)
    g2 = F.conv_transpose2d(dimg, ops["w3"], stride=4) * (z2 > 0).float()
    assert float(g2.abs().max()) < 2 ** 10
    dy2 = _ch(ops["k1"]).float() * g2 - (_ch(ops["P"]).float() * y2b + _ch(ops["Q"]).float())
    assert bool(fits_bf16(dy2 * 4).all())
    out["dy2"] = dy2.to(BF16)
    sg, sgy = g2.sum((0, 2, 3), dtype=torch.float64), (g2 * y2b).sum((0, 2, 3), dtype=torch.float64)
    ag, agy = g2.abs().sum((0, 2, 3), dtype=torch.float64), (g2 * y2b).abs().sum((0, 2, 3), dtype=torch.float64)
    out["sums3"] = torch.cat([sg, ops["a2c"] * sgy + ops["b2c"] * sg])
    bound = float(torch.maximum(torch.maximum(ag, agy), ops["a2c"].abs() * agy + ops["b2c"].abs() * ag).max())
    assert _exact(bound, 1), bound
    return Case("thin", (B, H, W), ops, out, dict(g2_max=float(g2.abs().max()), bound_sums3=bound))


def _corner_walk(n_out, B, H, W):
    """one pixel per output channel: the four corners of the first and of the last image first, then a walk over all pixels"""
    n = B * H * W
    pix = [walk(i, n) for i in range(n_out)]
    corners = [0, W - 1, (H - 1) * W, H * W - 1]
    corners += [(B - 1) * H * W + c for c in corners]
    pix[:8] = corners
    return torch.tensor(pix)


@functools.lru_cache(maxsize=2)
def select_case(B, H, W, seed=0):
    """-> dict of sub-cases, one per kernel, each a Case whose compared output is a bit copy of one operand"""
    base, g = _operands("dense", B, H, W, seed + 77)
    base["shift2"] = torch.zeros(C2, dtype=torch.float64)
    M, n = B * (H // 4) * (W // 4), B * H * W
    sub = {}
    # conv2: w2 one-hot, y2[p][o] = a1[p + tap(o)][in(o)], zeros outside the image included
    ops = dict(base)
    k = walk(torch.arange(C2), 9 * C1)
    ops["w2"] = torch.zeros(C2, C1, 3, 3, dtype=torch.float64)
    ops["w2"][torch.arange(C2), k % C1, (k // C1) // 3, (k // C1) % 3] = 1.0
    out = restate(ops, "B")
    a1p = F.pad(out["a1"], (1, 1, 1, 1))
    for o_ in range(C2):
        tap, cin = int(k[o_]) // C1, int(k[o_]) % C1
        assert torch.equal(out["y2_exact"][:, o_], a1p[:, cin, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W])
    sub["conv2"] = Case("select", (B, H, W), ops, out, dict(pos=k))
    # conv3 kernels: y2 arbitrary finite bit patterns, BN2 the identity
    ident = dict(scale2=torch.ones(C2, dtype=torch.float64), shift2=torch.zeros(C2, dtype=torch.float64),
                 bias3=torch.zeros(C3, dtype=torch.float64), k1=torch.ones(C2, dtype=torch.float64),
                 P=torch.zeros(C2, dtype=torch.float64), Q=torch.zeros(C2, dtype=torch.float64))
    y2 = random_bf16(g, (B, C2, H, W)).double()
    # conv3_fwd: w3 one-hot per output channel, tok[t][o] = relu(y2[4 ty + ky(o)][4 tx + kx(o)][in(o)])
    ops = dict(ident, y2=y2)
    k = walk(torch.arange(C3), 16 * C2)
    ops["w3"] = torch.zeros(C3, C2, 4, 4, dtype=torch.float64)
    ops["w3"][torch.arange(C3), k % C2, (k // C2) // 4, (k // C2) % 4] = 1.0
    out = restate(ops, "C")
    assert bool((out["tok"].double() == out["tok_exact"]).all())
    sub["conv3_fwd"] = Case("select", (B, H, W), ops, out, dict(pos=k))
    # conv3_bwd_data: w3 one-hot over out per (tap, in), dy2[pixel][ch] = dtok[token][out(tap, ch)] where y2 > 0
    ops = dict(ident, y2=y2, dtok=random_bf16(g, (M, C3)).double())
    k = walk(torch.arange(16 * C2), C3).view(16, C2)                      # out of (tap, in)
    ops["w3"] = torch.zeros(C3, C2, 4, 4, dtype=torch.float64)
    tap, cin = torch.meshgrid(torch.arange(16), torch.arange(C2), indexing="ij")
    ops["w3"][k, cin, tap // 4, tap % 4] = 1.0
    ops["a2c"], ops["b2c"] = torch.ones(C2, dtype=torch.float64), torch.zeros(C2, dtype=torch.float64)
    out = restate(ops, "D", sums=False)
    assert bool((out["dy2"].double() == out["dy2_exact"]).all())
    sub["conv3_bwd_data"] = Case("select", (B, H, W), ops, out, dict(pos=k))
    # conv3_wgrad: d tokens one-hot over the tokens, one token per output channel: dw3[o] = the a2 patch of token t(o)
    ops = dict(ident, y2=y2, w3=torch.zeros(C3, C2, 4, 4, dtype=torch.float64))
    t = walk(torch.arange(C3), M)
    ops["dtok"] = torch.zeros(M, C3, dtype=torch.float64)
    ops["dtok"][t, torch.arange(C3)] = 1.0
    ops["a2c"], ops["b2c"] = torch.ones(C2, dtype=torch.float64), torch.zeros(C2, dtype=torch.float64)
    out = restate(ops, "D")
    a2t = out["a2"].view(B, C2, H // 4, 4, W // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(M, C2, 4, 4)
    assert torch.equal(out["dw3"], a2t[t])
    sub["conv3_wgrad"] = Case("select", (B, H, W), ops, out, dict(pos=t))
    # conv2_wgrad: dy2 one-hot over the pixels, one pixel per output channel: dw2[o] = the a1 patch around pixel p(o)
    ops = dict(base)
    p = _corner_walk(C2, B, H, W)
    dy = torch.zeros(n, C2, dtype=torch.float64)
    dy[p, torch.arange(C2)] = 1.0
    ops["dy2_in"] = dy.view(B, H, W, C2).permute(0, 3, 1, 2).contiguous()
    out = restate(ops, "E")
    pat = F.unfold(out["a1"], 3, padding=1).view(B, C1, 3, 3, H * W).permute(0, 4, 1, 2, 3).reshape(n, C1, 3, 3)
    assert torch.equal(out["dw2"], pat[p])
    sub["conv2_wgrad"] = Case("select", (B, H, W), ops, out, dict(pos=p))
    return sub


def differing(a, b):
    """number of elements whose values differ (NaN differs from everything; +0 equals -0)"""
    return int((~(a.double() == b.double())).sum())
