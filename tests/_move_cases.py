"""Operands on which the row movers, the column sums, the grouped reduction and the table-gradient kernels have ONE right answer, the
float64 definitions of those kernels and the judges of their results (CPU only; tests/test_move_cases.py checks the conditions below and
that every judge sees every planted defect, tests/test_move_exact_gpu.py runs the kernels of csrc/pswin_move.hip and the table-gradient
stages of csrc/pswin_attn.hip).

Every value is an integer or a dyadic rational and every partial sum stays below 2^24 units of its smallest lsb, so that the result is one
exact number in any order of operations, with or without FMA contraction; the float32 evaluation of a definition equals the float64 one bit
for bit.  Where an output is bf16 there are two operand classes: `exact` (the result is a bf16 value) and `ties` (the f32 result is an odd
integer in [257, 511], halfway between two bf16 values: what tells round-to-nearest-even from anything else).

A judge is a plain function judge_*(got, ...) -> list of complaints (empty: nothing to object to) on CPU tensors.
"""
import functools
import zlib

import torch

import panoswin_oracle as po
from _gemm_exact_cases import BF16, LIMIT, gen, ints, is_tie, rne_bf16

F32 = torch.float32
F64 = torch.float64
GUARD = 4                                                     # rows of sentinel before and after a caller-owned output
BITS = {F32: torch.int32, BF16: torch.int16}
SENTINEL = {F32: 0xDEADBEEF - (1 << 32), BF16: 0xBEEF - (1 << 16)}      # -6.2e18 / -0.467: no result of any case here
DT_NAME = {F32: "f32", BF16: "bf16"}


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def cast(want64, dtype):
    """the float64 definition cast ONCE to the output dtype (every finite value here is exact in f32, so f64 -> f32 rounds nothing)"""
    return want64.float() if dtype == F32 else rne_bf16(want64)


def fits(t, dtype):
    """every element of the float64 tensor is a value of dtype"""
    return bool((t.to(dtype).double() == t).all())


def judge_values(got, want64, what="values"):
    want = cast(want64, got.dtype)
    if got.shape != want.shape:
        return [f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"]
    if torch.equal(got, want):
        return []
    bad = torch.nonzero(got != want)
    at = tuple(bad[0].tolist())
    return [f"{what}: {len(bad)} of {got.numel()} elements differ, first at {at}: got {got[at].item()!r}, want {want[at].item()!r}"]


def guarded(rows, C, dtype, fill=None):
    """[GUARD + rows + GUARD, C] of the sentinel bit pattern; fill: the value of the rows in between (NaN for outputs that must be written)"""
    buf = torch.full((rows + 2 * GUARD, C), SENTINEL[dtype], dtype=BITS[dtype]).view(dtype)
    if fill is not None:
        buf[GUARD:GUARD + rows] = fill
    return buf


def judge_guard(buf, want64, what="guarded output"):
    """buf [GUARD + rows + GUARD, C] after the kernel wrote `rows` rows at row GUARD of a `guarded` buffer"""
    rows = buf.shape[0] - 2 * GUARD
    b, out, s = bits(buf), [], SENTINEL[buf.dtype]
    if not bool((b[:GUARD] == s).all()):
        out.append(f"{what}: the guard band before the output was written")
    if not bool((b[GUARD + rows:] == s).all()):
        first = int(torch.nonzero((b[GUARD + rows:] != s).any(1))[0])
        out.append(f"{what}: the guard band after the output was written (its row {first})")
    inner = buf[GUARD:GUARD + rows]
    unwritten = (bits(inner) == s) | torch.isnan(inner) & ~torch.isnan(cast(want64.reshape(inner.shape), buf.dtype))
    if bool(unwritten.any()):
        out.append(f"{what}: {int(unwritten.any(1).sum())} rows hold elements that were never written, first row {int(torch.nonzero(unwritten.any(1))[0])}")
    return out + judge_values(inner, want64.reshape(inner.shape), what)


# ---------------------------------------------------------------------------------------------------------------------
# A. window gather and scatter-add
# ---------------------------------------------------------------------------------------------------------------------
GEOMS = {"pano5x9s3": (True, 5, 9, 3), "planar8x9s3": (False, 8, 9, 3), "pano13x25s3": (True, 13, 25, 3)}
GEOM_COUNTS = {"pano5x9s3": (45, 98, 53), "planar8x9s3": (72, 196, 124), "pano13x25s3": (325, 392, 67)}        # S, slots, padding slots
PADDED_GEOMS = tuple(GEOMS)
TABLE_GEOMS = PADDED_GEOMS + ("ident333",)
PATH8_WIDTHS = (8, 96, 192, 384, 768, 2048)                  # C / 8 <= 256: the 8-wide kernels (f32 -> bf16 gather, bf16 -> f32 scatter)
WIDTHS = PATH8_WIDTHS + (2056,)                              # 2056: 514 vectors, three trips of the generic kernels' 256-wide v loop
DT_PAIRS = ((F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16))
FLAGS = tuple((s, r, b) for s in (False, True) for r in (False, True) for b in (False, True))       # (scale, resid, bias)
BIG_B = 65536                                                # grid.y is the image on the 8-wide path: B > 65535 takes the generic kernels


@functools.lru_cache(maxsize=None)
def maps(geom):
    """(map int64 [n_slots] with -1 in the padding slots, inv int64 [S]); "ident<n>": map = inv = arange(n), the Mlp residual's form"""
    if geom.startswith("ident"):
        a = torch.arange(int(geom[5:]))
        return a, a
    pano, H, W, s = GEOMS[geom]
    wmap = (po.pano_window_map if pano else po.planar_window_map)(H, W, s)[0]
    return wmap, po.invert_window_map(wmap, H * W)


def rpb8(C):
    """rows per row group of the 8-wide kernels: a 256-thread block is C / 8 lanes x rpb rows, two row groups (u = 0, 1) per thread"""
    return 256 // (C // 8)


def tail_kinds(n, C):
    """what the LAST block of an 8-wide launch over n rows looks like"""
    rpb = rpb8(C)
    blocks = -(-n // (2 * rpb))
    rem = n - (blocks - 1) * 2 * rpb                         # rows of the last block, 1 .. 2 rpb
    kinds = set()
    if rem <= rpb:
        kinds.add("u1_past")                                 # the second row group lies wholly past the end: every row of it is clamped
    if rpb < rem < 2 * rpb:
        kinds.add("u1_cut")                                  # ... is cut part-way
    if rem < rpb:
        kinds.add("u0_cut")                                  # the first row group is cut part-way
    if blocks == 1:
        kinds.add("single")
    return kinds


def required_tails(C):
    """C = 2048 has rpb = 1: a row group is ONE row and cannot be cut part-way, so only the other two configurations exist there"""
    return {"u1_past", "single"} | ({"u1_cut", "u0_cut"} if rpb8(C) >= 2 else set())


def extra_geoms(C):
    """identity maps whose row counts give the 8-wide kernels at width C every tail of required_tails, whatever the table supplies"""
    rpb = rpb8(C)
    if rpb == 1:
        return ("ident2", "ident3")
    h = max(1, rpb // 2)
    return tuple(f"ident{n}" for n in (2 * rpb + h, 3 * rpb + h, 3 * rpb, rpb + 1))


def geoms_for(C):
    return TABLE_GEOMS + (extra_geoms(C) if C in PATH8_WIDTHS else ())


def scales_for(B, seed):
    """per image, from {0, 0.5, 1, 2}: even images get 0 or 0.5, odd images 2"""
    s = torch.full((B,), 2.0, dtype=F64)
    s[0::2] = (0.0, 0.5)[seed % 2]
    return s


def gather_case(C, geom, xdt, wdt, scaled, cls="exact", B=2, scale=None):
    """win[b, slot] = scale_b * x[b, map[slot]], +0 in the padding slots.  exact: x integer in [-128, 128]; ties (f32 -> bf16 only): x an odd
    integer in [257, 511], or twice one under a scale of 0.5"""
    wmap, inv = maps(geom)
    seed = seed_of("gather", C, geom, DT_NAME[xdt], DT_NAME[wdt], scaled, cls, B)
    g = gen(seed)
    S = len(inv)
    if cls == "ties":
        assert xdt == F32 and wdt == BF16
        x = (2.0 * ints(g, (B, S, C), 128, 255) + 1.0) * (2.0 if scaled else 1.0)
        sc = torch.full((B,), 0.5, dtype=F64) if scaled else None
    else:
        x = ints(g, (B, S, C), -128, 128)
        sc = None if not scaled else (scales_for(B, seed) if scale is None else torch.tensor(scale, dtype=F64))
    return dict(kind="gather", C=C, B=B, S=S, n_slots=len(wmap), wmap=wmap, inv=inv, x=x, scale=sc, xdt=xdt, wdt=wdt, cls=cls)


def gather_def(c, dtype=F64, x=None, swap_scale=False):
    x = (c["x"] if x is None else x).to(dtype)
    wmap = c["wmap"]
    out = x[:, wmap.clamp(min=0)]
    if c["scale"] is not None:
        sc = c["scale"].flip(0) if swap_scale else c["scale"]
        out = out * sc.to(dtype)[:, None, None]
    out[:, wmap < 0] = 0.0                                   # +0 whatever row 0 holds
    return out


def scatter_case(C, geom, wdt, xdt, flags=(True, True, True), cls="exact", B=2):
    """out[b, t] = resid[b, t] + scale_b * (win[b, inv[t]] + bias); flags = (scale, resid, bias) given at all.
    exact, f32 out: win in [-64, 64], bias in [-32, 32], resid in [-128, 128]: an integer or half-integer of magnitude <= 320.
    exact, bf16 out: halved ranges and win, bias even: an integer of magnitude <= 256 (under the scale 0.5 too).
    ties (bf16 out, all three flags): resid an even integer in [272, 494] (a bf16 value), scale_b (win + bias) an odd integer in [-15, 15]
    under the scales (0.5, 1) -- a scale of 2 would make every product even."""
    wmap, inv = maps(geom)
    seed = seed_of("scatter", C, geom, DT_NAME[wdt], DT_NAME[xdt], flags, cls, B)
    g = gen(seed)
    S, n = len(inv), len(wmap)
    use_scale, use_resid, use_bias = flags
    if cls == "ties":
        assert xdt == BF16 and all(flags) and B == 2
        sc = torch.tensor([0.5, 1.0], dtype=F64)
        bias = ints(g, (C,), -16, 16)
        odd = 2.0 * ints(g, (B, n, C), -8, 7) + 1.0
        win = odd / sc[:, None, None] - bias
        resid = 2.0 * ints(g, (B, S, C), 136, 247)
    elif xdt == BF16:
        sc = scales_for(B, seed)
        win, bias, resid = 2.0 * ints(g, (B, n, C), -16, 16), 2.0 * ints(g, (C,), -8, 8), ints(g, (B, S, C), -64, 64)
    else:
        sc = scales_for(B, seed)
        win, bias, resid = ints(g, (B, n, C), -64, 64), ints(g, (C,), -32, 32), ints(g, (B, S, C), -128, 128)
    return dict(kind="scatter", C=C, B=B, S=S, n_slots=n, wmap=wmap, inv=inv, win=win, scale=sc if use_scale else None,
                resid=resid if use_resid else None, bias=bias if use_bias else None, wdt=wdt, xdt=xdt, cls=cls, flags=flags)


def scatter_def(c, dtype=F64, win=None, swap_scale=False, bias_after_scale=False):
    w = (c["win"] if win is None else win).to(dtype)[:, c["inv"]]
    sc = torch.ones(c["B"], dtype=dtype) if c["scale"] is None else (c["scale"].flip(0) if swap_scale else c["scale"]).to(dtype)
    sc = sc[:, None, None]
    b = 0.0 if c["bias"] is None else c["bias"].to(dtype)
    r = 0.0 if c["resid"] is None else c["resid"].to(dtype)
    if bias_after_scale:
        return r + (sc * w + b)
    return r + sc * (w + b)


def mover_conditions(c):
    """the exactness conditions of a gather / scatter case -> complaints"""
    out = []
    if c["kind"] == "gather":
        want, src_dt, dst_dt = gather_def(c), c["xdt"], c["wdt"]
        terms = c["x"].abs().max() * (1.0 if c["scale"] is None else float(c["scale"].abs().max()))
        operands = [("x", c["x"], src_dt)]
    else:
        want, src_dt, dst_dt = scatter_def(c), c["wdt"], c["xdt"]
        sc = 1.0 if c["scale"] is None else float(c["scale"].abs().max())
        terms = (0.0 if c["resid"] is None else c["resid"].abs().max()) + sc * (c["win"].abs().max() + (0.0 if c["bias"] is None else c["bias"].abs().max()))
        operands = [("win", c["win"], src_dt), ("resid", c["resid"], dst_dt), ("bias", c["bias"], F32)]
        # the sum of the terms' magnitudes (ties: 494 + 1 * (46 + 16); the RESULT is checked to lie in [257, 511] below)
        if float(terms) > (556 if c["cls"] == "ties" else 256 if dst_dt == BF16 else 320):
            out.append(f"magnitude {float(terms)} beyond the class's bound")
    for name, t, dt in operands:
        if t is not None and not fits(t, dt):
            out.append(f"{name} is not exact in {DT_NAME[dt]}")
    if not bool((2.0 * want == (2.0 * want).round()).all()):
        out.append("a result is neither an integer nor a half-integer")
    if not 2.0 * float(terms) < LIMIT:                        # sum of |terms| per output element, in units of the smallest lsb (1/2)
        out.append("the partial sums are not bounded by 2^24 lsbs")
    if not bool((want.float().double() == want).all()):
        out.append("the result is not exact in f32")
    if dst_dt == BF16:
        if c["cls"] == "ties":
            live = want != 0                                  # the padding slots of a gather stay +0
            if not (bool(is_tie(want[live]).all()) and bool(((want[live].abs() >= 257) & (want[live].abs() <= 511) & (want[live] % 2 == 1)).all())):
                out.append("a result of the ties class is no odd integer in [257, 511]")
        elif not fits(want, BF16):
            out.append("a result of the exact class is no bf16 value")
    return out


def gather_params():
    """(C, geom, xdt, wdt, scaled, class): every width x table geometry x dtype pair x with / without a scale, the ties class wherever the
    output is bf16 from f32, and the 8-wide kernels on the extra row counts of their width"""
    out = []
    for C in WIDTHS:
        for geom in geoms_for(C):
            for xdt, wdt in (DT_PAIRS if geom in TABLE_GEOMS else ((F32, BF16),)):
                for scaled in (False, True):
                    out.append((C, geom, xdt, wdt, scaled, "exact"))
                    if (xdt, wdt) == (F32, BF16):
                        out.append((C, geom, xdt, wdt, scaled, "ties"))
    return out


FLAG_WIDTHS_8, FLAG_WIDTH_GENERIC, FLAG_GEOMS = (96, 768), 96, ("pano5x9s3", "pano13x25s3")


def scatter_params():
    """(C, geom, wdt, xdt, (scale, resid, bias), class): all three flags at every width x table geometry x dtype pair (ties wherever the
    output is bf16) and on the 8-wide kernel's extra row counts; the other seven flag combinations on the 8-wide path at C = 96, 768 and on
    the generic f32 -> f32 kernel at C = 96"""
    out, all_on = [], (True, True, True)
    for C in WIDTHS:
        for geom in geoms_for(C):
            for wdt, xdt in (DT_PAIRS if geom in TABLE_GEOMS else ((BF16, F32),)):
                out.append((C, geom, wdt, xdt, all_on, "exact"))
                if xdt == BF16:
                    out.append((C, geom, wdt, xdt, all_on, "ties"))
    for flags in FLAGS[:-1]:
        for geom in FLAG_GEOMS:
            out += [(C, geom, BF16, F32, flags, "exact") for C in FLAG_WIDTHS_8] + [(FLAG_WIDTH_GENERIC, geom, F32, F32, flags, "exact")]
    return out


def mover_id(p):
    return "-".join(DT_NAME.get(v, "".join("SRB"[i] if f else "-" for i, f in enumerate(v)) if isinstance(v, tuple) else
                                ("scaled" if v is True else "plain" if v is False else f"C{v}" if isinstance(v, int) else str(v))) for v in p)


def takes_8wide(C, src_dt, dst_dt, kind, B=2):
    """the dispatch of pswin_window_gather (f32 -> bf16) and pswin_window_scatter_add (bf16 -> f32)"""
    pair = (F32, BF16) if kind == "gather" else (BF16, F32)
    return (src_dt, dst_dt) == pair and C // 8 <= 256 and B <= 65535


def round_ties_away(want64):
    """bf16 by round-half-AWAY (the planted defect): add half an ulp to the magnitude bits and truncate"""
    b = want64.float().contiguous().view(torch.int32)
    return ((b + 0x8000) >> 16).to(torch.int16).view(BF16)


def poison_row0(c):
    """x of a gather case with row 0 of image 0 = +inf and row 0 of image 1 = NaN"""
    x = c["x"].clone()
    x[0, 0] = float("inf")
    x[1, 0] = float("nan")
    return x


def judge_poisoned_gather(got, got_finite, c):
    """got: the gather of poison_row0(c); got_finite: the gather of c itself (already judged)"""
    wmap = c["wmap"]
    pads, row0 = wmap < 0, wmap == 0
    out = []
    if bool((bits(got[:, pads]) != 0).any()):
        out.append(f"{int((bits(got[:, pads]) != 0).any(2).sum())} padding slots are not +0 (first bits {int(bits(got[:, pads])[bits(got[:, pads]) != 0][0]):#x})")
    want = gather_def(c, x=poison_row0(c))[:, row0]
    g0 = got[:, row0].double()
    if not (torch.equal(torch.isinf(g0), torch.isinf(want)) and torch.equal(torch.isnan(g0), torch.isnan(want)) and bool((g0[0] > 0).all())):
        out.append("the slots of row 0 do not carry +inf (image 0) / NaN (image 1)")
    rest = ~(pads | row0)
    if not torch.equal(got[:, rest], got_finite[:, rest]):
        out.append("a slot of another row changed with the non-finite row")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# B. interp_rows and its adjoint
# ---------------------------------------------------------------------------------------------------------------------
INTERP_S = 45
INTERP_P = (1, 98, 333)
INTERP_C = (4, 8, 96, 768, 1028)         # 4: a 1 x 256 block; 1028: 257 vectors, a second trip of the v loop for one lane
INTERP_TABLES = ("random", "row7", "identity")


def tap_table(kind, P, S=INTERP_S):
    """(idx int64 [P, 4], w float64 [P, 4]): weights are multiples of 1/16 that sum to 1.
    random: about a quarter of the weights exactly 0, their indices left at 0 (as geometry.pitch_tables leaves them); the other taps point
    at rows 1 .. S - 1, so that row 0 is reached by zero-weight taps only.  row7: every tap of every row points at row 7.
    identity: idx[p] = (p, 0, 0, 0), w = (1, 0, 0, 0), P = S."""
    g = gen(seed_of("taps", kind, P, S))
    if kind == "identity":
        assert P == S
        idx, w = torch.zeros(P, 4, dtype=torch.int64), torch.zeros(P, 4, dtype=F64)
        idx[:, 0], w[:, 0] = torch.arange(P), 1.0
        return idx, w
    live = torch.rand(P, 4, generator=g) >= 0.25
    live[:, 0] |= ~live.any(1)
    w = torch.zeros(P, 4, dtype=F64)
    for p in range(P):
        k = int(live[p].sum())
        cuts = torch.sort(torch.randperm(15, generator=g)[:k - 1] + 1).values.tolist()            # k positive parts of 16
        parts = [b - a for a, b in zip([0] + cuts, cuts + [16])]
        w[p, live[p]] = torch.tensor(parts, dtype=F64) / 16.0
    idx = torch.full((P, 4), 7, dtype=torch.int64) if kind == "row7" else torch.randint(1, S, (P, 4), generator=g)
    if kind == "random":
        idx[w == 0] = 0
    return idx, w


def tap_matrix(idx, w, S, dtype=F64, zero_tap_weight=0.0):
    """dense T [P, S] accumulated from the taps; zero_tap_weight: what a tap of weight 0 contributes (the planted defect)"""
    P = idx.shape[0]
    T = torch.zeros(P, S, dtype=dtype)
    ww = torch.where(w == 0, torch.full_like(w, zero_tap_weight), w).to(dtype)
    for k in range(4):
        T.index_put_((torch.arange(P), idx[:, k]), ww[:, k], accumulate=True)
    return T


def interp_case(kind, P, C, B=2, S=INTERP_S):
    idx, w = tap_table(kind, P, S)
    g = gen(seed_of("interp", kind, P, C))
    return dict(kind=kind, P=P, C=C, B=B, S=S, idx=idx, w=w, x=ints(g, (B, S, C), -256, 256), dout=ints(g, (B, P, C), -256, 256))


def interp_def(c, dtype=F64, zero_tap_weight=0.0):
    """(out [B, P, C] = T x, dx [B, S, C] = T^T dout)"""
    T = tap_matrix(c["idx"], c["w"], c["S"], dtype, zero_tap_weight)
    return T @ c["x"].to(dtype), T.t() @ c["dout"].to(dtype)


def reached_rows(c):
    """bool [S]: the source rows some NON-ZERO tap points at"""
    return (tap_matrix(c["idx"], c["w"], c["S"]) != 0).any(0)


def interp_conditions(c):
    out = []
    w, T = c["w"], tap_matrix(c["idx"], c["w"], c["S"]).abs()
    if not (bool((16 * w == (16 * w).round()).all()) and bool((w.sum(1) == 1).all()) and bool((w >= 0).all())):
        out.append("the weights are no multiples of 1/16 that sum to 1")
    if c["kind"] == "random" and not 0.15 < float((w == 0).double().mean()) < 0.35 and c["P"] > 16:
        out.append("not about a quarter of the weights are 0")
    if bool((c["idx"][w == 0] != 0).any()) and c["kind"] != "row7":
        out.append("a zero-weight tap's index is not 0")
    if not 16.0 * max(float((T @ c["x"].abs()).max()), float((T.t() @ c["dout"].abs()).max())) < LIMIT:
        out.append("the partial sums are not bounded by 2^24 lsbs")
    return out


def judge_interp(out, dx, c):
    want_out, want_dx = interp_def(c)
    res = judge_values(out, want_out, "out") + judge_values(dx, want_dx, "dx")
    dead = ~reached_rows(c)
    if bool((dx[:, dead] != 0).any()):
        res.append(f"dx: a source row that no non-zero tap reaches is not 0 (rows {torch.nonzero(dead).flatten().tolist()[:4]} ...)")
    if c["kind"] == "identity" and not (torch.equal(out.double(), c["x"]) and torch.equal(dx.double(), c["dout"])):
        res.append("the identity table does not return x and dout themselves")
    return res


# ---------------------------------------------------------------------------------------------------------------------
# C. column sums
# ---------------------------------------------------------------------------------------------------------------------
ROWSUM_MAX_BLOCKS, ROWSUM_DIRECT_MAX_ROWS = 2048, 1024


def ve_of(dt):
    return 8 if dt == BF16 else 4


def rowsum_geom(M, N, dt):
    """rowsum_blocks of csrc/pswin_move.hip: -> dict(vpr column groups, vprb groups per block, rpi rows per trip, ychunks, R blocks in x)"""
    vpr = N // ve_of(dt)
    vprb = min(vpr, 256)
    rpi = 256 // vprb
    ychunks = -(-vpr // vprb)
    R = max(1, min(-(-M // (rpi * 8)), max(ROWSUM_MAX_BLOCKS // ychunks, 1)))
    return dict(vpr=vpr, vprb=vprb, rpi=rpi, ychunks=ychunks, R=R)


def takes_direct(M, N, dt):
    """pswin_colsum with an output: one pass of rowsum_direct_kernel"""
    return M <= ROWSUM_DIRECT_MAX_ROWS and N // ve_of(dt) >= 2048


DIRECT_N = {BF16: (16384, 16392), F32: (8192, 8200)}          # 2048 and 2049 (f32: 2050) column groups: a last block with one (two) live groups
DIRECT_M = (1, 7, 8, 9, 1024, 1025)                           # 1025: the two-stage path at the same width
STAGE2_R = (1, 63, 64, 65, 255, 256, 257)                     # bf16 N = 2048 (rpi = 1): the edges of colsum_kernel's r + 192 < R; r += 256 loop
TWO_STAGE = ((BF16, 288), (BF16, 3072), (BF16, 8), (F32, 8), (F32, 3072))
TWO_STAGE_M = (1, 1003, 1025, 4097)                           # 1003: no multiple of rpi * 8 at any of the widths
CAPPED = ((BF16, 2048, 16389), (F32, 1024, 16389))            # R = 2048 and blocks 0 .. 4 add a ninth row
OPS_COLSUM = ((BF16, 2048),) + TWO_STAGE
SKIP_CASES = ((BF16, 3072, 4097), (F32, 1536, 4097))          # 384 column groups: two y-chunks, the second half-empty


def colsum_cases():
    """(dtype, N, M, class) of every C-ABI call with an output"""
    out = [(dt, N, M, "ints") for dt in (BF16, F32) for N in DIRECT_N[dt] for M in DIRECT_M]
    out += [(dt, DIRECT_N[dt][1], M, "big") for dt in (BF16, F32) for M in (9, 1025)]
    out += [(BF16, 2048, 8 * R - 3, "ints") for R in STAGE2_R] + [(BF16, 2048, 8 * 257 - 3, "big")]
    out += [(dt, N, M, "ints") for dt, N in TWO_STAGE for M in TWO_STAGE_M] + [(dt, N, 1003, "big") for dt, N in TWO_STAGE]
    out += [(dt, N, M, "ints") for dt, N, M in CAPPED]
    return out


def skip_ranges(N, dt):
    """(lo, hi) in columns: empty, everything, inside the first chunk, straddling group 256, the last group only"""
    ve = ve_of(dt)
    return ((5 * ve, 5 * ve), (0, N), (3 * ve, 40 * ve), (250 * ve, 260 * ve), (N - ve, N))


def colsum_case(dt, N, M, cls="ints"):
    """x as integers [M, N] (int16 / int32: the large cases would not fit as float64): ints in [-64, 64]; big: one row of +-2^15 among ints
    in [-8, 8], so that a dropped or doubled row changes the high bits"""
    g = gen(seed_of("colsum", DT_NAME[dt], N, M, cls))
    if cls == "big":
        x = torch.randint(-8, 9, (M, N), generator=g, dtype=torch.int32)
        x[M // 2] = (2 * torch.randint(0, 2, (N,), generator=g, dtype=torch.int32) - 1) * 2 ** 15
    else:
        x = torch.randint(-64, 65, (M, N), generator=g, dtype=torch.int16)
    return dict(x=x, dt=dt, N=N, M=M, cls=cls, **rowsum_geom(M, N, dt))


def colsum_def(c, dtype=F64, drop=None, double=None):
    s = c["x"].sum(0, dtype=dtype)
    if drop is not None:
        s = s - c["x"][drop].to(dtype)
    if double is not None:
        s = s + c["x"][double].to(dtype)
    return s


def partial_def(c, dtype=F64, skip=None, sum_skipped=False):
    """[R, N]: the partial row of block bx sums the rows r with (r // rpi) % R == bx; columns [skip_lo, skip_hi) hold zeros"""
    owner = (torch.arange(c["M"]) // c["rpi"]) % c["R"]
    part = torch.zeros(c["R"], c["N"], dtype=dtype).index_add_(0, owner, c["x"].to(dtype))
    if skip is not None and not sum_skipped:
        part[:, skip[0]:skip[1]] = 0.0
    return part


def colsum_conditions(c):
    bound = float(c["x"].abs().sum(0, dtype=F64).max())
    out = [] if bound < LIMIT else ["the partial sums are not bounded by 2^24"]
    if not fits(c["x"][:: max(1, c["M"] // 64)].double(), c["dt"]):
        out.append("an operand is not exact in its dtype")
    return out


def judge_partials(ws, c, skip=None):
    """ws [R, N]: the first stage's partial rows; with a skip range the skipped columns must be +0"""
    out = judge_values(ws, partial_def(c, skip=skip), "partial rows")
    if skip is not None and bool((bits(ws[:, skip[0]:skip[1]]) != 0).any()):
        out.append("partial rows: a skipped column is not +0")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# D. pswin_reduce_jobs
# ---------------------------------------------------------------------------------------------------------------------
RJ_ROWS = (1, 2, 16, 17, 128, 129, 1000)
RJ_MAX = 96                                                   # jobs per launch: the job table travels in the kernel arguments


def rj_groups_per_block(rows):
    """G of reduce_jobs_kernel: 1024 column groups x 1 row lane, 128 x 8 or 16 x 64"""
    return 1024 if rows <= 16 else (128 if rows <= 128 else 16)


def reduce_specs():
    """(rows, dtype, cols, ld, column offset) of every job"""
    out = []
    for rows in RJ_ROWS:
        G = rj_groups_per_block(rows)
        for dt in (F32, BF16):
            ve = ve_of(dt)
            for groups in (1, G - 1, G, G + 1, 2 * G + 1):
                if groups < 1:
                    continue
                out.append((rows, dt, ve * groups, ve * groups, 0))
                out.append((rows, dt, ve * groups, ve * (groups + 2), ve))
    return out


def reduce_src(spec, i=0):
    rows, dt, cols, ld, off = spec
    return ints(gen(seed_of("reduce", rows, DT_NAME[dt], cols, ld, off, i)), (rows, ld), -64, 64)


def reduce_def(src64, spec, dtype=F64, ld_is_cols=False):
    rows, dt, cols, ld, off = spec
    if ld_is_cols:                                            # the planted defect: rows read `cols` apart
        return src64.flatten()[off:off + rows * cols].reshape(rows, cols).to(dtype).sum(0)
    return src64[:, off:off + cols].to(dtype).sum(0)


def cycled(lst, n):
    """n entries of lst: evenly spread over it when trimmed (so that every row count, i.e. every lane shape, stays in), cycled beyond"""
    if n <= len(lst):
        return [lst[i * len(lst) // n] for i in range(n)]
    return [lst[i % len(lst)] for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------------
# E. table gradients
# ---------------------------------------------------------------------------------------------------------------------
TOK, PADT, NBINS = 49, 64, 169
BIN = torch.tensor([[(i // 7 - j // 7 + 6) * 13 + (i % 7 - j % 7 + 6) for i in range(TOK)] for j in range(TOK)])        # [j][i]


def dtab_cap(heads):
    """the tile-count cap of dtab_blocks (csrc/pswin_attn.hip): stage-1 workgroups per head"""
    return min(128, max(16, -(-512 // heads)))


def dtab_blocks(n_tiles, heads):
    return min(n_tiles, dtab_cap(heads))


def _up(n, m):
    return -(-n // m) * m


def table_shapes():
    """(heads, n_tiles, n_bias_windows, n_dist).  Per head count, n_tiles over cap - 1, cap, cap + 1, 2 cap + 1 (and 1, 15 .. 17 at one head,
    where n_tiles itself is the block count) without and with ONE distance tile; then the three (nb, n_dist) with nb != n_tiles, at tile
    counts beyond the cap rounded up to a multiple of nb, which walk (tile % nb) % n_dist."""
    base = [(1, n) for n in (1, 15, 16, 17, 127, 128, 129, 257)] + [(3, 127), (3, 129)] + [(24, n) for n in (21, 22, 23, 45)]
    out = [(h, n, n, nd) for h, n in base for nd in (0, 1)]
    for nb, nd in ((12, 4), (15, 15), (20, 5)):
        out += [(1, _up(129, nb), nb, nd), (1, _up(257, nb), nb, nd), (3, _up(129, nb), nb, nd), (24, _up(23, nb), nb, nd), (24, _up(45, nb), nb, nd)]
    return out


def table_case(heads, n_tiles, nb, n_dist):
    """g: dScore tiles [n_tiles, heads, 49 j, 49 i] of integers in [-16, 16]; dist [n_dist, 49 j, 49 i] of multiples of 1/8 in [0, 4]"""
    g = gen(seed_of("table", heads, n_tiles, nb, n_dist))
    return dict(heads=heads, n_tiles=n_tiles, nb=nb, n_dist=n_dist, g=ints(g, (n_tiles, heads, TOK, TOK), -16, 16),
                dist=ints(g, (n_dist, TOK, TOK), 0, 32) / 8.0 if n_dist else None)


def table_def(c, dtype=F64, transposed_bins=False, plain_modulo=False, absolute=False):
    """(dalpha or None, dbeta), [169, heads]: the definition of test_table_grads_batch_matches_single_jobs (index_add_ over the 169 bins)"""
    g = c["g"].to(dtype)
    g = g.abs() if absolute else g
    heads = c["heads"]
    idx = (BIN.t() if transposed_bins else BIN).flatten()
    dbeta = torch.zeros(NBINS, heads, dtype=dtype).index_add_(0, idx, g.sum(0).permute(1, 2, 0).reshape(TOK * TOK, heads))
    dalpha = None
    if c["n_dist"]:
        tile = torch.arange(c["n_tiles"])
        d = c["dist"].to(dtype)[tile % c["n_dist"] if plain_modulo else (tile % c["nb"]) % c["n_dist"]]
        dalpha = torch.zeros(NBINS, heads, dtype=dtype).index_add_(0, idx, (g * d[:, None]).sum(0).permute(1, 2, 0).reshape(TOK * TOK, heads))
    return dalpha, dbeta


def table_conditions(c):
    da, db = table_def(c, absolute=True)
    bound = 8.0 * max(float(db.max()), 0.0 if da is None else float(da.max()))
    out = [] if bound < LIMIT else ["the partial sums are not bounded by 2^24 lsbs"]
    if c["n_dist"] and not (bool((8 * c["dist"] == (8 * c["dist"]).round()).all()) and float(c["dist"].min()) >= 0 and float(c["dist"].max()) <= 4):
        out.append("a distance is no multiple of 1/8 in [0, 4]")
    return out


def pad64(t49):
    """[..., 49, 49] -> [..., 64, 64], zeros beyond"""
    out = torch.zeros(t49.shape[:-2] + (PADT, PADT), dtype=t49.dtype)
    out[..., :TOK, :TOK] = t49
    return out


def judge_table(dalpha, dbeta, c):
    wa, wb = table_def(c)
    out = judge_values(dbeta, wb, "dbeta")
    if wa is not None:
        out += judge_values(dalpha, wa, "dalpha")
    return out


def random_bit_table(n):
    """int32 [n, 49, 49]: arbitrary bit patterns, NaN payloads (quiet and signalling), infinities and both zeros among them"""
    g = gen(seed_of("bit table", n))
    t = torch.randint(-2 ** 31, 2 ** 31, (n, TOK, TOK), generator=g, dtype=torch.int64).to(torch.int32)
    special = torch.tensor([0x7fc00001, 0x7f800001, 0x7fffffff, 0x7f800000, 0x00000000, 0x00000001], dtype=torch.int64)
    special = torch.cat([special, special - 2 ** 31]).to(torch.int32)               # the same with the sign bit set
    t.view(-1)[:: 97][: len(special)] = special
    return t
