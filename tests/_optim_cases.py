"""Shared by tests/test_optim_cases.py (CPU) and tests/test_optim_exact_gpu.py: the float64 definition of the AdamW step of
csrc/pswin_optim.hip, a numpy float32 mirror of the kernels' own order of operations (one rounding per operation, the kernels are built
with -ffp-contract=off and their divisions and square roots are the correctly rounded sequences), the model of pswin_grad_sumsq's ranges
and of pswin_adamw_record's arithmetic in Python doubles, the operand classes, the planted defects and the judges.

The kernels are held to the mirror BIT FOR BIT.  The bounds of the mirror against the float64 definition count f32 roundings
(U = 2^-24 each) along the kernel's order and are applied to the magnitudes of the float64 intermediates; none was taken from a kernel's
output.  They prove that the mirror is AdamW, and they are what p falls back to should a division or a root turn out not to be
correctly rounded on the device.

NaN: IEEE 754 leaves the sign and the payload of a NaN that an invalid operation produces (inf * 0 here) to the implementation, so
the host this mirror runs on and gfx950 need not agree on them (x86's default NaN has the sign bit set).  same_bits() therefore asks
of a NaN only that it is a NaN at the same element; everything else, -0 included, is compared as a bit pattern."""
import math
import types

import numpy as np

F = np.float32
U = 2.0 ** -24                   # unit roundoff of f32
ETA = 2.0 ** -150                # the most a rounding to an f32 denormal (or to 0) loses, absolute
F32_MAX = float(np.finfo(np.float32).max)
BF16_OVERFLOW = float(np.array([0x7F7F8000], dtype=np.uint32).view(np.float32)[0])
MAX_GROUPS, PARTIALS, SQ_THREADS = 8, 1024, 256          # include/pswin.h, pswin_optim.hip
SWEEP4 = 256 * 256 * 16                                  # granules one trip of the update kernels' capped grid covers
RECIPE = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, wd=0.05)                  # the reference configs' optimizer
# (lr_mult, decay_mult) of the eight groups: the base group, a frozen one, no decay, and multipliers that are no powers of two
GROUP_MULTS = ((1.0, 1.0), (0.0, 0.0), (1.0, 0.0), (0.1, 0.5), (2.0, 3.0), (0.5, 1.0), (1.0, 2.0), (0.3, 0.7))
T_VALUES = (1, 2, 10, 1000, 6931, 100000)
SIZES = (4, 1024, 1028, 4 * SWEEP4 + 4, 4 * 100003)
CLASSES = ("training", "isolate_step", "isolate_decay", "eps_regime", "extremes", "ties")


def gam(k):
    """Higham's gamma_k: k roundings of relative size U, second-order terms included"""
    return k * U / (1.0 - k * U)


# ---- the constants of a launch -----------------------------------------------------------------------------------------------------
def _shift(x, ulps):
    return x + ulps * math.ulp(x)


def constants(lrs, t, b1, b2, eps, wd, decay_mults=None, lr_mults=None, pow_shift=(0, 0), defect=None):
    """The f32 constants of one launch, formed in double and rounded once as the kernels do.  lrs: the lr of every group in double
    (lr * (double)(float)lr_mult[k] on the plain path, the record's lr[k] on the scheduled one).  pow_shift moves the two results of
    pow by that many double ulps (safe_constants)."""
    lrs = np.broadcast_to(np.asarray(lrs, dtype=np.float64), (MAX_GROUPS,))
    dm = np.ones(MAX_GROUPS) if decay_mults is None or defect == "decay_mult_ignored" else \
        np.asarray([float(F(x)) for x in decay_mults], dtype=np.float64)
    tt = float(F(t)) - (1.0 if defect == "bias_t_minus_1" else 0.0)
    bc1 = np.float64(1.0 - _shift(math.pow(b1, tt), pow_shift[0]))
    bc2 = 1.0 - _shift(math.pow(b2, tt), pow_shift[1])
    c = types.SimpleNamespace(t=tt)
    with np.errstate(all="ignore"):
        if defect == "betas_f32":
            c.w1, c.w2 = F(1.0) - F(b1), F(1.0) - F(b2)
        else:
            c.w1, c.w2 = F(1.0 - b1), F(1.0 - b2)
        c.b1, c.b2, c.eps = F(b1), F(b2), F(eps)
        c.bc2s = F(math.sqrt(bc2))
        c.step_g = (lrs / bc1).astype(np.float32)
        dl = lrs * np.asarray(lr_mults, dtype=np.float64) if defect == "lr_mult_twice" else lrs
        c.decay_g = (dl * (wd * dm)).astype(np.float32)
    return c


def _const_bits(c):
    return np.concatenate([np.asarray([c.w1, c.w2, c.b2, c.eps, c.bc2s], dtype=np.float32), c.step_g, c.decay_g]).view(np.uint32)


def safe_constants(lrs, t, b1, b2, eps, wd, decay_mults=None):
    """True when no f32 constant changes while either pow result moves by up to 16 double ulps, the error the OpenCL specification
    allows a double pow: the device's pow need not be libm's.  (1 - x is monotone in x, so the two ends decide.)"""
    want = _const_bits(constants(lrs, t, b1, b2, eps, wd, decay_mults))
    return all(np.array_equal(want, _const_bits(constants(lrs, t, b1, b2, eps, wd, decay_mults, pow_shift=(a, b))))
               for a in (-16, 16) for b in (-16, 16))


def safe_t(t, lrs, b1, b2, eps, wd, decay_mults=None):
    """t, or the next step number after it whose constants are safe"""
    while not safe_constants(lrs, t, b1, b2, eps, wd, decay_mults):
        t += 1
    return t


def group_lrs(lr, mults=GROUP_MULTS):
    """lr of every group on the plain path: lr * (double)(float)lr_mult[k]; groups past the last run with multiplier 1"""
    m = [float(F(a)) for a, _ in mults] + [1.0] * (MAX_GROUPS - len(mults))
    return np.asarray([lr * x for x in m], dtype=np.float64)


def group_map(n4, run):
    """group of every granule: (i // run) % 8, the last granule one group further than its neighbour"""
    k = ((np.arange(n4) // run) % MAX_GROUPS).astype(np.uint8)
    if n4 > 1:
        k[-1] = (int(k[-2]) + 1) % MAX_GROUPS
    return k


# ---- the float32 mirror ------------------------------------------------------------------------------------------------------------
UPDATE_DEFECTS = ("decay_after_step", "eps_inside", "betas_f32", "no_lerp", "w2_gg", "bias_t_minus_1", "coef_not_in_v", "coef_stored",
                  "decay_mult_ignored", "lr_mult_twice", "group_next", "group_prev", "shadow_truncated", "shadow_before_update")
SUMSQ_DEFECTS = ("partial_short", "partial_overlap")
RECORD_DEFECTS = ("coef_no_1e6", "guard_on_norm_f")
DEFECTS = UPDATE_DEFECTS + SUMSQ_DEFECTS + RECORD_DEFECTS


def bf16_rne(x):
    """f32 -> bf16 bits (uint16), round to nearest even; a NaN stays a NaN"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((b + (np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)
    return np.where(np.isnan(x), ((b >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def bf16_value(bits):
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def mirror_update(p, g, m, v, c, group_of=None, coef=None, defect=None):
    """One step of adamw_flat_kernel / adamw_flat_sched_kernel on f32 arrays, in the kernels' order; c = constants(...).
    coef: the record's f32 clip coefficient (scheduled path), None on the plain path.  -> dict(p, m, v, shadow, g): g is the
    gradient buffer after the step, which the kernels never write."""
    for a in (p, g, m, v):
        assert a.dtype == np.float32
    n4 = p.size // 4
    k = np.zeros(n4, dtype=np.int64) if group_of is None else group_of.astype(np.int64)
    if defect == "group_next":
        k = np.roll(k, -1)
    elif defect == "group_prev":
        k = np.roll(k, 1)
    kk = np.repeat(k, 4)
    step, decay = c.step_g[kk], c.decay_g[kk]
    with np.errstate(all="ignore"):
        gs = g if coef is None else g * F(coef)                                   # 1. g' = g * coef
        gv = g if defect == "coef_not_in_v" else gs
        pe = p if defect == "decay_after_step" else p - decay * p                 # 2. pe -= decay * pe
        me = c.b1 * m + c.w1 * gs if defect == "no_lerp" else m + c.w1 * (gs - m)  # 3. me = m + w1 (g' - m)
        ve = c.b2 * v + (c.w2 * (gv * gv) if defect == "w2_gg" else (c.w2 * gv) * gv)      # 4. ve = b2 v + (w2 g') g'
        root = np.sqrt(ve)
        denom = (root + c.eps) / c.bc2s if defect == "eps_inside" else root / c.bc2s + c.eps   # 5.
        pe = pe - (step * me) / denom                                             # 6. pe -= (step_size me) / denom
        if defect == "decay_after_step":
            pe = pe - decay * pe
    for a in (pe, me, ve):
        assert a.dtype == np.float32
    if defect == "shadow_truncated":
        shadow = (pe.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    else:
        shadow = bf16_rne(p if defect == "shadow_before_update" else pe)          # 7. RNE to bf16
    return dict(p=pe, m=me, v=ve, shadow=shadow, g=gs if defect == "coef_stored" else g)


# ---- the float64 definition and the bounds of the mirror against it ----------------------------------------------------------------
def definition(p, g, m, v, lrs, t, b1, b2, eps, wd, decay_mults=None, group_of=None, coef=1.0):
    """torch.optim.AdamW with decoupled decay, by hand in float64, for group k with lr lrs[k] and weight decay wd * decay_mult[k]:
        p <- p - lr_k wd_k p;  m <- m + (1 - b1)(g' - m);  v <- b2 v + (1 - b2) g'^2;  p <- p - (lr_k / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    with g' = coef g.  The multipliers are the f32 values the entry points take."""
    lrs = np.broadcast_to(np.asarray(lrs, dtype=np.float64), (MAX_GROUPS,))
    dm = np.ones(MAX_GROUPS) if decay_mults is None else np.asarray([float(F(x)) for x in decay_mults], dtype=np.float64)
    n4 = p.size // 4
    kk = np.repeat(np.zeros(n4, dtype=np.int64) if group_of is None else group_of.astype(np.int64), 4)
    r = types.SimpleNamespace()
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        r.step = (lrs / (1.0 - b1 ** float(t)))[kk]
        r.bc2s = math.sqrt(1.0 - b2 ** float(t))
        r.G = coef * g
        r.Dp = (lrs * wd * dm)[kk] * p
        r.P1 = p - r.Dp
        r.Gm = r.G - m
        r.m = m + (1.0 - b1) * r.Gm
        r.v = b2 * v + (1.0 - b2) * r.G * r.G
        r.R = np.sqrt(r.v) / r.bc2s + eps
        r.S = r.step * r.m / r.R
        r.p = r.P1 - r.S
        # elements whose f32 evaluation leaves the f32 range although the definition does not: (w2 g') g' or v beyond the f32 maximum
        r.overflow = np.isfinite(v) & ((np.abs((1.0 - b2) * r.G * r.G) > F32_MAX) | (r.v > F32_MAX))
    r.w1, r.w2, r.b2, r.eps = 1.0 - b1, 1.0 - b2, b2, eps
    return r


def bounds(r, clipped=True):
    """Allowed |mirror - definition| per element.  Every f32 constant is a double rounded once (U); every operation rounds once (U of
    its result, or ETA where the result is an f32 denormal).  Along the kernel's order:
      g'     = fl(g coef_f): coef's rounding and the product: gam(2) |G|  (0 without clipping: `clipped`)
      p1     = fl(p - fl(decay_f p)): decay and its product gam(2) |D p|, the difference U |P1|               -> gam(3) |D p| + U |P1| + 2 ETA
      m      d = fl(g' - m): the error of g' and U |G - m|;  x = fl(w1_f d): w1 and the product, gam(2) more;  fl(m + x): U |M|
                                                                                  -> W1 (1 + gam(3)) e(g') + gam(4) W1 |G - m| + U |M| + 3 ETA
      v      fl(b2_f v): gam(2) B2 v;  fl(fl(w2_f g') g'): w2, two products and g' twice: gam(7) W2 G^2; the sum: U V.  All terms
             are positive, so the whole is at most gam(8) V, and ETA (1 + |G|) for a product that underflows (the first one's loss
             is multiplied by g')
      R      sqrt halves the relative error of v and rounds once: gam(5), and sqrt of v's absolute loss; / bc2s_f: gam(2) more;
             + eps_f: U eps and U R.  sqrt(v) / bc2s <= R and eps <= R, so the whole is at most gam(8) R plus the absolute part
      S      fl(fl(step_f m) / R): step, the product, the division and R's gam(8): gam(12) |S| (1 / (1 - x) folded into gam),
             m's error times STEP / R, and ETA / R for a product that underflows
      p      fl(p1 - S): U |P| and the two errors
      shadow RNE to bf16: half a bf16 ulp, at most 2^-8 of the value (2^-134 for a bf16 denormal), on top of p's
    An element with `overflow` has no bound on v, p and the shadow (the class states what it must be instead); one whose v is already
    inf must give exactly what the definition gives."""
    absG = np.abs(r.G)
    with np.errstate(all="ignore"):
        e_g = gam(2) * absG + ETA if clipped else np.zeros_like(absG)
        e_p1 = gam(3) * np.abs(r.Dp) + U * np.abs(r.P1) + 2 * ETA
        e_m = r.w1 * (1 + gam(3)) * e_g + gam(4) * r.w1 * np.abs(r.Gm) + U * np.abs(r.m) + 3 * ETA
        abs_v = ETA * (2.0 + absG)
        e_v = gam(8) * r.v + abs_v
        abs_r = np.sqrt(abs_v) / r.bc2s * (1 + gam(3)) + ETA
        rel_s = gam(12) + abs_r / r.R * (1 + gam(12))
        e_s = rel_s * np.abs(r.S) + (1 + gam(12)) * r.step * e_m / r.R + ETA / r.R + ETA
        e_p = (e_p1 + e_s) * (1 + U) + U * np.abs(r.p) + ETA
        e_sh = e_p + 2.0 ** -8 * (np.abs(r.p) + e_p) + 2.0 ** -134
    inf = np.full_like(absG, np.inf)
    vinf = np.isinf(r.v)
    t = dict(m=e_m, v=np.where(r.overflow, inf, np.where(vinf, 0.0, e_v)))
    t["p"] = np.where(r.overflow, inf, np.where(vinf, e_p1 * (1 + U) + U * np.abs(r.p) + ETA, e_p))
    t["shadow"] = np.where(r.overflow, inf, np.where(vinf, t["p"] + 2.0 ** -8 * (np.abs(r.p) + t["p"]) + 2.0 ** -134, e_sh))
    return t


def ratios(got, r, tol):
    """{quantity: largest |got - definition| / bound}: an element with a zero bound must be exact, an inf of the definition must be
    met, a NaN never passes"""
    out = {}
    for k in ("p", "m", "v", "shadow"):
        want = r.p if k == "shadow" else getattr(r, k)
        x = (bf16_value(got[k]) if k == "shadow" else got[k]).astype(np.float64)
        with np.errstate(all="ignore"):
            err = np.abs(x - want)
            err = np.where(x == want, 0.0, err)                   # inf - inf
            if k == "shadow":                                     # RNE beyond the largest bf16 (0x7F7F) is inf, from 0x7F7F8000 on
                err = np.where(np.isinf(x) & (np.sign(x) == np.sign(want)) & (np.abs(want) + tol["p"] >= BF16_OVERFLOW), 0.0, err)
            q = np.where(err == 0, 0.0, err / tol[k])
        q = np.where(np.isnan(x) | np.isnan(q), np.inf, q)
        q = np.where(np.isinf(tol[k]), 0.0, q)
        out[k] = float(q.max())
    return out


def same_bits(got, want):
    """number of elements whose bit patterns differ (f32 as int32, the shadow as uint16), a NaN matching any NaN; and the first one"""
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        nan_a, nan_b = np.isnan(a), np.isnan(b)
        a, b = a.view(np.uint32), b.view(np.uint32)
    elif a.dtype == np.uint16:
        nan_a, nan_b = np.isnan(bf16_value(a)), np.isnan(bf16_value(b))
    else:
        nan_a = nan_b = np.zeros(a.shape, dtype=bool)
    bad = np.where(nan_a | nan_b, nan_a != nan_b, a != b)
    n = int(bad.sum())
    return n, (int(np.argmax(bad)) if n else -1)


def ulp_distance(got, want):
    """largest distance of two finite f32 arrays in units in the last place"""
    def key(x):
        b = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return int(np.abs(key(got) - key(want)).max())


# ---- operand classes ---------------------------------------------------------------------------------------------------------------
def hyper(name):
    """the hyper-parameters a class runs with"""
    return dict(RECIPE, wd=0.0) if name == "ties" else dict(RECIPE)


def _training_g(rng, n):
    g = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    u = rng.random(n)
    tiny = (10.0 ** rng.uniform(-9, -7, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)
    g = np.where(u < 0.05, F(0), np.where(u < 0.10, tiny, g))
    if n >= 64:                      # small buffers too meet both kinds
        g[1::40], g[2::40] = F(0), tiny[2::40]
    return g.astype(np.float32)


def _warm_state(rng, n, steps=3):
    """m, v after `steps` mirror steps of the recipe from zero on gradients of the training kind"""
    h = RECIPE
    p, m, v = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    for t in range(1, steps + 1):
        out = mirror_update(p, _training_g(rng, n), m, v, constants(h["lr"], t, h["b1"], h["b2"], h["eps"], h["wd"]))
        m, v = out["m"], out["v"]
    return m, v


G_EXTREME = np.array([0.0, -0.0, 1.4e-45, -1e-40, 5e-39, 1e-30, -1e-30, 1e19, -1e20, 3e38, -3e38, 1e20, 1e-3], dtype=np.float32)
P_EXTREME = np.array([0.0, -0.0, 1e-40, -1e-44, 1e30, -1e30, 0.02], dtype=np.float32)
V_EXTREME = np.array([0.0, np.inf, 1e-6], dtype=np.float32)
M_EXTREME = np.array([0.0, -2.5e-4], dtype=np.float32)
TIE_LOW = np.array([0x7FFF, 0x8000, 0x8001], dtype=np.uint32)


def operands(name, seed, n, warm=False):
    """p, g, m, v (f32 numpy arrays of n elements) of one class.
      training       p ~ N(0, 0.02); g ~ N(0, 1e-3) with 5 % exact zeros and 5 % of magnitude 1e-9 .. 1e-7; m, v zero or (warm) the state
                     after three mirror steps
      isolate_step   training with p = 0: the decay term vanishes, the new p is the Adam term alone
      isolate_decay  g = m = v = 0: the new p is p - decay p, m and v stay +0
      eps_regime     m = v = 0, |g| log-uniform within 1e-12 .. 1e-6: 95 % in 1.6e-10 .. 1e-6, 5 % in 1e-12 .. 1.6e-10, so that at t = 1, 2
                     sqrt(v) / bc2s (= |g| at t = 1, 0.71 |g| at t = 2) lies within two decades of eps on either side for at least 90 % of the elements
      extremes       every combination of G_EXTREME x P_EXTREME x V_EXTREME x M_EXTREME (the lengths are coprime: element j takes entry
                     j mod length of each).  In the kernel's order (w2 g) g, |g| = 1e19 and 1e20 give a finite v, at 1e20 although g g itself
                     (1e40) is beyond the f32 range; |g| = 3e38 gives v = inf, a step of exactly 0 and a finite p
      ties           g = m = v = 0 (run with wd = 0: the update is the identity); p sweeps the bf16 ties (low half 0x8000) and their two
                     neighbours over every sign, exponents 0 .. 254 and even, odd and all-ones kept mantissas"""
    rng = np.random.default_rng(1000 * seed + CLASSES.index(name))
    z = np.zeros(n, dtype=np.float32)
    if name in ("training", "isolate_step"):
        m, v = _warm_state(rng, n) if warm else (z.copy(), z.copy())
        p = z.copy() if name == "isolate_step" else (rng.standard_normal(n) * 0.02).astype(np.float32)
        return p, _training_g(rng, n), m, v
    if name == "isolate_decay":
        p = (rng.standard_normal(n) * 0.02).astype(np.float32)
        p[::7] *= F(50.0)
        return p, z.copy(), z.copy(), z.copy()
    if name == "eps_regime":
        e = np.where(rng.random(n) < 0.95, rng.uniform(-9.8, -6, n), rng.uniform(-12, -9.8, n))
        g = (10.0 ** e * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)
        return z.copy(), g, z.copy(), z.copy()
    j = np.arange(n)
    if name == "extremes":
        return (P_EXTREME[j % 7].copy(), G_EXTREME[j % 13].copy(), M_EXTREME[j % 2].copy(), V_EXTREME[j % 3].copy())
    if name == "ties":
        low = TIE_LOW[j % 3]
        mant = np.array([0x00, 0x01, 0x2A, 0x55, 0x7E, 0x7F], dtype=np.uint32)[(j // 3) % 6]
        sign = ((j // 18) % 2).astype(np.uint32)
        expo = ((j // 36) * 7 + seed) % 255                                      # 0 (denormals) .. 254, all of them within 9180 elements
        bits = (sign << np.uint32(31)) | (expo.astype(np.uint32) << np.uint32(23)) | (mant << np.uint32(16)) | low
        return bits.astype(np.uint32).view(np.float32).copy(), z.copy(), z.copy(), z.copy()
    raise KeyError(name)


def check_class(name, p, g, m, v, t=1):
    """the conditions a class states about itself (asserted), on buffers large enough to show them -> the shares, for the report"""
    n = p.size
    h = hyper(name)
    c = constants(h["lr"], t, h["b1"], h["b2"], h["eps"], h["wd"])
    out = mirror_update(p, g, m, v, c)
    rep = {}
    if name in ("training", "isolate_step"):
        rep["zeros"], rep["tiny"] = float((g == 0).mean()), float(((np.abs(g) >= 1e-9) & (np.abs(g) <= 1e-7)).mean())
        if n >= 64:
            assert rep["zeros"] >= 0.02 and rep["tiny"] >= 0.02, rep
        if n >= 1024:
            assert 0.04 <= rep["zeros"] <= 0.10 and 0.04 <= rep["tiny"] <= 0.10, rep
        if name == "isolate_step":
            assert not p.any() and not np.signbit(p).any()
    elif name == "isolate_decay":
        assert not g.any() and not m.any() and not v.any() and p.all()
        assert same_bits(out["m"], np.zeros_like(m))[0] == 0 and same_bits(out["v"], np.zeros_like(v))[0] == 0     # +0, not -0
        with np.errstate(all="ignore"):
            assert same_bits(out["p"], p - c.decay_g[0] * p)[0] == 0
        rep["moved"] = float((out["p"] != p).mean())
        assert rep["moved"] >= 0.9 or n < 64
    elif name == "eps_regime":
        assert t in (1, 2) and not m.any() and not v.any()
        with np.errstate(all="ignore"):
            q = np.sqrt(out["v"].astype(np.float64)) / float(c.bc2s)
        rep["within_two_decades"] = float(((q >= 1e-10) & (q <= 1e-6)).mean())
        rep["below_eps"], rep["above_eps"] = float((q < 1e-8).mean()), float((q > 1e-8).mean())
        assert (np.abs(g) >= 0.99e-12).all() and (np.abs(g) <= 1.01e-6).all()
        if n >= 1024:
            assert rep["within_two_decades"] >= 0.90 and rep["below_eps"] >= 0.2 and rep["above_eps"] >= 0.2, rep
    elif name == "extremes":
        assert not any(np.isnan(out[k]).any() for k in ("p", "m", "v")) and np.isfinite(out["p"]).all()
        if n >= 7 * 13 * 3 * 2:
            ag = np.abs(g.astype(np.float64))
            # by magnitude with room around the f32 values (float32(1e19) lies below 1e19, float32(1e20) above 1e20)
            big, huge, fin = (ag > 9e18) & (ag < 2e20), ag > 2.9e38, np.isfinite(v)
            with np.errstate(all="ignore"):
                sq_over = big & (ag > 5e19)                                      # |g| = 1e20: g g = 1e40 is beyond f32, (w2 g) g = 1e37 is not
                assert np.isinf(g[sq_over] * g[sq_over]).all() and np.isfinite(g[big & ~sq_over] * g[big & ~sq_over]).all()
                assert np.isfinite(out["v"][big & fin]).all() and (out["v"][big & fin] > 1e34).all()
                assert np.isinf(out["v"][huge]).all() and np.isinf(out["v"][~fin]).all()
                stay = huge | ~fin                                                # the step is exactly 0: p is the decayed p
                assert same_bits(out["p"][stay], (p - c.decay_g[0] * p)[stay])[0] == 0
            den = (g != 0) & (ag < 1.17e-38)
            # the shares G_EXTREME gives them: 3, 2 and 3 of its 13 entries; a third of the elements start from v = inf
            assert abs(big.mean() - 3 / 13) < 0.01 and abs(huge.mean() - 2 / 13) < 0.01 and abs(den.mean() - 3 / 13) < 0.01
            assert abs((~fin).mean() - 1 / 3) < 0.01 and (big & fin).mean() > 0.15 and abs(sq_over.mean() - 2 / 13) < 0.01
            assert ((g[den] * g[den]) == 0).all() and (out["m"][den & (ag > 1e-43) & (m == 0)] != 0).all()
            for s, arr in (("g", g), ("p", p)):
                assert (arr == 0).any() and np.signbit(arr[arr == 0]).any() and not np.signbit(arr[arr == 0]).all(), s
            rep.update(v_inf=float(np.isinf(out["v"]).mean()), g_1e19_1e20=float(big.mean()), gg_overflows=float(sq_over.mean()), g_3e38=float(huge.mean()), g_denormal=float(den.mean()))
    elif name == "ties":
        low = p.view(np.uint32) & np.uint32(0xFFFF)
        assert np.isin(low, TIE_LOW).all() and np.isfinite(p).all() and h["wd"] == 0.0
        assert same_bits(out["p"], p)[0] == 0                                     # the identity on finite p
        rep["ties"], rep["neighbours"] = float((low == 0x8000).mean()), float((low != 0x8000).mean())
        assert rep["ties"] + rep["neighbours"] == 1.0
        if n >= 36 * 255:
            assert (bf16_rne(p) != (p.view(np.uint32) >> np.uint32(16))).mean() >= 0.4     # rounding up where truncation does not
            assert len(np.unique((p.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF))) >= 200
    return rep


# ---- pswin_grad_sumsq --------------------------------------------------------------------------------------------------------------
SUMSQ_N4 = (1, 1023, 1024, 1025, 768 * 1024, 768 * 1024 + 1, 1024 * 1024, 1024 * 1024 + 1024)


def partial_ranges(n4, defect=None):
    """[(lo, hi)] in granules: chunk = ceil(n4 / 1024), partial b covers [b chunk, min((b + 1) chunk, n4)) (include/pswin.h)"""
    chunk = -(-n4 // PARTIALS)
    out = []
    for b in range(PARTIALS):
        lo, hi = min(b * chunk, n4), min((b + 1) * chunk, n4)
        if defect == "partial_short" and hi > lo:
            hi -= 1
        if defect == "partial_overlap" and hi > lo:
            hi = min(hi + 1, n4)
        out.append((lo, hi))
    return out


def partial_sums(g, defect=None, exact=False):
    """the 1024 range sums of g^2 in double (a square of an f32 is exact in double): numpy's sum, which is exact and order-free for
    the integer gradients, or math.fsum (exact=True)"""
    sq = g.astype(np.float64) ** 2
    out = np.zeros(PARTIALS)
    for b, (lo, hi) in enumerate(partial_ranges(g.size // 4, defect)):
        seg = sq[4 * lo:4 * hi]
        out[b] = math.fsum(seg) if exact else seg.sum()
    return out


def partial_bound(n4):
    """Allowed |partial - fsum| relative to the range's sum (all terms are positive): the kernel adds in double, the squares are exact.
    A thread takes every 256th granule of its range: 3 additions inside a granule and one into its accumulator, then the 8 levels
    of the LDS tree: at most 4 ceil(chunk / 256) + 8 additions in a chain, 2^-53 each."""
    k = 4 * -(-(-(-n4 // PARTIALS)) // SQ_THREADS) + 8
    return k * 2.0 ** -53 / (1.0 - k * 2.0 ** -53)


def integer_gradient(seed, n):
    """integers in [-64, 64] with a third of zeros: every sum of squares is exact in double, in any order"""
    rng = np.random.default_rng(seed)
    g = rng.integers(-64, 65, n).astype(np.float32)
    g[rng.random(n) < 0.33] = 0.0
    return g


# ---- pswin_adamw_record ------------------------------------------------------------------------------------------------------------
def record_sum(partials):
    """adamw_record_kernel's sum of the 1024 partials in its own order: four in a row per thread, then the fixed LDS tree"""
    s = np.zeros(SQ_THREADS)
    with np.errstate(all="ignore"):
        for j in range(PARTIALS // SQ_THREADS):
            s = s + partials[j::PARTIALS // SQ_THREADS]
        w = SQ_THREADS // 2
        while w > 0:
            s[:w] = s[:w] + s[w:2 * w]
            w //= 2
    return float(s[0])


def record_model(sumsq, sched, lr, lr_mults, max_norm, skip_nonfinite, step, iteration, skipped, defect=None, norm=None):
    """pswin_adamw_record in Python doubles.  sumsq: the sum of the partials (None: no partials); sched: optim.parse_lr_config's dict;
    step / iteration / skipped: the counters before; norm: the norm itself instead of sumsq (a recorded one).
    -> dict of the record's fields and the counters after."""
    from panoswintransformerobjectdetection_amd.optim import scheduled_lr
    if norm is None:
        norm = 0.0 if sumsq is None else (math.sqrt(sumsq) if sumsq >= 0 and not math.isnan(sumsq) else math.nan)
    with np.errstate(all="ignore"):
        norm_f = F(norm)
        finite = bool(np.isfinite(norm_f)) if defect == "guard_on_norm_f" else math.isfinite(norm)
        coef = 1.0
        if max_norm > 0:
            c = max_norm / (norm + (0.0 if defect == "coef_no_1e6" else 1e-6))
            coef = 1.0 if c > 1.0 else c
        coef_f = F(coef)
    applied = (not skip_nonfinite) or finite
    mults = [float(F(x)) for x in (lr_mults if lr_mults is not None else [])] + [1.0] * MAX_GROUPS
    i = int(iteration)
    lrs = [scheduled_lr(sched, lr * mults[k], i) for k in range(MAX_GROUPS)]
    t = F(step) + F(1.0) if applied else F(step)
    return dict(lr=lrs, norm=norm, lr_base=F(lrs[0]), norm_f=norm_f, coef=coef_f, t=t, applied=int(applied), iteration=i,
                step_after=t, iteration_after=F(i + 1), skipped_after=F(skipped) + (F(0.0) if applied else F(1.0)))


FIXED = dict(policy="fixed", by_epoch=False)
# a constant warmup: one product with the ratio, no pow (gamma^0)
SCHED_CONSTANT = dict(policy="step", by_epoch=False, warmup="constant", warmup_iters=40, warmup_ratio=0.3, step=[1000, 2000])
# no pow in it while i < 40: linear warmup, e = 0 (gamma^0 is 1 in any pow)
SCHED_NO_POW = dict(policy="step", by_epoch=False, warmup="linear", warmup_iters=40, warmup_ratio=0.001, step=[1000, 2000])
# pow in both places: gamma^e with e >= 1, and the exponential warmup
SCHED_POW = dict(policy="step", by_epoch=False, warmup="exp", warmup_iters=40, warmup_ratio=0.001, step=[3, 7], gamma=0.3)


def f64_ulps(a, b):
    """distance of two finite doubles of one sign in units in the last place"""
    x, y = np.asarray([a, b], dtype=np.float64).view(np.int64)
    return abs(int(x) - int(y))
