"""Cases and float64 references for the static tables of an attention block on LAST-STAGE grids (2 to 8 rows): window maps, pad
slots, the shifted-window mask, the uv grid, xyzuv features and the per-window great-circle distances.  Shared by
tests/test_geom_cases.py (CPU: fallback.py and the oracle) and tests/test_geom_small_gpu.py (the HIP kernels).  numpy / torch only.

What happens on these grids and on no larger one: a pano map folds to less than one 7 x 7 window (3 x 6 -> 6 x 3 -> 18 tokens and 31
pad slots); a planar map has H < 7, so the roll happens inside the padding; and for H <= 6 a token (h, w) and its antipode
(H - 1 - h, w + W / 2) -- H rows apart in the north-south fold -- share a window, which never happens for H >= 8.  At an antipodal pair
the haversine argument a = sin^2(dv/2) + cos v1 cos v2 sin^2(du/2) is 1 up to rounding and d = 2 asin(sqrt(a)) is ill-conditioned
(d' = 1 / sqrt(a (1 - a))): an f32 result is off by up to 6.9e-4 there against 8.5e-7 elsewhere, and a > 1 would be a NaN.  So "the
distance is right" is judged in the well-conditioned domain, |sin^2(d / 2) - a64| <= DELTA, on EVERY pair, and element-wise against
float64 only where a64 <= A_KEEP.
"""
import math

import numpy as np
import torch

WS, WTOK = 7, 49
SHIFTS = tuple(range(7))
# (H, W) of the feature map; the same lists as oracle/gen_golden.py (SMALL_PANO, SMALL_PLANAR), which wrote tests/golden/small_grids.npz
SMALL_PANO = [(1, 2), (2, 4), (3, 5), (3, 6), (4, 7), (4, 8), (5, 9), (5, 10), (6, 11), (6, 12), (7, 13), (7, 14), (8, 16)]
SMALL_PLANAR = [(1, 1), (2, 4), (4, 7), (6, 6), (7, 7), (7, 8), (8, 13), (14, 15)]

# ---- constants of the checks, each with where it comes from ---------------------------------------------------------------------
U24 = 2.0 ** -24                     # half an ulp of an f32 in [0.5, 1): the unit the sin^2-domain figures are written in
# max |sin^2(d32 / 2) - a64| of the reference formula (po.haversine in f32 on the CPU; every entry was finite), measured with
# check_distances below and printed again by test_geom_cases.py::test_the_reference_formula_in_f32 (pytest -s):
#   13 pano grids x 7 shifts (436 982 pairs): 3.12 U24
#   generators: antipodes 4.49, self 4.39, poles 4.14, ulps 4.50 U24 (64 x 2 401 pairs each)
# It is what one expects of the formula: a is a sum of two products of f32-rounded sines and cosines (about 2 U24), the square root and
# the arc sine add a rounding each where d' is not large, and d near pi (ulp 2^-22) rounded to f32 moves sin^2(d / 2) by up to 0.5 U24.
REF_SIN2_ERR_GRIDS = 3.12 * U24
REF_SIN2_ERR_GENERATORS = 4.50 * U24
# the bound for the kernel: twice the larger figure, because the device's sinf / cosf / asinf are specified a little looser than libm's
DELTA = 2.0 * max(REF_SIN2_ERR_GRIDS, REF_SIN2_ERR_GENERATORS)          # 9.0 U24 = 5.4e-7
# haversine_kernel on an MI355X (the parity report's "geom_small_grids"): grids 4.71 U24, antipodes 5.20, self 4.99, poles 4.59, ulps
# 4.91; no NaN and no d > f32(pi) without a clamp of a, on these inputs.  Kept pairs: 0.034 (grids) and 0.065 of the tolerance.
# element-wise tolerance of tests/test_kernels_gpu.py::test_uv_grid_bit_exact_and_geometry (16 x 32), applied where a64 <= A_KEEP
D_RTOL, D_ATOL = 1e-5, 2e-6
A_KEEP = 0.99
# a64 > A_KEEP: 0.33 % of all grid pairs, at most 1.25 % in one (H, W, shift) case (measured, asserted per case by both test files)
SKIP_CAP = 0.02
# the reference formula in f32 stays at 0.027 of (D_RTOL, D_ATOL) on the kept pairs of the grids (worst: 8.5e-7, where a64 is just
# under A_KEEP and d' = 10).  The CPU test holds the oracle and fallback.py to a twentieth of the tolerance.
REF_KEPT_ERR_OVER_TOL = 0.027
REF_KEPT_BOUND = 0.05
# xyzuv features against float64 of the f32 uv: the project's numbers (tests/test_kernels_gpu.py, 16 x 32)
XYZ_RTOL, XYZ_ATOL = 1e-5, 1e-6
PI_F32 = float(np.float32(math.pi))


# ---- integer geometry -----------------------------------------------------------------------------------------------------------
def ceil_to(v, m=WS):
    return (v + m - 1) // m * m


def grid_dims(pano, H, W):
    """(Hp, Wp, nW) of the padded window grid: pano folds (H, W) to (2 H, ceil(W / 2)) first."""
    SH, SW = (2 * H, (W + 1) // 2) if pano else (H, W)
    Hp, Wp = ceil_to(SH), ceil_to(SW)
    return Hp, Wp, (Hp // WS) * (Wp // WS)


def check_map_invariants(wmap, inv, pano, H, W):
    """What holds for any correct map, without a fixture: every token once, map[inv[t]] == t, pad count nW * 49 - H * W."""
    wmap, inv = torch.as_tensor(wmap).long(), torch.as_tensor(inv).long()
    _, _, nW = grid_dims(pano, H, W)
    assert wmap.numel() == nW * WTOK and inv.numel() == H * W
    assert int(wmap.min()) >= -1 and int(wmap.max()) == H * W - 1
    assert torch.equal(torch.sort(wmap[wmap >= 0]).values, torch.arange(H * W))
    assert torch.equal(wmap[inv], torch.arange(H * W))
    assert int((wmap < 0).sum()) == nW * WTOK - H * W


# ---- float64 references ---------------------------------------------------------------------------------------------------------
def _pairs(uv1, uv2):
    a, b = torch.as_tensor(uv1).double(), torch.as_tensor(uv2).double()
    return a[..., :, None, :], b[..., None, :, :]


def dist64(uv1, uv2):
    """Great-circle distance in float64 WITHOUT the haversine form: unit vectors x = (cos v cos u, cos v sin u, sin v) of the f32 (u, v),
    then atan2(|x1 x x2|, x1 . x2), well conditioned at both ends.  [..., N, 2] x [..., M, 2] -> [..., N, M]."""
    def xyz(t):
        u, v = t[..., 0], t[..., 1]
        return torch.stack([torch.cos(v) * torch.cos(u), torch.cos(v) * torch.sin(u), torch.sin(v)], -1)

    a, b = _pairs(uv1, uv2)
    x1, x2 = torch.broadcast_tensors(xyz(a), xyz(b))
    return torch.atan2(torch.linalg.cross(x1, x2, dim=-1).norm(dim=-1), (x1 * x2).sum(-1))


def a64(uv1, uv2):
    """The haversine argument sin^2(dv / 2) + cos v1 cos v2 sin^2(du / 2) in float64 on the f32-rounded uv."""
    a, b = _pairs(uv1, uv2)
    du, dv = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1]
    return torch.sin(0.5 * dv) ** 2 + torch.cos(a[..., 1]) * torch.cos(b[..., 1]) * torch.sin(0.5 * du) ** 2


def sin2_err(d, a):
    """|sin^2(d / 2) - a64| in float64: the well-conditioned form of "d is the right distance"."""
    return (torch.sin(0.5 * torch.as_tensor(d).double()) ** 2 - a).abs()


def same_uv(uv1, uv2):
    """[..., N, M] bool: both slots hold the same (u, v) bit for bit (then d must be an exact 0)."""
    a, b = torch.as_tensor(uv1), torch.as_tensor(uv2)
    return (a[..., :, None, :] == b[..., None, :, :]).all(-1)


def xyzuv64(uv):
    """[sin u sin v, cos u sin v, cos v, u, v] in float64 of the f32 uv (HOT:926-932)."""
    t = torch.as_tensor(uv).double()
    u, v = t[..., 0], t[..., 1]
    return torch.stack([torch.sin(u) * torch.sin(v), torch.cos(u) * torch.sin(v), torch.cos(v), u, v], -1)


def check_distances(d, uv1, uv2, what, symmetric, elementwise, capped=True, delta=DELTA, tol_scale=1.0):
    """Every check of a distance table d [n, 49, 49] (f32) of uv1 x uv2 ([n, 49, 2] f32), on every pair.  symmetric: uv1 is uv2, the
    table must equal its transpose bit for bit.  elementwise: also |d - d64| <= D_RTOL d64 + D_ATOL where a64 <= A_KEEP; capped: with
    at most SKIP_CAP of the pairs left out (the grid cases; the antipodal and pole generators are judged in the sin^2 domain only).
    Returns (worst sin^2-domain error, worst kept-pair error over its tolerance, skipped fraction)."""
    d = torch.as_tensor(d).cpu()
    uv1, uv2 = torch.as_tensor(uv1).cpu(), torch.as_tensor(uv2).cpu()
    assert d.dtype == torch.float32 and d.shape == (uv1.shape[0], WTOK, WTOK), what
    assert bool(torch.isfinite(d).all()), (what, "not finite", int((~torch.isfinite(d)).sum()))
    assert float(d.min()) >= 0.0 and float(d.max()) <= PI_F32, (what, float(d.min()), float(d.max()))
    a = a64(uv1, uv2)
    e = sin2_err(d, a)
    assert float(e.max()) <= delta, (what, "sin^2 domain", float(e.max()) / U24, "U24 at", int(e.argmax()))
    same = same_uv(uv1, uv2)
    assert bool((d[same] == 0).all()), (what, "nonzero distance of a point to itself")
    if symmetric:
        assert torch.equal(d, d.transpose(1, 2)), (what, "not bit-symmetric")
    ratio, skipped = 0.0, 0.0
    if elementwise:
        keep = a <= A_KEEP
        skipped = 1.0 - float(keep.double().mean())
        assert skipped <= SKIP_CAP or not capped, (what, "ill-conditioned share", skipped)
        ref = dist64(uv1, uv2)
        r = (d.double() - ref).abs() / (tol_scale * (D_RTOL * ref + D_ATOL))
        ratio = float(r[keep].max())
        assert ratio <= 1.0, (what, "kept pairs: err / tol", ratio)
    return float(e.max()), ratio, skipped


# ---- adversarial uv windows for haversine_windows(uv1, uv2), which takes arbitrary uv ---------------------------------------------
N_GEN = 64


def _random_uv(seed, n=N_GEN):
    rng = np.random.RandomState(seed)
    u = rng.uniform(-math.pi, math.pi, (n, WTOK))
    v = rng.uniform(-math.pi / 2, math.pi / 2, (n, WTOK))
    return torch.from_numpy(np.stack([u, v], -1).astype(np.float32))


def gen_antipodes():
    """(a) 64 windows of 49 random points against their antipodes (u -+ pi, -v) in f32: the diagonal of every table is antipodal."""
    uv1 = _random_uv(1)
    pi = torch.tensor(PI_F32)
    uv2 = torch.stack([torch.where(uv1[..., 0] > 0, uv1[..., 0] - pi, uv1[..., 0] + pi), -uv1[..., 1]], -1)
    return uv1, uv2


def gen_self():
    """(b) the same points against themselves (one tensor for both sides): an exact-zero diagonal, a bit-symmetric table."""
    uv1 = _random_uv(1)
    return uv1, uv1


def gen_poles():
    """(c) points ON the poles, v = +-pi/2 as f32 (cos v = -4.4e-8, not 0), at random u, among ordinary points and one equator ring;
    against themselves.  Two slots on one pole are the same point at different uv: d is tiny, not an exact 0."""
    uv = _random_uv(2).clone()
    half = float(np.float32(math.pi / 2))
    uv[:, 0:16, 1] = half
    uv[:, 16:32, 1] = -half
    uv[:, 32:40, 1] = 0.0
    uv[1::2, 40:, 0] = 0.0                      # every other window: a meridian through both poles
    return uv, uv


def gen_ulps():
    """(d) pairs 1, 2 and 4 ulp apart: slot t of uv2 is slot t of uv1 moved by k ulp in u (t % 3 == 0), v (1) or both (2), k = 1, 2, 4
    by window.  Nothing here is the same uv, so no entry has to be an exact zero; all of them are tiny and none may be negative or NaN."""
    uv1 = _random_uv(3)
    bits = uv1.clone().view(torch.int32)
    k = torch.tensor([1, 2, 4], dtype=torch.int32)[torch.arange(N_GEN) % 3][:, None]
    t = torch.arange(WTOK)[None, :]
    bits[..., 0] += k * (t % 3 != 1)
    bits[..., 1] += k * (t % 3 != 0)
    uv2 = bits.view(torch.float32)
    assert bool(torch.isfinite(uv2).all()) and not bool((uv1 == uv2).all(-1).any())
    return uv1, uv2


# name -> (generator, uv1 is uv2)
GENERATORS = {"antipodes": (gen_antipodes, False), "self": (gen_self, True), "poles": (gen_poles, True), "ulps": (gen_ulps, False)}
