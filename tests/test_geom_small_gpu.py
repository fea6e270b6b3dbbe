"""The HIP kernels behind the static tables of an attention block -- window map and inverse, pad slots, shifted-window mask, uv grid,
xyzuv features, per-window great-circle distances, 64 x 64 tiles -- on the grids the LAST stage of a small input runs on
(tests/_geom_cases.py): against what the live reference built (tests/golden/small_grids.npz), against float64, and end to end
against the CPU oracle at the input heights no golden reaches (last stage 3 x 6, 5 x 10, 6 x 12).  Needs an MI355X."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _geom_cases as gc
import panoswin_oracle as po
from _util import TINY, build_filled, compare_to_golden, golden, record, run_and_collect

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

PANO = [(H, W, s) for (H, W) in gc.SMALL_PANO for s in gc.SHIFTS]
PLANAR = [(H, W, s) for (H, W) in gc.SMALL_PLANAR for s in gc.SHIFTS]
_WORST = {}


def _record(**values):
    """the kernel's own worst figures, gathered over the tests of this file, under "geom_small_grids" of the parity report"""
    _WORST.update(values)
    record("geom_small_grids", delta_u24=gc.DELTA / gc.U24, **_WORST)


@pytest.fixture(scope="module")
def gold():
    return golden("small_grids")


@pytest.mark.parametrize("pano,cases", [(True, PANO), (False, PLANAR)])
def test_maps_pads_and_grid(ops, gold, pano, cases):
    from panoswintransformerobjectdetection_amd import _lib
    for (H, W, s) in cases:
        ref = gold[f"{'pano' if pano else 'planar'}_{H}x{W}_s{s}"]
        wmap, inv, nW = ops.window_maps(pano, H, W, s, DEV)
        assert wmap.dtype == torch.int32 and inv.dtype == torch.int32
        assert np.array_equal(wmap.cpu().numpy(), ref), (H, W, s)
        if pano:
            assert np.array_equal(inv.cpu().numpy(), gold[f"pano_inv_{H}x{W}_s{s}"]), (H, W, s)
        assert np.array_equal(ops.window_pads(pano, H, W, s, DEV).cpu().numpy(), np.nonzero(ref < 0)[0]), (H, W, s)
        Hp, Wp, n = gc.grid_dims(pano, H, W)
        assert ref.size == Hp * Wp == n * gc.WTOK
        assert _lib.window_grid(_lib.MODE_PANO if pano else _lib.MODE_PLANAR, H, W) == (Hp, Wp, n) and nW == n, (H, W, s)
        gc.check_map_invariants(wmap.cpu(), inv.cpu(), pano, H, W)


def test_planar_mask(ops, gold):
    for (H, W, s) in PLANAR:
        if not s:
            continue
        m = ops.planar_mask(H, W, s, DEV)
        assert m.dtype == torch.float32
        assert torch.equal(m.cpu(), torch.from_numpy(gold[f"mask_{H}x{W}_s{s}"]).float()), (H, W, s)
        assert torch.equal(m, m.transpose(1, 2)), (H, W, s)


def test_uv_grid_and_uv_windows(ops, gold):
    from panoswintransformerobjectdetection_amd._lib import PswinError
    for (H, W) in gc.SMALL_PANO:
        uv = ops.uv_grid(H, W, DEV)
        assert np.array_equal(uv.cpu().numpy().reshape(H, W, 2), gold[f"uv_{H}x{W}"]), (H, W)
        for s in (0, 3):
            wmap, _, nW = ops.window_maps(True, H, W, s, DEV)
            uvw = ops.gather_uv(uv, wmap).cpu()
            assert np.array_equal(uvw.numpy().reshape(nW, gc.WTOK, 2), gold[f"uvwin_{H}x{W}_s{s}"]), (H, W, s)
            assert bool((uvw[wmap.cpu() < 0] == 0).all()), (H, W, s)
    for (H, W) in [(3, 2), (2, 1), (8, 7)]:
        with pytest.raises(PswinError):
            ops.uv_grid(H, W, DEV)


def test_xyzuv_features_against_float64(ops):
    worst = 0.0
    for (H, W) in gc.SMALL_PANO:
        uv = ops.uv_grid(H, W, DEV).cpu()
        feat = ops.abs_pos_features(H, W, DEV).cpu()
        ref = gc.xyzuv64(uv)
        assert feat.shape == (H * W, 5) and torch.equal(feat[:, 3:], uv), (H, W)
        worst = max(worst, float(((feat.double() - ref).abs() / (gc.XYZ_RTOL * ref.abs() + gc.XYZ_ATOL)).max()))
        assert torch.allclose(feat.double(), ref, rtol=gc.XYZ_RTOL, atol=gc.XYZ_ATOL), (H, W)
    _record(xyzuv_err_over_tol=worst)


def test_grid_distances(ops):
    """ops.window_dist on every pano case and shift: every pair finite, in [0, f32(pi)], right in the sin^2 domain to DELTA, an exact 0
    where both slots hold the same uv, the table bit-symmetric; element-wise against the float64 cross-product distance where
    a64 <= A_KEEP, which leaves out at most SKIP_CAP of a case's pairs."""
    worst, n = [0.0, 0.0, 0.0], 0
    for (H, W, s) in PANO:
        wmap, _, nW = ops.window_maps(True, H, W, s, DEV)
        uvw = ops.gather_uv(ops.uv_grid(H, W, DEV), wmap).view(nW, gc.WTOK, 2)
        d = ops.window_dist(H, W, s, DEV)
        assert torch.equal(d, d.transpose(1, 2)), (H, W, s)
        res = gc.check_distances(d, uvw, uvw, (H, W, s), symmetric=True, elementwise=True)
        worst = [max(a, b) for a, b in zip(worst, res)]
        n += d.numel()
    print(f"\ngrids: {n} pairs: max sin^2-domain error {worst[0] / gc.U24:.3f} U24 (DELTA {gc.DELTA / gc.U24:.2f}), kept-pair error over "
          f"tolerance {worst[1]:.4f}, largest share with a64 > {gc.A_KEEP} in one case {worst[2]:.3%}")
    _record(grids_sin2_err_u24=worst[0] / gc.U24, grids_kept_err_over_tol=worst[1], grids_max_skipped_share=worst[2], grids_pairs=n)
    assert n == 436982


@pytest.mark.parametrize("name", list(gc.GENERATORS))
def test_generator_distances(ops, name):
    """ops.haversine_windows on adversarial uv: exact antipodes, a point against itself, points on the poles, pairs 1 / 2 / 4 ulp apart.
    The antipodal and pole windows are judged in the sin^2 domain only; the other two also element-wise where a64 <= A_KEEP."""
    gen, same = gc.GENERATORS[name]
    uv1, uv2 = gen()
    g1 = uv1.to(DEV)
    g2 = g1 if same else uv2.to(DEV)
    d = ops.haversine_windows(g1, g2)
    e, r, sk = gc.check_distances(d, uv1, uv2, name, symmetric=same, elementwise=name in ("self", "ulps"), capped=False)
    print(f"\n{name}: max sin^2-domain error {e / gc.U24:.3f} U24 (DELTA {gc.DELTA / gc.U24:.2f}), kept-pair error over tolerance {r:.4f}")
    _record(**{f"{name}_sin2_err_u24": e / gc.U24, f"{name}_kept_err_over_tol": r})


@pytest.mark.parametrize("n", [1, 3, 50])
def test_tiles(ops, n):
    """Tiles of a table with distinct entries (a permutation of 1 .. n * 2401, exact in f32): fwd holds the table, bwd its transpose
    (the same buffer when the caller says the table is symmetric), everything outside the 49 x 49 corner is an exact zero."""
    from panoswintransformerobjectdetection_amd._lib import WPAD
    g = torch.Generator().manual_seed(n)
    table = (torch.randperm(n * gc.WTOK * gc.WTOK, generator=g).float() + 1).view(n, gc.WTOK, gc.WTOK).to(DEV)
    pad = (0, WPAD - gc.WTOK, 0, WPAD - gc.WTOK)
    t = ops.Tiles(table)
    assert t.n == n and t.fwd.shape == t.bwd.shape == (n, WPAD, WPAD) and t.fwd.data_ptr() != t.bwd.data_ptr()
    assert torch.equal(t.fwd, F.pad(table, pad))
    assert torch.equal(t.bwd, F.pad(table.transpose(1, 2), pad))
    sym = table + table.transpose(1, 2)
    ts = ops.Tiles(sym, symmetric=True)
    assert ts.bwd is ts.fwd
    assert torch.equal(ts.fwd, F.pad(sym, pad)) and torch.equal(ts.fwd, ts.fwd.transpose(1, 2))


def test_distance_and_mask_tiles_of_a_map_smaller_than_one_window(ops):
    from panoswintransformerobjectdetection_amd._lib import WPAD
    pad = (0, WPAD - gc.WTOK, 0, WPAD - gc.WTOK)
    t = ops.window_dist_tiles(3, 6, 3, DEV)
    d = ops.window_dist(3, 6, 3, DEV)
    assert d.shape == (1, gc.WTOK, gc.WTOK) and t.bwd is t.fwd
    assert torch.equal(t.fwd, F.pad(d, pad)) and torch.equal(t.fwd, t.fwd.transpose(1, 2))
    t = ops.planar_mask_tiles(4, 7, 3, DEV)
    m = ops.planar_mask(4, 7, 3, DEV)
    assert m.shape == (1, gc.WTOK, gc.WTOK) and t.bwd is t.fwd
    assert torch.equal(t.fwd, F.pad(m, pad)) and torch.equal(t.fwd, t.fwd.transpose(1, 2))


class _AsGolden:
    """A result dict of run_and_collect with the interface compare_to_golden reads of an .npz handle (files, [key] -> ndarray)."""

    def __init__(self, res):
        self.res = res
        self.files = list(res)

    def __getitem__(self, k):
        return self.res[k].numpy()


@pytest.mark.parametrize("shape", [(1, 3, 96, 192), (2, 3, 160, 320), (1, 3, 192, 384)])
def test_tiny_pano_fp32_where_the_last_stage_is_3x6_5x10_6x12(shape):
    """Inputs of 96, 160 and 192 rows: stages end at 3 x 6, 5 x 10 and 6 x 12 tokens, where antipodal tokens share a window.  Against the
    oracle on the CPU (pinned to the live reference at the first two shapes by tests/test_oracle_vs_reference.py), at the tolerances of
    tests/test_backbone_gpu.py::test_tiny_models_fp32."""
    from panoswintransformerobjectdetection_amd import SimplePanoSwinTransformer
    want = run_and_collect(build_filled(po.SimplePanoSwinTransformerOracle, TINY, True, "tiny"), shape, "tiny")
    assert tuple(want["out3"].shape[2:]) == (shape[2] // 32, shape[3] // 32)
    res = run_and_collect(build_filled(SimplePanoSwinTransformer, TINY, True, "tiny").to(DEV), shape, "tiny", device=DEV)
    for k, v in res.items():
        assert bool(torch.isfinite(v).all()), k
    compare_to_golden(res, _AsGolden(want), rtol=1e-4, atol=5e-4, grad_rtol=2e-3, grad_atol_frac=1e-3,
                      report="tiny_pano_%dx%d_fp32" % shape[2:])
