"""Host-side rules of the product that need no GPU: the feature list behind PSWIN_DISABLE, the row-tile rule of the tiled GEMM, the
row-split rule of the grouped weight gradients (the kernel's XCD-aware map expects 1, 2, 4 or a multiple of 8 splits)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    import panoswintransformerobjectdetection_amd.ops as ops
    return ops


def test_pswin_disable_turns_named_features_off_and_nothing_else():
    """(in a process of its own: the switches are read once, at import)"""
    code = ("import panoswintransformerobjectdetection_amd.ops as o; "
            "print(int(o.GROUPED_WGRAD), int(o.GEMM_NT), int(o.FUSED_WINDOW_ATTENTION), int(o.FUSED_MLP), int(o.LN_FUSED_MOVES), "
            "int(o.DEFER_TABLE_PARTIALS), int(o.GEMM_TN_RING), o.gemm_nt_tile(16384, 384, 1536))")
    env = dict(os.environ, PSWIN_DISABLE="grouped_wgrad, GEMM_NT", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0", "0", "1", "1", "1", "1", "1", "0"]                   # gemm_nt off: the library takes the layer (tile 0)
    ops = _ops()
    if not os.environ.get("PSWIN_DISABLE"):
        assert ops.GROUPED_WGRAD and ops.GEMM_NT


@pytest.mark.parametrize("M,K,N,tile", [
    (16384, 384, 1536, 128),      # stage 2 fc1, batch 8: 1,024 tiles of 128 rows = two rounds of the 512 tile slots
    (16384, 1536, 384, 128),      # stage 2 fc2: 512 tiles of 64 rows, but 256 of 128 rows fit the chip once (four-stage form)
    (19600, 384, 384, 96),        # stage 2 proj: 614 tiles of 64 rows spill into a second round, 410 of 96 rows do not
    (19600, 1152, 384, 96),       # stage 2 qkv data gradient
    (74480, 192, 576, 128),       # stage 1 qkv: many rounds
    (5880, 768, 2304, 128),       # stage 3 qkv forward at batch 8: 552 tiles of 128 rows -> the HIP kernel
    (4096, 3072, 768, 0),         # stage 3 fc2 forward: long contraction over 128 tiles -> the library
    (4900, 384, 1152, 0),         # stage 2 qkv at batch 2 -> the library
    (4900, 384, 384, 64),         # stage 2 proj at batch 2: 154 tiles, four-stage form
])
def test_row_tile_rule_of_the_tiled_gemm(M, K, N, tile):
    assert _ops().gemm_nt_tile(M, K, N) == tile


def test_row_splits_of_the_grouped_weight_gradients_divide_over_the_xcds():
    ops = _ops()
    for M in (64, 500, 1024, 1470, 4096, 4900, 5880, 9000, 16384, 19600, 65536, 74480, 262144, 275576):
        s = ops.grouped_wgrad_splits(M)
        assert s in (1, 2, 4) or s % 8 == 0, (M, s)
        assert 1 <= s <= max(1, M // 64)
        if M >= 4096:
            assert 1024 <= M / s <= 3072, (M, s)                                # about 2,048 rows per workgroup
    assert ops.grouped_wgrad_splits(19600) == 8 and ops.grouped_wgrad_splits(5880) == 4 and ops.grouped_wgrad_splits(4096) == 2


def _linear_products():
    """(M, K, N) of every product the Linear layers of PanoSwin-T / -S run on the tiled GEMM, stages 0-3 (qkv, proj, fc1, fc2 and the
    PatchMerging reduction into the stage; both have C = 96 and the same layer shapes, only the depths differ), forward and data gradient,
    over batches 1-32 at four resolutions; rows = tokens, or whole windows in pano and planar mode"""
    from panoswintransformerobjectdetection_amd import _lib
    shapes = set()
    for h, w in ((256, 512), (384, 768), (512, 1024), (1024, 2048)):
        for s in range(4):
            C, hs, ws = 96 << s, h // 4 >> s, w // 4 >> s
            layers = [(C, 3 * C), (C, C), (C, 4 * C), (4 * C, C)] + ([(2 * C, C)] if s else [])
            per_image = {hs * ws} | {_lib.window_grid(mode, hs, ws)[2] * 49 for mode in (_lib.MODE_PANO, _lib.MODE_PLANAR)}
            for B in range(1, 33):
                for M in per_image:
                    for K, N in layers:
                        shapes |= {(B * M, K, N), (B * M, N, K)}
    return sorted(shapes)


def test_every_tile_the_rule_hands_an_entry_point_is_one_it_accepts():
    """gemm_nt_tile(..., entry) returns 0 (library; never with required=True) or a row tile of GEMM_NT_TILES[entry], for every entry of
    the tiled GEMM: a 96-row tile reaches the plain epilogue only (the f32 and GELU forms raise PSWIN_ERR_ARG on it)"""
    ops = _ops()
    lib = ops._lib.load()
    assert ops.GEMM_NT_TILES == {"pswin_gemm_nt": (64, 96, 128), "pswin_gemm_nt_f32": (64, 128),
                                 "pswin_gemm_nt_gelu_fwd": (64, 128), "pswin_gemm_nt_gelu_bwd": (64, 128)}
    shapes = _linear_products()
    assert {(40960, 384, 192), (9216, 192, 768), (9216, 768, 192)} <= set(shapes)
    for entry, tiles in ops.GEMM_NT_TILES.items():
        for required in (False, True):
            for M, K, N in shapes:
                t = ops.gemm_nt_tile(M, K, N, entry, required)
                assert t in tiles or (t == 0 and not required), (entry, required, M, K, N, t)
                if entry == "pswin_gemm_nt_gelu_bwd" and t:
                    assert lib.pswin_gemm_nt_partial_rows(M, t) > 0, (M, K, N, t)


@pytest.mark.parametrize("M,K,N,entry", [
    (40960, 384, 192, "pswin_gemm_nt_f32"),        # PatchMerging 0 -> 1 at batch 5, 512 x 1024 (out_f32)
    (9216, 192, 768, "pswin_gemm_nt_gelu_fwd"),    # stage-1 fc1 at batch 2, 384 x 768
    (9216, 192, 768, "pswin_gemm_nt_gelu_bwd"),    # its fc2 data gradient + GELU backward
])
def test_entries_without_96_row_tiles_get_the_64_row_form(M, K, N, entry):
    ops = _ops()
    assert ops.gemm_nt_tile(M, K, N) == 96                                  # the plain epilogue: 96-row tiles fit one round
    assert ops.gemm_nt_tile(M, K, N, entry) == ops.gemm_nt_rows(M, N) == 64
    assert ops.gemm_nt_tile(M, K, N, entry, required=True) == 64
    assert ops._lib.load().pswin_gemm_nt_partial_rows(M, 64) > 0
