"""PanoStretch / RollAug / RandomFlip / Resize host side (panoswintransformerobjectdetection_amd/pano_aug.py) against the reference's
outputs in tests/golden/pano_aug.npz (tools/gen_pano_aug_golden.py), and the numpy restatement of the image warp (tests/_pano_ref.py)
that the GPU tests use as their checker.  No GPU needed."""
import ctypes
import os
import sys

import numpy as np
import pytest

import _pano_ref as R
from _util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture():
    d = np.load(os.path.join(GOLDEN, "pano_aug.npz"))
    return {k: d[k] for k in d.files}


def fixture_cases():
    """List of dicts: src, boxes_in, labels_in, params (one image, pano_aug layout), clip01, img, boxes, labels, seed, pos, chances."""
    d = _fixture()
    out = []
    for k in range(int(d["n_cases"])):
        s = int(d["case_src"][k])
        p = {key: d["case_" + key][k:k + 1] for key in ("stretch", "kx", "ky", "roll", "roll_dist", "shift", "flip")}
        out.append(dict(k=k, src_id=s, src=d[f"src{s}"], boxes_in=d[f"boxes{s}"], labels_in=d[f"labels{s}"], params=p,
                        clip01=bool(d["case_clip01"][k]), img=(np.cumsum(d[f"img_dx{k}"], axis=1, dtype=np.int64) % 256).astype(np.uint8),
                        boxes=d[f"out_boxes{k}"], labels=d[f"out_labels{k}"], seed=int(d["case_seed"][k]), pos=int(d["case_pos"][k]),
                        chances=d["case_chances"][k], kxy=tuple(d["kxy"])))
    return out


CASES = fixture_cases()


def test_fixture_covers_the_contract():
    combos = {(bool(c["params"]["stretch"][0]), bool(c["params"]["roll"][0]), bool(c["params"]["flip"][0])) for c in CASES}
    assert len(combos) == 8
    assert {c["src"].shape for c in CASES} == {(64, 128, 3), (49, 98, 3)}
    shifts = {(int(c["params"]["shift"][0]), c["src"].shape[1]) for c in CASES if c["params"]["roll"][0]}
    assert any(s == 0 for s, _ in shifts) and any(s == w - 1 for s, w in shifts)
    ks = {(float(c["params"]["kx"][0]), float(c["params"]["ky"][0])) for c in CASES if c["params"]["stretch"][0]}
    assert (2.0, 0.5) in ks and (0.5, 2.0) in ks
    merged = [c for c in CASES if len(c["labels"]) != len(c["labels_in"]) or not np.array_equal(np.sort(c["labels"]), np.sort(c["labels_in"]))]
    assert len(merged) >= 4                        # the seam merge (a cross product) ran


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"case{c['k']}")
def test_restatement_reproduces_reference_images(case):
    p = case["params"]
    got = R.warp(case["src"], p["stretch"][0], p["kx"][0], p["ky"][0], int(p["shift"][0]), p["flip"][0])
    assert got.dtype == np.uint8 and np.array_equal(got, case["img"])


def test_transform_boxes_reproduces_reference_boxes_and_labels():
    from panoswintransformerobjectdetection_amd import pano_aug as P
    for c in CASES:
        H, W = c["src"].shape[:2]
        b, l = P.transform_boxes([c["boxes_in"]], [c["labels_in"]], H, W, c["params"], clip01=c["clip01"])
        assert b[0].dtype == np.float32 and l[0].dtype == np.int64
        assert np.array_equal(b[0], c["boxes"]), (c["k"], b[0], c["boxes"])
        assert np.array_equal(l[0], c["labels"]), (c["k"], l[0], c["labels"])


def test_stretch_moves_a_corner_at_x_eq_W_across_the_seam():
    from panoswintransformerobjectdetection_amd import pano_aug as P
    pts = P._stretch_corners(np.array([[100.0, 20.0], [128.0, 40.0]]), 64, 128, 1.7, 0.6)
    assert round(float(pts[1, 0]), 2) == -0.32
    b, _ = P.transform_one(np.array([[100, 20, 128, 40]], np.float32), np.array([3]), 64, 128, True, 1.7, 0.6, False, 0.0, False)
    assert b[0, 2] == 0.0 and b[0, 0] > 64                       # np.round(-0.32) = -0.0


def test_seeded_draws_reproduce_the_reference_parameters():
    from panoswintransformerobjectdetection_amd import pano_aug as P
    groups = {}
    for c in CASES:
        if c["seed"] >= 0:
            groups.setdefault((c["src_id"], c["seed"]), []).append(c)
    assert len(groups) >= 17
    for (_, seed), cs in groups.items():
        cs = sorted(cs, key=lambda c: c["pos"])
        ch = cs[0]["chances"]
        got = P.draw_pano_params(len(cs), cs[0]["src"].shape[1], cs[0]["kxy"], ch[0], ch[1], ch[2], rng=np.random.RandomState(seed))
        for i, c in enumerate(cs):
            for key, want in c["params"].items():
                assert got[key][i] == want[0], (seed, i, key, got[key][i], want[0])


def test_make_pano_params_matches_the_drawn_layout():
    from panoswintransformerobjectdetection_amd import pano_aug as P
    p = P.make_pano_params([True, False], [2.0, 3.0], [0.5, 3.0], [0.9999999, None], [False, True], 128)
    assert list(p["shift"]) == [127, 0] and list(p["roll"]) == [True, False] and p["roll_dist"][0] == 0.99999
    assert list(p["kx"]) == [2.0, 1.0] and list(p["ky"]) == [0.5, 1.0]
    a = P.params_array(p)
    assert a.dtype == np.float64 and a.shape == (2, 4) and list(a[:, 3]) == [P.STRETCH, P.FLIP]


def test_rescale_size_and_resize_boxes_hand_computed():
    from panoswintransformerobjectdetection_amd import pano_aug as P
    assert P.rescale_size(512, 1024, (800, 1333)) == (667, 1333)        # sf = 1333/1024; 512 * sf = 666.5 -> int(667.0)
    assert P.rescale_size(512, 1024, (480, 1333)) == (480, 960)         # sf = 480/512
    assert P.rescale_size(1024, 2048, (800, 1333)) == (667, 1333)
    assert P.rescale_size(1024, 2048, (1333, 480)) == (480, 960)        # either order of the tuple: sf = 480/1024
    b = P.resize_boxes(np.array([[10, 20, 1024, 512], [-5, 10, 1100, 600]], np.float32), 512, 1024, 480, 960)
    assert b.dtype == np.float32
    assert np.array_equal(b, np.array([[9.375, 18.75, 960, 480], [0, 9.375, 960, 480]], np.float32))
    sizes = [P.rescale_size(512, 1024, s) for s in [(480, 1333), (800, 1333)]]
    assert P.padded_size(sizes, 32) == (672, 1344)


def test_transform_draws_pano_parameters_then_the_scale_per_image():
    from panoswintransformerobjectdetection_amd import pano_aug as P
    t = P.PanoTrainTransform(rng=np.random.RandomState(3))
    params, scales = t.draw(3, 1024)
    rng = np.random.RandomState(3)
    for i in range(3):
        p = P.draw_pano_params(1, 1024, rng=rng)
        assert all(p[k][0] == params[k][i] for k in p)
        assert scales[i] == P.TRAIN_RESIZE_SCALES[rng.randint(len(P.TRAIN_RESIZE_SCALES))]


def test_argument_errors_without_a_gpu():
    import torch
    from panoswintransformerobjectdetection_amd import PswinError, _lib
    from panoswintransformerobjectdetection_amd import pano_aug as P
    imgs = torch.zeros(2, 8, 16, 3, dtype=torch.uint8)
    with pytest.raises(PswinError):
        P.pano_warp(imgs, P.make_pano_params([False] * 2, [1.0] * 2, [1.0] * 2, None, [False] * 2, 16))
    with pytest.raises(PswinError):
        P.resize_normalize_pad(imgs, [(8, 16)] * 2)
    with pytest.raises(PswinError):
        P.PanoTrainTransform()(imgs, [np.zeros((0, 4), np.float32)] * 2, [np.zeros(0, np.int64)] * 2)
    with pytest.raises(PswinError):
        P.transform_boxes([np.zeros((2, 4), np.float32)], [np.zeros(1, np.int64)], 8, 16,
                          P.make_pano_params([False], [1.0], [1.0], None, [False], 16))
    # the C entry points reject bad shapes before they touch a device
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    a = ctypes.cast(buf, ctypes.c_void_p).value
    b = a + 2048
    ok = (a, a + 1024, b, 2, 8, 16, 3, None)
    for i, v in ((5, 15), (6, 5), (6, 0), (4, 1), (2, a), (1, None), (3, 0)):
        bad = list(ok)
        bad[i] = v
        assert lib.pswin_pano_warp_u8(*bad) == -1, (i, v)
    ok = (a, a + 1024, a + 1536, 1, b, 2, 8, 16, 32, 32, None)
    for i, v in ((8, 0), (9, -4), (5, 0), (2, None), (4, None)):
        bad = list(ok)
        bad[i] = v
        assert lib.pswin_pano_resize_normalize_pad(*bad) == -1, (i, v)


def test_restated_resize_is_exact_at_scale_1_and_follows_the_float_statement():
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (6, 10, 3)).astype(np.uint8)
    assert np.array_equal(R.resize_u8_f32(img, 6, 10), img.astype(np.float32))
    up = R.resize_u8_f32(img, 12, 20)
    # scale 2: output (0, 0) sits at source (-0.25 -> 0, -0.25 -> 0); output (1, 1) at (0.25, 0.25)
    assert up[0, 0, 0] == img[0, 0, 0]
    want = 0.75 * (0.75 * float(img[0, 0, 0]) + 0.25 * float(img[0, 1, 0])) + 0.25 * (0.75 * float(img[1, 0, 0]) + 0.25 * float(img[1, 1, 0]))
    assert up[1, 1, 0] == np.floor(want + 0.5)


def _reference_or_skip(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    import gen_pano_aug_golden as G
    path, modules = list(sys.path), set(sys.modules)
    ref = G.load_reference()
    if ref is None:
        pytest.skip("the reference tree (PSWIN_REFERENCE_ROOT) or scipy is not on this machine")
    assert sys.path == path and not any(m == "lzx" or m.startswith("lzx.") for m in set(sys.modules) - modules)
    return G, ref


def test_random_cases_against_the_live_reference(monkeypatch):
    """Random images, boxes and seeds through the reference's own functions and through pano_aug + the restatement."""
    G, ref = _reference_or_skip(monkeypatch)
    from panoswintransformerobjectdetection_amd import pano_aug as P
    rng = np.random.RandomState(1234)
    for trial in range(6):
        H, W = [(32, 64), (25, 50), (40, 80)][trial % 3]
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        n = rng.randint(1, 6)
        x1 = rng.randint(0, W - 4, n)
        y1 = rng.randint(0, H - 4, n)
        boxes = np.stack([x1, y1, np.minimum(x1 + rng.randint(2, W // 2, n), W), np.minimum(y1 + rng.randint(2, H // 2, n), H)], 1)
        boxes[0, 0], boxes[-1, 2] = 0, W                   # something on the seam
        boxes = boxes.astype(np.float32)
        labels = rng.randint(0, 5, n).astype(np.int64)
        seed, chances = 500 + trial, (0.7, 0.7, 0.5)
        outs, drawn = G.run_seeded(ref, img, boxes, labels, seed, 3, chances)
        p = P.draw_pano_params(3, W, G.KXY, *chances, rng=np.random.RandomState(seed))
        for i, ((im, b, l), dp) in enumerate(zip(outs, drawn)):
            assert all(p[k][i] == dp[k] for k in dp), (trial, i)
            got = R.warp(img, p["stretch"][i], p["kx"][i], p["ky"][i], int(p["shift"][i]), p["flip"][i])
            assert np.array_equal(got, im), (trial, i)
            pi = {k: v[i:i + 1] for k, v in p.items()}
            gb, gl = P.transform_boxes([boxes], [labels], H, W, pi)
            assert np.array_equal(gb[0], b) and np.array_equal(gl[0], l), (trial, i)
