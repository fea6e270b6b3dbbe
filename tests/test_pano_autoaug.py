"""The streetwin AutoAugment on the host (pano_aug.draw_auto_augment, crop_boxes, the plan validation, the C entry's argument checks)
against the reference's recorded results in tests/golden/pano_autoaug.npz (tools/gen_pano_autoaug_golden.py), and the numpy
restatement of the two-stage pixel contract (tests/_pano_crop_ref.py) that the GPU tests use as their checker.  No GPU needed."""
import ctypes
import os
import sys

import numpy as np
import pytest

import _pano_crop_ref as C
import _pano_ref as R
from _util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _P():
    from panoswintransformerobjectdetection_amd import pano_aug as P
    return P


def fixture_cases():
    d = np.load(os.path.join(GOLDEN, "pano_autoaug.npz"))
    ends = np.cumsum(d["case_n_boxes"])
    out = []
    for k in range(int(d["n_cases"])):
        s = int(d["case_src"][k])
        rows = slice(int(ends[k] - d["case_n_boxes"][k]), int(ends[k]))
        out.append(dict(k=k, hw=tuple(int(v) for v in d["src_hw"][s]), boxes_in=d[f"boxes{s}"], labels_in=d[f"labels{s}"],
                        seed=int(d["case_seed"][k]), policy=int(d["case_policy"][k]), draws=[int(v) for v in d["case_draws"][k] if v >= 0],
                        plan=tuple(int(v) for v in d["case_plan"][k]), img_shape=tuple(int(v) for v in d["case_img_shape"][k]),
                        boxes=d["out_boxes"][rows], labels=d["out_labels"][rows], ratio_v=[float(v) for v in d["case_ratio_v"][k]],
                        has_ratio_v=bool(d["case_has_ratio_v"][k]), lr_noadj=int(d["case_lr_noadj"][k]),
                        next_rand=float(d["case_next_rand"][k])))
    cfg = dict(first_scales=[tuple(int(v) for v in s) for s in d["first_scales"]], crop_size=tuple(int(v) for v in d["crop_size"]),
               crop_type="absolute_range")
    return out, cfg, [tuple(int(v) for v in s) for s in d["train_scales"]]


CASES, CFG, SCALES = fixture_cases()


def test_the_module_constant_is_the_recipe_the_fixture_was_drawn_with():
    P = _P()
    assert P.STREETWIN_AUTO_AUGMENT == CFG and [tuple(s) for s in P.TRAIN_RESIZE_SCALES] == SCALES


def test_fixture_covers_the_contract():
    assert 38 <= len(CASES) <= 60
    assert {c["policy"] for c in CASES} == {0, 1}
    assert {c["hw"] for c in CASES} >= {(512, 1024), (64, 128), (49, 98)}
    crops = [c["plan"] for c in CASES if c["policy"]]
    assert any(p[2] == 0 for p in crops) and any(p[3] == 0 for p in crops)                       # top, left
    assert any(p[2] + p[4] == p[0] for p in crops) and any(p[3] + p[5] == p[1] for p in crops)   # bottom, right
    pano = [c["plan"] for c in CASES if c["policy"] and c["hw"][1] == 2 * c["hw"][0]]
    assert any(p[3] == 0 for p in pano) and any(p[3] + p[5] == p[1] for p in pano)               # also on a 2:1 panorama
    assert any(c["policy"] and len(c["boxes"]) == 0 for c in CASES)                              # every box dropped
    assert any(0 < len(c["boxes"]) < len(c["boxes_in"]) for c in CASES)                          # some dropped
    assert any(c["lr_noadj"] == 1 for c in CASES) and any(c["lr_noadj"] == 0 for c in CASES)
    assert all((c["lr_noadj"] == -1) == (c["policy"] == 0) == (not c["has_ratio_v"]) for c in CASES)


def _check_case(P, c, rng):
    H, W = c["hw"]
    aa = P.draw_auto_augment(H, W, CFG, rng, SCALES)
    assert aa["policy"] == c["policy"] and aa["draws"] == c["draws"], (c["k"], aa["draws"], c["draws"])
    assert tuple(aa["plan"]) == c["plan"], (c["k"], aa["plan"], c["plan"])
    assert aa["plan"][6:] + (3,) == c["img_shape"]
    b, l = P.auto_augment_boxes(c["boxes_in"], c["labels_in"], H, W, aa)
    assert b.dtype == np.float32 and l.dtype == np.int64
    assert np.array_equal(b, c["boxes"]), (c["k"], b, c["boxes"])
    assert np.array_equal(l, c["labels"]), (c["k"], l, c["labels"])
    assert aa["pano_ratio_v"] == c["ratio_v"] and all(type(v) is float for v in aa["pano_ratio_v"])
    assert {None: -1, False: 0, True: 1}[aa["pano_lr_noadj"]] == c["lr_noadj"]
    if c["policy"]:
        y1, x1, y2, x2 = aa["crop"]
        assert (y1, x1, y2 - y1, x2 - x1) == c["plan"][2:6]
    else:
        assert aa["crop"] is None
    assert rng.rand() == c["next_rand"], c["k"]                                  # the stream stands where the reference's does


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"case{c['k']}")
def test_seeded_draws_and_the_box_chain_reproduce_the_reference(case):
    _check_case(_P(), case, np.random.RandomState(case["seed"]))


def test_crop_boxes_hand_computed():
    P = _P()
    boxes = np.array([[20, 30, 40, 50], [5, 25, 30, 90], [100, 10, 120, 20]], np.float32)      # inside, straddling, outside
    b, l = P.crop_boxes(boxes, np.array([7, 8, 9]), offset_w=10, offset_h=20, crop_h=60, crop_w=50)
    assert b.dtype == np.float32 and l.dtype == np.int64
    assert np.array_equal(b, np.array([[10, 10, 30, 30], [0, 5, 20, 60]], np.float32)) and list(l) == [7, 8]
    b, l = P.crop_boxes(boxes[2:], np.array([9]), 10, 20, 60, 50)                  # allow_negative_crop: nothing left is valid
    assert b.shape == (0, 4) and l.shape == (0,)
    b, l = P.crop_boxes(np.zeros((0, 4), np.float32), np.zeros(0, np.int64), 1, 2, 3, 4)
    assert b.shape == (0, 4) and l.shape == (0,)
    touching = np.array([[0, 20, 10, 40]], np.float32)                             # ends on the crop's left edge: x2 == x1 == 0
    assert len(P.crop_boxes(touching, np.array([1]), 10, 20, 60, 50)[0]) == 0


def test_one_scale_draws_nothing_and_a_narrow_image_is_cropped_whole():
    P = _P()
    rng, twin = np.random.RandomState(5), np.random.RandomState(5)
    cfg = dict(first_scales=[(40, 1333)], crop_size=(30, 50), crop_type="absolute_range")
    for _ in range(20):
        aa = P.draw_auto_augment(96, 64, cfg, rng, [(64, 1333)])
        want = [int(twin.randint(0, 2))]
        if want[0]:
            ch, cw = int(twin.randint(30, 51)), int(twin.randint(30, 51))          # h1 x w1 = 60 x 40: both from the height's range
            want += [ch, cw, int(twin.randint(0, 60 - ch + 1)), int(twin.randint(0, max(40 - cw, 0) + 1))]
            assert aa["plan"][:2] == (60, 40) and aa["cw"] == min(cw, 40 - aa["offset_w"]) and aa["ch"] == ch
            assert aa["pano_lr_noadj"] == (aa["cw"] == 40)
        assert aa["draws"] == want
    with pytest.raises(P.PswinError):
        P.draw_auto_augment(96, 64, dict(cfg, crop_type="relative"), rng)


def _reference_or_skip(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    import gen_pano_autoaug_golden as G
    path, modules = list(sys.path), dict(sys.modules)
    ref = G.load_reference()
    if ref is None:
        pytest.skip("the reference tree (PSWIN_REFERENCE_ROOT) is not on this machine")
    assert sys.path == path and dict(sys.modules) == modules                  # the interpreter is as it was: no stand-in left behind
    return G, ref


def test_fresh_seeds_against_the_live_reference(monkeypatch):
    G, ref = _reference_or_skip(monkeypatch)
    P = _P()
    rng = np.random.RandomState(4321)
    n_crop = 0
    for trial in range(24):
        H, W = [(512, 1024), (64, 128), (49, 98), (96, 64)][trial % 4]
        n = rng.randint(1, 7)
        x1, y1 = rng.randint(0, W - 4, n), rng.randint(0, H - 4, n)
        boxes = np.stack([x1, y1, np.minimum(x1 + rng.randint(2, W, n), W), np.minimum(y1 + rng.randint(2, H, n), H)], 1).astype(np.float32)
        labels = rng.randint(0, 5, n).astype(np.int64)
        seed = 9000 + trial
        r = G.run_seeded(ref, H, W, boxes, labels, seed)
        c = dict(k=trial, hw=(H, W), boxes_in=boxes, labels_in=labels, **r)
        _check_case(P, c, np.random.RandomState(seed))
        n_crop += r["policy"]
    assert 0 < n_crop < 24


def test_the_default_transform_consumes_the_stream_as_before():
    """PanoTrainTransform() without the keyword: draw() is the pano parameters and one randint per image, nothing else."""
    P = _P()
    t = P.PanoTrainTransform(rng=np.random.RandomState(11))
    assert t.auto_augment is None
    params, scales = t.draw(5, 1024)
    rng = np.random.RandomState(11)
    for i in range(5):
        p = P.draw_pano_params(1, 1024, rng=rng)
        assert all(p[k][0] == params[k][i] for k in p)
        assert scales[i] == P.TRAIN_RESIZE_SCALES[rng.randint(len(P.TRAIN_RESIZE_SCALES))]
    assert t.rng.rand() == rng.rand()


def test_the_auto_augment_transform_draws_pano_parameters_then_the_policy_per_image():
    P = _P()
    t = P.PanoTrainTransform(auto_augment=P.STREETWIN_AUTO_AUGMENT, rng=np.random.RandomState(3))
    params, aas = t.draw_auto(4, 64, 128)
    rng = np.random.RandomState(3)
    for i in range(4):
        p = P.draw_pano_params(1, 128, rng=rng)
        assert all(p[k][0] == params[k][i] for k in p)
        assert aas[i] == P.draw_auto_augment(64, 128, P.STREETWIN_AUTO_AUGMENT, rng)
    assert t.rng.rand() == rng.rand()


def test_argument_errors_without_a_gpu():
    import torch
    from panoswintransformerobjectdetection_amd import PswinError, _lib
    P = _P()
    imgs = torch.zeros(2, 8, 16, 3, dtype=torch.uint8)
    with pytest.raises(PswinError):
        P.resize_crop_resize_normalize_pad(imgs, [(0, 0, 0, 0, 0, 0, 8, 16)] * 2)                # CPU tensor
    with pytest.raises(PswinError):
        P.PanoTrainTransform(auto_augment=P.STREETWIN_AUTO_AUGMENT)(imgs, [np.zeros((0, 4), np.float32)] * 2, [np.zeros(0, np.int64)] * 2)
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    a = ctypes.cast(buf, ctypes.c_void_p).value
    ok = (a, a + 1024, a + 1536, 1, a + 2048, 2, 8, 16, 32, 32, None)
    for i, v in ((0, None), (1, None), (2, None), (4, None), (5, 0), (5, 65536), (6, 0), (7, -1), (8, 0), (9, -4), (8, 4 * 65535 + 1)):
        bad = list(ok)
        bad[i] = v
        assert lib.pswin_pano_resize_crop_resize_normalize_pad(*bad) == -1, (i, v)


def test_host_plan_validation():
    P = _P()
    ok = dict(h1=40, w1=80, cy=4, cx=10, ch=30, cw=60, oh=32, ow=64)
    assert P._host_plan([ok, (0, 0, 0, 0, 0, 0, 16, 32)], 2, "t") == [(40, 80, 4, 10, 30, 60, 32, 64), (0, 0, 0, 0, 0, 0, 16, 32)]
    for bad in (dict(ok, ch=37), dict(ok, cx=21), dict(ok, cy=-1), dict(ok, cw=0), dict(ok, oh=0), dict(ok, w1=0), dict(ok, h1=-3),
                (40, 80, 4, 10, 30, 60, 32), {k: v for k, v in ok.items() if k != "ow"}, dict(ok, oh="x")):
        with pytest.raises(P.PswinError):
            P._host_plan([bad], 1, "t")
    with pytest.raises(P.PswinError):
        P._host_plan([ok], 2, "t")                                                  # one row for two images


def test_host_plan_errors_reach_the_caller_of_the_kernel_wrapper(monkeypatch):
    """A crop outside h1 x w1 and an output larger than pad_hw raise before any launch (the image check is stubbed: no GPU here)."""
    import torch
    P = _P()
    monkeypatch.setattr(P, "_check_images", lambda *a, **k: None)
    imgs = torch.zeros(1, 8, 16, 3, dtype=torch.uint8)
    with pytest.raises(P.PswinError, match="leaves the intermediate image"):
        P.resize_crop_resize_normalize_pad(imgs, [(40, 80, 20, 10, 30, 60, 32, 64)])
    with pytest.raises(P.PswinError, match="exceeds the padded size"):
        P.resize_crop_resize_normalize_pad(imgs, [(40, 80, 4, 10, 30, 60, 32, 64)], pad_hw=(32, 32))
    with pytest.raises(P.PswinError, match="pad_hw"):
        P.resize_crop_resize_normalize_pad(imgs, torch.zeros(1, 8, dtype=torch.int32))


def test_restated_contract_clamps_inside_the_crop_not_the_image():
    rng = np.random.RandomState(1)
    img = rng.randint(0, 256, (8, 16, 3)).astype(np.uint8)
    assert np.array_equal(C.resize_crop_resize_u8(img, (0, 0, 0, 0, 0, 0, 4, 8)), R.resize_u8_f32(img, 4, 8))
    # scale 1 then a crop then scale 2: the last output column replicates the crop's last column, not its neighbour in the image
    got = C.resize_crop_resize_u8(img, (8, 16, 2, 3, 4, 5, 8, 10))
    crop = img[2:6, 3:8]
    assert np.array_equal(got, R.resize_u8_f32(crop, 8, 10))
    assert np.array_equal(got[0, -1], crop[0, -1].astype(np.float32)) and np.array_equal(got[-1, 0], crop[-1, 0].astype(np.float32))
    out = C.normalize_pad(got, (1.0, 2.0, 3.0), (0.5, 0.25, 2.0), True, 9, 12)
    assert out.shape == (3, 9, 12) and np.all(out[:, 8:] == 0) and np.all(out[:, :, 10:] == 0)
    assert out[0, 0, 0] == (got[0, 0, 2] - 1.0) * 0.5 and out[2, 3, 4] == (got[3, 4, 0] - 3.0) * 2.0
