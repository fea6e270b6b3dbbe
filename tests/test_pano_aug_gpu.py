"""The pano augmentation kernels (csrc/pswin_pano.hip) on the MI355X: the warp against the reference's images
(tests/golden/pano_aug.npz) and against the numpy restatement at training sizes; the resize against a torch statement; both kernels
in one captured graph; PanoTrainTransform feeding the bf16 backbone."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _pano_ref as R
from test_pano_aug import CASES

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _P():
    from panoswintransformerobjectdetection_amd import pano_aug as P
    return P


def _stack_params(ps):
    return {k: np.concatenate([p[k] for p in ps]) for k in ps[0]}


@pytest.mark.parametrize("src_id", [0, 1])
def test_warp_reproduces_the_reference_images_exactly(src_id):
    P = _P()
    cs = [c for c in CASES if c["src_id"] == src_id]
    src = np.stack([c["src"] for c in cs])
    out = P.pano_warp(torch.from_numpy(src).to(DEV), _stack_params([c["params"] for c in cs])).cpu().numpy()
    for i, c in enumerate(cs):
        bad = int((out[i] != c["img"]).sum())
        assert bad == 0, (c["k"], bad)


def _smooth_batch(B, H, W, seed):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = 128 + 60 * np.sin(2 * np.pi * x / W * 3) * np.cos(np.pi * y / H * 2)
    imgs = base[None, :, :, None] + rng.normal(0, 25, (B, H, W, 3)).astype(np.float32)
    return np.clip(np.round(imgs), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("B,H,W", [(8, 512, 1024), (8, 1024, 2048), (3, 257, 514)])
def test_warp_matches_the_restatement_at_training_sizes(B, H, W, record_property):
    P = _P()
    imgs = _smooth_batch(B, H, W, H)
    params = P.draw_pano_params(B, W, rng=np.random.RandomState(W + B))
    params["stretch"][0] = True
    out = P.pano_warp(torch.from_numpy(imgs).to(DEV), params).cpu().numpy()
    n_diff, worst = 0, 0
    for i in range(B):
        want = R.warp(imgs[i], params["stretch"][i], params["kx"][i], params["ky"][i], int(params["shift"][i]), params["flip"][i])
        d = np.abs(out[i].astype(np.int16) - want.astype(np.int16))
        n_diff += int((d != 0).sum())
        worst = max(worst, int(d.max()))
    px = B * H * W
    record_property("pixels_differing", n_diff)
    print(f"\nwarp {B}x{H}x{W}: {n_diff} of {px} pixel channels differ from the float64 restatement, worst {worst} LSB")
    assert worst <= 1 and n_diff <= max(1, px // 1_000_000), (n_diff, worst)


def test_warp_without_stretch_is_exactly_roll_and_flip():
    P = _P()
    B, H, W = 6, 33, 130
    imgs = np.random.RandomState(5).randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    params = P.make_pano_params([False] * B, [1.0] * B, [1.0] * B, [0.0, 0.5, 0.99999, 0.123456, None, 0.7], [False, True] * 3, W)
    out = P.pano_warp(torch.from_numpy(imgs).to(DEV), params).cpu().numpy()
    for i in range(B):
        want = np.roll(imgs[i], int(params["shift"][i]), axis=1)
        if params["flip"][i]:
            want = want[:, ::-1]
        assert np.array_equal(out[i], want), i
    one = P.pano_warp(torch.from_numpy(imgs[..., :1].copy()).to(DEV), params).cpu().numpy()       # C = 1
    assert np.array_equal(one[..., 0], out[..., 0])


def _torch_statement(imgs, sizes, mean, std, to_rgb, Hp, Wp):
    """F.interpolate(bilinear, align_corners=False, antialias=False) -> floor(x + 0.5) -> normalise -> pad: (u8 stage, output)."""
    P = _P()
    norm = P.norm_tensor(mean, std, DEV)
    x = imgs.permute(0, 3, 1, 2).float()
    if to_rgb:
        x = x.flip(1)
    u8 = torch.zeros(len(sizes), 3, Hp, Wp, device=DEV)
    out = torch.zeros(len(sizes), 3, Hp, Wp, device=DEV)
    for i, (h, w) in enumerate(sizes):
        r = F.interpolate(x[i:i + 1], size=(h, w), mode="bilinear", align_corners=False, antialias=False)
        r = torch.floor(r + 0.5).clamp(0, 255)
        u8[i, :, :h, :w] = r[0]
        out[i, :, :h, :w] = (r[0] - norm[:3, None, None]) * norm[3:, None, None]
    return u8, out, norm


@pytest.mark.parametrize("H,W,sizes,exact", [
    (64, 128, [(64, 128), (128, 256), (32, 64)], True),             # scale factors 1, 2, 1/2
    (512, 1024, [(667, 1333), (480, 960), (600, 1200)], False),
    (1024, 2048, [(667, 1333), (800, 1600)], False),
    (49, 98, [(37, 75), (49, 98)], False),
])
def test_resize_normalize_pad_against_torch(H, W, sizes, exact):
    P = _P()
    B = len(sizes)
    imgs = torch.from_numpy(_smooth_batch(B, H, W, 7)).to(DEV)
    Hp, Wp = P.padded_size(sizes, 32)
    got = P.resize_normalize_pad(imgs, sizes, P.IMG_NORM_MEAN, P.IMG_NORM_STD, True, 32)
    assert tuple(got.shape) == (B, 3, Hp, Wp)
    u8, want, norm = _torch_statement(imgs, sizes, P.IMG_NORM_MEAN, P.IMG_NORM_STD, True, Hp, Wp)
    inside = torch.zeros(B, 1, Hp, Wp, dtype=torch.bool, device=DEV)
    for i, (h, w) in enumerate(sizes):
        inside[i, :, :h, :w] = True
    inside = inside.expand(B, 3, Hp, Wp)
    assert torch.all(got[~inside] == 0)                                            # the pad is written, exactly 0
    u8_got = torch.round(got / norm[3:, None, None] + norm[:3, None, None])
    du = (u8_got - u8)[inside].abs()
    assert du.max().item() <= (0 if exact else 1), du.max().item()
    same = inside & (u8_got == u8)
    ulp = (want[same].view(torch.int32).long() - got[same].view(torch.int32).long()).abs()    # never 0: the means are not integers
    assert ulp.max().item() <= 1
    print(f"\nresize {H}x{W} -> {sizes}: {int((du != 0).sum())} of {int(inside.sum())} values 1 LSB off the torch statement")


def test_both_kernels_in_one_captured_graph_replay_new_parameters():
    P = _P()
    B, H, W = 4, 128, 256
    sizes = [(96, 192), (128, 256), (64, 128), (112, 224)]
    Hp, Wp = P.padded_size(sizes, 32)
    imgs = torch.from_numpy(_smooth_batch(B, H, W, 3)).to(DEV)
    prm = P.params_tensor(P.draw_pano_params(B, W, rng=np.random.RandomState(0)), DEV)
    hw = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    norm = P.norm_tensor(P.IMG_NORM_MEAN, P.IMG_NORM_STD, DEV)
    warped = torch.empty_like(imgs)
    x = torch.empty(B, 3, Hp, Wp, device=DEV)

    def step():
        P.pano_warp(imgs, prm, out=warped)
        P.resize_normalize_pad(warped, hw, pad_hw=(Hp, Wp), out=x, norm=norm)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    torch.cuda.synchronize()
    new = P.draw_pano_params(B, W, rng=np.random.RandomState(1))
    new_sizes = [(128, 256), (64, 128), (100, 200), (128, 224)]
    prm.copy_(P.params_tensor(new, DEV))
    hw.copy_(torch.tensor(new_sizes, dtype=torch.int32))
    x.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    eager = P.resize_normalize_pad(P.pano_warp(imgs, new), new_sizes, pad_hw=(Hp, Wp))
    assert torch.equal(x, eager)


def test_pano_train_transform_feeds_the_bf16_backbone():
    from _util import TINY
    from panoswintransformerobjectdetection_amd import SimplePanoSwinTransformer
    P = _P()
    B, H, W = 2, 128, 256
    imgs = torch.from_numpy(_smooth_batch(B, H, W, 9)).to(DEV)
    boxes = [np.array([[0, 20, 40, 60], [200, 10, 256, 90]], np.float32), np.array([[30, 30, 90, 100]], np.float32)]
    labels = [np.array([1, 2], np.int64), np.array([0], np.int64)]
    t = P.PanoTrainTransform(img_scales=[(128, 1333), (96, 1333)], rng=np.random.RandomState(2))
    x, b, l, metas = t(imgs, boxes, labels)
    assert x.dtype == torch.float32 and x.shape[0] == B and x.shape[2] % 32 == 0 and x.shape[3] % 32 == 0
    for i, m in enumerate(metas):
        h, w = m["img_shape"][:2]
        assert b[i].dtype == np.float32 and (b[i][:, 0::2] <= w).all() and (b[i][:, 1::2] <= h).all() and len(l[i]) == len(b[i])
    torch.manual_seed(0)
    model = SimplePanoSwinTransformer(**TINY, compute_dtype=torch.bfloat16).to(DEV).eval()
    model.init_weights(None)
    with torch.no_grad():
        outs = model(x)
    assert len(outs) == 4 and all(torch.isfinite(o.float()).all() for o in outs)


@pytest.mark.parametrize("C", [1, 2, 4])
def test_warp_other_channel_counts_on_the_vector_store_path(C):
    """W % 4 == 0 takes the 32-bit store path; every channel count matches the restatement exactly."""
    P = _P()
    B, H, W = 3, 40, 128
    imgs = _smooth_batch(B, H, W, 30 + C)[..., :3]
    imgs = np.ascontiguousarray(np.concatenate([imgs, imgs[..., :1] // 2 + 60], -1)[..., :C])
    params = P.make_pano_params([True, True, False], [1.6, 0.7, 1.0], [0.55, 1.9, 1.0], [0.3, None, 0.81], [True, False, True], W)
    out = P.pano_warp(torch.from_numpy(imgs).to(DEV), params).cpu().numpy()
    for i in range(B):
        want = R.warp(imgs[i], params["stretch"][i], params["kx"][i], params["ky"][i], int(params["shift"][i]), params["flip"][i])
        assert np.array_equal(out[i], want), (C, i)


def test_resize_without_the_channel_swap():
    P = _P()
    sizes = [(64, 128), (128, 256), (32, 64)]
    imgs = torch.from_numpy(_smooth_batch(3, 64, 128, 21)).to(DEV)
    got = P.resize_normalize_pad(imgs, sizes, P.IMG_NORM_MEAN, P.IMG_NORM_STD, False, 32)
    _, want, _ = _torch_statement(imgs, sizes, P.IMG_NORM_MEAN, P.IMG_NORM_STD, False, *P.padded_size(sizes, 32))
    assert torch.equal(got, want)                   # scale factors 1, 2, 1/2: exact
    swapped = P.resize_normalize_pad(imgs, sizes, P.IMG_NORM_MEAN, P.IMG_NORM_STD, True, 32)
    assert not torch.equal(got, swapped)


def test_caller_buffers_are_checked_before_the_launch():
    P = _P()
    from panoswintransformerobjectdetection_amd import PswinError
    B, H, W = 2, 32, 64
    imgs = torch.from_numpy(_smooth_batch(B, H, W, 4)).to(DEV)
    prm = P.params_tensor(P.draw_pano_params(B, W, rng=np.random.RandomState(4)), DEV)
    bad_out = {
        "cpu": torch.empty(B, H, W, 3, dtype=torch.uint8),
        "shape": torch.empty(B + 1, H, W, 3, dtype=torch.uint8, device=DEV),
        "dtype": torch.empty(B, H, W, 3, dtype=torch.float32, device=DEV),
        "view": torch.empty(B, H, W, 6, dtype=torch.uint8, device=DEV)[..., :3],
        "alias": imgs,
    }
    for name, out in bad_out.items():
        with pytest.raises(PswinError):
            P.pano_warp(imgs, prm, out=out)
    big = torch.zeros(imgs.numel() + W * 3, dtype=torch.uint8, device=DEV)       # out overlaps the input by all but one row
    with pytest.raises(PswinError):
        P.pano_warp(big[:imgs.numel()].view(imgs.shape), prm, out=big[W * 3:].view(imgs.shape))
    sizes = [(32, 64), (16, 32)]
    Hp, Wp = P.padded_size(sizes, 32)
    hw = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    norm = P.norm_tensor(P.IMG_NORM_MEAN, P.IMG_NORM_STD, DEV)
    bad_x = {
        "cpu": torch.empty(B, 3, Hp, Wp),
        "batch": torch.empty(B + 1, 3, Hp, Wp, device=DEV),
        "pad": torch.empty(B, 3, Hp, Wp + 32, device=DEV),
        "dtype": torch.empty(B, 3, Hp, Wp, device=DEV, dtype=torch.bfloat16),
        "view": torch.empty(B, 3, Hp, 2 * Wp, device=DEV)[..., ::2],
        "alias_norm": norm,
    }
    for name, out in bad_x.items():
        with pytest.raises(PswinError):
            P.resize_normalize_pad(imgs, hw, pad_hw=(Hp, Wp), out=out, norm=norm)
    bad_norm = {
        "cpu": norm.cpu(),
        "dtype": norm.double(),
        "size": torch.zeros(3, device=DEV),
        "view": torch.zeros(12, device=DEV)[::2],
    }
    for name, n in bad_norm.items():
        with pytest.raises(PswinError):
            P.resize_normalize_pad(imgs, hw, pad_hw=(Hp, Wp), norm=n)
    ok = torch.empty(B, 3, Hp, Wp, device=DEV)
    assert P.resize_normalize_pad(imgs, hw, pad_hw=(Hp, Wp), out=ok, norm=norm) is ok
    warped = torch.empty_like(imgs)
    assert P.pano_warp(imgs, prm, out=warped) is warped


def test_pano_train_transform_uses_one_draw_for_the_pixels_and_the_boxes():
    """x and the boxes equal the two kernels and the host box path run with the parameters the same seed draws; img_metas records them."""
    P = _P()
    B, H, W = 3, 64, 128
    imgs = torch.from_numpy(_smooth_batch(B, H, W, 12)).to(DEV)
    boxes = [np.array([[0, 10, 30, 40], [100, 5, 128, 50]], np.float32), np.array([[20, 20, 60, 60]], np.float32),
             np.array([[0, 0, 128, 64]], np.float32)]
    labels = [np.array([1, 2], np.int64), np.array([3], np.int64), np.array([0], np.int64)]
    scales = [(64, 1333), (48, 1333), (96, 1333)]
    x, b, l, metas = P.PanoTrainTransform(img_scales=scales, rng=np.random.RandomState(8))(imgs, boxes, labels)
    params, picked = P.PanoTrainTransform(img_scales=scales, rng=np.random.RandomState(8)).draw(B, W)
    sizes = [P.rescale_size(H, W, s) for s in picked]
    want = P.resize_normalize_pad(P.pano_warp(imgs, params), sizes, size_divisor=32)
    assert torch.equal(x, want)
    wb, wl = P.transform_boxes(boxes, labels, H, W, params)
    for i, m in enumerate(metas):
        assert m["img_shape"][:2] == sizes[i] and m["scale"] == picked[i] and m["flip"] == bool(params["flip"][i])
        assert m["roll_shift"] == params["shift"][i] and (m["pano_stretch"] is None) == (not params["stretch"][i])
        assert np.array_equal(b[i], P.resize_boxes(wb[i], H, W, *sizes[i])) and np.array_equal(l[i], wl[i])
    assert any(m["pano_stretch"] for m in metas) and any(m["flip"] for m in metas)
