"""pswin_pano_resize_crop_resize_normalize_pad (csrc/pswin_pano.hip) on the MI355X: against the numpy restatement where the float
arithmetic is exact, bit for bit against the chain of the existing resize kernel (resize, crop in torch, resize) at ragged and at
recipe sizes, the device-side clamping of the plan, a captured graph replayed with another plan, and
PanoTrainTransform(auto_augment=STREETWIN_AUTO_AUGMENT) end to end."""
import numpy as np
import pytest
import torch

import _pano_crop_ref as C
from test_pano_aug_gpu import _smooth_batch

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _P():
    from panoswintransformerobjectdetection_amd import pano_aug as P
    return P


def _chain(P, imgs, plans, pad_hw, to_rgb=True):
    """What a user builds from the existing kernel: resize to h1 x w1 (identity normalisation, no channel swap: the float output holds
    the uint8 values), crop in torch, resize to oh x ow with the real normalisation, the channel swap applied once."""
    out = []
    for i, (h1, w1, cy, cx, ch, cw, oh, ow) in enumerate(plans):
        img = imgs[i:i + 1]
        if h1:
            first = P.resize_normalize_pad(img, [(h1, w1)], mean=(0, 0, 0), std=(1, 1, 1), to_rgb=False, size_divisor=1)
            u8 = torch.round(first).to(torch.uint8).permute(0, 2, 3, 1)
            assert torch.equal(u8.float().permute(0, 3, 1, 2), first)
            img = u8[:, cy:cy + ch, cx:cx + cw].contiguous()
        out.append(P.resize_normalize_pad(img, [(oh, ow)], to_rgb=to_rgb, pad_hw=pad_hw))
    return torch.cat(out)


def test_exact_geometry_equals_the_numpy_restatement_bit_for_bit():
    P = _P()
    plans = [(0, 0, 0, 0, 0, 0, 32, 64), (128, 256, 5, 9, 48, 80, 96, 160), (64, 128, 0, 0, 64, 128, 32, 64)]
    imgs = _smooth_batch(3, 64, 128, 17)
    for to_rgb in (True, False):
        got = P.resize_crop_resize_normalize_pad(torch.from_numpy(imgs).to(DEV), plans, to_rgb=to_rgb)
        assert tuple(got.shape) == (3, 3, 96, 160)
        norm = P.norm_tensor(P.IMG_NORM_MEAN, P.IMG_NORM_STD, "cpu").numpy()
        want = C.batch(imgs, plans, norm, to_rgb, 96, 160)
        assert np.array_equal(got.cpu().numpy(), want)
        for i, p in enumerate(plans):
            assert torch.all(got[i, :, p[6]:] == 0) and torch.all(got[i, :, :, p[7]:] == 0)        # the pad, exactly 0
    # a blend across the crop's border would show: column 79 of the crop replicates, its neighbour in the image differs
    inter = C.R.resize_u8_f32(imgs[1], 128, 256)
    assert not np.array_equal(inter[5:53, 88], inter[5:53, 89])


RAGGED = [(37, 75, 3, 70, 30, 5, 45, 9),            # touches the right edge
          (37, 75, 0, 10, 37, 1, 50, 3),            # one column
          (37, 75, 20, 4, 17, 33, 23, 50),          # ends on the bottom row
          (0, 0, 0, 0, 0, 0, 41, 83)]


def test_ragged_shapes_equal_the_chain_of_existing_kernels():
    P = _P()
    imgs = torch.from_numpy(_smooth_batch(4, 49, 98, 23)).to(DEV)
    pad_hw = P.padded_size([p[6:] for p in RAGGED], 1)
    assert pad_hw == (50, 83)                                                      # odd Wp: the scalar store path
    got = P.resize_crop_resize_normalize_pad(imgs, RAGGED, size_divisor=1)
    assert tuple(got.shape) == (4, 3, 50, 83)
    assert torch.equal(got, _chain(P, imgs, RAGGED, pad_hw))
    assert torch.equal(P.resize_crop_resize_normalize_pad(imgs, RAGGED, size_divisor=1, to_rgb=False), _chain(P, imgs, RAGGED, pad_hw, False))


def test_both_kernel_paths_at_recipe_size_equal_the_chain():
    P = _P()
    plans = [(400, 800, 1, 200, 389, 393) + P.rescale_size(389, 393, (800, 1333)),        # LDS tile, upscale
             (600, 1200, 0, 816, 600, 384) + P.rescale_size(600, 384, (480, 1333)),       # LDS tile, factor 1.25, ends on the last column
             (600, 1200, 0, 300, 600, 600, 75, 75)]                                        # shrinks by 8: every thread on its own
    assert plans[0][6:] == (800, 808) and plans[1][6:] == (750, 480)
    imgs = torch.from_numpy(_smooth_batch(3, 512, 1024, 31)).to(DEV)
    pad_hw = P.padded_size([p[6:] for p in plans], 32)
    got = P.resize_crop_resize_normalize_pad(imgs, plans)
    assert torch.equal(got, _chain(P, imgs, plans, pad_hw))


def test_a_shrink_at_the_edge_of_the_lds_tile_mixes_both_paths_in_one_image():
    """43 output rows from 120: a 4-row tile reads 10 or 11 intermediate rows, the tile holds 10, so neighbouring workgroups take
    different paths; 60 from 120 (exactly 2) always fits."""
    P = _P()
    plans = [(120, 240, 0, 0, 120, 240, 43, 86), (120, 240, 0, 0, 120, 240, 60, 120), (120, 240, 7, 3, 113, 237, 41, 85)]
    imgs = torch.from_numpy(_smooth_batch(3, 64, 128, 37)).to(DEV)
    got = P.resize_crop_resize_normalize_pad(imgs, plans, size_divisor=1)
    assert torch.equal(got, _chain(P, imgs, plans, (60, 120)))


def test_device_plan_is_clamped_like_the_host_would_clamp_it():
    P = _P()
    imgs = torch.from_numpy(_smooth_batch(3, 49, 98, 41)).to(DEV)
    clamped = [(0, 0, 0, 0, 0, 0, 30, 60), (37, 75, 10, 20, 27, 40, 33, 50), (37, 75, 2, 3, 20, 30, 25, 41)]
    loose = [list(p) for p in clamped]
    loose[1][4] += 3                                                               # ch = h1 - cy + 3, on the second image of three
    pad_hw = (40, 64)
    want = P.resize_crop_resize_normalize_pad(imgs, clamped, pad_hw=pad_hw)
    got = P.resize_crop_resize_normalize_pad(imgs, torch.tensor(loose, dtype=torch.int32, device=DEV), pad_hw=pad_hw)
    assert torch.equal(got, want)
    assert torch.equal(want, _chain(P, imgs, clamped, pad_hw))
    # every other clamp: negative offsets, a crop past the right edge, an output larger than the pad
    loose = [[0, 0, 0, 0, 0, 0, 30, 60], [37, 75, -4, -2, 100, 200, 33, 50], [37, 75, 2, 70, 20, 30, 99, 99]]
    tight = [(0, 0, 0, 0, 0, 0, 30, 60), (37, 75, 0, 0, 37, 75, 33, 50), (37, 75, 2, 70, 20, 5, 40, 64)]
    got = P.resize_crop_resize_normalize_pad(imgs, torch.tensor(loose, dtype=torch.int32, device=DEV), pad_hw=pad_hw)
    assert torch.equal(got, P.resize_crop_resize_normalize_pad(imgs, tight, pad_hw=pad_hw))


def test_policy_0_rows_equal_the_existing_resize_kernel():
    P = _P()
    sizes = [(37, 75), (49, 98), (20, 33)]
    imgs = torch.from_numpy(_smooth_batch(3, 49, 98, 43)).to(DEV)
    got = P.resize_crop_resize_normalize_pad(imgs, [(0, 0, 0, 0, 0, 0) + s for s in sizes])
    assert torch.equal(got, P.resize_normalize_pad(imgs, sizes))


def test_captured_graph_replays_another_plan():
    P = _P()
    B, H, W = 3, 64, 128
    plans = [(0, 0, 0, 0, 0, 0, 96, 192), (100, 200, 10, 20, 80, 120, 96, 144), (0, 0, 0, 0, 0, 0, 64, 128)]
    new_plans = [(90, 180, 0, 60, 90, 120, 72, 96), (0, 0, 0, 0, 0, 0, 50, 100), (100, 200, 30, 0, 70, 200, 35, 100)]
    Hp, Wp = 96, 192
    imgs = torch.from_numpy(_smooth_batch(B, H, W, 3)).to(DEV)
    prm = P.params_tensor(P.draw_pano_params(B, W, rng=np.random.RandomState(0)), DEV)
    plan = torch.tensor(plans, dtype=torch.int32, device=DEV)
    norm = P.norm_tensor(P.IMG_NORM_MEAN, P.IMG_NORM_STD, DEV)
    warped = torch.empty_like(imgs)
    x = torch.empty(B, 3, Hp, Wp, device=DEV)

    def step():
        P.pano_warp(imgs, prm, out=warped)
        P.resize_crop_resize_normalize_pad(warped, plan, pad_hw=(Hp, Wp), out=x, norm=norm)

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
    prm.copy_(P.params_tensor(new, DEV))
    plan.copy_(torch.tensor(new_plans, dtype=torch.int32))
    x.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    eager = P.resize_crop_resize_normalize_pad(P.pano_warp(imgs, new), new_plans, pad_hw=(Hp, Wp))
    assert torch.equal(x, eager)


def test_caller_buffers_are_checked_before_the_launch():
    P = _P()
    B, H, W = 2, 32, 64
    imgs = torch.from_numpy(_smooth_batch(B, H, W, 4)).to(DEV)
    plans = [(0, 0, 0, 0, 0, 0, 32, 64), (40, 80, 4, 8, 30, 60, 16, 32)]
    Hp, Wp = P.padded_size([p[6:] for p in plans], 32)
    plan = torch.tensor(plans, dtype=torch.int32, device=DEV)
    norm = P.norm_tensor(P.IMG_NORM_MEAN, P.IMG_NORM_STD, DEV)
    for out in (torch.empty(B, 3, Hp, Wp), torch.empty(B + 1, 3, Hp, Wp, device=DEV), torch.empty(B, 3, Hp, Wp + 32, device=DEV),
                torch.empty(B, 3, Hp, Wp, device=DEV, dtype=torch.bfloat16), torch.empty(B, 3, Hp, 2 * Wp, device=DEV)[..., ::2], norm):
        with pytest.raises(P.PswinError):
            P.resize_crop_resize_normalize_pad(imgs, plan, pad_hw=(Hp, Wp), out=out, norm=norm)
    for n in (norm.cpu(), norm.double(), torch.zeros(3, device=DEV), torch.zeros(12, device=DEV)[::2]):
        with pytest.raises(P.PswinError):
            P.resize_crop_resize_normalize_pad(imgs, plan, pad_hw=(Hp, Wp), norm=n)
    for bad in (plan.cpu(), plan.long(), plan[:, :7].contiguous(), torch.zeros(B, 16, dtype=torch.int32, device=DEV)[:, ::2]):
        with pytest.raises(P.PswinError):
            P.resize_crop_resize_normalize_pad(imgs, bad, pad_hw=(Hp, Wp))
    with pytest.raises(P.PswinError):
        P.resize_crop_resize_normalize_pad(imgs, plan)                               # a device plan needs pad_hw
    with pytest.raises(P.PswinError):
        P.resize_crop_resize_normalize_pad(imgs, [plans[0], (40, 80, 20, 8, 30, 60, 16, 32)])      # the crop leaves 40 x 80
    with pytest.raises(P.PswinError):
        P.resize_crop_resize_normalize_pad(imgs, plans, pad_hw=(16, 64))             # an output larger than the pad
    ok = torch.empty(B, 3, Hp, Wp, device=DEV)
    assert P.resize_crop_resize_normalize_pad(imgs, plan, pad_hw=(Hp, Wp), out=ok, norm=norm) is ok
    assert torch.equal(ok, P.resize_crop_resize_normalize_pad(imgs, plans))


def test_the_streetwin_recipe_end_to_end():
    from _util import TINY
    from panoswintransformerobjectdetection_amd import SimplePanoSwinTransformer
    P = _P()
    B, H, W = 4, 64, 128
    imgs = torch.from_numpy(_smooth_batch(B, H, W, 12)).to(DEV)
    boxes = [np.array([[0, 10, 30, 40], [100, 5, 128, 50]], np.float32), np.array([[20, 20, 60, 60]], np.float32),
             np.array([[0, 0, 128, 64]], np.float32), np.array([[40, 8, 90, 60], [2, 2, 6, 6]], np.float32)]
    labels = [np.array([1, 2], np.int64), np.array([3], np.int64), np.array([0], np.int64), np.array([4, 1], np.int64)]
    x, b, l, metas = P.PanoTrainTransform(auto_augment=P.STREETWIN_AUTO_AUGMENT, rng=np.random.RandomState(3))(imgs, boxes, labels)
    params, aas = P.PanoTrainTransform(auto_augment=P.STREETWIN_AUTO_AUGMENT, rng=np.random.RandomState(3)).draw_auto(B, H, W)
    plans = [a["plan"] for a in aas]
    assert {a["policy"] for a in aas} == {0, 1}
    want = P.resize_crop_resize_normalize_pad(P.pano_warp(imgs, params), plans, size_divisor=32)
    assert torch.equal(x, want) and x.shape[2] % 32 == 0 and x.shape[3] % 32 == 0
    wb, wl = P.transform_boxes(boxes, labels, H, W, params)
    for i, (m, a) in enumerate(zip(metas, aas)):
        h1, w1, cy, cx, ch, cw, oh, ow = a["plan"]
        eb, el = P.auto_augment_boxes(wb[i], wl[i], H, W, a)
        assert np.array_equal(b[i], eb) and np.array_equal(l[i], el) and b[i].dtype == np.float32 and len(b[i]) == len(l[i])
        assert (b[i][:, 0::2] <= ow).all() and (b[i][:, 1::2] <= oh).all() and (b[i] >= 0).all()
        assert m["img_shape"] == (oh, ow, 3) and m["scale"] == a["scale"] and m["auto_augment_policy"] == a["policy"]
        assert m["batch_input_shape"] == tuple(x.shape[2:]) and m["pad_shape"][0] % 32 == 0 and m["pad_shape"][0] >= oh
        assert m["flip"] == bool(params["flip"][i]) and m["roll_shift"] == params["shift"][i]
        if a["policy"]:
            assert m["crop"] == (cy, cx, cy + ch, cx + cw) and m["pano_ratio_v"] == [cy / h1, (cy + ch) / h1]
            assert m["pano_lr_noadj"] == (cw == w1)
            assert np.array_equal(m["scale_factor"], np.array([ow / cw, oh / ch, ow / cw, oh / ch], np.float32))
        else:
            assert m["crop"] is None and m["pano_ratio_v"] == [0.0, 1.0] and m["pano_lr_noadj"] is None
            assert np.array_equal(m["scale_factor"], np.array([ow / W, oh / H, ow / W, oh / H], np.float32))
    torch.manual_seed(0)
    model = SimplePanoSwinTransformer(**TINY, compute_dtype=torch.bfloat16).to(DEV).eval()
    model.init_weights(None)
    with torch.no_grad():
        outs = model(x)
    assert len(outs) == 4 and all(torch.isfinite(o.float()).all() for o in outs)
