"""pswin_pano_masks (csrc/pswin_pano.hip) on the MI355X, bit for bit: against the host definition (pano_aug.transform_masks_one) on a
batch that mixes every path, at padded widths with a store tail, against pano_warp on the same planes, on pre-filled buffers, on
out-of-contract device inputs, as a captured graph replayed on new draws, the wrapper's checks, and PanoTrainTransform.with_targets
feeding MiniMaskRCNN.heads_loss.

The kernel's tile as built: a workgroup of 16 x 16 threads writes 16 output rows x 256 columns (MASK_TY x MASK_COLS; a thread owns 16
consecutive columns of one row and stores them as 16 bytes, as four 32-bit words or as bytes) for all Gmax rows of one image; the grid
is (ceil(Wp / 256), ceil(Hp / 16), B)."""
import numpy as np
import pytest
import torch

import _pano_masks_ref as C

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
TILE_ROWS, TILE_COLS = 16, 256
H, W, GIN, GMAX = 48, 80, 3, 5


def _P():
    from panoswintransformerobjectdetection_amd import pano_aug as P
    return P


def _params(P, rows):
    """rows: (stretch, kx, ky, shift, flip) per image -> the dict of make_pano_params with the shifts as given."""
    st, kx, ky, sh, fl = zip(*rows)
    p = P.make_pano_params(list(st), list(kx), list(ky), None, list(fl), W)
    p["shift"] = np.array(sh, np.int64)
    return p


def _want(P, src, params, plans, rows, pad_hw, gmax=GMAX):
    """The definition, padded to [B, gmax, Hp, Wp]."""
    out = np.zeros((len(src), gmax) + tuple(pad_hw), np.uint8)
    for b, m in enumerate(P.transform_masks(list(src), params, plans, rows, pad_hw)):
        out[b, :len(m)] = m
    return out


# policy 0 up-resize, stretch, flip, roll 0, a merged row | policy 1 shrink then enlarge, crop at (5, 7), roll W - 1 | count 0, stretch
MIXED_PARAMS = [(1, 1.4, 0.7, 0, True), (0, 1.0, 1.0, W - 1, False), (1, 0.6, 1.9, 33, True)]
MIXED_PLANS = [(0, 0, 0, 0, 0, 0, 150, 250), (36, 60, 5, 7, 20, 31, 157, 243), (0, 0, 0, 0, 0, 0, 30, 50)]
MIXED_ROWS = [[[0, -1], [2, 1], [1, -1], [0, 2], [2, -1]], [[1, -1], [0, -1]], np.zeros((0, 2), np.int32)]


def _src():
    return np.stack([C.blobs(GIN, H, W, 40 + b) for b in range(3)])


def test_kernel_equals_the_definition_on_a_batch_that_mixes_every_path():
    P = _P()
    src, params, pad_hw = _src(), _params(P, MIXED_PARAMS), (160, 288)
    assert set(np.unique(src)) == {0, 1, 7, 255} and GIN != GMAX
    assert -(-pad_hw[0] // TILE_ROWS) > 1 and -(-pad_hw[1] // TILE_COLS) > 1 and len(src) > 1      # several workgroups along x, y, z
    dst = torch.empty(3, GMAX, *pad_hw, dtype=torch.uint8, device=DEV)
    got = P.warp_resize_masks(torch.from_numpy(src).to(DEV), params, MIXED_PLANS, MIXED_ROWS, pad_hw=pad_hw, out=dst)
    assert got is dst
    want = _want(P, src, params, MIXED_PLANS, MIXED_ROWS, pad_hw)
    assert np.array_equal(got.cpu().numpy(), want)
    assert want[0, 1].sum() > max(want[0, 0].sum(), want[0, 2].sum()) and not want[2].any() and not want[1, 2:].any()
    assert want[0].any() and want[1].any()


@pytest.mark.parametrize("Wp", [37, 52, 64, 276])
def test_store_tails_against_4_and_16_bytes_and_an_aligned_row(Wp):
    """37: byte stores, the third thread of a row writes 5 of its 16 columns; 52, 276: 32-bit stores, the last thread of a row writes one
    word of its four (52 = 3 * 16 + 4, 276 = 17 * 16 + 4); 64: 16-byte stores.  oh < Hp, ow < Wp, ow not a multiple of 4; Hp = 40 spans
    three workgroups along y, 276 two along x."""
    P = _P()
    Hp, ow = 40, Wp - 6 if Wp != 37 else 34
    assert ow % 4 and ow < Wp
    plans = [(0, 0, 0, 0, 0, 0, 33, ow), (36, 60, 5, 7, 20, 31, 37, ow - 9), (0, 0, 0, 0, 0, 0, 30, 17)]
    src, params = _src(), _params(P, MIXED_PARAMS)
    got = P.warp_resize_masks(torch.from_numpy(src).to(DEV), params, plans, MIXED_ROWS, pad_hw=(Hp, Wp))
    assert tuple(got.shape) == (3, GMAX, Hp, Wp)
    assert np.array_equal(got.cpu().numpy(), _want(P, src, params, plans, MIXED_ROWS, (Hp, Wp)))


def test_identity_plan_equals_pano_warp_on_the_same_planes():
    P = _P()
    src, params = _src(), _params(P, MIXED_PARAMS)
    rows = [np.stack([np.arange(GIN), np.full(GIN, -1)], 1)] * 3
    got = P.warp_resize_masks(torch.from_numpy(src).to(DEV), params, [(0, 0, 0, 0, 0, 0, H, W)] * 3, rows, size_divisor=1)
    assert tuple(got.shape) == (3, GIN, H, W)
    planes = torch.from_numpy((src != 0).astype(np.uint8).reshape(3 * GIN, H, W, 1)).to(DEV)
    per_plane = {k: np.repeat(v, GIN) for k, v in params.items()}
    assert torch.equal(got.reshape(3 * GIN, H, W, 1), P.pano_warp(planes, per_plane))


def test_every_byte_is_written_whatever_the_buffer_held():
    P = _P()
    src, params, pad_hw = torch.from_numpy(_src()).to(DEV), _params(P, MIXED_PARAMS), (160, 276)
    outs = []
    for fill in (0xFF, 0, 0xFF):
        dst = torch.full((3, GMAX) + pad_hw, fill, dtype=torch.uint8, device=DEV)
        outs.append(P.warp_resize_masks(src, params, MIXED_PLANS, MIXED_ROWS, pad_hw=pad_hw, out=dst).clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and int(outs[0].max()) == 1


def test_out_of_contract_device_inputs_are_clamped_as_the_contract_says():
    P = _P()
    src, params, pad_hw = _src(), _params(P, MIXED_PARAMS), (48, 64)
    loose = [[0, 0, 0, 0, 0, 0, 99, 99], [36, 60, 30, 50, 20, 31, 40, 50], [36, 60, -4, -2, 100, 200, 33, 50]]   # crops that leave 36 x 60
    tight = [(0, 0, 0, 0, 0, 0, 48, 64), (36, 60, 30, 50, 6, 10, 40, 50), (36, 60, 0, 0, 36, 60, 33, 50)]
    rows = np.full((3, GMAX, 2), -1, np.int32)
    rows[0, :, 0] = [0, GIN, -7, 2, 1]                       # rows = Gin and -7 read nothing
    rows[0, :, 1] = [GIN, 1, 2, -7, -1]
    rows[1, :, 0] = [2, 1, 0, 1, 2]
    rows[2, :, 0] = [0, 1, 2, 0, 1]
    count = [GMAX + 3, -2, 2]                               # clamped to [0, Gmax]
    dev = lambda a, dt: torch.tensor(a, dtype=dt, device=DEV)
    got = P.warp_resize_masks(torch.from_numpy(src).to(DEV), P.params_tensor(params, DEV), dev(loose, torch.int32),
                              torch.from_numpy(rows).to(DEV), dev(count, torch.int32), pad_hw=pad_hw)
    torch.cuda.synchronize()
    want = _want(P, src, params, tight, [rows[0], rows[1][:0], rows[2][:2]], pad_hw)
    assert np.array_equal(got.cpu().numpy(), want)
    assert want[0, 0].any() and want[0, 1].any() and want[0, 2].any() and not want[1].any() and not want[2, 2:].any()


def test_one_captured_graph_replays_on_new_draws():
    P = _P()
    src_h, pad_hw = _src(), (160, 288)
    src = torch.from_numpy(src_h).to(DEV)
    first = _params(P, MIXED_PARAMS)
    prm, plan = P.params_tensor(first, DEV), torch.tensor(MIXED_PLANS, dtype=torch.int32, device=DEV)
    packed, cnt = P.pack_rows(MIXED_ROWS, GMAX)
    rows, count = torch.from_numpy(packed).to(DEV), torch.from_numpy(cnt).to(DEV)
    dst = torch.empty(3, GMAX, *pad_hw, dtype=torch.uint8, device=DEV)

    def step():
        P.warp_resize_masks(src, prm, plan, rows, count, pad_hw=pad_hw, out=dst)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    torch.cuda.synchronize()
    new = _params(P, [(0, 1.0, 1.0, 17, True), (1, 1.8, 1.3, 0, False), (1, 0.9, 0.55, 79, False)])
    new_plans = [(30, 50, 2, 3, 25, 40, 100, 160), (0, 0, 0, 0, 0, 0, 24, 40), (0, 0, 0, 0, 0, 0, 160, 267)]
    new_rows = [[[2, -1]], [[0, 1], [1, -1], [2, 0]], [[1, 2], [0, -1], [0, -1], [2, -1], [1, 0]]]
    packed, cnt = P.pack_rows(new_rows, GMAX)
    prm.copy_(P.params_tensor(new, DEV))
    plan.copy_(torch.tensor(new_plans, dtype=torch.int32))
    rows.copy_(torch.from_numpy(packed))
    count.copy_(torch.from_numpy(cnt))
    dst.fill_(0xFF)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), _want(P, src_h, new, new_plans, new_rows, pad_hw))


def test_the_wrapper_rejects_bad_buffers_before_any_launch():
    P = _P()
    src = torch.from_numpy(_src()).to(DEV)
    params, pad_hw = _params(P, MIXED_PARAMS), (160, 288)
    ok = torch.empty(3, GMAX, *pad_hw, dtype=torch.uint8, device=DEV)
    call = lambda s=src, out=ok, **k: P.warp_resize_masks(s, params, MIXED_PLANS, MIXED_ROWS, pad_hw=pad_hw, out=out, **k)
    for bad in (src.cpu(), src.float(), src[:, :, :, :79], src[0]):                       # a CPU tensor, a wrong dtype, an odd W, 3 dims
        with pytest.raises(P.PswinError):
            call(s=bad)
    for out in (ok.cpu(), ok.float(), torch.empty(3, GMAX, pad_hw[0], 2 * pad_hw[1], dtype=torch.uint8, device=DEV)[..., ::2],
                torch.empty(3, GMAX + 1, *pad_hw, dtype=torch.uint8, device=DEV)[:, :GMAX], ok[:, :, :, :272]):
        with pytest.raises(P.PswinError):
            call(out=out)
    big = torch.empty(3 * GIN * H * W + 3 * GMAX * 16 * 32, dtype=torch.uint8, device=DEV)   # a dst that overlaps src
    s2 = big[:3 * GIN * H * W].view(3, GIN, H, W)
    s2.copy_(src)
    with pytest.raises(P.PswinError):
        P.warp_resize_masks(s2, params, [(0, 0, 0, 0, 0, 0, 16, 32)] * 3, MIXED_ROWS, pad_hw=(16, 32),
                            out=big[GIN * H * W:GIN * H * W + 3 * GMAX * 16 * 32].view(3, GMAX, 16, 32))
    rows_t = torch.from_numpy(P.pack_rows(MIXED_ROWS, GMAX)[0]).to(DEV)
    count_t = torch.tensor([5, 2, 0], dtype=torch.int32, device=DEV)
    for r, c in ((rows_t.long(), count_t), (rows_t, count_t.long()), (rows_t, None), (rows_t.cpu(), count_t), (rows_t[:, :, :1], count_t),
                 (rows_t, count_t[:2])):
        with pytest.raises(P.PswinError):
            P.warp_resize_masks(src, params, MIXED_PLANS, r, c, pad_hw=pad_hw)
    with pytest.raises(P.PswinError):
        P.warp_resize_masks(src, params, torch.tensor(MIXED_PLANS, dtype=torch.int32, device=DEV), MIXED_ROWS)    # a device plan needs pad_hw
    with pytest.raises(P.PswinError):
        P.warp_resize_masks(src, params, MIXED_PLANS, MIXED_ROWS, pad_hw=(100, 288))        # an output larger than the pad
    with pytest.raises(P.PswinError):
        P.warp_resize_masks(src, P.params_tensor(params, DEV).float(), MIXED_PLANS, MIXED_ROWS, pad_hw=pad_hw)
    assert call() is ok


def test_with_targets_feeds_the_mask_rcnn_heads():
    """The end of the chain: annotations -> with_targets -> heads_loss.  The masks the launch wrote equal, byte for byte, those copy_from
    puts there from the host definition, and so do boxes, labels and count; the losses of the two PaddedTargets are compared within the
    2e-3 relative bound this suite uses between two calls of heads_loss on the same annotations (tests/test_detector_padded_gpu.py: the
    heads' convolutions are not bit-stable from call to call)."""
    from _util import TINY
    from test_detector_padded_gpu import _fixed_keys
    from panoswintransformerobjectdetection_amd import detector as det
    P = _P()
    B, h, w = 2, 64, 128
    rng = np.random.RandomState(5)
    imgs = torch.from_numpy(rng.randint(0, 256, (B, h, w, 3)).astype(np.uint8)).to(DEV)
    boxes = [np.array([[0, 10, 30, 50], [98, 10, 128, 50], [40, 20, 90, 60]], np.float32), np.array([[10, 5, 70, 40], [60, 30, 120, 62]], np.float32)]
    labels = [np.array([3, 3, 7], np.int64), np.array([1, 5], np.int64)]
    masks = []
    for b in boxes:
        m = np.zeros((len(b), h, w), np.uint8)
        for i, (x1, y1, x2, y2) in enumerate(b.astype(int)):
            m[i, y1:y2, x1:x2] = 255
        masks.append(m)
    t = P.PanoTrainTransform(img_scales=[(128, 256)], rng=np.random.RandomState(2))
    x, T, metas = t.with_targets(imgs, boxes, labels, [torch.from_numpy(m).to(DEV) for m in masks])
    assert tuple(x.shape) == (B, 3, 128, 256) and tuple(T.masks.shape) == (B, T.max_gt, 128, 256) and T.masks.dtype == torch.uint8
    # the same draws, on the host
    t2 = P.PanoTrainTransform(img_scales=[(128, 256)], rng=np.random.RandomState(2))
    params, scales = t2.draw(B, w)
    wb, wl, maps = P.transform_boxes(boxes, labels, h, w, params, row_map=True)
    plans = [(0, 0, 0, 0, 0, 0, 128, 256)] * B
    host = P.transform_masks(masks, params, plans, maps, (128, 256))
    U = det.PaddedTargets.allocate(B, T.max_gt, DEV, mask_hw=(128, 256))
    U.copy_from([P.resize_boxes(v, h, w, 128, 256) for v in wb], wl, host)
    assert torch.equal(T.masks, U.masks) and torch.equal(T.boxes, U.boxes) and torch.equal(T.labels, U.labels) and torch.equal(T.count, U.count)
    assert T.masks.any() and int(T.masks.max()) == 1

    torch.manual_seed(0)
    m = det.MiniMaskRCNN(dict(TINY, compute_dtype=torch.float32), num_classes=80).to(DEV).train()
    m.backbone.init_weights(None)
    m.rand_like = _fixed_keys()
    with torch.no_grad():
        feats = m.backbone(x)
        got = m.heads_loss(feats, T, (128, 256))
        want = m.heads_loss(feats, U, (128, 256))
    assert bool(torch.isfinite(got["loss_mask"])) and float(got["loss_mask"]) > 0
    for k in want:
        assert abs(float(got[k]) - float(want[k])) <= 2e-3 * max(abs(float(want[k])), 1e-3), (k, float(got[k]), float(want[k]))
