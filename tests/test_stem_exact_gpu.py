"""The tile kernels of the fused PatchEmbed stem (csrc/pswin_stem.hip, csrc/pswin_stem_tiles.inc), driven through stem.py on operands
with ONE right answer (tests/_stem_exact_cases.py; tests/test_stem_exact.py shows on the CPU that the cases see planted defects).
Every comparison is on bit patterns -- int16 views of bf16, int32 views of f32 -- and by value only where the expected value is 0
(the sign of a zero is not part of the contract).  There is no tolerance in this file.

Each kernel gets the EXPECTED upstream tensors, so a failure names one kernel; test_chain_dense feeds the kernels their own outputs.
Every output buffer that stem.py allocates and the workspace hold NaN before each call, every kernel runs twice and must return
the same bits, and the packing kernel must equal the host packing on every case's weights.

Shapes (B, H, W) and what each is the smallest to reach: (1, 4, 4) one token, every lane but one clamped to M - 1, tiles almost
entirely outside the image; (1, 16, 32) exactly one 16-row tile, two 8-row tiles, one 32-token weight-gradient step; (1, 20, 36)
ragged for both tile heights, M = 45; (2, 24, 40) a halo that must not read the neighbouring image, M = 120; (3, 52, 100) M = 975:
two conv3_fwd workgroups with a ragged end, eight token groups, a last tile column 4 pixels wide.  `thin` only:
(3, 144, 320) 270 16-row tiles on a grid of 256 (conv2_fwd with its prefetch live, conv2_bwd: second trip), 540 8-row tiles on a grid
of 512 (conv1_stats, conv2_wgrad: second trip), M = 8640: conv3_wgrad with per = 3 steps in 90 workgroups per tap row;
(1, 512, 1028) M = 32896 = 257 token groups on a grid of 256: one workgroup of conv3_bwd_stats / conv3_bwd_data makes a second
trip through both weight halves.  These counts are asserted from the launch rules below.

Observed on the MI355X: all 110 kernel tests equal bit for bit (no kernel had to be changed), 8.8 s in all, the slowest 2.3 s (it builds the
(3, 144, 320) case).  Trip counts there: (3, 144, 320) 270 tiles on 256 workgroups and 540 tiles on 512 workgroups, i.e. 14 and 28
workgroups make a second trip; conv3_wgrad 90 workgroups per tap row with 3 steps each; (1, 512, 1028) 257 token groups on 256
workgroups, workgroup 0 takes groups 0 and 256.  Shares the classes reached at the five small shapes in the order above (conditions
on the operands, asserted in _stem_exact_cases.case and identical on every host):
  dense  z1 == 0 on 8.8 / 6.2 / 6.5 / 6.4 / 6.4 % and z2 == 0 on 11.3 / 2.9 / 2.6 / 2.4 / 3.8 % of the elements, 45-49 % of z1 and
         33-56 % of z2 on either side of 0
  ties   exact bf16 ties: y2 10.8 / 14.9 / 15.8 / 13.4 / 16.4 %, tokens 20.8 / 20.0 / 18.0 / 19.5 / 20.0 %, dy2 12.4 / 12.6 / 14.2 /
         11.2 / 14.0 %, g1 5.3 / 6.8 / 6.9 / 6.6 / 0 %
test_chain_dense compares sum g1 and sum g1 yhat1 at the first four shapes; at (3, 52, 100) the chain's larger dy2 takes them past the
exactness bound and G, dw2 and everything upstream are compared."""
import pytest
import torch

import _stem_exact_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
SMALL = sc.SMALL_SHAPES
NAN = float("nan")


class _NanTorch:
    """torch as stem.py sees it in this file: every floating-point buffer it allocates with empty / empty_like holds NaN"""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*args, **kw):
        t = torch.empty(*args, **kw)
        return t.fill_(NAN) if t.is_floating_point() else t

    @staticmethod
    def empty_like(t, **kw):
        return torch.full_like(t, NAN, **kw)


@pytest.fixture(autouse=True)
def stem(monkeypatch):
    from panoswintransformerobjectdetection_amd import stem as module
    monkeypatch.setattr(module, "torch", _NanTorch())
    probe = module.conv1_stats.__globals__["torch"].empty(3, device=DEV)
    assert bool(torch.isnan(probe).all())
    return module


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same(got, want, what):
    """bit patterns equal; where the expected value is 0, the value is (either sign)"""
    if want.dtype == torch.float64:
        assert bool((want.float().double() == want).all()), what          # the expectation is an f32 number
        want = want.float()
    want = want.to(got.device).reshape(got.shape)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    ok = (_bits(got) == _bits(want)) | ((want == 0) & (got == 0))
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} elements differ; first at {i}: got {got[i].item()!r} "
                             f"(bits {_bits(got)[i].item():#x}), want {want[i].item()!r} (bits {_bits(want)[i].item():#x})")


def test_the_comparison_sees_one_bit_and_no_zero_sign():
    want = torch.tensor([1.0, -0.0, 0.0, 3.0], dtype=torch.float64)
    _same(torch.tensor([1.0, 0.0, -0.0, 3.0], device=DEV), want, "signed zeros")
    for dtype in (torch.float32, BF16):
        got = want.to(dtype).to(DEV)
        _bits(got)[3] += 1
        with pytest.raises(AssertionError, match="1 of 4 elements differ"):
            _same(got, want if dtype == torch.float32 else want.to(BF16), "one ulp")
    with pytest.raises(AssertionError):
        _same(torch.tensor([1.0, NAN, 0.0, 3.0], device=DEV), want, "NaN where 0 is expected")


def _twice(fn, ws=None):
    """run a kernel twice on a NaN workspace: identical bits"""
    outs = []
    for _ in range(2):
        if ws is not None:
            ws.fill_(NAN)
        r = fn()
        outs.append([t.clone() for t in (r if isinstance(r, tuple) else (r,))])
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b)), "two calls returned different bits"
    return outs[0] if len(outs[0]) > 1 else outs[0][0]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(BF16).to(DEV)


def _f32(*rows):
    return torch.stack([r.float() for r in rows]).contiguous().to(DEV)


class _Dev:
    """a case's operands on the device, in the kernels' layouts"""

    def __init__(self, stem, c):
        o = c.ops
        self.stem, self.c, self.shape = stem, c, c.shape
        if "x" in o:
            self.x = o["x"].float().to(DEV)
            self.x4 = stem.pack_input(self.x)
            B, H, W = c.shape
            _same(self.x4[..., :3], _nhwc(o["x"]), "pack_input")
            assert bool((self.x4[..., 3].float() == 1).all())
            self.w1p = stem.pack_w1(o["w1"].float().to(DEV))
            self.prm1 = _f32(o["scale1"], o["shift1"], o["a1c"], o["b1c"])
            self.ws = stem.workspace(self.x)
        else:
            B, H, W = c.shape
            self.ws = stem.workspace(torch.empty(B, 3, H, W, device=DEV))        # (only its shape and device are read)
        if o.get("w2") is not None:
            w2 = o["w2"].float().to(DEV)
            self.w2p, self.w2t = stem.pack_taps(w2, False), stem.pack_taps(w2, True)
        if o.get("w3") is not None:
            w3 = o["w3"].float().to(DEV)
            self.w3p, self.w3t = stem.pack_taps(w3, False), stem.pack_taps(w3, True)
        if "scale2" in o:
            self.sc2, self.sh2 = o["scale2"].float().to(DEV), o["shift2"].float().to(DEV)
        if "bias3" in o:
            self.bias3 = o["bias3"].float().to(DEV)
        if "a2c" in o:
            self.prm2 = _f32(o["scale2"], o["shift2"], o["a2c"], o["b2c"])
        if "k1" in o:
            self.prm5 = _f32(o["scale2"], o["shift2"], o["k1"], o["P"], o["Q"])
        if "dtok" in o:
            self.dtok = o["dtok"].to(BF16).to(DEV).contiguous()
        if "dy2_in" in o:
            self.dy2_in = _nhwc(o["dy2_in"])
        y2 = o["y2"] if "y2" in o else c.out.get("y2")             # the expected upstream activation
        if y2 is not None:
            self.y2 = _nhwc(y2)


_DEV_CACHE = {}


def _dev(stem, c):
    key = id(c)
    if key not in _DEV_CACHE:
        if len(_DEV_CACHE) >= 3:
            _DEV_CACHE.clear()
        _DEV_CACHE[key] = (c, _Dev(stem, c))
    d = _DEV_CACHE[key][1]
    d.stem = stem
    return d


# --- one function per kernel: run twice on NaN buffers, compare what the class compares --------------------------------------
def run_pack_weights(d):
    o = d.c.ops
    got = d.stem.pack_weights(o["w1"].float().to(DEV), o["w2"].float().to(DEV), o["w3"].float().to(DEV))
    for g, w, name in zip(got, (d.w1p, d.w2p, d.w2t, d.w3p, d.w3t), ("w1p", "w2p", "w2t", "w3p", "w3t")):
        assert torch.equal(_bits(g), _bits(w)), name


def run_conv1_stats(d):
    sums = _twice(lambda: d.stem.conv1_stats(d.x4, d.w1p, d.ws), d.ws)
    _same(sums, d.c.out["sums1"], "conv1_stats sums1")
    return sums


def run_conv2_fwd(d):
    y2, sums2 = _twice(lambda: d.stem.conv2_fwd(d.x4, d.w1p, d.prm1[0], d.prm1[1], d.w2p, d.ws), d.ws)
    keys = sc.compared(d.c.cls, "B", d.shape) if d.c.cls != "select" else ("y2",)
    _same(y2, _nhwc(d.c.out["y2"]), "conv2_fwd y2")
    if "sums2" in keys:
        _same(sums2, d.c.out["sums2"], "conv2_fwd sums2")
    if "sums2_sum" in keys:
        _same(sums2[:64], d.c.out["sums2_sum"], "conv2_fwd sum y2")
    y2n, none = d.stem.conv2_fwd(d.x4, d.w1p, d.prm1[0], d.prm1[1], d.w2p, d.ws, want_stats=False)
    assert none is None and torch.equal(_bits(y2n), _bits(y2))
    return y2, sums2


def run_conv3_fwd(d, y2=None):
    tok = _twice(lambda: d.stem.conv3_fwd(d.y2 if y2 is None else y2, d.sc2, d.sh2, d.w3p, d.bias3))
    _same(tok, d.c.out["tok"], "conv3_fwd tokens")
    return tok


def run_conv3_bwd_stats(d, y2=None):
    sums = _twice(lambda: d.stem.conv3_bwd_stats(d.dtok, d.y2 if y2 is None else y2, d.prm2, d.w3t, d.ws), d.ws)
    _same(sums, d.c.out["sums3"], "conv3_bwd_stats sums3")
    return sums


def run_conv3_bwd_data(d, y2=None):
    dy2 = _twice(lambda: d.stem.conv3_bwd_data(d.dtok, d.y2 if y2 is None else y2, d.prm5, d.w3t))
    _same(dy2, _nhwc(d.c.out["dy2"]), "conv3_bwd_data dy2")
    return dy2


def run_conv3_wgrad(d, y2=None):
    y2 = d.y2 if y2 is None else y2
    for direct in (True, False):
        dw3 = _twice(lambda: d.stem.conv3_wgrad(d.dtok, y2, d.sc2, d.sh2, d.ws, direct=direct), d.ws)
        _same(dw3.contiguous(), d.c.out["dw3"], f"conv3_wgrad dw3 (direct={direct})")
    return dw3


def run_conv2_wgrad(d, dy2=None, want=None):
    dy2 = d.dy2_in if dy2 is None else dy2
    for direct in (True, False):
        dw2 = _twice(lambda: d.stem.conv2_wgrad(d.x4, d.w1p, d.prm1[0], d.prm1[1], dy2, d.ws, direct=direct), d.ws)
        _same(dw2.contiguous(), d.c.out["dw2"] if want is None else want, f"conv2_wgrad dw2 (direct={direct})")
    return dw2


def run_conv2_bwd(d, dy2=None, want=None, keys=None):
    dy2 = d.dy2_in if dy2 is None else dy2
    sg, sgy, G = _twice(lambda: d.stem.conv2_bwd(d.x4, d.w1p, d.prm1, dy2, d.w2t, d.ws), d.ws)
    want = d.c.out if want is None else want
    keys = sc.compared(d.c.cls, "E", d.shape) if keys is None else keys
    for k, got in (("sg1", sg), ("sgy1", sgy), ("G", G)):
        if k in keys:
            _same(got.contiguous(), want[k], "conv2_bwd " + k)


CLS = ["dense", "ties"]


@pytest.mark.parametrize("B,H,W", SMALL)
@pytest.mark.parametrize("cls", CLS)
def test_pack_weights(stem, cls, B, H, W):
    run_pack_weights(_dev(stem, sc.case(cls, B, H, W)))


@pytest.mark.parametrize("B,H,W", SMALL)
def test_conv1_stats(stem, B, H, W):
    run_conv1_stats(_dev(stem, sc.case("dense", B, H, W)))


@pytest.mark.parametrize("B,H,W", SMALL)
@pytest.mark.parametrize("cls", CLS)
def test_conv2_fwd(stem, cls, B, H, W):
    run_conv2_fwd(_dev(stem, sc.case(cls, B, H, W)))


@pytest.mark.parametrize("B,H,W", SMALL)
@pytest.mark.parametrize("cls", CLS)
def test_conv3_fwd(stem, cls, B, H, W):
    run_conv3_fwd(_dev(stem, sc.case(cls, B, H, W)))


@pytest.mark.parametrize("B,H,W", SMALL)
def test_conv3_bwd_stats(stem, B, H, W):
    run_conv3_bwd_stats(_dev(stem, sc.case("dense", B, H, W)))


@pytest.mark.parametrize("B,H,W", SMALL)
@pytest.mark.parametrize("cls", CLS)
def test_conv3_bwd_data(stem, cls, B, H, W):
    run_conv3_bwd_data(_dev(stem, sc.case(cls, B, H, W)))


@pytest.mark.parametrize("B,H,W", SMALL)
def test_conv3_wgrad(stem, B, H, W):
    run_conv3_wgrad(_dev(stem, sc.case("dense", B, H, W)))


@pytest.mark.parametrize("B,H,W", SMALL)
def test_conv2_wgrad(stem, B, H, W):
    run_conv2_wgrad(_dev(stem, sc.case("dense", B, H, W)))


@pytest.mark.parametrize("B,H,W", SMALL)
@pytest.mark.parametrize("cls", CLS)
def test_conv2_bwd(stem, cls, B, H, W):
    run_conv2_bwd(_dev(stem, sc.case(cls, B, H, W)))


# --- select: every output a bit copy; the failure message's index gives the output channel, info["pos"] its tap ------------------
def _select(stem, B, H, W, name):
    c = sc.select_case(B, H, W)[name]
    return _Dev(stem, c)


@pytest.mark.parametrize("B,H,W", SMALL)
def test_select_conv2_fwd(stem, B, H, W):
    d = _select(stem, B, H, W, "conv2")
    run_pack_weights(d)
    run_conv2_fwd(d)


@pytest.mark.parametrize("B,H,W", SMALL)
def test_select_conv3_fwd(stem, B, H, W):
    run_conv3_fwd(_select(stem, B, H, W, "conv3_fwd"))


@pytest.mark.parametrize("B,H,W", SMALL)
def test_select_conv3_bwd_data(stem, B, H, W):
    run_conv3_bwd_data(_select(stem, B, H, W, "conv3_bwd_data"))


@pytest.mark.parametrize("B,H,W", SMALL)
def test_select_conv3_wgrad(stem, B, H, W):
    run_conv3_wgrad(_select(stem, B, H, W, "conv3_wgrad"))


@pytest.mark.parametrize("B,H,W", SMALL)
def test_select_conv2_wgrad(stem, B, H, W):
    run_conv2_wgrad(_select(stem, B, H, W, "conv2_wgrad"))


# --- the kernels on their own outputs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SMALL)
def test_chain_dense(stem, B, H, W):
    c = sc.case("dense", B, H, W)
    d = _dev(stem, c)
    run_pack_weights(d)
    run_conv1_stats(d)
    y2, _ = run_conv2_fwd(d)
    run_conv3_fwd(d, y2)
    run_conv3_bwd_stats(d, y2)
    dy2 = run_conv3_bwd_data(d, y2)
    run_conv3_wgrad(d, y2)
    # conv2's backward kernels on the chain's dy2: the expectation from the same restatement; each output is compared where its
    # float64 exactness bound holds on this larger gradient (dy2 and g1 are multiples of 1/4, yhat1 of 1/2)
    e = sc.restate(dict(c.ops, dy2_in=c.out["dy2"].double()), "E")
    assert sc._exact(e["bound_dw2"], 2)
    run_conv2_wgrad(d, dy2, e["dw2"])
    keys = [k for k, ok in (("sg1", sc._exact(e["bound_out5"], 3)), ("sgy1", sc._exact(e["bound_out5"], 3)),
                            ("G", sc._exact(e["bound_G"], 2) and sc._exact(e["bound_g1"], 2))) if ok]
    print("chain", (B, H, W), "conv2_bwd outputs compared:", keys)
    assert "G" in keys or B * H * W > 4096
    run_conv2_bwd(d, dy2, e, keys)


# --- beyond one sweep of the grids: `thin`, one function per kernel -----------------------------------------------------------------
def _trip(stem):
    n = sc.launch_counts(*sc.TRIP_SHAPE)
    # grid_for (pswin_stem.hip:721): min(tiles, 256 per_cu); per_cu = 1 for the 16-row kernels, 2 for the 8-row kernels
    assert n["tiles16"] == 270 and n["grid16"] == 256 and n["tiles8"] == 540 and n["grid8"] == 512
    # pswin_stem_conv3_wgrad (:815-832): 270 steps of 32 tokens, 128 splits -> per = 3 -> 90 workgroups per tap row
    assert n["M"] == 8640 and n["per"] == 3 and n["splits"] == 90
    return _dev(stem, sc.case("thin", *sc.TRIP_SHAPE))


def test_trips_conv1_stats(stem):
    run_conv1_stats(_trip(stem))


def test_trips_conv2_fwd(stem):
    run_conv2_fwd(_trip(stem))


def test_trips_conv3_fwd(stem):
    run_conv3_fwd(_trip(stem))


def test_trips_conv3_bwd_stats(stem):
    run_conv3_bwd_stats(_trip(stem))


def test_trips_conv3_bwd_data(stem):
    run_conv3_bwd_data(_trip(stem))


def test_trips_conv3_wgrad(stem):
    run_conv3_wgrad(_trip(stem))


def test_trips_conv2_wgrad(stem):
    run_conv2_wgrad(_trip(stem))


def test_trips_conv2_bwd(stem):
    run_conv2_bwd(_trip(stem))


def _groups(stem):
    n = sc.launch_counts(*sc.GROUP_SHAPE)
    # pswin_stem_conv3_bwd_stats / _data (:786-812): persistent, min(groups of 128 tokens, 256) workgroups
    assert n["M"] == 32896 and n["groups"] == 257 and n["grid_groups"] == 256
    return _dev(stem, sc.case_groups(*sc.GROUP_SHAPE))


def test_groups_conv3_bwd_stats(stem):
    run_conv3_bwd_stats(_groups(stem))


def test_groups_conv3_bwd_data(stem):
    run_conv3_bwd_data(_groups(stem))
