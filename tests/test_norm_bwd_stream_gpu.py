"""The persistent LayerNorm backward kernels (csrc/pswin_norm.hip) where their workgroups make different numbers of trips.  A
workgroup makes its first request and as many dropped stores as a trip makes in front of the row loop, and enters the loop without a
test: with 3/2 sweeps of the resident grid workgroups with two trips stand next to workgroups with one, with 7/2 sweeps four trips next
to three and the last prefetch runs past the end, one row beyond a sweep gives one workgroup a second trip of a single row, and
S = rpb + 1 tokens per image puts the rows of a trip into two images.  Checked as in tests/test_norm_rows_gpu.py (whose case builders
this file uses): exact-row against generic kernels bit for bit on every output, and against a float64 reference of the same inputs.
The largest case moves about 45 MB per tensor.  Needs an MI355X."""
import pytest
import torch

from detfill import det_uniform
from test_norm_rows_gpu import (BF16OUT, DEV, DX_BF16, DX_F32, EPS, F32OUT, _both_paths, _check, _gather_case, _leaf, _leaf64, _ln64,
                                _nchw_case, _stats)

pytestmark = pytest.mark.gpu


def _grid(ops, C):
    """(resident grid of the backward kernels, rows per workgroup and trip) at width C = 12 L"""
    return ops._lib.load().pswin_ln_partial_rows(1 << 24, C), 256 // (C // 12)


def _sweeps(ops, C, num, den):
    blocks, rpb = _grid(ops, C)
    rows = blocks * rpb * num // den
    assert rows * den == blocks * rpb * num and ops._lib.load().pswin_ln_partial_rows(rows, C) == blocks
    return rows


def _shortcut_ex_case(ops, C, B, S):
    """scatter_add_layer_norm in token order: its backward is the LayerNorm backward kernel with the shortcut gradient, the shortcut
    bias sums (RSUM), a bf16 dy and the extra bf16 output (the branch gradient scale_b * dx) -- the form the training step launches"""
    tag = f"nbs:{C}:{S}"
    win = det_uniform((B, S, C), tag + "w", 2.0).to(torch.bfloat16)
    x = det_uniform((B, S, C), tag + "x", 2.0)
    gamma, beta = det_uniform((C,), tag + "g", 0.5, 1.0), det_uniform((C,), tag + "b", 0.5)
    pbias, fbias = det_uniform((C,), tag + "pb", 0.5), det_uniform((C,), tag + "fb", 0.5)
    s1, s2 = torch.tensor([0.75, 1.25][:B]), torch.tensor([1.25, 0.5][:B])
    gy = det_uniform((B, S, C), tag + "gy").to(torch.bfloat16)
    gx = det_uniform((B, S, C), tag + "gx")
    ident = ops.identity_map(S, DEV)

    def run():
        wd, xd, gd, bd, fb = _leaf(win), _leaf(x), _leaf(gamma), _leaf(beta), _leaf(fbias)
        y, x1 = ops.scatter_add_layer_norm(wd, xd, ident, None, s1.to(DEV), pbias.to(DEV), gd, bd, EPS, torch.bfloat16, res_bias=fb,
                                           res_scale=s2.to(DEV))
        mean, rstd = _stats(y)
        ((y.float() * gy.to(DEV).float()).sum() + (x1 * gx.to(DEV)).sum()).backward()
        return dict(y=y.detach(), x1=x1.detach(), mean=mean, rstd=rstd, dwin=wd.grad, dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad,
                    dres_sum=fb.grad)

    fast, generic = _both_paths(run)
    wr, xr, gr, br = _leaf64(win.float()), _leaf64(x), _leaf64(gamma), _leaf64(beta)
    x1r = xr + (wr + pbias.double()) * s1.double()[:, None, None]
    yr, mu, rstd = _ln64(x1r, gr, br)
    ((yr * gy.double()).sum() + (x1r * gx.double()).sum()).backward()
    ref = dict(y=yr.detach(), x1=x1r.detach(), mean=mu.detach(), rstd=rstd.detach(), dwin=wr.grad, dx=xr.grad, dgamma=gr.grad,
               dbeta=br.grad, dres_sum=(gx.double() * s2.double()[:, None, None]).sum((0, 1)))
    tols = dict(y=BF16OUT, x1=F32OUT, mean=F32OUT, rstd=F32OUT, dwin=DX_BF16, dx=DX_F32, dgamma="param", dbeta="param", dres_sum="param")
    _check(fast, generic, ref, tols)


@pytest.mark.parametrize("C", [96, 768])
@pytest.mark.parametrize("num,den", [(3, 2), (7, 2)])
def test_shortcut_backward_with_unequal_trips(ops, C, num, den):
    """3/2 sweeps: workgroups with two trips next to workgroups with one; 7/2: four trips next to three"""
    rows = _sweeps(ops, C, num, den)
    assert rows % 2 == 0
    _shortcut_ex_case(ops, C, 2, rows // 2)


@pytest.mark.parametrize("C", [96, 768])
def test_gather_backward_with_unequal_trips(ops, C):
    """the same 3/2 sweeps through layer_norm_gather: shortcut gradient and bias sums, bf16 dy, no extra output"""
    rows = _sweeps(ops, C, 3, 2)
    _gather_case(ops, C, 2, rows // 2, None, None, torch.float32, torch.bfloat16, True, True, False)


def test_nchw_backward_with_unequal_trips(ops):
    """7/2 sweeps of the NCHW backward kernel with the fused closing add at C = 768: 2 images of 64 x 112 tokens"""
    rows = _sweeps(ops, 768, 7, 2)
    assert rows == 2 * 64 * 112
    _nchw_case(ops, 768, 2, 64, 112, True, False)


def test_gather_backward_one_row_beyond_a_sweep(ops):
    """blocks * rpb + 1 rows at C = 384: one workgroup makes a trip of a single row"""
    blocks, rpb = _grid(ops, 384)
    _gather_case(ops, 384, 1, blocks * rpb + 1, None, None, torch.float32, torch.bfloat16, True, True, False)


def test_gather_backward_rows_straddle_two_images(ops):
    """2 images of rpb + 1 tokens at C = 96: the rows of a workgroup's trip lie in two images"""
    _, rpb = _grid(ops, 96)
    _gather_case(ops, 96, 2, rpb + 1, None, None, torch.float32, torch.bfloat16, True, True, False)
