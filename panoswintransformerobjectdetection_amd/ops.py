"""Operators of the PanoSwin hot path: torch.autograd wrappers over the C-ABI kernels (include/pswin.h).

Every function here launches hand-written gfx950 kernels from libpswin_hip.so on the current HIP stream.
There is no PyTorch/CPU fallback: a CPU tensor or a missing library raises ``PswinError``.
Reference file:line citations use HOT = mmdet/models/backbones/simple_panoswin_transformer.py.
"""
import ctypes
import math
import os

import torch
import torch.nn.functional as F

from . import _lib
from . import grad_queue
from ._lib import BF16, F32, MODE_PANO, MODE_PLANAR, WPAD, WTOK, PswinError, call, dtype_code, ptr
# the end-of-pass gradient queue: every "sum these partial rows" of the backward pass goes through sum_rows
from .grad_queue import deferred_reductions_available, flush_if_pending, flush_reductions, grad_slot, set_deferred_reductions, sum_rows  # noqa: F401

_CACHE = {}
# Feature switches.  Every one of them selects between two HIP paths (a fused kernel or the chain of kernels it replaces), never a CPU
# path; tests flip the module attributes to compare the two.  ONE environment variable remains for same-box A/B runs of the whole step:
# PSWIN_DISABLE="name[,name...]" turns the named features off (names = the lower-case attribute names below).
_DISABLED = {n.strip().lower() for n in os.environ.get("PSWIN_DISABLE", "").split(",") if n.strip()}


def _on(name):
    return name not in _DISABLED


# the per-window qkv -> attention -> proj kernel where it exists (C = 96); off: the unfused chain
FUSED_WINDOW_ATTENTION = _on("fused_window_attention")
# the tiled HIP GEMM (pswin_gemm_nt) for the Linear layers of stages 1-3 where it measured faster than the library kernels
# (profiles/r02_gemm_nt_vs_library.txt, profiles/r04_ab_runs.json); off: library GEMMs for those layers
GEMM_NT = _on("gemm_nt")
# fc2's data gradient + the backward of fc1's bias + GELU in one kernel (pswin_gemm_nt_gelu_bwd); off: two kernels
FUSED_GELU_BWD = _on("fused_gelu_bwd")
# fc1 with the bias + GELU in its epilogue (pswin_gemm_nt_gelu_fwd) and fc2 as one autograd node; off: GEMM, then a streaming bias + GELU pass
FUSED_MLP = _on("fused_mlp")
# off: the dScore-tile sums of an attention module run inside its backward instead of in one launch at the end of the pass
DEFER_TABLE_PARTIALS = _on("defer_table_partials")
# per-sample DropPath: the tiled GEMMs of the Mlp and the weight-gradient launch leave out the rows of the samples whose branch was
# dropped (factor 0: the branch output is multiplied by zero and every gradient into it is an exact zero); off: everything is computed
SAMPLE_SKIP = _on("sample_skip")


def _dev_key(device):
    device = torch.device(device)
    return (device.type, device.index if device.index is not None else torch.cuda.current_device())


def clear_caches():
    _CACHE.clear()


# ------------------------------------------------------------------------------------------------
# static (input independent) tables, cached per feature-map shape and device
# ------------------------------------------------------------------------------------------------
def window_maps(pano, H, W, shift, device):
    """(map int32 [nW*49], inv int32 [H*W], nW): WindowTransition + pad_x + window_partition as an index map
    (HOT:376-409, 486-491, 64-75) and its inverse (HOT:78-92, 516-528)."""
    key = ("map", bool(pano), H, W, shift, _dev_key(device))
    if key not in _CACHE:
        mode = MODE_PANO if pano else MODE_PLANAR
        _, _, nW = _lib.window_grid(mode, H, W)
        wmap = torch.empty(nW * WTOK, dtype=torch.int32, device=device)
        inv = torch.empty(H * W, dtype=torch.int32, device=device)
        call("pswin_window_map", wmap, mode, H, W, shift, ptr(wmap), ptr(inv))
        _CACHE[key] = (wmap, inv, nW)
    return _CACHE[key]


def window_pads(pano, H, W, shift, device):
    """int32 [nW*49 - H*W]: the window slots no token maps to (the zero rows of pad_x, HOT:486-491), ascending"""
    key = ("pads", bool(pano), H, W, shift, _dev_key(device))
    if key not in _CACHE:
        wmap, _, _ = window_maps(pano, H, W, shift, device)
        _CACHE[key] = torch.nonzero(wmap < 0).flatten().to(torch.int32).contiguous()
    return _CACHE[key]


def identity_map(S, device):
    """int32 arange(S): the row movers with this map are plain (scaled, residual-added, dtype-converting) row copies."""
    key = ("ident", S, _dev_key(device))
    if key not in _CACHE:
        _CACHE[key] = torch.arange(S, dtype=torch.int32, device=device)
    return _CACHE[key]


def planar_mask(H, W, shift, device):
    """BasicLayer._get_attention_mask (HOT:664-688): f32 [nW, 49, 49] of 0 / -100."""
    key = ("mask", H, W, shift, _dev_key(device))
    if key not in _CACHE:
        _, _, nW = _lib.window_grid(MODE_PLANAR, H, W)
        mask = torch.empty(nW, WTOK, WTOK, dtype=torch.float32, device=device)
        call("pswin_planar_mask", mask, H, W, shift, ptr(mask))
        _CACHE[key] = mask
    return _CACHE[key]


def uv_grid(H, W, device):
    """make_uv_hw2 (HOT:153-189): f32 [H*W, 2]."""
    key = ("uv", H, W, _dev_key(device))
    if key not in _CACHE:
        uv = torch.empty(H * W, 2, dtype=torch.float32, device=device)
        call("pswin_uv_grid", uv, H, W, ptr(uv))
        _CACHE[key] = uv
    return _CACHE[key]


def abs_pos_features(H, W, device):
    """xyzuv features of _pano_abs_position (HOT:926-932): f32 [H*W, 5]."""
    key = ("xyzuv", H, W, _dev_key(device))
    if key not in _CACHE:
        uv = uv_grid(H, W, device)
        feat = torch.empty(H * W, 5, dtype=torch.float32, device=device)
        call("pswin_abs_pos_features", feat, ptr(uv), H * W, ptr(feat))
        _CACHE[key] = feat
    return _CACHE[key]


def gather_uv(uv, wmap):
    out = torch.empty(wmap.numel(), 2, dtype=torch.float32, device=uv.device)
    call("pswin_gather_uv", uv, ptr(uv), ptr(wmap), wmap.numel(), ptr(out))
    return out


def haversine_windows(uv1, uv2):
    """haversine22 per window (lzx/models/great_circle.py:71-86): [n, 49, 2] x [n, 49, 2] -> [n, 49, 49]."""
    uv1, uv2 = uv1.contiguous().float(), uv2.contiguous().float()
    n = uv1.numel() // (2 * WTOK)
    dist = torch.empty(n, WTOK, WTOK, dtype=torch.float32, device=uv1.device)
    call("pswin_haversine_windows", dist, ptr(uv1), ptr(uv2), n, ptr(dist))
    return dist


def window_dist(H, W, shift, device):
    """Great-circle distance table of a pano block: [nW, 49, 49], identical for every image and step."""
    key = ("dist", H, W, shift, _dev_key(device))
    if key not in _CACHE:
        wmap, _, nW = window_maps(True, H, W, shift, device)
        uvw = gather_uv(uv_grid(H, W, device), wmap).view(nW, WTOK, 2)
        _CACHE[key] = haversine_windows(uvw, uvw)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------
# row movers
# ------------------------------------------------------------------------------------------------
def _gather_raw(x, wmap, scale, n_slots, out_dtype):
    B, S, C = x.shape
    win = torch.empty(B, n_slots, C, dtype=out_dtype, device=x.device)
    nreal = min(S, n_slots)
    call("pswin_window_gather", x, ptr(x), dtype_code(x), ptr(wmap), ptr(scale), ptr(win), dtype_code(win), B, S,
         n_slots, C, algo_bytes=B * C * (nreal * x.element_size() + n_slots * win.element_size()))
    return win


def _scatter_raw(win, inv, resid, scale, S, out_dtype, bias=None):
    B, n_slots, C = win.shape
    out = torch.empty(B, S, C, dtype=out_dtype, device=win.device)
    call("pswin_window_scatter_add", win, ptr(win), dtype_code(win), ptr(inv), ptr(resid), ptr(scale), ptr(bias), ptr(out),
         dtype_code(out), B, S, n_slots, C,
         algo_bytes=B * S * C * (win.element_size() + out.element_size() * (1 if resid is None else 2)))
    return out


class _WindowGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wmap, inv, out_dtype):
        ctx.save_for_backward(inv)
        ctx.S, ctx.in_dtype = x.shape[1], x.dtype
        return _gather_raw(x.contiguous(), wmap, None, wmap.numel(), out_dtype)

    @staticmethod
    def backward(ctx, dwin):
        (inv,) = ctx.saved_tensors
        return _scatter_raw(dwin.contiguous(), inv, None, None, ctx.S, ctx.in_dtype), None, None, None


def window_gather(x, wmap, inv, out_dtype=None):
    """[B, S, C] -> [B, nW*49, C]: shift + pad + window partition in one indexed row copy."""
    return _WindowGather.apply(x, wmap, inv, out_dtype or x.dtype)


class _WindowScatterAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, win, resid, wmap, inv, scale, bias, bias_grad_elsewhere):
        ctx.save_for_backward(wmap, scale)
        ctx.win_dtype = win.dtype
        ctx.bias_grad = bias is not None and not bias_grad_elsewhere
        b = None if bias is None else bias.detach().float().contiguous()
        return _scatter_raw(win.contiguous(), inv, resid.contiguous(), scale, resid.shape[1], resid.dtype, b)

    @staticmethod
    def backward(ctx, dout):
        wmap, scale = ctx.saved_tensors
        dout = dout.contiguous()
        dwin = _gather_raw(dout, wmap, scale, wmap.numel(), ctx.win_dtype)
        dbias = None
        if ctx.bias_grad and ctx.needs_input_grad[5]:       # generic path: one extra pass (the blocks avoid it, see below)
            g = dout.float() if scale is None else dout.float() * scale[:, None, None]
            dbias = colsum(g.reshape(-1, g.shape[-1]))
        return dwin, dout, None, None, None, dbias, None


def window_scatter_add(win, resid, wmap, inv, scale=None, bias=None, bias_grad_elsewhere=False):
    """resid + scale_b * (window_reverse(win) + bias): window reverse + crop + reverse shift + DropPath + residual
    (HOT:483, 516-533) in one indexed row copy.  win [B, nW*49, C], resid [B, S, C].

    bias: the bias of the Linear that produced win (so that the GEMM needs no epilogue).  bias_grad_elsewhere=True:
    this op returns no gradient for it; the caller obtains it from layer_norm_gather(..., res_bias=bias), whose
    backward kernel reads the shortcut gradient anyway."""
    return _WindowScatterAdd.apply(win, resid, wmap, inv, scale, bias, bias_grad_elsewhere)


class _PatchMergeGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, H, W, out_dtype):
        B, S, C = x.shape
        ctx.geom = (B, H, W, C, x.dtype)
        H2, W2 = (H + 1) // 2, (W + 1) // 2
        x = x.contiguous()
        out = torch.empty(B, H2 * W2, 4 * C, dtype=out_dtype, device=x.device)
        call("pswin_patch_merge_gather", x, ptr(x), dtype_code(x), ptr(out), dtype_code(out), B, H, W, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, H, W, C, dt = ctx.geom
        dout = dout.contiguous()
        dx = torch.empty(B, H * W, C, dtype=dt, device=dout.device)
        call("pswin_patch_merge_scatter", dout, ptr(dout), dtype_code(dout), ptr(dx), dtype_code(dx), B, H, W, C)
        return dx, None, None, None


def patch_merge_gather(x, H, W, out_dtype=None):
    """PatchMerging's 2x2 strided gather + concat (HOT:560-573): [B, H*W, C] -> [B, ceil(H/2)*ceil(W/2), 4C]."""
    return _PatchMergeGather.apply(x, H, W, out_dtype or x.dtype)


class _LayerNormGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, wmap, inv, out_dtype, passthrough, res_bias, res_scale, add_rows=None):
        B, S, C = x.shape
        x = x.contiguous()
        n_out = S if wmap is None else wmap.numel()
        y = torch.empty(B, n_out, C, dtype=out_dtype, device=x.device)
        mean = torch.empty(B, S, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        if add_rows is None:
            call("pswin_ln_gather_fwd", x, ptr(x), dtype_code(x), ptr(wmap), ptr(gamma), ptr(beta), float(eps), ptr(y),
                 dtype_code(y), ptr(mean), ptr(rstd), B, S, n_out, C,
                 algo_bytes=B * C * (min(S, n_out) * x.element_size() + n_out * y.element_size()))
        else:
            if wmap is not None or add_rows.shape != (S, C) or add_rows.dtype != torch.float32 or passthrough:
                raise PswinError("layer_norm_gather(add_rows=...) takes f32 [S, C] rows, no window map and no passthrough")
            add_rows = add_rows.contiguous()
            call("pswin_ln_gather_fwd_add", x, ptr(x), dtype_code(x), None, ptr(gamma), ptr(beta), float(eps), ptr(add_rows), ptr(y),
                 dtype_code(y), ptr(mean), ptr(rstd), B, S, n_out, C, timed_as="pswin_ln_gather_fwd",
                 algo_bytes=B * C * (S * x.element_size() + n_out * y.element_size()) + 4 * S * C)
        ctx.has_add = add_rows is not None
        ctx.save_for_backward(x, gamma, mean, rstd, inv, res_scale)
        ctx.n_out = n_out
        ctx.want_res_sum = res_bias is not None
        ctx.owners = (gamma, beta, res_bias)
        if passthrough:
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dres=None):
        x, gamma, mean, rstd, inv, res_scale = ctx.saved_tensors
        B, S, C = x.shape
        dx = torch.empty_like(x)
        dres_sum = None
        if dres is not None:
            if x.dtype != torch.float32:
                raise PswinError("the residual passthrough of layer_norm_gather needs an fp32 residual stream")
            dres = dres.float().contiguous()
        if ctx.want_res_sum and dres is None:
            raise PswinError("layer_norm_gather(res_bias=...) needs the passthrough output to be used as the shortcut")
        if dy is None:                                   # only the shortcut was used downstream
            if ctx.want_res_sum:
                g = dres if res_scale is None else dres * res_scale[:, None, None]
                dres_sum = colsum(g.reshape(-1, C), owners=ctx.owners[2:])
            return dres, torch.zeros_like(gamma), torch.zeros_like(gamma), None, None, None, None, None, dres_sum, None, None
        dy = dy.contiguous()
        lib = _lib.load()
        ws = torch.empty(lib.pswin_ln_workspace(B * S, C), dtype=torch.float32, device=x.device)
        nseg = 3 if ctx.want_res_sum else 2
        # partial rows only ([dgamma | dbeta | dres_sum] per block); summed by the grouped reduction
        call("pswin_ln_gather_bwd", x, ptr(dy), dtype_code(dy), ptr(inv), ptr(x), dtype_code(x), ptr(mean), ptr(rstd),
             ptr(gamma), ptr(dres), ptr(res_scale), ptr(dres) if ctx.want_res_sum else None, ptr(dx), None, None, ptr(ws),
             B, S, ctx.n_out, C, algo_bytes=B * S * C * (dy.element_size() + (2 if dres is None else 3) * x.element_size()))
        sums = sum_rows(ws, lib.pswin_ln_partial_rows(B * S, C), nseg * C, owners=ctx.owners)
        if ctx.want_res_sum:
            dres_sum = sums[2 * C:]
        # the added rows' gradient: a per-element sum over the batch (one pass, no framework two-pass reduction)
        dadd = (dy.float().sum(0) if B > 1 else dy[0].float()) if ctx.has_add else None
        return dx, sums[:C], sums[C:2 * C], None, None, None, None, None, dres_sum, None, dadd


def layer_norm_gather(x, gamma, beta, eps, wmap=None, inv=None, out_dtype=None, passthrough=False, res_bias=None,
                      res_scale=None, add_rows=None):
    """LayerNorm over the last dim of x [B, S, C], written through a window map (norm1 + shift + pad + window
    partition, HOT:503-513) or in place order (wmap=None: norm2 / output norms).  Padding slots are zero rows.

    passthrough=True returns (y, x'): x' is x itself, to be used for the residual shortcut (x' + f(y)); the gradient
    that flows back into x' is then added to dx INSIDE the LayerNorm backward kernel instead of by a separate
    accumulation pass over the residual stream (one per block half in the reference's autograd graph).

    res_bias (with passthrough): the bias b of the branch x' + scale_b * (f(y) + b) that window_scatter_add(...,
    bias=b, bias_grad_elsewhere=True) adds; its gradient, sum_{b,t} res_scale[b] * grad(x')[b][t], is accumulated by
    the same backward kernel (which reads grad(x') anyway) and returned here."""
    if add_rows is not None:        # + f32 [S, C] rows after the affine (the absolute position encoding): pswin_ln_gather_fwd_add
        return _LayerNormGather.apply(x, gamma, beta, eps, wmap, inv, out_dtype or x.dtype, passthrough, res_bias, res_scale, add_rows)
    return _LayerNormGather.apply(x, gamma, beta, eps, wmap, inv, out_dtype or x.dtype, passthrough, res_bias, res_scale)


# the window gather (or bf16 cast) of window_scatter_add's backward from inside the LayerNorm backward kernel (pswin_ln_gather_bwd_ex) and
# the next block's norm1 + partition from inside the residual add (pswin_scatter_add_ln_fwd_map); off: separate kernels
LN_FUSED_MOVES = _on("ln_fused_moves")


class _ScatterAddLayerNorm(torch.autograd.Function):
    """window_scatter_add + LayerNorm in one forward pass (pswin_scatter_add_ln_fwd[_map]); the backward pass is the LayerNorm backward
    kernel (with the shortcut gradient folded in, as layer_norm_gather(passthrough=True)) which also writes the window gather of
    window_scatter_add's backward (pswin_ln_gather_bwd_ex) -- or, with ln_fused_moves off / fp32 windows, followed by that gather."""

    @staticmethod
    def forward(ctx, win, resid, wmap, inv, scale, bias, gamma, beta, eps, out_dtype, res_bias, res_scale, in_pads, out_inv, out_n, out_pads):
        B, S, C = resid.shape
        if resid.dtype != torch.float32:
            raise PswinError("scatter_add_layer_norm needs an fp32 residual stream")
        win, resid = win.contiguous(), resid.contiguous()
        x1 = torch.empty_like(resid)
        n_y = S if out_inv is None else int(out_n)
        y = torch.empty(B, n_y, C, dtype=out_dtype, device=resid.device)
        mean = torch.empty(B, S, dtype=torch.float32, device=resid.device)
        rstd = torch.empty_like(mean)
        b = None if bias is None else bias.detach().float().contiguous()
        abytes = B * C * (win.shape[1] * win.element_size() + 8 * S + n_y * y.element_size())
        if out_inv is None:
            call("pswin_scatter_add_ln_fwd", win, ptr(win), dtype_code(win), ptr(inv), ptr(resid), ptr(scale), ptr(b), ptr(x1),
                 ptr(gamma), ptr(beta), float(eps), ptr(y), dtype_code(y), ptr(mean), ptr(rstd), B, S, win.shape[1], C, algo_bytes=abytes)
        else:
            call("pswin_scatter_add_ln_fwd_map", win, ptr(win), dtype_code(win), ptr(inv), ptr(resid), ptr(scale), ptr(b), ptr(x1),
                 ptr(gamma), ptr(beta), float(eps), ptr(y), dtype_code(y), ptr(mean), ptr(rstd), B, S, win.shape[1], C, ptr(out_inv), n_y,
                 ptr(out_pads), n_y - S, algo_bytes=abytes, timed_as="pswin_scatter_add_ln_fwd")
        ctx.save_for_backward(x1, gamma, mean, rstd, wmap, scale, res_scale, inv, in_pads, out_inv)
        ctx.win_dtype, ctx.want_res_sum, ctx.n_in, ctx.n_y = win.dtype, res_bias is not None, win.shape[1], n_y
        ctx.owners = (gamma, beta, res_bias)
        return y, x1

    @staticmethod
    def backward(ctx, dy, dres):
        x1, gamma, mean, rstd, wmap, scale, res_scale, inv, in_pads, out_inv = ctx.saved_tensors
        B, S, C = x1.shape
        if dy is None:
            raise PswinError("scatter_add_layer_norm: the normalised output must be used")
        if ctx.want_res_sum and dres is None:
            raise PswinError("scatter_add_layer_norm(res_bias=...) needs the second output to be used as the shortcut")
        dy = dy.contiguous()
        dres = None if dres is None else dres.float().contiguous()
        dx1 = torch.empty_like(x1)
        lib = _lib.load()
        ws = torch.empty(lib.pswin_ln_workspace(B * S, C), dtype=torch.float32, device=x1.device)
        nseg = 3 if ctx.want_res_sum else 2
        n_pads = ctx.n_in - S
        fused = (LN_FUSED_MOVES and ctx.win_dtype == torch.bfloat16 and C <= 1024 and (inv is not None or n_pads == 0)
                 and (n_pads == 0 or in_pads is not None))
        abytes = B * S * C * (dy.element_size() + (2 if dres is None else 3) * 4)
        if fused:                                            # dwin = scale_b * dx1 through the window map, from the same kernel
            dwin = torch.empty(B, ctx.n_in, C, dtype=torch.bfloat16, device=x1.device)
            call("pswin_ln_gather_bwd_ex", x1, ptr(dy), dtype_code(dy), ptr(out_inv), ptr(x1), dtype_code(x1), ptr(mean), ptr(rstd),
                 ptr(gamma), ptr(dres), ptr(res_scale), ptr(dres) if ctx.want_res_sum else None, ptr(dx1), None, None, ptr(ws),
                 B, S, ctx.n_y, C, ptr(dwin), ptr(inv), ctx.n_in, ptr(scale), ptr(in_pads), n_pads,
                 algo_bytes=abytes + B * ctx.n_in * C * 2, timed_as="pswin_ln_gather_bwd")
        else:
            call("pswin_ln_gather_bwd", x1, ptr(dy), dtype_code(dy), ptr(out_inv), ptr(x1), dtype_code(x1), ptr(mean), ptr(rstd),
                 ptr(gamma), ptr(dres), ptr(res_scale), ptr(dres) if ctx.want_res_sum else None, ptr(dx1), None, None, ptr(ws),
                 B, S, ctx.n_y, C, algo_bytes=abytes)
        sums = sum_rows(ws, lib.pswin_ln_partial_rows(B * S, C), nseg * C, owners=ctx.owners)
        dres_sum = sums[2 * C:] if ctx.want_res_sum else None
        if not fused:
            dwin = _gather_raw(dx1, wmap, scale, wmap.numel(), ctx.win_dtype)      # window_scatter_add's backward
        return dwin, dx1, None, None, None, None, sums[:C], sums[C:2 * C], None, None, dres_sum, None, None, None, None, None


def scatter_add_layer_norm(win, resid, wmap, inv, scale, bias, gamma, beta, eps, out_dtype=None, res_bias=None,
                           res_scale=None, in_pads=None, out=None):
    """(y, x1) with x1 = resid + scale_b * (window_reverse(win) + bias) and y = LayerNorm(x1): window_scatter_add(...,
    bias_grad_elsewhere=True) followed by layer_norm_gather(x1, passthrough=True, res_bias=..., res_scale=...) as ONE
    forward kernel (the shortcut sum is not re-read by a LayerNorm kernel).  x1 is the tensor to use for the next
    shortcut.  The gradient of `bias` is not returned here (it comes from the LayerNorm that produced `resid` with
    res_bias=bias); res_bias / res_scale as in layer_norm_gather.
    inv=None: `win` is in token order (wmap: the identity map).  in_pads: window_pads of the map `win` is laid out by (lets the backward
    kernel write the gathered gradient itself).  out=(out_inv, n_out, out_pads): y is written through the token -> slot map out_inv into
    [B, n_out, C] with zero rows at out_pads -- the NEXT block's norm1 + shift + pad + window partition (layer_norm_gather(x1, ..., wmap,
    inv)) fused into this pass."""
    out_inv, out_n, out_pads = out if out is not None else (None, 0, None)
    return _ScatterAddLayerNorm.apply(win, resid, wmap, inv, scale, bias, gamma, beta, eps, out_dtype or resid.dtype,
                                      res_bias, res_scale, in_pads, out_inv, out_n, out_pads)


class _LayerNormNCHW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, H, W, passthrough):
        B, S, C = x.shape
        x = x.contiguous()
        y = torch.empty(B, C, H, W, dtype=torch.float32, device=x.device)
        mean = torch.empty(B, S, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        call("pswin_ln_nchw_fwd", x, ptr(x), ptr(gamma), ptr(beta), float(eps), ptr(y), ptr(mean), ptr(rstd), B, S, C,
             algo_bytes=2 * x.numel() * 4)
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.owners = (gamma, beta)
        if passthrough:
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dres=None):
        x, gamma, mean, rstd = ctx.saved_tensors
        B, S, C = x.shape
        if dy is None:
            return dres, torch.zeros_like(gamma), torch.zeros_like(gamma), None, None, None, None
        dy = dy.float().contiguous()
        if dres is not None:
            dres = dres.float().contiguous()
        dx = torch.empty_like(x)
        lib = _lib.load()
        ws = torch.empty(lib.pswin_ln_workspace(B * S, C), dtype=torch.float32, device=x.device)
        call("pswin_ln_nchw_bwd", x, ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(dres), ptr(dx), None, None,
             ptr(ws), B, S, C, algo_bytes=(3 if dres is None else 4) * x.numel() * 4)
        sums = sum_rows(ws, lib.pswin_ln_partial_rows(B * S, C), 2 * C, owners=ctx.owners)
        return dx, sums[:C], sums[C:], None, None, None, None


class _ScatterAddLayerNormNCHW(torch.autograd.Function):
    """The end of a stage in one autograd node and one forward kernel (pswin_scatter_add_ln_nchw_fwd): x = resid + scale_b * (y + bias)
    (the closing MLP branch of the last block, HOT:536) and the output norm of x written as NCHW (HOT:975-977).
    Returns (normed NCHW map, x).  Backward: ONE pswin_ln_nchw_bwd_ex launch yields d(resid) (with the gradient that reaches x from the
    next stage folded in, as layer_norm_nchw(passthrough=True)) AND d(y) = bf16(scale_b * dx) -- the cast that window_scatter_add's
    backward otherwise runs as a pass of its own.  The bias gradient is obtained elsewhere (norm2's backward, res_bias)."""

    @staticmethod
    def forward(ctx, y, resid, scale, bias, gamma, beta, eps, H, W):
        B, S, C = resid.shape
        b = None if bias is None else bias.detach().float().contiguous()
        y, resid = y.contiguous(), resid.contiguous()
        x = torch.empty_like(resid)
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=x.device)
        mean = torch.empty(B, S, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        call("pswin_scatter_add_ln_nchw_fwd", x, ptr(y), ptr(resid), ptr(scale), ptr(b), ptr(x), ptr(gamma), ptr(beta), float(eps),
             ptr(out), ptr(mean), ptr(rstd), B, S, C, timed_as="pswin_ln_nchw_fwd", algo_bytes=x.numel() * (2 + 3 * 4))
        ctx.save_for_backward(x, gamma, mean, rstd, scale)
        ctx.owners = (gamma, beta)
        ctx.y_dtype = y.dtype
        return out, x

    @staticmethod
    def backward(ctx, dout, dres):
        x, gamma, mean, rstd, scale = ctx.saved_tensors
        B, S, C = x.shape
        if dout is None:                                  # only the residual stream was used downstream
            dx = dres.float().contiguous()
            dy = _gather_raw(dx, identity_map(S, x.device), scale, S, ctx.y_dtype)
            return dy, dx, None, None, torch.zeros_like(gamma), torch.zeros_like(gamma), None, None, None
        dout = dout.float().contiguous()
        if dres is not None:
            dres = dres.float().contiguous()
        dx = torch.empty_like(x)
        ex = torch.empty(B, S, C, dtype=torch.bfloat16, device=x.device)
        lib = _lib.load()
        ws = torch.empty(lib.pswin_ln_workspace(B * S, C), dtype=torch.float32, device=x.device)
        call("pswin_ln_nchw_bwd_ex", x, ptr(dout), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(dres), ptr(dx), None, None,
             ptr(ws), ptr(ex), ptr(scale), B, S, C, timed_as="pswin_ln_nchw_bwd",
             algo_bytes=(3 if dres is None else 4) * x.numel() * 4 + 2 * x.numel())
        sums = sum_rows(ws, lib.pswin_ln_partial_rows(B * S, C), 2 * C, owners=ctx.owners)
        return ex.to(ctx.y_dtype), dx, None, None, sums[:C], sums[C:], None, None, None


def scatter_add_layer_norm_nchw_supported(y, resid):
    """bf16 branch rows, fp32 residual stream, a shape the NCHW LayerNorm kernels tile"""
    return (LN_FUSED_MOVES and y.dtype == torch.bfloat16 and resid.dtype == torch.float32 and y.shape == resid.shape
            and bool(_lib.load().pswin_ln_nchw_supported(resid.shape[1], resid.shape[2])))


def scatter_add_layer_norm_nchw(y, resid, scale, bias, gamma, beta, eps, H, W):
    """(LayerNorm_NCHW(x), x) with x = resid + scale_b * (y + bias): see _ScatterAddLayerNormNCHW"""
    return _ScatterAddLayerNormNCHW.apply(y, resid, scale, bias, gamma, beta, eps, H, W)


def layer_norm_nchw(x, gamma, beta, eps, H, W, passthrough=False):
    """LayerNorm over the channels of x [B, H*W, C] (fp32) returned as a contiguous NCHW map [B, C, H, W]: the output
    norms of the backbone (HOT:975-977) without the separate transpose pass, forward and backward.  Falls back to
    layer_norm_gather + permute when the shape does not fit the kernel's tiling."""
    B, S, C = x.shape
    if x.dtype != torch.float32 or not _lib.load().pswin_ln_nchw_supported(S, C):
        out = layer_norm_gather(x, gamma, beta, eps, passthrough=passthrough)
        y, x2 = out if passthrough else (out, None)
        y = y.float().view(B, H, W, C).permute(0, 3, 1, 2).contiguous()
        return (y, x2) if passthrough else y
    return _LayerNormNCHW.apply(x, gamma, beta, eps, H, W, passthrough)


class _LayerNormPatchMerge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, H, W, out_dtype):
        B, S, C = x.shape
        x = x.contiguous()
        H2, W2 = (H + 1) // 2, (W + 1) // 2
        y = torch.empty(B, H2 * W2, 4 * C, dtype=out_dtype, device=x.device)
        mean = torch.empty(B, H2 * W2, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        call("pswin_ln_patch_merge_fwd", x, ptr(x), dtype_code(x), ptr(gamma), ptr(beta), float(eps), ptr(y),
             dtype_code(y), ptr(mean), ptr(rstd), B, H, W, C)
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.owners = (gamma, beta)
        ctx.geom = (H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        B, S, C = x.shape
        H, W = ctx.geom
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        rows = B * ((H + 1) // 2) * ((W + 1) // 2)
        lib = _lib.load()
        ws = torch.empty(lib.pswin_ln_workspace(rows, 4 * C), dtype=torch.float32, device=x.device)
        call("pswin_ln_patch_merge_bwd", x, ptr(dy), dtype_code(dy), ptr(x), dtype_code(x), ptr(mean), ptr(rstd),
             ptr(gamma), ptr(dx), None, None, ptr(ws), B, H, W, C)
        sums = sum_rows(ws, lib.pswin_ln_partial_rows(rows, 4 * C), 8 * C, owners=ctx.owners)
        return dx, sums[:4 * C], sums[4 * C:], None, None, None, None


def layer_norm_patch_merge(x, gamma, beta, eps, H, W, out_dtype=None):
    """PatchMerging's pad + 2x2 strided gather + concat + LayerNorm(4C) (HOT:563-574) in one kernel."""
    return _LayerNormPatchMerge.apply(x, gamma, beta, eps, H, W, out_dtype or x.dtype)


class _BatchNormReLU(torch.autograd.Function):
    """nn.BatchNorm2d (batch or running statistics) + ReLU on a channels-last NCHW tensor (HOT:742-748)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, eps, momentum, train, pre_bias):
        N, C, H, W = y.shape
        rows = y.permute(0, 2, 3, 1)
        assert rows.is_contiguous(), "BatchNorm+ReLU kernel expects a channels-last activation"
        M = N * H * W
        z = torch.empty_like(y)                                     # preserves the channels-last strides
        mean = torch.empty(C, dtype=torch.float32, device=y.device)
        rstd = torch.empty_like(mean)
        ws = torch.empty(_lib.load().pswin_bn_workspace(C), dtype=torch.float32, device=y.device)
        call("pswin_bn_relu_fwd", y, ptr(y), dtype_code(y), ptr(gamma), ptr(beta), ptr(pre_bias), float(eps), float(momentum),
             int(train), ptr(running_mean), ptr(running_var), ptr(z), ptr(mean), ptr(rstd), ptr(ws), M, C)
        ctx.save_for_backward(y, gamma, beta, mean, rstd)
        ctx.train = bool(train)
        ctx.pre_bias_shape = None if pre_bias is None else pre_bias.shape
        return z

    @staticmethod
    def backward(ctx, dz):
        y, gamma, beta, mean, rstd = ctx.saved_tensors
        N, C, H, W = y.shape
        dz = dz.contiguous(memory_format=torch.channels_last)
        dy = torch.empty_like(y)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        ws = torch.empty(_lib.load().pswin_bn_workspace(C), dtype=torch.float32, device=y.device)
        call("pswin_bn_relu_bwd", y, ptr(dz), ptr(y), dtype_code(y), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd),
             int(ctx.train), ptr(dy), ptr(dgamma), ptr(dbeta), ptr(ws), N * H * W, C)
        # a constant added in front of batch-statistics BN has an exactly zero gradient; in eval mode it is sum(dy)
        dpre = None
        if ctx.pre_bias_shape is not None:
            dpre = torch.zeros(ctx.pre_bias_shape, dtype=torch.float32, device=y.device) if ctx.train else \
                colsum(dy.permute(0, 2, 3, 1).reshape(-1, C))
        return dy, dgamma, dbeta, None, None, None, None, None, dpre


def batch_norm_relu(y, bn, training, pre_bias=None):
    """ReLU(BatchNorm2d(y + pre_bias)) for a channels-last y with the parameters / buffers of the nn.BatchNorm2d
    module `bn`; pre_bias (the convolution bias) is never materialised on the activation."""
    use_batch = training or bn.running_mean is None
    counted = training and bn.num_batches_tracked is not None
    momentum = bn.momentum
    if momentum is None:                                  # nn.BatchNorm2d's cumulative average: 1 / (batches seen, this one included)
        momentum = 1.0 / (float(bn.num_batches_tracked) + 1.0) if counted else 0.0
    z = _BatchNormReLU.apply(y, bn.weight, bn.bias, bn.running_mean if (training or not use_batch) else None,
                             bn.running_var if (training or not use_batch) else None, bn.eps, momentum, use_batch,
                             pre_bias)
    if counted:                                           # only a batch the kernel accepted is counted
        bn.num_batches_tracked.add_(1)
    return z


def colsum(x2d, zero_cols=None, owners=()):
    """fp32 column sums of a [M, N] matrix (N % 8 == 0): bias gradients and split-K partial reductions.
    zero_cols=(lo, hi): columns known to sum to zero (not read on the large-matrix path; see pswin_colsum_skip).
    owners: see sum_rows."""
    x2d = x2d.contiguous()
    M, N = x2d.shape
    if M <= 4096:
        return sum_rows(x2d, M, N, owners=owners)
    n_ws = _lib.load().pswin_colsum_workspace(M, N, dtype_code(x2d))
    ws = torch.empty(n_ws, dtype=torch.float32, device=x2d.device)
    if zero_cols is None:
        call("pswin_colsum", x2d, ptr(x2d), dtype_code(x2d), M, N, None, ptr(ws))      # first stage: partial rows
    else:
        call("pswin_colsum_skip", x2d, ptr(x2d), dtype_code(x2d), M, N, int(zero_cols[0]), int(zero_cols[1]), ptr(ws))
    return sum_rows(ws, n_ws // N, N, owners=owners)


def colsum_channels(dy):
    """f32 [C]: the sum of an NCHW gradient over batch and pixels (a convolution's bias gradient) as a fixed-order column sum of its
    channels-last rows, for ANY channel count: rows narrower than / not a multiple of 8 columns (the RPN's 3- and 12-channel heads)
    are zero-padded to the next multiple of 8 first, so that no framework two-pass reduction -- the kind that returns stale results
    from the second replay of a captured hipGraph -- is left on the path."""
    C = dy.shape[1]
    if dy.dtype not in (torch.bfloat16, torch.float32):
        dy = dy.float()
    rows = dy.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1).reshape(-1, C)
    if C % 8:
        rows = F.pad(rows, (0, 8 - C % 8))
    return colsum(rows)[:C]


def gemm_nt_supported(x2d, n_out):
    """bf16 rows x [n_out, K] weight on the tiled HIP GEMM (pswin_gemm_nt): the Linear layers of stages 1-3"""
    return (x2d.dtype == torch.bfloat16 and x2d.is_cuda and x2d.dim() == 2
            and bool(_lib.load().pswin_gemm_nt_supported(x2d.shape[0], x2d.shape[1], n_out)))


# the row tiles each entry point of the tiled GEMM accepts (csrc/pswin_gemm_nt.hip): 96-row tiles exist for the plain epilogue only
GEMM_NT_TILES = {"pswin_gemm_nt": (64, 96, 128), "pswin_gemm_nt_f32": (64, 128),
                 "pswin_gemm_nt_gelu_fwd": (64, 128), "pswin_gemm_nt_gelu_bwd": (64, 128)}


def gemm_nt_tile(M, K, N, entry="pswin_gemm_nt", required=False):
    """Row-tile height (one of GEMM_NT_TILES[entry]) with which `entry` computes [M, K] x [N, K]^T, or 0 = leave it to the library.
    required=True: the product has no library counterpart (the fused GELU forms): gemm_nt_rows where the rule would answer 0.
    From profiles/r02_gemm_nt_vs_library.txt (MI355X, PanoSwin-T shapes at batch 8) and the in-step A/Bs of round 4
    (profiles/r04_ab_runs.json: gemm_nt_*): the HIP kernel wins wherever the rows fill the chip (M >= 8192: stages 1-2), on the narrow
    outputs with a short contraction at 4-6 k rows, and wherever 128-row tiles still give every CU two rounds of work (stage 3's qkv / fc1
    at batch 8); 128-row tiles then, or when they make the launch fit the chip ONCE (<= 256 tiles: the kernel's four-stage form,
    csrc/pswin_gemm_nt.hip) while 64-row tiles would not; 96-row tiles where the entry has them and 64-row tiles would spill into a
    second round; 64-row tiles otherwise."""
    rows, t128 = gemm_nt_rows(M, N), -(-M // 128) * (N // 192)
    if (not GEMM_NT or not bool(_lib.load().pswin_gemm_nt_supported(M, K, N))
            or (M < 8192 and not (N <= 768 and K <= 1536) and t128 < 512)):
        return rows if required else 0
    if rows == 64 and 96 in GEMM_NT_TILES[entry]:
        # 64-row tiles that spill into a second, mostly empty round of the 512 tile slots (two workgroups per CU): 96-row tiles in one
        t64, t96 = -(-M // 64) * (N // 192), -(-M // 96) * (N // 192)
        if 512 < t64 <= 768 and t96 <= 512:
            return 96
    return rows


def gemm_nt_rows(M, N):
    """the row-tile height of the tiled GEMM's 64 / 128-row forms for a product that runs on it in any case"""
    t64, t128 = -(-M // 64) * (N // 192), -(-M // 128) * (N // 192)
    if t128 < 512 and t64 > 256 and t128 <= 256:
        return 128
    return 128 if t128 >= 512 else 64


def transpose_weights(pairs):
    """dst = src^T for every (src [R, C], dst [C, R]) pair of contiguous bf16 matrices, one launch (pswin_transpose_jobs)."""
    if not pairs:
        return
    arr = (_lib.TransposeJob * len(pairs))()
    for a, (src, dst) in zip(arr, pairs):
        assert src.dtype == dst.dtype == torch.bfloat16 and src.is_contiguous() and dst.is_contiguous()
        assert dst.shape == (src.shape[1], src.shape[0])
        a.src, a.dst, a.rows, a.cols = src.data_ptr(), dst.data_ptr(), src.shape[0], src.shape[1]
    call("pswin_transpose_jobs", pairs[0][0], ctypes.cast(arr, ctypes.c_void_p), len(pairs))


# the three-stage ring kernel for weight gradients (pswin_gemm_tn_ring, round 3); off: library batched GEMMs
GEMM_TN_RING = _on("gemm_tn_ring")
# partial slabs of the row splits in bf16 (what the library's batched GEMM writes; half the slab traffic), f32 for a single split
GEMM_TN_RING_BF16 = True
# the Linear's bias gradient (column sums of dy) from the weight-gradient launch instead of a pass of its own; off: pswin_colsum
GEMM_TN_RING_BIAS = _on("gemm_tn_ring_bias")


# Weight gradients held back to the end of the backward pass and issued as one launch per tile geometry (pswin_gemm_tn_ring_jobs) when
# the parameter-gradient reductions are deferred too (set_deferred_reductions): a workgroup then contracts GROUPED_WGRAD_ROWS rows
# instead of M / (256 / tiles).  off: one launch per weight gradient, where autograd produces it
GROUPED_WGRAD = _on("grouped_wgrad")
GROUPED_WGRAD_ROWS = 2048                 # swept 1,024 / 2,048 / 4,096: profiles/r04_ab_runs.json


def grouped_wgrad_splits(M):
    """row splits of one weight gradient inside the grouped launch: about GROUPED_WGRAD_ROWS rows per workgroup, in counts that divide
    over the 8 XCDs (1, 2, 4 or a multiple of 8: the kernel gives a split to 8, 4, 2 XCDs or one, csrc/pswin_gemm_tn.hip)"""
    s = max(1, min(M // 64, (M + GROUPED_WGRAD_ROWS // 2) // GROUPED_WGRAD_ROWS))
    if s >= 6:
        s = max(8, (s + 4) // 8 * 8)
    elif s >= 3:
        s = 4
    return max(1, min(M // 64, s))


def queue_weight_gradient(dy, x, weight, bias, zero_cols, live=None):
    """dW = dy^T x (and the bias gradient, the column sums of dy) through the grouped end-of-pass launch, if this backward pass may
    postpone them (see set_deferred_reductions): returns (dw f32 [N, K], db f32 [N] or None) -- tensors that are FILLED when the pass
    ends -- or None = launch now.  The operands stay referenced by the queue until then.  live: the rows' sample liveness (wgrad_live)."""
    M, N = dy.shape
    K = x.shape[1]
    if not (GROUPED_WGRAD and dy.dtype == torch.bfloat16 and gemm_tn_ring_splits(M, N, K) > 0):
        return None
    q = grad_queue.deferring((weight, bias))              # None as well when deferral is off
    if q is None:
        return None
    splits = grouped_wgrad_splits(M)
    x = x.contiguous()
    slot = grad_slot(weight)
    dev = x.device
    out = slot if slot is not None else torch.empty(N * K, dtype=torch.float32, device=dev)
    if splits == 1:
        part = out                                        # the finished f32 gradient straight from the kernel: nothing to reduce
    else:
        part = torch.empty(splits, N, K, dtype=torch.bfloat16 if GEMM_TN_RING_BF16 else torch.float32, device=dev)
        q.add_reduction(part, splits, N * K, out)
    dbp = db = None
    if bias is not None:
        db = torch.empty(N, dtype=torch.float32, device=dev)
        dbp = db if splits == 1 else torch.empty(splits, N, dtype=torch.float32, device=dev)
        if splits > 1:
            q.add_reduction(dbp, splits, N, db)
        db = db.view(N)                                   # fresh views: see sum_rows
    zlo, zhi = (0, 0) if zero_cols is None else (int(zero_cols[0]), int(zero_cols[1]))
    q.add_weight_gradient(dy, x, part, dbp, splits, zlo, zhi, wgrad_live(live, M, splits))
    return out.view(N, K), db


def gemm_tn_ring_splits(M, N, K):
    """Row splits for pswin_gemm_tn_ring on dy [M, N], x [M, K], or 0 = not for this shape.  ONE rule per configuration, whether the
    product is launched alone or inside the grouped launch (the two modes then run the same arithmetic: the deferred step stays bit-equal
    to the immediate one): about GROUPED_WGRAD_ROWS rows per workgroup by default; with grouped_wgrad disabled the round-3 rule, one
    workgroup per CU and launch."""
    if not GEMM_TN_RING or M < 512 or not bool(_lib.load().pswin_gemm_tn_ring_supported(M, N, K)):
        return 0
    if GROUPED_WGRAD:
        return grouped_wgrad_splits(M)
    return int(_lib.load().pswin_gemm_tn_ring_splits(M, N, K, 0))


def sample_liveness(scale, rows_per_sample, M):
    """The liveness argument (sample_scale f32 [B] contiguous on the device, rows_per_sample) of a kernel over M sample-major rows, or
    None: no factor vector (no DropPath in this pass), the switch is off, or the rows are not B <= 64 whole samples."""
    if scale is None or not SAMPLE_SKIP or rows_per_sample <= 0 or M % rows_per_sample or not 0 < M // rows_per_sample <= 64:
        return None
    if scale.dtype != torch.float32 or scale.numel() != M // rows_per_sample:
        return None
    return scale.detach().contiguous(), int(rows_per_sample)


def wgrad_live_rows_ok(M, splits):
    """the ring kernel keeps the live 64-row slabs of a workgroup's row range in one 64-bit mask (csrc/pswin_gemm_tn.hip)"""
    return splits > 0 and -(-M // splits) <= 64 * 64


def wgrad_live(live, M, splits):
    """`live` if the ring kernel takes it for a weight gradient over M rows in `splits` row ranges, else None"""
    return live if live is not None and wgrad_live_rows_ok(M, splits) else None


def gemm_tn_ring(dy, x, splits, out_dtype=torch.float32, bias_sums=False, zero_cols=None, live=None):
    """[splits, N, K] partial sums of dy^T x over `splits` row ranges (dy [M, N], x [M, K] bf16) in f32 or bf16.
    Roofline bookkeeping: algorithmic bytes = dY and X read once + the f32 gradient written once, 2 (MK + MN) + 4 NK; the
    split partial slabs are an implementation artefact and are reported separately (partial_bytes), never as algorithmic traffic.
    bias_sums=True: also the f32 [splits, N] column sums of dy per row range (the Linear's bias-gradient partials, from the same
    launch; zero_cols=(lo, hi) columns written as zeros) -> (partials, bias partials)."""
    dy, x = dy.contiguous(), x.contiguous()
    M, N = dy.shape
    K = x.shape[1]
    part = torch.empty(splits, N, K, dtype=out_dtype, device=x.device)
    live = wgrad_live(live, M, splits)
    if live is not None:                                  # the one-product entry points take no liveness: a one-entry job table
        dbp = torch.empty(splits, N, dtype=torch.float32, device=x.device) if bias_sums else None
        zlo, zhi = (0, 0) if zero_cols is None else (int(zero_cols[0]), int(zero_cols[1]))
        grad_queue._launch_wgrads([grad_queue.weight_grad(dy, x, part, dbp, int(splits), zlo, zhi, live)])
        return (part, dbp) if bias_sums else part
    if not bias_sums:
        call("pswin_gemm_tn_ring", x, ptr(dy), ptr(x), ptr(part), dtype_code(part), M, N, K, int(splits),
             algo_bytes=2 * (M * K + M * N) + 4 * N * K, algo_flops=2 * M * K * N, partial_bytes=part.element_size() * splits * N * K)
        return part
    dbp = torch.empty(splits, N, dtype=torch.float32, device=x.device)
    zlo, zhi = (0, 0) if zero_cols is None else (int(zero_cols[0]), int(zero_cols[1]))
    call("pswin_gemm_tn_ring_bias", x, ptr(dy), ptr(x), ptr(part), dtype_code(part), ptr(dbp), zlo, zhi, M, N, K, int(splits),
         algo_bytes=2 * (M * K + M * N) + 4 * N * K, algo_flops=2 * M * K * N, timed_as="pswin_gemm_tn_ring",
         partial_bytes=part.element_size() * splits * N * K)
    return part, dbp


def gemm_nt(x2d, w, bias=None, tile_m=0, out_f32=False, live=None):
    """y = x2d @ w^T (+ bias): x2d [M, K] bf16, w [N, K] bf16, bias f32 [N] or None -> [M, N] bf16 (out_f32: f32, pswin_gemm_nt_f32).
    live = (sample_scale, rows_per_sample), bf16 result only: the rows of dead samples are not read and come out as zeros
    (pswin_gemm_nt_live; rows_per_sample must be a multiple of tile_m)."""
    x2d, w = x2d.contiguous(), w.contiguous()
    M, K = x2d.shape
    N = w.shape[0]
    b = None if bias is None else bias.detach().float().contiguous()
    if out_f32:
        y = torch.empty(M, N, dtype=torch.float32, device=x2d.device)
        call("pswin_gemm_nt_f32", x2d, ptr(x2d), ptr(w), ptr(b), ptr(y), M, K, N, int(tile_m), timed_as="pswin_gemm_nt",
             algo_bytes=2 * (M * K + N * K) + 4 * M * N, algo_flops=2 * M * K * N)
        return y
    y = torch.empty(M, N, dtype=torch.bfloat16, device=x2d.device)
    if live is not None:                                  # (booked as the full problem, like every launch that skips dead samples)
        call("pswin_gemm_nt_live", x2d, ptr(x2d), ptr(w), ptr(b), ptr(y), M, K, N, int(tile_m), ptr(live[0]), live[1],
             timed_as="pswin_gemm_nt", algo_bytes=2 * (M * K + M * N + N * K), algo_flops=2 * M * K * N)
        return y
    call("pswin_gemm_nt", x2d, ptr(x2d), ptr(w), ptr(b), ptr(y), M, K, N, int(tile_m),
         algo_bytes=2 * (M * K + M * N + N * K), algo_flops=2 * M * K * N)
    return y


def rows_addressable(M, width):
    """The streaming kernels address their row operands through 32-bit buffer offsets: M rows of `width` bf16 elements must stay below
    the 0xFFFFFF00 sentinel (the launchers return PSWIN_ERR_ARG otherwise -- the *_supported predicates below check it first, so an
    oversize batch falls through to the next path instead of raising)."""
    return M * width * 2 < 0xFFFFFF00


def skinny_gemm_shape_ok(M, K, N):
    return M >= 4096 and rows_addressable(M, max(K, N)) and bool(_lib.load().pswin_gemm_skinny_supported(K, N))


def skinny_gemm_supported(x2d, n_out):
    """bf16 rows x a small weight: the shapes pswin_gemm_skinny is instantiated for (stage-0 projections, stage-1 proj)"""
    return x2d.dtype == torch.bfloat16 and x2d.is_cuda and skinny_gemm_shape_ok(x2d.shape[0], x2d.shape[1], n_out)


def skinny_gemm(x2d, w, bias=None, transpose_w=False):
    """y = x2d @ W^T (+ bias) through the streaming HIP GEMM (weights resident in LDS).  transpose_w=False: w is the
    nn.Linear weight [N, K]; transpose_w=True: w is [K, N] and y = x2d @ w (the data gradient with the same weight)."""
    x2d = x2d.contiguous()
    w = w.contiguous()
    M, K = x2d.shape
    N = w.shape[1] if transpose_w else w.shape[0]
    y = torch.empty(M, N, dtype=torch.bfloat16, device=x2d.device)
    b = None if bias is None else bias.detach().float().contiguous()
    call("pswin_gemm_skinny", x2d, ptr(x2d), ptr(w), ptr(b), ptr(y), M, K, N, int(transpose_w),
         algo_bytes=2 * M * (K + N))
    return y


def linear_product(x2d, wb, bias=None, b_lp=None, out_f32=False, skinny=False, live=None):
    """y = x2d @ wb^T (+ bias) on the first kernel that takes the shape: the streaming GEMM (skinny=True; the stage-0 shapes), the
    tiled HIP GEMM where gemm_nt_tile picks it (stages 1-3), else the library GEMM (with b_lp, bias's bf16 copy, if given).
    out_f32: an f32 result where the tiled HIP GEMM runs (its epilogue writes it), a cast of the bf16 result elsewhere."""
    M, K = x2d.shape
    N = wb.shape[0]
    if skinny and skinny_gemm_supported(x2d, N):
        y = skinny_gemm(x2d, wb, bias)
        return y.float() if out_f32 else y
    tile = gemm_nt_tile(M, K, N, "pswin_gemm_nt_f32" if out_f32 else "pswin_gemm_nt") if x2d.dtype == torch.bfloat16 else 0
    if tile:
        return gemm_nt(x2d, wb, bias, tile, out_f32=out_f32, live=live)
    if live is not None:
        raise PswinError("linear_product: sample liveness needs the tiled HIP GEMM (mlp_sample_skip decides that before the call)")
    bb = None if bias is None else (b_lp if b_lp is not None else bias.to(x2d.dtype))
    with _lib.timed("lib_gemm_fwd", 2 * (M * K + M * N + N * K), 2 * M * K * N):
        y = F.linear(x2d, wb, bb)
    return y.float() if out_f32 else y


def _pick_split(M, n_tiles):
    """Number of K-splits for a weight-gradient GEMM with contraction length M and n_tiles output tiles: a divisor
    of M that gives hipBLASLt about a thousand independent tiles while each split keeps >= 512 rows."""
    want = max(1, min(M // 512, -(-1024 // n_tiles)))
    best = 1
    for c in range(1, min(M, 4 * want) + 1):
        if M % c == 0 and abs(c - want) < abs(best - want):
            best = c
    return best


class _LinearSplitK(torch.autograd.Function):
    """y = x W^T + b with bf16 operands and fp32 master parameters.

    Forward and dX are plain hipBLASLt GEMMs.  dW = dY^T X contracts over up to 275k window tokens into an output of
    a few dozen tiles, which a single GEMM launch maps onto a few dozen workgroups (measured 470-535 us for the
    stage-0 shapes on MI355X against a 20-50 us HBM floor); it is issued as a batched GEMM over row chunks (an
    explicit split-K, 55-75 us) whose fp32 partial sum also removes the bf16 -> fp32 gradient cast."""

    @staticmethod
    def forward(ctx, x, weight, bias, w_lp, b_lp, zero_bias_cols=None, w_lp_t=None, out_f32=False, live=None):
        # w_lp / b_lp: this step's bf16 copies of the fp32 master parameters (refreshed by ONE multi-tensor cast per
        # forward, see SimplePanoSwinTransformer._refresh_lowp); gradients go to the fp32 masters.
        wb = w_lp if w_lp is not None else weight.to(x.dtype)
        ctx.save_for_backward(x, wb, w_lp_t)            # w_lp_t: this step's [K, N] copy of wb (data gradient on pswin_gemm_nt) or None
        ctx.has_bias = bias is not None
        ctx.zero_bias_cols = zero_bias_cols
        ctx.weight, ctx.bias = weight, bias                 # for grad_slot / owners: dW may be summed straight into its flat slot
        ctx.live = live                                     # sample liveness of the rows: the weight gradient leaves dead samples out
        return linear_product(x, wb, bias, b_lp, out_f32, skinny=True)

    @staticmethod
    def backward(ctx, dy):
        x, wb, wbt = ctx.saved_tensors
        if dy.dtype != x.dtype:                             # out_f32: the gradient arrives in fp32
            dy = dy.to(x.dtype)
        dx, dw, db = linear_backward(x, wb, dy, ctx.weight, ctx.bias if ctx.has_bias else None, ctx.zero_bias_cols,
                                     ctx.needs_input_grad[0], wbt, wgrad_live=ctx.live)
        return dx, dw, db, None, None, None, None, None, None


def linear_backward(x, wb, dy, weight, bias, zero_bias_cols, need_dx, wbt=None, wgrad_live=None, dgrad_live=None):
    """Gradients of y = x wb^T (+ bias) for bf16 rows x [M, K], wb [N, K]: (dx or None, dW f32 [N, K], dbias f32 [N] or
    None).  weight / bias: the fp32 master parameters the gradients belong to (grad_slot / deferred reductions).
    wbt: wb^T [K, N] if the caller keeps one (dx then runs on pswin_gemm_nt where that is the faster kernel).
    wgrad_live / dgrad_live: the rows' sample liveness for the weight gradient / the data gradient (the latter only where the caller
    knows that dx runs on the tiled GEMM with whole tiles per sample: mlp_sample_skip)."""
    dy = dy.contiguous()
    M, N = dy.shape
    K = x.shape[1]
    dx = None
    if need_dx:
        # data gradient with the streaming kernel (weight transposed while it is staged) where that beats the library:
        # the three stage-0 shapes with 96 output columns and the stage-0 fc2 (96 -> 384 columns)
        tile = gemm_nt_tile(M, N, K) if (wbt is not None and dy.dtype == torch.bfloat16) else 0
        if K == 96 and N in (96, 288, 384) and skinny_gemm_supported(dy, K):
            dx = skinny_gemm(dy, wb, None, transpose_w=True)
        elif tile:
            dx = gemm_nt(dy, wbt, None, tile, live=dgrad_live)
        else:
            if dgrad_live is not None:
                raise PswinError("linear_backward: sample liveness of the data gradient needs the tiled HIP GEMM")
            with _lib.timed("lib_gemm_dgrad", 2 * (M * K + M * N + N * K), 2 * M * K * N):
                dx = dy @ wb
    queued = queue_weight_gradient(dy, x, weight, bias, zero_bias_cols, wgrad_live)
    return (dx, *(queued if queued is not None else weight_gradient(dy, x, weight, bias, zero_bias_cols, wgrad_live)))


def weight_gradient(dy, x, weight, bias=None, zero_bias_cols=None, live=None):
    """dW = dy^T x (f32 [N, K]) and the bias gradient (f32 [N] or None), launched now: the ring kernel (the bias gradient rides along),
    else the library's batched GEMM over row chunks or a plain GEMM; a split's partial slabs summed by sum_rows.  weight / bias: the
    fp32 master parameters the gradients belong to (grad_slot / deferred reductions)."""
    M, N = dy.shape
    K = x.shape[1]
    sp = 0
    rs = gemm_tn_ring_splits(M, N, K) if dy.dtype == torch.bfloat16 else 0
    db_part = None
    if rs:                                                   # the ring-pipelined HIP weight-gradient kernel; the bias gradient rides along
        pdt = torch.bfloat16 if (GEMM_TN_RING_BF16 and rs > 1) else torch.float32
        if bias is not None and GEMM_TN_RING_BIAS:
            part, db_part = gemm_tn_ring(dy, x, rs, pdt, bias_sums=True, zero_cols=zero_bias_cols, live=live)
        else:
            part = gemm_tn_ring(dy, x, rs, pdt, live=live)
        ch, sp = rs, rs
    else:
        ch = _pick_split(M, -(-N // 64) * -(-K // 64))
        with _lib.timed("lib_gemm_wgrad", 2 * (M * K + M * N) + 4 * N * K, 2 * M * K * N):
            if ch > 1:
                part = torch.bmm(dy.view(ch, M // ch, N).transpose(1, 2), x.view(ch, M // ch, K))
            else:
                dw = (dy.t() @ x).float()
    if ch > 1:
        dw = sum_rows(part, ch, N * K, out=grad_slot(weight), owners=(weight,)).view(N, K)
    else:
        if sp:
            dw = part.view(N, K).float()
        flush_if_pending((weight,))                          # an immediate gradient behind a postponed one of the same weight
    if db_part is not None:
        db = sum_rows(db_part, db_part.shape[0], N, owners=(bias,))
    else:
        db = colsum(dy, zero_bias_cols, owners=(bias,)) if bias is not None else None
    return dw, db


def linear(x, lin, cd, use_bias=True, zero_bias_cols=None, out_f32=False, live=None):
    """nn.Linear on rows.  fp32: F.linear (parity path).  bf16: split-K weight gradient, fp32 parameter gradients.
    use_bias=False: the caller applies lin.bias itself (fused into the next row kernel).  zero_bias_cols=(lo, hi): output
    columns whose gradient sums to zero over the rows (their bias gradient is zero; the column sum skips them).
    live: the rows' sample liveness (sample_liveness) when the gradient of dropped samples' rows is an exact zero (the Linear sits inside a
    DropPath branch): the weight gradient leaves those rows out."""
    if cd == torch.float32:
        return F.linear(x.float(), lin.weight, lin.bias if use_bias else None)
    shp = x.shape
    w_lp, b_lp, w_lp_t = _lowp(lin)
    return _LinearSplitK.apply(x.to(cd).reshape(-1, shp[-1]), lin.weight, lin.bias if use_bias else None, w_lp,
                               b_lp if use_bias else None, zero_bias_cols, w_lp_t, out_f32,
                               live).view(*shp[:-1], lin.weight.shape[0])


def _lowp(lin):
    """(weight, bias, transposed weight): this step's bf16 shadows of an nn.Linear's fp32 parameters (SimplePanoSwinTransformer.
    _refresh_lowp / _refresh_transposed), None where the Linear has none"""
    w_lp, b_lp = lin.__dict__.get("_lowp") or (None, None)
    return w_lp, b_lp, lin.__dict__.get("_lowp_t")


class _Fc1Gelu(torch.autograd.Function):
    """h = gelu(x W1^T + b1) for the stage-0 Mlp in ONE streaming pass (pswin_fc1_gelu_fwd); the backward pass recomputes
    the pre-activation (K = 96) instead of storing it: dy = dh gelu'(.), db1 = column sums of dy, dx = dy W1 (streaming
    GEMM), dW1 = dy^T x (library batched GEMM over row chunks + fixed-order column sum)."""

    @staticmethod
    def forward(ctx, x, weight, bias, w_lp):
        wb = w_lp if w_lp is not None else weight.to(x.dtype)
        x = x.contiguous()
        M, K = x.shape
        N = wb.shape[0]
        h = torch.empty(M, N, dtype=x.dtype, device=x.device)
        b = bias.detach().float().contiguous()
        call("pswin_fc1_gelu_fwd", x, ptr(x), ptr(wb), ptr(b), ptr(h), M, K, N, algo_bytes=2 * M * (K + N))
        ctx.save_for_backward(x, wb, b)
        ctx.weight, ctx.bias = weight, bias
        return h

    @staticmethod
    def backward(ctx, dh):
        x, wb, b = ctx.saved_tensors
        M, K = x.shape
        N = wb.shape[0]
        dh = dh.to(x.dtype).contiguous()
        dy = torch.empty_like(dh)
        lib = _lib.load()
        ws = torch.empty(lib.pswin_fc1_gelu_workspace(N), dtype=torch.float32, device=x.device)
        call("pswin_fc1_gelu_bwd", x, ptr(x), ptr(wb), ptr(b), ptr(dh), ptr(dy), None, ptr(ws), M, K, N,
             algo_bytes=2 * M * (K + 2 * N))
        db = sum_rows(ws, lib.pswin_fc1_gelu_partial_rows(M), N, owners=(ctx.bias,))
        dx = skinny_gemm(dy, wb, None, transpose_w=True) if ctx.needs_input_grad[0] else None
        dw, _ = weight_gradient(dy, x, ctx.weight)               # launched here, never queued for the grouped end-of-pass launch
        return dx, dw, db, None


class _Mlp0(torch.autograd.Function):
    """fc2_nobias(gelu(fc1(x))) of the stage-0 Mlp (HOT:50-58, C = 96) as one autograd node.  Forward: pswin_fc1_gelu_fwd (h is kept,
    the pre-activation is not) + the streaming GEMM.  Backward: g = (dy W2) * gelu'(x W1^T + b1) in ONE pass (pswin_mlp0_bwd: fc2's
    data gradient never reaches memory), then dx = g W1 (streaming GEMM), dW1 = g^T x and dW2 = dy^T h (ring kernel)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, w1_lp, w2_lp):
        x = x.contiguous()
        w1b = (w1_lp if w1_lp is not None else w1.to(x.dtype)).contiguous()
        w2b = (w2_lp if w2_lp is not None else w2.to(x.dtype)).contiguous()
        M, K = x.shape
        N = w1b.shape[0]
        h = torch.empty(M, N, dtype=x.dtype, device=x.device)
        b = b1.detach().float().contiguous()
        if MLP0_FUSED_FWD:                                   # both products in one pass: h is written once and not read back
            y = torch.empty(M, K, dtype=x.dtype, device=x.device)
            call("pswin_mlp0_fwd", x, ptr(x), ptr(w1b), ptr(b), ptr(w2b), ptr(h), ptr(y), M, K, N,
                 algo_bytes=2 * M * (2 * K + N), algo_flops=4 * M * K * N)
        else:
            call("pswin_fc1_gelu_fwd", x, ptr(x), ptr(w1b), ptr(b), ptr(h), M, K, N, algo_bytes=2 * M * (K + N))
            y = skinny_gemm(h, w2b, None)
        ctx.save_for_backward(x, w1b, b, h, w2b)
        ctx.params = (w1, b1, w2)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1b, b, h, w2b = ctx.saved_tensors
        w1, b1, w2 = ctx.params
        M, K = x.shape
        N = w1b.shape[0]
        dy = dy.to(x.dtype).contiguous()
        g = torch.empty(M, N, dtype=x.dtype, device=x.device)
        lib = _lib.load()
        ring_bias = GEMM_TN_RING_BIAS and gemm_tn_ring_splits(M, N, K) > 0     # the fc1 weight-gradient launch also sums g's columns
        ws = None
        if not ring_bias:
            rows = lib.pswin_mlp0_bwd_partial_rows(M)
            ws = torch.empty(rows, N, dtype=torch.float32, device=x.device)
        call("pswin_mlp0_bwd", x, ptr(x), ptr(w1b), ptr(b), ptr(dy), ptr(w2b), ptr(g), None, ptr(ws), M, K, N,
             algo_bytes=2 * M * (2 * K + N), algo_flops=4 * M * K * N)
        if ring_bias:
            dx, dw1, db1 = linear_backward(x, w1b, g, w1, b1, None, ctx.needs_input_grad[0])
        else:
            db1 = sum_rows(ws, rows, N, owners=(b1,))
            dx, dw1, _ = linear_backward(x, w1b, g, w1, None, None, ctx.needs_input_grad[0])
        _, dw2, _ = linear_backward(h, w2b, dy, w2, None, None, False)
        return dx, dw1, db1, dw2, None, None


# off: the stage-0 Mlp as fc1 + GELU node and fc2 node (pswin_fc1_gelu_bwd)
MLP0_FUSED = _on("mlp0_fused")
# off: its forward as pswin_fc1_gelu_fwd + the streaming GEMM for fc2
MLP0_FUSED_FWD = _on("mlp0_fused_fwd")


def mlp0_fused_shape_ok(M, C, hidden):
    """pswin_mlp0_fwd / _bwd take [M, C] rows and an [M, hidden] activation: both must be 32-bit addressable (M < ~5.6 M rows at
    hidden = 384: batch 170 at 512 x 1024, batch 42 at 1024 x 2048); larger batches fall through to the unfused path."""
    lib = _lib.load()
    return (M >= 4096 and rows_addressable(M, max(C, hidden)) and bool(lib.pswin_mlp0_bwd_supported(C, hidden))
            and fc1_gelu_shape_ok(M, C, hidden) and skinny_gemm_shape_ok(M, hidden, C))


def mlp0_fused_supported(x2d, hidden):
    return (MLP0_FUSED and x2d.dtype == torch.bfloat16 and x2d.is_cuda and x2d.dim() == 2
            and mlp0_fused_shape_ok(x2d.shape[0], x2d.shape[1], hidden))


def mlp0_fused(x2d, fc1, fc2):
    """fc2_nobias(gelu(fc1(x2d))) for the stage-0 Mlp as one autograd node: see _Mlp0."""
    return _Mlp0.apply(x2d, fc1.weight, fc1.bias, fc2.weight, _lowp(fc1)[0], _lowp(fc2)[0])


def fc1_gelu_shape_ok(M, K, N):
    return M >= 4096 and rows_addressable(M, max(K, N)) and bool(_lib.load().pswin_fc1_gelu_supported(K, N))


def fc1_gelu_supported(x2d, n_out):
    return x2d.dtype == torch.bfloat16 and x2d.is_cuda and fc1_gelu_shape_ok(x2d.shape[0], x2d.shape[1], n_out)


def fc1_gelu(x2d, weight, bias, w_lp=None):
    return _Fc1Gelu.apply(x2d, weight, bias, w_lp)


class _BiasGelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, bias):
        y = y.contiguous()
        M, N = y.numel() // y.shape[-1], y.shape[-1]
        h = torch.empty_like(y)
        b = None if bias is None else bias.detach().float().contiguous()
        call("pswin_bias_gelu_fwd", y, ptr(y), dtype_code(y), ptr(b), ptr(h), M, N, algo_bytes=2 * y.numel() * y.element_size())
        ctx.save_for_backward(y, b)
        ctx.bias = bias
        return h

    @staticmethod
    def backward(ctx, dh):
        y, b = ctx.saved_tensors
        return bias_gelu_backward(y, dh.to(y.dtype).contiguous(), b, ctx.bias)


def bias_gelu_backward(y, dh, b, bias):
    """(dL/dy, the bias gradient f32 [N] or None without b) of h = gelu(y + b) for y, dh [..., N] (pswin_bias_gelu_bwd); b: the f32 bias
    the forward pass added, bias the parameter it came from"""
    M, N = y.numel() // y.shape[-1], y.shape[-1]
    dy = torch.empty_like(y)
    lib = _lib.load()
    ws = torch.empty(lib.pswin_bias_gelu_workspace(M, N), dtype=torch.float32, device=y.device)
    call("pswin_bias_gelu_bwd", y, ptr(dh), ptr(y), dtype_code(y), ptr(b), ptr(dy), None, ptr(ws), M, N,
         algo_bytes=3 * y.numel() * y.element_size())
    return dy, (sum_rows(ws, lib.pswin_bias_gelu_partial_rows(M, N, dtype_code(y)), N, owners=(bias,)) if b is not None else None)


def gelu_data_gradient(dout, wb, wbt, pre, b, b1, live=None):
    """Backward of out = gelu(pre + b) @ wb^T (fc2 without its bias over fc1's bias + GELU) as far as pre: (dL/dpre, fc1's bias gradient
    f32 [N] or None without b).  dout [M, C], wb [C, N], pre [M, N] bf16; b: the f32 bias the forward pass added, b1 its parameter.
    wbt = wb^T: fc2's data gradient, the GELU backward and the bias-gradient partial rows in ONE kernel (pswin_gemm_nt_gelu_bwd);
    None: the library GEMM, then pswin_bias_gelu_bwd."""
    M, N = pre.shape
    C = wb.shape[0]
    if wbt is None:
        with _lib.timed("lib_gemm_dgrad", 2 * (M * N + M * C + N * C), 2 * M * N * C):
            dh = dout @ wb
        return bias_gelu_backward(pre, dh, b, b1)
    tile = gemm_nt_tile(M, C, N, "pswin_gemm_nt_gelu_bwd", required=True)
    dpre = torch.empty_like(pre)
    rows = _lib.load().pswin_gemm_nt_partial_rows(M, tile)
    ws = torch.empty(rows, N, dtype=torch.float32, device=pre.device)
    if live is not None:         # dead samples: zero rows of bias partials, their rows of dpre stay UNWRITTEN (mlp_sample_skip)
        call("pswin_gemm_nt_gelu_bwd_live", pre, ptr(dout), ptr(wbt), ptr(pre), ptr(b), ptr(dpre), ptr(ws), M, C, N, tile, ptr(live[0]), live[1],
             timed_as="pswin_gemm_nt_gelu_bwd", algo_bytes=2 * (M * C + 2 * M * N + N * C), algo_flops=2 * M * N * C)
        return dpre, (sum_rows(ws, rows, N, owners=(b1,)) if b is not None else None)
    call("pswin_gemm_nt_gelu_bwd", pre, ptr(dout), ptr(wbt), ptr(pre), ptr(b), ptr(dpre), ptr(ws), M, C, N, tile,
         algo_bytes=2 * (M * C + 2 * M * N + N * C), algo_flops=2 * M * N * C)
    return dpre, (sum_rows(ws, rows, N, owners=(b1,)) if b is not None else None)


class _BiasGeluLinear(torch.autograd.Function):
    """out = gelu(y + b1) @ W2^T: fc1's bias + nn.GELU followed by fc2 WITHOUT its bias (HOT:50-58; the caller adds fc2's bias with
    the residual).  One function so that the backward pass can run the data gradient of fc2 and the backward of bias + GELU
    in ONE kernel (pswin_gemm_nt_gelu_bwd): dL/dh [M, 4C] is never written or re-read, and the fc1 bias gradient comes
    out of the same epilogue as per-tile column sums."""

    @staticmethod
    def forward(ctx, y, b1, w2, w2_lp, w2_lp_t):
        y = y.contiguous()
        shp = y.shape
        y2 = y.view(-1, shp[-1])
        M, N = y2.shape
        h = torch.empty_like(y2)
        b = None if b1 is None else b1.detach().float().contiguous()
        call("pswin_bias_gelu_fwd", y2, ptr(y2), dtype_code(y2), ptr(b), ptr(h), M, N, algo_bytes=2 * y2.numel() * y2.element_size())
        wb = w2_lp if w2_lp is not None else w2.to(y.dtype)
        out = linear_product(h, wb)
        ctx.save_for_backward(y2, b, h, wb, w2_lp_t)
        ctx.params = (b1, w2)
        return out.view(*shp[:-1], wb.shape[0])

    @staticmethod
    def backward(ctx, dout):
        y2, b, h, wb, wbt = ctx.saved_tensors
        b1, w2 = ctx.params
        M, N = y2.shape
        C = wb.shape[0]
        dout = dout.reshape(M, C).contiguous()
        # fused even in the narrow stage-3 case the plain rule leaves to the library
        fused = wbt is not None and GEMM_NT and bool(_lib.load().pswin_gemm_nt_supported(M, C, N))
        dpre, db = gelu_data_gradient(dout, wb, wbt if fused else None, y2, b, b1)
        _, dw, _ = linear_backward(h, wb, dout, w2, None, None, False)
        return dpre.view_as(y2), db, dw, None, None


class MlpSkip:
    """Which products of one _MlpFused call leave out the dead samples' rows (mlp_sample_skip): fwd = fc1 + GELU and fc2 of the forward
    pass, gelu_bwd = fc2's data gradient + GELU backward, dgrad = fc1's data gradient, dw1 / dw2 = the two weight gradients."""
    __slots__ = ("fwd", "gelu_bwd", "dgrad", "dw1", "dw2")

    def __init__(self, fwd=False, gelu_bwd=False, dgrad=False, dw1=False, dw2=False):
        self.fwd, self.gelu_bwd, self.dgrad, self.dw1, self.dw2 = fwd, gelu_bwd, dgrad, dw1, dw2

    def __repr__(self):
        return "MlpSkip(" + ", ".join(f"{k}={getattr(self, k)}" for k in self.__slots__) + ")"


def mlp_sample_skip(M, C, hidden, rows_per_sample, transposed=(True, True), need_dx=True):
    """The ONE decision per _MlpFused call ([M, C] rows of B = M / rows_per_sample samples, hidden columns inside) about sample
    skipping.  A product that skips a dead sample in the forward pass leaves that sample's rows of `pre` and `h` UNWRITTEN, and the GELU
    backward leaves its rows of d(pre) unwritten: whatever torch.empty returned stays there, possibly NaN patterns, and 0 x NaN = NaN.
    Those three tensors never leave the node, so the rule is that every reader skips exactly the same rows:
      * fwd: only if ALL six products can skip exactly -- the four GEMMs run on pswin_gemm_nt with whole row tiles per sample (fc2's
        forward and fc1's data gradient go to the library at stage 3; transposed = the node holds (w1^T, w2^T)), both weight gradients
        run on the ring kernel with whole 64-row slabs per sample; then all six get the liveness;
      * otherwise nothing skips in the forward pass and the backward products decide one by one, each with defined operands: the
        GELU backward only if the two readers of d(pre) skip exactly, fc1's data gradient and the weight gradients wherever their kernel
        takes the liveness (their dead rows of dy are exact zeros; a weight-gradient slab that straddles two samples is contracted)."""
    B = M // rows_per_sample if rows_per_sample > 0 else 0
    if not SAMPLE_SKIP or rows_per_sample <= 0 or M != B * rows_per_sample or not 0 < B <= 64:
        return MlpSkip()
    whole = lambda tile: tile > 0 and rows_per_sample % tile == 0
    t_fc1 = gemm_nt_tile(M, C, hidden, "pswin_gemm_nt_gelu_fwd", required=True)
    t_fc2 = gemm_nt_tile(M, hidden, C)
    t_gelu = gemm_nt_tile(M, C, hidden, "pswin_gemm_nt_gelu_bwd", required=True) if transposed[1] else 0
    t_dgrad = gemm_nt_tile(M, hidden, C) if transposed[0] else 0
    s1, s2 = gemm_tn_ring_splits(M, hidden, C), gemm_tn_ring_splits(M, C, hidden)
    dw1, dw2 = s1 > 0 and wgrad_live_rows_ok(M, s1), s2 > 0 and wgrad_live_rows_ok(M, s2)
    slabs = rows_per_sample % 64 == 0
    dgrad_exact = whole(t_dgrad) if need_dx else True
    gelu_bwd = whole(t_gelu) and dgrad_exact and dw1 and slabs
    fwd = whole(t_fc1) and whole(t_fc2) and gelu_bwd and dw2
    return MlpSkip(fwd, gelu_bwd, whole(t_dgrad) and need_dx, dw1, dw2)


class _MlpFused(torch.autograd.Function):
    """fc2(gelu(fc1(x) + b1)) WITHOUT fc2's bias for bf16 rows on the tiled GEMM (stages 1-3; HOT:44-61): fc1 with the bias + GELU
    in its epilogue (pswin_gemm_nt_gelu_fwd: the pre-activation is written once and never re-read in the forward pass), fc2;
    backward: fc2's data gradient with the GELU backward and the fc1 bias gradient in its epilogue (pswin_gemm_nt_gelu_bwd),
    fc1's data gradient on the transposed weight copy, the two weight gradients as everywhere.
    sample_scale / rows_per_sample: the per-sample DropPath factors of the branch (None: none): the products named by mlp_sample_skip
    leave out the rows of the samples whose factor is 0; their rows of the result and of dx are zeros."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, w1_lp, w1_lp_t, w2_lp, w2_lp_t, sample_scale=None, rows_per_sample=0):
        x = x.contiguous()
        M, K = x.shape
        w1b = w1_lp if w1_lp is not None else w1.to(x.dtype)
        w2b = w2_lp if w2_lp is not None else w2.to(x.dtype)
        N = w1b.shape[0]
        b = b1.detach().float().contiguous()
        pre = torch.empty(M, N, dtype=x.dtype, device=x.device)
        h = torch.empty_like(pre)
        live = sample_liveness(sample_scale, rows_per_sample, M)
        skip = MlpSkip()
        if live is not None:
            skip = mlp_sample_skip(M, K, N, rows_per_sample, (w1_lp_t is not None, w2_lp_t is not None), ctx.needs_input_grad[0])
        tile = gemm_nt_tile(M, K, N, "pswin_gemm_nt_gelu_fwd", required=True)
        if skip.fwd:
            call("pswin_gemm_nt_gelu_fwd_live", x, ptr(x), ptr(w1b), ptr(b), ptr(pre), ptr(h), M, K, N, tile, ptr(live[0]), live[1],
                 timed_as="pswin_gemm_nt_gelu_fwd", algo_bytes=2 * (M * K + 2 * M * N + N * K), algo_flops=2 * M * K * N)
        else:
            call("pswin_gemm_nt_gelu_fwd", x, ptr(x), ptr(w1b), ptr(b), ptr(pre), ptr(h), M, K, N, tile,
                 algo_bytes=2 * (M * K + 2 * M * N + N * K), algo_flops=2 * M * K * N)
        out = linear_product(h, w2b, live=live if skip.fwd else None)
        ctx.save_for_backward(x, pre, h, b, w1b, w1_lp_t, w2b, w2_lp_t)
        ctx.params = (w1, b1, w2)
        ctx.live, ctx.skip = live, skip
        return out

    @staticmethod
    def backward(ctx, dout):
        x, pre, h, b, w1b, w1bt, w2b, w2bt = ctx.saved_tensors
        w1, b1, w2 = ctx.params
        live, skip = ctx.live, ctx.skip
        pick = lambda on: live if on else None
        dout = dout.contiguous()
        dpre, db = gelu_data_gradient(dout, w2b, w2bt, pre, b, b1, pick(skip.gelu_bwd))     # fused: mlp_fused_supported checked the shape
        _, dw2, _ = linear_backward(h, w2b, dout, w2, None, None, False, wgrad_live=pick(skip.dw2))
        dx, dw1, _ = linear_backward(x, w1b, dpre, w1, None, None, ctx.needs_input_grad[0], w1bt, wgrad_live=pick(skip.dw1),
                                     dgrad_live=pick(skip.dgrad))
        return dx, dw1, db, dw2, None, None, None, None, None, None


def mlp_fused_supported(x2d, hidden):
    return (GEMM_NT and FUSED_GELU_BWD and FUSED_MLP and x2d.dtype == torch.bfloat16 and x2d.is_cuda and x2d.dim() == 2 and x2d.shape[0] >= 64
            and bool(_lib.load().pswin_gemm_nt_supported(x2d.shape[0], x2d.shape[1], hidden)))


def mlp_fused(x2d, fc1, fc2, sample_scale=None, rows_per_sample=0):
    """fc2_nobias(gelu(fc1(x2d))) as one autograd node on the tiled GEMM kernels: see _MlpFused."""
    (w1_lp, _, w1_lp_t), (w2_lp, _, w2_lp_t) = _lowp(fc1), _lowp(fc2)
    return _MlpFused.apply(x2d, fc1.weight, fc1.bias, fc2.weight, w1_lp, w1_lp_t, w2_lp, w2_lp_t, sample_scale, rows_per_sample)


def bias_gelu_linear(y, bias1, lin2):
    """lin2(gelu(y + bias1)) without lin2's bias (bf16 rows): see _BiasGeluLinear."""
    w_lp, _, w_lp_t = _lowp(lin2)
    out = _BiasGeluLinear.apply(y.reshape(-1, y.shape[-1]), bias1, lin2.weight, w_lp, w_lp_t)
    return out.view(*y.shape[:-1], lin2.weight.shape[0])


def bias_gelu(y, bias):
    """gelu(y + bias) (exact, erf) on [..., N]; the backward pass also returns the bias gradient (column sums of
    dy) from the same pass: fc1 bias + nn.GELU of Mlp (HOT:50-57) without a GEMM epilogue or a separate reduction."""
    return _BiasGelu.apply(y, bias)


class _InterpRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, wgt):
        B, S, C = x.shape
        P = idx.shape[0]
        ctx.save_for_backward(idx, wgt)
        ctx.geom = (B, S, P, C)
        x = x.contiguous()
        out = torch.empty(B, P, C, dtype=torch.float32, device=x.device)
        call("pswin_interp_rows", x, ptr(x), ptr(idx), ptr(wgt), ptr(out), B, S, P, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        idx, wgt = ctx.saved_tensors
        B, S, P, C = ctx.geom
        dout = dout.contiguous()
        dx = torch.zeros(B, S, C, dtype=torch.float32, device=dout.device)
        call("pswin_interp_rows_adjoint", dout, ptr(dout), ptr(idx), ptr(wgt), ptr(dx), B, S, P, C)
        return dx, None, None


def interp_rows(x, idx, wgt):
    """out[b, p] = sum_k wgt[p, k] x[b, idx[p, k]]: a static bilinear F.grid_sample as a 4-tap row gather."""
    return _InterpRows.apply(x.float(), idx, wgt)


# ------------------------------------------------------------------------------------------------
# window attention
# ------------------------------------------------------------------------------------------------
class Tiles:
    """A [n, 49, 49] fp32 table as zero-padded 64 x 64 tiles: `fwd` holds tile[i][j], `bwd` the transposed tile[j][i]
    (the same buffer when the table is symmetric, e.g. self-attention distances and the shifted-window mask)."""

    def __init__(self, table, symmetric=False):
        table = table.contiguous().float()
        assert table.dim() == 3 and table.shape[1:] == (WTOK, WTOK)
        self.n = table.shape[0]
        self.table = table
        self.fwd = torch.empty(self.n, WPAD, WPAD, dtype=torch.float32, device=table.device)
        call("pswin_attn_pad_tiles", table, ptr(table), self.n, 0, ptr(self.fwd))
        if symmetric:
            self.bwd = self.fwd
        else:
            self.bwd = torch.empty_like(self.fwd)
            call("pswin_attn_pad_tiles", table, ptr(table), self.n, 1, ptr(self.bwd))


def window_dist_tiles(H, W, shift, device):
    """Tiles of window_dist (symmetric: haversine of a window with itself)."""
    key = ("dist_tiles", H, W, shift, _dev_key(device))
    if key not in _CACHE:
        _CACHE[key] = Tiles(window_dist(H, W, shift, device), symmetric=True)
    return _CACHE[key]


def planar_mask_tiles(H, W, shift, device):
    key = ("mask_tiles", H, W, shift, _dev_key(device))
    if key not in _CACHE:
        _CACHE[key] = Tiles(planar_mask(H, W, shift, device), symmetric=True)
    return _CACHE[key]


def _as_tiles(t):
    if t is None or isinstance(t, Tiles):
        return t
    return Tiles(t)


class _WindowAttention(torch.autograd.Function):
    """softmax(scale q k^T + bias) v per (window, head); q, k, v either slices of one fused [rows, 3C] buffer
    (k = v = None) or three separate [rows, C] tensors."""

    @staticmethod
    def forward(ctx, q_or_qkv, k, v, alpha, beta, dist, mask, heads, scale, n_bias_windows, chunks):
        fused = k is None
        x = q_or_qkv.contiguous()
        C = heads * _lib.HEAD_DIM
        rows = x.shape[0]
        assert rows % WTOK == 0
        n = rows // WTOK
        if fused:
            assert x.shape[1] == 3 * C, "fused qkv must be [rows, 3C] with C = heads * 32"
            ld = 3 * C
            es = x.element_size()
            qp, kp, vp = x.data_ptr(), x.data_ptr() + C * es, x.data_ptr() + 2 * C * es
        else:
            k, v = k.contiguous(), v.contiguous()
            assert x.shape == k.shape == v.shape and x.shape[1] == C
            assert x.dtype == k.dtype == v.dtype
            ld = C
            qp, kp, vp = x.data_ptr(), k.data_ptr(), v.data_ptr()
        alpha_p, beta_p = (alpha if dist is not None else None), beta
        alpha = alpha.contiguous() if dist is not None else None
        beta = beta.contiguous()
        out = torch.empty(rows, C, dtype=x.dtype, device=x.device)
        lse = torch.empty(n, heads, WPAD, dtype=torch.float32, device=x.device)
        call("pswin_attn_fwd", x, ctypes.c_void_p(qp), ctypes.c_void_p(kp), ctypes.c_void_p(vp), ld,
             ptr(None if dist is None else dist.fwd), 0 if dist is None else dist.n, ptr(alpha), ptr(beta),
             ptr(None if mask is None else mask.fwd), 0 if mask is None else mask.n, ptr(out), C, ptr(lse),
             int(chunks or 0), n, n_bias_windows, heads, float(scale), dtype_code(x),
             algo_bytes=n * heads * 4 * WTOK * _lib.HEAD_DIM * x.element_size())
        ctx.fused, ctx.heads, ctx.scale, ctx.nb, ctx.n, ctx.C = fused, heads, float(scale), n_bias_windows, n, C
        ctx.dist, ctx.mask, ctx.chunks = dist, mask, chunks
        ctx.owners = (alpha_p, beta_p)
        ctx.save_for_backward(x, k, v, lse, alpha, beta)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, k, v, lse, alpha, beta = ctx.saved_tensors
        dx, dk, dv, dalpha, dbeta = attention_backward(x, k, v, lse, alpha, beta, ctx.dist, ctx.mask, dout, ctx.heads, ctx.scale,
                                                       ctx.nb, ctx.chunks, ctx.needs_input_grad[3] or ctx.needs_input_grad[4],
                                                       ctx.owners)
        return dx, dk, dv, dalpha, dbeta, None, None, None, None, None, None


def attention_backward(x, k, v, lse, alpha, beta, dist, mask, dout, heads, scale, nb, chunks, need_tables, owners, packed=False):
    """Backward of the attention core (pswin_attn_bwd + the table-gradient kernels): x = fused [rows, 3C] qkv (k = v =
    None) or q with separate k, v; packed=True: x = [n, heads, 3, 49, 32] (what the fused forward kernel saves), the
    gradient still comes back as one row-major [rows, 3C] tensor.  Returns (dx, dk, dv, dalpha, dbeta); owners = the
    (alpha, beta) parameters."""
    C = heads * _lib.HEAD_DIM
    n = x.shape[0] if packed else x.shape[0] // WTOK
    fused = k is None
    dout = dout.contiguous()
    es = x.element_size()
    ld_in, win_stride, head_stride = None, None, _lib.HEAD_DIM
    if packed:
        dx = torch.empty(n * WTOK, 3 * C, dtype=x.dtype, device=x.device)
        ld = 3 * C
        blk = WTOK * _lib.HEAD_DIM
        qp, kp, vp = x.data_ptr(), x.data_ptr() + blk * es, x.data_ptr() + 2 * blk * es
        dqp, dkp, dvp = dx.data_ptr(), dx.data_ptr() + C * es, dx.data_ptr() + 2 * C * es
        dk = dv = None
        ld_in, win_stride, head_stride = _lib.HEAD_DIM, heads * 3 * blk, 3 * blk
    elif fused:
        dx = torch.empty_like(x)
        ld = 3 * C
        qp, kp, vp = x.data_ptr(), x.data_ptr() + C * es, x.data_ptr() + 2 * C * es
        dqp, dkp, dvp = dx.data_ptr(), dx.data_ptr() + C * es, dx.data_ptr() + 2 * C * es
        dk = dv = None
    else:
        dx, dk, dv = torch.empty_like(x), torch.empty_like(k), torch.empty_like(v)
        ld = C
        qp, kp, vp = x.data_ptr(), k.data_ptr(), v.data_ptr()
        dqp, dkp, dvp = dx.data_ptr(), dk.data_ptr(), dv.data_ptr()
    lib = _lib.load()
    chunks = chunks or lib.pswin_attn_suggest_chunks(n, nb, heads, 1)
    dalpha = dbeta = gsum = None
    if need_tables:
        gsum = torch.empty(chunks * nb, heads, WPAD, WPAD, dtype=torch.float32, device=x.device)
    ld_in = ld if ld_in is None else ld_in
    win_stride = WTOK * ld_in if win_stride is None else win_stride
    call("pswin_attn_bwd_ex", x, ctypes.c_void_p(qp), ctypes.c_void_p(kp), ctypes.c_void_p(vp), ld_in, win_stride, head_stride,
         ptr(None if dist is None else dist.bwd), 0 if dist is None else dist.n, ptr(alpha), ptr(beta),
         ptr(None if mask is None else mask.bwd), 0 if mask is None else mask.n, ptr(dout), C, ptr(lse),
         ctypes.c_void_p(dqp), ctypes.c_void_p(dkp), ctypes.c_void_p(dvp), ld, ptr(gsum),
         chunks, n, nb, heads, scale, dtype_code(x),
         algo_bytes=n * heads * 7 * WTOK * _lib.HEAD_DIM * x.element_size())
    if need_tables:
        dalpha, dbeta = grad_queue.table_gradients(gsum, None if dist is None else dist.bwd, chunks * nb, nb, 0 if dist is None else dist.n,
                                                   heads, owners, DEFER_TABLE_PARTIALS)
    return dx, dk, dv, dalpha, dbeta


def window_attention(qkv, alpha, beta, dist, mask, heads, scale, n_bias_windows, k=None, v=None, chunks=None):
    """BasicWindowAttention.forward between qkv and proj (HOT:288-308).

    qkv: [n*49, 3C] (or q with k, v given: three [n*49, C]); alpha/beta: [169, heads] f32 tables;
    dist: great-circle table, a [nW, 49, 49] f32 tensor or a prebuilt ``Tiles`` (None in planar mode: beta only,
    HOT:257-258); mask: f32 [nM, 49, 49] tensor / ``Tiles`` / None; window n uses bias window n % n_bias_windows.
    chunks: work items per bias window (None = library heuristic).  Returns [n*49, C].
    """
    return _WindowAttention.apply(qkv, k, v, alpha, beta, _as_tiles(dist), _as_tiles(mask), heads, scale,
                                  n_bias_windows, chunks)


class _WindowAttentionFused(torch.autograd.Function):
    """WindowAttention.forward (HOT:274-323) as ONE kernel per direction-of-use: qkv Linear, attention core and proj Linear
    of a window run out of registers (pswin_win_attn_fused_fwd); the qkv tensor is written only when a backward pass
    will read it.  The backward pass is the unfused chain on the saved tensors (proj gradients, pswin_attn_bwd, qkv
    gradients): identical kernels and summation order to the unfused path."""

    @staticmethod
    def forward(ctx, x, w_qkv, b_qkv, w_proj, alpha, beta, dist, mask, heads, scale, n_bias_windows, wq_lp, wp_lp, grad_mode):
        x = x.contiguous()
        rows, C = x.shape
        n = rows // WTOK
        assert rows % WTOK == 0 and C == heads * _lib.HEAD_DIM
        wq = (wq_lp if wq_lp is not None else w_qkv.to(x.dtype)).contiguous()
        wp = (wp_lp if wp_lp is not None else w_proj.to(x.dtype)).contiguous()
        bq = None if b_qkv is None else b_qkv.detach().float().contiguous()
        alpha_c = alpha.detach().contiguous() if dist is not None else None
        beta_c = beta.detach().contiguous()
        # grad_mode = torch.is_grad_enabled() of the CALLER (inside forward() it is always off, and needs_input_grad
        # ignores torch.no_grad()): without a backward pass to come, qkv / the attention output / lse are never written
        save = grad_mode and any(ctx.needs_input_grad)
        y = torch.empty_like(x)
        qkv = att = lse = None
        if save:
            qkv = torch.empty(n, heads, 3, WTOK, _lib.HEAD_DIM, dtype=x.dtype, device=x.device)     # packed blocks (pswin_attn_bwd_ex)
            att = torch.empty_like(x)
            lse = torch.empty(n, heads, WPAD, dtype=torch.float32, device=x.device)
        flops = n * (2 * WTOK * C * 3 * C + heads * 4 * WTOK * WTOK * _lib.HEAD_DIM + 2 * WTOK * C * C)
        call("pswin_win_attn_fused_fwd", x, ptr(x), ptr(wq), ptr(bq), ptr(wp), ptr(None if dist is None else dist.fwd),
             0 if dist is None else dist.n, ptr(alpha_c), ptr(beta_c), ptr(None if mask is None else mask.fwd),
             0 if mask is None else mask.n, ptr(y), ptr(qkv), ptr(att), ptr(lse), n, n_bias_windows, C, heads, float(scale),
             dtype_code(x), algo_bytes=rows * C * 2 * (6 if save else 2), algo_flops=flops)
        if save:
            ctx.save_for_backward(x, qkv, att, lse, wq, wp, alpha_c, beta_c)
            ctx.params = (w_qkv, b_qkv, w_proj, alpha if dist is not None else None, beta)
            ctx.cfg = (dist, mask, heads, float(scale), n_bias_windows)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, qkv, att, lse, wq, wp, alpha_c, beta_c = ctx.saved_tensors
        w_qkv, b_qkv, w_proj, alpha, beta = ctx.params
        dist, mask, heads, scale, nb = ctx.cfg
        C = x.shape[1]
        datt, dwp, _ = linear_backward(att, wp, dy, w_proj, None, None, True)
        dqkv, _, _, dalpha, dbeta = attention_backward(qkv, None, None, lse, alpha_c, beta_c, dist, mask, datt, heads, scale, nb,
                                                        None, ctx.needs_input_grad[4] or ctx.needs_input_grad[5], (alpha, beta),
                                                        packed=True)
        # the K third of d(qkv) sums to zero over every window (rows of dS sum to 0): its bias gradient is not summed
        dx, dwq, dbq = linear_backward(x, wq, dqkv, w_qkv, b_qkv, (C, 2 * C), ctx.needs_input_grad[0])
        return dx, dwq, dbq, dwp, dalpha, dbeta, None, None, None, None, None, None, None, None


def fused_windows_addressable(n_windows, C):
    """the bound the fused attention launchers enforce on the packed q, k, v save: n_windows * 49 * 3C * 2 bytes < 0x7fffffff00"""
    return n_windows * WTOK * 3 * C * 2 < 0x7fffffff00


def window_attention_fused_supported(x2d, heads):
    return (x2d.is_cuda and x2d.dim() == 2 and x2d.dtype == torch.bfloat16 and fused_windows_addressable(x2d.shape[0] // WTOK, x2d.shape[1])
            and bool(_lib.load().pswin_win_attn_fused_supported(x2d.shape[1], heads, BF16)))


def window_attention_fused(x2d, attn, dist, mask, n_bias_windows):
    """proj(attention(qkv(x2d))) WITHOUT the proj bias for window rows x2d [n*49, C] and the parameter holder `attn`
    (qkv, proj, the two tables, num_heads, scale): see _WindowAttentionFused."""
    return _WindowAttentionFused.apply(x2d, attn.qkv.weight, attn.qkv.bias, attn.proj.weight,
                                       attn.sphere_position_alpha_table_Te, attn.sphere_position_beta_table_Te,
                                       _as_tiles(dist), _as_tiles(mask), attn.num_heads, attn.scale, n_bias_windows,
                                       _lowp(attn.qkv)[0], _lowp(attn.proj)[0], torch.is_grad_enabled())


# ------------------------------------------------------------------------------------------------
# the caller's side: RoIAlign over the FPN pyramid
# ------------------------------------------------------------------------------------------------
def _roi_levels(ptrs_fwd, ptrs_bwd, shapes, strides):
    lv = _lib.RoiLevels()
    lv.n_levels = len(shapes)
    for l, ((H, W), s) in enumerate(zip(shapes, strides)):
        lv.feat[l] = ptrs_fwd[l] if ptrs_fwd else None
        lv.dfeat[l] = ptrs_bwd[l] if ptrs_bwd else None
        lv.H[l], lv.W[l], lv.spatial_scale[l] = H, W, 1.0 / s
    return lv


class _RoiAlignFPN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rois, roi_level, P, sampling_ratio, aligned, strides, *feats):
        C = feats[0].shape[1]
        dt = feats[0].dtype
        if len(feats) > 4 or any(f.dtype != dt or f.shape[1] != C or f.dim() != 4 for f in feats):
            raise PswinError("roi_align_fpn: up to four NCHW maps of one dtype and channel count")
        if not _lib.load().pswin_roi_align_supported(C, dtype_code(feats[0])):
            raise PswinError(f"roi_align_fpn: unsupported channel count {C} for {dt}")
        nhwc = [f.permute(0, 2, 3, 1).contiguous() for f in feats]          # a pixel's channels = one contiguous row
        rois = rois.detach().float().contiguous()
        roi_level = roi_level.to(torch.int32).contiguous()
        R = rois.shape[0]
        out = torch.empty(R, P, P, C, dtype=dt, device=rois.device)
        shapes = [tuple(f.shape[2:]) for f in feats]
        lv = _roi_levels([f.data_ptr() for f in nhwc], None, shapes, strides)
        call("pswin_roi_align_fwd", out, ctypes.byref(lv), ptr(rois), ptr(roi_level), R, C, P, int(sampling_ratio), int(aligned),
             dtype_code(out), ptr(out))
        ctx.save_for_backward(rois, roi_level)
        ctx.cfg = (P, int(sampling_ratio), int(aligned), tuple(strides), shapes, [f.shape[0] for f in feats], C, dt)
        return out.permute(0, 3, 1, 2)                                      # [R, C, P, P] (channels-last in memory)

    @staticmethod
    def backward(ctx, dout):
        rois, roi_level = ctx.saved_tensors
        P, sr, aligned, strides, shapes, batches, C, dt = ctx.cfg
        d = dout.permute(0, 2, 3, 1).to(dt).contiguous()                    # [R, P, P, C]
        grads = [torch.zeros(b, H, W, C, dtype=torch.float32, device=d.device) for b, (H, W) in zip(batches, shapes)]
        lv = _roi_levels(None, [g.data_ptr() for g in grads], shapes, strides)
        call("pswin_roi_align_bwd", d, ctypes.byref(lv), ptr(rois), ptr(roi_level), rois.shape[0], C, P, sr, aligned, dtype_code(d), ptr(d))
        return (None, None, None, None, None, None) + tuple(g.permute(0, 3, 1, 2).to(dt) for g in grads)


def map_roi_levels(rois, num_levels, finest_scale=56):
    """SingleRoIExtractor.map_roi_levels (mmdet/models/roi_heads/roi_extractors/single_level_roi_extractor.py:55-60): rois [R, 5]."""
    scale = torch.sqrt((rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2]))
    return torch.floor(torch.log2(scale / finest_scale + 1e-6)).clamp(min=0, max=num_levels - 1).long()


def roi_align_fpn(feats, strides, rois, out_size, sampling_ratio=0, aligned=True, finest_scale=56, roi_level=None):
    """SingleRoIExtractor(RoIAlign(out_size, sampling_ratio)) over up to four NCHW pyramid levels (single_level_roi_extractor.py:78-108,
    configs/_base_/models/mask_rcnn_swin_fpn.py:44-48): rois [R, 5] = (batch index, x1, y1, x2, y2) in image pixels -> [R, C, out, out].
    Forward and backward are HIP kernels (pswin_roi_align_fwd / _bwd); only the feature maps receive a gradient."""
    if roi_level is None:
        roi_level = map_roi_levels(rois, len(feats), finest_scale)
    return _RoiAlignFPN.apply(rois, roi_level, int(out_size), sampling_ratio, aligned, tuple(strides), *feats)


_NMS_COUNTS = {}


def nms_groups(box_list, iou_thr):
    """Greedy NMS of several score-sorted box lists in ONE launch (pswin_nms_groups; a workgroup per list): list of bool keep masks.
    box_list: f32 [n_g, 4] tensors on one HIP device, n_g <= 2048 (the RPN's nms_pre = 2000 per image and pyramid level)."""
    ns = tuple(int(b.shape[0]) for b in box_list)
    dev = box_list[0].device
    nmax = -(-max(ns) // 64) * 64                    # the kernels work on whole 64-row chunks
    if nmax == 0:
        return [torch.zeros(0, dtype=torch.bool, device=dev) for _ in ns]
    if nmax > 2048:
        raise PswinError(f"nms_groups: at most 2048 boxes per list, got {max(ns)}")
    key = (ns, _dev_key(dev))
    if key not in _NMS_COUNTS:                      # static per feature-map geometry: no host-to-device copy inside a captured step
        _NMS_COUNTS[key] = torch.tensor(ns, dtype=torch.int32, device=dev)
    boxes = torch.zeros(len(ns), nmax, 4, dtype=torch.float32, device=dev)
    for g, b in enumerate(box_list):
        boxes[g, :ns[g]] = b.detach().float()
    keep = torch.empty(len(ns), nmax, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(_lib.load().pswin_nms_workspace(len(ns), nmax)), dtype=torch.uint8, device=dev)
    call("pswin_nms_groups", boxes, ptr(boxes), ptr(_NMS_COUNTS[key]), len(ns), nmax, ctypes.c_float(float(iou_thr)), ptr(keep), ptr(ws))
    return [keep[g, :ns[g]].bool() for g in range(len(ns))]


def max_iou_assign_batch(cand, gt, gt_count, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, match_low_quality=True, lead_gt=0, want_max_iou=True):
    """MaxIoUAssigner.assign for a padded batch in TWO launches (pswin_max_iou_assign): (gt_inds int64 [B, N], max_iou f32 [B, N] or None).
    cand: f32 [N, 4] shared by the images or [B, N, 4]; gt: f32 [B, Gmax, 4]; gt_count: int32 [B] ON THE DEVICE (rows past it are padding);
    lead_gt: the number of leading candidates that are the image's own gt rows (those past the count come back as -1).  No host-to-device
    copy and no host synchronisation: the call can be captured, and a replay reads whatever boxes and counts the buffers hold then.  The
    partial maxima live in one workspace per (B, N, Gmax, device), written in full by every call before it is read."""
    if gt.dim() != 3 or gt.shape[2] != 4 or cand.dim() not in (2, 3) or cand.shape[-1] != 4 or (cand.dim() == 3 and cand.shape[0] != gt.shape[0]):
        raise PswinError(f"max_iou_assign_batch: candidates [N, 4] or [B, N, 4] and gt [B, Gmax, 4], got {tuple(cand.shape)} and {tuple(gt.shape)}")
    B, Gmax = int(gt.shape[0]), int(gt.shape[1])
    N = int(cand.shape[-2])
    if gt_count.dtype != torch.int32 or tuple(gt_count.shape) != (B,) or gt_count.device != gt.device or cand.device != gt.device:
        raise PswinError("max_iou_assign_batch: gt_count must be an int32 [B] tensor on the device of the boxes")
    cand, gt, gt_count = cand.detach().float().contiguous(), gt.detach().float().contiguous(), gt_count.contiguous()
    nbytes = int(_lib.load().pswin_max_iou_assign_workspace(B, N, Gmax))
    _lib.check(min(nbytes, 0), "pswin_max_iou_assign_workspace")
    key = ("assign_ws", B, N, Gmax, _dev_key(gt.device))
    if key not in _CACHE:
        _CACHE[key] = torch.empty(nbytes, dtype=torch.uint8, device=gt.device)
    inds = torch.empty(B, N, dtype=torch.int64, device=gt.device)
    miou = torch.empty(B, N, dtype=torch.float32, device=gt.device) if want_max_iou else None
    call("pswin_max_iou_assign", gt, ptr(cand), int(cand.dim() == 3), ptr(gt), ptr(gt_count), B, N, Gmax, int(lead_gt),
         ctypes.c_float(float(pos_iou_thr)), ctypes.c_float(float(neg_iou_thr)), ctypes.c_float(float(min_pos_iou)), int(bool(match_low_quality)),
         ptr(inds), ptr(miou), ptr(_CACHE[key]))
    return inds, miou


def _sample_inputs(what, gt_inds, key):
    if gt_inds.dim() != 2 or gt_inds.dtype != torch.int64 or tuple(key.shape) != tuple(gt_inds.shape) or key.device != gt_inds.device:
        raise PswinError(f"{what}: gt_inds int64 [B, N] and key [B, N] on one device, got {tuple(gt_inds.shape)} {gt_inds.dtype} and "
                         f"{tuple(key.shape)}")
    return gt_inds.contiguous(), key.detach().float().contiguous()


def sample_ranks(gt_inds, key, n_pos, n_neg):
    """detector.sample_ranks on the GPU (pswin_sample_ranks): (pos_rank int64 [B, n_pos], neg_rank int64 [B, n_neg]) -- the first
    candidates of the positive and of the negative order by (composed float32 key, index).  gt_inds int64 [B, N]; key f32 [B, N], finite
    and >= 0.  A fixed number of launches for given (N, max(n_pos, n_neg)), no host synchronisation, no atomics: the call can be captured,
    and a replay ranks whatever the buffers hold then.  The tree's partial lists live in one workspace per (B, N, k, device), written by
    every call before it is read.  CPU tensors: the definition."""
    if not gt_inds.is_cuda:
        from . import detector
        return detector.sample_ranks(gt_inds, key, n_pos, n_neg)
    gt_inds, key = _sample_inputs("sample_ranks", gt_inds, key)
    B, N = (int(v) for v in gt_inds.shape)
    n_pos, n_neg = int(n_pos), int(n_neg)
    k = max(n_pos, n_neg)
    nbytes = int(_lib.load().pswin_sample_workspace(B, N, k))
    _lib.check(min(nbytes, 0), "pswin_sample_workspace")
    ws_key = ("sample_ws", B, N, k, _dev_key(gt_inds.device))
    if ws_key not in _CACHE:
        _CACHE[ws_key] = torch.empty(nbytes, dtype=torch.uint8, device=gt_inds.device)
    pos_rank = torch.empty(B, n_pos, dtype=torch.int64, device=gt_inds.device)
    neg_rank = torch.empty(B, n_neg, dtype=torch.int64, device=gt_inds.device)
    call("pswin_sample_ranks", key, ptr(gt_inds), ptr(key), B, N, n_pos, n_neg, ptr(pos_rank), ptr(neg_rank), ptr(_CACHE[ws_key]))
    return pos_rank, neg_rank


def rpn_targets(gt_inds, key, anchors, gt, n_pos_max, n_tot):
    """detector.rpn_targets on the GPU (pswin_sample_ranks, then one launch of pswin_rpn_targets): (idx int64 [B, n_pos_max + n_tot], valid
    f32 of that shape, pos_valid bool [B, n_pos_max], reg_t f32 [B, n_pos_max, 4]).  gt_inds int64 [B, A]; key f32 [B, A]; anchors f32
    [A, 4]; gt f32 [B, Gmax, 4].  Capturable as sample_ranks is.  CPU tensors: the definition."""
    if not gt_inds.is_cuda:
        from . import detector
        return detector.rpn_targets(gt_inds, key, anchors, gt, n_pos_max, n_tot)
    gt_inds, key = _sample_inputs("rpn_targets", gt_inds, key)
    B, N = (int(v) for v in gt_inds.shape)
    if tuple(anchors.shape) != (N, 4) or gt.dim() != 3 or gt.shape[0] != B or gt.shape[2] != 4 or anchors.device != key.device or gt.device != key.device:
        raise PswinError(f"rpn_targets: anchors [{N}, 4] and gt [{B}, Gmax, 4] on the device of gt_inds, got {tuple(anchors.shape)} and {tuple(gt.shape)}")
    n_pos_max, n_tot, Gmax, dev = int(n_pos_max), int(n_tot), int(gt.shape[1]), key.device
    anchors, gt = anchors.detach().float().contiguous(), gt.detach().float().contiguous()
    pos_rank, neg_rank = sample_ranks(gt_inds, key, n_pos_max, n_tot)
    idx = torch.empty(B, n_pos_max + n_tot, dtype=torch.int64, device=dev)
    valid = torch.empty(B, n_pos_max + n_tot, dtype=torch.float32, device=dev)
    pos_valid = torch.empty(B, n_pos_max, dtype=torch.uint8, device=dev)
    reg_t = torch.empty(B, n_pos_max, 4, dtype=torch.float32, device=dev)
    call("pswin_rpn_targets", key, ptr(gt_inds), ptr(pos_rank), ptr(neg_rank), ptr(anchors), ptr(gt), B, N, Gmax, n_pos_max, n_tot, ptr(idx),
         ptr(valid), ptr(pos_valid), ptr(reg_t))
    return idx, valid, pos_valid.view(torch.bool), reg_t


def roi_targets(gt_inds, key, cand, gt, gt_labels, num_classes, n_pos_max, n_tot, stds):
    """detector.roi_targets on the GPU (pswin_sample_ranks, then one launch of pswin_roi_targets): (rois f32 [B, n_tot, 4], labels int64
    [B, n_tot], reg_t f32 [B, n_pos_max, 4], pos_valid bool [B, n_pos_max], gt_idx int64 [B, n_pos_max]).  gt_inds int64 [B, N]; key f32
    [B, N]; cand f32 [B, N, 4]; gt f32 [B, Gmax, 4]; gt_labels int64 [B, Gmax].  Capturable as sample_ranks is.  CPU tensors: the definition."""
    if not gt_inds.is_cuda:
        from . import detector
        return detector.roi_targets(gt_inds, key, cand, gt, gt_labels, num_classes, n_pos_max, n_tot, stds)
    gt_inds, key = _sample_inputs("roi_targets", gt_inds, key)
    B, N = (int(v) for v in gt_inds.shape)
    dev = key.device
    if tuple(cand.shape) != (B, N, 4) or gt.dim() != 3 or gt.shape[0] != B or gt.shape[2] != 4 or tuple(gt_labels.shape) != tuple(gt.shape[:2]) or \
            gt_labels.dtype != torch.int64 or any(t.device != dev for t in (cand, gt, gt_labels)):
        raise PswinError(f"roi_targets: cand [{B}, {N}, 4], gt [{B}, Gmax, 4] and int64 gt_labels [{B}, Gmax] on the device of gt_inds, got "
                         f"{tuple(cand.shape)}, {tuple(gt.shape)} and {tuple(gt_labels.shape)} {gt_labels.dtype}")
    n_pos_max, n_tot, Gmax = int(n_pos_max), int(n_tot), int(gt.shape[1])
    cand, gt, gt_labels = cand.detach().float().contiguous(), gt.detach().float().contiguous(), gt_labels.contiguous()
    pos_rank, neg_order = sample_ranks(gt_inds, key, n_pos_max, n_tot)
    rois = torch.empty(B, n_tot, 4, dtype=torch.float32, device=dev)
    labels = torch.empty(B, n_tot, dtype=torch.int64, device=dev)
    reg_t = torch.empty(B, n_pos_max, 4, dtype=torch.float32, device=dev)
    pos_valid = torch.empty(B, n_pos_max, dtype=torch.uint8, device=dev)
    gt_idx = torch.empty(B, n_pos_max, dtype=torch.int64, device=dev)
    std4 = (ctypes.c_float * 4)(*[float(v) for v in stds])
    call("pswin_roi_targets", key, ptr(gt_inds), ptr(pos_rank), ptr(neg_order), ptr(cand), ptr(gt), ptr(gt_labels), B, N, Gmax, n_pos_max, n_tot,
         int(num_classes), ctypes.cast(std4, ctypes.c_void_p), ptr(rois), ptr(labels), ptr(reg_t), ptr(pos_valid), ptr(gt_idx))
    return rois, labels, reg_t, pos_valid.view(torch.bool), gt_idx


def mask_targets(masks, rois, gt_idx, pos_valid, size=28):
    """detector.mask_targets on the GPU in one launch (pswin_mask_targets): f32 [B P, size, size] of 0 / 1.  masks uint8 [B, Gmax, H, W];
    rois f32 [B, P, 4]; gt_idx int64 [B, P]; pos_valid bool [B, P].  Reads at most four bytes of the one assigned bitmap per sample point
    and nothing for a row whose pos_valid is false.  CPU tensors: the definition."""
    if not masks.is_cuda:
        from . import detector
        return detector.mask_targets(masks, rois, gt_idx, pos_valid, size)
    if masks.dim() != 4 or masks.dtype != torch.uint8 or rois.dim() != 3 or rois.shape[0] != masks.shape[0] or rois.shape[2] != 4 or \
            tuple(gt_idx.shape) != tuple(rois.shape[:2]) or tuple(pos_valid.shape) != tuple(rois.shape[:2]) or gt_idx.dtype != torch.int64 or \
            pos_valid.dtype not in (torch.bool, torch.uint8) or any(t.device != masks.device for t in (rois, gt_idx, pos_valid)):
        raise PswinError(f"mask_targets: masks uint8 [B, Gmax, H, W], rois [B, P, 4], gt_idx int64 [B, P] and pos_valid bool [B, P] on one "
                         f"device, got {tuple(masks.shape)} {masks.dtype}, {tuple(rois.shape)}, {tuple(gt_idx.shape)} {gt_idx.dtype}, "
                         f"{tuple(pos_valid.shape)} {pos_valid.dtype}")
    B, Gmax, H, W = (int(v) for v in masks.shape)
    P, size = int(rois.shape[1]), int(size)
    masks, rois, gt_idx = masks.contiguous(), rois.detach().float().contiguous(), gt_idx.contiguous()
    pv = pos_valid.contiguous().view(torch.uint8)
    out = torch.empty(B * P, size, size, dtype=torch.float32, device=masks.device)
    call("pswin_mask_targets", rois, ptr(masks), ptr(rois), ptr(gt_idx), ptr(pv), B, P, Gmax, H, W, size, ptr(out), algo_bytes=B * P * size * size * 8)
    return out


def _level_sizes(level_sizes):
    ns = (ctypes.c_int * len(level_sizes))(*[int(n) for n in level_sizes])
    return ns, ctypes.cast(ns, ctypes.c_void_p)


def rpn_proposals_supported(level_sizes, B, nms_pre, max_per_img):
    """Whether pswin_rpn_proposals takes the shape: at most 8 levels, nms_pre <= 2048, P = min(max_per_img, sum of min(nms_pre, n_l))
    <= 2048, B L <= 2048, B A < 2^31 and a workspace below 2^31 bytes (the entry point's own check, asked here without a launch)."""
    if not 1 <= len(level_sizes) <= 8 or min(int(n) for n in level_sizes) < 1 or sum(int(n) for n in level_sizes) * int(B) >= 1 << 31:
        return False
    ns, nsp = _level_sizes(level_sizes)
    return int(_lib.load().pswin_rpn_proposals_workspace(nsp, len(level_sizes), int(B), int(nms_pre), int(max_per_img))) > 0


def rpn_proposals_rows_per_workgroup():
    """The scores one workgroup of pswin_rpn_proposals sorts: the chunk of its reduction trees"""
    return int(_lib.load().pswin_rpn_proposals_rows_per_workgroup())


def rpn_proposals_launches(level_sizes, nms_pre, max_per_img):
    """The kernel launches of one pswin_rpn_proposals call on these level sizes, whatever the batch"""
    ns, nsp = _level_sizes(level_sizes)
    n = int(_lib.load().pswin_rpn_proposals_launches(nsp, len(level_sizes), int(nms_pre), int(max_per_img)))
    _lib.check(min(n, 0), "pswin_rpn_proposals_launches")
    return n


def rpn_proposals(scores, deltas, anchors, nms_pre, iou_thr, max_per_img, img_hw):
    """detector.proposals_batch on the GPU (pswin_rpn_proposals): (rois f32 [B, P, 4], scores f32 [B, P], count int32 [B]) with
    P = min(max_per_img, sum over the levels of min(nms_pre, n_l)) -- ALL P rows of every image as MiniMaskRCNN._proposals leaves them, the
    suppressed tail (score -1e4) behind the count[b] survivors.  scores f32 [B, A] raw logits; deltas f32 [B, A, 4]; anchors: the list of
    the levels' f32 [n_l, 4] tensors (make_anchors), A = their sum.  NaN scores and scores <= -1e4 are outside the contract.

    LAUNCHES: rpn_proposals_launches(level sizes, nms_pre, max_per_img) kernels -- the selection passes (one per fourfold reduction of the
    largest level's chunks of 8192 scores), the two launches of pswin_nms_groups, the passes of the final order -- plus the one
    concatenation of the anchors: 7 for the five levels of a 512 x 1024 image with either cfg (3 + 2 + 1 + 1), for any batch size.  No
    atomics, no host synchronisation, no host-to-device copy: the call can be captured, and a replay works on whatever the buffers hold
    then.  The trees' partial lists, the decoded boxes and the NMS masks live in one workspace per (level sizes, B, nms_pre, max_per_img,
    device), every part of it written by a call before the call reads it.  Limits: rpn_proposals_supported; beyond them PswinError.
    CPU tensors: the definition."""
    anchors = list(anchors)
    if not scores.is_cuda:
        from . import detector
        return detector.proposals_batch(scores, deltas, anchors, dict(nms_pre=nms_pre, nms=iou_thr, max_per_img=max_per_img), img_hw)
    if scores.dim() != 2 or deltas.dim() != 3 or tuple(deltas.shape) != tuple(scores.shape) + (4,) or not anchors or \
            any(a.dim() != 2 or a.shape[1] != 4 or a.shape[0] < 1 for a in anchors) or sum(a.shape[0] for a in anchors) != scores.shape[1]:
        raise PswinError(f"rpn_proposals: scores [B, A], deltas [B, A, 4] and per-level anchors [n_l, 4] that sum to A, got "
                         f"{tuple(scores.shape)}, {tuple(deltas.shape)} and {[tuple(a.shape) for a in anchors]}")
    dev = scores.device
    if any(t.device != dev for t in [deltas] + anchors):
        raise PswinError("rpn_proposals: scores, deltas and anchors must be on one device")
    sizes = tuple(int(a.shape[0]) for a in anchors)
    B, L = int(scores.shape[0]), len(sizes)
    nms_pre, max_per_img, H, W = int(nms_pre), int(max_per_img), int(img_hw[0]), int(img_hw[1])
    if not rpn_proposals_supported(sizes, B, nms_pre, max_per_img):
        raise PswinError(f"rpn_proposals: outside the kernels' limits (levels <= 8, nms_pre <= 2048, P <= 2048, B L <= 2048, B A < 2^31): "
                         f"level sizes {sizes}, B = {B}, nms_pre = {nms_pre}, max_per_img = {max_per_img}")
    P = min(max_per_img, sum(min(nms_pre, n) for n in sizes))
    scores, deltas = scores.detach().float().contiguous(), deltas.detach().float().contiguous()
    flat = torch.cat([a.detach().float() for a in anchors], 0) if L > 1 else anchors[0].detach().float().contiguous()
    ns, nsp = _level_sizes(sizes)
    ws_key = ("proposals_ws", sizes, B, nms_pre, max_per_img, _dev_key(dev))
    if ws_key not in _CACHE:
        _CACHE[ws_key] = torch.empty(int(_lib.load().pswin_rpn_proposals_workspace(nsp, L, B, nms_pre, max_per_img)), dtype=torch.uint8, device=dev)
    rois = torch.empty(B, P, 4, dtype=torch.float32, device=dev)
    out_scores = torch.empty(B, P, dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    call("pswin_rpn_proposals", scores, ptr(scores), ptr(deltas), ptr(flat), nsp, L, B, nms_pre, ctypes.c_float(float(iou_thr)), max_per_img, H, W,
         ptr(rois), ptr(out_scores), ptr(count), ptr(_CACHE[ws_key]))
    return rois, out_scores, count


def _lowp_or_f32(t):
    return t if t.dtype in (torch.float32, torch.bfloat16) else t.float()


def multiclass_nms_batch(rois, roi_count, cls, deltas, stds, img_hw, scale_factor, score_thr, iou_thr, K):
    """detector.detect_post for a batch on the GPU (pswin_multiclass_nms_scores -> sort -> pswin_multiclass_nms -> sort ->
    pswin_multiclass_nms_select): (boxes f32 [B, K, 4], scores f32 [B, K], labels int64 [B, K], count int32 [B], source int32 [B, K]).
    rois f32 [B, R, 4]; roi_count int32 [B] ON THE DEVICE; cls [B, R, C + 1] and deltas [B, R, 4 C] logits, f32 or bf16; scale_factor
    f32 [B, 4] or None.  R <= 1024, C <= 128, K <= 1024.  The two sorts are torch's stable sorts, per (image, class) list and per image;
    no host-to-device copy and no host synchronisation, so the call can be captured.  CPU tensors: the definition."""
    if not cls.is_cuda:
        from . import detector
        return detector.detect_post(rois, roi_count, cls, deltas, stds, img_hw, scale_factor, score_thr, iou_thr, K)
    if cls.dim() != 3 or rois.dim() != 3 or deltas.dim() != 3 or rois.shape[2] != 4 or rois.shape[:2] != cls.shape[:2] or \
            deltas.shape[:2] != cls.shape[:2] or deltas.shape[2] != 4 * (cls.shape[2] - 1):
        raise PswinError(f"multiclass_nms_batch: rois [B, R, 4], cls [B, R, C + 1], deltas [B, R, 4 C], got {tuple(rois.shape)}, "
                         f"{tuple(cls.shape)}, {tuple(deltas.shape)}")
    B, R, C = int(cls.shape[0]), int(cls.shape[1]), int(cls.shape[2]) - 1
    dev = cls.device
    if roi_count.dtype != torch.int32 or tuple(roi_count.shape) != (B,) or roi_count.device != dev:
        raise PswinError("multiclass_nms_batch: roi_count must be an int32 [B] tensor on the device of the logits")
    if scale_factor is not None and (scale_factor.dtype != torch.float32 or tuple(scale_factor.shape) != (B, 4) or scale_factor.device != dev):
        raise PswinError("multiclass_nms_batch: scale_factor must be an f32 [B, 4] tensor on the device of the logits, or None")
    rois, roi_count = rois.detach().float().contiguous(), roi_count.contiguous()
    cls, deltas = _lowp_or_f32(cls.detach()).contiguous(), _lowp_or_f32(deltas.detach()).contiguous()
    scale = None if scale_factor is None else scale_factor.contiguous()
    nbytes = int(_lib.load().pswin_multiclass_nms_workspace(B, R, C))
    _lib.check(min(nbytes, 0), "pswin_multiclass_nms_workspace")
    key = ("detect_ws", B, R, C, _dev_key(dev))
    if key not in _CACHE:
        _CACHE[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    std4 = (ctypes.c_float * 4)(*[float(v) for v in stds])
    stdp = ctypes.cast(std4, ctypes.c_void_p)
    H, W = int(img_hw[0]), int(img_hw[1])
    keys = torch.empty(B, C, R, dtype=torch.float32, device=dev)
    call("pswin_multiclass_nms_scores", cls, ptr(cls), dtype_code(cls), ptr(roi_count), B, R, C, ctypes.c_float(float(score_thr)), ptr(keys))
    skeys, sidx = torch.sort(keys, dim=-1, descending=True, stable=True)                  # equal scores: ascending proposal
    final = torch.empty(B, R * C, dtype=torch.float32, device=dev)
    call("pswin_multiclass_nms", cls, ptr(skeys), ptr(sidx), ptr(rois), ptr(deltas), dtype_code(deltas), stdp, H, W, ptr(scale), B, R, C,
         ctypes.c_float(float(iou_thr)), ptr(final), ptr(_CACHE[key]))
    tkeys, tidx = torch.sort(final, dim=-1, descending=True, stable=True)                 # equal scores: ascending r * C + c
    K = int(K)
    boxes = torch.empty(B, K, 4, dtype=torch.float32, device=dev)
    scores = torch.empty(B, K, dtype=torch.float32, device=dev)
    labels = torch.empty(B, K, dtype=torch.int64, device=dev)
    source = torch.empty(B, K, dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    call("pswin_multiclass_nms_select", cls, ptr(tkeys), ptr(tidx), R * C, min(K, R * C), ptr(rois), ptr(deltas), dtype_code(deltas), stdp, H, W,
         ptr(scale), B, R, C, K, ptr(boxes), ptr(scores), ptr(labels), ptr(source), ptr(count))
    return boxes, scores, labels, count, source


def paste_masks(mask_logits, labels, boxes, count, thr, out_hw, out=None):
    """detector.paste_masks_batch on the GPU in one launch (pswin_paste_masks): uint8 [B, K, H, W].  mask_logits [B K, C, 28, 28], f32 or
    bf16, in any dense layout (its strides are passed on: the mask head's channels-last output is read in place); labels int64 [B, K];
    boxes f32 [B, K, 4] in the output image's pixels; count int32 [B] ON THE DEVICE.  Every byte of the output is written (zeros behind
    count[b]), so `out` may be a buffer that is reused.  CPU tensors: the definition."""
    if not mask_logits.is_cuda:
        from . import detector
        res = detector.paste_masks_batch(mask_logits, labels, boxes, count, thr, out_hw)
        return res if out is None else out.copy_(res)
    H, W = int(out_hw[0]), int(out_hw[1])
    if labels.dim() != 2 or mask_logits.dim() != 4 or tuple(mask_logits.shape[2:]) != (28, 28) or mask_logits.shape[0] != labels.numel() or \
            tuple(boxes.shape) != tuple(labels.shape) + (4,):
        raise PswinError(f"paste_masks: mask_logits [B K, C, 28, 28], labels [B, K], boxes [B, K, 4], got {tuple(mask_logits.shape)}, "
                         f"{tuple(labels.shape)}, {tuple(boxes.shape)}")
    B, K, C = int(labels.shape[0]), int(labels.shape[1]), int(mask_logits.shape[1])
    dev = mask_logits.device
    if count.dtype != torch.int32 or tuple(count.shape) != (B,) or count.device != dev or labels.dtype != torch.int64:
        raise PswinError("paste_masks: count must be an int32 [B] tensor on the device of the logits, labels int64")
    lg = _lowp_or_f32(mask_logits.detach())
    if min(lg.stride()) < 1:
        lg = lg.contiguous()
    labels, boxes, count = labels.contiguous(), boxes.detach().float().contiguous(), count.contiguous()
    if out is None:
        out = torch.empty(B, K, H, W, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, K, H, W) or not out.is_contiguous() or out.device != dev:
        raise PswinError(f"paste_masks: out must be a contiguous uint8 [{B}, {K}, {H}, {W}] tensor on the device of the logits")
    sn, sc, sy, sx = (int(v) for v in lg.stride())
    call("pswin_paste_masks", lg, ptr(lg), dtype_code(lg), sn, sc, sy, sx, ptr(labels), ptr(boxes), ptr(count), B, K, C, H, W,
         ctypes.c_float(float(thr)), ptr(out), algo_bytes=B * K * H * W)
    return out


# ------------------------------------------------------------------------------------------------
# COCO run-length encoding of masks on the GPU (csrc/pswin_rle.hip; rle.py states the format and holds the definitions)
# ------------------------------------------------------------------------------------------------
def rle_supported(n_masks, H, W, K=None, C=None):
    """Whether the RLE kernels take the shape: H, W <= 65536 and H W < 2^32 (positions are uint32, pycocotools' own limit), fewer than
    2^31 masks and, for the fused paste, its limits K <= 1024 and C <= 128."""
    return 1 <= int(n_masks) < 1 << 31 and 1 <= int(H) <= 65536 and 1 <= int(W) <= 65536 and int(H) * int(W) < 1 << 32 and \
        (K is None or 1 <= int(K) <= 1024) and (C is None or 1 <= int(C) <= 128)


def _rle_workspace(N, H, W, dev):
    key = ("rle_ws", N, H, W, _dev_key(dev))
    if key not in _CACHE:
        nbytes = ctypes.c_longlong(0)
        _lib.check(_lib.load().pswin_rle_workspace(N, H, W, ctypes.byref(nbytes)), "pswin_rle_workspace")
        _CACHE[key] = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    return _CACHE[key]


def rle_encode(masks, count=None, capacity=None, out=None):
    """rle.encode_masks on the GPU (pswin_rle_encode): uint8 [N, H, W] or [B, K, H, W] masks -> rle.RleMasks.  count int32 [B] ON THE
    DEVICE: rows past it are not read and own no runs.  Four launches whatever the batch holds; no atomics, no host synchronisation, no
    host-to-device copy: the call can be captured.  The bit-planes and the scans live in one workspace per (N, H, W, device), every part of
    it written by a call before the call reads it.  `out`: an RleMasks to reuse; nothing at or past `capacity` is written.  Limits:
    rle_supported; beyond them PswinError.  CPU tensors: the definition."""
    from . import rle
    if not masks.is_cuda:
        return rle.encode_masks_definition(masks, count, capacity, out)
    N, B, K, H, W = rle._shape_nbk(masks, count)
    dev = masks.device
    if not rle_supported(N, H, W):
        raise PswinError(f"rle_encode: outside the kernels' limits (H, W <= 65536, H W < 2^32, N < 2^31): {tuple(masks.shape)}")
    if count is not None:
        if count.device != dev:
            raise PswinError("rle_encode: count must be on the device of the masks")
        count = count.contiguous()
    out = rle._out_for(out, N, H, W, dev, capacity, B, K, count, "rle_encode")
    call("pswin_rle_encode", masks, ptr(masks), ptr(count), N, K or 1, H, W, ptr(out.offsets), ptr(out.runs), out.capacity,
         ptr(_rle_workspace(N, H, W, dev)), algo_bytes=N * H * W)
    return out


def paste_masks_rle(mask_logits, labels, boxes, count, thr, out_hw, capacity=None, out=None):
    """rle_encode(paste_masks(mask_logits, labels, boxes, count, thr, out_hw), count) without the bitmap (pswin_paste_masks_rle): the
    column bits come from the paste's own sample -- the same float32 expression, compared with thr -- so the runs equal the bitmap
    route's bit for bit.  Arguments as paste_masks (the logits' strides are passed on), capacity / out as rle_encode.  Four launches, no
    atomics, no host synchronisation: capturable.  CPU tensors: the definition."""
    from . import rle
    if not mask_logits.is_cuda:
        return rle.paste_masks_rle(mask_logits, labels, boxes, count, thr, out_hw, capacity, out)
    H, W = int(out_hw[0]), int(out_hw[1])
    if labels.dim() != 2 or mask_logits.dim() != 4 or tuple(mask_logits.shape[2:]) != (28, 28) or mask_logits.shape[0] != labels.numel() or \
            tuple(boxes.shape) != tuple(labels.shape) + (4,):
        raise PswinError(f"paste_masks_rle: mask_logits [B K, C, 28, 28], labels [B, K], boxes [B, K, 4], got {tuple(mask_logits.shape)}, "
                         f"{tuple(labels.shape)}, {tuple(boxes.shape)}")
    B, K, C = int(labels.shape[0]), int(labels.shape[1]), int(mask_logits.shape[1])
    dev = mask_logits.device
    if count.dtype != torch.int32 or tuple(count.shape) != (B,) or count.device != dev or labels.dtype != torch.int64:
        raise PswinError("paste_masks_rle: count must be an int32 [B] tensor on the device of the logits, labels int64")
    if not rle_supported(B * K, H, W, K, C) or B > 65535:
        raise PswinError(f"paste_masks_rle: outside the kernels' limits (H, W <= 65536, H W < 2^32, K <= 1024, C <= 128, B <= 65535): "
                         f"B = {B}, K = {K}, C = {C}, {H} x {W}")
    lg = _lowp_or_f32(mask_logits.detach())
    if min(lg.stride()) < 1:
        lg = lg.contiguous()
    labels, boxes, count = labels.contiguous(), boxes.detach().float().contiguous(), count.contiguous()
    out = rle._out_for(out, B * K, H, W, dev, capacity, B, K, count, "paste_masks_rle")
    sn, sc, sy, sx = (int(v) for v in lg.stride())
    call("pswin_paste_masks_rle", lg, ptr(lg), dtype_code(lg), sn, sc, sy, sx, ptr(labels), ptr(boxes), ptr(count), B, K, C, H, W,
         ctypes.c_float(float(thr)), ptr(out.offsets), ptr(out.runs), out.capacity, ptr(_rle_workspace(B * K, H, W, dev)))
    return out


# ------------------------------------------------------------------------------------------------
# test-time augmentation: the merges of tta.py on the GPU (csrc/pswin_augtest.hip)
# ------------------------------------------------------------------------------------------------
def _aug_views(views):
    """tta.View list -> (the host array of pswin_aug_view, its pointer); V <= 8"""
    if not 1 <= len(views) <= 8:
        raise PswinError(f"test-time augmentation takes 1 to 8 views, got {len(views)}")
    arr = (_lib.AugView * len(views))()
    for a, v in zip(arr, views):
        a.img_h, a.img_w, a.flip = int(v.img_hw[0]), int(v.img_hw[1]), int(bool(v.flip))
        a.scale[:] = [float(s) for s in v.scale_factor]
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _aug_out(out, what, dev, *specs):
    """the output buffers of a call: new ones, or the caller's `out` tuple checked against (shape, dtype) specs"""
    if out is None:
        return tuple(torch.empty(shape, dtype=dt, device=dev) for shape, dt in specs)
    out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
    if len(out) != len(specs) or any(o.dtype != dt or tuple(o.shape) != tuple(shape) or o.device != dev or not o.is_contiguous()
                                     for o, (shape, dt) in zip(out, specs)):
        raise PswinError(f"{what}: out must be contiguous tensors of {[(tuple(sh), dt) for sh, dt in specs]} on the inputs' device")
    return out


def aug_merge_proposals_supported(V, B, P, max_per_img):
    """Whether pswin_aug_merge_proposals takes the shape: V <= 8, V P <= 8192 and a workspace below 2^31 bytes"""
    return int(_lib.load().pswin_aug_merge_proposals_workspace(int(V), int(B), int(P), int(max_per_img))) > 0


def aug_merge_proposals_launches(V, P, max_per_img):
    """The kernel launches of one pswin_aug_merge_proposals call, whatever the batch"""
    n = int(_lib.load().pswin_aug_merge_proposals_launches(int(V), int(P), int(max_per_img)))
    _lib.check(min(n, 0), "pswin_aug_merge_proposals_launches")
    return n


def aug_merge_proposals(props, scores, count, views, iou_thr, max_per_img, out=None):
    """tta.merge_aug_proposals on the GPU, bit for bit (pswin_aug_merge_proposals: three launches): props f32 [V, B, P, 4], scores f32
    [V, B, P], count int32 [V, B] ON THE DEVICE -> (rois f32 [B, Pm, 4], scores f32 [B, Pm], count int32 [B]), Pm = min(max_per_img, V P).
    V <= 8, V P <= 8192; beyond: PswinError.  No atomics, no host synchronisation; the workspace is cached per shape and every part of it
    that a call reads the call has written.  out: (rois, scores, count) buffers to write instead of new ones (every element is written).
    CPU tensors: the definition."""
    if not props.is_cuda:
        from . import tta
        return tta.merge_aug_proposals(props, scores, count, views, iou_thr, max_per_img)
    if props.dim() != 4 or props.shape[3] != 4 or tuple(scores.shape) != tuple(props.shape[:3]) or tuple(count.shape) != tuple(props.shape[:2]) or \
            len(views) != props.shape[0]:
        raise PswinError(f"aug_merge_proposals: props [V, B, P, 4], scores [V, B, P], count [V, B] and V views, got {tuple(props.shape)}, "
                         f"{tuple(scores.shape)}, {tuple(count.shape)} and {len(views)}")
    V, B, P = (int(v) for v in props.shape[:3])
    dev = props.device
    if count.dtype != torch.int32 or count.device != dev or scores.device != dev:
        raise PswinError("aug_merge_proposals: count must be an int32 tensor on the device of the proposals")
    max_per_img = int(max_per_img)
    if not aug_merge_proposals_supported(V, B, P, max_per_img):
        raise PswinError(f"aug_merge_proposals: outside the kernels' limits (V <= 8, V P <= 8192): V = {V}, B = {B}, P = {P}")
    props, scores, count = props.detach().float().contiguous(), scores.detach().float().contiguous(), count.contiguous()
    key = ("aug_proposals_ws", V, B, P, max_per_img, _dev_key(dev))
    if key not in _CACHE:
        _CACHE[key] = torch.empty(int(_lib.load().pswin_aug_merge_proposals_workspace(V, B, P, max_per_img)), dtype=torch.uint8, device=dev)
    Pm = min(max_per_img, V * P)
    rois, out_scores, out_count = _aug_out(out, "aug_merge_proposals", dev, ((B, Pm, 4), torch.float32), ((B, Pm), torch.float32), ((B,), torch.int32))
    arr, vp = _aug_views(views)
    call("pswin_aug_merge_proposals", props, ptr(props), ptr(scores), ptr(count), vp, V, B, P, ctypes.c_float(float(iou_thr)), max_per_img,
         ptr(rois), ptr(out_scores), ptr(out_count), ptr(_CACHE[key]))
    return rois, out_scores, out_count


def aug_map_rois(boxes, views, out=None):
    """tta.map_to_view of boxes f32 [B, N, 4] into every view, bit for bit, in one launch (pswin_aug_map_rois): f32 [V, B, N, 4].
    CPU tensors: the definition."""
    if not boxes.is_cuda:
        from . import tta
        return torch.stack([tta.map_to_view(boxes, v) for v in views])
    if boxes.dim() != 3 or boxes.shape[2] != 4:
        raise PswinError(f"aug_map_rois: boxes [B, N, 4], got {tuple(boxes.shape)}")
    boxes = boxes.detach().float().contiguous()
    B, N = int(boxes.shape[0]), int(boxes.shape[1])
    out, = _aug_out(out, "aug_map_rois", boxes.device, ((len(views), B, N, 4), torch.float32))
    arr, vp = _aug_views(views)
    call("pswin_aug_map_rois", boxes, ptr(boxes), vp, len(views), B, N, ptr(out))
    return out


def aug_merge_bboxes(rois_v, cls_v, deltas_v, stds, views, out=None):
    """tta.merge_aug_bboxes on the GPU in one launch (pswin_aug_merge_bboxes): rois_v / cls_v / deltas_v are sequences of V tensors
    [B, R, 4] / [B, R, C + 1] / [B, R, 4 C] (or one stacked tensor each); cls and deltas f32 or bf16 of one dtype each, read in place ->
    (boxes f32 [B, R, 4 C], scores f32 [B, R, C + 1]).  R <= 1024, C <= 128, V <= 8.  CPU tensors: the definition."""
    rois_v, cls_v, deltas_v = list(rois_v), list(cls_v), list(deltas_v)
    if not cls_v[0].is_cuda:
        from . import tta
        return tta.merge_aug_bboxes(rois_v, cls_v, deltas_v, stds, views)
    V = len(views)
    if not (len(rois_v) == len(cls_v) == len(deltas_v) == V):
        raise PswinError(f"aug_merge_bboxes: one rois, cls and deltas tensor per view, got {len(rois_v)}, {len(cls_v)}, {len(deltas_v)} for {V} views")
    B, R, C = int(cls_v[0].shape[0]), int(cls_v[0].shape[1]), int(cls_v[0].shape[2]) - 1
    dev = cls_v[0].device
    rois_v = [r.detach().float().contiguous() for r in rois_v]
    cdt = cls_v[0].dtype if cls_v[0].dtype in (torch.float32, torch.bfloat16) else torch.float32
    ddt = deltas_v[0].dtype if deltas_v[0].dtype in (torch.float32, torch.bfloat16) else torch.float32
    cls_v = [c.detach().to(cdt).contiguous() for c in cls_v]
    deltas_v = [d.detach().to(ddt).contiguous() for d in deltas_v]
    for r, c, d in zip(rois_v, cls_v, deltas_v):
        if tuple(r.shape) != (B, R, 4) or tuple(c.shape) != (B, R, C + 1) or tuple(d.shape) != (B, R, 4 * C) or r.device != dev or d.device != dev:
            raise PswinError(f"aug_merge_bboxes: every view takes rois [B, R, 4], cls [B, R, C + 1], deltas [B, R, 4 C] on one device, got "
                             f"{tuple(r.shape)}, {tuple(c.shape)}, {tuple(d.shape)}")

    def ptrs(ts):
        a = (ctypes.c_void_p * V)(*[t.data_ptr() for t in ts])
        return a, ctypes.cast(a, ctypes.c_void_p)
    (ra, rp), (ca, cp), (da, dp) = ptrs(rois_v), ptrs(cls_v), ptrs(deltas_v)
    std4 = (ctypes.c_float * 4)(*[float(v) for v in stds])
    boxes, scores = _aug_out(out, "aug_merge_bboxes", dev, ((B, R, 4 * C), torch.float32), ((B, R, C + 1), torch.float32))
    arr, vp = _aug_views(views)
    call("pswin_aug_merge_bboxes", boxes, rp, cp, dp, dtype_code(cls_v[0]), dtype_code(deltas_v[0]), ctypes.cast(std4, ctypes.c_void_p), vp, V, B,
         R, C, ptr(boxes), ptr(scores))
    return boxes, scores


def multiclass_nms_boxes_batch(merged_boxes, merged_scores, roi_count, score_thr, iou_thr, K, out=None):
    """detector.multiclass_nms for every image of a batch on GIVEN boxes and probabilities (pswin_multiclass_nms_scores_boxes -> sort ->
    pswin_multiclass_nms_boxes -> sort -> pswin_multiclass_nms_select_boxes), the chain of multiclass_nms_batch behind its softmax and
    decode: merged_boxes f32 [B, R, 4 C], merged_scores f32 [B, R, C + 1], roi_count int32 [B] ON THE DEVICE (the first roi_count[b] rows
    of image b take part) -> (boxes f32 [B, K, 4], scores f32 [B, K], labels int64 [B, K], count int32 [B], source int32 [B, K]).
    Capturable as multiclass_nms_batch is.  CPU tensors: the definition (tta.nms_merged)."""
    if not merged_boxes.is_cuda:
        from . import tta
        return tta.nms_merged(merged_boxes, merged_scores, roi_count, score_thr, iou_thr, K)
    if merged_boxes.dim() != 3 or merged_scores.dim() != 3 or merged_boxes.shape[:2] != merged_scores.shape[:2] or \
            merged_boxes.shape[2] != 4 * (merged_scores.shape[2] - 1):
        raise PswinError(f"multiclass_nms_boxes_batch: boxes [B, R, 4 C] and scores [B, R, C + 1], got {tuple(merged_boxes.shape)}, "
                         f"{tuple(merged_scores.shape)}")
    B, R, C = int(merged_scores.shape[0]), int(merged_scores.shape[1]), int(merged_scores.shape[2]) - 1
    dev = merged_boxes.device
    if roi_count.dtype != torch.int32 or tuple(roi_count.shape) != (B,) or roi_count.device != dev:
        raise PswinError("multiclass_nms_boxes_batch: roi_count must be an int32 [B] tensor on the device of the boxes")
    mb, ms, roi_count = merged_boxes.detach().float().contiguous(), merged_scores.detach().float().contiguous(), roi_count.contiguous()
    nbytes = int(_lib.load().pswin_multiclass_nms_workspace(B, R, C))
    _lib.check(min(nbytes, 0), "pswin_multiclass_nms_workspace")
    key = ("detect_ws", B, R, C, _dev_key(dev))
    if key not in _CACHE:
        _CACHE[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    keys = torch.empty(B, C, R, dtype=torch.float32, device=dev)
    call("pswin_multiclass_nms_scores_boxes", mb, ptr(ms), ptr(roi_count), B, R, C, ctypes.c_float(float(score_thr)), ptr(keys))
    skeys, sidx = torch.sort(keys, dim=-1, descending=True, stable=True)                  # equal scores: ascending proposal
    final = torch.empty(B, R * C, dtype=torch.float32, device=dev)
    call("pswin_multiclass_nms_boxes", mb, ptr(skeys), ptr(sidx), ptr(mb), B, R, C, ctypes.c_float(float(iou_thr)), ptr(final), ptr(_CACHE[key]))
    tkeys, tidx = torch.sort(final, dim=-1, descending=True, stable=True)                 # equal scores: ascending r * C + c
    K = int(K)
    boxes, scores, labels, count, source = _aug_out(out, "multiclass_nms_boxes_batch", dev, ((B, K, 4), torch.float32), ((B, K), torch.float32),
                                                    ((B, K), torch.int64), ((B,), torch.int32), ((B, K), torch.int32))
    call("pswin_multiclass_nms_select_boxes", mb, ptr(tkeys), ptr(tidx), R * C, min(K, R * C), ptr(mb), B, R, C, K, ptr(boxes), ptr(scores),
         ptr(labels), ptr(source), ptr(count))
    return boxes, scores, labels, count, source


def paste_masks_aug(logit_list, flips, labels, boxes, count, thr, out_hw, out=None):
    """paste_masks of tta.merge_aug_masks(logit_list, flips, labels) in one launch (pswin_paste_masks_aug): uint8 [B, K, H, W].  logit_list:
    up to 24 tensors [B K, C, 28, 28] of one dtype (f32 or bf16), each in any dense layout (its strides are passed on); flips: one bool
    per source.  The merged probability is never written to memory.  Everything else as paste_masks.  CPU tensors: the definition."""
    logit_list, flips = list(logit_list), [bool(f) for f in flips]
    if not logit_list[0].is_cuda:
        from . import detector, tta
        prob = tta.merge_aug_masks(logit_list, flips, labels)
        B, K = labels.shape
        res = torch.zeros(B, K, int(out_hw[0]), int(out_hw[1]), dtype=torch.uint8)
        for b, n in enumerate(count.tolist()):
            if n:
                res[b, :n] = detector.paste_masks(prob.reshape(B, K, 28, 28)[b, :n], boxes[b, :n].float(), int(out_hw[0]), int(out_hw[1]), thr)
        return res if out is None else out.copy_(res)
    N = len(logit_list)
    if not 1 <= N <= 24 or len(flips) != N:
        raise PswinError(f"paste_masks_aug: 1 to 24 mask sources and one flip flag each, got {N} and {len(flips)}")
    H, W = int(out_hw[0]), int(out_hw[1])
    B, K, C = int(labels.shape[0]), int(labels.shape[1]), int(logit_list[0].shape[1])
    dev = logit_list[0].device
    dt = logit_list[0].dtype if logit_list[0].dtype in (torch.float32, torch.bfloat16) else torch.float32
    srcs = []
    for l in logit_list:
        if l.dim() != 4 or tuple(l.shape) != (B * K, C, 28, 28) or l.device != dev:
            raise PswinError(f"paste_masks_aug: every source is [B K, C, 28, 28] = {(B * K, C, 28, 28)} on one device, got {tuple(l.shape)}")
        l = l.detach().to(dt)
        srcs.append(l if min(l.stride()) >= 1 else l.contiguous())
    if labels.dim() != 2 or tuple(boxes.shape) != (B, K, 4) or count.dtype != torch.int32 or tuple(count.shape) != (B,) or count.device != dev or \
            labels.dtype != torch.int64:
        raise PswinError("paste_masks_aug: labels int64 [B, K], boxes [B, K, 4], count int32 [B] on the device of the logits")
    labels, boxes, count = labels.contiguous(), boxes.detach().float().contiguous(), count.contiguous()
    if out is None:
        out = torch.empty(B, K, H, W, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, K, H, W) or not out.is_contiguous() or out.device != dev:
        raise PswinError(f"paste_masks_aug: out must be a contiguous uint8 [{B}, {K}, {H}, {W}] tensor on the device of the logits")
    st = _lib.AugMaskSources()
    st.count = N
    for i, (l, f) in enumerate(zip(srcs, flips)):
        st.logits[i], st.flip[i] = l.data_ptr(), int(f)
        st.stride_n[i], st.stride_c[i], st.stride_y[i], st.stride_x[i] = (int(v) for v in l.stride())
    call("pswin_paste_masks_aug", srcs[0], ctypes.byref(st), dtype_code(srcs[0]), ptr(labels), ptr(boxes), ptr(count), B, K, C, H, W,
         ctypes.c_float(float(thr)), ptr(out), algo_bytes=B * K * H * W)
    return out


def roi_targets_ranked(gt_inds, key, cand, gt, gt_labels, num_classes, n_pos_max, n_tot, stds):
    """cascade.roi_targets_ranked on the GPU: roi_targets' five results and pos_rank int64 [B, n_pos_max], the ranks they were drawn by
    (pswin_sample_ranks once, then one launch of pswin_roi_targets on those ranks).  Arguments and limits as roi_targets; capturable as
    sample_ranks is.  CPU tensors: the definition."""
    if not gt_inds.is_cuda:
        from . import cascade
        return cascade.roi_targets_ranked(gt_inds, key, cand, gt, gt_labels, num_classes, n_pos_max, n_tot, stds)
    gt_inds, key = _sample_inputs("roi_targets_ranked", gt_inds, key)
    B, N = (int(v) for v in gt_inds.shape)
    dev = key.device
    if tuple(cand.shape) != (B, N, 4) or gt.dim() != 3 or gt.shape[0] != B or gt.shape[2] != 4 or tuple(gt_labels.shape) != tuple(gt.shape[:2]) or \
            gt_labels.dtype != torch.int64 or any(t.device != dev for t in (cand, gt, gt_labels)):
        raise PswinError(f"roi_targets_ranked: cand [{B}, {N}, 4], gt [{B}, Gmax, 4] and int64 gt_labels [{B}, Gmax] on the device of gt_inds, got "
                         f"{tuple(cand.shape)}, {tuple(gt.shape)} and {tuple(gt_labels.shape)} {gt_labels.dtype}")
    n_pos_max, n_tot, Gmax = int(n_pos_max), int(n_tot), int(gt.shape[1])
    cand, gt, gt_labels = cand.detach().float().contiguous(), gt.detach().float().contiguous(), gt_labels.contiguous()
    pos_rank, neg_order = sample_ranks(gt_inds, key, n_pos_max, n_tot)
    rois = torch.empty(B, n_tot, 4, dtype=torch.float32, device=dev)
    labels = torch.empty(B, n_tot, dtype=torch.int64, device=dev)
    reg_t = torch.empty(B, n_pos_max, 4, dtype=torch.float32, device=dev)
    pos_valid = torch.empty(B, n_pos_max, dtype=torch.uint8, device=dev)
    gt_idx = torch.empty(B, n_pos_max, dtype=torch.int64, device=dev)
    std4 = (ctypes.c_float * 4)(*[float(v) for v in stds])
    call("pswin_roi_targets", key, ptr(gt_inds), ptr(pos_rank), ptr(neg_order), ptr(cand), ptr(gt), ptr(gt_labels), B, N, Gmax, n_pos_max, n_tot,
         int(num_classes), ctypes.cast(std4, ctypes.c_void_p), ptr(rois), ptr(labels), ptr(reg_t), ptr(pos_valid), ptr(gt_idx))
    return rois, labels, reg_t, pos_valid.view(torch.bool), gt_idx, pos_rank


def cascade_rows_per_workgroup():
    """The rows one workgroup of pswin_cascade_refine / pswin_giou_rows_fwd / _bwd takes"""
    return int(_lib.load().pswin_cascade_rows_per_workgroup())


def refine_rois(rois, cls, deltas, labels, stds, img_hw):
    """cascade.refine_rois on the GPU in one launch (pswin_cascade_refine): (new_rois f32 [B, R, 4], used int64 [B, R]).  rois f32
    [B, R, 4]; cls [B, R, C + 1] and deltas [B, R, 4 C], f32 or bf16, read in place (the box head's bf16 output under autocast is not
    copied); labels int64 [B, R] or None.  C <= 128.  The argmax is torch.argmax's on the same values, ties included.  No gradient, no
    host synchronisation: the call can be captured.  CPU tensors: the definition."""
    if not cls.is_cuda:
        from . import cascade
        return cascade.refine_rois(rois, cls, deltas, labels, stds, img_hw)
    if cls.dim() != 3 or tuple(rois.shape) != tuple(cls.shape[:2]) + (4,) or deltas.dim() != 3 or deltas.shape[:2] != cls.shape[:2] or \
            deltas.shape[2] != 4 * (cls.shape[2] - 1) or cls.shape[2] < 2:
        raise PswinError(f"refine_rois: rois [B, R, 4], cls [B, R, C + 1], deltas [B, R, 4 C], got {tuple(rois.shape)}, {tuple(cls.shape)}, "
                         f"{tuple(deltas.shape)}")
    B, R, C = int(cls.shape[0]), int(cls.shape[1]), int(cls.shape[2]) - 1
    dev = cls.device
    if labels is not None and (labels.dtype != torch.int64 or tuple(labels.shape) != (B, R) or labels.device != dev):
        raise PswinError(f"refine_rois: labels must be an int64 [{B}, {R}] tensor on the device of the logits, or None")
    if rois.device != dev or deltas.device != dev:
        raise PswinError("refine_rois: rois, cls and deltas must be on one device")
    rois = rois.detach().float().contiguous()
    cls, deltas = _lowp_or_f32(cls.detach()).contiguous(), _lowp_or_f32(deltas.detach()).contiguous()
    labels = None if labels is None else labels.contiguous()
    new_rois = torch.empty(B, R, 4, dtype=torch.float32, device=dev)
    used = torch.empty(B, R, dtype=torch.int64, device=dev)
    std4 = (ctypes.c_float * 4)(*[float(v) for v in stds])
    call("pswin_cascade_refine", cls, ptr(rois), ptr(cls), dtype_code(cls), ptr(deltas), dtype_code(deltas), ptr(labels), B, R, C,
         ctypes.cast(std4, ctypes.c_void_p), int(img_hw[0]), int(img_hw[1]), ptr(new_rois), ptr(used),
         algo_bytes=B * R * (C * cls.element_size() + 4 * deltas.element_size() + 16 + 16 + 8))
    return new_rois, used


class _GIoURows(torch.autograd.Function):
    """cascade.giou_rows as one node: the forward launch writes the [N] rows; the backward launch recomputes the forward from the saved
    INPUTS (nothing else is kept) and writes every element of the [N, 4 C] gradient in the dtype of `deltas` -- no float copy of the
    prediction, no zero fill, no scatter."""

    @staticmethod
    def forward(ctx, rois, deltas, labels, weight, target, stds, eps):
        N, C = int(deltas.shape[0]), int(deltas.shape[1]) // 4
        out = torch.empty(N, dtype=torch.float32, device=deltas.device)
        std4 = (ctypes.c_float * 4)(*[float(v) for v in stds])
        call("pswin_giou_rows_fwd", deltas, ptr(rois), ptr(deltas), dtype_code(deltas), ptr(labels), ptr(weight), ptr(target), N, C,
             ctypes.cast(std4, ctypes.c_void_p), ctypes.c_double(float(eps)), ptr(out), algo_bytes=N * (4 * deltas.element_size() + 48))
        ctx.save_for_backward(rois, deltas, labels, weight, target)
        ctx.cfg = (tuple(float(v) for v in stds), float(eps))
        return out

    @staticmethod
    def backward(ctx, grad_rows):
        rois, deltas, labels, weight, target = ctx.saved_tensors
        stds, eps = ctx.cfg
        N, C = int(deltas.shape[0]), int(deltas.shape[1]) // 4
        grad_rows = grad_rows.float().contiguous()
        grad = torch.empty_like(deltas)
        std4 = (ctypes.c_float * 4)(*stds)
        call("pswin_giou_rows_bwd", deltas, ptr(rois), ptr(deltas), dtype_code(deltas), ptr(labels), ptr(weight), ptr(target), ptr(grad_rows), N, C,
             ctypes.cast(std4, ctypes.c_void_p), ctypes.c_double(eps), ptr(grad), algo_bytes=N * (4 * C + 4) * deltas.element_size() + N * 52)
        return None, grad, None, None, None, None, None


def giou_rows(rois, deltas, labels, weight, target, stds, eps=1e-6):
    """cascade.giou_rows on the GPU (pswin_giou_rows_fwd, and pswin_giou_rows_bwd for the gradient of `deltas`): f32 [N] = weight *
    (1 - GIoU(decoded box, target)).  rois f32 [N, 4]; deltas [N, 4 C], f32 or bf16, read in place and the only input with a gradient;
    labels int64 [N]; weight f32 [N]; target f32 [N, 4].  C <= 128.  One launch per direction, no atomics, no host synchronisation: the
    call can be captured.  CPU tensors: the definition."""
    if not deltas.is_cuda:
        from . import cascade
        return cascade.giou_rows(rois, deltas, labels, weight, target, stds, eps)
    if deltas.dim() != 2 or deltas.shape[1] % 4 or deltas.shape[1] < 4 or tuple(rois.shape) != (deltas.shape[0], 4) or \
            tuple(target.shape) != tuple(rois.shape) or tuple(labels.shape) != (deltas.shape[0],) or tuple(weight.shape) != tuple(labels.shape) or \
            labels.dtype != torch.int64 or any(t.device != deltas.device for t in (rois, labels, weight, target)):
        raise PswinError(f"giou_rows: rois [N, 4], deltas [N, 4 C], int64 labels [N], weight [N], target [N, 4] on one device, got "
                         f"{tuple(rois.shape)}, {tuple(deltas.shape)}, {tuple(labels.shape)} {labels.dtype}, {tuple(weight.shape)}, {tuple(target.shape)}")
    if deltas.dtype not in (torch.float32, torch.bfloat16):
        raise PswinError(f"giou_rows: deltas must be float32 or bfloat16, got {deltas.dtype}")
    return _GIoURows.apply(rois.detach().float().contiguous(), deltas.contiguous(), labels.contiguous(), weight.detach().float().contiguous(),
                           target.detach().float().contiguous(), stds, eps)


# ------------------------------------------------------------------------------------------------
# the detector's training losses, row by row (csrc/pswin_losses.hip; definitions: losses.py)
# ------------------------------------------------------------------------------------------------
# off: ce_rows / l1_rows / mask_bce_rows / rpn_losses evaluate the torch definitions of losses.py on the GPU
LOSS_KERNELS = _on("loss_kernels")


def losses_rows_per_workgroup():
    """The rows one workgroup of the ce_rows / l1_rows kernels takes"""
    return int(_lib.load().pswin_losses_rows_per_workgroup())


def rpn_losses_chunk():
    """The anchors one workgroup of pswin_rpn_losses_bwd owns"""
    return int(_lib.load().pswin_rpn_losses_chunk())


def _loss_input(name, what, t):
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise PswinError(f"{name}: {what} must be float32 or bfloat16, got {t.dtype}")


class _CERows(torch.autograd.Function):
    """losses.ce_rows as one node: only the inputs are saved, the backward launch recomputes the row statistics and writes every element of
    the [N, C + 1] gradient in the dtype of `cls`."""

    @staticmethod
    def forward(ctx, cls, labels):
        N, C = int(cls.shape[0]), int(cls.shape[1]) - 1
        out = torch.empty(N, dtype=torch.float32, device=cls.device)
        call("pswin_ce_rows_fwd", cls, ptr(cls), dtype_code(cls), ptr(labels), N, C, ptr(out), algo_bytes=N * ((C + 1) * cls.element_size() + 12))
        ctx.save_for_backward(cls, labels)
        return out

    @staticmethod
    def backward(ctx, grad_rows):
        cls, labels = ctx.saved_tensors
        N, C = int(cls.shape[0]), int(cls.shape[1]) - 1
        grad_rows = grad_rows.float().contiguous()
        grad = torch.empty_like(cls)
        call("pswin_ce_rows_bwd", cls, ptr(cls), dtype_code(cls), ptr(labels), ptr(grad_rows), N, C, ptr(grad),
             algo_bytes=N * (2 * (C + 1) * cls.element_size() + 12))
        return grad, None


def ce_rows(cls, labels):
    """losses.ce_rows on the GPU (pswin_ce_rows_fwd, and pswin_ce_rows_bwd for the gradient of `cls`): f32 [N] = logsumexp(row) -
    row[label].  cls [N, C + 1], f32 or bf16, read in place; labels int64 [N], a label outside [0, C] gives a zero row.  C <= 128.  One
    launch per direction, no atomics, no host synchronisation: the call can be captured.  CPU tensors: the definition."""
    if not cls.is_cuda or not LOSS_KERNELS:
        from . import losses
        return losses.ce_rows(cls, labels)
    if cls.dim() != 2 or cls.shape[1] < 2 or tuple(labels.shape) != (cls.shape[0],) or labels.dtype != torch.int64 or labels.device != cls.device:
        raise PswinError(f"ce_rows: cls [N, C + 1] and int64 labels [N] on one device, got {tuple(cls.shape)}, {tuple(labels.shape)} {labels.dtype}")
    _loss_input("ce_rows", "cls", cls)
    return _CERows.apply(cls.contiguous(), labels.contiguous())


class _L1Rows(torch.autograd.Function):
    """losses.l1_rows as one node, as _GIoURows: inputs saved, every element of the [N, 4 C] gradient written in the dtype of `reg`."""

    @staticmethod
    def forward(ctx, reg, labels, weight, target):
        N, C = int(reg.shape[0]), int(reg.shape[1]) // 4
        out = torch.empty(N, dtype=torch.float32, device=reg.device)
        call("pswin_l1_rows_fwd", reg, ptr(reg), dtype_code(reg), ptr(labels), ptr(weight), ptr(target), N, C, ptr(out),
             algo_bytes=N * (4 * reg.element_size() + 32))
        ctx.save_for_backward(reg, labels, weight, target)
        return out

    @staticmethod
    def backward(ctx, grad_rows):
        reg, labels, weight, target = ctx.saved_tensors
        N, C = int(reg.shape[0]), int(reg.shape[1]) // 4
        grad_rows = grad_rows.float().contiguous()
        grad = torch.empty_like(reg)
        call("pswin_l1_rows_bwd", reg, ptr(reg), dtype_code(reg), ptr(labels), ptr(weight), ptr(target), ptr(grad_rows), N, C, ptr(grad),
             algo_bytes=N * (4 * C + 4) * reg.element_size() + N * 36)
        return grad, None, None, None


def l1_rows(reg, labels, weight, target):
    """losses.l1_rows on the GPU (pswin_l1_rows_fwd / _bwd): f32 [N] = weight * sum_4 |reg[n, 4 lab : 4 lab + 4] - target[n]|.  reg
    [N, 4 C], f32 or bf16, read in place and the only input with a gradient; labels int64 [N] (clamped to [0, C)); weight f32 [N]; target
    f32 [N, 4].  C <= 128.  Capturable as giou_rows is.  CPU tensors: the definition."""
    if not reg.is_cuda or not LOSS_KERNELS:
        from . import losses
        return losses.l1_rows(reg, labels, weight, target)
    if reg.dim() != 2 or reg.shape[1] % 4 or reg.shape[1] < 4 or tuple(target.shape) != (reg.shape[0], 4) or tuple(labels.shape) != (reg.shape[0],) or \
            tuple(weight.shape) != tuple(labels.shape) or labels.dtype != torch.int64 or any(t.device != reg.device for t in (labels, weight, target)):
        raise PswinError(f"l1_rows: reg [N, 4 C], int64 labels [N], weight [N], target [N, 4] on one device, got {tuple(reg.shape)}, "
                         f"{tuple(labels.shape)} {labels.dtype}, {tuple(weight.shape)}, {tuple(target.shape)}")
    _loss_input("l1_rows", "reg", reg)
    return _L1Rows.apply(reg.contiguous(), labels.contiguous(), weight.detach().float().contiguous(), target.detach().float().contiguous())


def _mask_strides(logits):
    """the element strides of dense [M, C, S, S] logits as pswin_mask_bce_rows_* takes them (a channel dimension of size 1 may carry any
    stride: the NCHW ones are passed), or None if the memory is neither NCHW nor channels-last"""
    M, C, S, _ = (int(v) for v in logits.shape)
    if logits.is_contiguous():
        return C * S * S, S * S, S, 1
    if logits.is_contiguous(memory_format=torch.channels_last):
        return C * S * S, 1, S * C, C
    return None


class _MaskBCERows(torch.autograd.Function):
    """losses.mask_bce_rows as one node: the forward reads the label's channel through the logits' strides and leaves it as f32 [M, S, S];
    that copy (1 / C of the logits) is what is saved -- the C-channel logits are NOT kept alive until the backward -- and the backward
    writes every element of a gradient with the logits' shape, dtype and strides in memory order."""

    @staticmethod
    def forward(ctx, logits, labels, target, weight):
        M, C, S, _ = (int(v) for v in logits.shape)
        out = torch.empty(M, dtype=torch.float32, device=logits.device)
        picked = torch.empty(M, S, S, dtype=torch.float32, device=logits.device) if ctx.needs_input_grad[0] else None
        call("pswin_mask_bce_rows_fwd", logits, ptr(logits), dtype_code(logits), *_mask_strides(logits), ptr(labels), ptr(target), ptr(weight), M, C, S,
             ptr(out), ptr(picked), algo_bytes=M * (S * S * (logits.element_size() + 8) + 16))
        ctx.save_for_backward(picked, labels, target, weight)
        ctx.like = (logits.shape, logits.stride(), logits.dtype, _mask_strides(logits))
        return out

    @staticmethod
    def backward(ctx, grad_rows):
        picked, labels, target, weight = ctx.saved_tensors
        shape, stride, dtype, strides = ctx.like
        M, C, S, _ = (int(v) for v in shape)
        grad_rows = grad_rows.float().contiguous()
        grad = torch.empty_strided(shape, stride, dtype=dtype, device=picked.device)
        call("pswin_mask_bce_rows_bwd", grad, ptr(picked), dtype_code(grad), *strides, ptr(labels), ptr(target), ptr(weight), ptr(grad_rows), M, C, S,
             ptr(grad), algo_bytes=M * (S * S * (C * grad.element_size() + 8) + 20))
        return grad, None, None, None


def mask_bce_rows(logits, labels, target, weight):
    """losses.mask_bce_rows on the GPU (pswin_mask_bce_rows_fwd / _bwd): f32 [M] = weight * mean over the map of BCE-with-logits of
    logits[m, lab_m] against target[m].  logits [M, C, S, S], f32 or bf16, NCHW or channels-last memory, read in place (any other memory is
    copied to NCHW first) and the only input with a gradient, which has the logits' strides; labels int64 [M] (clamped to [0, C)); target
    f32 [M, S, S]; weight f32 [M].  C <= 128, S <= 56.  Capturable.  CPU tensors: the definition."""
    if not logits.is_cuda or not LOSS_KERNELS:
        from . import losses
        return losses.mask_bce_rows(logits, labels, target, weight)
    if logits.dim() != 4 or logits.shape[2] != logits.shape[3] or tuple(target.shape) != (logits.shape[0],) + tuple(logits.shape[2:]) or \
            tuple(labels.shape) != (logits.shape[0],) or tuple(weight.shape) != tuple(labels.shape) or labels.dtype != torch.int64 or \
            any(t.device != logits.device for t in (labels, target, weight)):
        raise PswinError(f"mask_bce_rows: logits [M, C, S, S], int64 labels [M], target [M, S, S], weight [M] on one device, got "
                         f"{tuple(logits.shape)}, {tuple(labels.shape)} {labels.dtype}, {tuple(target.shape)}, {tuple(weight.shape)}")
    _loss_input("mask_bce_rows", "logits", logits)
    if _mask_strides(logits) is None:
        logits = logits.contiguous()
    return _MaskBCERows.apply(logits, labels.contiguous(), target.detach().float().contiguous(), weight.detach().float().contiguous())


class _RpnLosses(torch.autograd.Function):
    """losses.rpn_losses as one node: the backward launch writes every element of both [B, A] and [B, A, 4] gradients -- the sampled values
    at the valid slots' anchors, zeros everywhere else -- without a zero fill or a scatter."""

    @staticmethod
    def forward(ctx, cls_all, reg_all, idx, valid, pos_valid, reg_t):
        (B, A), S, P = (int(v) for v in cls_all.shape), int(idx.shape[1]), int(pos_valid.shape[1])
        out = torch.empty(B, 2, dtype=torch.float32, device=cls_all.device)
        call("pswin_rpn_losses_fwd", cls_all, ptr(cls_all), ptr(reg_all), ptr(idx), ptr(valid), ptr(pos_valid), ptr(reg_t), B, A, S, P, ptr(out),
             algo_bytes=B * (S * 16 + P * 33))
        ctx.save_for_backward(cls_all, reg_all, idx, valid, pos_valid, reg_t)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        cls_all, reg_all, idx, valid, pos_valid, reg_t = ctx.saved_tensors
        (B, A), S, P = (int(v) for v in cls_all.shape), int(idx.shape[1]), int(pos_valid.shape[1])
        grad_out = grad_out.float().contiguous()
        grad_cls, grad_reg = torch.empty_like(cls_all), torch.empty_like(reg_all)
        call("pswin_rpn_losses_bwd", cls_all, ptr(cls_all), ptr(reg_all), ptr(idx), ptr(valid), ptr(pos_valid), ptr(reg_t), ptr(grad_out), B, A, S, P,
             ptr(grad_cls), ptr(grad_reg), algo_bytes=B * A * 20)
        return grad_cls, grad_reg, None, None, None, None


def rpn_losses(cls_all, reg_all, idx, valid, pos_valid, reg_t):
    """losses.rpn_losses on the GPU (pswin_rpn_losses_fwd / _bwd): f32 [B, 2], the class BCE and the box L1 of every image's sampled
    anchors, each divided by max(the image's valid slots, 1).  cls_all f32 [B, A] and reg_all f32 [B, A, 4] (the inputs with a gradient);
    idx int64 [B, S], valid f32 [B, S], pos_valid bool [B, P], reg_t f32 [B, P, 4]: what rpn_targets returns, P <= S.  Capturable.
    CPU tensors: the definition."""
    if not cls_all.is_cuda or not LOSS_KERNELS:
        from . import losses
        return losses.rpn_losses(cls_all, reg_all, idx, valid, pos_valid, reg_t)
    ok = cls_all.dim() == 2 and tuple(reg_all.shape) == tuple(cls_all.shape) + (4,) and idx.dim() == 2 and idx.shape[0] == cls_all.shape[0] and \
        tuple(valid.shape) == tuple(idx.shape) and pos_valid.dim() == 2 and pos_valid.shape[0] == idx.shape[0] and \
        1 <= pos_valid.shape[1] <= idx.shape[1] and tuple(reg_t.shape) == tuple(pos_valid.shape) + (4,)
    if not ok or idx.dtype != torch.int64 or pos_valid.dtype not in (torch.bool, torch.uint8) or cls_all.dtype != torch.float32 or \
            reg_all.dtype != torch.float32 or any(t.device != cls_all.device for t in (reg_all, idx, valid, pos_valid, reg_t)):
        raise PswinError(f"rpn_losses: float32 cls_all [B, A] and reg_all [B, A, 4], int64 idx [B, S], valid [B, S], bool pos_valid [B, P], reg_t "
                         f"[B, P, 4], P <= S, on one device, got {tuple(cls_all.shape)} {cls_all.dtype}, {tuple(reg_all.shape)} {reg_all.dtype}, "
                         f"{tuple(idx.shape)} {idx.dtype}, {tuple(valid.shape)}, {tuple(pos_valid.shape)} {pos_valid.dtype}, {tuple(reg_t.shape)}")
    return _RpnLosses.apply(cls_all.contiguous(), reg_all.contiguous(), idx.contiguous(), valid.detach().float().contiguous(),
                            pos_valid.contiguous().view(torch.uint8), reg_t.detach().float().contiguous())


# ------------------------------------------------------------------------------------------------
# qkv Linear + attention core in one kernel for C = 192 / 384 (pswin_qkv_attn_fused_fwd, round 3)
# ------------------------------------------------------------------------------------------------
# off: the unfused chain qkv GEMM -> pswin_attn_fwd
FUSED_QKV_ATTENTION = _on("fused_qkv_attention")


class _WindowAttentionQkvFused(torch.autograd.Function):
    """self.qkv(x) and the attention core of WindowAttention.forward (HOT:287-308) as ONE kernel per (window, head) wave; the proj
    Linear stays with the caller.  Training mode stores q, k, v (packed [n, heads, 3, 49, 32]) and the log-sum-exp rows; the backward
    pass is the unfused one on them (pswin_attn_bwd_ex, then the qkv weight / data gradients): identical kernels and summation order
    to the unfused path."""

    @staticmethod
    def forward(ctx, x, w_qkv, b_qkv, alpha, beta, dist, mask, heads, scale, n_bias_windows, wq_lp, wq_lp_t, grad_mode, live=None):
        x = x.contiguous()
        rows, C = x.shape
        n = rows // WTOK
        assert rows % WTOK == 0 and C == heads * _lib.HEAD_DIM
        ctx.live = live                                     # sample liveness of the window rows: for the qkv weight gradient
        wq = (wq_lp if wq_lp is not None else w_qkv.to(x.dtype)).contiguous()
        bq = None if b_qkv is None else b_qkv.detach().float().contiguous()
        alpha_c = alpha.detach().contiguous() if dist is not None else None
        beta_c = beta.detach().contiguous()
        save = grad_mode and any(ctx.needs_input_grad)
        y = torch.empty_like(x)
        qkv = lse = None
        if save:
            qkv = torch.empty(n, heads, 3, WTOK, _lib.HEAD_DIM, dtype=x.dtype, device=x.device)
            lse = torch.empty(n, heads, WPAD, dtype=torch.float32, device=x.device)
        flops = n * (2 * WTOK * C * 3 * C + heads * 4 * WTOK * WTOK * _lib.HEAD_DIM)
        call("pswin_qkv_attn_fused_fwd", x, ptr(x), ptr(wq), ptr(bq), ptr(None if dist is None else dist.fwd), 0 if dist is None else dist.n,
             ptr(alpha_c), ptr(beta_c), ptr(None if mask is None else mask.fwd), 0 if mask is None else mask.n, ptr(y), ptr(qkv), ptr(lse), n,
             n_bias_windows, C, heads, float(scale), dtype_code(x), algo_bytes=rows * C * 2 * (5 if save else 2), algo_flops=flops)
        if save:
            ctx.save_for_backward(x, qkv, lse, wq, alpha_c, beta_c, wq_lp_t)
            ctx.params = (w_qkv, b_qkv, alpha if dist is not None else None, beta)
            ctx.cfg = (dist, mask, heads, float(scale), n_bias_windows)
        return y

    @staticmethod
    def backward(ctx, datt):
        x, qkv, lse, wq, alpha_c, beta_c, wq_t = ctx.saved_tensors
        w_qkv, b_qkv, alpha, beta = ctx.params
        dist, mask, heads, scale, nb = ctx.cfg
        C = x.shape[1]
        dqkv, _, _, dalpha, dbeta = attention_backward(qkv, None, None, lse, alpha_c, beta_c, dist, mask, datt, heads, scale, nb, None,
                                                        ctx.needs_input_grad[3] or ctx.needs_input_grad[4], (alpha, beta), packed=True)
        # the K third of d(qkv) sums to zero over every window (rows of dS sum to 0): its bias gradient is not summed
        dx, dwq, dbq = linear_backward(x, wq, dqkv, w_qkv, b_qkv, (C, 2 * C), ctx.needs_input_grad[0], wq_t, wgrad_live=ctx.live)
        return dx, dwq, dbq, dalpha, dbeta, None, None, None, None, None, None, None, None, None


def window_attention_qkv_fused_supported(x2d, heads):
    return (FUSED_QKV_ATTENTION and x2d.is_cuda and x2d.dim() == 2 and x2d.dtype == torch.bfloat16
            and fused_windows_addressable(x2d.shape[0] // WTOK, x2d.shape[1])
            and bool(_lib.load().pswin_qkv_attn_fused_supported(x2d.shape[1], heads, BF16)))


def window_attention_qkv_fused(x2d, attn, dist, mask, n_bias_windows, live=None):
    """attention(qkv(x2d)) -- everything of WindowAttention.forward in front of self.proj -- for window rows x2d [n*49, C] and the
    parameter holder `attn`: see _WindowAttentionQkvFused.  live: the rows' sample liveness (sample_liveness) for the weight gradient."""
    wq_lp, _, wq_lp_t = _lowp(attn.qkv)
    return _WindowAttentionQkvFused.apply(x2d, attn.qkv.weight, attn.qkv.bias, attn.sphere_position_alpha_table_Te,
                                          attn.sphere_position_beta_table_Te, _as_tiles(dist), _as_tiles(mask), attn.num_heads, attn.scale,
                                          n_bias_windows, wq_lp, wq_lp_t, torch.is_grad_enabled(), live)
