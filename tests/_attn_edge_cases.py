"""Inputs for the window-attention tests (tests/test_kernels_gpu.py, tests/test_attention_edges.py, tests/test_attention_edges_gpu.py):
the random cases the kernel tests have always used, and three kinds of input whose answer is known better than "close to the oracle".

One-hot rows: an additive mask that is 0 at ONE key of every query row and -100 (the reference's own mask value) at the other 48.  The
softmax weight of the selected key is then 1 to 1e-20, so the output row is the selected V row, dV is the sum of the dO rows that selected
the key, and dQ = dK = 0.  Families (select_keys): "perm" (row i of window w selects key (i + w) % 49: with 49 windows every (row, key) pair
occurs once, key 48 and the zero-padded uv slots included), "column" (every row of window w selects key w: 49 rows accumulate into one dV
row, the other 48 are zero) and "image" (a per-image table: row i of window (b, w) selects key (i + 7 w + 3 b) % 49).

Row offsets: a per-row constant out of ROW_OFFSETS added to all 49 keys of a row.  Softmax does not change; a kernel that subtracts a wrong
row maximum overflows (+100) or loses the row (-100, the reference's fully masked row).

The rounding model: attention64 evaluates the attention in float64 and, given `rnd`, rounds where the bf16 kernels round, so that the error
of a kernel can be judged against the error its rounding points explain (fused_model: the same for the qkv -> attention (-> proj) kernels)."""
import copy
import math

import torch

import panoswin_oracle as po
from detfill import det_uniform

DEV = "cuda:0"
TOK = 49
MASKED = -100.0
ROW_OFFSETS = (100.0, -100.0, 0.0, 37.5)

# (family, n_rep, nW, chunks): chunks = 1 puts all n_rep images of a bias window into one work item (batch loop + prefetch path)
CORE_ONEHOT = [("perm", 2, 49, None), ("column", 1, 49, None), ("image", 2, 7, None)]
CORE_ONEHOT_LOOP = ("perm", 4, 49, 1)
# (family, B, nW, pano)
FUSED_ONEHOT = [("perm", 2, 49, True), ("column", 1, 49, False), ("image", 2, 7, False)]
# the random cases of the row-offset and rounding-model tests: subsets of the parameter lists of tests/test_kernels_gpu.py
CORE_RANDOM = [(2, 3, 2, True, 0), (2, 3, 3, False, 3), (2, 3, 2, False, 4)]                 # (n_rep, nW, heads, pano, mask_kind)
FUSED_RANDOM = [(96, 2, 3, True, 0), (96, 3, 4, False, 3), (96, 2, 3, False, 4),
                (192, 2, 3, True, 0), (192, 3, 4, False, 3), (192, 2, 3, False, 4)]           # (C, B, nW, pano, mask_kind)
FUSED_MODEL = [(96, 2, 3, True, 0), (96, 3, 4, False, 3), (192, 2, 3, True, 0), (192, 3, 4, False, 3), (384, 2, 3, True, 0),
               (384, 2, 3, False, 3)]


# ---- the random cases -----------------------------------------------------------------------------------------------------------------
def _attn_case(n_rep, nW, heads, pano, mask_kind, seed):
    C = heads * 32
    n = n_rep * nW
    x = det_uniform((n * 49, 3 * C), f"att:{seed}:qkv", 1.5)
    alpha = det_uniform((169, heads), f"att:{seed}:a", 0.3)
    beta = det_uniform((169, heads), f"att:{seed}:b", 0.3)
    uv = torch.stack([det_uniform((nW, 49), f"att:{seed}:u", math.pi), det_uniform((nW, 49), f"att:{seed}:v", math.pi / 2)], -1)
    uv[0, 45:] = 0.0
    dist = po.haversine(uv, uv) if pano else None
    mask = None
    if mask_kind == 3:
        mask = torch.where(det_uniform((nW, 49, 49), f"att:{seed}:m") > 0.4, torch.tensor(-100.0), torch.tensor(0.0))
    elif mask_kind == 4:
        mask = torch.where(det_uniform((n_rep, nW, 49, 49), f"att:{seed}:m4") > 0.4, torch.tensor(-100.0), torch.tensor(0.0))
    gout = det_uniform((n * 49, C), f"att:{seed}:g", 1.0)
    return x, alpha, beta, dist, mask, gout


def _attn_oracle(x, alpha, beta, dist, mask, gout, heads, n_rep, nW):
    C = heads * 32
    x = x.clone().requires_grad_(True)
    alpha, beta = alpha.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    idx = po.relative_position_index(7).reshape(-1)
    b = beta[idx].reshape(49, 49, heads)
    if dist is not None:
        bias = dist[..., None] * alpha[idx].reshape(49, 49, heads)[None] + b
        bias = bias.repeat(n_rep, 1, 1, 1)
    else:
        bias = b[None]
    qkv = x.view(-1, 49, 3, C)
    out = po.window_attention_core(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], 32 ** -0.5, bias.permute(0, 3, 1, 2), mask,
                                   heads, 0.0, False).reshape(-1, C)
    (out * gout).sum().backward()
    return out.detach(), x.grad, alpha.grad, beta.grad


def _fused_case(B, nW, pano, mask_kind, seed, C=96):
    from detfill import det_fill_module
    att = po.WindowAttention(C, 7, C // 32)
    det_fill_module(att, f"fz:{seed}")
    with torch.no_grad():                       # the kernel's operands are bf16: the oracle sees the same rounded weights
        for lin in (att.qkv, att.proj):
            lin.weight.copy_(lin.weight.to(torch.bfloat16).float())
    n = B * nW
    x = det_uniform((n, 49, C), f"fz:{seed}:x", 1.0).to(torch.bfloat16).float()
    uv = torch.stack([det_uniform((nW, 49), f"fz:{seed}:u", math.pi), det_uniform((nW, 49), f"fz:{seed}:v", math.pi / 2)], -1)
    uv[0, 44:] = 0.0                            # zero-uv padding slots
    mask = None
    if mask_kind == 3:
        mask = torch.where(det_uniform((nW, 49, 49), f"fz:{seed}:m") > 0.4, torch.tensor(-100.0), torch.tensor(0.0))
    elif mask_kind == 4:
        mask = torch.where(det_uniform((B, nW, 49, 49), f"fz:{seed}:m4") > 0.4, torch.tensor(-100.0), torch.tensor(0.0))
    gout = det_uniform((n, 49, C), f"fz:{seed}:g", 1.0).to(torch.bfloat16).float()
    return att, x, uv, mask, gout


def _fused_run(ops, att_cpu, x, uv, mask, gout, B, nW, pano, mask_kind, fused, C=96):
    """The product's WindowAttention chain on the GPU in bf16: the fused kernel (C = 96: with the proj Linear; C = 192 / 384: qkv +
    attention core, then the proj GEMM) or the three-kernel chain."""
    from panoswintransformerobjectdetection_amd.backbone import WindowAttention, _linear
    heads = C // 32
    att = WindowAttention(C, 7, heads)
    att.load_state_dict(att_cpu.state_dict())
    att = att.to(DEV)
    xd = x.to(DEV).to(torch.bfloat16).view(-1, C).requires_grad_(True)
    uvd = uv.to(DEV)
    dist = ops.Tiles(ops.haversine_windows(uvd, uvd), symmetric=True) if pano else None
    mt = None if mask is None else ops.Tiles(mask.reshape(-1, 49, 49).to(DEV))
    nb = B * nW if mask_kind == 4 else nW
    if fused and C == 96:
        y = ops.window_attention_fused(xd, att, dist, mt, nb)
    elif fused:
        assert ops.window_attention_qkv_fused_supported(xd, heads)
        y = _linear(ops.window_attention_qkv_fused(xd, att, dist, mt, nb), att.proj, torch.bfloat16, use_bias=False)
    else:
        qkv = _linear(xd, att.qkv, torch.bfloat16)
        o = ops.window_attention(qkv, att.sphere_position_alpha_table_Te, att.sphere_position_beta_table_Te, dist, mt, heads,
                                 att.scale, nb)
        y = _linear(o, att.proj, torch.bfloat16, use_bias=False)
    y.backward(gout.to(DEV).to(torch.bfloat16).view(-1, C))
    grads = {k: p.grad.detach().float().cpu() for k, p in att.named_parameters() if p.grad is not None}
    return y.detach().float().cpu(), xd.grad.float().cpu(), grads


# ---- one-hot rows ---------------------------------------------------------------------------------------------------------------------
def select_keys(family, n_rep, nW):
    """-> (sel [n_tables, 49] long: the key that row i of bias window t selects, mask_kind of the table: 3 per window, 4 per image)"""
    i = torch.arange(TOK)
    w = torch.arange(nW)[:, None]
    if family == "perm":
        return (i[None] + w) % TOK, 3
    if family == "column":
        return (w % TOK).expand(nW, TOK).contiguous(), 3
    assert family == "image"
    b = torch.arange(n_rep)[:, None, None]
    return ((i[None, None] + 7 * w[None] + 3 * b) % TOK).reshape(n_rep * nW, TOK), 4


def onehot_mask(sel):
    """[n_tables, 49, 49] float: 0 at (row, selected key), -100 everywhere else"""
    return torch.full((sel.shape[0], TOK, TOK), MASKED).scatter_(2, sel[..., None], 0.0)


def selected_rows(sel, n):
    """flat row index n' * 49 + sel(n', i) of the V row that output row (n', i) must equal; window n' uses table n' % n_tables"""
    wsel = sel.repeat(n // sel.shape[0], 1)
    return (torch.arange(n)[:, None] * TOK + wsel).reshape(-1)


def oracle_mask(mask, mask_kind, n_rep, nW):
    """the table in the shape the oracle wants: [nW, 49, 49] or [B, nW, 49, 49]"""
    return mask.reshape(n_rep, nW, TOK, TOK) if mask_kind == 4 else mask


def unselected_weight(p, sel):
    """p [n, heads, 49, 49] softmax weights -> the largest summed weight of the 48 unselected keys of a row, and the largest single one"""
    n = p.shape[0]
    wsel = sel.repeat(n // sel.shape[0], 1)[:, None, :, None].expand(n, p.shape[1], TOK, 1)
    rest = p.scatter(3, wsel, 0.0)
    return rest.sum(-1).max().item(), rest.max().item()


def table_grad_scale(dout, v, sel, heads, dist):
    """What a dS of the order of dP at the selected entries would leave in the tables, in float64: per table bin and head the sum of
    |dP(i, sel(i))| = |dO[i] . v[sel(i)]| (times the distance for alpha).  -> (largest alpha entry or None, largest beta entry)"""
    n = dout.shape[0] // TOK
    rows = selected_rows(sel, n)
    d = v.shape[1] // heads
    dp = (dout.double().view(-1, heads, d) * v.double()[rows].view(-1, heads, d)).sum(-1).abs()
    i = torch.arange(TOK).repeat(n)
    j = rows % TOK
    bins = po.relative_position_index(7)[i, j]
    gb = torch.zeros(169, heads, dtype=torch.float64).index_add_(0, bins, dp)
    ga = None
    if dist is not None:
        wd = dist.double()[torch.arange(n).repeat_interleave(TOK) % dist.shape[0], i, j]
        ga = torch.zeros(169, heads, dtype=torch.float64).index_add_(0, bins, dp * wd[:, None]).max().item()
    return ga, gb.max().item()


# ---- row offsets ----------------------------------------------------------------------------------------------------------------------
def row_offset_mask(mask, nW):
    """mask (or a zero table [nW, 49, 49]) + ROW_OFFSETS[i % 4] on all 49 keys of query row i"""
    base = torch.zeros(nW, TOK, TOK) if mask is None else mask
    c = torch.tensor(ROW_OFFSETS)[torch.arange(TOK) % len(ROW_OFFSETS)]
    return base + c[:, None]


# ---- float64 evaluation, with the kernels' rounding points on request --------------------------------------------------------------------
def bf16_round(t):
    """round to nearest even, the mode of every f32 -> bf16 conversion in the kernels (the kernels round f32 values: so does this)"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def core_bias(alpha, beta, dist, heads, n_rep):
    """[1 | n, heads, 49, 49] float64: d * alpha[idx] + beta[idx] (pano) or beta[idx]"""
    idx = po.relative_position_index(7).reshape(-1)
    b = beta.double()[idx].reshape(TOK, TOK, heads)
    if dist is None:
        return b[None].permute(0, 3, 1, 2)
    bias = dist.double()[..., None] * alpha.double()[idx].reshape(TOK, TOK, heads)[None] + b
    return bias.repeat(n_rep, 1, 1, 1).permute(0, 3, 1, 2)


def attention64(q, k, v, scale, bias, mask, heads, rnd=None, l_rounded=False):
    """softmax(scale q k^T + bias + mask) v in float64.  q, k, v [n, 49, C]; bias [1 | n, heads, 49, 49]; mask None or any shape
    [.., 49, 49] with n_tables tables in all (window n uses table n % n_tables).  rnd: applied to the weights exp(s - max) before the
    product with v and to the output, as the bf16 kernels do; l_rounded: the denominator is the sum of the ROUNDED weights (the fused
    kernels: a column of ones in the P.V product) instead of the unrounded ones (the core kernel).  -> (out [n, 49, C], weights)"""
    n, O, C = q.shape
    d = C // heads
    split = lambda t: t.double().reshape(n, O, heads, d).permute(0, 2, 1, 3)
    s = (split(q) @ split(k).transpose(-2, -1)) * scale + bias
    if mask is not None:
        m = mask.double().reshape(-1, O, O)
        s = s + m.repeat(n // m.shape[0], 1, 1)[:, None]
    p = torch.exp(s - s.amax(-1, keepdim=True))
    pr = rnd(p) if rnd else p
    o = (pr @ split(v)) / (pr if l_rounded else p).sum(-1, keepdim=True)
    o = o.transpose(1, 2).reshape(n, O, C)
    return (rnd(o) if rnd else o), p / p.sum(-1, keepdim=True)


def fused_v64(att, x):
    """[n * 49, C] float64: the V rows x Wv^T + b_v of the module's qkv Linear"""
    C = x.shape[-1]
    return x.double().reshape(-1, C) @ att.qkv.weight.double()[2 * C:].T + att.qkv.bias.double()[2 * C:]


def fused_model(att, x, uv, mask, pano, B, rnd=None):
    """The WindowAttention module in float64 -> (attention rows [n * 49, C], proj_nobias of them, softmax weights).  rnd: applied where
    the fused kernels round: qkv after the Linear, the weights, the attention rows, the proj output."""
    n, _, C = x.shape
    r = rnd or (lambda t: t)
    qkv = r(x.double().reshape(-1, C) @ att.qkv.weight.double().T + att.qkv.bias.double()).reshape(n, TOK, 3, C)
    dist = po.haversine(uv.double(), uv.double()) if pano else None
    bias = att.bias(dist, pano).detach().double()
    if pano:
        bias = bias.repeat(B, 1, 1, 1)
    o, p = attention64(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], att.scale, bias, mask, att.heads, rnd, l_rounded=True)
    o = o.reshape(-1, C)
    return o, r(o @ att.proj.weight.double().T), p


def module_oracle(att, x, uv, mask, pano, gout, B):
    """The oracle module in float64, without the proj bias (the kernels leave it to the residual kernel) -> (y, dx, parameter gradients)"""
    m = copy.deepcopy(att).double()
    xo = x.double().clone().requires_grad_(True)
    yo = m(xo, uv.double().repeat(B, 1, 1), mask, pano) - m.proj.bias
    (yo * gout.double()).sum().backward()
    return yo.detach(), xo.grad, {k: p.grad for k, p in m.named_parameters() if p.grad is not None}


def err_stats(got, model, truth):
    """(rms(got - truth), rms(model - truth), max|got - truth|, max|model - truth|)"""
    a, b = got.double() - truth, model - truth
    return a.pow(2).mean().sqrt().item(), b.pow(2).mean().sqrt().item(), a.abs().max().item(), b.abs().max().item()


# ---- the cases as the CPU and the GPU tests both build them ----------------------------------------------------------------------------
def core_onehot_case(family, n_rep, nW, heads, pano, bf16):
    """-> x, alpha, beta, dist, mask [n_tables, 49, 49], gout, sel, mask_kind: q, k, v, tables and distances of _attn_case, one-hot mask"""
    x, alpha, beta, dist, _, gout = _attn_case(n_rep, nW, heads, pano, 0, f"oh:{family}{n_rep}{nW}{heads}")
    if bf16:
        x, gout = x.to(torch.bfloat16).float(), gout.to(torch.bfloat16).float()
    sel, kind = select_keys(family, n_rep, nW)
    return x, alpha, beta, dist, onehot_mask(sel), gout, sel, kind


def fused_onehot_case(family, B, nW, pano, C):
    """-> att, x, uv, mask [n_tables, 49, 49], gout, sel, mask_kind: module, input and uv of _fused_case, one-hot mask"""
    att, x, uv, _, gout = _fused_case(B, nW, pano, 0, f"oh:{family}{C}{B}{nW}", C)
    sel, kind = select_keys(family, B, nW)
    return att, x, uv, onehot_mask(sel), gout, sel, kind
