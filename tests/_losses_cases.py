"""Shared inputs of tests/test_losses.py and tests/test_losses_gpu.py (CPU tensors, built once and never written to), the expressions the
models evaluated before the loss kernels existed (`*_before`: the torch statements of detector.py / cascade.py at that commit), and the
error rule both files hold the row operations to."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

ROWS = 64          # pswin_losses_rows_per_workgroup(): asserted by the tests that build sizes around it
CHUNK = 4096       # pswin_rpn_losses_chunk(): likewise


def bf16_exact(t):
    return t.to(torch.bfloat16).float()


def row_sizes(rows=ROWS):
    return (1, rows - 1, rows + 1, 3 * rows + 5)


# ---- the error rule --------------------------------------------------------------------------------------------------------------------
def ulp32(t):
    """the float32 ulp of every |element| of a float64 tensor (the spacing of 0 is the smallest denormal)"""
    return torch.from_numpy(np.spacing(np.abs(t.double().numpy()).astype(np.float32)).astype(np.float64)).reshape(t.shape)


def half_ulp_bf16(t):
    """half a bfloat16 ulp of every |element|: bf16 keeps 8 significant bits, so half an ulp of v is 2^(e - 8) for 2^e <= |v| < 2^(e + 1)"""
    mag = t.double().abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(mag)) - 8)


def within(got, f32, truth, what, bf16=False):
    """Element by element: |got - truth| <= max(4 e32, 4 ulp32(|truth|)) with e32 = |f32 - truth| the float32 CPU definition's own error
    on that element, plus half a bf16 ulp of the truth where `got` was rounded to bf16.  NaN / inf never pass.  Prints and returns
    (the largest error of got, the largest error of the float32 definition)."""
    got, f32, truth = got.detach().double().cpu(), f32.detach().double().cpu(), truth.detach().double().cpu()
    assert got.shape == truth.shape == f32.shape, (what, got.shape, truth.shape)
    assert bool(torch.isfinite(got).all()), what
    e32 = (f32 - truth).abs()
    bound = torch.maximum(4 * e32, 4 * ulp32(truth))
    if bf16:
        bound = bound + half_ulp_bf16(truth)
    err = (got - truth).abs()
    worst = float(err.max()) if err.numel() else 0.0
    print(f"{what}: kernel error {worst:.3e} / float32 definition {float(e32.max()):.3e} (largest value {float(truth.abs().max()):.3e})")
    bad = err > bound
    assert not bool(bad.any()), (what, int(bad.sum()), float((err - bound).max()))
    return worst, float(e32.max())


# ---- ce_rows -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ce_case(N, C1, seed=0):
    """(cls [N, C1] bf16-exact, labels, upstream): random logits, and from N >= 9 the planted rows -- 0 / 1: one logit at +80 and the
    rest at -80 (label on it / off it); 2: all logits equal at about 3e4; 3: bf16 ties (a grid of 1 / 4 with the maximum twice); 4 / 5:
    labels 0 and C; 6 / 7: labels -1 and C + 1 (zero rows); 8: label far outside"""
    g = torch.Generator().manual_seed(300 + seed + 11 * N + C1)
    cls = torch.randn(N, C1, generator=g) * 3
    labels = torch.randint(0, C1, (N,), generator=g)
    cls[0] = -80.0
    cls[0, C1 // 2] = 80.0
    labels[0] = C1 // 2
    if N >= 9:
        cls[1] = cls[0]
        labels[1] = (C1 // 2 + 1) % C1
        cls[2] = 3e4
        cls[3] = torch.round(cls[3] * 4) / 4
        cls[3, 0] = cls[3, C1 - 1] = float(cls[3].max())
        labels[4], labels[5], labels[6], labels[7], labels[8] = 0, C1 - 1, -1, C1, 1 << 40
    return bf16_exact(cls), labels, torch.rand(N, generator=g) + 0.5


# ---- l1_rows -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def l1_case(N, C, seed=0):
    """(reg [N, 4 C] bf16-exact, labels, weight, target, upstream): about a third of the weights 0; from N >= 9: rows 0 / 1 equal their
    target exactly in one coordinate (sign(0) = 0), rows 2 / 3 have weight 0 and hold inf / NaN in the prediction and the target, rows
    4 / 5 carry labels below 0 and above C - 1 (clamped)"""
    g = torch.Generator().manual_seed(400 + seed + 11 * N + C)
    reg = bf16_exact(torch.randn(N, 4 * C, generator=g))
    labels = torch.randint(0, C, (N,), generator=g)
    weight = (torch.rand(N, generator=g) + 0.5) * (torch.rand(N, generator=g) > 0.35).float()
    target = bf16_exact(torch.randn(N, 4, generator=g))
    if N >= 9:
        weight[:6] = torch.tensor([1.0, 0.75, 0.0, 0.0, 1.25, 1.0])
        labels[4], labels[5] = -3, C + 5
        target[0, 1] = reg[0, 4 * int(labels[0]) + 1]
        target[1, 3] = reg[1, 4 * int(labels[1]) + 3]
        reg[2] = float("inf")
        reg[3, ::2] = float("nan")
        target[3, 0], target[2, 2] = float("nan"), float("-inf")
    else:
        weight[0] = 1.0
    return reg, labels, weight.float(), target, torch.rand(N, generator=g) + 0.5


# ---- mask_bce_rows -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mask_case(M, C, S, seed=0):
    """(logits [M, C, S, S] bf16-exact NCHW, labels, target, weight, upstream): logits of scale 8 with +-60 planted, 0 / 1 targets; from
    M >= 3: row 1 has weight 0 and NaN logits in every channel, row 2 a label above C - 1 (clamped); from M > 3 a third of the weights 0
    and a label below 0"""
    g = torch.Generator().manual_seed(500 + seed + 11 * M + 3 * C + S)
    logits = torch.randn(M, C, S, S, generator=g) * 8
    logits[:, :, 0, 0], logits[:, :, S - 1, S - 1], logits[:, :, 0, S - 1] = 60.0, -60.0, 0.0
    labels = torch.randint(0, C, (M,), generator=g)
    target = (torch.rand(M, S, S, generator=g) > 0.5).float()
    weight = torch.ones(M)
    if M > 3:
        weight = (torch.rand(M, generator=g) > 0.35).float()
        weight[0], weight[2], weight[3] = 1.0, 1.0, 1.0
        labels[3] = -2
    if M >= 3:
        weight[1] = 0.0
        logits[1] = float("nan")
        labels[2] = C + 3
    return bf16_exact(logits), labels, target, weight, torch.rand(M, generator=g) + 0.5


# ---- rpn_losses --------------------------------------------------------------------------------------------------------------------------
RPN_B, RPN_P, RPN_S = 3, 8, 24


@functools.lru_cache(maxsize=None)
def rpn_case(A, chunk=CHUNK, seed=0):
    """(cls_all [3, A], reg_all [3, A, 4], idx [3, 24], valid, pos_valid [3, 8], reg_t [3, 8, 4], upstream [3, 2]).
    Image 0: positives in slots 0-4 on the first and the last anchor and on both sides of the first chunk boundary (A > chunk; otherwise
    in the middle), valid negatives in slots 8-17; its invalid slots REPEAT the first and the last anchor, and one holds an index outside
    [0, A).  Image 1 has no valid slot (its indices point at real anchors).  Image 2: random distinct anchors, 6 positives, all 16
    negatives.  One positive of images 0 and 2 equals its target exactly in one coordinate."""
    g = torch.Generator().manual_seed(600 + seed + A)
    B, P, S = RPN_B, RPN_P, RPN_S
    cls_all, reg_all = torch.randn(B, A, generator=g) * 3, torch.randn(B, A, 4, generator=g)
    idx = torch.stack([torch.randperm(A, generator=g)[:S] for _ in range(B)])
    edge = chunk if A > chunk else A // 2
    lead = list(dict.fromkeys([0, A - 1, edge - 1, edge]))                                      # (A = chunk + 1: the last anchor IS past the edge)
    idx[0] = torch.tensor(lead + [a for a in idx[0].tolist() if a not in lead][:S - len(lead)])
    valid, pos_valid = torch.zeros(B, S), torch.zeros(B, P, dtype=torch.bool)
    pos_valid[0, :5], valid[0, :5], valid[0, 8:18] = True, 1.0, 1.0
    idx[0, 5], idx[0, 6], idx[0, 7], idx[0, 18], idx[0, 19] = 0, A - 1, A + 5, edge, -1          # invalid slots: repeats and out of range
    pos_valid[2, :6], valid[2, :6], valid[2, 8:] = True, 1.0, 1.0
    reg_t = torch.randn(B, P, 4, generator=g)
    reg_t[0, 1, 2] = reg_all[0, idx[0, 1], 2]
    reg_t[2, 0, 0] = reg_all[2, idx[2, 0], 0]
    return cls_all, reg_all, idx, valid, pos_valid, reg_t, torch.rand(B, 2, generator=g) + 0.5


# ---- the models' expressions before the kernels --------------------------------------------------------------------------------------
def rpn_loss_before(cls_all, reg_all, idx, valid, pos_valid, d_t):
    B, n_pos_max, n_tot = cls_all.shape[0], pos_valid.shape[1], idx.shape[1] - pos_valid.shape[1]
    loss_cls = loss_reg = cls_all.new_zeros(())
    tgt = torch.cat([torch.ones(n_pos_max), torch.zeros(n_tot)]).to(cls_all.dtype)
    avg = valid.sum(1).clamp(min=1)
    bce = F.binary_cross_entropy_with_logits(cls_all.gather(1, idx), tgt[None].expand(B, -1), reduction="none")
    l_cls = (bce * valid).sum(1) / avg
    reg_p = reg_all.gather(1, idx[:, :n_pos_max, None].expand(-1, -1, 4))
    l_reg = ((reg_p - d_t).abs().sum(2) * pos_valid.to(cls_all.dtype)).sum(1) / avg
    for b in range(B):
        loss_cls, loss_reg = loss_cls + l_cls[b], loss_reg + l_reg[b]
    return loss_cls / B, loss_reg / B


def cls_loss_before(cls, labels_c):
    return F.cross_entropy(cls, labels_c)


def box_loss_before(reg, labels_b, reg_t, pos_valid):
    (B, n_tot), n_pos_max, C = labels_b.shape, pos_valid.shape[1], reg.shape[1] // 4
    labels_c, reg_t, pv = labels_b.reshape(-1), reg_t.reshape(-1, 4), pos_valid.reshape(-1).to(reg.dtype)
    pos_sel = torch.cat([torch.arange(n_pos_max) + b * n_tot for b in range(B)])
    pl = labels_c[pos_sel].clamp(max=C - 1)
    ar = torch.arange(pos_sel.numel())
    reg_p = reg[pos_sel].view(-1, C, 4)[ar, pl]
    return ((reg_p - reg_t).abs().sum(1) * pv).sum() / (B * n_tot)


def mask_loss_before(logits, pl, mt, pv):
    logit_c = logits[torch.arange(pl.numel()), pl]
    lm = F.binary_cross_entropy_with_logits(logit_c, mt, reduction="none").mean((1, 2))
    return (lm * pv).sum() / pv.sum().clamp(min=1)


# ---- a head-shaped case for the four compositions --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def heads_case(seed=0):
    """What the hooks of one tiny step see: B = 2 images, n_tot = 24 sampled rows of which the first n_pos_max = 6 are positive slots,
    C = 5 classes, 7 x 7 masks, 300 anchors with 8 + 24 RPN slots (in-range, distinct anchors per image: rpn_targets' contract)."""
    g = torch.Generator().manual_seed(700 + seed)
    B, n_tot, P, C, S, A = 2, 24, 6, 5, 7, 300
    pos_valid = torch.tensor([[True, True, True, True, False, False], [True, False, False, False, False, False]])
    labels_b = torch.full((B, n_tot), C)
    labels_b[:, :P] = torch.where(pos_valid, torch.randint(0, C, (B, P), generator=g), torch.full((B, P), C))
    d = dict(cls=torch.randn(B * n_tot, C + 1, generator=g) * 2, reg=torch.randn(B * n_tot, 4 * C, generator=g), labels_b=labels_b,
             reg_t=torch.randn(B, P, 4, generator=g) * pos_valid[:, :, None], pos_valid=pos_valid,
             logits=torch.randn(B * P, C, S, S, generator=g) * 3, pl=labels_b[:, :P].reshape(-1).clamp(max=C - 1),
             mt=(torch.rand(B * P, S, S, generator=g) > 0.5).float() * pos_valid.reshape(-1)[:, None, None], pv=pos_valid.reshape(-1).float(),
             cls_all=torch.randn(B, A, generator=g) * 2, reg_all=torch.randn(B, A, 4, generator=g),
             idx=torch.stack([torch.randperm(A, generator=g)[:32] for _ in range(B)]), rpn_reg_t=torch.randn(B, 8, 4, generator=g))
    d["rpn_pos_valid"] = torch.tensor([[True] * 5 + [False] * 3, [False] * 8])
    d["valid"] = torch.cat([d["rpn_pos_valid"].float(), torch.tensor([[1.0] * 19 + [0.0] * 5, [1.0] * 24])], 1)
    d["rpn_reg_t"] = d["rpn_reg_t"] * d["rpn_pos_valid"][:, :, None]
    return d
