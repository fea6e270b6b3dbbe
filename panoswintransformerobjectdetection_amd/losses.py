"""The detector's training losses between "targets built" and "backward through the heads": the five losses of detector.MiniMaskRCNN and
the class and mask losses of cascade.MiniCascadeRCNN's stages.

Every loss is a ROW operation and the small sum that remains.  Each row operation has a DEFINITION in plain torch here (CPU and GPU;
`dtype=` is the arithmetic, so float64 is the truth the tests measure errors against) and runs on the GPU as one HIP launch per direction
(csrc/pswin_losses.hip through ops.ce_rows / l1_rows / mask_bce_rows / rpn_losses): the heads' bf16 outputs are read in place, every
element of a gradient is written once by plain stores -- no float copy of the logits, no zero fill, no scatter, no atomics.

  ce_rows        CrossEntropyLoss, row by row: logsumexp(row) - row[label]
  l1_rows        L1Loss behind BBoxHead.loss on the deltas of the row's class: weight * sum_4 |reg[4 label ..] - target|
  mask_bce_rows  FCNMaskHead.loss: weight * mean over the map of BCE-with-logits on the label's channel
  rpn_losses     AnchorHead.loss_single of the sampled anchors, per image: the class BCE and the box L1, each divided by the image's samples

The `*_dispatch` functions are what the models call through their hooks (MiniMaskRCNN.rpn_loss / cls_loss / box_loss / mask_loss): on
CUDA tensors the kernel and the sum that remains, on CPU tensors the expression the models evaluated before the kernels existed,
statement by statement (`*_loss_torch`).  The `*_definition` functions compose the row definitions exactly as the dispatch functions
compose the kernels: the tests and tools/bench_losses.py substitute them for the hooks to compare the two on the GPU."""
import torch
import torch.nn.functional as F


def _zero(dtype, device):
    return torch.zeros((), dtype=dtype, device=device)


# ------------------------------------------------------------------------------------------------------------------------
# row definitions
# ------------------------------------------------------------------------------------------------------------------------
def ce_rows(cls, labels, dtype=torch.float32):
    """Softmax cross-entropy of every row: cls [N, C + 1] (any float dtype), labels long [N] -> [N] = logsumexp(row) - row[label], the
    row's maximum subtracted from every logit first.  A label outside [0, C] makes its row contribute exactly 0 and receive an all-zero
    gradient row.  Differentiable in `cls`.  dtype: the arithmetic; the result is of that dtype."""
    C1 = cls.shape[1]
    on = (labels >= 0) & (labels < C1)
    x = cls.to(dtype)
    z = x - x.detach().max(1, keepdim=True)[0]                    # shifted first: at logits of 3e4 the difference to the label survives
    rows = z.exp().sum(1).log() - z.gather(1, labels.clamp(0, C1 - 1)[:, None])[:, 0]
    return torch.where(on, rows, _zero(dtype, cls.device))


def l1_rows(reg, labels, weight, target, dtype=torch.float32):
    """Class-selected L1 of every row: reg [N, 4 C] (any float dtype), labels long [N], weight f32 [N], target f32 [N, 4] -> [N] =
    weight * sum_4 |reg[n, 4 lab : 4 lab + 4] - target[n]|.  Labels are clamped to [0, C).  A row whose weight is 0 contributes exactly 0
    and receives a zero gradient whatever its numbers are (infinities and NaNs included): its inputs are replaced before anything is
    computed from them.  The gradient in the label's columns is sign(reg - target) * (weight * upstream), sign(0) = 0.  Differentiable
    in `reg`."""
    N, C = reg.shape[0], reg.shape[1] // 4
    on = weight != 0
    zero = _zero(dtype, reg.device)
    r4 = reg.reshape(N, C, 4)[torch.arange(N, device=reg.device), labels.clamp(0, C - 1)].to(dtype)
    r4 = torch.where(on[:, None], r4, zero)
    tgt = torch.where(on[:, None], target.to(dtype), zero)
    w = torch.where(on, weight.to(dtype), zero)
    return torch.where(on, w * (r4 - tgt).abs().sum(1), zero)


def mask_bce_rows(logits, labels, target, weight, dtype=torch.float32):
    """BCE-with-logits on the label's channel: logits [M, C, S, S] (any float dtype, any strides), labels long [M], target f32 [M, S, S] of
    0 / 1, weight f32 [M] -> [M] = weight * mean over the map of F.binary_cross_entropy_with_logits(logits[m, lab_m], target[m]).
    Labels are clamped to [0, C); weight-0 rows as in l1_rows.  Differentiable in `logits`."""
    M, C = logits.shape[:2]
    on = weight != 0
    zero = _zero(dtype, logits.device)
    x = logits[torch.arange(M, device=logits.device), labels.clamp(0, C - 1)].to(dtype)
    x = torch.where(on[:, None, None], x, zero)
    t = torch.where(on[:, None, None], target.to(dtype), zero)
    w = torch.where(on, weight.to(dtype), zero)
    rows = w * F.binary_cross_entropy_with_logits(x, t, reduction="none").mean((1, 2))
    return torch.where(on, rows, zero)


def rpn_losses(cls_all, reg_all, idx, valid, pos_valid, reg_t, dtype=torch.float32):
    """The RPN's two losses per image on what detector.rpn_targets returns: cls_all f32 [B, A], reg_all f32 [B, A, 4], idx long [B, S],
    valid f32 [B, S], pos_valid bool [B, P], reg_t f32 [B, P, 4], P <= S -> [B, 2]:
      [b, 0] = sum_s valid * BCE(cls_all[b, idx[b, s]], s < P ? 1 : 0) / avg_b,  [b, 1] = sum_{p < P} pos_valid * sum_4 |reg_all[b, idx[b, p]]
      - reg_t[b, p]| / avg_b,  avg_b = max(sum_s valid, 1).
    A slot whose valid (pos_valid) is 0 or whose index is outside [0, A) is skipped: whatever the tensors hold there, it contributes 0,
    receives no gradient and does not count in avg_b.  Differentiable in cls_all and reg_all."""
    A, S, P = cls_all.shape[1], idx.shape[1], pos_valid.shape[1]
    zero = _zero(dtype, cls_all.device)
    inside = (idx >= 0) & (idx < A)
    safe = idx.clamp(0, A - 1)
    v = torch.where(inside, valid.to(dtype), zero)
    x = torch.where(v != 0, cls_all.to(dtype).gather(1, safe), zero)
    tgt = torch.cat([torch.ones(P, dtype=dtype, device=idx.device), torch.zeros(S - P, dtype=dtype, device=idx.device)])
    avg = v.sum(1).clamp(min=1)
    l_cls = (F.binary_cross_entropy_with_logits(x, tgt[None].expand_as(x), reduction="none") * v).sum(1) / avg
    pv = pos_valid & inside[:, :P]
    diff = reg_all.to(dtype).gather(1, safe[:, :P, None].expand(-1, -1, 4)) - reg_t.to(dtype)
    l_reg = torch.where(pv[:, :, None], diff, zero).abs().sum(2).sum(1) / avg
    return torch.stack([l_cls, l_reg], 1)


# ------------------------------------------------------------------------------------------------------------------------
# what remains behind the rows
# ------------------------------------------------------------------------------------------------------------------------
def rpn_loss_of_rows(rows):
    """(loss_rpn_cls, loss_rpn_bbox) from rpn_losses' [B, 2]: summed over the images in image order, divided by B"""
    tot = rows[0]
    for b in range(1, rows.shape[0]):
        tot = tot + rows[b]
    tot = tot / rows.shape[0]
    return tot[0], tot[1]


def _all_rows(pos_valid, reg_t, n_tot):
    """weight f32 [B n_tot] and target f32 [B n_tot, 4] of ALL sampled rows: pos_valid / reg_t in the first n_pos_max rows of every image,
    zeros behind them (as MiniCascadeRCNN._stage_losses builds them)"""
    B, n_pos_max = pos_valid.shape
    with torch.no_grad():
        weight = torch.cat([pos_valid.float(), pos_valid.new_zeros(B, n_tot - n_pos_max, dtype=torch.float32)], 1).reshape(-1)
        target = torch.cat([reg_t.reshape(B, n_pos_max, 4), reg_t.new_zeros(B, n_tot - n_pos_max, 4)], 1).reshape(-1, 4)
    return weight, target


def _rpn_loss(fn, cls_all, reg_all, idx, valid, pos_valid, reg_t):
    return rpn_loss_of_rows(fn(cls_all, reg_all, idx, valid, pos_valid, reg_t))


def _cls_loss(fn, cls, labels):
    return fn(cls, labels).sum() / cls.shape[0]


def _box_loss(fn, reg, labels_b, reg_t, pos_valid):
    B, n_tot = labels_b.shape
    weight, target = _all_rows(pos_valid, reg_t, n_tot)
    return fn(reg, labels_b.reshape(-1), weight, target).sum() / (B * n_tot)


def _mask_loss(fn, logits, labels, target, pv):
    return fn(logits, labels, target, pv).sum() / pv.sum().clamp(min=1)


# ------------------------------------------------------------------------------------------------------------------------
# the expressions of the models before the kernels (the CPU path: unchanged, statement by statement)
# ------------------------------------------------------------------------------------------------------------------------
def rpn_loss_torch(cls_all, reg_all, idx, valid, pos_valid, d_t):
    B, n_pos_max, n_tot = cls_all.shape[0], pos_valid.shape[1], idx.shape[1] - pos_valid.shape[1]
    loss_cls = loss_reg = cls_all.new_zeros(())
    tgt = torch.cat([torch.ones(n_pos_max, device=idx.device), torch.zeros(n_tot, device=idx.device)])
    avg = valid.sum(1).clamp(min=1)                                                           # [B]
    bce = F.binary_cross_entropy_with_logits(cls_all.gather(1, idx), tgt[None].expand(B, -1), reduction="none")
    l_cls = (bce * valid).sum(1) / avg
    reg_p = reg_all.gather(1, idx[:, :n_pos_max, None].expand(-1, -1, 4))
    l_reg = ((reg_p - d_t).abs().sum(2) * pos_valid.float()).sum(1) / avg
    for b in range(B):                                                                        # per image, then over the batch in image order
        loss_cls, loss_reg = loss_cls + l_cls[b], loss_reg + l_reg[b]
    return loss_cls / B, loss_reg / B


def cls_loss_torch(cls, labels):
    return F.cross_entropy(cls.float(), labels)


def box_loss_torch(reg, labels_b, reg_t, pos_valid):
    B, n_tot = labels_b.shape
    n_pos_max, C = pos_valid.shape[1], reg.shape[1] // 4
    labels_c, reg_t, pv = labels_b.reshape(-1), reg_t.reshape(-1, 4), pos_valid.reshape(-1).float()
    pos_sel = torch.cat([torch.arange(n_pos_max, device=reg.device) + b * n_tot for b in range(B)])
    pl = labels_c[pos_sel].clamp(max=C - 1)
    ar = torch.arange(pos_sel.numel(), device=reg.device)
    reg_p = reg.float()[pos_sel].view(-1, C, 4)[ar, pl]
    return ((reg_p - reg_t).abs().sum(1) * pv).sum() / (B * n_tot)


def mask_loss_torch(logits, labels, target, pv):
    logits = logits.float()
    logit_c = logits[torch.arange(labels.numel(), device=labels.device), labels]
    lm = F.binary_cross_entropy_with_logits(logit_c, target, reduction="none").mean((1, 2))
    return (lm * pv).sum() / pv.sum().clamp(min=1)


# ------------------------------------------------------------------------------------------------------------------------
# the models' hooks
# ------------------------------------------------------------------------------------------------------------------------
def rpn_loss_dispatch(cls_all, reg_all, idx, valid, pos_valid, d_t):
    """(loss_rpn_cls, loss_rpn_bbox) of a batch from the flattened RPN outputs and rpn_targets' results.  On the GPU one HIP launch per
    direction (ops.rpn_losses -> pswin_rpn_losses_fwd / _bwd) and the sum over the images; on the CPU rpn_loss_torch."""
    if cls_all.is_cuda:
        from . import ops
        return _rpn_loss(ops.rpn_losses, cls_all, reg_all, idx, valid, pos_valid, d_t)
    return rpn_loss_torch(cls_all, reg_all, idx, valid, pos_valid, d_t)


def cls_loss_dispatch(cls, labels):
    """The mean cross-entropy of cls [N, C + 1] (as the box head returns it: bf16 under autocast) against labels long [N].  On the GPU
    ops.ce_rows (pswin_ce_rows_fwd / _bwd) and rows.sum() / N; on the CPU cls_loss_torch."""
    if cls.is_cuda:
        from . import ops
        return _cls_loss(ops.ce_rows, cls, labels)
    return cls_loss_torch(cls, labels)


def box_loss_dispatch(reg, labels_b, reg_t, pos_valid):
    """The box head's L1 loss: reg [B n_tot, 4 C] (as the head returns it), labels_b long [B, n_tot], reg_t f32 [B, n_pos_max, 4],
    pos_valid bool [B, n_pos_max] -- the positives are the first n_pos_max rows of every image -- divided by B n_tot.  On the GPU
    ops.l1_rows (pswin_l1_rows_fwd / _bwd) over ALL rows with weight 0 behind the positives; on the CPU box_loss_torch."""
    if reg.is_cuda:
        from . import ops
        return _box_loss(ops.l1_rows, reg, labels_b, reg_t, pos_valid)
    return box_loss_torch(reg, labels_b, reg_t, pos_valid)


def mask_loss_dispatch(logits, labels, target, pv):
    """The mask head's loss: logits [M, C, S, S] (as the head returns them: bf16 and channels-last under autocast), labels long [M] in
    [0, C), target f32 [M, S, S], pv f32 [M] (1 for a valid positive) -> sum of the valid rows' mean BCE / max(their number, 1).  On the
    GPU ops.mask_bce_rows (pswin_mask_bce_rows_fwd / _bwd); on the CPU mask_loss_torch."""
    if logits.is_cuda:
        from . import ops
        return _mask_loss(ops.mask_bce_rows, logits, labels, target, pv)
    return mask_loss_torch(logits, labels, target, pv)


def rpn_loss_definition(cls_all, reg_all, idx, valid, pos_valid, d_t):
    return _rpn_loss(rpn_losses, cls_all, reg_all, idx, valid, pos_valid, d_t)


def cls_loss_definition(cls, labels):
    return _cls_loss(ce_rows, cls, labels)


def box_loss_definition(reg, labels_b, reg_t, pos_valid):
    return _box_loss(l1_rows, reg, labels_b, reg_t, pos_valid)


def mask_loss_definition(logits, labels, target, pv):
    return _mask_loss(mask_bce_rows, logits, labels, target, pv)


DEFINITION_HOOKS = dict(rpn_loss=rpn_loss_definition, cls_loss=cls_loss_definition, box_loss=box_loss_definition, mask_loss=mask_loss_definition)
KERNEL_HOOKS = dict(rpn_loss=rpn_loss_dispatch, cls_loss=cls_loss_dispatch, box_loss=box_loss_dispatch, mask_loss=mask_loss_dispatch)
