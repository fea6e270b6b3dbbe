"""A minimal Mask R-CNN training step around the MI355X PanoSwin backbone (BASELINE.json configs[2]).

Scope: the CALLER of the hot path, built only far enough to time an end-to-end detector step with the backbone's share in
it.  mmcv / mmdet / torchvision are not installed, so this is a self-contained pure-PyTorch restatement of ONE pipeline with
the reference's configuration numbers (configs/_base_/models/mask_rcnn_swin_fpn.py:21-115):

  FPN (mmdet/models/necks/fpn.py: laterals 1x1, top-down nearest upsampling, 3x3 output convs, 5th level by stride-2
  subsampling) -> RPNHead (3 anchors: scale 8, ratios 0.5 / 1 / 2, strides 4..64; MaxIoU assigner 0.7 / 0.3 / 0.3, random
  sampler 256 @ 0.5, sigmoid cross-entropy + L1 on deltas) -> proposals (nms_pre 2000 per level, NMS 0.7, 1000 per image)
  -> StandardRoIHead (MaxIoU 0.5, ground truth added as proposals, random sampler 512 @ 0.25; RoIAlign 7 -> Shared2FC 1024
  -> 80 classes, cross-entropy + L1 with stds 0.1 / 0.2; RoIAlign 14 -> 4 convs + deconv -> 28 x 28 masks, BCE on the class
  channel), called as TwoStageDetector.forward_train does (mmdet/models/detectors/two_stage.py:116-175).

PARITY: unpinned.  The reference tree does not contain mmcv.ops (RoIAlign, NMS CUDA sources) nor a fixture for any head,
so nothing here is checked against reference outputs.  RoIAlign is the published operator with the config's sampling_ratio = 0
(adaptive grid) as hand-written HIP kernels, forward and backward (csrc/pswin_roi.hip, checked against a plain PyTorch statement
of the definition in tests/); NMS is the greedy rule: on the CPU a fixed-point iteration (nms_keep), on the GPU pswin_nms_groups.  The
proposal stage (per level top nms_pre, decode, NMS, top max_per_img: proposals_batch, the stacked _proposals) runs on the GPU once per
batch as HIP kernels whose launch count does not depend on the batch size (ops.rpn_proposals -> csrc/pswin_proposals.hip, all images'
levels in one pswin_nms_groups call); beyond the kernels' limits the definition runs on the device image by image.  The other
head operators are ordinary PyTorch-ROCm operators (MIOpen / hipBLASLt, bf16 autocast).

TARGETS: a PaddedTargets (fixed shapes, the box count of every image on the device: the form a captured step is replayed on with the
next batch's annotations), or a list of dicts per image, which heads_loss pads on entry (PaddedTargets.of; shapes tied to that batch).
There is one target path for both: each stage's MaxIoUAssigner for the whole batch (max_iou_assign_batch, pinned to the reference's own
results: tests/golden/max_iou_assign_batch.npz), then everything between "assigned" and "loss" once per batch -- the RandomSampler, the
box targets and the mask targets (sample_ranks, rpn_targets, roi_targets, mask_targets below).  On the CPU these definitions run; on the
GPU the HIP kernels pinned to them (ops.max_iou_assign_batch -> pswin_max_iou_assign; ops.rpn_targets / roi_targets / mask_targets ->
csrc/pswin_targets.hip), and a missing kernel is an error.  The sampler's tie rule is stated once, at sample_ranks.

INFERENCE: `heads_predict` / `simple_test` (TwoStageDetector.simple_test, mmdet/models/detectors/two_stage.py:217) return a Detections:
fixed shapes, the detection count of every image on the device, no host synchronisation -- one captured graph serves every batch.  The
definitions are multiclass_nms and paste_masks below (pure PyTorch; pinned to the reference where its tree allows:
tests/golden/detect_post.npz); on the GPU both run as HIP kernels for the whole batch (ops.multiclass_nms_batch -> pswin_multiclass_nms,
ops.paste_masks -> pswin_paste_masks).
"""
import math

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import losses
from .backbone import SimplePanoSwinTransformer


# ------------------------------------------------------------------------------------------------------------------------
# boxes
# ------------------------------------------------------------------------------------------------------------------------
def box_iou(a, b):
    """[N, 4] x [M, 4] (x1, y1, x2, y2) -> [N, M]"""
    area_a = (a[:, 2] - a[:, 0]).clamp(min=0) * (a[:, 3] - a[:, 1]).clamp(min=0)
    area_b = (b[:, 2] - b[:, 0]).clamp(min=0) * (b[:, 3] - b[:, 1]).clamp(min=0)
    lt = torch.max(a[:, None, :2], b[None, :, :2])
    rb = torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area_a[:, None] + area_b[None] - inter).clamp(min=1e-6)


def box_iof(a, b):
    """intersection over the area of the FIRST box (mmdet bbox_overlaps(mode='iof')): [N, 4] x [M, 4] -> [N, M]"""
    area_a = (a[:, 2] - a[:, 0]).clamp(min=0) * (a[:, 3] - a[:, 1]).clamp(min=0)
    lt = torch.max(a[:, None, :2], b[None, :, :2])
    rb = torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    return wh[..., 0] * wh[..., 1] / area_a[:, None].clamp(min=1e-6)


def max_iou_assign(bboxes, gt_bboxes, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, match_low_quality=True, gt_bboxes_ignore=None,
                   ignore_iof_thr=-1.0, ignore_wrt_candidates=True):
    """MaxIoUAssigner.assign (mmdet/core/bbox/assigners/max_iou_assigner.py:85-212; gt_max_assign_all=True): long [N] with
    -1 = ignore, 0 = negative, i + 1 = positive matched to gt i.  Pinned by the reference's own vectors
    (tests/test_utils/test_assigner.py:14-151 -> tests/golden/detector_reference_vectors.json).  No host synchronisation and static
    shapes for non-empty inputs (the step is captured in a hipGraph): the reference's sequential low-quality loop, in which a later
    gt overwrites an earlier one, is the maximum over the matching gt indices."""
    N, G = bboxes.shape[0], gt_bboxes.shape[0]
    inds = torch.full((N,), -1, dtype=torch.long, device=bboxes.device)
    if N == 0 or G == 0:
        return inds.zero_() if G == 0 else inds                                                   # :147-153
    overlaps = box_iou(gt_bboxes, bboxes)                                                         # [G, N]  (:105)
    if ignore_iof_thr > 0 and gt_bboxes_ignore is not None and gt_bboxes_ignore.numel() > 0:    # :107-117
        if ignore_wrt_candidates:
            ign = box_iof(bboxes, gt_bboxes_ignore).max(1)[0]
        else:
            ign = box_iof(gt_bboxes_ignore, bboxes).max(0)[0]
        overlaps = torch.where((ign > ignore_iof_thr)[None], overlaps.new_full((), -1.0), overlaps)
    best, arg = overlaps.max(0)
    inds = torch.where((best >= 0) & (best < neg_iou_thr), torch.zeros_like(inds), inds)          # :170-172
    inds = torch.where(best >= pos_iou_thr, arg + 1, inds)                                        # :179-180
    if match_low_quality:                                                                         # :182-197
        gbest = overlaps.max(1)[0]
        hit = (overlaps == gbest[:, None]) & (gbest[:, None] >= min_pos_iou)
        last = (hit.long() * torch.arange(1, G + 1, device=bboxes.device)[:, None]).max(0)[0]
        inds = torch.where(last > 0, last, inds)
    return inds


_CONSTS = {}


def _const(values, like, dtype=None):
    """A small constant tensor on `like`'s device (of its dtype unless one is given), built once: a host-to-device copy per call would
    also break hipGraph capture.  Shared by its callers: read it, never write it."""
    key = (tuple(float(v) for v in values), str(like.device), dtype or like.dtype)
    if key not in _CONSTS:
        _CONSTS[key] = torch.tensor(key[0], device=like.device, dtype=key[2])
    return _CONSTS[key]


def encode_deltas(src, dst, stds):
    """DeltaXYWHBBoxCoder.encode (means 0)"""
    sw, sh = (src[:, 2] - src[:, 0]).clamp(min=1e-3), (src[:, 3] - src[:, 1]).clamp(min=1e-3)
    dw, dh = (dst[:, 2] - dst[:, 0]).clamp(min=1e-3), (dst[:, 3] - dst[:, 1]).clamp(min=1e-3)
    sx, sy = (src[:, 0] + src[:, 2]) * 0.5, (src[:, 1] + src[:, 3]) * 0.5
    dx, dy = (dst[:, 0] + dst[:, 2]) * 0.5, (dst[:, 1] + dst[:, 3]) * 0.5
    d = torch.stack([(dx - sx) / sw, (dy - sy) / sh, torch.log(dw / sw), torch.log(dh / sh)], 1)
    return d / _const(stds, d)


def decode_deltas(src, deltas, stds, max_shape):
    d = deltas * _const(stds, deltas)
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    sx, sy = (src[:, 0] + src[:, 2]) * 0.5, (src[:, 1] + src[:, 3]) * 0.5
    clip = abs(math.log(16 / 1000))
    w, h = sw * d[:, 2].clamp(-clip, clip).exp(), sh * d[:, 3].clamp(-clip, clip).exp()
    x, y = sx + sw * d[:, 0], sy + sh * d[:, 1]
    H, W = max_shape
    return torch.stack([(x - w * 0.5).clamp(0, W), (y - h * 0.5).clamp(0, H), (x + w * 0.5).clamp(0, W), (y + h * 0.5).clamp(0, H)], 1)


def _topk_stable(scores, k):
    """The k largest scores and their indices, ties broken by index (stable sort).  torch.topk picks among EQUAL scores in an order
    that depends on the timing of its atomics: with bf16 RPN logits (thousands of exactly equal values at initialisation) two passes
    over bit-identical feature maps then keep different proposals -- same losses to six digits, feature-map gradients 11 % apart
    (seen between replays of one captured step).  mmdet's own top-k has the same property; a stand-in that is replayed from a hipGraph
    and compared with an eager step should not."""
    s, i = torch.sort(scores, descending=True, stable=True)
    return s[:k], i[:k]


def nms_keep(boxes, iou_thr, iters=12):
    """Greedy NMS on score-sorted boxes as a fixed point: keep[j] = not any(i < j: keep[i] and IoU(i, j) > thr).  Starting
    from "keep all", every sweep fixes at least one more level of the suppression chains; `iters` sweeps of one [n, n]
    mask-vector product each, no host synchronisation (the step is captured in a hipGraph: a static sweep count).  Exact
    when no suppression chain is deeper than `iters`; APPROXIMATE beyond that (the default 12 is not checked for convergence
    in the step; tests/test_detector_heads.py compares 32 sweeps with the sequential rule)."""
    over = torch.triu(box_iou(boxes, boxes) > iou_thr, diagonal=1).float()
    keep = torch.ones(boxes.shape[0], device=boxes.device)
    for _ in range(iters):
        keep = (keep @ over == 0).float()
    return keep.bool()


def nms_keep_groups(box_list, iou_thr):
    """nms_keep for several score-sorted box lists.  On the GPU: the exact greedy rule, all lists in one HIP launch (ops.nms_groups ->
    pswin_nms_groups; <= 2048 boxes per list); on the CPU (the definition tests): the fixed-point form above, list by list."""
    if box_list and box_list[0].is_cuda and max(b.shape[0] for b in box_list) <= 2048:
        from . import ops
        return ops.nms_groups(box_list, iou_thr)
    return [nms_keep(b, iou_thr) for b in box_list]


def max_iou_assign_batch(cand, gt, gt_count, pos, neg, min_pos, match_low_quality, lead_gt=0):
    """max_iou_assign for a padded batch: (gt_inds long [B, N], max_iou f32 [B, N]).  cand [N, 4] (shared by the images) or [B, N, 4];
    gt [B, Gmax, 4] of which the first gt_count[b] (int32 [B]) rows of image b are boxes.  With lead_gt > 0 the first lead_gt candidates
    of an image are its own padded gt rows (add_gt_as_proposals): those past the count are padding, come back as gt_inds = -1 /
    max_iou = -1 and take part in no maximum.  An image without boxes: every other candidate 0 / 0 (max_iou_assigner.py:147-153).
    On the GPU: two HIP launches for the whole batch that read the counts from the device (ops.max_iou_assign_batch ->
    pswin_max_iou_assign), so a captured step follows the buffers; on the CPU (the definition): image by image through
    max_iou_assign on the valid rows."""
    if gt.is_cuda:
        from . import ops
        return ops.max_iou_assign_batch(cand, gt, gt_count, pos, neg, min_pos, match_low_quality, lead_gt)
    B, N = gt.shape[0], cand.shape[-2]
    inds = torch.full((B, N), -1, dtype=torch.long)
    best = torch.full((B, N), -1.0)
    for b, G in enumerate(gt_count.tolist()):
        c = cand[b] if cand.dim() == 3 else cand
        valid = torch.ones(N, dtype=torch.bool)
        valid[G:lead_gt] = False
        if G == 0:
            inds[b, valid], best[b, valid] = 0, 0.0
            continue
        inds[b, valid] = max_iou_assign(c[valid], gt[b, :G], pos, neg, min_pos, match_low_quality)
        best[b, valid] = box_iou(gt[b, :G], c[valid]).max(0)[0]
    return inds, best


# ------------------------------------------------------------------------------------------------------------------------
# sampling, box targets and mask targets of a padded batch (the definitions; on the GPU: csrc/pswin_targets.hip through ops)
# ------------------------------------------------------------------------------------------------------------------------
def sample_ranks(gt_inds, key, n_pos, n_neg):
    """RandomSampler with static shapes for a batch: gt_inds long [B, N] (an assigner's result), key f32 [B, N] (finite, >= 0) ->
    (pos_rank long [B, n_pos], neg_rank long [B, n_neg]), n_pos, n_neg <= N.  A candidate that does not belong to a list goes BEHIND
    its members: behind = where(gt_inds < 0, key + 4, key + 2) in float32 (ignored rows, the gt padding among them, behind everything).
    pos_rank is the order of where(gt_inds > 0, key, behind), neg_rank that of where(gt_inds == 0, key, behind), first columns only.

    TIES.  The sort is STABLE: equal composed keys come out in ascending index, the choice _topk_stable makes and for the same reason
    (a captured graph, its replays and the definition must agree on the bit).  The order is that of the float32 COMPOSED key fl(key + 2),
    which keeps 2^-22 of the key's 2^-24 resolution, not that of `key`: so every outcome is one an unstable argsort of the same composed
    keys could have produced."""
    N = gt_inds.shape[1]
    if n_pos > N or n_neg > N:
        raise ValueError(f"sample_ranks: n_pos = {n_pos} and n_neg = {n_neg} must not exceed the {N} candidates")
    key = key.float()
    behind = torch.where(gt_inds < 0, key + 4, key + 2)
    pos_rank = torch.sort(torch.where(gt_inds > 0, key, behind), dim=1, stable=True)[1][:, :n_pos]
    neg_rank = torch.sort(torch.where(gt_inds == 0, key, behind), dim=1, stable=True)[1][:, :n_neg]
    return pos_rank, neg_rank


def _encode_rows(src, dst, stds, ok):
    """encode_deltas on [B, P, 4] rows, rows whose `ok` is false ZERO (a loss multiplies them by 0)"""
    d = encode_deltas(src.reshape(-1, 4), dst.reshape(-1, 4), stds).reshape(src.shape)
    return torch.where(ok[..., None], d, torch.zeros_like(d))


def rpn_targets(gt_inds, key, anchors, gt, n_pos_max, n_tot):
    """The RPN's sampled targets of a padded batch: gt_inds long [B, A], key f32 [B, A], anchors f32 [A, 4] (shared), gt f32 [B, Gmax, 4]
    -> (idx long [B, n_pos_max + n_tot], valid f32 of that shape, pos_valid bool [B, n_pos_max], reg_t f32 [B, n_pos_max, 4]).
    idx = (pos_rank, neg_rank) of sample_ranks(gt_inds, key, n_pos_max, n_tot); a positive slot is valid when it holds a positive, a
    negative slot when it holds a negative AND lies in front of n_tot - (the number of valid positives); reg_t =
    encode_deltas(anchors[pos_rank], gt[(gt_inds - 1).clamp(min=0)[pos_rank]], stds 1), rows of invalid positive slots zero."""
    B = gt_inds.shape[0]
    pos_rank, neg_rank = sample_ranks(gt_inds, key, n_pos_max, n_tot)
    pos_valid = gt_inds.gather(1, pos_rank) > 0
    n_pos = pos_valid.sum(1, keepdim=True)
    neg_valid = (gt_inds.gather(1, neg_rank) == 0) & (torch.arange(n_tot, device=key.device)[None] < (n_tot - n_pos))
    arg = (gt_inds - 1).clamp(min=0).gather(1, pos_rank)
    dst = gt[torch.arange(B, device=gt.device)[:, None], arg]
    reg_t = _encode_rows(anchors[pos_rank], dst, (1.0, 1.0, 1.0, 1.0), pos_valid)
    return torch.cat([pos_rank, neg_rank], 1), torch.cat([pos_valid, neg_valid], 1).float(), pos_valid, reg_t


def roi_targets(gt_inds, key, cand, gt, gt_labels, num_classes, n_pos_max, n_tot, stds):
    """The RoI head's sampled RoIs and targets of a padded batch: gt_inds long [B, N], key f32 [B, N], cand f32 [B, N, 4], gt f32
    [B, Gmax, 4], gt_labels long [B, Gmax] -> (rois f32 [B, n_tot, 4], labels long [B, n_tot], reg_t f32 [B, n_pos_max, 4], pos_valid bool
    [B, n_pos_max], gt_idx long [B, n_pos_max]).  The first n_pos_max RoIs are pos_rank of sample_ranks(gt_inds, key, n_pos_max, n_tot).
    The positive slots that found no positive were filled with the lowest-key non-positives (they count as background): the negatives
    proper are the NEXT ones of the negative order, neg_order[(j + filler).clamp(max=N - 1)] with filler = n_pos_max - (valid positives),
    so that no RoI is sampled twice.  labels: the matched gt's label in a valid positive slot, num_classes (background) elsewhere;
    gt_idx = (gt_inds - 1).clamp(min=0)[pos_rank]; reg_t = encode_deltas(rois, gt[gt_idx], stds), rows of invalid slots zero."""
    B, N = gt_inds.shape
    bi = torch.arange(B, device=gt.device)[:, None]
    pos_rank, neg_order = sample_ranks(gt_inds, key, n_pos_max, n_tot)
    pos_valid = gt_inds.gather(1, pos_rank) > 0
    filler = n_pos_max - pos_valid.sum(1, keepdim=True)
    take = (torch.arange(n_tot - n_pos_max, device=key.device)[None] + filler).clamp(max=N - 1)    # < n_tot: inside neg_order
    idx = torch.cat([pos_rank, neg_order.gather(1, take)], 1)
    rois = cand[bi, idx]
    gt_idx = (gt_inds - 1).clamp(min=0).gather(1, pos_rank)
    labels = torch.full_like(idx, num_classes)
    labels[:, :n_pos_max] = torch.where(pos_valid, gt_labels.gather(1, gt_idx), labels[:, :n_pos_max])
    reg_t = _encode_rows(rois[:, :n_pos_max], gt[bi, gt_idx], stds, pos_valid)
    return rois, labels, reg_t, pos_valid, gt_idx


def mask_targets(masks, rois, gt_idx, pos_valid, size=28, dtype=torch.float32, return_float=False):
    """The mask head's targets of a padded batch: masks uint8 [B, Gmax, H, W], rois f32 [B, P, 4] in image pixels, gt_idx long [B, P],
    pos_valid bool [B, P] -> f32 [B * P, size, size] of 0 / 1 (return_float: the sampled float image instead).  Sample point (i, j) of a
    RoI lies at t = (j + 0.5) / size along its sides, in normalised coordinates gx = (x0 + (x1 - x0) * t) / W * 2 - 1; the ONE assigned
    bitmap masks[b, gt_idx[b, p]] is sampled there bilinearly with grid_sample's align_corners=False geometry and zero padding, then
    `>= 0.5`.  Rows whose pos_valid is false are zeros (the loss masks them).  dtype: the arithmetic (float64: the truth the GPU test
    measures the near-threshold set against).

    PARITY: unpinned.  The reference's BitmapMasks.crop_and_resize calls mmcv.ops.roi_align, which the reference tree does not contain,
    so nothing pins these targets to the reference's."""
    B, G, H, W = masks.shape
    P = rois.shape[1]
    t = (torch.arange(size, device=rois.device, dtype=dtype) + 0.5) / size
    out = []
    for b in range(B):
        r = rois[b].to(dtype)
        gx = (r[:, 0:1] + (r[:, 2:3] - r[:, 0:1]) * t[None]) / W * 2 - 1
        gy = (r[:, 1:2] + (r[:, 3:4] - r[:, 1:2]) * t[None]) / H * 2 - 1
        grid = torch.stack([gx[:, None, :].expand(-1, size, size), gy[:, :, None].expand(-1, size, size)], -1)   # [P, size, size, 2]
        plane = masks[b][gt_idx[b].clamp(0, G - 1)].to(dtype)[:, None]                                         # [P, 1, H, W]
        smp = F.grid_sample(plane, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0]
        out.append(torch.where(pos_valid[b][:, None, None], smp, torch.zeros_like(smp)))
    img = torch.cat(out)
    return img if return_float else (img >= 0.5).float()


def rpn_targets_dispatch(gt_inds, key, anchors, gt, n_pos_max, n_tot):
    """rpn_targets.  On the GPU: HIP kernels for the whole batch (ops.rpn_targets -> pswin_sample_ranks, pswin_rpn_targets); on the CPU
    the definition."""
    if gt_inds.is_cuda:
        from . import ops
        return ops.rpn_targets(gt_inds, key, anchors, gt, n_pos_max, n_tot)
    return rpn_targets(gt_inds, key, anchors, gt, n_pos_max, n_tot)


def proposals_batch(cls_all, reg_all, anchors, cfg, img_hw):
    """The RPN's proposals of a batch (the definition of ops.rpn_proposals): MiniMaskRCNN._proposals image by image, stacked.  cls_all f32
    [B, A] raw logits and reg_all f32 [B, A, 4] as _rpn_flatten returns them, anchors: the per-level list of make_anchors, cfg: nms_pre,
    nms, max_per_img -> (rois f32 [B, P, 4], scores f32 [B, P], count int32 [B]) with P = min(max_per_img, sum over the levels of
    min(nms_pre, n_l)).  ALL P rows are defined, not only the survivors (the training path hands the suppressed tail to the RoI assigner
    as candidates too): count[b] is the number of rows whose score is > -1e4, the survivors of the NMS, and they lead; the suppressed
    candidates follow in the order of the concatenated levels."""
    with torch.no_grad():
        props = [MiniMaskRCNN._proposals(cls_all[b], reg_all[b], anchors, cfg, img_hw) for b in range(cls_all.shape[0])]
    scores = torch.stack([p[1] for p in props])
    return torch.stack([p[0] for p in props]), scores, (scores > -1e4).sum(1).to(torch.int32)


def proposals_batch_dispatch(cls_all, reg_all, anchors, cfg, img_hw):
    """proposals_batch.  On the GPU inside the kernels' limits (ops.rpn_proposals_supported): HIP kernels for the whole batch, a number
    of launches that does not depend on B (ops.rpn_proposals -> pswin_rpn_proposals); outside the limits the definition on the device,
    image by image, as nms_keep_groups falls back for lists above 2048; on the CPU the definition."""
    if cls_all.is_cuda:
        from . import ops
        if ops.rpn_proposals_supported([a.shape[0] for a in anchors], cls_all.shape[0], cfg["nms_pre"], cfg["max_per_img"]):
            return ops.rpn_proposals(cls_all, reg_all, anchors, cfg["nms_pre"], cfg["nms"], cfg["max_per_img"], img_hw)
    return proposals_batch(cls_all, reg_all, anchors, cfg, img_hw)


def roi_targets_dispatch(gt_inds, key, cand, gt, gt_labels, num_classes, n_pos_max, n_tot, stds):
    """roi_targets.  On the GPU: HIP kernels for the whole batch (ops.roi_targets -> pswin_sample_ranks, pswin_roi_targets); on the CPU
    the definition."""
    if gt_inds.is_cuda:
        from . import ops
        return ops.roi_targets(gt_inds, key, cand, gt, gt_labels, num_classes, n_pos_max, n_tot, stds)
    return roi_targets(gt_inds, key, cand, gt, gt_labels, num_classes, n_pos_max, n_tot, stds)


def mask_targets_dispatch(masks, rois, gt_idx, pos_valid, size=28):
    """mask_targets.  On the GPU one HIP launch (ops.mask_targets -> pswin_mask_targets); on the CPU the definition."""
    if masks.is_cuda:
        from . import ops
        return ops.mask_targets(masks, rois, gt_idx, pos_valid, size)
    return mask_targets(masks, rois, gt_idx, pos_valid, size)


class PaddedTargets:
    """The annotations of a batch in buffers of a fixed shape, for a captured detector step: boxes f32 [B, Gmax, 4], labels int64
    [B, Gmax], count int32 [B] (the first count[b] rows of image b are boxes, the rest zeros) and masks uint8 [B, Gmax, H, W] or None
    (Faster R-CNN).  The captured step reads the buffers; `copy_from` puts the next batch into them, outside the capture and on the
    stream the step is replayed on.  rle: the masks' COCO run-length encoding (rle.RleMasks of B Gmax masks, e.g.
    RleMasks.from_lists(annotations, device, K=Gmax)) or None; only the mask metric of evaluation.py reads it, and allocate / of /
    copy_from leave it alone."""

    def __init__(self, boxes, labels, count, masks=None, rle=None):
        self.boxes, self.labels, self.count, self.masks, self.rle = boxes, labels, count, masks, rle
        self.list_counts = None                      # of(lists): the host's copy of the counts, by which the RoI stage lays out its keys

    @classmethod
    def of(cls, targets):
        """`targets` itself if it is a PaddedTargets; a list of dicts per image (boxes [G, 4], labels [G], masks [G, H, W] or none), padded
        with zeros to Gmax = max(1, the largest count).  Device operations of host-known shapes only, and `count` is a cached constant
        (_const: read it, never copy_from into it), so that a captured step may take lists: its warm-up passes fill the cache."""
        if isinstance(targets, cls):
            return targets
        counts = tuple(int(t["boxes"].shape[0]) for t in targets)
        B, Gmax, ref = len(counts), max(1, *counts), targets[0]["boxes"]
        out = cls(ref.new_zeros(B, Gmax, 4, dtype=torch.float32), ref.new_zeros(B, Gmax, dtype=torch.long), _const(counts, ref, torch.int32))
        if "masks" in targets[0]:
            out.masks = ref.new_zeros(B, Gmax, *targets[0]["masks"].shape[1:], dtype=torch.uint8)
        for b, (t, n) in enumerate(zip(targets, counts)):
            out.boxes[b, :n], out.labels[b, :n] = t["boxes"], t["labels"]
            if out.masks is not None:
                out.masks[b, :n] = t["masks"].to(torch.uint8)
        out.list_counts = counts
        return out

    @classmethod
    def allocate(cls, B, max_gt, device, mask_hw=None):
        masks = None if mask_hw is None else torch.zeros(B, max_gt, int(mask_hw[0]), int(mask_hw[1]), dtype=torch.uint8, device=device)
        return cls(torch.zeros(B, max_gt, 4, device=device), torch.zeros(B, max_gt, dtype=torch.long, device=device),
                   torch.zeros(B, dtype=torch.int32, device=device), masks)

    @property
    def max_gt(self):
        return self.boxes.shape[1]

    def copy_from(self, boxes, labels, masks=None):
        """boxes / labels (/ masks): one [G, 4] / [G] (/ [G, H, W]) numpy array or tensor per image (what PanoTrainTransform returns).
        Pads with zeros and copies into the existing buffers in place."""
        from ._lib import PswinError
        B, Gmax = self.boxes.shape[:2]
        if len(boxes) != B or len(labels) != B or (masks is not None and len(masks) != B):
            raise PswinError(f"PaddedTargets.copy_from: the buffers hold {B} images, got {len(boxes)} box and {len(labels)} label arrays")
        if (masks is None) != (self.masks is None):
            raise PswinError("PaddedTargets.copy_from: masks must be given exactly when the buffers were allocated with mask_hw")
        bx, lb = [torch.as_tensor(v).detach().to("cpu", torch.float32).reshape(-1, 4) for v in boxes], \
                 [torch.as_tensor(v).detach().to("cpu", torch.long).reshape(-1) for v in labels]
        counts = [v.shape[0] for v in bx]
        if max(counts) > Gmax:
            raise PswinError(f"PaddedTargets.copy_from: an image has {max(counts)} boxes, the buffers hold max_gt = {Gmax}")
        if any(l.shape[0] != n for l, n in zip(lb, counts)) or (masks is not None and any(len(m) != n for m, n in zip(masks, counts))):
            raise PswinError("PaddedTargets.copy_from: one label (and one mask) per box")
        hb, hl = torch.zeros(B, Gmax, 4), torch.zeros(B, Gmax, dtype=torch.long)
        for b, n in enumerate(counts):
            hb[b, :n], hl[b, :n] = bx[b], lb[b]
        self.boxes.copy_(hb)
        self.labels.copy_(hl)
        self.count.copy_(torch.tensor(counts, dtype=torch.int32))
        if masks is not None:
            self.masks.zero_()
            for b, n in enumerate(counts):
                if n:
                    self.masks[b, :n].copy_(torch.as_tensor(masks[b]).to(torch.uint8))
        return self

    def as_lists(self):
        """The list-of-dicts form of the same annotations (reads the counts back: not for a captured step)."""
        out = []
        for b, n in enumerate(self.count.tolist()):
            d = {"boxes": self.boxes[b, :n], "labels": self.labels[b, :n]}
            if self.masks is not None:
                d["masks"] = self.masks[b, :n]
            out.append(d)
        return out


# ------------------------------------------------------------------------------------------------------------------------
# inference: class-wise NMS, mask paste, the fixed-shape result
# ------------------------------------------------------------------------------------------------------------------------
def decode_deltas_per_class(rois, deltas, stds, max_shape):
    """decode_deltas for [R, 4 C] deltas, one box per class of every RoI (delta2bbox on the bbox head's output,
    mmdet/core/bbox/coder/delta_xywh_bbox_coder.py:134-237): [R, 4 C]"""
    R, C = deltas.shape[0], deltas.shape[1] // 4
    src = rois[:, None, :].expand(R, C, 4).reshape(-1, 4)
    return decode_deltas(src, deltas.reshape(-1, 4), stds, max_shape).reshape(R, 4 * C)


def multiclass_nms(multi_bboxes, multi_scores, score_thr, iou_thr, max_num):
    """Class-wise NMS of one image (multiclass_nms, mmdet/core/post_processing/bbox_nms.py:7-93, with mmcv's batched_nms: a box suppresses
    only boxes of its own class).  multi_bboxes [R, 4 C], multi_scores [R, C + 1] with the background column last (ignored) ->
    (dets [k, 5] = box and score, labels long [k], flat_index long [k] = r * C + c of each detection).

    The candidates are the (r, c) with score > score_thr (strict).  Within a class the greedy rule runs in descending score: a candidate
    is dropped when a kept candidate before it has box_iou > iou_thr with it.  The survivors of all classes are ordered by descending
    score and cut to max_num (max_num <= 0: no cut).

    TIES.  The reference leaves candidates of equal score to an unstable sort.  Here equal scores are ordered by ASCENDING flat index
    r * C + c, inside the NMS (where, within a class, that is ascending r) and in the final order: the choice _topk_stable makes, for the
    same reason -- a captured graph and its definition must agree on the bit."""
    R, C = multi_scores.shape[0], multi_scores.shape[1] - 1
    boxes, scores = multi_bboxes.reshape(R * C, 4), multi_scores[:, :C].reshape(-1)
    cand = torch.nonzero(scores > score_thr)[:, 0]                     # ascending flat index
    cand = cand[torch.sort(scores[cand], descending=True, stable=True)[1]]
    labels = cand % C
    keep = torch.ones(cand.numel(), dtype=torch.bool, device=cand.device)
    for c in torch.unique(labels).tolist():
        pos = torch.nonzero(labels == c)[:, 0]                         # this class, in the order the rule visits it
        b = boxes[cand[pos]]
        over = box_iou(b, b) > iou_thr
        kc = torch.ones(pos.numel(), dtype=torch.bool, device=cand.device)
        for i in range(pos.numel() - 1):
            kc[i + 1:] &= ~(over[i, i + 1:] & kc[i])
        keep[pos] = kc
    sel = cand[keep]
    if max_num > 0:
        sel = sel[:max_num]
    return torch.cat([boxes[sel], scores[sel, None]], 1), sel % C, sel


def paste_masks(mask_prob, boxes, img_h, img_w, thr, return_float=False):
    """_do_paste_mask(skip_empty=False) followed by `>= thr` (mmdet/models/roi_heads/mask_heads/fcn_mask_head.py:274-299, 306-377):
    mask_prob [N, 28, 28] probabilities, boxes [N, 4] in the output image's pixels -> bool [N, img_h, img_w] (return_float: the sampled
    float image instead).  Pixel centre (x + 0.5, y + 0.5) is mapped to the box's normalised coordinates, (p - lo) / (hi - lo) * 2 - 1,
    and the mask sampled there bilinearly with grid_sample's align_corners=False geometry and zero padding.  Degenerate boxes as the
    reference: an INFINITE normalised coordinate (a side of zero length) becomes 0, the mask's centre line.  A NaN coordinate (0 / 0: a
    pixel centre exactly on such a side), which the reference hands to grid_sample, samples nothing here: the value is 0."""
    N = mask_prob.shape[0]
    dt = mask_prob.dtype if mask_prob.dtype == torch.float64 else torch.float32
    boxes = boxes.to(dt)
    x0, y0, x1, y1 = torch.split(boxes, 1, dim=1)
    gy = (torch.arange(img_h, device=boxes.device, dtype=dt) + 0.5 - y0) / (y1 - y0) * 2 - 1     # [N, h]
    gx = (torch.arange(img_w, device=boxes.device, dtype=dt) + 0.5 - x0) / (x1 - x0) * 2 - 1     # [N, w]
    gy, gx = torch.where(torch.isinf(gy), torch.zeros_like(gy), gy), torch.where(torch.isinf(gx), torch.zeros_like(gx), gx)
    dead = torch.isnan(gy)[:, :, None] | torch.isnan(gx)[:, None, :]
    gy, gx = torch.nan_to_num(gy, nan=-3.0), torch.nan_to_num(gx, nan=-3.0)                        # outside the mask
    grid = torch.stack([gx[:, None, :].expand(N, img_h, img_w), gy[:, :, None].expand(N, img_h, img_w)], 3)
    img = F.grid_sample(mask_prob[:, None].to(dt), grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0]
    img = torch.where(dead, torch.zeros_like(img), img)
    return img if return_float else img >= thr


def detect_post(rois, roi_count, cls, deltas, stds, img_hw, scale_factor, score_thr, iou_thr, K, dtype=torch.float32):
    """The box half of the test-time post-processing of a batch, image by image through multiclass_nms (the definition of
    ops.multiclass_nms_batch): rois [B, R, 4] of which the first roi_count[b] are proposals, cls [B, R, C + 1] logits, deltas [B, R, 4 C]
    -> (boxes [B, K, 4], scores [B, K], labels long [B, K], count int32 [B], source int32 [B, K]), rows past count[b] zeros.  Softmax,
    decode_deltas with stds clipped to img_hw, division by scale_factor [B, 4] unless None, multiclass_nms(score_thr, iou_thr, K).
    dtype: the arithmetic (float64: the truth the GPU tests measure errors against)."""
    B, R, C = cls.shape[0], cls.shape[1], cls.shape[2] - 1
    dev = cls.device
    boxes, scores = torch.zeros(B, K, 4, dtype=dtype, device=dev), torch.zeros(B, K, dtype=dtype, device=dev)
    labels, source = torch.zeros(B, K, dtype=torch.long, device=dev), torch.zeros(B, K, dtype=torch.int32, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    for b, n in enumerate(roi_count.tolist()):
        n = max(0, min(int(n), R))
        if n == 0:
            continue
        sc = F.softmax(cls[b, :n].to(dtype), dim=-1)
        bx = decode_deltas_per_class(rois[b, :n].to(dtype), deltas[b, :n].to(dtype), stds, img_hw)
        if scale_factor is not None:
            bx = bx / scale_factor[b].to(dtype).repeat(C)
        dets, lab, flat = multiclass_nms(bx, sc, score_thr, iou_thr, K)
        k = dets.shape[0]
        boxes[b, :k], scores[b, :k], labels[b, :k], source[b, :k], count[b] = dets[:, :4], dets[:, 4], lab, flat.to(torch.int32), k
    return boxes, scores, labels, count, source


def paste_masks_batch(mask_logits, labels, boxes, count, thr, out_hw):
    """The mask half (the definition of ops.paste_masks): mask_logits [B K, C, 28, 28], labels long [B, K], boxes [B, K, 4], count [B] ->
    uint8 [B, K, H, W]: paste_masks of sigmoid(the label's channel) for the first count[b] rows of image b, zeros behind them."""
    B, K = labels.shape
    H, W = int(out_hw[0]), int(out_hw[1])
    out = torch.zeros(B, K, H, W, dtype=torch.uint8, device=mask_logits.device)
    lg = mask_logits.reshape(B, K, *mask_logits.shape[1:])
    for b, n in enumerate(count.tolist()):
        if n:
            prob = lg[b, torch.arange(n, device=lg.device), labels[b, :n]].float().sigmoid()
            out[b, :n] = paste_masks(prob, boxes[b, :n].float(), H, W, thr).to(torch.uint8)
    return out


class Detections:
    """The detections of a batch in tensors of a fixed shape, the inference counterpart of PaddedTargets: boxes f32 [B, K, 4], scores f32
    [B, K], labels int64 [B, K], count int32 [B] ON THE DEVICE (the first count[b] rows of image b are detections, in descending score;
    the rest are zeros, masks included), source int32 [B, K] (the flat index r * C + c of each detection: proposal r, class c) and masks
    uint8 [B, K, H, W] or None (Faster R-CNN).  rle: the masks' COCO run-length encoding (rle.RleMasks) or None --
    heads_predict(mask_format="rle") fills it and leaves masks None."""

    def __init__(self, boxes, scores, labels, count, source, masks=None, rle=None):
        self.boxes, self.scores, self.labels, self.count, self.source, self.masks, self.rle = boxes, scores, labels, count, source, masks, rle

    def as_lists(self):
        """Per image (dets [k, 5], labels [k], masks bool [k, H, W] or None) -- reads the counts back: not for a captured step."""
        out = []
        for b, n in enumerate(self.count.tolist()):
            dets = torch.cat([self.boxes[b, :n], self.scores[b, :n, None]], 1)
            out.append((dets, self.labels[b, :n], None if self.masks is None else self.masks[b, :n].bool()))
        return out

    def as_results(self, num_classes):
        """Per image what the reference's simple_test followed by encode_mask_results hands to the results file (mmdet/apis/test.py:60,
        mmdet/core/mask/utils.py:36-63): (bbox_results, segm_results) -- bbox_results a list of num_classes float32 arrays [k_c, 5]
        (bbox2result, mmdet/core/bbox/transforms.py:99), segm_results a list of num_classes lists of {"size": [H, W], "counts": bytes}
        (cls_segms[labels[i]].append(...) of fcn_mask_head.py:302: a row's place in its class list follows row order, as in the arrays).
        The runs come from `rle` when it is set, otherwise from rle.encode_masks(masks, count); without masks only bbox_results.
        Reads back: not for a captured step."""
        from . import rle as rle_mod
        K = self.boxes.shape[1]
        enc = self.rle
        if enc is None and self.masks is not None:
            enc = rle_mod.encode_masks(self.masks.contiguous(), self.count)
        per_image = None if enc is None else enc.to_lists()
        rows = torch.cat([self.boxes.float(), self.scores.float()[:, :, None]], 2).cpu().numpy()
        labels = self.labels.cpu().numpy()
        out = []
        for b, n in enumerate(self.count.tolist()):
            n = max(0, min(int(n), K))
            lab = labels[b, :n]
            bbox = [rows[b, :n][lab == c] for c in range(num_classes)]
            if per_image is None:
                out.append(bbox)
                continue
            segm = [[] for _ in range(num_classes)]
            for k in range(n):
                segm[int(lab[k])].append(per_image[b][k])
            out.append((bbox, segm))
        return out


class Proposals:
    """The RPN's proposals of a batch in tensors of a fixed shape: boxes f32 [B, R, 4], scores f32 [B, R], count int32 [B] ON THE DEVICE.
    The first count[b] rows of image b are the survivors of the RPN's NMS, in descending score; what follows them is not a proposal."""

    def __init__(self, boxes, scores, count):
        self.boxes, self.scores, self.count = boxes, scores, count

    def as_lists(self):
        """Per image an ndarray (count, 5) of x1, y1, x2, y2, score, what the reference's RPN.simple_test returns -- reads back: not for
        a captured step."""
        rows = torch.cat([self.boxes.float(), self.scores.float()[:, :, None]], 2).cpu().numpy()
        return [rows[b, :max(0, min(n, rows.shape[1]))] for b, n in enumerate(self.count.tolist())]


def multiclass_nms_batch(rois, roi_count, cls, deltas, stds, img_hw, scale_factor, score_thr, iou_thr, K):
    """detect_post for a batch.  On the GPU: HIP kernels for the whole batch that read the proposal counts from the device
    (ops.multiclass_nms_batch -> pswin_multiclass_nms), so a captured call follows the buffers; on the CPU: the definition."""
    if cls.is_cuda:
        from . import ops
        return ops.multiclass_nms_batch(rois, roi_count, cls, deltas, stds, img_hw, scale_factor, score_thr, iou_thr, K)
    return detect_post(rois, roi_count, cls, deltas, stds, img_hw, scale_factor, score_thr, iou_thr, K)


def paste_masks_dispatch(mask_logits, labels, boxes, count, thr, out_hw):
    """paste_masks_batch.  On the GPU one HIP launch (ops.paste_masks -> pswin_paste_masks); on the CPU the definition."""
    if mask_logits.is_cuda:
        from . import ops
        return ops.paste_masks(mask_logits, labels, boxes, count, thr, out_hw)
    return paste_masks_batch(mask_logits, labels, boxes, count, thr, out_hw)


def paste_masks_rle_dispatch(mask_logits, labels, boxes, count, thr, out_hw, capacity=None):
    """rle.paste_masks_rle: the RLE of paste_masks_batch.  On the GPU the fused HIP route (ops.paste_masks_rle -> pswin_paste_masks_rle), which
    never forms the bitmap; on the CPU the definition."""
    from . import rle
    return rle.paste_masks_rle(mask_logits, labels, boxes, count, thr, out_hw, capacity)


# ------------------------------------------------------------------------------------------------------------------------
# neck and heads
# ------------------------------------------------------------------------------------------------------------------------
class _AddConvBias(torch.autograd.Function):
    """y = x + bias[None, :, None, None] whose bias gradient is a fixed-order column sum through the C ABI (ops.colsum on the
    channels-last rows).  A convolution's own bias gradient is one of the framework's two-pass global reductions
    (MIOpen ConvolutionBackwardBias / at::sum): 29 launches of ~21 us per step here, and the kind of reduction that returns stale
    results when a captured hipGraph is replayed (pitfalls) -- the head stand-ins of the step ARE replayed."""

    @staticmethod
    def forward(ctx, x, bias):
        ctx.bias_dtype = bias.dtype
        return x + bias.to(x.dtype).view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, dy):
        if dy.is_cuda:
            from . import ops
            db = ops.colsum_channels(dy)                # every channel count through the C ABI (narrow rows are zero-padded)
        else:
            db = dy.float().sum((0, 2, 3))              # CPU: the definition tests only
        return dy, db.to(ctx.bias_dtype)


def conv_bias(m, x):
    """m(x) for an nn.Conv2d / nn.ConvTranspose2d with the bias added (and its gradient summed) by _AddConvBias"""
    if isinstance(m, nn.ConvTranspose2d):
        y = F.conv_transpose2d(x, m.weight, None, m.stride, m.padding, m.output_padding, m.groups, m.dilation)
    else:
        y = F.conv2d(x, m.weight, None, m.stride, m.padding, m.dilation, m.groups)
    return y if m.bias is None else _AddConvBias.apply(y, m.bias)


class FPN(nn.Module):
    def __init__(self, in_channels=(96, 192, 384, 768), out_channels=256, num_outs=5):
        super().__init__()
        self.lateral = nn.ModuleList(nn.Conv2d(c, out_channels, 1) for c in in_channels)
        self.output = nn.ModuleList(nn.Conv2d(out_channels, out_channels, 3, padding=1) for _ in in_channels)
        self.num_outs = num_outs

    def forward(self, feats):
        lat = [conv_bias(l, f) for l, f in zip(self.lateral, feats)]
        for i in range(len(lat) - 1, 0, -1):
            lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode="nearest")
        outs = [conv_bias(o, x) for o, x in zip(self.output, lat)]
        while len(outs) < self.num_outs:
            outs.append(F.max_pool2d(outs[-1], 1, stride=2))
        return outs


class RPNHead(nn.Module):
    def __init__(self, channels=256, num_anchors=3):
        super().__init__()
        self.conv = nn.Conv2d(channels, channels, 3, padding=1)
        self.cls = nn.Conv2d(channels, num_anchors, 1)
        self.reg = nn.Conv2d(channels, num_anchors * 4, 1)

    def forward(self, feats):
        outs = []
        for f in feats:
            t = F.relu(conv_bias(self.conv, f))
            outs.append((conv_bias(self.cls, t), conv_bias(self.reg, t)))
        return outs


_ANCHORS = {}


def make_anchors(shapes, strides, device, scale=8.0, ratios=(0.5, 1.0, 2.0)):
    """AnchorGenerator(scales=[8], ratios=[0.5, 1, 2]).grid_anchors (mmdet/core/anchor/anchor_generator.py; center_offset 0,
    scale_major): per level [H * W * 3, 4], location-major with x fastest (the conv output order).  A stride may be an (x, y) pair; the
    base size is then min(stride), as in the reference.  Layout pinned by tests/test_utils/test_anchor.py:22-40 of the reference
    (tests/golden/detector_reference_vectors.json).  Cached per geometry: constants of the step (and building them copies host data,
    which a hipGraph capture refuses)."""
    strides = [tuple(s) if isinstance(s, (tuple, list)) else (s, s) for s in strides]
    key = (tuple(tuple(int(v) for v in sh) for sh in shapes), tuple(strides), str(device), scale, tuple(ratios))
    if key in _ANCHORS:
        return _ANCHORS[key]
    out = []
    for (H, W), (stx, sty) in zip(shapes, strides):
        s = min(stx, sty)
        r = torch.tensor(ratios, device=device)
        hr, wr = torch.sqrt(r), 1.0 / torch.sqrt(r)
        ws, hs = s * scale * wr, s * scale * hr
        base = torch.stack([-0.5 * ws, -0.5 * hs, 0.5 * ws, 0.5 * hs], 1)                         # centred on the cell corner
        sy, sx = torch.meshgrid(torch.arange(H, device=device) * sty, torch.arange(W, device=device) * stx, indexing="ij")
        shift = torch.stack([sx, sy, sx, sy], -1).reshape(-1, 1, 4).float()
        out.append((shift + base[None]).reshape(-1, 4))
    _ANCHORS[key] = out
    return out


class BBoxHead(nn.Module):
    def __init__(self, channels=256, roi=7, fc=1024, num_classes=80):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(channels * roi * roi, fc), nn.Linear(fc, fc)
        self.cls, self.reg = nn.Linear(fc, num_classes + 1), nn.Linear(fc, num_classes * 4)

    def forward(self, x):
        x = F.relu(self.fc2(F.relu(self.fc1(x.flatten(1)))))
        return self.cls(x), self.reg(x)


class MaskHead(nn.Module):
    def __init__(self, channels=256, num_convs=4, num_classes=80):
        super().__init__()
        self.convs = nn.ModuleList(nn.Conv2d(channels, channels, 3, padding=1) for _ in range(num_convs))
        self.up = nn.ConvTranspose2d(channels, channels, 2, stride=2)
        self.logits = nn.Conv2d(channels, num_classes, 1)

    def forward(self, x):
        for c in self.convs:
            x = F.relu(conv_bias(c, x))
        return conv_bias(self.logits, F.relu(conv_bias(self.up, x)))


def roi_align(feats, strides, rois, out_size, finest_scale=56, sampling_ratio=0):
    """SingleRoIExtractor + RoIAlign(output_size, sampling_ratio = 0: adaptive ceil(roi / output) samples per bin) over 4 FPN levels
    (configs/_base_/models/mask_rcnn_swin_fpn.py:44-48, 63-67).  rois [B, n, 4] in image pixels (the same number per image) ->
    [B * n, C, out, out].  One HIP kernel per direction (ops.roi_align_fpn -> pswin_roi_align_fwd / _bwd): every RoI is sampled on
    the level its scale maps to (finest_scale = 56, as mmdet) and only there."""
    from . import ops
    B, n, _ = rois.shape
    bidx = torch.arange(B, device=rois.device, dtype=rois.dtype)[:, None, None].expand(B, n, 1)
    rois5 = torch.cat([bidx, rois], -1).reshape(B * n, 5)
    return ops.roi_align_fpn(list(feats), strides, rois5, out_size, sampling_ratio, True, finest_scale)


# ------------------------------------------------------------------------------------------------------------------------
# the detector
# ------------------------------------------------------------------------------------------------------------------------
class MiniMaskRCNN(nn.Module):
    """backbone -> FPN -> RPN -> RoI heads with the train_cfg numbers of configs/_base_/models/mask_rcnn_swin_fpn.py.
    `heads_loss(feats, targets)` is everything behind the backbone; `forward_train` = backbone + heads_loss.  At test time
    `heads_predict(feats, img_hw)` is everything behind the backbone with the test_cfg numbers (mask_rcnn_swin_fpn.py:117-127) and
    `simple_test` = backbone + heads_predict: a Detections."""

    STRIDES = (4, 8, 16, 32, 64)
    rand_like = staticmethod(torch.rand_like)    # the samplers' random keys (tests substitute a fixed sequence to compare eager and replayed steps)
    roi_align = staticmethod(roi_align)          # the HIP operator; tests of the head stand-ins on the CPU substitute the PyTorch statement
    assign = staticmethod(max_iou_assign_batch)  # the target assigner of a batch (both stages, once per batch each)
    rpn_targets = staticmethod(rpn_targets_dispatch)      # the RPN's sampler and box targets, once per batch
    roi_targets = staticmethod(roi_targets_dispatch)      # the RoI head's sampler, RoIs, labels and box targets, once per batch
    mask_targets = staticmethod(mask_targets_dispatch)    # the mask head's targets, once per batch
    proposals = staticmethod(proposals_batch_dispatch)    # the RPN's proposals (top nms_pre, decode, NMS, top max_per_img), once per batch
    multiclass_nms = staticmethod(multiclass_nms_batch)   # test time: softmax, decode, class-wise NMS, top K of a batch
    paste = staticmethod(paste_masks_dispatch)            # test time: the detections' masks pasted into the image
    paste_rle = staticmethod(paste_masks_rle_dispatch)    # test time: the run-length encoding of those masks without the bitmaps
    rpn_loss = staticmethod(losses.rpn_loss_dispatch)     # the RPN's two losses from the flattened outputs and rpn_targets' results
    cls_loss = staticmethod(losses.cls_loss_dispatch)     # the box head's cross-entropy on its logits as they are
    box_loss = staticmethod(losses.box_loss_dispatch)     # the box head's L1 on the deltas of every row's class
    mask_loss = staticmethod(losses.mask_loss_dispatch)   # the mask head's BCE on the label's channel of its logits as they are
    BBOX_STDS = (0.1, 0.1, 0.2, 0.2)

    def __init__(self, backbone_cfg, num_classes=80):
        super().__init__()
        self.backbone = SimplePanoSwinTransformer(**backbone_cfg)
        c = self.backbone.num_features
        self.neck = FPN(c, 256, 5)
        self.rpn = RPNHead(256, 3)
        self.bbox_head = BBoxHead(256, 7, 1024, num_classes)
        self.mask_head = MaskHead(256, 4, num_classes)
        self.num_classes = num_classes
        self.rpn_cfg = dict(pos=0.7, neg=0.3, min_pos=0.3, num=256, pos_fraction=0.5, nms_pre=2000, max_per_img=1000, nms=0.7)
        self.rcnn_cfg = dict(pos=0.5, num=512, pos_fraction=0.25, mask_size=28)
        self.test_cfg = dict(rpn=dict(nms_pre=1000, max_per_img=1000, nms=0.7),
                             rcnn=dict(score_thr=0.05, nms=0.5, max_per_img=100, mask_thr_binary=0.5))
        for part in (self.neck, self.rpn, self.mask_head):
            for m in part.modules():
                if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                    nn.init.normal_(m.weight, std=0.01)
                    nn.init.zeros_(m.bias)
        # The convolutional heads in channels-last memory format (PSWIN_HEADS_CHANNELS_LAST=0: NCHW) (MIOpen's bf16 kernels are NHWC: in NCHW
        # every convolution is wrapped in layout transposes, 150 launches / 0.9 ms per step); needs its own find-db records
        # (tools/miopen_find_heads.sh)
        self.channels_last = os.environ.get("PSWIN_HEADS_CHANNELS_LAST", "1") != "0"
        if self.channels_last:
            for part in (self.neck, self.rpn, self.mask_head):
                part.to(memory_format=torch.channels_last)

    def head_parameters(self):
        bb = {id(p) for p in self.backbone.parameters()}
        return [p for p in self.parameters() if id(p) not in bb]

    # -- RPN ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _rpn_flatten(rpn_outs):
        """the RPN's outputs of all levels as f32 [B, A] scores and [B, A, 4] deltas, in the anchors' order"""
        B = rpn_outs[0][0].shape[0]
        cls_all = torch.cat([c.permute(0, 2, 3, 1).reshape(B, -1) for c, _ in rpn_outs], 1).float()          # [B, A]
        reg_all = torch.cat([r.permute(0, 2, 3, 1).reshape(B, -1, 4) for _, r in rpn_outs], 1).float()       # [B, A, 4]
        return cls_all, reg_all

    @staticmethod
    def _proposals(cls_b, reg_b, anchors, cfg, img_hw):
        """The proposals of one image (no gradient; both the training and the test path, each with its own cfg): per level top nms_pre,
        decode, NMS, then the best max_per_img over the levels -> (boxes [n, 4], scores [n]) in descending score.  A suppressed box
        carries the score -1e4, so the survivors lead: (scores > -1e4).sum() of them."""
        boxes_l, tops_l, at = [], [], 0
        for a_l in anchors:
            n = a_l.shape[0]
            sc = cls_b[at:at + n]
            k = min(cfg["nms_pre"], n)
            top, ti = _topk_stable(sc, k)
            boxes_l.append(decode_deltas(a_l[ti], reg_b[at:at + n][ti], (1.0, 1.0, 1.0, 1.0), img_hw))
            tops_l.append(top)
            at += n
        keeps = nms_keep_groups(boxes_l, cfg["nms"])                   # the levels of one image: one launch on the GPU
        scores_l = [torch.where(kp, top, top.new_full((), -1e4)) for kp, top in zip(keeps, tops_l)]
        bx, sc = torch.cat(boxes_l), torch.cat(scores_l)
        top, ti = _topk_stable(sc, min(cfg["max_per_img"], sc.numel()))
        return bx[ti], top

    def _rpn_losses_and_proposals(self, rpn_outs, anchors, targets, img_hw):
        cfg = self.rpn_cfg
        B = rpn_outs[0][0].shape[0]
        flat_a = torch.cat(anchors, 0)
        cls_all, reg_all = self._rpn_flatten(rpn_outs)
        n_pos_max, n_tot = int(cfg["num"] * cfg["pos_fraction"]), cfg["num"]
        targets = PaddedTargets.of(targets)
        # MaxIoUAssigner(pos 0.7, neg 0.3, min_pos 0.3, match_low_quality) -- configs/_base_/models/mask_rcnn_swin_fpn.py:79-85; the anchors
        # are shared by the images
        inds_all = self.assign(flat_a, targets.boxes, targets.count, cfg["pos"], cfg["neg"], cfg["min_pos"], True)[0]
        # assign, sample and encode once per batch (rpn_targets); one key vector per image, drawn in image order
        proto = cls_all.new_empty(flat_a.shape[0])
        key = torch.stack([self.rand_like(proto) for _ in range(B)])
        idx, valid, pos_valid, d_t = self.rpn_targets(inds_all, key, flat_a, targets.boxes, n_pos_max, n_tot)
        loss_cls, loss_reg = self.rpn_loss(cls_all, reg_all, idx, valid, pos_valid, d_t)             # per image, then over the batch: already / B
        with torch.no_grad():                                                                     # once per batch; the RoI head takes a list
            proposals = list(self.proposals(cls_all, reg_all, anchors, cfg, img_hw)[0].unbind(0))
        return loss_cls, loss_reg, proposals

    # -- RoI heads ------------------------------------------------------------------------------------------------------
    def _roi_losses(self, feats, proposals, targets, img_hw):
        cfg = self.rcnn_cfg
        n_tot, n_pos_max = cfg["num"], int(cfg["num"] * cfg["pos_fraction"])
        targets = PaddedTargets.of(targets)
        B, Gmax, R = len(proposals), targets.max_gt, proposals[0].shape[0]
        with torch.no_grad():
            # MaxIoUAssigner(pos 0.5, neg 0.5, min_pos 0.5, match_low_quality=True) -- mask_rcnn_swin_fpn.py:101-107; add_gt_as_proposals:
            # the padded gt rows lead
            cand_all = torch.cat([targets.boxes, torch.stack(proposals)], 1)
            inds_all = self.assign(cand_all, targets.boxes, targets.count, cfg["pos"], cfg["pos"], cfg["pos"], True, lead_gt=Gmax)[0]
            # the negatives are gt_inds == 0, and the ignored rows (the gt padding) sort behind everything in both orders, so that a
            # padding row is never drawn as a RoI or as a background filler (sample_ranks); once per batch.  One key vector per image, drawn
            # in image order: Gmax + R keys, or for padded lists the G_b + R keys of the image's own rows (the padding's key stays 0)
            def keys(n):
                k = self.rand_like(cand_all.new_empty(n + R))
                return k if n == Gmax else torch.cat([k[:n], k.new_zeros(Gmax - n), k[n:]])
            key = torch.stack([keys(n) for n in targets.list_counts or [Gmax] * B])
            rois_b, labels_b, reg_t, pos_valid, gt_idx = self.roi_targets(inds_all, key, cand_all, targets.boxes, targets.labels,
                                                                          self.num_classes, n_pos_max, n_tot, (0.1, 0.1, 0.2, 0.2))
            labels_c, pv = labels_b.reshape(-1), pos_valid.reshape(-1).float()
            pl = labels_b[:, :n_pos_max].reshape(-1).clamp(max=self.num_classes - 1)
        x = self.roi_align(feats[:4], self.STRIDES[:4], rois_b, 7)
        cls, reg = self.bbox_head(x.to(feats[0].dtype))
        # the losses take the heads' outputs as they are (bf16 under autocast): no float copy, no indexing of a prediction (losses.py)
        loss_cls = self.cls_loss(cls, labels_c)
        loss_bbox = self.box_loss(reg, labels_b, reg_t, pos_valid)
        if targets.masks is None:                                                                 # Faster R-CNN: no mask branch
            return loss_cls, loss_bbox, None
        # masks on the positive RoIs (the first n_pos_max of every image)
        xm = self.roi_align(feats[:4], self.STRIDES[:4], rois_b[:, :n_pos_max], 14)
        logits = self.mask_head(xm.to(feats[0].dtype))                                            # [B * P, classes, 28, 28]
        with torch.no_grad():                                                                     # once per batch: the assigned bitmap only
            mt = self.mask_targets(targets.masks, rois_b[:, :n_pos_max], gt_idx, pos_valid, cfg["mask_size"])
        loss_mask = self.mask_loss(logits, pl, mt, pv)
        return loss_cls, loss_bbox, loss_mask

    def heads_loss(self, feats, targets, img_hw):
        """Everything behind the backbone: dict of the 5 Mask R-CNN losses (two_stage.py:116-175).  targets: a PaddedTargets -- fixed shapes
        whatever the images' box counts, the form a captured step can be replayed on -- or a list of dicts (boxes, labels, masks) per image,
        which is padded here (PaddedTargets.of) and from then on IS one: both forms run the same assigner, sampler and target code.  Without
        masks it is the Faster R-CNN step (4 losses).  An image without boxes has only negative candidates, in either form."""
        targets = PaddedTargets.of(targets)
        if self.channels_last:
            feats = [f.contiguous(memory_format=torch.channels_last) for f in feats]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=feats[0].is_cuda):
            fpn = self.neck([f for f in feats])
            rpn_outs = self.rpn(fpn)
        anchors = make_anchors([f.shape[2:] for f in fpn], self.STRIDES, feats[0].device)
        l_rpn_cls, l_rpn_reg, proposals = self._rpn_losses_and_proposals(rpn_outs, anchors, targets, img_hw)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=feats[0].is_cuda):
            l_cls, l_bbox, l_mask = self._roi_losses(fpn, proposals, targets, img_hw)
        losses = {"loss_rpn_cls": l_rpn_cls, "loss_rpn_bbox": l_rpn_reg, "loss_cls": l_cls, "loss_bbox": l_bbox}
        if l_mask is not None:
            losses["loss_mask"] = l_mask
        return losses

    def forward_train(self, img, targets):
        return self.heads_loss(self.backbone(img), targets, img.shape[2:])

    # -- inference ------------------------------------------------------------------------------------------------------
    def _test_proposals(self, feats, img_hw):
        """What every test path starts with: the neck, the RPN head and the proposals under test_cfg["rpn"] -> (fpn, rois f32 [B, R, 4],
        scores f32 [B, R], count int32 [B])"""
        if self.channels_last:
            feats = [f.contiguous(memory_format=torch.channels_last) for f in feats]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=feats[0].is_cuda):
            fpn = self.neck([f for f in feats])
            rpn_outs = self.rpn(fpn)
        anchors = make_anchors([f.shape[2:] for f in fpn], self.STRIDES, feats[0].device)
        cls_all, reg_all = self._rpn_flatten(rpn_outs)
        rois, scores, count = self.proposals(cls_all, reg_all, anchors, self.test_cfg["rpn"], img_hw)
        return fpn, rois, scores, count

    @torch.no_grad()
    def heads_propose(self, feats, img_hw, scale_factor=None, rescale=False):
        """The RPN alone at test time (RPN.simple_test, detectors/rpn.py:96-114): a Proposals with R = test_cfg rpn max_per_img rows per
        image at most.  rescale=True: the boxes are divided by scale_factor f32 [B, 4] (w, h, w, h), as the reference does.  No host
        synchronisation, no data-dependent shape: the call can be captured and replayed, alone or with RecallAccumulator.update."""
        from ._lib import PswinError
        if rescale and scale_factor is None:
            raise PswinError("heads_propose: rescale=True needs scale_factor [B, 4]")
        _, rois, scores, count = self._test_proposals(feats, img_hw)
        return Proposals(rois / scale_factor[:, None, :] if rescale else rois, scores, count)

    @torch.no_grad()
    def simple_test_rpn(self, img, **kw):
        """backbone + heads_propose: a Proposals for the batch"""
        return self.heads_propose(self.backbone(img), img.shape[2:], **kw)

    def _paste_outputs(self, mask_logits, labels, boxes, count, thr, out_hw, mask_format, rle_capacity):
        """(masks, rle) of heads_predict for its mask_format"""
        if mask_format == "rle":
            return None, self.paste_rle(mask_logits, labels, boxes, count, thr, out_hw, rle_capacity)
        masks = self.paste(mask_logits, labels, boxes, count, thr, out_hw)
        if mask_format == "bitmap":
            return masks, None
        from . import rle
        return masks, rle.encode_masks(masks, count, rle_capacity)

    @staticmethod
    def _check_mask_format(mask_format):
        if mask_format not in ("bitmap", "rle", "both"):
            from ._lib import PswinError
            raise PswinError(f'heads_predict: mask_format must be "bitmap", "rle" or "both", got {mask_format!r}')

    @torch.no_grad()
    def heads_predict(self, feats, img_hw, scale_factor=None, rescale=False, with_masks=True, return_raw=False, ori_hw=None,
                      mask_format="bitmap", rle_capacity=None):
        """Everything behind the backbone at test time (two_stage.py:217 simple_test; test_mixins.py simple_test_bboxes / simple_test_mask):
        a Detections with K = test_cfg rcnn max_per_img rows per image.  scale_factor: f32 [B, 4] device tensor (w, h, w, h) or None.
        rescale=True: the boxes are divided by it before the NMS, as the reference does, and multiplied back to form the mask RoIs; the
        masks are then pasted at ori_hw (one size for the batch), otherwise at img_hw.  with_masks=False: the Faster R-CNN result.
        return_raw=True: also a dict of the tensors the post-processing consumed -- rois [B, R, 4], roi_count [B], cls [B, R, C + 1],
        deltas [B, R, 4 C], mask_logits [B K, C, 28, 28] -- so that the definitions can be applied to exactly those.
        mask_format: "bitmap" (masks uint8 [B, K, H, W]), "rle" (masks None, rle = the RleMasks of self.paste_rle with rle_capacity runs --
        the bitmaps are never formed) or "both".
        No host synchronisation, no host-to-device copy, no data-dependent shape: the call can be captured and replayed."""
        from ._lib import PswinError
        self._check_mask_format(mask_format)
        if rescale and (scale_factor is None or (with_masks and ori_hw is None)):
            raise PswinError("heads_predict: rescale=True needs scale_factor [B, 4] and, with masks, ori_hw=(H, W)")
        cfg = self.test_cfg["rcnn"]
        fpn, rois, _, roi_count = self._test_proposals(feats, img_hw)                             # [B, R, 4]; the survivors of the RPN's NMS lead
        B, R, C, K = rois.shape[0], rois.shape[1], self.num_classes, cfg["max_per_img"]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=feats[0].is_cuda):
            x = self.roi_align(fpn[:4], self.STRIDES[:4], rois, 7)
            cls, reg = self.bbox_head(x.to(feats[0].dtype))
        cls, reg = cls.view(B, R, C + 1), reg.view(B, R, 4 * C)
        sf = scale_factor if rescale else None
        boxes, scores, labels, count, source = self.multiclass_nms(rois, roi_count, cls, reg, self.BBOX_STDS, img_hw, sf, cfg["score_thr"],
                                                                   cfg["nms"], K)
        masks = mask_logits = rle = None
        if with_masks:
            mask_rois = boxes * sf[:, None, :] if rescale else boxes                              # back at the test scale (test_mixins.py:275-281)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=feats[0].is_cuda):
                xm = self.roi_align(fpn[:4], self.STRIDES[:4], mask_rois, 14)
                mask_logits = self.mask_head(xm.to(feats[0].dtype))                               # [B * K, classes, 28, 28]
            masks, rle = self._paste_outputs(mask_logits, labels, boxes, count, cfg["mask_thr_binary"], ori_hw if rescale else img_hw,
                                             mask_format, rle_capacity)
        out = Detections(boxes, scores, labels, count, source, masks, rle)
        if return_raw:
            return out, dict(rois=rois, roi_count=roi_count, cls=cls, deltas=reg, mask_logits=mask_logits)
        return out

    @torch.no_grad()
    def simple_test(self, img, **kw):
        """backbone + heads_predict (TwoStageDetector.simple_test): a Detections for the batch"""
        return self.heads_predict(self.backbone(img), img.shape[2:], **kw)

    # -- test-time augmentation (tta.py) ----------------------------------------------------------------------------------
    @torch.no_grad()
    def view_box_outputs(self, fpn, rois, img_hw, dtype=None):
        """The box outputs of ONE test view given its RoIs (aug_test_bboxes' loop body, test_mixins.py:170-188): fpn = the view's pyramid,
        rois f32 [B, R, 4] in the view's pixels -> (rois [B, R, 4], cls [B, R, C + 1], deltas [B, R, 4 C], stds), what the decoder takes.
        dtype: what the RoI features are cast to (default: the pyramid's)."""
        B, R, C = rois.shape[0], rois.shape[1], self.num_classes
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=rois.is_cuda):
            x = self.roi_align(fpn[:4], self.STRIDES[:4], rois, 7)
            cls, reg = self.bbox_head(x.to(dtype or fpn[0].dtype))
        return rois, cls.view(B, R, C + 1), reg.view(B, R, 4 * C), self.BBOX_STDS

    @torch.no_grad()
    def view_mask_logits(self, fpn, rois, dtype=None):
        """The mask logits of ONE test view given its RoIs (aug_test_mask's loop body, test_mixins.py:325-336): rois f32 [B, K, 4] in the
        view's pixels -> a list of [B K, C, 28, 28], one per mask head."""
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=rois.is_cuda):
            xm = self.roi_align(fpn[:4], self.STRIDES[:4], rois, 14)
            return [self.mask_head(xm.to(dtype or fpn[0].dtype))]

    def aug_heads_predict(self, feats_list, views, **kw):
        """tta.aug_heads_predict: everything behind the backbone of aug_test -- a Detections at the original image scale"""
        from . import tta
        return tta.aug_heads_predict(self, feats_list, views, **kw)

    def aug_test(self, imgs_list, views, **kw):
        """backbone per view + aug_heads_predict (TwoStageDetector.aug_test, two_stage.py:236-245): imgs_list = one image batch per view
        (pano_aug.test_views builds them), views = their tta.View"""
        from . import tta
        return tta.aug_test(self, imgs_list, views, **kw)


def synthetic_targets(batch, H, W, device, num_classes=80, seed=0):
    """COCO-shaped synthetic targets as the reference's own detector tests build them (tests/test_models/test_forward.py:
    326-392, _demo_mm_inputs: RandomState(0), 1-9 boxes per image from uniform centre / size, labels in [1, classes),
    random bitmap masks); masks here are the box interiors with a random 8 x 8 pattern so that they are learnable shapes
    of the right size rather than 50 % noise at full resolution."""
    import numpy as np
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(batch):
        n = rng.randint(1, 10)
        cx, cy, bw, bh = rng.rand(n, 4).T
        x1, y1 = ((cx * W) - (W * bw / 2)).clip(0, W), ((cy * H) - (H * bh / 2)).clip(0, H)
        x2, y2 = ((cx * W) + (W * bw / 2)).clip(0, W), ((cy * H) + (H * bh / 2)).clip(0, H)
        boxes = np.stack([x1, y1, np.maximum(x2, x1 + 2), np.maximum(y2, y1 + 2)], 1).astype(np.float32)
        labels = rng.randint(1, num_classes, size=n)
        masks = np.zeros((n, H, W), dtype=np.uint8)
        for i, (a, b, c, d) in enumerate(boxes.astype(int)):
            pat = rng.randint(0, 2, (8, 8)).astype(np.uint8)
            hh, ww = max(d - b, 1), max(c - a, 1)
            masks[i, b:b + hh, a:a + ww] = np.kron(pat, np.ones((hh // 8 + 1, ww // 8 + 1), dtype=np.uint8))[:hh, :ww]
        out.append({"boxes": torch.from_numpy(boxes).to(device), "labels": torch.from_numpy(labels).long().to(device),
                    "masks": torch.from_numpy(masks).to(device)})
    return out
