"""Cascade Mask R-CNN heads around the MI355X PanoSwin backbone: MiniCascadeRCNN beside detector.MiniMaskRCNN, with the configuration
numbers of configs/_base_/models/cascade_mask_rcnn_swin_fpn.py and configs/swin/cascade_mask_rcnn_swin_*_giou_4conv1f_*.

It follows the step MiniMaskRCNN takes: every piece has a DEFINITION in plain torch here (CPU and GPU), the pieces a cascade adds to the
detector's run on the GPU as HIP kernels for the whole batch (csrc/pswin_cascade.hip through ops.refine_rois / ops.giou_rows), and a
missing kernel is an error.

  refine_rois     BBoxHead.regress_by_class on the class CascadeRoIHead picks (cascade_roi_head.py:270-286 in training, :342-350 at test
                  time): the label, or for a background RoI the argmax of its foreground logits.
  giou_rows       GIoULoss(eps 1e-6) on decoded boxes, row by row (bbox_head.py:245-264 with reg_decoded_bbox=True; iou_loss.py:85-102;
                  iou2d_calculator.py:111-159), differentiable in the deltas.
  ensemble_*      the test-time mean of the three stages' class probabilities and mask probabilities (cascade_roi_head.py:352-356, 391-396),
                  handed on as logits so that the existing post-processing kernels take them.
  stage_sample /  a stage's assigner, sampler and targets with FIXED shapes, and the hand-over of its refined RoIs to the next stage:
  stage_handover  refine_bboxes' boolean filter of the ground-truth rows (bbox_head.py:445-450) becomes "ignored by the next assigner".

PARITY: the definitions of refine_rois and giou_rows are pinned to the reference's own functions (tests/golden/cascade.npz, written by
tools/gen_cascade_golden.py); the heads around them are stand-ins, as MiniMaskRCNN's are."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import detector as det
from .detector import PaddedTargets, _const

WH_CLIP = abs(math.log(16 / 1000))


# ------------------------------------------------------------------------------------------------------------------------
# definitions
# ------------------------------------------------------------------------------------------------------------------------
def decode_deltas_unclipped(src, deltas, stds):
    """detector.decode_deltas without the clip to an image (delta2bbox with max_shape=None, delta_xywh_bbox_coder.py:188-220): [N, 4].
    The clamp of dw and dh to +-|log(16 / 1000)| stays."""
    d = deltas * _const(stds, deltas)
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    sx, sy = (src[:, 0] + src[:, 2]) * 0.5, (src[:, 1] + src[:, 3]) * 0.5
    w, h = sw * d[:, 2].clamp(-WH_CLIP, WH_CLIP).exp(), sh * d[:, 3].clamp(-WH_CLIP, WH_CLIP).exp()
    x, y = sx + sw * d[:, 0], sy + sh * d[:, 1]
    return torch.stack([x - w * 0.5, y - h * 0.5, x + w * 0.5, y + h * 0.5], 1)


def giou_aligned(pred, target, eps=1e-6):
    """bbox_overlaps(pred, target, mode='giou', is_aligned=True, eps) as iou2d_calculator.py:111-159 orders its operations: [N, 4] x [N, 4]
    -> [N].  Union and enclosing area are each max(., eps) (torch.max of two tensors: on a tie its gradient is halved, as there)."""
    area1 = (pred[:, 2] - pred[:, 0]) * (pred[:, 3] - pred[:, 1])
    area2 = (target[:, 2] - target[:, 0]) * (target[:, 3] - target[:, 1])
    lt, rb = torch.max(pred[:, :2], target[:, :2]), torch.min(pred[:, 2:], target[:, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1]
    union = area1 + area2 - overlap
    enclosed_lt, enclosed_rb = torch.min(pred[:, :2], target[:, :2]), torch.max(pred[:, 2:], target[:, 2:])
    e = _const((eps,), union)                                          # a cached constant: no host-to-device copy inside a capture
    union = torch.max(union, e)
    ious = overlap / union
    enclose_wh = (enclosed_rb - enclosed_lt).clamp(min=0)
    enclose_area = torch.max(enclose_wh[:, 0] * enclose_wh[:, 1], e)
    return ious - (enclose_area - union) / enclose_area


def giou_rows(rois, deltas, labels, weight, target, stds, eps=1e-6, dtype=torch.float32):
    """The GIoU loss of every row on its decoded box: rois f32 [N, 4], deltas [N, 4 C] (any float dtype), labels long [N], weight f32 [N],
    target f32 [N, 4] -> f32 [N] = weight * (1 - giou_aligned(decode_deltas_unclipped(rois, the four deltas of class labels, stds), target)).
    Labels are clamped to [0, C).  A row whose weight is 0 contributes exactly 0 and receives a zero gradient whatever its numbers are
    (infinities included): its inputs are replaced before anything is computed from them.  Differentiable in `deltas`.
    dtype: the arithmetic (float64: the truth the tests measure errors against); the result is of that dtype."""
    N, C = deltas.shape[0], deltas.shape[1] // 4
    on = weight != 0
    lab = labels.clamp(0, C - 1)
    d4 = deltas.view(N, C, 4)[torch.arange(N, device=deltas.device), lab].to(dtype)
    zero4 = torch.zeros((), dtype=dtype, device=deltas.device)
    d4 = torch.where(on[:, None], d4, zero4)
    src = torch.where(on[:, None], rois.to(dtype), zero4)
    tgt = torch.where(on[:, None], target.to(dtype), zero4)
    w = torch.where(on, weight.to(dtype), zero4)
    loss = w * (1 - giou_aligned(decode_deltas_unclipped(src, d4, stds), tgt, eps))
    return torch.where(on, loss, zero4)


def refine_rois(rois, cls, deltas, labels, stds, img_hw, dtype=torch.float32):
    """The next stage's RoIs of a batch: rois f32 [B, R, 4], cls [B, R, C + 1] logits, deltas [B, R, 4 C], labels long [B, R] or None ->
    (new_rois [B, R, 4], used long [B, R]).  used = labels where labels < C (a negative label counts as 0), else the argmax of
    cls[..., :C] -- the first maximum, as torch.argmax has it; labels=None: the argmax for every row (the test path).  new_rois =
    detector.decode_deltas(rois, the four deltas of `used`, stds, img_hw).  No gradient.  dtype: the arithmetic of the decode."""
    with torch.no_grad():
        B, R, C = cls.shape[0], cls.shape[1], cls.shape[2] - 1
        used = torch.argmax(cls[..., :C], dim=-1)
        if labels is not None:
            used = torch.where(labels < C, labels.clamp(min=0), used)
        d4 = deltas.reshape(B * R, C, 4)[torch.arange(B * R, device=cls.device), used.reshape(-1)].to(dtype)
        new = det.decode_deltas(rois.reshape(-1, 4).to(dtype), d4, stds, img_hw)
        return new.reshape(B, R, 4), used


def ensemble_logits(cls_list):
    """log of the mean of the stages' softmaxes: a list of [B, R, C + 1] logits -> f32 [B, R, C + 1].  This is what the existing
    multiclass_nms_batch is fed: its own softmax gives the mean back, because the mean's rows sum to 1.  It differs from the reference's
    plain mean of the scores (cascade_roi_head.py:352-356) by float32 rounding only: one log and one exp per score; a mean below the
    smallest normal float32 is raised to it."""
    mean = sum(F.softmax(c.float(), dim=-1) for c in cls_list) / float(len(cls_list))
    return mean.clamp(min=torch.finfo(torch.float32).tiny).log()


def ensemble_mask_logits(logit_list, labels):
    """logit of the mean of the stages' mask probabilities of each detection's class (cascade_roi_head.py:391-396): a list of
    [B K, C, 28, 28] logits and labels long [B, K] -> f32 [B K, 1, 28, 28], to be pasted with labels 0.  The mean is kept inside
    [tiny, 1 - 2^-24] so that the logit is finite."""
    lab = labels.reshape(-1)
    ar = torch.arange(lab.numel(), device=lab.device)
    mean = sum(l[ar, lab].float().sigmoid() for l in logit_list) / float(len(logit_list))
    mean = mean.clamp(torch.finfo(torch.float32).tiny, 1.0 - 2.0 ** -24)
    return (mean.log() - torch.log1p(-mean))[:, None]


def roi_targets_ranked(gt_inds, key, cand, gt, gt_labels, num_classes, n_pos_max, n_tot, stds):
    """detector.roi_targets and the positive ranks it drew them by: (rois, labels, reg_t, pos_valid, gt_idx, pos_rank long [B, n_pos_max]).
    The ranks say WHICH candidate a positive slot holds, which the hand-over needs to recognise the ground-truth rows."""
    pos_rank = det.sample_ranks(gt_inds, key, n_pos_max, n_tot)[0]
    return det.roi_targets(gt_inds, key, cand, gt, gt_labels, num_classes, n_pos_max, n_tot, stds) + (pos_rank,)


def refine_rois_dispatch(rois, cls, deltas, labels, stds, img_hw):
    """refine_rois.  On the GPU one HIP launch that reads the logits in place (ops.refine_rois -> pswin_cascade_refine); on the CPU the
    definition."""
    if cls.is_cuda:
        from . import ops
        return ops.refine_rois(rois, cls, deltas, labels, stds, img_hw)
    return refine_rois(rois, cls, deltas, labels, stds, img_hw)


def giou_rows_dispatch(rois, deltas, labels, weight, target, stds, eps=1e-6):
    """giou_rows.  On the GPU one HIP launch per direction (ops.giou_rows -> pswin_giou_rows_fwd / _bwd); on the CPU the definition."""
    if deltas.is_cuda:
        from . import ops
        return ops.giou_rows(rois, deltas, labels, weight, target, stds, eps)
    return giou_rows(rois, deltas, labels, weight, target, stds, eps)


def roi_targets_ranked_dispatch(gt_inds, key, cand, gt, gt_labels, num_classes, n_pos_max, n_tot, stds):
    """roi_targets_ranked.  On the GPU: HIP kernels for the whole batch (ops.roi_targets_ranked -> pswin_sample_ranks, pswin_roi_targets);
    on the CPU the definition."""
    if gt_inds.is_cuda:
        from . import ops
        return ops.roi_targets_ranked(gt_inds, key, cand, gt, gt_labels, num_classes, n_pos_max, n_tot, stds)
    return roi_targets_ranked(gt_inds, key, cand, gt, gt_labels, num_classes, n_pos_max, n_tot, stds)


# ------------------------------------------------------------------------------------------------------------------------
# heads
# ------------------------------------------------------------------------------------------------------------------------
class ConvFCBBoxHead(nn.Module):
    """The 4conv1f box head's shape (ConvFCBBoxHead with num_shared_convs=4, num_shared_fcs=1, norm_cfg BN): 4 x (3 x 3 conv, BatchNorm2d,
    ReLU) on the 7 x 7 RoI features, one fc, then the cls and reg Linear layers.  The convolutions carry no bias: a norm layer follows."""

    def __init__(self, channels=256, conv_channels=256, roi=7, fc=1024, num_classes=80):
        super().__init__()
        chans = [channels] + [conv_channels] * 4
        self.convs = nn.ModuleList(nn.Conv2d(a, b, 3, padding=1, bias=False) for a, b in zip(chans[:-1], chans[1:]))
        self.norms = nn.ModuleList(nn.BatchNorm2d(conv_channels) for _ in range(4))
        self.fc = nn.Linear(conv_channels * roi * roi, fc)
        self.cls, self.reg = nn.Linear(fc, num_classes + 1), nn.Linear(fc, num_classes * 4)

    def forward(self, x):
        for c, n in zip(self.convs, self.norms):
            x = F.relu(n(c(x)))
        x = F.relu(self.fc(x.flatten(1)))
        return self.cls(x), self.reg(x)


def _mask_head(in_channels, channels, num_classes):
    m = det.MaskHead(channels, 4, num_classes)
    if channels != in_channels:
        m.convs[0] = nn.Conv2d(in_channels, channels, 3, padding=1)
    return m


class MiniCascadeRCNN(det.MiniMaskRCNN):
    """backbone -> FPN -> RPN -> three cascaded RoI stages (CascadeRoIHead) with the train_cfg numbers of
    configs/_base_/models/cascade_mask_rcnn_swin_fpn.py and the heads of the *_giou_4conv1f_* configs.  The backbone, the FPN, the RPN, its
    losses and its proposals are MiniMaskRCNN's; `heads_loss` returns the two RPN losses and, per stage i, `s{i}.loss_cls`,
    `s{i}.loss_bbox` and `s{i}.loss_mask`, each already multiplied by stage_loss_weights[i]; `heads_predict` returns a Detections from the
    ensemble of the three stages.  Both run with fixed shapes and without a host synchronisation: one captured graph each.

    Per stage: MaxIoUAssigner(pos = neg = min_pos = 0.5 / 0.6 / 0.7, match_low_quality=False), RandomSampler(512, 0.25,
    add_gt_as_proposals), cross-entropy over the sampled RoIs, GIoULoss x 10 on the positives' decoded boxes divided by the number of
    sampled RoIs, the parent's mask loss on the stage's positives.

    WHERE THE STAND-IN DEPARTS FROM THE REFERENCE
      * SyncBN of the 4conv1f heads is per-rank BatchNorm2d here.
      * The RPN's box loss stays the parent's L1 on the deltas; the cascade base config uses SmoothL1(beta 1 / 9).
      * refine_bboxes removes the sampled ground-truth boxes from the next stage's proposals, which changes their number.  Here the next
        stage's candidates are always [the padded gt rows | all 512 refined RoIs], and the refined RoIs that were ground-truth rows are
        marked ignored after the assignment (stage_sample): no sampler can draw them, and the shapes stay fixed.
      * The next stage of the reference samples from (its gt boxes + the up to 512 kept RoIs) and draws fewer than 512 when they do not hold
        enough negatives.  With fixed shapes every stage fills its 512 slots as detector.roi_targets does: negatives first.
      * Class-agnostic regression and the joint gradient clipping of the heads are not part of it.  aug_test is tta.aug_heads_predict
        through view_box_outputs / view_mask_logits below."""

    refine = staticmethod(refine_rois_dispatch)                   # a stage's class choice, regression and clip, once per batch
    giou_rows = staticmethod(giou_rows_dispatch)                  # the box loss on decoded boxes, row by row
    roi_targets_ranked = staticmethod(roi_targets_ranked_dispatch)   # a stage's sampler, RoIs, labels and the ranks of its positives
    NUM_STAGES = 3
    STAGE_LOSS_WEIGHTS = (1.0, 0.5, 0.25)
    GIOU_LOSS_WEIGHT, GIOU_EPS = 10.0, 1e-6

    def __init__(self, backbone_cfg, num_classes=80, conv_channels=256, fc_channels=1024, mask_channels=256):
        """conv_channels / fc_channels / mask_channels: the widths of the head stand-ins (the reference's: 256 / 1024 / 256; tests of the
        step's structure on the CPU take narrow ones)."""
        super().__init__(backbone_cfg, num_classes)
        del self.bbox_head, self.mask_head
        self.bbox_heads = nn.ModuleList(ConvFCBBoxHead(256, conv_channels, 7, fc_channels, num_classes) for _ in range(self.NUM_STAGES))
        self.mask_heads = nn.ModuleList(_mask_head(256, mask_channels, num_classes) for _ in range(self.NUM_STAGES))
        self.rpn_cfg = dict(self.rpn_cfg, nms_pre=2000, max_per_img=2000)            # inside ops.rpn_proposals_supported's 2048
        self.rcnn_cfg = [dict(pos=thr, num=512, pos_fraction=0.25, mask_size=28, stds=stds)
                         for thr, stds in zip((0.5, 0.6, 0.7), ((0.1, 0.1, 0.2, 0.2), (0.05, 0.05, 0.1, 0.1), (0.033, 0.033, 0.067, 0.067)))]
        for part in (self.bbox_heads, self.mask_heads):
            for m in part.modules():
                if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                    nn.init.normal_(m.weight, std=0.01)
                    if m.bias is not None:
                        nn.init.zeros_(m.bias)
        for h in self.bbox_heads:                                                     # BBoxHead.init_weights
            nn.init.normal_(h.cls.weight, 0, 0.01)
            nn.init.normal_(h.reg.weight, 0, 0.001)
            nn.init.zeros_(h.cls.bias)
            nn.init.zeros_(h.reg.bias)
        if self.channels_last:
            for part in (self.bbox_heads, self.mask_heads):
                part.to(memory_format=torch.channels_last)

    # -- training -------------------------------------------------------------------------------------------------------
    def stage_sample(self, i, cand, targets, drop=None):
        """Stage i's assigner, sampler and targets on cand f32 [B, Gmax + n, 4] = [the padded gt rows | n proposals], no gradient:
        dict(rois [B, 512, 4], labels long [B, 512], pos_valid bool [B, 128], gt_idx long [B, 128], pos_rank long [B, 128], gt_inds long
        [B, Gmax + n]).  drop: bool [B, 128] or None -- the leading proposals that were ground-truth rows of the stage before
        (stage_handover); they get gt_inds = -1 AFTER the assignment, so sample_ranks orders them behind every member and no slot holds one
        while 512 other candidates exist -- which they do: every dropped row is a box of the image, and those lead `cand` again.
        One draw of keys per image through self.rand_like, laid out as MiniMaskRCNN._roi_losses lays them out."""
        cfg = self.rcnn_cfg[i]
        n_tot, n_pos_max = cfg["num"], int(cfg["num"] * cfg["pos_fraction"])
        B, Gmax = targets.boxes.shape[:2]
        n = cand.shape[1] - Gmax
        with torch.no_grad():
            inds = self.assign(cand, targets.boxes, targets.count, cfg["pos"], cfg["pos"], cfg["pos"], False, lead_gt=Gmax)[0]
            if drop is not None:
                lead = inds[:, Gmax:Gmax + drop.shape[1]]
                inds = torch.cat([inds[:, :Gmax], torch.where(drop, torch.full_like(lead, -1), lead), inds[:, Gmax + drop.shape[1]:]], 1)

            def keys(g):
                k = self.rand_like(cand.new_empty(g + n))
                return k if g == Gmax else torch.cat([k[:g], k.new_zeros(Gmax - g), k[g:]])
            key = torch.stack([keys(g) for g in targets.list_counts or [Gmax] * B])
            rois, labels, _, pos_valid, gt_idx, pos_rank = self.roi_targets_ranked(inds, key, cand, targets.boxes, targets.labels, self.num_classes,
                                                                                   n_pos_max, n_tot, cfg["stds"])
        return dict(rois=rois, labels=labels, pos_valid=pos_valid, gt_idx=gt_idx, pos_rank=pos_rank, gt_inds=inds)

    def stage_handover(self, i, sample, cls, reg, targets, img_hw):
        """What stage i hands to stage i + 1, no gradient: (cand f32 [B, Gmax + 512, 4], drop bool [B, 128], used long [B, 512]).  cls
        [B * 512, C + 1] and reg [B * 512, 4 C]: the stage's box head on sample["rois"].  Every RoI is regressed by the deltas of its label,
        a background RoI by those of its best foreground class, and clipped to the image (self.refine); the gt rows lead the candidates
        again; drop marks the valid positives that WERE gt rows (pos_rank < Gmax), which refine_bboxes removes."""
        B, n_tot = sample["labels"].shape
        C, Gmax = self.num_classes, targets.boxes.shape[1]
        with torch.no_grad():
            new_rois, used = self.refine(sample["rois"], cls.detach().view(B, n_tot, C + 1), reg.detach().view(B, n_tot, 4 * C), sample["labels"],
                                         self.rcnn_cfg[i]["stds"], img_hw)
            drop = sample["pos_valid"] & (sample["pos_rank"] < Gmax)
            return torch.cat([targets.boxes, new_rois], 1), drop, used

    def _stage_losses(self, i, feats, sample, targets):
        """(loss_cls, loss_bbox, loss_mask or None, cls, reg) of stage i on its sample, unweighted"""
        cfg = self.rcnn_cfg[i]
        rois_b, labels_b, pos_valid, gt_idx = sample["rois"], sample["labels"], sample["pos_valid"], sample["gt_idx"]
        B, n_tot = labels_b.shape
        n_pos_max = pos_valid.shape[1]
        labels_c = labels_b.reshape(-1)
        x = self.roi_align(feats[:4], self.STRIDES[:4], rois_b, 7)
        cls, reg = self.bbox_heads[i](x.to(feats[0].dtype))
        loss_cls = self.cls_loss(cls, labels_c)
        with torch.no_grad():
            bi = torch.arange(B, device=rois_b.device)[:, None]
            weight = torch.cat([pos_valid.float(), pos_valid.new_zeros(B, n_tot - n_pos_max, dtype=torch.float32)], 1).reshape(-1)
            target = torch.cat([targets.boxes[bi, gt_idx], rois_b.new_zeros(B, n_tot - n_pos_max, 4)], 1).reshape(-1, 4)
        rows = self.giou_rows(rois_b.reshape(-1, 4), reg, labels_c, weight, target, cfg["stds"], self.GIOU_EPS)
        loss_bbox = self.GIOU_LOSS_WEIGHT * rows.float().sum() / (B * n_tot)
        if targets.masks is None:
            return loss_cls, loss_bbox, None, cls, reg
        pv = pos_valid.reshape(-1).float()
        pl = labels_b[:, :n_pos_max].reshape(-1).clamp(max=self.num_classes - 1)
        xm = self.roi_align(feats[:4], self.STRIDES[:4], rois_b[:, :n_pos_max], 14)
        logits = self.mask_heads[i](xm.to(feats[0].dtype))
        with torch.no_grad():
            mt = self.mask_targets(targets.masks, rois_b[:, :n_pos_max], gt_idx, pos_valid, cfg["mask_size"])
        return loss_cls, loss_bbox, self.mask_loss(logits, pl, mt, pv), cls, reg

    def _cascade_losses(self, feats, proposals, targets, img_hw):
        losses = {}
        cand, drop = torch.cat([targets.boxes, torch.stack(proposals)], 1), None
        for i in range(self.NUM_STAGES):
            sample = self.stage_sample(i, cand, targets, drop)
            l_cls, l_bbox, l_mask, cls, reg = self._stage_losses(i, feats, sample, targets)
            w = self.STAGE_LOSS_WEIGHTS[i]
            losses[f"s{i}.loss_cls"], losses[f"s{i}.loss_bbox"] = l_cls * w, l_bbox * w
            if l_mask is not None:
                losses[f"s{i}.loss_mask"] = l_mask * w
            if i + 1 < self.NUM_STAGES:
                cand, drop, _ = self.stage_handover(i, sample, cls, reg, targets, img_hw)
        return losses

    def heads_loss(self, feats, targets, img_hw):
        """Everything behind the backbone: the two RPN losses and the nine weighted stage losses (cascade_roi_head.py:201-288); without masks
        the six box losses.  targets: a PaddedTargets or a list of dicts per image, as MiniMaskRCNN.heads_loss takes them.  No host
        synchronisation and no data-dependent shape: with a PaddedTargets one captured step serves every batch."""
        targets = PaddedTargets.of(targets)
        if self.channels_last:
            feats = [f.contiguous(memory_format=torch.channels_last) for f in feats]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=feats[0].is_cuda):
            fpn = self.neck([f for f in feats])
            rpn_outs = self.rpn(fpn)
        anchors = det.make_anchors([f.shape[2:] for f in fpn], self.STRIDES, feats[0].device)
        l_rpn_cls, l_rpn_reg, proposals = self._rpn_losses_and_proposals(rpn_outs, anchors, targets, img_hw)
        losses = {"loss_rpn_cls": l_rpn_cls, "loss_rpn_bbox": l_rpn_reg}
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=feats[0].is_cuda):
            losses.update(self._cascade_losses(fpn, proposals, targets, img_hw))
        return losses

    # -- inference ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def heads_predict(self, feats, img_hw, scale_factor=None, rescale=False, with_masks=True, return_raw=False, ori_hw=None,
                      mask_format="bitmap", rle_capacity=None):
        """Everything behind the backbone at test time (cascade_roi_head.py:290-414): a Detections with the parent's keywords.  The
        proposals go through the three stages (argmax class, regress, clip); the class scores are the mean of the three softmaxes
        (ensemble_logits), the boxes the last stage's deltas on the last RoIs, the masks the mean over the three mask heads of the
        sigmoid of the label's channel (ensemble_mask_logits), pasted as MiniMaskRCNN pastes.  return_raw=True: also a dict of rois
        (list of three [B, R, 4]), roi_count [B], cls and deltas (lists of three), mask_logits (list of three [B K, C, 28, 28] or None).
        No host synchronisation, no data-dependent shape: the call can be captured and replayed."""
        from ._lib import PswinError
        self._check_mask_format(mask_format)
        if rescale and (scale_factor is None or (with_masks and ori_hw is None)):
            raise PswinError("heads_predict: rescale=True needs scale_factor [B, 4] and, with masks, ori_hw=(H, W)")
        cfg = self.test_cfg["rcnn"]
        auto = dict(device_type="cuda", dtype=torch.bfloat16, enabled=feats[0].is_cuda)
        fpn, rois, _, roi_count = self._test_proposals(feats, img_hw)
        B, R, C, K = rois.shape[0], rois.shape[1], self.num_classes, cfg["max_per_img"]
        rois_s, cls_s, reg_s = [rois], [], []
        for i in range(self.NUM_STAGES):
            with torch.autocast(**auto):
                x = self.roi_align(fpn[:4], self.STRIDES[:4], rois_s[i], 7)
                cls, reg = self.bbox_heads[i](x.to(feats[0].dtype))
            cls_s.append(cls.view(B, R, C + 1))
            reg_s.append(reg.view(B, R, 4 * C))
            if i + 1 < self.NUM_STAGES:
                rois_s.append(self.refine(rois_s[i], cls_s[i], reg_s[i], None, self.rcnn_cfg[i]["stds"], img_hw)[0])
        sf = scale_factor if rescale else None
        boxes, scores, labels, count, source = self.multiclass_nms(rois_s[-1], roi_count, ensemble_logits(cls_s), reg_s[-1],
                                                                   self.rcnn_cfg[-1]["stds"], img_hw, sf, cfg["score_thr"], cfg["nms"], K)
        masks = mask_logits = rle = None
        if with_masks:
            mask_rois = boxes * sf[:, None, :] if rescale else boxes
            with torch.autocast(**auto):
                xm = self.roi_align(fpn[:4], self.STRIDES[:4], mask_rois, 14).to(feats[0].dtype)
                mask_logits = [h(xm) for h in self.mask_heads]
            masks, rle = self._paste_outputs(ensemble_mask_logits(mask_logits, labels), torch.zeros_like(labels), boxes, count,
                                             cfg["mask_thr_binary"], ori_hw if rescale else img_hw, mask_format, rle_capacity)
        out = det.Detections(boxes, scores, labels, count, source, masks, rle)
        if return_raw:
            return out, dict(rois=rois_s, roi_count=roi_count, cls=cls_s, deltas=reg_s, mask_logits=mask_logits)
        return out

    # -- test-time augmentation (tta.py) ----------------------------------------------------------------------------------
    @torch.no_grad()
    def view_box_outputs(self, fpn, rois, img_hw, dtype=None):
        """The box outputs of ONE test view given its RoIs (CascadeRoIHead.aug_test's loop body, cascade_roi_head.py:424-455): the three
        stages run in the view, `refine` clips to the view's img_hw -> (the last stage's RoIs [B, R, 4], ensemble_logits of the three
        stages [B, R, C + 1], the last stage's deltas [B, R, 4 C], the last stage's stds)."""
        B, R, C = rois.shape[0], rois.shape[1], self.num_classes
        auto = dict(device_type="cuda", dtype=torch.bfloat16, enabled=rois.is_cuda)
        rois_s, cls_s, reg = [rois], [], None
        for i in range(self.NUM_STAGES):
            with torch.autocast(**auto):
                x = self.roi_align(fpn[:4], self.STRIDES[:4], rois_s[i], 7)
                cls, reg = self.bbox_heads[i](x.to(dtype or fpn[0].dtype))
            cls_s.append(cls.view(B, R, C + 1))
            reg = reg.view(B, R, 4 * C)
            if i + 1 < self.NUM_STAGES:
                rois_s.append(self.refine(rois_s[i], cls_s[i], reg, None, self.rcnn_cfg[i]["stds"], img_hw)[0])
        return rois_s[-1], ensemble_logits(cls_s), reg, self.rcnn_cfg[-1]["stds"]

    @torch.no_grad()
    def view_mask_logits(self, fpn, rois, dtype=None):
        """The mask logits of ONE test view given its RoIs (cascade_roi_head.py:476-490): a list of three [B K, C, 28, 28], one per stage's
        mask head -- merge_aug_masks takes all V x 3 as sources."""
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=rois.is_cuda):
            xm = self.roi_align(fpn[:4], self.STRIDES[:4], rois, 14).to(dtype or fpn[0].dtype)
            return [h(xm) for h in self.mask_heads]
