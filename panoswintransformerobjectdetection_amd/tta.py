"""Test-time augmentation: the second test path of the reference's detectors (`aug_test`), for MiniMaskRCNN and MiniCascadeRCNN.

The reference runs the backbone on several resized and / or horizontally flipped copies of an image (MultiScaleFlipAug) and merges the
heads' results: TwoStageDetector.aug_test (mmdet/models/detectors/two_stage.py:236-245), RPNTestMixin.aug_test_rpn
(mmdet/models/dense_heads/rpn_test_mixin.py), BBoxTestMixin.aug_test_bboxes and MaskTestMixin.aug_test_mask
(mmdet/models/roi_heads/test_mixins.py:166-198, 319-348), CascadeRoIHead.aug_test (mmdet/models/roi_heads/cascade_roi_head.py:416-503),
with merge_aug_proposals / merge_aug_bboxes / merge_aug_masks (mmdet/core/post_processing/merge_augs.py) and bbox_mapping /
bbox_mapping_back (mmdet/core/bbox/transforms.py:34-55).

As everywhere behind the backbone, every piece has a DEFINITION here in plain torch, float32 operation by operation (they run on CPU
tensors and are what the tests compare with), and on CUDA tensors the hot part runs as HIP kernels with fixed shapes and without a host
synchronisation (csrc/pswin_augtest.hip through ops.aug_*): a call can be captured and replayed.  A missing kernel is an error.

PARITY: map_to_view, map_back, merge_aug_bboxes (V <= 4 bit for bit), merge_aug_masks and the mapping / concatenation / re-sort / cut of
merge_aug_proposals are pinned to the reference's own functions (tests/golden/aug_test.npz, written by tools/gen_augtest_golden.py).  The
NMS proper is unpinned, as everywhere here: mmcv.ops.nms is not in the reference tree.

The reference's aug_test handles one image; here the B images of a batch share the views' geometry (View is host data, fixed when a
call is captured)."""
import torch
import torch.nn.functional as F

from . import detector as det
from .detector import _const


class View:
    """The geometry of one test view, the same for every image of a batch: img_hw = the view's unpadded (h, w) (img_meta['img_shape']),
    scale_factor = four floats (w, h, w, h) (img_meta['scale_factor']) and flip (horizontal only).  Host data."""

    def __init__(self, img_hw, scale_factor=(1.0, 1.0, 1.0, 1.0), flip=False):
        self.img_hw = (int(img_hw[0]), int(img_hw[1]))
        sf = tuple(float(s) for s in ((scale_factor,) * 4 if isinstance(scale_factor, (int, float)) else scale_factor))
        if len(sf) != 4 or min(sf) <= 0:
            raise ValueError(f"View: scale_factor is four positive floats (w, h, w, h), got {scale_factor}")
        self.scale_factor, self.flip = sf, bool(flip)

    def is_identity(self):
        return not self.flip and self.scale_factor == (1.0, 1.0, 1.0, 1.0)

    def __repr__(self):
        return f"View(img_hw={self.img_hw}, scale_factor={self.scale_factor}, flip={self.flip})"


# ------------------------------------------------------------------------------------------------------------------------
# definitions
# ------------------------------------------------------------------------------------------------------------------------
def _flip_x(boxes, w):
    """bbox_flip(direction='horizontal') (transforms.py:8-31): x0' = w - x2, x2' = w - x0; [..., 4 k]"""
    b = boxes.reshape(-1, 4)
    return torch.stack([w - b[:, 2], b[:, 1], w - b[:, 0], b[:, 3]], 1).reshape(boxes.shape)


def map_to_view(boxes, view):
    """bbox_mapping (transforms.py:34-43): boxes [..., 4 k] at the original scale -> the view's pixels.  Multiply by the scale factor,
    then flip with the view's width."""
    out = (boxes.reshape(-1, 4) * _const(view.scale_factor, boxes)).reshape(boxes.shape)
    return _flip_x(out, float(view.img_hw[1])) if view.flip else out


def map_back(boxes, view):
    """bbox_mapping_back (transforms.py:46-55): boxes [..., 4 k] in the view's pixels -> the original scale.  Un-flip with the view's
    width, then divide by the scale factor."""
    b = _flip_x(boxes, float(view.img_hw[1])) if view.flip else boxes
    return (b.reshape(-1, 4) / _const(view.scale_factor, boxes)).reshape(boxes.shape)


def merge_aug_proposals(props, scores, count, views, iou_thr, max_per_img):
    """merge_aug_proposals (merge_augs.py:12-80) for a batch: props [V, B, P, 4] in each view's pixels, scores [V, B, P], count int [V, B]
    -> (rois f32 [B, Pm, 4], scores f32 [B, Pm], count int32 [B]) with Pm = min(max_per_img, V P).  The first count[v][b] rows of every
    view are mapped back (:61-70) and concatenated view-major (:71); the greedy rule runs in descending score (a candidate is dropped when
    a kept one before it has detector.box_iou > iou_thr with it: the stand-in of mmcv.ops.nms, :72-74); the first max_per_img survivors
    in descending score are kept (:75-79).  Rows past the count are zeros.

    TIES.  The reference leaves equal scores to an unstable sort.  Here they go to the smaller concatenated position, in the rule's
    order and in the cut, as detector._topk_stable does: a captured graph and this definition must agree on the bit."""
    V, B, P = props.shape[:3]
    Pm = min(int(max_per_img), V * P)
    rois, out_scores = props.new_zeros(B, Pm, 4, dtype=torch.float32), props.new_zeros(B, Pm, dtype=torch.float32)
    out_count = torch.zeros(B, dtype=torch.int32, device=props.device)
    counts = count.tolist()
    for b in range(B):
        bx = torch.cat([map_back(props[v, b, :max(0, min(int(counts[v][b]), P))].float(), views[v]) for v in range(V)])
        sc = torch.cat([scores[v, b, :max(0, min(int(counts[v][b]), P))].float() for v in range(V)])
        order = torch.sort(sc, descending=True, stable=True)[1]
        bx, sc = bx[order], sc[order]
        n = sc.numel()
        keep = torch.ones(n, dtype=torch.bool, device=props.device)
        for i in range(n - 1):
            if keep[i]:
                keep[i + 1:] &= ~(det.box_iou(bx[i:i + 1], bx[i + 1:])[0] > iou_thr)
        bx, sc = bx[keep][:Pm], sc[keep][:Pm]
        k = sc.numel()
        rois[b, :k], out_scores[b, :k], out_count[b] = bx, sc, k
    return rois, out_scores, out_count


def merge_aug_bboxes(rois_v, cls_v, deltas_v, stds, views, dtype=torch.float32):
    """aug_test_bboxes' per-view results and merge_aug_bboxes (test_mixins.py:170-193, merge_augs.py:83-109) for a batch: rois_v
    [V, B, R, 4] in each view's pixels, cls_v [V, B, R, C + 1] logits, deltas_v [V, B, R, 4 C] (tensors or sequences of V) -> (boxes
    [B, R, 4 C], scores [B, R, C + 1]) at the original scale.  Per view: softmax, detector.decode_deltas_per_class clipped to the VIEW's
    img_hw (get_bboxes with rescale=False), map_back.  Over the views: the sum in view order, in float32, divided by V.

    That equals the reference's torch.stack(..).mean(0) bit for bit for V <= 4.  For V >= 5 torch's own summation order differs (and is
    not one answer across its kernels); the sequential order is this project's choice.  dtype: the arithmetic (float64: the truth the GPU
    test measures errors against)."""
    V = len(views)
    boxes = scores = None
    for v in range(V):
        cls, deltas, rois = cls_v[v].to(dtype), deltas_v[v].to(dtype), rois_v[v].to(dtype)
        B, R, C = cls.shape[0], cls.shape[1], cls.shape[2] - 1
        sc = F.softmax(cls, dim=-1)
        bx = det.decode_deltas_per_class(rois.reshape(B * R, 4), deltas.reshape(B * R, 4 * C), stds, views[v].img_hw)
        bx = map_back(bx, views[v]).reshape(B, R, 4 * C)
        boxes, scores = (bx, sc) if v == 0 else (boxes + bx, scores + sc)
    return boxes / float(V), scores / float(V)


def merge_aug_masks(logit_list, flips, labels):
    """aug_test_mask's per-source probabilities and merge_aug_masks (test_mixins.py:333-337, merge_augs.py:120-150) on the detections'
    own class: a list of N logits [B K, C, 28, 28], one flip flag per source, labels long [B, K] -> f32 [B K, 28, 28].  The sigmoid of the
    label's channel, reversed in x for a flipped source, summed in source order and divided by N -- what numpy's np.mean(list, axis=0)
    gives on float32 arrays, bit for bit."""
    lab = labels.reshape(-1)
    ar = torch.arange(lab.numel(), device=lab.device)
    acc = None
    for l, f in zip(logit_list, flips):
        p = l[ar, lab].float().sigmoid()
        p = p.flip(-1) if f else p
        acc = p if acc is None else acc + p
    return acc / float(len(logit_list))


def nms_merged(boxes, scores, roi_count, score_thr, iou_thr, K):
    """detector.multiclass_nms image by image on merged boxes [B, R, 4 C] and scores [B, R, C + 1], the first roi_count[b] rows of image b
    taking part (the definition of ops.multiclass_nms_boxes_batch): (boxes [B, K, 4], scores [B, K], labels long [B, K], count int32 [B],
    source int32 [B, K]) as detector.detect_post returns them."""
    B, R = scores.shape[:2]
    dev, dtype = scores.device, scores.dtype
    ob, os_ = torch.zeros(B, K, 4, dtype=dtype, device=dev), torch.zeros(B, K, dtype=dtype, device=dev)
    ol, src = torch.zeros(B, K, dtype=torch.long, device=dev), torch.zeros(B, K, dtype=torch.int32, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    for b, n in enumerate(roi_count.tolist()):
        n = max(0, min(int(n), R))
        if n == 0:
            continue
        dets, lab, flat = det.multiclass_nms(boxes[b, :n], scores[b, :n], score_thr, iou_thr, K)
        k = dets.shape[0]
        ob[b, :k], os_[b, :k], ol[b, :k], src[b, :k], cnt[b] = dets[:, :4], dets[:, 4], lab, flat.to(torch.int32), k
    return ob, os_, ol, cnt, src


def aug_detect_post(rois_v, roi_count, cls_v, deltas_v, stds, views, score_thr, iou_thr, K, dtype=torch.float32):
    """The box half of aug_test (test_mixins.py:166-198): merge_aug_bboxes, then detector.multiclass_nms per image on the merged boxes and
    scores -> nms_merged's five results."""
    boxes, scores = merge_aug_bboxes(rois_v, cls_v, deltas_v, stds, views, dtype)
    return nms_merged(boxes, scores, roi_count, score_thr, iou_thr, K)


# ------------------------------------------------------------------------------------------------------------------------
# dispatch: the definitions on CPU tensors, the kernels on CUDA tensors
# ------------------------------------------------------------------------------------------------------------------------
def merge_aug_proposals_dispatch(props, scores, count, views, iou_thr, max_per_img):
    if props.is_cuda:
        from . import ops
        return ops.aug_merge_proposals(props, scores, count, views, iou_thr, max_per_img)
    return merge_aug_proposals(props, scores, count, views, iou_thr, max_per_img)


def map_rois_dispatch(boxes, views):
    """map_to_view of boxes [B, N, 4] into every view: [V, B, N, 4] (one launch on the GPU)"""
    if boxes.is_cuda:
        from . import ops
        return ops.aug_map_rois(boxes, views)
    return torch.stack([map_to_view(boxes, v) for v in views])


def merge_aug_bboxes_dispatch(rois_v, cls_v, deltas_v, stds, views):
    if cls_v[0].is_cuda:
        from . import ops
        return ops.aug_merge_bboxes(rois_v, cls_v, deltas_v, stds, views)
    return merge_aug_bboxes(rois_v, cls_v, deltas_v, stds, views)


def nms_merged_dispatch(boxes, scores, roi_count, score_thr, iou_thr, K):
    if boxes.is_cuda:
        from . import ops
        return ops.multiclass_nms_boxes_batch(boxes, scores, roi_count, score_thr, iou_thr, K)
    return nms_merged(boxes, scores, roi_count, score_thr, iou_thr, K)


def paste_masks_aug_dispatch(logit_list, flips, labels, boxes, count, thr, out_hw):
    """detector.paste_masks of merge_aug_masks for the first count[b] detections of every image: uint8 [B, K, H, W].  On the GPU one
    launch that keeps the merged probability in LDS (ops.paste_masks_aug -> pswin_paste_masks_aug)."""
    from . import ops
    return ops.paste_masks_aug(logit_list, flips, labels, boxes, count, thr, out_hw)


# ------------------------------------------------------------------------------------------------------------------------
# the test path
# ------------------------------------------------------------------------------------------------------------------------
def _pad_rows(t, P):
    return t if t.shape[1] == P else F.pad(t, (0, 0) * (t.dim() - 2) + (0, P - t.shape[1]))


@torch.no_grad()
def aug_heads_predict(model, feats_list, views, with_masks=True, ori_hw=None, return_raw=False):
    """Everything behind the backbone of aug_test for a MiniMaskRCNN or a MiniCascadeRCNN: feats_list = the backbone's feature maps of
    every view (each a list of B-image tensors), views = their View -> a detector.Detections at the ORIGINAL image scale, masks pasted at
    ori_hw (default: the first view's img_hw).

      per view   FPN, RPN, model.proposals with the view's img_hw                                   (aug_test_rpn)
      merge      merge_aug_proposals with the test_cfg's rpn numbers; the merged RoIs mapped into every view
      per view   model.view_box_outputs: RoIAlign 7 and the box head(s) (the cascade: its three stages, refined and clipped in the view)
      merge      merge_aug_bboxes, then class-wise NMS on the merged boxes and scores                (aug_test_bboxes)
      per view   the detections mapped into the view, model.view_mask_logits: RoIAlign 14 and the mask head(s)
      merge      merge_aug_masks over all sources (the cascade: V x 3), pasted at ori_hw            (aug_test_mask)

    ONE unflipped view is not an augmentation: as BaseDetector.forward_test hands a single view to simple_test
    (mmdet/models/detectors/base.py:152-167), it goes to model.heads_predict(rescale=True) with the view's scale factor.

    return_raw=True: also a dict of what the merges consumed -- views, props / prop_scores / prop_count (the views' padded proposals),
    rois [B, R, 4] and roi_count (merged), rois_v, cls_v, deltas_v (lists of V), stds, mask_logits (list of N) and mask_flips.
    No host synchronisation, no host-to-device copy and no data-dependent shape on CUDA tensors: the call can be captured and replayed."""
    views = list(views)
    if len(views) != len(feats_list) or not views:
        raise ValueError(f"aug_heads_predict: one View per set of feature maps, got {len(views)} and {len(feats_list)}")
    ori_hw = tuple(ori_hw) if ori_hw is not None else views[0].img_hw
    dev = feats_list[0][0].device
    if len(views) == 1 and not views[0].flip:
        B = feats_list[0][0].shape[0]
        sf = _const(views[0].scale_factor, feats_list[0][0], torch.float32)[None].expand(B, 4).contiguous()
        return model.heads_predict(feats_list[0], views[0].img_hw, scale_factor=sf, rescale=True, with_masks=with_masks, return_raw=return_raw,
                                   ori_hw=ori_hw)
    rpn_cfg, cfg = model.test_cfg["rpn"], model.test_cfg["rcnn"]
    auto = dict(device_type="cuda", dtype=torch.bfloat16, enabled=dev.type == "cuda")
    fpns, props, pscores, pcount = [], [], [], []
    for feats, view in zip(feats_list, views):
        if model.channels_last:
            feats = [f.contiguous(memory_format=torch.channels_last) for f in feats]
        with torch.autocast(**auto):
            fpn = model.neck([f for f in feats])
            rpn_outs = model.rpn(fpn)
        anchors = det.make_anchors([f.shape[2:] for f in fpn], model.STRIDES, dev)
        cls_all, reg_all = model._rpn_flatten(rpn_outs)
        r, s, c = model.proposals(cls_all, reg_all, anchors, rpn_cfg, view.img_hw)
        fpns.append(fpn)
        props.append(r)
        pscores.append(s)
        pcount.append(c)
    P = max(p.shape[1] for p in props)                             # views of different sizes may yield different row counts: pad with rows
    props = torch.stack([_pad_rows(p, P) for p in props])         # the counts leave out
    pscores = torch.stack([_pad_rows(s, P) for s in pscores])
    pcount = torch.stack(pcount)
    rois, _, roi_count = merge_aug_proposals_dispatch(props, pscores, pcount, views, rpn_cfg["nms"], rpn_cfg["max_per_img"])
    B, R = rois.shape[:2]
    K = cfg["max_per_img"]
    rois_in = map_rois_dispatch(rois, views)                      # [V, B, R, 4]
    rois_v, cls_v, deltas_v = [], [], []
    for v, view in enumerate(views):
        r, c, d, stds = model.view_box_outputs(fpns[v], rois_in[v], view.img_hw, dtype=feats_list[v][0].dtype)
        rois_v.append(r)
        cls_v.append(c)
        deltas_v.append(d)
    mboxes, mscores = merge_aug_bboxes_dispatch(rois_v, cls_v, deltas_v, stds, views)
    boxes, scores, labels, count, source = nms_merged_dispatch(mboxes, mscores, roi_count, cfg["score_thr"], cfg["nms"], K)
    masks, mask_logits, mask_flips = None, None, None
    if with_masks:
        mrois = map_rois_dispatch(boxes, views)                   # [V, B, K, 4]
        mask_logits, mask_flips = [], []
        for v, view in enumerate(views):
            for l in model.view_mask_logits(fpns[v], mrois[v], dtype=feats_list[v][0].dtype):
                mask_logits.append(l)
                mask_flips.append(view.flip)
        masks = paste_masks_aug_dispatch(mask_logits, mask_flips, labels, boxes, count, cfg["mask_thr_binary"], ori_hw)
    out = det.Detections(boxes, scores, labels, count, source, masks)
    if return_raw:
        return out, dict(views=views, props=props, prop_scores=pscores, prop_count=pcount, rois=rois, roi_count=roi_count, rois_v=rois_v,
                         cls_v=cls_v, deltas_v=deltas_v, stds=stds, merged_boxes=mboxes, merged_scores=mscores, mask_logits=mask_logits,
                         mask_flips=mask_flips)
    return out


@torch.no_grad()
def aug_test(model, imgs_list, views, **kw):
    """backbone per view + aug_heads_predict (TwoStageDetector.aug_test): imgs_list = one normalised, padded image batch per view"""
    return aug_heads_predict(model, [model.backbone(img) for img in imgs_list], views, **kw)
