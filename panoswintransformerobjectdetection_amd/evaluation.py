"""Mean average precision of the detectors' fixed-shape results: the last step of train -> predict -> score, on the device.

The reference scores a model with mmdet/core/evaluation/mean_ap.py (CustomDataset.evaluate(metric='mAP') -> eval_map): class by class,
tpfp_default marks every detection of an image as true positive, false positive or ignored, the detections of all images are sorted by
score, and average_precision(mode='area') integrates the precision / recall curve.  This module states those rules as definitions on
padded batches (pure torch, any device; pinned to the reference's own results: tests/golden/eval_map.npz, tools/gen_eval_golden.py) and
runs them on the GPU as HIP kernels that read a Detections and a PaddedTargets in place (csrc/pswin_eval.hip), so that detections never
leave the device between `heads_predict` and the score:

    acc = MapAccumulator(num_classes=80, iou_thrs=(0.5, 0.75), max_per_img=100, capacity_images=5000, device="cuda")
    for batch in loader:
        acc.update(model.simple_test(img), targets)       # no host synchronisation; may be captured with the prediction
    result = acc.summarize()                              # reads back: mean_ap [T, S], ap [T, S, C], num_gts [S, C], num_dets [C]

THE MATCH IS NOT SEQUENTIAL.  In tpfp_default a detection can only match the box it overlaps most (one argmax over the class's boxes of
the image, regular boxes first and ignored ones stacked behind them, ties to the first index).  Below the threshold it is a false positive
(if its own area is inside the area range, when ranges are given); on an ignored box or one outside the range it is neither; otherwise it
is a true positive exactly when it is the first, in descending score, of the detections that chose this box with an IoU at or above the
threshold.  `match_pairs` states that, and the marks are pinned EXACTLY: the IoU is bbox_overlaps' float32 expression in its order of
operations and every comparison is made in float32.

TIES.  The reference leaves equal scores to an unstable argsort.  Here equal scores keep the order (image, row), inside an image and in the
global order: the choice detector._topk_stable makes, for the same reason (a captured graph, its replays and the definition must agree on
the bit).  Scores must be positive floats: the global order sorts their bit patterns.

MASKS.  eval_map has no mask path.  MapAccumulator's "segm" metric is this project's choice: the same matching rule on the IoU of the
full-resolution bitmaps, a pixel counting where its byte is not zero, areas being pixel counts.  The reference's own mask metric is the
COCO route (metric='segm' -> COCOeval), which CocoAccumulator below provides.

Only mode='area' and tpfp_default are in scope; '11points' and tpfp_imagenet are not.

PROPOSAL RECALL.  The reference measures the RPN alone with mmdet/core/evaluation/recall.py (evaluate(metric='proposal_fast') ->
fast_eval_recall -> eval_recalls): per image and per proposal number N, the regular ground-truth boxes are matched to the first N
proposals greedily and ONE TO ONE -- this match IS sequential: every round takes the largest IoU left, records it, and deletes its box
and its proposal -- and the recall at a threshold is the share of boxes whose recorded IoU reaches it.  `proposal_round_ious` states the
rounds (ties: the lowest box, then the lowest proposal; which proposal an equal IoU takes decides what later rounds still have, so it is
part of the contract), `recall_hits` the count, `RecallAccumulator` runs both over a data set, on the GPU as one HIP launch per batch
that reads a Proposals and a PaddedTargets in place (csrc/pswin_recall.hip).  Pinned to the reference's own results, rounds bit for bit:
tests/golden/recall.npz, tools/gen_recall_golden.py.

    acc = RecallAccumulator(proposal_nums=(100, 300, 1000), device="cuda")
    for batch in loader:
        acc.update(model.simple_test_rpn(img), targets)   # no host synchronisation; may be captured with the proposals
    result = acc.summarize()                              # reads back: recalls f64 [Kn, T], ar f64 [Kn], num_gts

THE COCO PROTOCOL.  Every swin config of the reference ends in evaluation = dict(metric='bbox') or ['bbox', 'segm']: COCOeval
(mmdet/datasets/coco.py, street.py:354-535), whose bbox_mAP / segm_mAP are the figures its logs carry.  PARITY: unpinned -- pycocotools is
neither in the reference tree nor on the build hosts, so this part is built from the published algorithm, stated here completely; the
tests hold the definitions to a plain-loop restatement and to hand-derived answers, and the kernels (csrc/pswin_coco.hip) to the
definitions bit for bit.

    acc = CocoAccumulator(num_classes=80, iou="bbox", max_dets=(100, 300, 1000), capacity_images=5000, max_per_img=100, device="cuda")
    for batch in loader:
        acc.update(model.simple_test(img), targets, crowd)    # one launch, no host synchronisation; may be captured with the prediction
    ev = acc.accumulate()                                     # precision f64 [T, 101, C, A, M], recall f64 [T, C, A, M], num_gts [A, C]
    res = acc.summarize(ev)                                   # stats f64 [12], 'bbox_mAP', 'bbox_mAP_50', ..., 'AR@100', ap_per_class

 1. RECORDS.  Per image, the detections of a class in descending score, equal scores keeping the row order; globally per class descending
    score, then (image slot, row): sort_records.  A detection's rank is its position among the detections of its class in its image; it
    counts for max_dets[m] when rank < max_dets[m].  The greedy match of the first m detections is a prefix of the full match, so the
    match is made once and cut by rank when accumulating.
 2. IOU, in double.  Boxes become x = x1, y = y1, w = x2 - x1, h = y2 - y1, each float32 widened first.  w = min(dx + dw, gx + gw) -
    max(dx, gx), likewise h; w <= 0 or h <= 0 gives 0; i = w h; the union is da + ga - i, or da alone for a crowd box; IoU = i / u.
    Masks: i, da, ga are pixel counts (a byte counts where it is non-zero), the same expression, 0 when the union is 0.  Only pairs of one
    class inside both counts exist.
 3. AREAS.  Detection: dw dh in double, or the pixel count.  Ground truth: gt_area if given (COCO's annotation field), else the same
    expression on the box or mask -- the default is this project's choice.
 4. IGNORED ground truth, per range a: crowd or area < lo_a or area > hi_a.  The interval is closed.
 5. MATCH, per (image, class, threshold t, range a), detections in rank order: the candidates are the class's boxes with iou >=
    min(t, 1 - 1e-10) that are unmatched so far or crowd; the detection takes the greatest under (not ignored before ignored, higher IoU,
    HIGHER index) -- the closed form of the published loop, which tests `<` before it assigns, so that a later equal IoU replaces an
    earlier one.  A matched detection is ignored when its box is; an unmatched one when its own area is < lo_a or > hi_a.  A matched box
    that is not crowd is taken for the rest of the chain, ignored or not.
 6. ACCUMULATE, per (t, class, a, m) over the records with rank < max_dets[m] in the global order: tp / fp are the cumulative counts of
    (matched, not ignored) / (unmatched, not ignored); npig the not-ignored boxes of (class, a).  npig == 0: every entry is -1.  Else in
    double rc = tp / npig, pr = tp / (fp + tp + 2.220446049250313e-16); recall = rc[-1] (0 without records); pr made non-increasing from
    the right; for each of np.linspace(0, 1, 101) the precision at the first index with rc >= r (searchsorted, side='left'), or 0.
 7. SUMMARIZE, in numpy on the host: each statistic is the mean over the entries > -1, or -1: AP over all t (range 0, last m), at t = 0.5
    and 0.75 (found with np.isclose), for ranges 1, 2, 3; AR for range 0 at each of the first three max_dets, for ranges 1, 2, 3 at the
    last.  COCOeval's `scores` array, the 'proposal' route (useCats = 0) and JSON files are out of scope; the masks' RLE for
    results files is rle.py (Detections.as_results); the mask metric reads bitmaps or, by _mask_route's rule, the masks' RLE.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import PswinError
from .detector import Detections, PaddedTargets, Proposals

MARK_IGNORED, MARK_TP, MARK_FP = 0, 1, 2
AP_CHUNK = 1024           # records one workgroup of pswin_ap_segments takes per trip (pswin_ap_segments_chunk(); tests aim at it)
MAX_RECORDS = 1 << 24     # the cumulative counts of a class stay exact in float32, as the reference holds them
_EPS32 = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------------------------------------------------------------
# definitions (any device)
# ------------------------------------------------------------------------------------------------------------------------
def box_areas(boxes):
    """(x2 - x1) (y2 - y1) in float32 of every row of [..., 4]"""
    b = boxes.float()
    return (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])


def _pairs(dets, gts):
    """bool [B, K, Gmax]: detection inside its count, box inside its count, one class"""
    K, G = dets.labels.shape[1], gts.labels.shape[1]
    dev = dets.labels.device
    dk = torch.arange(K, device=dev)[None, :] < dets.count[:, None]
    gk = torch.arange(G, device=dev)[None, :] < gts.count[:, None]
    return dk[:, :, None] & gk[:, None, :] & (dets.labels[:, :, None] == gts.labels[:, None, :])


def box_iou_pairs(dets, gts):
    """f32 [B, K, Gmax]: bbox_overlaps' float32 expression overlap / max(area_d + area_g - overlap, 1e-6) for the pairs with
    k < dets.count[b], g < gts.count[b] and equal labels, -1 for every other pair."""
    d, g = dets.boxes.float()[:, :, None, :], gts.boxes.float()[:, None, :, :]
    a1, a2 = box_areas(dets.boxes)[:, :, None], box_areas(gts.boxes)[:, None, :]
    xs, ys = torch.maximum(d[..., 0], g[..., 0]), torch.maximum(d[..., 1], g[..., 1])
    xe, ye = torch.minimum(d[..., 2], g[..., 2]), torch.minimum(d[..., 3], g[..., 3])
    overlap = (xe - xs).clamp(min=0) * (ye - ys).clamp(min=0)
    union = (a1 + a2 - overlap).clamp(min=1e-6)
    return torch.where(_pairs(dets, gts), overlap / union, torch.full_like(overlap, -1.0))


def mask_areas(dets, gts):
    """(f32 [B, K], f32 [B, Gmax]): the number of non-zero bytes of every mask inside its count, 0 past it"""
    def one(masks, count):
        n = (masks != 0).flatten(2).sum(2)
        inside = torch.arange(masks.shape[1], device=masks.device)[None, :] < count[:, None]
        return torch.where(inside, n, torch.zeros_like(n)).float()
    return one(dets.masks, dets.count), one(gts.masks, gts.count)


def mask_iou_pairs(dets, gts):
    """f32 [B, K, Gmax], the layout of box_iou_pairs, for dets.masks uint8 [B, K, H, W] and gts.masks uint8 [B, Gmax, H, W]: a pixel counts
    where its byte is non-zero; inter and both areas are exact integers; float32(double(inter) / double(union)), 0 when the union is 0."""
    d, g = (dets.masks != 0).flatten(2), (gts.masks != 0).flatten(2)
    dt = torch.float32 if d.shape[2] < (1 << 24) else torch.float64            # sums of 0 / 1 below 2^24: exact in float32
    inter = torch.matmul(d.to(dt), g.to(dt).transpose(1, 2)).double()
    union = d.sum(2).double()[:, :, None] + g.sum(2).double()[:, None, :] - inter
    iou = torch.where(union == 0, torch.zeros_like(inter), inter / union.clamp(min=1)).float()
    return torch.where(_pairs(dets, gts), iou, torch.full_like(iou, -1.0))


def _ranges(area_ranges, device):
    """None, or (min f32 [S], max f32 [S])"""
    if area_ranges is None:
        return None
    r = torch.tensor([[float(a), float(b)] for a, b in area_ranges], dtype=torch.float32, device=device)
    return r[:, 0], r[:, 1]


def match_pairs(iou, dets, gts, ignore, iou_thrs, area_ranges, det_area, gt_area):
    """tpfp_default on a padded batch: uint8 [T, S, B, K] of 0 (ignored, or past the count), 1 (true positive), 2 (false positive).
    iou f32 [B, K, Gmax] as box_iou_pairs / mask_iou_pairs return it (a negative entry is no candidate); ignore bool [B, Gmax] or None --
    on an argmax tie regular boxes come before ignored ones, then the lower index wins; iou_thrs: floats in (0, 1], compared as float32;
    area_ranges: None or (min_area, max_area) pairs (the reference's scale_ranges squared), compared as float32 with det_area f32 [B, K]
    and gt_area f32 [B, Gmax].  Equal scores: the lower row is in front.  Reads the counts back (a definition, not for a captured step)."""
    B, K, G = iou.shape
    dev = iou.device
    T, S = len(iou_thrs), 1 if area_ranges is None else len(area_ranges)
    thr = torch.tensor([float(t) for t in iou_thrs], dtype=torch.float32, device=dev)
    rng = _ranges(area_ranges, dev)
    marks = torch.zeros(T, S, B, K, dtype=torch.uint8, device=dev)
    for b, (nd, ng) in enumerate(zip(dets.count.tolist(), gts.count.tolist())):
        nd, ng = max(0, min(nd, K)), max(0, min(ng, G))
        if nd == 0:
            continue
        best = torch.full((nd,), -1.0, device=dev)
        arg = torch.zeros(nd, dtype=torch.long, device=dev)
        ign = torch.zeros(max(ng, 1), dtype=torch.bool, device=dev)
        if ng:
            if ignore is not None:
                ign = ignore[b, :ng].bool()
            perm = torch.sort(ign.long(), stable=True)[1]                  # regular boxes first, each group in ascending index
            v = iou[b, :nd, :ng][:, perm]
            best, first = v.max(1)[0], v.argmax(1)                         # argmax: the first of equal maxima
            arg = perm[first]
        has = best >= 0
        sc = dets.scores[b, :nd]
        rows = torch.arange(nd, device=dev)
        front = (sc[:, None] > sc[None, :]) | ((sc[:, None] == sc[None, :]) & (rows[:, None] < rows[None, :]))     # [j, k]: j before k
        same = (arg[:, None] == arg[None, :]) & has[:, None] & has[None, :]
        prev = torch.where(front & same, best[:, None].expand(nd, nd), torch.full((nd, nd), -1.0, device=dev)).max(0)[0]
        m_ign = ign[arg] & has
        for t in range(T):
            below = ~has | ~(best >= thr[t])
            for s in range(S):
                d_in = torch.ones(nd, dtype=torch.bool, device=dev)
                m_in = d_in
                if rng is not None:
                    da, ga = det_area[b, :nd], gt_area[b, arg.clamp(max=G - 1)]
                    d_in, m_in = (da >= rng[0][s]) & (da < rng[1][s]), (ga >= rng[0][s]) & (ga < rng[1][s])
                matched = torch.where(m_ign | ~m_in, 0, torch.where(prev >= thr[t], MARK_FP, MARK_TP))
                marks[t, s, b, :nd] = torch.where(below, torch.where(d_in, MARK_FP, 0), matched).to(torch.uint8)
    return marks


def count_gts(gts, ignore, gt_area, area_ranges, num_classes):
    """int32 [B, S, C]: the regular boxes of every image per (range, class) -- the reference's num_gts, image by image"""
    B, G = gts.labels.shape
    dev = gts.labels.device
    ok = (torch.arange(G, device=dev)[None, :] < gts.count[:, None]) & (gts.labels >= 0) & (gts.labels < num_classes)
    if ignore is not None:
        ok = ok & ~ignore.bool()
    rng = _ranges(area_ranges, dev)
    inr = ok[:, None, :] if rng is None else ok[:, None, :] & (gt_area[:, None, :] >= rng[0][None, :, None]) & \
        (gt_area[:, None, :] < rng[1][None, :, None])
    onehot = gts.labels.clamp(0, num_classes - 1)[:, :, None] == torch.arange(num_classes, device=dev)[None, None, :]
    return (inr[:, :, :, None] & onehot[:, None, :, :]).sum(2).to(torch.int32)


def precision_recall_sorted(marks, num_gts):
    """(recall f64 [n], precision f32 [n]) of marks uint8 [n] in sorted order, as eval_map computes them: integer cumulative counts,
    recall = tp / max(num_gts, eps) in float64, precision = float32(tp / max(tp + fp, eps))."""
    tp, fp = (marks == MARK_TP).cumsum(0), (marks == MARK_FP).cumsum(0)
    precision = tp.float() / (tp + fp).float().clamp(min=_EPS32)
    return tp.double() / max(float(num_gts), _EPS32), precision


def average_precision_sorted(marks, num_gts):
    """average_precision(mode='area') on marks uint8 [n] in sorted order: 0-dim f32.  The curve of precision_recall_sorted with (0, 0) in
    front and (1, 0) behind, precision made monotone from the right, the sum of (recall step) x precision where recall changes, in
    float64, rounded to float32.  num_gts == 0 gives 0."""
    if int(num_gts) == 0 or marks.numel() == 0:
        return torch.zeros((), dtype=torch.float32, device=marks.device)
    recall, precision = precision_recall_sorted(marks, num_gts)
    z, one = recall.new_zeros(1), recall.new_ones(1)
    mrec, mpre = torch.cat([z, recall, one]), torch.cat([z, precision.double(), z])
    mpre = torch.cummax(mpre.flip(0), 0)[0].flip(0)
    ind = torch.nonzero(mrec[1:] != mrec[:-1])[:, 0]
    return ((mrec[ind + 1] - mrec[ind]) * mpre[ind + 1]).sum().float()


def ap_segments(marks_sorted, bounds, num_gts):
    """f32 [T, S, C]: average_precision_sorted of every (threshold, range, class).  marks_sorted uint8 [T, S, N] in the global order
    (class, descending score, slot, row), bounds int [C + 1] (class c owns records bounds[c] .. bounds[c + 1] - 1), num_gts int [S, C]."""
    T, S = marks_sorted.shape[:2]
    C = bounds.numel() - 1
    bd, ng = bounds.tolist(), num_gts.tolist()
    ap = torch.zeros(T, S, C, dtype=torch.float32, device=marks_sorted.device)
    for t in range(T):
        for s in range(S):
            for c in range(C):
                ap[t, s, c] = average_precision_sorted(marks_sorted[t, s, bd[c]:bd[c + 1]], ng[s][c])
    return ap


def sort_records(scores, labels, num_classes):
    """The global order of records (score f32 [N] positive, label int32 [N] with num_classes for "no record"): (order long [N], bounds
    int32 [C + 1]).  A stable sort of the int64 key label << 32 | (0x7fffffff - the score's bit pattern): class, then descending score,
    then the position (slot, row)."""
    key = (labels.long() << 32) | (0x7FFFFFFF - scores.contiguous().view(torch.int32).long())
    order = torch.sort(key, stable=True)[1]
    bounds = torch.searchsorted(labels[order].contiguous(), torch.arange(num_classes + 1, dtype=labels.dtype, device=labels.device))
    return order, bounds.to(torch.int32)


# ------------------------------------------------------------------------------------------------------------------------
# the list form: the reference's eval_map on its own arguments
# ------------------------------------------------------------------------------------------------------------------------
def padded_from_lists(det_results, annotations, num_classes=None):
    """(Detections, PaddedTargets, ignore bool [B, Gmax], num_classes) on the CPU from eval_map's arguments: det_results per image either
    a list of per-class [n, 5] arrays (x1, y1, x2, y2, score) or what Detections.as_lists() gives, (dets [k, 5], labels [k], masks);
    annotations per image a dict of bboxes [n, 4], labels [n] and optionally bboxes_ignore, labels_ignore.  Rows keep their order (class
    by class for the per-class form); ignored boxes follow the regular ones, as tpfp_default stacks them."""
    rows = []
    for res in det_results:
        if isinstance(res, tuple) and len(res) == 3 and torch.is_tensor(res[0]):
            if num_classes is None:
                raise PswinError("padded_from_lists: the Detections.as_lists() form needs num_classes")
            rows.append((res[0].detach().cpu().float().reshape(-1, 5), res[1].detach().cpu().long().reshape(-1)))
        else:
            num_classes = len(res) if num_classes is None else num_classes
            d = [torch.as_tensor(np.asarray(a, dtype=np.float32)).reshape(-1, 5) for a in res]
            rows.append((torch.cat(d), torch.cat([torch.full((a.shape[0],), c, dtype=torch.long) for c, a in enumerate(d)])))
    B, K = len(rows), max(1, max(r[0].shape[0] for r in rows))
    dets = Detections(torch.zeros(B, K, 4), torch.zeros(B, K), torch.zeros(B, K, dtype=torch.long),
                      torch.tensor([r[0].shape[0] for r in rows], dtype=torch.int32), torch.zeros(B, K, dtype=torch.int32))
    for b, (d, l) in enumerate(rows):
        dets.boxes[b, :len(l)], dets.scores[b, :len(l)], dets.labels[b, :len(l)] = d[:, :4], d[:, 4], l
    gl = []
    for ann in annotations:
        bx = torch.as_tensor(np.asarray(ann["bboxes"], dtype=np.float32)).reshape(-1, 4)
        lb = torch.as_tensor(np.asarray(ann["labels"])).long().reshape(-1)
        ig = torch.zeros(lb.shape[0], dtype=torch.bool)
        if ann.get("labels_ignore", None) is not None:
            bi = torch.as_tensor(np.asarray(ann["bboxes_ignore"], dtype=np.float32)).reshape(-1, 4)
            li = torch.as_tensor(np.asarray(ann["labels_ignore"])).long().reshape(-1)
            bx, lb, ig = torch.cat([bx, bi]), torch.cat([lb, li]), torch.cat([ig, torch.ones(li.shape[0], dtype=torch.bool)])
        gl.append((bx, lb, ig))
    G = max(1, max(g[1].shape[0] for g in gl))
    gts = PaddedTargets(torch.zeros(B, G, 4), torch.zeros(B, G, dtype=torch.long), torch.tensor([g[1].shape[0] for g in gl], dtype=torch.int32))
    ignore = torch.zeros(B, G, dtype=torch.bool)
    for b, (bx, lb, ig) in enumerate(gl):
        gts.boxes[b, :len(lb)], gts.labels[b, :len(lb)], ignore[b, :len(lb)] = bx, lb, ig
    return dets, gts, ignore, num_classes


def eval_map_lists(det_results, annotations, scale_ranges=None, iou_thr=0.5, num_classes=None):
    """The reference's eval_map(det_results, annotations, scale_ranges, iou_thr) from the definitions above, with its return value:
    (mean_ap, [dict(num_gts, num_dets, recall, precision, ap) per class]) -- scalars without scale_ranges, one entry per range with
    them.  det_results may also be what Detections.as_lists() produces (then num_classes is required)."""
    dets, gts, ignore, C = padded_from_lists(det_results, annotations, num_classes)
    area_ranges = None if scale_ranges is None else [(r[0] ** 2, r[1] ** 2) for r in scale_ranges]
    S = 1 if area_ranges is None else len(area_ranges)
    det_area, gt_area = box_areas(dets.boxes), box_areas(gts.boxes)
    marks = match_pairs(box_iou_pairs(dets, gts), dets, gts, ignore, (iou_thr,), area_ranges, det_area, gt_area)[0]     # [S, B, K]
    num_gts = count_gts(gts, ignore, gt_area, area_ranges, C).sum(0)                                                      # [S, C]
    live = torch.arange(dets.labels.shape[1])[None, :] < dets.count[:, None]
    results = []
    for c in range(C):
        sel = (live & (dets.labels == c)).reshape(-1)
        order = torch.sort(dets.scores.reshape(-1)[sel], descending=True, stable=True)[1]
        rec, pre, ap = [], [], []
        for s in range(S):
            m = marks[s].reshape(-1)[sel][order]
            r, p = precision_recall_sorted(m, int(num_gts[s, c]))
            rec.append(r.numpy()), pre.append(p.numpy()), ap.append(average_precision_sorted(m, int(num_gts[s, c])).numpy())
        if scale_ranges is None:
            results.append(dict(num_gts=int(num_gts[0, c]), num_dets=int(sel.sum()), recall=rec[0], precision=pre[0], ap=ap[0][()]))
        else:
            results.append(dict(num_gts=num_gts[:, c].numpy().astype(int), num_dets=int(sel.sum()), recall=np.stack(rec),
                                precision=np.stack(pre), ap=np.stack(ap)))
    aps = np.array([[np.float64(np.reshape(r["ap"], -1)[s]) for r in results] for s in range(S)]).reshape(S, C)
    has = num_gts.numpy() > 0
    mean_ap = [float(aps[s][has[s]].mean()) if has[s].any() else 0.0 for s in range(S)]
    return (mean_ap[0] if scale_ranges is None else mean_ap), results


# ------------------------------------------------------------------------------------------------------------------------
# the kernels (csrc/pswin_eval.hip) and the dispatch: on CPU tensors every step runs the definitions
# ------------------------------------------------------------------------------------------------------------------------
def _floats(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


def _check_batch(dets, gts):
    B, K = dets.labels.shape
    if gts.labels.shape[0] != B:
        raise PswinError(f"evaluation: {B} images of detections, {gts.labels.shape[0]} of targets")
    for name, t, dt in (("dets.boxes", dets.boxes, torch.float32), ("dets.scores", dets.scores, torch.float32),
                        ("dets.labels", dets.labels, torch.int64), ("dets.count", dets.count, torch.int32),
                        ("targets.boxes", gts.boxes, torch.float32), ("targets.labels", gts.labels, torch.int64),
                        ("targets.count", gts.count, torch.int32)):
        if t.dtype != dt or not t.is_contiguous() or t.device != dets.labels.device:
            raise PswinError(f"evaluation: {name} must be a contiguous {dt} tensor on {dets.labels.device}")


def _check_masks(dets, gts):
    if dets.masks is None or gts.masks is None:
        raise PswinError("evaluation: the mask metric needs dets.masks and targets.masks")
    if dets.masks.shape[2:] != gts.masks.shape[2:] or dets.masks.dtype != torch.uint8 or gts.masks.dtype != torch.uint8:
        raise PswinError(f"evaluation: masks must be uint8 of one size, got {tuple(dets.masks.shape)} {dets.masks.dtype} and "
                         f"{tuple(gts.masks.shape)} {gts.masks.dtype}")


def _mask_route(dets, gts):
    """How the mask metric reads a batch's masks -- ONE rule for pair_iou_dispatch, mask / rle_inter_pairs_dispatch and both accumulators:
    "bitmap" if both sides have bitmaps (dets.masks and targets.masks; the route and the bits it always had); otherwise "rle" if each side
    has bitmaps or runs (dets.rle / targets.rle, rle.RleMasks) -- a side that has only bitmaps is encoded on the spot with
    rle.encode_masks(masks, count), four launches and still capturable; otherwise the PswinError of _check_masks.  The sizes (height,
    width) of the two sides must agree."""
    d_rle, g_rle = getattr(dets, "rle", None), getattr(gts, "rle", None)
    if (dets.masks is not None and gts.masks is not None) or (dets.masks is None and d_rle is None) or (gts.masks is None and g_rle is None):
        _check_masks(dets, gts)
        return "bitmap"
    B, K, G = dets.labels.shape[0], dets.labels.shape[1], gts.labels.shape[1]
    sizes = []
    for who, side, rows in (("dets", dets, K), ("targets", gts, G)):
        if side.masks is not None:
            if side.masks.dtype != torch.uint8 or tuple(side.masks.shape[:2]) != (B, rows) or side.masks.dim() != 4:
                raise PswinError(f"evaluation: {who}.masks must be uint8 [{B}, {rows}, H, W], got {side.masks.dtype} {tuple(side.masks.shape)}")
            sizes.append(tuple(int(v) for v in side.masks.shape[2:]))
        else:
            enc = side.rle
            if enc.offsets.numel() != B * rows + 1 or enc.offsets.dtype != torch.int64 or enc.runs.dtype != torch.uint32 or \
                    enc.offsets.device != dets.labels.device or enc.runs.device != dets.labels.device or not enc.offsets.is_contiguous() or \
                    not enc.runs.is_contiguous() or not 1 <= enc.capacity <= enc.runs.numel():
                raise PswinError(f"evaluation: {who}.rle must hold int64 offsets [{B * rows + 1}] and uint32 runs of its capacity on "
                                 f"{dets.labels.device}")
            sizes.append((enc.height, enc.width))
    if sizes[0] != sizes[1]:
        raise PswinError(f"evaluation: masks of one size, got {sizes[0]} for the detections and {sizes[1]} for the targets")
    return "rle"


def _rle_sides(dets, gts):
    """(det_rle, gt_rle) of the "rle" route: the side's runs, or its bitmaps encoded on the spot"""
    from . import rle
    d = dets.rle if dets.masks is None else rle.encode_masks(dets.masks.contiguous(), dets.count)
    g = gts.rle if gts.masks is None else rle.encode_masks(gts.masks.contiguous(), gts.count)
    return d, g


def rle_inter_workspace(B, K, G, det_capacity, gt_capacity, device):
    """a fresh workspace of pswin_rle_inter_workspace bytes for pswin_rle_inter_pairs / pswin_rle_iou_pairs"""
    nbytes = ctypes.c_longlong(0)
    _lib.check(_lib.load().pswin_rle_inter_workspace(B, K, G, int(det_capacity), int(gt_capacity), ctypes.byref(nbytes)),
               "pswin_rle_inter_workspace")
    return torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)


def _rle_pairs_args(dets, gts, d, g, who):
    (B, K), G = dets.labels.shape, gts.labels.shape[1]
    if not (1 <= B <= 65535 and 1 <= K <= COCO_MAX_K and 1 <= G <= COCO_MAX_G and d.height * d.width < 1 << 31):
        raise PswinError(f"{who}: B = {B}, K = {K}, Gmax = {G}, {d.height} x {d.width} is outside the run-length kernels' limits "
                         f"(K <= {COCO_MAX_K}, Gmax <= {COCO_MAX_G}, H W < 2^31)")
    p = _lib.ptr
    return (p(d.offsets), p(d.runs), d.capacity, p(dets.labels), p(dets.count), p(g.offsets), p(g.runs), g.capacity, p(gts.labels),
            p(gts.count), B, K, G, d.height, d.width)


def _iou_from_counts(inter, areas, K):
    """mask_iou_pairs' float32 IoU and mask_areas' two f32 areas from inter_pairs' integers"""
    da, ga = areas[:, :K].double(), areas[:, K:].double()
    union = da[:, :, None] + ga[:, None, :] - inter.double()
    iou = torch.where(union == 0, torch.zeros_like(union), inter.double() / union.clamp(min=1)).float()
    return torch.where(inter < 0, torch.full_like(iou, -1.0), iou), da.float(), ga.float()


def _out(out, shape, dtype, device, what):
    """`out` after a check of its shape, or a fresh buffer"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise PswinError(f"{what}: out must be a contiguous {dtype} tensor {tuple(shape)} on {device}")
    return out


def pair_iou_dispatch(dets, gts, iou="bbox", out=None, rle_overflow=None):
    """(iou f32 [B, K, Gmax], det_area f32 [B, K], gt_area f32 [B, Gmax]) of the box or the mask metric.  On the GPU: pswin_box_iou_pairs,
    pswin_mask_iou_pairs or, by _mask_route's rule, pswin_rle_iou_pairs on the masks' runs, into the three buffers of `out` if given; on
    the CPU the definitions.  rle_overflow: an int32 [1] flag on the device that the run-length route sets when a run pool was too small
    (rle.inter_pairs_definition says what the results are then); it is never cleared here."""
    _check_batch(dets, gts)
    route = None
    if iou == "segm":
        route = _mask_route(dets, gts)
    elif iou != "bbox":
        raise PswinError(f"evaluation: iou must be 'bbox' or 'segm', got {iou!r}")
    if not dets.labels.is_cuda:
        if route == "rle":
            inter, areas, over = rle_inter_pairs_dispatch(dets, gts)
            if rle_overflow is not None:
                rle_overflow |= over
            return _iou_from_counts(inter, areas, dets.labels.shape[1])
        if iou == "segm":
            return (mask_iou_pairs(dets, gts),) + mask_areas(dets, gts)
        return box_iou_pairs(dets, gts), box_areas(dets.boxes), box_areas(gts.boxes)
    (B, K), G = dets.labels.shape, gts.labels.shape[1]
    dev, bufs = dets.labels.device, out or (None, None, None)
    out = _out(bufs[0], (B, K, G), torch.float32, dev, "pair_iou_dispatch")
    det_area, gt_area = _out(bufs[1], (B, K), torch.float32, dev, "pair_iou_dispatch"), _out(bufs[2], (B, G), torch.float32, dev, "pair_iou_dispatch")
    p = _lib.ptr
    if route == "rle":
        d, g = _rle_sides(dets, gts)
        args = _rle_pairs_args(dets, gts, d, g, "pair_iou_dispatch")
        over = torch.zeros(1, dtype=torch.int32, device=dev) if rle_overflow is None else _out(rle_overflow, (1,), torch.int32, dev, "pair_iou_dispatch")
        ws = rle_inter_workspace(B, K, G, d.capacity, g.capacity, dev)
        _lib.call("pswin_rle_iou_pairs", out, *args, p(out), p(det_area), p(gt_area), p(over), p(ws), algo_bytes=12 * (d.capacity + g.capacity))
    elif iou == "segm":
        dm, gm = dets.masks.contiguous(), gts.masks.contiguous()
        H, W = dm.shape[2:]
        n = _lib.load().pswin_mask_iou_workspace(B, K, G)
        _lib.check(min(n, 0), "pswin_mask_iou_workspace")
        ws = torch.empty(n, dtype=torch.uint8, device=out.device)
        pairs = B * K * G                                  # an upper bound of the bytes read: every pair of one class inside the counts
        _lib.call("pswin_mask_iou_pairs", out, p(dm), p(dets.labels), p(dets.count), p(gm), p(gts.labels), p(gts.count), B, K, G, H, W, p(out),
                  p(det_area), p(gt_area), p(ws), algo_bytes=(B * (K + G) + 2 * pairs) * H * W)
    else:
        _lib.call("pswin_box_iou_pairs", out, p(dets.boxes), p(dets.labels), p(dets.count), p(gts.boxes), p(gts.labels), p(gts.count), B, K, G,
                  p(out), p(det_area), p(gt_area), algo_bytes=B * (K + G) * 24 + B * K * G * 4)
    return out, det_area, gt_area


def _flags(ignore, gts):
    if ignore is None:
        return None
    if ignore.shape != gts.labels.shape or ignore.dtype not in (torch.bool, torch.uint8) or ignore.device != gts.labels.device:
        raise PswinError(f"evaluation: ignore must be bool {tuple(gts.labels.shape)} on {gts.labels.device}")
    return ignore.contiguous()


def ap_segments_dispatch(marks_sorted, bounds, num_gts, out=None):
    """ap_segments.  On the GPU one launch, a workgroup per (threshold, range, class) (pswin_ap_segments), into `out` if given; on the CPU
    the definition."""
    if not marks_sorted.is_cuda:
        return ap_segments(marks_sorted, bounds, num_gts)
    T, S, N = marks_sorted.shape
    C = bounds.numel() - 1
    marks_sorted, bounds, num_gts = marks_sorted.contiguous(), bounds.to(torch.int32).contiguous(), num_gts.to(torch.int32).contiguous()
    if tuple(num_gts.shape) != (S, C) or marks_sorted.dtype != torch.uint8:
        raise PswinError(f"ap_segments: marks uint8 [T, S, N], bounds [C + 1], num_gts [S, C]; got {tuple(marks_sorted.shape)}, "
                         f"{tuple(bounds.shape)}, {tuple(num_gts.shape)}")
    ap = _out(out, (T, S, C), torch.float32, marks_sorted.device, "ap_segments_dispatch")
    _lib.call("pswin_ap_segments", ap, _lib.ptr(marks_sorted), _lib.ptr(bounds), _lib.ptr(num_gts), T, S, C, N, _lib.ptr(ap),
              algo_bytes=2 * T * S * N)
    return ap


_RLE_OVERFLOW = ("{}: a run pool was too small for its masks (RleMasks.offsets[N] > capacity), so masks were scored as empty; produce the "
                 "runs again with a larger capacity (heads_predict's rle_capacity, encode_masks' capacity)")


class MapAccumulator:
    """mAP over a data set, batch by batch, in buffers of a fixed shape on `device`.  iou_thrs: T thresholds; scale_ranges: None or S
    pairs as the reference's eval_map takes them (their squares bound the areas); capacity_images: the image slots; max_per_img: K, the
    rows of a Detections; iou: "bbox" or "segm".

    A record is a detection row's score f32, label int32 and its T x S marks; image `cursor + b` of all updates owns rows
    [slot K, slot K + K) of rec_score / rec_label [capacity, K] and rec_marks [T, S, capacity, K].  An unused row carries label C."""

    def __init__(self, num_classes, iou_thrs=(0.5,), scale_ranges=None, capacity_images=1024, max_per_img=100, iou="bbox", device="cpu"):
        self.C, self.K, self.capacity, self.iou = int(num_classes), int(max_per_img), int(capacity_images), iou
        self.iou_thrs = tuple(float(t) for t in iou_thrs)
        self.area_ranges = None if scale_ranges is None else tuple((float(r[0]) ** 2, float(r[1]) ** 2) for r in scale_ranges)
        self.T, self.S = len(self.iou_thrs), 1 if scale_ranges is None else len(scale_ranges)
        if iou not in ("bbox", "segm"):
            raise PswinError(f"MapAccumulator: iou must be 'bbox' or 'segm', got {iou!r}")
        if not (self.C >= 1 and self.K >= 1 and self.capacity >= 1 and 1 <= self.T <= 16 and 1 <= self.S <= 8):
            raise PswinError("MapAccumulator: num_classes, max_per_img, capacity_images >= 1, 1 to 16 thresholds, 1 to 8 ranges")
        if any(not 0 < t <= 1 for t in self.iou_thrs):
            raise PswinError(f"MapAccumulator: thresholds must lie in (0, 1], got {self.iou_thrs}")
        if self.capacity * self.K > MAX_RECORDS:
            raise PswinError(f"MapAccumulator: capacity_images x max_per_img must not exceed {MAX_RECORDS} records")
        dev = torch.device(device)
        self.rec_score = torch.zeros(self.capacity, self.K, device=dev)
        self.rec_label = torch.full((self.capacity, self.K), self.C, dtype=torch.int32, device=dev)
        self.rec_marks = torch.zeros(self.T, self.S, self.capacity, self.K, dtype=torch.uint8, device=dev)
        self.num_gts = torch.zeros(self.S, self.C, dtype=torch.int32, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        self.rle_overflow = torch.zeros(1, dtype=torch.int32, device=dev)          # set by the run-length route of "segm" (_mask_route)

    def reset(self):
        """Forget every record, in place (stream-ordered; the buffers keep their addresses for a captured update)."""
        self.rec_score.zero_(), self.rec_marks.zero_(), self.num_gts.zero_(), self.cursor.zero_(), self.overflow.zero_()
        self.rle_overflow.zero_()
        self.rec_label.fill_(self.C)
        return self

    def update(self, dets, targets, ignore=None, out=None):
        """Score one batch: marks uint8 [T, S, B, K], and the batch's records appended at the cursor, which advances by B.  dets: a
        Detections with K = max_per_img rows; targets: a PaddedTargets, or the list form, padded on entry (PaddedTargets.of: the one
        host read, of the lists' box counts); ignore: bool [B, Gmax] or None.  No host synchronisation and no data-dependent shape: it
        can be captured with the prediction.  An image without detections and boxes contributes nothing, so a short last batch is padded
        with such images.  Image slots at or past the capacity are not written; summarize() raises then.  out: the GPU path's buffer for
        the marks, if the caller keeps one.  Polygon ground truth for iou="segm": targets.rle = polygons.polygons_to_rle(PolygonBatch) is
        an RleMasks like any other."""
        gts = PaddedTargets.of(targets)
        B, K = dets.labels.shape
        if K != self.K or dets.labels.device != self.cursor.device:
            raise PswinError(f"MapAccumulator.update: detections [{B}, {K}] on {dets.labels.device}, the accumulator holds max_per_img = "
                             f"{self.K} on {self.cursor.device}")
        ignore = _flags(ignore, gts)
        iou, det_area, gt_area = pair_iou_dispatch(dets, gts, self.iou, rle_overflow=self.rle_overflow)
        G = gts.labels.shape[1]
        if not iou.is_cuda:
            marks = match_pairs(iou, dets, gts, ignore, self.iou_thrs, self.area_ranges, det_area, gt_area)
            per_image = count_gts(gts, ignore, gt_area, self.area_ranges, self.C)
            live = torch.arange(K)[None, :] < dets.count[:, None]
            label = torch.where(live & (dets.labels >= 0) & (dets.labels < self.C), dets.labels, self.C).to(torch.int32)
            score = torch.where(live, dets.scores, torch.zeros_like(dets.scores))
            for b in range(B):
                slot = int(self.cursor) + b
                if slot >= self.capacity:
                    self.overflow.fill_(1)
                    continue
                self.rec_score[slot], self.rec_label[slot], self.rec_marks[:, :, slot] = score[b], label[b], marks[:, :, b]
                self.num_gts += per_image[b]
        else:
            marks = _out(out, (self.T, self.S, B, K), torch.uint8, iou.device, "MapAccumulator.update")
            p = _lib.ptr
            ranges = None if self.area_ranges is None else _floats([v for r in self.area_ranges for v in r])
            _lib.call("pswin_eval_match", iou, p(iou), p(dets.scores), p(dets.labels), p(dets.count), p(gts.labels), p(gts.count), p(ignore),
                      p(det_area), p(gt_area), _floats(self.iou_thrs), self.T, ranges, self.S, B, K, G, self.C, self.capacity, p(self.cursor),
                      p(marks), p(self.rec_score), p(self.rec_label), p(self.rec_marks), p(self.num_gts), p(self.overflow),
                      algo_bytes=B * K * G * 4 + 2 * self.T * self.S * B * K + B * K * 24)
        self.cursor.add_(B)
        return marks

    def summarize(self):
        """Reads back: dict(mean_ap f32 [T, S], ap f32 [T, S, C], num_gts int32 [S, C], num_dets int32 [C]) on the CPU.  mean_ap is the mean
        over the classes with num_gts > 0, or 0.0 if there are none, as the reference reports it."""
        if int(self.overflow):
            raise PswinError(f"MapAccumulator: more than capacity_images = {self.capacity} images were given; the records past it are lost")
        if int(self.rle_overflow):
            raise PswinError(_RLE_OVERFLOW.format("MapAccumulator"))
        order, bounds = sort_records(self.rec_score.reshape(-1), self.rec_label.reshape(-1), self.C)
        marks_sorted = self.rec_marks.reshape(self.T, self.S, -1).index_select(2, order)
        ap = ap_segments_dispatch(marks_sorted, bounds, self.num_gts).cpu()
        num_gts, bounds = self.num_gts.cpu(), bounds.cpu()
        has = num_gts > 0
        mean_ap = torch.zeros(self.T, self.S)
        for s in range(self.S):
            if has[s].any():
                mean_ap[:, s] = ap[:, s, has[s]].double().mean(1).float()
        return dict(mean_ap=mean_ap, ap=ap, num_gts=num_gts, num_dets=bounds[1:] - bounds[:-1])


# ------------------------------------------------------------------------------------------------------------------------
# proposal recall: definitions (any device)
# ------------------------------------------------------------------------------------------------------------------------
RECALL_MAX_G, RECALL_MAX_R = 512, 2048          # boxes and proposals per image one workgroup of pswin_recall_match keeps in LDS
DEFAULT_RECALL_THRS = np.arange(0.5, 0.96, 0.05)


def _thresholds(iou_thrs):
    """float64 [T] of a number, a sequence or an array, every value as it came"""
    return np.atleast_1d(np.asarray(iou_thrs, dtype=np.float64)).reshape(-1)


def box_iou_matrix(rows, cols):
    """f32 [g, n] of boxes [g, 4] and [n, 4]: box_iou_pairs' expression without counts and labels.  Symmetric in its operands bit for bit
    (float addition, max and min commute), so the reference's exchange of the operands when there are more rows than columns is
    invisible."""
    r, c = rows.float()[:, None, :], cols.float()[None, :, :]
    xs, ys = torch.maximum(r[..., 0], c[..., 0]), torch.maximum(r[..., 1], c[..., 1])
    xe, ye = torch.minimum(r[..., 2], c[..., 2]), torch.minimum(r[..., 3], c[..., 3])
    overlap = (xe - xs).clamp(min=0) * (ye - ys).clamp(min=0)
    return overlap / (box_areas(rows)[:, None] + box_areas(cols)[None, :] - overlap).clamp(min=1e-6)


def greedy_rounds(iou):
    """f32 [g] of iou f32 [g, n]: round j's IoU.  Every round takes, among the live rows and live columns, every row's largest entry at
    its lowest column, then the lowest row among the largest of those; it records the value and deletes the row and the column.  Rounds
    j >= n > 0 record -1; n == 0 records 0 in every round."""
    g, n = iou.shape
    rec = iou.new_zeros(g)
    if n == 0 or g == 0:
        return rec
    live_r, live_c = torch.ones(g, dtype=torch.bool, device=iou.device), torch.ones(n, dtype=torch.bool, device=iou.device)
    gone = iou.new_full((), float("-inf"))
    for j in range(g):
        if j >= n:
            rec[j:] = -1.0
            break
        m = torch.where(live_r[:, None] & live_c[None, :], iou, gone)
        col = m.argmax(1)                                  # argmax: the first of equal maxima
        best = m.gather(1, col[:, None])[:, 0]
        r = best.argmax()
        rec[j] = best[r]
        live_r[r], live_c[col[r]] = False, False
    return rec


def proposal_round_ious(props, gts, proposal_nums, ignore=None):
    """f32 [Kn, B, Gmax]: out[k, b, j] is the IoU that round j of the greedy one-to-one matching records (greedy_rounds) for image b with
    its first n = min(clamp(props.count[b], 0, R), proposal_nums[k]) proposals as columns and, as rows, its boxes inside gts.count[b] that
    `ignore` (bool [B, Gmax] or None) does not flag, in their order.  The index is the ROUND, not the box.  There is no label test:
    proposals have no class.  Slots past the number of rows hold -2.  Reads the counts back (a definition, not for a captured step)."""
    (B, R), G = props.scores.shape, gts.boxes.shape[1]
    nums = [int(v) for v in proposal_nums]
    out = torch.full((len(nums), B, G), -2.0, dtype=torch.float32, device=props.boxes.device)
    for b, (npr, ng) in enumerate(zip(props.count.tolist(), gts.count.tolist())):
        npr, ng = max(0, min(npr, R)), max(0, min(ng, G))
        rows = gts.boxes[b, :ng].float()
        if ignore is not None:
            rows = rows[~ignore[b, :ng].bool()]
        if rows.shape[0] == 0:
            continue
        iou = box_iou_matrix(rows, props.boxes[b, :npr])
        for k, num in enumerate(nums):
            out[k, b, :rows.shape[0]] = greedy_rounds(iou[:, :max(0, min(npr, num))])
    return out


def _recall_hits(rounds, iou_thrs):
    """(hits int64 [Kn, T], num_gts int64 0-dim) as tensors on rounds' device"""
    thr = torch.as_tensor(_thresholds(iou_thrs), device=rounds.device)
    real = rounds > -2
    hit = (rounds.double()[..., None] >= thr) & real[..., None]
    return hit.sum((1, 2)), real[0].sum()


def recall_hits(rounds, iou_thrs):
    """(hits int64 [Kn, T], num_gts int) of rounds f32 [Kn, B, Gmax]: per (proposal number, threshold) the slots with a value > -2 (a
    round of a box) and double(value) >= double(threshold); num_gts is the number of such slots of one proposal number.  THE COMPARISON
    IS IN DOUBLE, on thresholds kept as float64: the reference compares its float32 IoUs with a float64 threshold array, and with
    np.arange(0.5, 0.96, 0.05) an IoU of exactly 0.65, 0.7, 0.75, 0.9 or 0.95 in float32 is then a miss at the threshold of that name,
    where a float32 comparison calls it a hit.  This is NOT the float32 comparison match_pairs / MapAccumulator make (tpfp_default
    compares float32 with a Python float, which numpy keeps in float32)."""
    hits, num = _recall_hits(rounds, iou_thrs)
    return hits, int(num)


def eval_recalls_lists(gts, proposals, proposal_nums=(100, 300, 1000), iou_thrs=0.5):
    """The reference's eval_recalls(gts, proposals, proposal_nums, iou_thrs) from the definitions above: float64 [Kn, T].  gts: per
    image an array (n, 4) or None; proposals: per image (k, 4), taken in their order, or (k, 5) with a score, ordered by descending
    score -- equal scores keep their order (the project's tie rule; the reference's is a reversed unstable argsort).  The first
    proposal_nums[-1] are kept.  recalls = hits / float(num_gts) in double: NaN when there is no box at all, as the reference gives."""
    nums = [int(v) for v in np.atleast_1d(np.asarray(proposal_nums)).reshape(-1)]
    rows, boxes = [], []
    for p, g in zip(proposals, gts):
        p = np.asarray(p)
        if p.ndim == 2 and p.shape[1] == 5:
            p = p[np.argsort(-p[:, 4], kind="stable")]
        rows.append(torch.as_tensor(p.reshape(-1, p.shape[1] if p.ndim == 2 else 4)[:max(nums[-1], 0), :4].astype(np.float32)))
        boxes.append(torch.zeros(0, 4) if g is None else torch.as_tensor(np.asarray(g, dtype=np.float32)).reshape(-1, 4))
    B, R, G = len(rows), max(1, max(r.shape[0] for r in rows)), max(1, max(g.shape[0] for g in boxes))
    props = Proposals(torch.zeros(B, R, 4), torch.zeros(B, R), torch.tensor([r.shape[0] for r in rows], dtype=torch.int32))
    targets = PaddedTargets(torch.zeros(B, G, 4), torch.zeros(B, G, dtype=torch.long), torch.tensor([g.shape[0] for g in boxes], dtype=torch.int32))
    for b, (r, g) in enumerate(zip(rows, boxes)):
        props.boxes[b, :r.shape[0]], targets.boxes[b, :g.shape[0]] = r, g
    hits, num_gts = recall_hits(proposal_round_ious(props, targets, nums), iou_thrs)
    with np.errstate(divide="ignore", invalid="ignore"):
        return hits.numpy().astype(np.float64) / np.float64(num_gts)


# ------------------------------------------------------------------------------------------------------------------------
# proposal recall: the kernel (csrc/pswin_recall.hip) and the accumulator
# ------------------------------------------------------------------------------------------------------------------------
def recall_supported(B, R, G, Kn, T):
    """Whether pswin_recall_match takes the shape: the boxes and proposals of an image fit one workgroup's LDS"""
    return 1 <= B <= 65535 and 1 <= R <= RECALL_MAX_R and 1 <= G <= RECALL_MAX_G and 1 <= Kn <= 8 and 1 <= T <= 16


class RecallAccumulator:
    """Proposal recall (AR@N) over a data set, batch by batch: hits int64 [Kn, T] and num_gts int64 [1] on `device`.  proposal_nums: Kn
    numbers >= 1, ascending as the reference expects them; iou_thrs: T thresholds in (0, 1], kept as float64."""

    def __init__(self, proposal_nums=(100, 300, 1000), iou_thrs=DEFAULT_RECALL_THRS, device="cpu"):
        self.proposal_nums = tuple(int(v) for v in np.atleast_1d(np.asarray(proposal_nums)).reshape(-1))
        self.iou_thrs = _thresholds(iou_thrs)
        self.Kn, self.T = len(self.proposal_nums), len(self.iou_thrs)
        if not (1 <= self.Kn <= 8 and 1 <= self.T <= 16):
            raise PswinError("RecallAccumulator: 1 to 8 proposal numbers, 1 to 16 thresholds")
        if any(v < 1 for v in self.proposal_nums) or any(not 0 < t <= 1 for t in self.iou_thrs):
            raise PswinError(f"RecallAccumulator: proposal numbers >= 1 and thresholds in (0, 1], got {self.proposal_nums}, {self.iou_thrs}")
        dev = torch.device(device)
        self.hits = torch.zeros(self.Kn, self.T, dtype=torch.int64, device=dev)
        self.num_gts = torch.zeros(1, dtype=torch.int64, device=dev)
        self._nums = (ctypes.c_int * self.Kn)(*self.proposal_nums)
        self._thrs = (ctypes.c_double * self.T)(*[float(t) for t in self.iou_thrs])

    def reset(self):
        """Forget every batch, in place (stream-ordered; the buffers keep their addresses for a captured update)."""
        self.hits.zero_(), self.num_gts.zero_()
        return self

    def update(self, proposals, targets, ignore=None, out=None):
        """Score one batch: the rounds f32 [Kn, B, Gmax] (proposal_round_ious), their hits and the batch's boxes added to the accumulators.
        proposals: a Proposals; targets: a PaddedTargets, or the list form, padded on entry (PaddedTargets.of); ignore: bool [B, Gmax] or
        None -- flagged boxes are left out before the matching, as fast_eval_recall drops them.  On the GPU inside recall_supported one HIP
        launch with no host synchronisation and no data-dependent shape, which can be captured with heads_propose (out: its buffer for
        the rounds, if the caller keeps one); outside it, and on the CPU, the definitions (on the GPU they read the counts back)."""
        gts = PaddedTargets.of(targets)
        dev = self.hits.device
        if proposals.boxes.dim() != 3 or gts.boxes.shape[0] != proposals.boxes.shape[0]:
            raise PswinError(f"RecallAccumulator.update: proposals {tuple(proposals.boxes.shape)}, targets {tuple(gts.boxes.shape)}")
        for name, t, dt in (("proposals.boxes", proposals.boxes, torch.float32), ("proposals.count", proposals.count, torch.int32),
                            ("targets.boxes", gts.boxes, torch.float32), ("targets.count", gts.count, torch.int32)):
            if t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise PswinError(f"RecallAccumulator.update: {name} must be a contiguous {dt} tensor on {dev}")
        ignore = _flags(ignore, gts)
        (B, R), G = proposals.boxes.shape[:2], gts.boxes.shape[1]
        if not (dev.type == "cuda" and recall_supported(B, R, G, self.Kn, self.T)):
            rounds = proposal_round_ious(proposals, gts, self.proposal_nums, ignore)
            hits, num = _recall_hits(rounds, self.iou_thrs)
            self.hits.add_(hits), self.num_gts.add_(num)
            if out is not None:
                rounds = _out(out, rounds.shape, torch.float32, dev, "RecallAccumulator.update").copy_(rounds)
            return rounds
        rounds = _out(out, (self.Kn, B, G), torch.float32, dev, "RecallAccumulator.update")
        p = _lib.ptr
        _lib.call("pswin_recall_match", rounds, p(proposals.boxes), p(proposals.count), p(gts.boxes), p(gts.count), p(ignore), self._nums,
                  self.Kn, self._thrs, self.T, B, R, G, p(rounds), p(self.hits), p(self.num_gts),
                  algo_bytes=self.Kn * B * (min(R, max(self.proposal_nums)) * 16 + G * 20))
        return rounds

    def summarize(self):
        """Reads back once: dict(recalls f64 [Kn, T] = hits / float(num_gts), NaN without a box; ar f64 [Kn], their mean over the
        thresholds as fast_eval_recall reports it; num_gts int)."""
        both = torch.cat([self.hits.reshape(-1), self.num_gts]).cpu().numpy()
        num_gts = int(both[-1])
        with np.errstate(divide="ignore", invalid="ignore"):
            recalls = both[:-1].reshape(self.Kn, self.T).astype(np.float64) / np.float64(num_gts)
        return dict(recalls=recalls, ar=recalls.mean(axis=1), num_gts=num_gts)


# ------------------------------------------------------------------------------------------------------------------------
# the COCO protocol: definitions (any device)
# ------------------------------------------------------------------------------------------------------------------------
COCO_MAX_K, COCO_MAX_G, COCO_MAX_T, COCO_MAX_A, COCO_MAX_M = 1024, 512, 16, 8, 4      # pswin_coco_supported
COCO_CHUNK = 1024         # records one workgroup of pswin_coco_accumulate takes per trip (pswin_coco_accumulate_chunk(); tests aim at it)
COCO_REC_THRS = np.linspace(0.0, 1.0, int(np.round((1.0 - 0.0) / 0.01)) + 1)
COCO_AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
COCO_EPS = float(np.spacing(1))
FLAG_MATCHED, FLAG_IGNORED = 1, 2


def coco_iou_thrs(iou_thrs=None):
    """float64 [T]: the thresholds as given, or the reference's default np.linspace(.5, .95, 10)"""
    if iou_thrs is None:
        return np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    return _thresholds(iou_thrs)


def _crowd_flags(crowd, gts):
    if crowd is None:
        return torch.zeros(gts.labels.shape, dtype=torch.bool, device=gts.labels.device)
    return crowd.bool()


def coco_pair_iou(dets, gts, crowd=None, iou="bbox", mask_counts=None):
    """(iou f64 [B, K, Gmax], det_area f64 [B, K], gt_area f64 [B, Gmax]) by rule 2 and 3: for the pairs with k < dets.count[b],
    g < gts.count[b] and equal labels inter / union in double, the union being the detection's area alone for a crowd box; -1 for every
    other pair.  Boxes: x, y, w = x2 - x1, h = y2 - y1 of the float32 corners widened to double; masks: integer pixel counts, from the
    bitmaps or, if given, from mask_counts = (inter, areas) as mask_inter_pairs / rle.inter_pairs_definition return them."""
    cr = _crowd_flags(crowd, gts)
    if iou == "segm" and mask_counts is not None:
        K = dets.labels.shape[1]
        inter = mask_counts[0].clamp(min=0).double()
        da, ga = mask_counts[1][:, :K].double(), mask_counts[1][:, K:].double()
    elif iou == "segm":
        d, g = (dets.masks != 0).flatten(2), (gts.masks != 0).flatten(2)
        inter = torch.matmul(d.double(), g.double().transpose(1, 2))              # sums of 0 / 1 in double: exact
        da, ga = d.sum(2).double(), g.sum(2).double()
    else:
        d, g = dets.boxes.double(), gts.boxes.double()
        dx, dy, dw, dh = d[..., 0, None], d[..., 1, None], (d[..., 2] - d[..., 0])[..., None], (d[..., 3] - d[..., 1])[..., None]
        gx, gy, gw, gh = g[:, None, :, 0], g[:, None, :, 1], (g[..., 2] - g[..., 0])[:, None, :], (g[..., 3] - g[..., 1])[:, None, :]
        w = torch.minimum(dx + dw, gx + gw) - torch.maximum(dx, gx)
        h = torch.minimum(dy + dh, gy + gh) - torch.maximum(dy, gy)
        inter = torch.where((w <= 0) | (h <= 0), torch.zeros_like(w), w * h)
        da, ga = (dw * dh)[..., 0], (gw * gh)[:, 0, :]
    union = torch.where(cr[:, None, :], da[:, :, None].expand_as(inter), da[:, :, None] + ga[:, None, :] - inter)
    hit = inter > 0
    v = torch.where(hit, inter / torch.where(hit, union, torch.ones_like(union)), torch.zeros_like(inter))
    return torch.where(_pairs(dets, gts), v, torch.full_like(v, -1.0)), da, ga


def _coco_ranges(area_ranges, device):
    r = torch.tensor([[float(a), float(b)] for a, b in (COCO_AREA_RANGES if area_ranges is None else area_ranges)], dtype=torch.float64,
                     device=device)
    return r[:, 0], r[:, 1]


def _image_order(scores, n):
    """the rows 0 .. n - 1 of an image in (descending score bits, ascending row): sort_records' order inside one image"""
    return torch.sort(0x7FFFFFFF - scores[:n].contiguous().view(torch.int32).long(), stable=True)[1]


def coco_match(iou, dets, gts, crowd, det_area, gt_area, iou_thrs, area_ranges, num_classes):
    """Rules 1, 4 and 5 on a padded batch: (flags uint8 [T, A, B, K] of FLAG_MATCHED | FLAG_IGNORED, rank int32 [B, K]).  iou f64
    [B, K, Gmax] as coco_pair_iou returns it; crowd bool [B, Gmax] or None; det_area f64 [B, K], gt_area f64 [B, Gmax] (the areas the
    ranges are applied to).  Rows past the count or with a label outside [0, num_classes) have flags 0 and rank 0.  The closed form of the
    published loop: a detection takes, among its class's boxes with iou >= min(t, 1 - 1e-10) that are unmatched or crowd, the maximum
    under (not ignored, iou, index).  Reads the counts back (a definition, not for a captured step)."""
    B, K, G = iou.shape
    dev = iou.device
    thr = torch.as_tensor(np.minimum(_thresholds(iou_thrs), 1 - 1e-10), device=dev)
    lo, hi = _coco_ranges(area_ranges, dev)
    T, A = thr.numel(), lo.numel()
    cr_all = _crowd_flags(crowd, gts)
    flags = torch.zeros(T, A, B, K, dtype=torch.uint8, device=dev)
    rank = torch.zeros(B, K, dtype=torch.int32, device=dev)
    for b, (nd, ng) in enumerate(zip(dets.count.tolist(), gts.count.tolist())):
        nd, ng = max(0, min(nd, K)), max(0, min(ng, G))
        if nd == 0:
            continue
        labs = dets.labels[b, :nd].tolist()
        cr, ga = cr_all[b, :ng], gt_area[b, :ng].double()
        ign = (cr[None, :] | (ga[None, :] < lo[:, None]) | (ga[None, :] > hi[:, None]))[None].expand(T, A, ng)
        taken = torch.zeros(T, A, ng, dtype=torch.bool, device=dev)
        index = torch.arange(1, ng + 1, device=dev)
        seen = {}
        for k in _image_order(dets.scores[b], nd).tolist():
            lab = labs[k]
            if not 0 <= lab < num_classes:
                continue
            rank[b, k] = seen.get(lab, 0)
            seen[lab] = seen.get(lab, 0) + 1
            da = det_area[b, k].double()
            outside = ((da < lo) | (da > hi))[None, :].expand(T, A)
            if ng == 0:
                flags[:, :, b, k] = outside.to(torch.uint8) * FLAG_IGNORED
                continue
            v = iou[b, k, :ng]
            cand = (v[None, None, :] >= thr[:, None, None]) & (~taken | cr)
            regular = cand & ~ign
            pool = torch.where(regular.any(-1, keepdim=True), regular, cand)
            best = torch.where(pool, v, torch.full_like(v, -1.0)).max(-1, keepdim=True)[0]
            g1 = ((pool & (v == best)).long() * index).max(-1, keepdim=True)[0]           # the winner's index + 1: the HIGHEST of equals
            matched = g1[..., 0] > 0
            g = (g1 - 1).clamp(min=0)
            ig = torch.where(matched, ign.gather(-1, g)[..., 0], outside)
            flags[:, :, b, k] = matched.to(torch.uint8) * FLAG_MATCHED + ig.to(torch.uint8) * FLAG_IGNORED
            taken.scatter_(-1, g, taken.gather(-1, g) | matched[..., None])
    return flags, rank


def coco_count_gts(gts, crowd, gt_area, area_ranges, num_classes):
    """int32 [A, C]: the boxes of the batch that are not ignored (rule 4), per (range, class)"""
    B, G = gts.labels.shape
    dev = gts.labels.device
    lo, hi = _coco_ranges(area_ranges, dev)
    ok = (torch.arange(G, device=dev)[None, :] < gts.count[:, None]) & (gts.labels >= 0) & (gts.labels < num_classes) & ~_crowd_flags(crowd, gts)
    ga = gt_area.double()
    inr = ok[:, None, :] & ~(ga[:, None, :] < lo[None, :, None]) & ~(ga[:, None, :] > hi[None, :, None])
    onehot = gts.labels.clamp(0, num_classes - 1)[:, :, None] == torch.arange(num_classes, device=dev)[None, None, :]
    return (inr[:, :, :, None] & onehot[:, None, :, :]).sum((0, 2)).to(torch.int32)


def coco_records(dets, num_classes):
    """(score f32 [B, K], label int32 [B, K]) as an accumulator stores them: score 0 past the count, label C past it or outside [0, C)"""
    K = dets.labels.shape[1]
    live = torch.arange(K, device=dets.labels.device)[None, :] < dets.count[:, None]
    label = torch.where(live & (dets.labels >= 0) & (dets.labels < num_classes), dets.labels, num_classes).to(torch.int32)
    return torch.where(live, dets.scores, torch.zeros_like(dets.scores)), label


def coco_accumulate(scores, labels, ranks, flags, num_gts, max_dets, num_classes, rec_thrs=COCO_REC_THRS):
    """Rule 6 in numpy on the host: dict(precision f64 [T, R, C, A, M], recall f64 [T, C, A, M], num_gts int32 [A, C]).  scores f32 [N],
    labels int32 [N] (num_classes: no record), ranks [N], flags uint8 [T, A, N], num_gts int [A, C]."""
    order, bounds = sort_records(scores.reshape(-1), labels.reshape(-1), num_classes)
    order, bounds = order.cpu().numpy(), bounds.cpu().numpy()
    T, A = flags.shape[:2]
    f = flags.reshape(T, A, -1).cpu().numpy()[:, :, order]
    rk = ranks.reshape(-1).cpu().numpy().astype(np.int64)[order]
    npig_all = num_gts.cpu().numpy().astype(np.int32)
    rec_thrs = np.asarray(rec_thrs, dtype=np.float64)
    R, M, C = len(rec_thrs), len(max_dets), num_classes
    precision, recall = -np.ones((T, R, C, A, M)), -np.ones((T, C, A, M))
    for c in range(C):
        seg = slice(int(bounds[c]), int(bounds[c + 1]))
        for m, cap in enumerate(max_dets):
            fm = f[:, :, seg][:, :, rk[seg] < int(cap)]
            ig = (fm & FLAG_IGNORED) != 0
            tps, fps = ((fm & FLAG_MATCHED) != 0) & ~ig, ((fm & FLAG_MATCHED) == 0) & ~ig
            tp_sum, fp_sum = np.cumsum(tps, axis=2).astype(dtype=float), np.cumsum(fps, axis=2).astype(dtype=float)
            for a in range(A):
                npig = int(npig_all[a, c])
                if npig == 0:
                    continue
                for t in range(T):
                    tp, fp = tp_sum[t, a], fp_sum[t, a]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, c, a, m] = rc[-1] if nd else 0
                    if nd:
                        pr = np.maximum.accumulate(pr[::-1])[::-1]
                    inds = np.searchsorted(rc, rec_thrs, side="left")
                    q = np.zeros(R)
                    q[inds < nd] = pr[inds[inds < nd]]
                    precision[t, :, c, a, m] = q
    return dict(precision=precision, recall=recall, num_gts=npig_all)


def _coco_stat(values):
    s = values[values > -1]
    return -1.0 if s.size == 0 else float(np.mean(s))


def coco_summarize(ev, iou_thrs=None, max_dets=(100, 300, 1000), iou="bbox"):
    """Rule 7 on the host: dict(stats f64 [12] in COCOeval's order, the reference's '{iou}_mAP', '_mAP_50', '_mAP_75', '_mAP_s', '_mAP_m',
    '_mAP_l' as float(f'{v:.3f}'), '{iou}_mAP_copypaste', 'AR@{m}' per max_dets, 'AR_s/m/l@{last}', ap_per_class f64 [C]).  A statistic
    whose threshold, range or max_dets entry does not exist is -1."""
    precision, recall = ev["precision"], ev["recall"]
    thrs = coco_iou_thrs(iou_thrs)
    A, M = precision.shape[3], precision.shape[4]

    def ap(a, thr=None):
        if a >= A:
            return -1.0
        p = precision
        if thr is not None:
            p = p[np.where(np.isclose(thrs, thr))[0]]
        return _coco_stat(p[:, :, :, a, -1])

    def ar(a, m):
        return _coco_stat(recall[:, :, a, m]) if a < A and m < M else -1.0

    stats = np.array([ap(0), ap(0, 0.5), ap(0, 0.75), ap(1), ap(2), ap(3), ar(0, 0), ar(0, 1), ar(0, 2), ar(1, M - 1), ar(2, M - 1), ar(3, M - 1)])
    res = dict(stats=stats)
    for i, name in enumerate(("mAP", "mAP_50", "mAP_75", "mAP_s", "mAP_m", "mAP_l")):
        res[f"{iou}_{name}"] = float(f"{stats[i]:.3f}")
    res[f"{iou}_mAP_copypaste"] = f"{stats[0]:.3f} {stats[1]:.3f} {stats[2]:.3f} {stats[3]:.3f} {stats[4]:.3f} {stats[5]:.3f}"
    for m, num in enumerate(max_dets):
        res[f"AR@{int(num)}"] = float(f"{ar(0, m):.3f}")
    for a, name in ((1, "s"), (2, "m"), (3, "l")):
        res[f"AR_{name}@{int(max_dets[-1])}"] = float(f"{ar(a, M - 1):.3f}")
    per_class = np.full(precision.shape[2], np.nan)
    for c in range(precision.shape[2]):
        p = precision[:, :, c, 0, -1]
        p = p[p > -1]
        if p.size:
            per_class[c] = np.mean(p)
    res["ap_per_class"] = per_class
    return res


def coco_eval_lists(det_results, annotations, num_classes=None, iou_thrs=None, max_dets=(100, 300, 1000), classwise=False):
    """The reference's evaluate(metric='bbox') on eval_map_lists' argument forms (padded_from_lists): bboxes_ignore / labels_ignore are
    the crowd regions.  Returns the reference's dict (coco_summarize's, with 'stats'; 'ap_per_class' only when classwise)."""
    dets, gts, crowd, C = padded_from_lists(det_results, annotations, num_classes)
    iou, det_area, gt_area = coco_pair_iou(dets, gts, crowd)
    thrs = coco_iou_thrs(iou_thrs)
    flags, rank = coco_match(iou, dets, gts, crowd, det_area, gt_area, thrs, None, C)
    score, label = coco_records(dets, C)
    ev = coco_accumulate(score, label, rank, flags, coco_count_gts(gts, crowd, gt_area, None, C), max_dets, C)
    res = coco_summarize(ev, thrs, max_dets)
    if not classwise:
        del res["ap_per_class"]
    return res


# ------------------------------------------------------------------------------------------------------------------------
# the COCO protocol: the kernels (csrc/pswin_coco.hip) and the accumulator
# ------------------------------------------------------------------------------------------------------------------------
def coco_supported(B, K, G, T, A, M):
    """Whether pswin_coco_match / pswin_coco_accumulate take the shape (pswin_coco_supported): an image's detections and boxes fit one
    workgroup's LDS, and a lane keeps the matched bits of its G / 64 columns in one register"""
    return 1 <= B <= 65535 and 1 <= K <= COCO_MAX_K and 1 <= G <= COCO_MAX_G and 1 <= T <= COCO_MAX_T and 1 <= A <= COCO_MAX_A and \
        1 <= M <= COCO_MAX_M


def _doubles(values):
    return (ctypes.c_double * len(values))(*[float(v) for v in values])


def coco_accumulate_dispatch(scores, labels, ranks, flags, num_gts, max_dets, num_classes, rec_thrs=COCO_REC_THRS):
    """coco_accumulate.  On the GPU: sort_records and a gather with torch, then one launch, a workgroup per (threshold, range, cap, class)
    (pswin_coco_accumulate), and one read-back; on the CPU the definition."""
    if not flags.is_cuda:
        return coco_accumulate(scores, labels, ranks, flags, num_gts, max_dets, num_classes, rec_thrs)
    T, A = flags.shape[:2]
    R, M, C = len(rec_thrs), len(max_dets), int(num_classes)
    order, bounds = sort_records(scores.reshape(-1), labels.reshape(-1), C)
    N = order.numel()
    if N > MAX_RECORDS or ranks.dtype != torch.int16 or flags.dtype != torch.uint8 or tuple(num_gts.shape) != (A, C):
        raise PswinError(f"coco_accumulate: at most {MAX_RECORDS} records, ranks int16, flags uint8 [T, A, N], num_gts [A, C]")
    flags_sorted = flags.reshape(T * A, N).index_select(1, order).contiguous()
    rank_sorted = ranks.reshape(-1).index_select(0, order).contiguous()
    num_gts = num_gts.to(torch.int32).contiguous()
    dev = flags.device
    precision, recall = torch.empty(T, R, C, A, M, dtype=torch.float64, device=dev), torch.empty(T, C, A, M, dtype=torch.float64, device=dev)
    p = _lib.ptr
    _lib.call("pswin_coco_accumulate", flags_sorted, p(flags_sorted), p(rank_sorted), p(bounds), p(num_gts),
              (ctypes.c_int * M)(*[int(v) for v in max_dets]), M, _doubles(rec_thrs), R, T, A, C, N, p(precision), p(recall),
              algo_bytes=T * A * M * 2 * 3 * N + 8 * T * (R + 1) * C * A * M)
    return dict(precision=precision.cpu().numpy(), recall=recall.cpu().numpy(), num_gts=num_gts.cpu().numpy())


def mask_inter_pairs(dets, gts):
    """(inter int32 [B, K, Gmax], areas int32 [B, K + Gmax]): the pixels that are non-zero in both masks for the pairs of box_iou_pairs,
    -1 for every other pair; the pixel counts of image b's detections (first K) and boxes (last Gmax), 0 past a count"""
    d, g = (dets.masks != 0).flatten(2), (gts.masks != 0).flatten(2)
    inter = torch.matmul(d.double(), g.double().transpose(1, 2)).to(torch.int32)
    inter = torch.where(_pairs(dets, gts), inter, torch.full_like(inter, -1))

    def one(m, count):
        inside = torch.arange(m.shape[1], device=m.device)[None, :] < count[:, None]
        return torch.where(inside, m.sum(2), torch.zeros_like(m.sum(2))).to(torch.int32)
    return inter, torch.cat([one(d, dets.count), one(g, gts.count)], 1)


def mask_inter_pairs_dispatch(dets, gts, out=None):
    """mask_inter_pairs.  On the GPU pswin_mask_inter_pairs (mask_iou_pairs' two kernels, storing the integers; any bitmap size), into
    the two buffers of `out` if given; on the CPU the definition."""
    _check_batch(dets, gts)
    _check_masks(dets, gts)
    if not dets.labels.is_cuda:
        return mask_inter_pairs(dets, gts)
    (B, K), G, dev = dets.labels.shape, gts.labels.shape[1], dets.labels.device
    bufs = out or (None, None)
    inter = _out(bufs[0], (B, K, G), torch.int32, dev, "mask_inter_pairs_dispatch")
    areas = _out(bufs[1], (B, K + G), torch.int32, dev, "mask_inter_pairs_dispatch")
    dm, gm = dets.masks.contiguous(), gts.masks.contiguous()
    H, W = dm.shape[2:]
    p = _lib.ptr
    _lib.call("pswin_mask_inter_pairs", inter, p(dm), p(dets.labels), p(dets.count), p(gm), p(gts.labels), p(gts.count), B, K, G, H, W, p(inter),
              p(areas), algo_bytes=(B * (K + G) + 2 * B * K * G) * H * W)
    return inter, areas


def rle_inter_pairs_dispatch(dets, gts, out=None, workspace=None):
    """(inter int32 [B, K, Gmax], areas int32 [B, K + Gmax], overflow int32 [1]): mask_inter_pairs from the masks' runs, for a batch that
    _mask_route sends the run-length way (dets.rle / targets.rle; a side that has only bitmaps is encoded on the spot).  On the GPU
    pswin_rle_inter_pairs (two launches, no host synchronisation: capturable), into the three buffers of `out` if given -- a given
    overflow flag is set, never cleared -- and with `workspace` (rle_inter_workspace) if the caller keeps one; on the CPU
    rle.inter_pairs_definition, which also says what a pool that was too small does to the results."""
    from . import rle
    _check_batch(dets, gts)
    if _mask_route(dets, gts) != "rle":
        raise PswinError("rle_inter_pairs_dispatch: both sides have bitmaps; that batch goes to mask_inter_pairs_dispatch")
    d, g = _rle_sides(dets, gts)
    bufs = out or (None, None, None)
    if not dets.labels.is_cuda:
        inter, areas, over = rle.inter_pairs_definition(d, dets.labels, dets.count, g, gts.labels, gts.count)
        if bufs[2] is not None:
            flag = bufs[2]
            flag |= over                                   # in place: the caller's flag is set, never cleared
            over = flag
        return inter, areas, over
    (B, K), G, dev = dets.labels.shape, gts.labels.shape[1], dets.labels.device
    args = _rle_pairs_args(dets, gts, d, g, "rle_inter_pairs_dispatch")
    inter = _out(bufs[0], (B, K, G), torch.int32, dev, "rle_inter_pairs_dispatch")
    areas = _out(bufs[1], (B, K + G), torch.int32, dev, "rle_inter_pairs_dispatch")
    over = torch.zeros(1, dtype=torch.int32, device=dev) if bufs[2] is None else _out(bufs[2], (1,), torch.int32, dev, "rle_inter_pairs_dispatch")
    ws = rle_inter_workspace(B, K, G, d.capacity, g.capacity, dev) if workspace is None else workspace
    p = _lib.ptr
    _lib.call("pswin_rle_inter_pairs", inter, *args, p(inter), p(areas), p(over), p(ws), algo_bytes=12 * (d.capacity + g.capacity))
    return inter, areas, over


class CocoAccumulator:
    """bbox / segm mAP and AR by the COCO protocol over a data set, batch by batch, in buffers of a fixed shape on `device` (the rules:
    the module docstring).  iou_thrs: None (the reference's ten) or T thresholds in (0, 1]; max_dets: 1 to 4 ascending caps per (image,
    class); area_ranges: None (all, small, medium, large) or A closed (lo, hi) pairs, the first being "all"; capacity_images: the image
    slots; max_per_img: K, the rows of a Detections.

    A record is a detection row's score f32, label int32, rank int16 and its T x A flags; image `cursor + b` of all updates owns rows
    [slot K, slot K + K) of rec_score / rec_label / rec_rank [capacity, K] and rec_flags [T, A, capacity, K].  An unused row has label C."""

    def __init__(self, num_classes, iou="bbox", iou_thrs=None, max_dets=(100, 300, 1000), area_ranges=None, capacity_images=5000,
                 max_per_img=100, device="cuda"):
        self.C, self.K, self.capacity, self.iou = int(num_classes), int(max_per_img), int(capacity_images), iou
        self.iou_thrs = coco_iou_thrs(iou_thrs)
        self.max_dets = tuple(int(v) for v in np.atleast_1d(np.asarray(max_dets)).reshape(-1))
        self.area_ranges = tuple((float(a), float(b)) for a, b in (COCO_AREA_RANGES if area_ranges is None else area_ranges))
        self.T, self.A, self.M = len(self.iou_thrs), len(self.area_ranges), len(self.max_dets)
        if iou not in ("bbox", "segm"):
            raise PswinError(f"CocoAccumulator: iou must be 'bbox' or 'segm', got {iou!r}")
        if not (1 <= self.C <= 65535 and 1 <= self.K <= COCO_MAX_K and self.capacity >= 1 and 1 <= self.T <= COCO_MAX_T and
                1 <= self.A <= COCO_MAX_A and 1 <= self.M <= COCO_MAX_M):
            raise PswinError(f"CocoAccumulator: 1 to 65535 classes, max_per_img in [1, {COCO_MAX_K}], capacity_images >= 1, 1 to {COCO_MAX_T} "
                             f"thresholds, 1 to {COCO_MAX_A} ranges, 1 to {COCO_MAX_M} max_dets")
        if any(not 0 < t <= 1 for t in self.iou_thrs) or any(not a <= b for a, b in self.area_ranges):
            raise PswinError(f"CocoAccumulator: thresholds in (0, 1] and ranges lo <= hi, got {self.iou_thrs}, {self.area_ranges}")
        if any(v < 1 for v in self.max_dets) or list(self.max_dets) != sorted(self.max_dets):
            raise PswinError(f"CocoAccumulator: max_dets must be ascending numbers >= 1, got {self.max_dets}")
        if self.capacity * self.K > MAX_RECORDS:
            raise PswinError(f"CocoAccumulator: capacity_images x max_per_img must not exceed {MAX_RECORDS} records")
        dev = torch.device(device)
        self.rec_score = torch.zeros(self.capacity, self.K, device=dev)
        self.rec_label = torch.full((self.capacity, self.K), self.C, dtype=torch.int32, device=dev)
        self.rec_rank = torch.zeros(self.capacity, self.K, dtype=torch.int16, device=dev)
        self.rec_flags = torch.zeros(self.T, self.A, self.capacity, self.K, dtype=torch.uint8, device=dev)
        self.num_gts = torch.zeros(self.A, self.C, dtype=torch.int32, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        self.rle_overflow = torch.zeros(1, dtype=torch.int32, device=dev)          # set by the run-length route of "segm" (_mask_route)
        self._thrs = _doubles(self.iou_thrs)
        self._ranges = _doubles([v for r in self.area_ranges for v in r])

    def reset(self):
        """Forget every record, in place (stream-ordered; the buffers keep their addresses for a captured update)."""
        self.rec_score.zero_(), self.rec_rank.zero_(), self.rec_flags.zero_(), self.num_gts.zero_(), self.cursor.zero_(), self.overflow.zero_()
        self.rle_overflow.zero_()
        self.rec_label.fill_(self.C)
        return self

    def update(self, dets, targets, crowd=None, gt_area=None, out=None):
        """Score one batch: flags uint8 [T, A, B, K] (FLAG_MATCHED | FLAG_IGNORED), and the batch's records appended at the cursor, which
        advances by B.  dets: a Detections with K = max_per_img rows; targets: a PaddedTargets, or the list form, padded on entry; crowd:
        bool [B, Gmax] or None; gt_area: f32 / f64 [B, Gmax] or None (the annotations' area; None: the box's or the mask's own).  On the
        GPU ONE launch for boxes (pswin_coco_match), three for masks (pswin_mask_inter_pairs' two in front, or by _mask_route's rule
        pswin_rle_inter_pairs' two on the masks' runs, which sets rle_overflow when a run pool was too small), no host synchronisation and
        no data-dependent shape: it can be captured with the prediction.  A shape outside coco_supported raises before any launch.
        Image slots at or past the capacity are not written; accumulate() raises then.  out: a buffer for the flags, if the caller keeps one.
        Polygon ground truth: targets.rle = polygons.polygons_to_rle(PolygonBatch) is an RleMasks like any other."""
        gts = PaddedTargets.of(targets)
        B, K = dets.labels.shape
        dev = self.cursor.device
        if K != self.K or dets.labels.device != dev:
            raise PswinError(f"CocoAccumulator.update: detections [{B}, {K}] on {dets.labels.device}, the accumulator holds max_per_img = "
                             f"{self.K} on {dev}")
        _check_batch(dets, gts)
        route = _mask_route(dets, gts) if self.iou == "segm" else None
        crowd = _flags(crowd, gts)
        G = gts.labels.shape[1]
        if gt_area is not None:
            if gt_area.shape != gts.labels.shape or gt_area.dtype not in (torch.float32, torch.float64) or gt_area.device != dev:
                raise PswinError(f"CocoAccumulator.update: gt_area must be f32 or f64 {tuple(gts.labels.shape)} on {dev}")
            gt_area = gt_area.double().contiguous()
        if not dev.type == "cuda":
            counts = None
            if route == "rle":
                counts = rle_inter_pairs_dispatch(dets, gts, out=(None, None, self.rle_overflow))[:2]
            iou, det_area, own_area = coco_pair_iou(dets, gts, crowd, self.iou, counts)
            area = own_area if gt_area is None else gt_area
            flags, rank = coco_match(iou, dets, gts, crowd, det_area, area, self.iou_thrs, self.area_ranges, self.C)
            if out is not None:
                flags = _out(out, flags.shape, torch.uint8, dev, "CocoAccumulator.update").copy_(flags)
            score, label = coco_records(dets, self.C)
            live = gts.count.clamp(0, G)
            for b in range(B):
                slot = int(self.cursor) + b
                if slot >= self.capacity:
                    self.overflow.fill_(1)
                    continue
                self.rec_score[slot], self.rec_label[slot], self.rec_rank[slot] = score[b], label[b], rank[b].to(torch.int16)
                self.rec_flags[:, :, slot] = flags[:, :, b]
                one = PaddedTargets(gts.boxes[b:b + 1], gts.labels[b:b + 1], live[b:b + 1])
                self.num_gts += coco_count_gts(one, None if crowd is None else crowd[b:b + 1], area[b:b + 1], self.area_ranges, self.C)
        else:
            if not coco_supported(B, K, G, self.T, self.A, self.M):
                raise PswinError(f"CocoAccumulator.update: B = {B}, K = {K}, Gmax = {G}, T = {self.T}, A = {self.A}, M = {self.M} is outside "
                                 f"coco_supported (K <= {COCO_MAX_K}, Gmax <= {COCO_MAX_G})")
            flags = _out(out, (self.T, self.A, B, K), torch.uint8, dev, "CocoAccumulator.update")
            p = _lib.ptr
            inter = areas = None
            if route == "rle":
                inter, areas = rle_inter_pairs_dispatch(dets, gts, out=(None, None, self.rle_overflow))[:2]
            elif route == "bitmap":
                inter, areas = mask_inter_pairs_dispatch(dets, gts)
            _lib.call("pswin_coco_match", flags, p(dets.boxes), p(dets.scores), p(dets.labels), p(dets.count), p(gts.boxes), p(gts.labels),
                      p(gts.count), p(crowd), p(gt_area), p(inter), p(areas), self._thrs, self.T, self._ranges, self.A, B, K, G, self.C,
                      self.capacity, p(self.cursor), p(flags), p(self.rec_score), p(self.rec_label), p(self.rec_rank), p(self.rec_flags),
                      p(self.num_gts), p(self.overflow), algo_bytes=B * (K + G) * 32 + 2 * self.T * self.A * B * K)
        self.cursor.add_(B)
        return flags

    def accumulate(self):
        """Reads back: dict(precision f64 [T, 101, C, A, M], recall f64 [T, C, A, M], num_gts int32 [A, C]) as numpy arrays; -1 where a
        (class, range) has no counted box."""
        if int(self.overflow):
            raise PswinError(f"CocoAccumulator: more than capacity_images = {self.capacity} images were given; the records past it are lost")
        if int(self.rle_overflow):
            raise PswinError(_RLE_OVERFLOW.format("CocoAccumulator"))
        return coco_accumulate_dispatch(self.rec_score, self.rec_label, self.rec_rank, self.rec_flags, self.num_gts, self.max_dets, self.C)

    def summarize(self, ev=None):
        """coco_summarize of accumulate() (or of `ev`, its earlier result)"""
        return coco_summarize(self.accumulate() if ev is None else ev, self.iou_thrs, self.max_dets, self.iou)
