"""Inputs for the sampler / box-target / mask-target tests (tests/test_targets.py on the CPU, tests/test_targets_gpu.py on the MI355X),
and the padded branch of MiniMaskRCNN as it stood before detector.sample_ranks / rpn_targets / roi_targets / mask_targets existed,
restated image by image (this repository's own lines; the one change: every argsort is left as it was, so the comparison is made on
inputs whose composed keys are pairwise distinct)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _assign_cases as ac

SENTINEL = [1.25, 2.25, 250.25, 120.25]      # in the padding rows: a box that overlaps half the image, so that reading one would show
SENTINEL_LABEL = 77


# ---- the sampler's inputs --------------------------------------------------------------------------------------------------------------
POPULATIONS = ("all_positive", "no_positive", "all_ignored", "few_positive", "mix")
KEY_KINDS = ("distinct", "eighths", "tiny")


def population(kind, B, N, gen):
    """gt_inds long [B, N]"""
    if kind == "all_positive":
        return torch.randint(1, 10, (B, N), generator=gen)
    if kind == "no_positive":
        return -torch.randint(0, 2, (B, N), generator=gen)                       # negatives and ignored
    if kind == "all_ignored":
        return torch.full((B, N), -1, dtype=torch.long)
    if kind == "few_positive":                                                  # fewer positives than any n_pos > 1 (one where N allows it)
        g = -torch.randint(0, 2, (B, N), generator=gen)
        if N > 2:
            g[:, N // 2] = 3
        return g
    return torch.randint(-1, 4, (B, N), generator=gen)                          # a mix: -1, 0 and three gts


def keys(kind, B, N, gen):
    """key f32 [B, N], finite and >= 0.  distinct: multiples of 2^-20 below 1, all different -- exact under + 2 and + 4, so the composed
    keys of a list are pairwise distinct too.  eighths: multiples of 1/8 (many exact ties).  tiny: j * 2^-24, all different, whose
    composed keys fl(key + 2) / fl(key + 4) tie four / eight at a time."""
    if kind == "distinct":
        return torch.stack([torch.randperm(1 << 20, generator=gen)[:N] for _ in range(B)]).float() / (1 << 20)
    if kind == "eighths":
        return torch.randint(0, 8, (B, N), generator=gen).float() / 8
    return torch.stack([torch.randperm(N, generator=gen) for _ in range(B)]).float() * 2.0 ** -24


def composed(gt_inds, key):
    """the two composed keys of detector.sample_ranks, f32 [B, N] each"""
    behind = torch.where(gt_inds < 0, key + 4, key + 2)
    return torch.where(gt_inds > 0, key, behind), torch.where(gt_inds == 0, key, behind)


def composed_keys_distinct(gt_inds, key):
    return all(int(torch.unique(row).numel()) == row.numel() for c in composed(gt_inds, key) for row in c)


# ---- the two stages' inputs ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_case(Gmax, n_extra, lead, seed):
    """A padded batch with counts (Gmax, 0, 1): (gt_inds long [3, N], key f32 [3, N] distinct, cand f32 [3, N, 4], gt f32 [3, Gmax, 4],
    gt_labels long [3, Gmax], count int32 [3]) as CPU tensors, assigned by the CPU definition.  lead: the candidates are cat(padded gt
    rows, n_extra boxes) and the assigner runs with lead_gt = Gmax (the RoI stage); otherwise n_extra boxes shared by the images (the
    RPN: cand[0] is the anchor list).  Padding rows hold SENTINEL / SENTINEL_LABEL."""
    from panoswintransformerobjectdetection_amd import detector as det
    counts = (Gmax, 0, 1)
    gts = [ac.gt_boxes(g, seed + 7 * b) for b, g in enumerate(counts)]
    gt, count = ac.padded_gt(gts, Gmax)
    labels = np.full((3, Gmax), SENTINEL_LABEL, np.int64)
    rng = np.random.RandomState(seed)
    for b, g in enumerate(counts):
        gt[b, g:] = SENTINEL
        labels[b, :g] = rng.randint(0, 60, g)
    if lead:
        cand = np.stack([np.concatenate([gt[b], ac.candidates(n_extra, gts[b], seed + 100 + b)]) for b in range(3)])
    else:
        cand = np.broadcast_to(ac.candidates(n_extra, gts[0], seed + 100), (3, n_extra, 4)).copy()
    cand, gt, count, labels = torch.from_numpy(cand), torch.from_numpy(gt), torch.from_numpy(count), torch.from_numpy(labels)
    thr = (0.5, 0.5, 0.5, True) if lead else (0.7, 0.3, 0.3, True)
    gt_inds = det.max_iou_assign_batch(cand if lead else cand[0], gt, count, *thr, lead_gt=Gmax if lead else 0)[0]
    key = keys("distinct", 3, cand.shape[1], torch.Generator().manual_seed(seed + 5))
    return gt_inds, key, cand, gt, labels, count


# ---- the parent's padded branch, image by image ------------------------------------------------------------------------------------------
def parent_rpn_image(gt_inds, key, flat_a, gt, n_pos_max, n_tot):
    """_rpn_losses_and_proposals, padded branch: (pos_rank, neg_rank, idx, valid, pos_valid, d_t) of one image"""
    from panoswintransformerobjectdetection_amd.detector import encode_deltas
    label = gt_inds.clamp(max=1).to(flat_a.dtype)
    arg = (gt_inds - 1).clamp(min=0)
    behind = torch.where(label < 0, key + 4, key + 2)
    pos_rank = torch.argsort(torch.where(label == 1, key, behind))[:n_pos_max]
    pos_valid = label[pos_rank] == 1
    neg_rank = torch.argsort(torch.where(label == 0, key, behind))[:n_tot]
    n_pos = pos_valid.sum()
    neg_valid = (label[neg_rank] == 0) & (torch.arange(n_tot, device=key.device) < (n_tot - n_pos))
    idx = torch.cat([pos_rank, neg_rank])
    valid = torch.cat([pos_valid, neg_valid]).float()
    d_t = encode_deltas(flat_a[pos_rank], gt[arg[pos_rank]], (1.0, 1.0, 1.0, 1.0))
    return pos_rank, neg_rank, idx, valid, pos_valid, d_t


def parent_roi_image(gt_inds, key, cand, gt, gl, num_classes, n_pos_max, n_tot):
    """_roi_losses, padded branch: (rois, labels, reg_t, pos_valid, gt_idx) of one image"""
    from panoswintransformerobjectdetection_amd.detector import encode_deltas
    is_pos, arg = gt_inds > 0, (gt_inds - 1).clamp(min=0)
    is_neg = gt_inds == 0
    behind = torch.where(gt_inds < 0, key + 4, key + 2)
    pos_rank = torch.argsort(torch.where(is_pos, key, behind))[:n_pos_max]
    pos_valid = is_pos[pos_rank]
    filler = n_pos_max - pos_valid.sum()
    neg_order = torch.argsort(torch.where(is_neg, key, behind))
    take = (torch.arange(n_tot - n_pos_max, device=key.device) + filler).clamp(max=neg_order.numel() - 1)
    neg_rank = neg_order[take]
    idx = torch.cat([pos_rank, neg_rank])
    lab = torch.where(torch.cat([pos_valid, torch.zeros_like(neg_rank, dtype=torch.bool)]), gl[arg[idx]], torch.full_like(idx, num_classes))
    return cand[idx], lab, encode_deltas(cand[pos_rank], gt[arg[pos_rank]], (0.1, 0.1, 0.2, 0.2)), pos_valid, arg[pos_rank]


def parent_mask_image(masks_b, rois_bp, gt_idx_b, img_hw, ms):
    """_roi_losses, mask targets of one image: ALL gt bitmaps as channels through grid_sample, then the assigned channel picked"""
    n_pos_max = rois_bp.shape[0]
    t = (torch.arange(ms, device=rois_bp.device, dtype=torch.float32) + 0.5) / ms
    H, W = img_hw
    r = rois_bp
    gx = (r[:, 0:1] + (r[:, 2:3] - r[:, 0:1]) * t[None]) / W * 2 - 1
    gy = (r[:, 1:2] + (r[:, 3:4] - r[:, 1:2]) * t[None]) / H * 2 - 1
    grid = torch.stack([gx[:, None, :].expand(-1, ms, ms), gy[:, :, None].expand(-1, ms, ms)], -1).reshape(1, -1, ms, 2)
    gm = masks_b.float()[None]
    smp = F.grid_sample(gm, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    smp = smp[0].view(gm.shape[1], n_pos_max, ms, ms)
    return (smp[gt_idx_b, torch.arange(n_pos_max, device=smp.device)] >= 0.5).float()


# ---- the mask targets' inputs ------------------------------------------------------------------------------------------------------------
MASK_GMAX, MASK_P, MASK_COUNTS = 16, 128, (9, 1)
NEAR = 1e-4              # a point whose float64 value lies within NEAR of 0.5 may fall either way in float32
NEAR_SHARE = 1e-3        # at most this share of the points may be such points


@functools.lru_cache(maxsize=None)
def mask_case(H, W, seed=0):
    """(masks uint8 [2, 16, H, W], rois f32 [2, 128, 4], gt_idx long [2, 128], pos_valid bool [2, 128], count) as CPU tensors: the
    synthetic_targets bitmaps of an image with 9 boxes and of one cut to 1 box, the planes past the count filled with ONES.  RoIs per
    image: its gt boxes, those jittered by +-15 % of their size, boxes partly outside the image on every side, zero width, zero height,
    one pixel, the whole image, then more jittered ones; every 7th row (and the rows with a wild gt_idx) has pos_valid false."""
    from panoswintransformerobjectdetection_amd.detector import synthetic_targets
    tg = next(t for t in (synthetic_targets(2, H, W, "cpu", seed=s) for s in range(seed, seed + 400)) if t[0]["boxes"].shape[0] == 9)
    masks = torch.ones(2, MASK_GMAX, H, W, dtype=torch.uint8)
    boxes = []
    for b, n in enumerate(MASK_COUNTS):
        masks[b, :n] = tg[b]["masks"][:n]
        boxes.append(tg[b]["boxes"][:n])
    g = torch.Generator().manual_seed(seed + 11)
    rois = torch.zeros(2, MASK_P, 4)
    gt_idx = torch.zeros(2, MASK_P, dtype=torch.long)
    pos_valid = torch.ones(2, MASK_P, dtype=torch.bool)
    special = torch.tensor([[-0.3 * W, 0.2 * H, 0.4 * W, 0.7 * H], [0.6 * W, 0.1 * H, 1.3 * W, 0.8 * H], [0.2 * W, -0.4 * H, 0.7 * W, 0.5 * H],
                            [0.3 * W, 0.55 * H, 0.8 * W, 1.35 * H], [-0.2 * W, -0.2 * H, 1.2 * W, 1.2 * H],
                            [0.37 * W + 0.3, 0.1 * H, 0.37 * W + 0.3, 0.9 * H],            # zero width
                            [0.1 * W, 0.41 * H + 0.3, 0.9 * W, 0.41 * H + 0.3],            # zero height
                            [0.5 * W + 0.2, 0.5 * H + 0.2, 0.5 * W + 1.2, 0.5 * H + 1.2],  # one pixel
                            [0.0, 0.0, float(W), float(H)]])                               # the whole image
    for b, n in enumerate(MASK_COUNTS):
        bx = boxes[b]
        for p in range(MASK_P):
            i = p % n
            wh = torch.cat([bx[i, 2:] - bx[i, :2]] * 2)
            if p < n:
                rois[b, p] = bx[i]
            elif 2 * n <= p < 2 * n + special.shape[0]:
                rois[b, p] = special[p - 2 * n]
            else:
                rois[b, p] = bx[i] + (torch.rand(4, generator=g) * 0.3 - 0.15) * wh
            gt_idx[b, p] = i
        pos_valid[b, 5::7] = False
        gt_idx[b, 5], gt_idx[b, 12] = 300, -5                       # invalid rows may hold anything
    return masks, rois, gt_idx, pos_valid, torch.tensor(MASK_COUNTS, dtype=torch.int32)


def near_threshold(masks, rois, gt_idx, pos_valid, size=28):
    """bool [B P, size, size]: the points whose float64 value lies within NEAR of 0.5; and the float64 targets"""
    from panoswintransformerobjectdetection_amd import detector as det
    val = det.mask_targets(masks, rois, gt_idx, pos_valid, size, dtype=torch.float64, return_float=True)
    return (val - 0.5).abs() <= NEAR, (val >= 0.5).float()
