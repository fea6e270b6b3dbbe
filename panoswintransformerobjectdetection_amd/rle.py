"""COCO run-length encoding (RLE) of instance masks: the definitions (numpy / torch on the CPU), the fixed-shape container of a batch's runs
and the entry points that dispatch to the HIP kernels (ops.rle_encode, ops.paste_masks_rle -> csrc/pswin_rle.hip).

The reference's test loop turns every image's masks into RLE (`encode_mask_results`, mmdet/core/mask/utils.py:36-63, called from
mmdet/apis/test.py:60 and :100) before results are gathered or written (`_segm2json`, mmdet/datasets/coco.py:235-300).  It does so through
pycocotools' maskApi.c.

PARITY: unpinned.  pycocotools is neither on the development machine nor in the reference tree, so nothing here is compared against it.
The rules below are stated completely and restated independently as plain loops in tests/_rle_cases.py.

  rle_encode (rleEncode).  The mask [H, W] is scanned in COLUMN-MAJOR order, linear position x * H + y.  counts[0] is the length of the
    leading run of zeros -- 0 when the first pixel is set -- then the runs alternate; they sum to H * W.  Equivalently: with
    p_0 < p_1 < ... the positions whose pixel differs from its predecessor (the predecessor of position 0 being 0),
    counts = diff([0, p_0, ..., p_last, H * W]).  A non-zero byte is foreground (this project's choice: pycocotools compares raw byte
    values; the masks here are 0 / 1).  Positions and counts are uint32, so H * W < 2^32, as in pycocotools.
  rle_to_string / rle_from_string (rleToString / rleFrString).  Run i is written as x = counts[i] - (counts[i - 2] if i > 2 else 0), a
    signed value, five bits at a time, low bits first: c = x & 0x1f; x >>= 5 (arithmetic); more = (x != -1) if (c & 0x10) else (x != 0);
    if more: c |= 0x20; the character is c + 48.  At most 7 characters per run.  Reading undoes it: the last group's bit 0x10 extends the sign.
  rle_decode, rle_area: the bitmap back, and the sum of the odd-indexed counts.
  rle_inter (the integer part of rleIou).  For one mask with counts c[0 .. n): p[i] = c[0] + ... + c[i], f[i] = the sum of the odd-indexed
    c[j], j <= i, and p[-1] = f[-1] = 0.  For a position x in [0, H W], i(x) is the number of i with p[i] <= x (an upper bound), and
    F(x) = f[i - 1] + (x - p[i - 1] if i is odd and i < n else 0) is the number of foreground positions below x.  Then
    rle_area(c) = f[n - 1] and rle_inter(cd, cg) = the sum over the odd i of cd of F_g(p_d[i]) - F_g(p_d[i - 1]).  Integers only, so the
    order of the sum does not matter; zero-length runs (a leading c[0] = 0, or runs of 0 inside foreign RLE such as [0, 3, 0, 2, 4, 0, 1])
    need no special case.  The IoU is float32(double(inter) / double(area_d + area_g - inter)), 0 when the union is 0, as for bitmaps
    (evaluation.mask_iou_pairs).  tests/_rle_iou_cases.py restates it as the two-pointer loop of rleIou.
  inter_pairs_definition: rle_inter and rle_area over the same-class pairs of a padded batch, in the layout of
    evaluation.mask_inter_pairs.  HIP tensors: csrc/pswin_rle_iou.hip through evaluation.rle_inter_pairs_dispatch.

RleMasks holds the runs of N masks in buffers of a fixed shape (the RLE counterpart of Detections / PaddedTargets), so that a captured
inference step can produce them and a captured scoring step can read them; the strings are made on the host when results are read back
(to_lists) and parsed on the host (from_lists): producing them on the device is out of scope, and so is a fused form for test-time
augmentation.  Polygon annotations (frPyObjects) become RleMasks through polygons.polygons_to_rle.
"""
import numpy as np
import torch

from ._lib import PswinError


# ------------------------------------------------------------------------------------------------------------------------
# the format
# ------------------------------------------------------------------------------------------------------------------------
def rle_encode(mask):
    """mask [H, W] (any dtype; non-zero = foreground) -> counts, a uint32 array"""
    m = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask) != 0
    if m.ndim != 2:
        raise PswinError(f"rle_encode takes one [H, W] mask, got shape {m.shape}")
    flat = m.T.reshape(-1)                                                     # position x * H + y
    prev = np.concatenate([[False], flat[:-1]])
    p = np.flatnonzero(flat != prev)
    return np.diff(np.concatenate([[0], p, [flat.size]])).astype(np.uint32)


def rle_to_string(counts):
    """counts -> the bytes pycocotools stores under "counts" """
    cnt = np.asarray(counts, dtype=np.int64)
    x = cnt.copy()
    x[3:] -= cnt[1:-2]
    n = x.size
    chars = np.zeros((n, 7), dtype=np.uint8)
    active = np.zeros((n, 7), dtype=bool)
    live = np.ones(n, dtype=bool)
    for r in range(7):                                                         # 32 + 1 sign bits in groups of five
        c = x & 0x1f
        x = x >> 5                                                             # arithmetic on int64
        more = np.where((c & 0x10) != 0, x != -1, x != 0)
        chars[:, r] = (c | (more.astype(np.int64) << 5)) + 48
        active[:, r] = live
        live = live & more
    return chars[active].tobytes()


def rle_from_string(s):
    """the inverse of rle_to_string: a uint32 array"""
    c = np.frombuffer(bytes(s), dtype=np.uint8).astype(np.int64) - 48
    if c.size == 0:
        return np.zeros(0, dtype=np.uint32)
    ends = (c & 0x20) == 0
    if not ends[-1]:
        raise PswinError("rle_from_string: the string ends inside a run")
    starts = np.concatenate([[0], np.flatnonzero(ends)[:-1] + 1])
    group = np.cumsum(ends) - ends
    k = np.arange(c.size) - starts[group]                                      # the character's place in its run
    x = np.add.reduceat((c & 0x1f) << (5 * k), starts)
    last = np.flatnonzero(ends)
    neg = (c[last] & 0x10) != 0
    x = np.where(neg, x | (np.int64(-1) << (5 * (k[last] + 1))), x)
    out = x.copy()                                                             # counts[i] = x[i] + counts[i - 2] for i > 2: two running sums
    out[1::2] = np.cumsum(x[1::2])
    out[2::2] = np.cumsum(x[2::2])
    return (out & 0xffffffff).astype(np.uint32)


def rle_decode(counts, height, width):
    """counts -> uint8 [H, W] of 0 / 1"""
    cnt = np.asarray(counts, dtype=np.int64)
    if int(cnt.sum()) != height * width:
        raise PswinError(f"rle_decode: the runs sum to {int(cnt.sum())}, not to {height} x {width}")
    flat = np.repeat((np.arange(cnt.size) & 1).astype(np.uint8), cnt)
    return np.ascontiguousarray(flat.reshape(width, height).T)


def rle_area(counts):
    return int(np.asarray(counts, dtype=np.int64)[1::2].sum())


def _fg_below(p, f, x):
    """F(x) of the module docstring for the tables (p, f) of one mask, at every position of the array x"""
    n = p.size
    i = np.searchsorted(p, x, side="right")                                    # the number of p[i] <= x
    pp, ff = np.concatenate([[0], p]), np.concatenate([[0], f])                # shifted by one: pp[i] = p[i - 1]
    return ff[i] + np.where(((i & 1) == 1) & (i < n), x - pp[i], 0)


def rle_inter(cd, cg):
    """The number of positions that are foreground in both masks, from their counts alone (the module docstring states the rule)"""
    cd, cg = np.asarray(cd, dtype=np.int64).reshape(-1), np.asarray(cg, dtype=np.int64).reshape(-1)
    pd, pg = np.cumsum(cd), np.cumsum(cg)
    fg = np.cumsum(np.where(np.arange(cg.size) & 1, cg, 0))
    ends = pd[1::2]
    starts = pd[0::2][:ends.size]                                              # p_d[i - 1] for the odd i
    return int((_fg_below(pg, fg, ends) - _fg_below(pg, fg, starts)).sum())


# ------------------------------------------------------------------------------------------------------------------------
# the runs of a batch
# ------------------------------------------------------------------------------------------------------------------------
def default_capacity(n_masks, width):
    """n (30 W + 1): in exact arithmetic a pasted mask crosses the threshold at most 29 times per column (the bilinear sample is linear in
    y on each of the 29 cell intervals), the join with the previous column makes 30 boundaries, and each mask has one final run.  float32
    rounding could add a crossing, and bitmaps from elsewhere obey no bound: overflow is reported (RleMasks), never silent."""
    return max(1, int(n_masks) * (30 * int(width) + 1))


class RleMasks:
    """The runs of N masks of one size in fixed-shape buffers: offsets int64 [N + 1] -- mask n owns runs[offsets[n] : offsets[n + 1]] and
    offsets[N] is what the batch needs -- and runs uint32 [>= capacity].  Masks are in index order and runs in scan order: the contents are
    a function of the inputs alone.  For detections B, K and count (int32 [B]) say which rows are detections (n = b K + k, k < count[b]);
    the rows behind them own no runs, so offsets stays flat across them.
    Overflow: offsets is always whole and exact; nothing is written at an index >= capacity; a mask whose range lies below capacity is
    written whole.  to_lists() raises when offsets[N] > capacity."""

    def __init__(self, offsets, runs, height, width, capacity=None, B=None, K=None, count=None):
        self.offsets, self.runs, self.height, self.width = offsets, runs, int(height), int(width)
        self.capacity = int(runs.numel() if capacity is None else capacity)
        self.B, self.K, self.count = B, K, count

    @classmethod
    def allocate(cls, n_masks, height, width, device, capacity=None, B=None, K=None, count=None):
        cap = default_capacity(n_masks, width) if capacity is None else int(capacity)
        if cap < 1:
            raise PswinError(f"RleMasks: capacity must be at least 1, got {cap}")
        return cls(torch.empty(n_masks + 1, dtype=torch.int64, device=device), torch.empty(cap, dtype=torch.uint32, device=device), height, width,
                   cap, B, K, count)

    @property
    def n_masks(self):
        return int(self.offsets.numel()) - 1

    def mask_counts(self):
        """Per mask its uint32 counts (an empty array for a row that is no detection) -- reads back: not for a captured step."""
        off = self.offsets.cpu().numpy()
        if int(off[-1]) > self.capacity:
            raise PswinError(f"RleMasks: the batch needs offsets[N] = {int(off[-1])} runs but capacity = {self.capacity}; encode again with "
                             f"a larger capacity")
        runs = self.runs[:max(int(off[-1]), 1)].cpu().numpy()
        return [runs[off[n]:off[n + 1]] for n in range(off.size - 1)]

    @classmethod
    def from_lists(cls, lists, device, K=None):
        """The inverse of to_lists(): per image a list of {"size": [H, W], "counts": bytes (pycocotools' string) or a sequence of ints} ->
        an RleMasks with B = len(lists), K (default: the largest count, at least 1), count int32 [B] and a pool of exactly the runs'
        total (at least 1).  Checked on the host: one size for all masks, runs that sum to H W, at most K masks per image.
        from_lists(x.to_lists(), ...) has x's offsets and x's runs below offsets[N]."""
        B = len(lists)
        counts = [len(per) for per in lists]
        K = max([1] + counts) if K is None else int(K)
        if B < 1 or K < 1 or max(counts) > K:
            raise PswinError(f"RleMasks.from_lists: {B} images with {counts} masks do not fit K = {K}")
        size, per_mask = None, []
        for per in lists:
            for d in per:
                hw = tuple(int(v) for v in d["size"])
                size = hw if size is None else size
                if len(hw) != 2 or hw != size or min(hw) < 1:
                    raise PswinError(f"RleMasks.from_lists: masks of one size [H, W], got {list(hw)} after {list(size)}")
                c = d["counts"]
                c = rle_from_string(c) if isinstance(c, (bytes, bytearray)) else np.asarray(c, dtype=np.int64).reshape(-1)
                if c.size and (int(c.min()) < 0 or int(c.max()) > 0xffffffff):
                    raise PswinError("RleMasks.from_lists: counts are uint32")
                if int(c.astype(np.int64).sum()) != hw[0] * hw[1]:
                    raise PswinError(f"RleMasks.from_lists: the runs sum to {int(c.astype(np.int64).sum())}, not to {hw[0]} x {hw[1]}")
                per_mask.append(c.astype(np.uint32))
            per_mask += [np.zeros(0, dtype=np.uint32)] * (K - len(per))
        if size is None:
            raise PswinError("RleMasks.from_lists: no mask gives the size")
        total = sum(c.size for c in per_mask)
        host = cls.allocate(B * K, size[0], size[1], "cpu", max(total, 1), B, K, torch.tensor(counts, dtype=torch.int32))
        _fill(host, per_mask)
        if total == 0:
            host.runs.zero_()
        return cls(host.offsets.to(device), host.runs.to(device), size[0], size[1], host.capacity, B, K, host.count.to(device))

    def to_lists(self):
        """Per image (one image when the masks are no detections) a list of {"size": [H, W], "counts": bytes}, one per detection row in row
        order -- what pycocotools' encode returns.  Raises PswinError when the pool was too small.  Reads back: not for a captured step."""
        per_mask = self.mask_counts()
        size = [self.height, self.width]
        if self.count is None:
            return [[dict(size=size, counts=rle_to_string(c)) for c in per_mask]]
        out = []
        for b, n in enumerate(self.count.tolist()):
            n = max(0, min(int(n), self.K))
            out.append([dict(size=size, counts=rle_to_string(per_mask[b * self.K + k])) for k in range(n)])
        return out


def _shape_nbk(masks, count):
    if masks.dtype != torch.uint8 or masks.dim() not in (3, 4) or not masks.is_contiguous():
        raise PswinError(f"encode_masks: masks must be a contiguous uint8 [N, H, W] or [B, K, H, W] tensor, got {masks.dtype} "
                         f"{tuple(masks.shape)}")
    H, W = int(masks.shape[-2]), int(masks.shape[-1])
    if masks.dim() == 4:
        B, K = int(masks.shape[0]), int(masks.shape[1])
    else:
        if count is not None:
            raise PswinError("encode_masks: count goes with [B, K, H, W] masks")
        B, K = None, None
    N = int(masks.numel() // max(H * W, 1)) if H * W else 0
    if N < 1 or H < 1 or W < 1:
        raise PswinError(f"encode_masks: empty masks {tuple(masks.shape)}")
    if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (B,)):
        raise PswinError("encode_masks: count must be an int32 [B] tensor")
    return N, B, K, H, W


def _fill(out, per_mask):
    """the definition's side of the overflow contract: offsets whole, runs below capacity only"""
    off = np.concatenate([[0], np.cumsum([c.size for c in per_mask])]).astype(np.int64)
    out.offsets.copy_(torch.from_numpy(off))
    flat = np.concatenate(per_mask) if per_mask else np.zeros(0, dtype=np.uint32)
    n = min(flat.size, out.capacity)
    if n:
        out.runs[:n] = torch.from_numpy(flat[:n].astype(np.uint32))
    return out


def _out_for(out, N, H, W, device, capacity, B, K, count, who):
    if out is None:
        return RleMasks.allocate(N, H, W, device, capacity, B, K, count)
    cap = out.capacity if capacity is None else int(capacity)
    if out.offsets.dtype != torch.int64 or out.offsets.numel() != N + 1 or out.runs.dtype != torch.uint32 or cap < 1 or \
            cap > out.runs.numel() or out.offsets.device != device or out.runs.device != device or not out.offsets.is_contiguous() or \
            not out.runs.is_contiguous():
        raise PswinError(f"{who}: out must hold int64 offsets [{N + 1}] and contiguous uint32 runs of at least capacity = {cap} on the "
                         f"device of the input")
    out.height, out.width, out.capacity, out.B, out.K, out.count = H, W, cap, B, K, count
    return out


def encode_masks_definition(masks, count=None, capacity=None, out=None):
    """encode_masks on the CPU: rle_encode of every mask that is a detection row, laid out as RleMasks lays them out"""
    N, B, K, H, W = _shape_nbk(masks, count)
    out = _out_for(out, N, H, W, masks.device, capacity, B, K, count, "encode_masks")
    m = masks.reshape(N, H, W).numpy()
    if count is None:
        live = np.ones(N, dtype=bool)
    else:
        live = (np.arange(K)[None, :] < np.clip(count.numpy().astype(np.int64), 0, K)[:, None]).reshape(-1)
    return _fill(out, [rle_encode(m[n]) if live[n] else np.zeros(0, dtype=np.uint32) for n in range(N)])


def encode_masks(masks, count=None, capacity=None, out=None):
    """uint8 [N, H, W] or [B, K, H, W] masks (contiguous; non-zero = foreground) -> RleMasks.  count int32 [B] (with the 4-d form): rows
    k >= count[b] (clamped to [0, K]) are not read and own no runs.  capacity: the length of the run pool (default_capacity); out: an
    RleMasks to reuse.  HIP tensors: ops.rle_encode (no host synchronisation: capturable); CPU tensors: the definition."""
    if masks.is_cuda:
        from . import ops
        return ops.rle_encode(masks, count, capacity, out)
    return encode_masks_definition(masks, count, capacity, out)


def paste_masks_rle(mask_logits, labels, boxes, count, thr, out_hw, capacity=None, out=None):
    """By definition encode_masks(detector.paste_masks_batch(mask_logits, labels, boxes, count, thr, out_hw), count).  HIP tensors:
    ops.paste_masks_rle, which forms the column bits from the 28 x 28 logits and never writes the bitmap; CPU tensors: the definition."""
    if mask_logits.is_cuda:
        from . import ops
        return ops.paste_masks_rle(mask_logits, labels, boxes, count, thr, out_hw, capacity, out)
    from . import detector
    masks = detector.paste_masks_batch(mask_logits, labels, boxes, count, thr, out_hw)
    return encode_masks_definition(masks, count.to(torch.int32), capacity, out)


# ------------------------------------------------------------------------------------------------------------------------
# intersections and areas of a padded batch, from the runs
# ------------------------------------------------------------------------------------------------------------------------
def _counts_of_side(enc, count, B, rows, who):
    """per mask (b, row): its counts; an empty array for a row past the count; None for a mask inside the count that is not whole"""
    if enc.offsets.numel() != B * rows + 1:
        raise PswinError(f"inter_pairs_definition: {who} holds {enc.offsets.numel() - 1} masks, the batch has {B} x {rows}")
    off = enc.offsets.cpu().numpy()
    runs = enc.runs.cpu().numpy()[:enc.capacity]
    live = np.clip(count.cpu().numpy().astype(np.int64), 0, rows)
    out = []
    for b in range(B):
        for r in range(rows):
            o0, o1 = int(off[b * rows + r]), int(off[b * rows + r + 1])
            if r >= live[b]:
                out.append(np.zeros(0, dtype=np.int64))
            elif 0 <= o0 <= o1 <= enc.capacity:
                out.append(runs[o0:o1].astype(np.int64))
            else:
                out.append(None)
    return out


def inter_pairs_definition(det_rle, det_labels, det_count, gt_rle, gt_labels, gt_count):
    """(inter int32 [B, K, G], areas int32 [B, K + G], overflow int32 [1]) from two RleMasks of one size, with the layout and the -1 / 0
    conventions of evaluation.mask_inter_pairs: inter is rle_inter for the pairs with k < det_count[b], g < gt_count[b] (both clamped) and
    equal labels, -1 for every other pair; areas are rle_area of image b's detections (first K) and boxes (last G), 0 past a count.
    Overflow: a mask inside its count is whole when 0 <= offsets[n] <= offsets[n + 1] <= capacity; one that is not has area 0 and
    intersection 0 in its pairs, nothing of it is read, and overflow is 1."""
    (B, K), G = det_labels.shape, gt_labels.shape[1]
    if (det_rle.height, det_rle.width) != (gt_rle.height, gt_rle.width):
        raise PswinError(f"inter_pairs_definition: masks of {det_rle.height} x {det_rle.width} against {gt_rle.height} x {gt_rle.width}")
    d = _counts_of_side(det_rle, det_count, B, K, "det_rle")
    g = _counts_of_side(gt_rle, gt_count, B, G, "gt_rle")
    dl, gl = det_labels.cpu().numpy(), gt_labels.cpu().numpy()
    dn, gn = np.clip(det_count.cpu().numpy().astype(np.int64), 0, K), np.clip(gt_count.cpu().numpy().astype(np.int64), 0, G)
    inter = np.full((B, K, G), -1, dtype=np.int64)
    areas = np.zeros((B, K + G), dtype=np.int64)
    overflow = int(any(c is None for c in d + g))
    for b in range(B):
        for k in range(dn[b]):
            cd = d[b * K + k]
            areas[b, k] = 0 if cd is None else rle_area(cd)
        for j in range(gn[b]):
            cg = g[b * G + j]
            areas[b, K + j] = 0 if cg is None else rle_area(cg)
        for k in range(dn[b]):
            for j in range(gn[b]):
                if dl[b, k] == gl[b, j]:
                    cd, cg = d[b * K + k], g[b * G + j]
                    inter[b, k, j] = 0 if cd is None or cg is None else rle_inter(cd, cg)
    return torch.from_numpy(inter.astype(np.int32)), torch.from_numpy(areas.astype(np.int32)), torch.tensor([overflow], dtype=torch.int32)
