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

RleMasks holds the runs of N masks in buffers of a fixed shape (the RLE counterpart of Detections / PaddedTargets), so that a captured
inference step can produce them; the strings are made on the host when results are read back (to_lists): producing them on the device is
out of scope, and so are RLE inputs to the mask IoU kernels, a fused form for test-time augmentation and polygon / frPyObjects decoding.
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
