"""Cases of the RLE tests (test_rle.py on the CPU, test_rle_gpu.py on the GPU), a restatement of pycocotools' rleEncode / rleToString /
rleFrString as plain loops -- written statement by statement after the C and independent of the vectorised forms in
panoswintransformerobjectdetection_amd/rle.py -- and encoders with one planted defect each, which the cases must tell from the truth."""
import numpy as np
import torch

HAND_ENCODE = [
    (np.array([[0, 1, 0], [0, 1, 0], [0, 0, 0]], dtype=np.uint8), [3, 2, 4]),
    (np.ones((2, 3), dtype=np.uint8), [0, 6]),
    (np.zeros((2, 3), dtype=np.uint8), [6]),
]
HAND_STRING = [([3, 2, 4], b"324"), ([0, 100, 5, 40], b"0T35TN")]


# ---- the C, as loops -------------------------------------------------------------------------------------------------------
def loop_encode(mask):
    """rleEncode for one mask: M is the column-major byte string (a pixel is foreground when its byte is non-zero)"""
    h, w = mask.shape
    M = [1 if mask[j % h, j // h] != 0 else 0 for j in range(h * w)]
    cnts, c, p = [], 0, 0
    for j in range(h * w):
        if M[j] != p:
            cnts.append(c)
            c = 0
            p = M[j]
        c += 1
    cnts.append(c)
    return cnts


def loop_to_string(cnts):
    s = bytearray()
    for i in range(len(cnts)):
        x = int(cnts[i])
        if i > 2:
            x -= int(cnts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5                                      # Python's >> on a negative int is arithmetic, as C's on a long
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            s.append(c + 48)
    return bytes(s)


def loop_from_string(s):
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[len(cnts) - 2]
        cnts.append(x & 0xffffffff)
    return cnts


def loop_decode(cnts, h, w):
    flat, v = [], 0
    for c in cnts:
        flat += [v] * int(c)
        v = 1 - v
    m = np.zeros((h, w), dtype=np.uint8)
    for j, b in enumerate(flat):
        m[j % h, j // h] = b
    return m


# ---- masks -----------------------------------------------------------------------------------------------------------------
def patterns(H, W, seed=0):
    """name -> uint8 [H, W]: the patterns at which a tail, a carry, a join or a second word can go wrong"""
    g = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = {
        "zeros": np.zeros((H, W), np.uint8),
        "ones": np.ones((H, W), np.uint8),
        "checker": ((yy + xx) & 1).astype(np.uint8),
        "checker1": ((yy + xx + 1) & 1).astype(np.uint8),            # starts with 1: H W + 1 runs for odd H, the maximum
        "hstripe1": (yy & 1).astype(np.uint8),
        "hstripe64": ((yy // 64) & 1).astype(np.uint8) ^ 1,
        "vstripe": (xx & 1).astype(np.uint8),
        "vstripe1": ((xx + 1) & 1).astype(np.uint8),
        "rand01": (g.random((H, W)) < 0.01).astype(np.uint8),
        "rand50": (g.random((H, W)) < 0.5).astype(np.uint8),
        "rand99": (g.random((H, W)) < 0.99).astype(np.uint8),
        "bytes": ((g.random((H, W)) < 0.5) * g.choice(np.array([2, 255], np.uint8), (H, W))).astype(np.uint8),
    }
    corners = np.zeros((H, W), np.uint8)
    corners[0, 0] = corners[0, W - 1] = corners[H - 1, 0] = corners[H - 1, W - 1] = 1
    out["corners"] = corners
    for name, (ya, yb, xa, xb) in dict(c00=(0, 0, 0, 0), c01=(0, 0, W - 1, W - 1), c10=(H - 1, H - 1, 0, 0), c11=(H - 1, H - 1, W - 1, W - 1)).items():
        m = np.zeros((H, W), np.uint8)
        m[ya, xa] = 1
        out[name] = m
    join11 = np.zeros((H, W), np.uint8)                               # every column ends in 1; the next starts in 1 (even x) or in 0 (odd x)
    join11[H - 1, :] = 1
    join11[0, 0::2] = 1
    out["join"] = join11
    return out


CPU_SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (3, 3), (7, 4), (64, 3), (65, 2), (130, 3)]
GPU_H = (1, 2, 63, 64, 65, 128, 130)
GPU_W = (1, 15, 16, 17, 64, 65, 257)


def cpu_masks():
    out = [(f"hand{i}", m) for i, (m, _) in enumerate(HAND_ENCODE)]
    for H, W in CPU_SHAPES:
        out += [(f"{name}_{H}x{W}", m) for name, m in patterns(H, W).items()]
    return out


STRING_CASES = [
    [3, 2, 4], [0, 100, 5, 40], [0], [7], [0, 6], [31, 32, 33], [15, 16, 17, 1, 1, 40000],
    [5, 1 << 15, (1 << 15) + 3, 1, 1 << 15], [1, (1 << 30) + 5, 2, 7, (1 << 30) + 9, 3], [(1 << 32) - 1],
    [10, 20, 30, 10, 5, 1000, 4, 999, 1 << 20, 3],                    # negative deltas at i = 3, 4, ...; i = 2 has none
    [100, 100, 50, 84, 66, 83],                                       # deltas -16 and -17 at the sign bit of one group
    [9, 9, 9, 9, 9, 9], [1, 2, 1024, 2, 1, 2],
]


def paste_inputs(B, K, C, H, W, logits="noise", seed=0):
    """(mask_logits f32 [B K, C, 28, 28], labels, boxes, count) for the fused producer: labels at 0 and C - 1 among others; boxes that are
    the whole image, fractional, half and wholly outside, degenerate (x0 == x1, y0 == y1, both, x0 == x1 on a pixel centre), huge and
    inverted"""
    g = torch.Generator().manual_seed(seed)
    N = B * K
    if logits == "noise":
        lg = (torch.rand(N, C, 28, 28, generator=g) * 2 - 1) * 4
    elif logits == "blob":
        yy, xx = torch.meshgrid(torch.arange(28.), torch.arange(28.), indexing="ij")
        r = ((yy - 13.5) ** 2 + (xx - 13.5) ** 2).sqrt()
        lg = (9.0 - r)[None, None].expand(N, C, 28, 28) + torch.rand(N, C, 1, 1, generator=g)
    else:
        lg = torch.full((N, C, 28, 28), float(logits))
    w, h = float(W), float(H)
    pool = [
        [0, 0, w, h], [0.3 * w + 0.37, 0.2 * h + 0.61, 0.8 * w - 0.13, 0.9 * h - 0.29], [-0.5 * w, 0.1 * h, 0.5 * w, 0.7 * h], [2 * w, 2 * h, 3 * w, 3 * h],
        [0.5 * w, 0.1 * h, 0.5 * w, 0.9 * h], [0.1 * w, 0.5 * h, 0.9 * w, 0.5 * h], [0.4 * w, 0.4 * h, 0.4 * w, 0.4 * h],
        [50.5, 0, 50.5, h], [-1e6, -1e6, 1e6, 1e6], [0.8 * w, 0.9 * h, 0.2 * w, 0.1 * h], [0.5, 0.5, 0.5, 0.5], [0, 0, 1e6, 1],
    ]
    idx = (torch.arange(N) + seed) % len(pool)
    boxes = torch.tensor(pool, dtype=torch.float32)[idx].reshape(B, K, 4)
    labels = ((torch.arange(N) * 3 + seed) % C).reshape(B, K)
    labels[0, 0], labels[-1, -1] = 0, C - 1
    count = torch.tensor([K - (b % 2) * 2 for b in range(B)], dtype=torch.int32)
    return lg.contiguous(), labels.long(), boxes, count


# ---- planted defects -------------------------------------------------------------------------------------------------------
def _defect_row_major(mask):
    h, w = mask.shape
    return loop_encode(mask.reshape(-1).reshape(w, h).T)         # its column-major scan is the row-major scan of mask


def _defect_no_leading_zero(mask):
    c = loop_encode(mask)
    return c[1:] if c[0] == 0 else c


def _defect_no_final_run(mask):
    return loop_encode(mask)[:-1]


def _positions_with_join(mask, join):
    """boundaries when the predecessor of a column's first pixel is join(x); the truth is the last pixel of column x - 1"""
    h, w = mask.shape
    m = mask != 0
    pos = []
    for x in range(w):
        prev = join(m, x)
        for y in range(h):
            if m[y, x] != prev:
                pos.append(x * h + y)
            prev = m[y, x]
    return list(np.diff([0] + pos + [h * w]))


def _defect_join_ignored(mask):
    return _positions_with_join(mask, lambda m, x: False)


def _defect_join_wrong_column(mask):
    return _positions_with_join(mask, lambda m, x: m[-1, x])


def _defect_delta_at_2(cnts):
    s = bytearray()
    for i in range(len(cnts)):
        x = int(cnts[i]) - (int(cnts[i - 2]) if i > 1 else 0)
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            s.append((c | 0x20 if more else c) + 48)
    return bytes(s)


def _defect_logical_shift(cnts):
    s = bytearray()
    for i in range(len(cnts)):
        x = (int(cnts[i]) - (int(cnts[i - 2]) if i > 2 else 0)) & 0xffffffffffffffff
        more, n = True, 0
        while more and n < 13:
            c = x & 0x1f
            x >>= 5                                      # on the unsigned value: zeros come in at the top
            more = (x != 0xffffffffffffffff) if (c & 0x10) else (x != 0)
            s.append((c | 0x20 if more else c) + 48)
            n += 1
    return bytes(s)


def _defect_rows_past_count(masks, count):
    B, K = masks.shape[:2]
    return [loop_encode(masks[b, k]) for b in range(B) for k in range(K)]


ENCODE_DEFECTS = dict(row_major=_defect_row_major, no_leading_zero=_defect_no_leading_zero, no_final_run=_defect_no_final_run,
                      join_ignored=_defect_join_ignored, join_wrong_column=_defect_join_wrong_column)
STRING_DEFECTS = dict(delta_at_2=_defect_delta_at_2, logical_shift=_defect_logical_shift)
BATCH_DEFECTS = dict(rows_past_count=_defect_rows_past_count)


def batch_truth(masks, count):
    B, K = masks.shape[:2]
    return [loop_encode(masks[b, k]) if k < max(0, min(int(count[b]), K)) else [] for b in range(B) for k in range(K)]


def results_truth(boxes, scores, labels, count, masks, num_classes):
    """bbox2result + cls_segms + encode_mask_results as loops, on numpy arrays of a Detections"""
    out = []
    B, K = labels.shape
    for b in range(B):
        n = max(0, min(int(count[b]), K))
        bbox = [[] for _ in range(num_classes)]
        segm = [[] for _ in range(num_classes)]
        for i in range(n):
            c = int(labels[b, i])
            bbox[c].append(list(boxes[b, i]) + [scores[b, i]])
            segm[c].append(dict(size=[int(masks.shape[2]), int(masks.shape[3])], counts=loop_to_string(loop_encode(masks[b, i]))))
        out.append(([np.asarray(r, dtype=np.float32).reshape(-1, 5) for r in bbox], segm))
    return out


# ---- the kernels' formulation, pass by pass (csrc/pswin_rle.hip), in Python integers -------------------------------------------
def emulate_kernel_passes(masks, live, capacity, poison=0xA5A5A5A5):
    """What the four launches compute, restated on the CPU: (1) bit-planes word (n, w, x) = pixels 64 w .. 64 w + 63 of column x;
    (2) per column trans = w ^ ((w << 1) | carry) masked to the valid rows, its popcount, the exclusive sum over the columns and the
    exclusive maximum of the last boundary's position; (3) offsets = exclusive sum over the masks of boundaries + 1 (0 for a mask that
    is not live); (4) per column position - previous for each set bit, the last column adding H W - previous; stores only below
    `capacity`.  -> (offsets list [N + 1], runs list [capacity] with `poison` where nothing was written)"""
    N, H, W = masks.shape
    HW, M64 = (H + 63) // 64, (1 << 64) - 1
    planes = [[[0] * W for _ in range(HW)] for _ in range(N)]
    for n in range(N):
        if live[n]:
            for x in range(W):
                for y in range(H):
                    if masks[n, y, x] != 0:
                        planes[n][y // 64][x] |= 1 << (y & 63)

    def trans(word, carry, valid):
        t = word ^ (((word << 1) & M64) | carry)
        return t if valid >= 64 else t & ((1 << valid) - 1)

    def join(pl, x):
        return (pl[HW - 1][x - 1] >> ((H - 1) & 63)) & 1 if x > 0 else 0

    colstart, lastpos, totals = [[0] * W for _ in range(N)], [[0] * W for _ in range(N)], [0] * N
    for n in range(N):
        if not live[n]:
            continue
        run_sum = run_max = 0
        for x in range(W):
            carry, c, lp = join(planes[n], x), 0, 0
            for w in range(HW):
                tr = trans(planes[n][w][x], carry, H - 64 * w)
                carry = planes[n][w][x] >> 63
                c += bin(tr).count("1")
                if tr:
                    lp = x * H + 64 * w + tr.bit_length() - 1
            colstart[n][x], lastpos[n][x] = run_sum, run_max
            run_sum, run_max = run_sum + c, max(run_max, lp)
        totals[n] = run_sum + 1
    offsets = [0]
    for n in range(N):
        offsets.append(offsets[-1] + totals[n])
    runs = [poison] * capacity
    for n in range(N):
        if not live[n]:
            continue
        for x in range(W):
            slot, prev, carry = offsets[n] + colstart[n][x], lastpos[n][x], join(planes[n], x)
            for w in range(HW):
                tr = trans(planes[n][w][x], carry, H - 64 * w)
                carry = planes[n][w][x] >> 63
                while tr:
                    pos = x * H + 64 * w + (tr & -tr).bit_length() - 1
                    tr &= tr - 1
                    if slot < capacity:
                        runs[slot] = pos - prev
                    prev, slot = pos, slot + 1
            if x == W - 1 and slot < capacity:
                runs[slot] = H * W - prev
    return offsets, runs
