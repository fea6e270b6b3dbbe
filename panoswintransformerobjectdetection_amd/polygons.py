"""COCO polygon annotations to masks: the rule (plain loops on the CPU), the fixed-shape container of a batch's polygons and the entry
points that dispatch to the HIP kernels (pswin_poly_masks of csrc/pswin_poly.hip, in a library of its own: _poly_lib).

The reference rasterises every non-crowd instance from its polygons: `LoadAnnotations._poly2mask` (mmdet/datasets/pipelines/loading.py:
266-291) and `polygon_to_bitmap` (mmdet/core/mask/structures.py:1010-1024) both call maskUtils.frPyObjects(polygons, h, w), then
maskUtils.merge(rles) and decode the result at once.  That is pycocotools' rleFrPoly (maskApi.c) followed by a union.

PARITY: unpinned.  pycocotools is neither on the development machine nor in the reference tree, so nothing here is compared against it.
The rule below restates the published rleFrPoly completely; tests/_poly_cases.py restates it a second time, independently, column by
column.  If pycocotools ever becomes available, that restatement is where a pin attaches.

  rle_from_polygon(xy, h, w).  One polygon part is a flat sequence x0, y0, x1, y1, ... of k >= 3 points (doubles) for an image of h rows
  and w columns.  All arithmetic is IEEE double without fused multiply-add; int(.) truncates toward zero.
    1. Vertices.  X[j] = int(5 x_j + 0.5), Y[j] = int(5 y_j + 0.5); X[k] = X[0], Y[k] = Y[0].
    2. Points.  For each edge j, from (xs, ys) = (X[j], Y[j]) to (xe, ye) = (X[j + 1], Y[j + 1]): dx = |xe - xs|, dy = |ye - ys|.  The
       edge is flipped when (dx >= dy and xs > xe) or (dx < dy and ys > ye); flipping swaps the two ends for the arithmetic only.  If
       dx >= dy: s = double(ye - ys) / dx and for d = 0 .. dx, with t = dx - d if flipped else d, the point is u = xs + t,
       v = int(ys + s t + 0.5).  Otherwise s = double(xe - xs) / dy and for d = 0 .. dy the point is v = ys + t, u = int(xs + s t + 0.5).
       The points are listed in the polygon's own direction.  A zero-length edge (dx = dy = 0) contributes the one point u = xs; its v is
       never read (see 3) and is not computed: there is no 0 / 0 here or in the kernel.
    3. Events.  For consecutive points j - 1, j of the whole list with u[j] != u[j - 1]: xd = (min(u[j], u[j - 1]) + 0.5) / 5 - 0.5 (u
       moves by at most 1 per point, so this is the C code's u[j] < u[j - 1] ? u[j] : u[j] - 1); the pair is skipped unless xd is an
       integer with 0 <= xd <= w - 1.  yd = (min(v[j], v[j - 1]) + 0.5) / 5 - 0.5, clamped to [0, h], then ceil.  The event is the
       position xd h + yd -- column-major, as everywhere in rle.py; with yd = h it is the top of the next column.  The neighbours of a
       zero-length edge's point have its u, or lie left of column 0 with it, so no pair that reaches yd holds it.
    4. Runs.  Append the position h w; sort; take differences from 0; copy the first difference; for each later difference a positive
       one is appended, a zero one is dropped together with its successor, which is added to the last run (a zero that is the last
       difference is simply dropped).
  What follows from the rule (tests/test_polygons.py re-establishes each on thousands of polygons): the runs sum to h w and are canonical
  (rle_encode(rle_decode(.)) returns them); the decoded bitmap is "toggle one bit at every event position, then take the prefix XOR in
  scan order".  And since the point list is a closed walk in u with steps of at most 1 wherever u >= 1, it passes between u = 5 c + 2 and
  5 c + 3 an even number of times: EVERY COLUMN HOLDS AN EVEN NUMBER OF EVENTS.  So the prefix XOR starts from 0 at the top of every
  column, an event with yd = h changes nothing, and a column's bits are a function of the events of that column alone -- which is what
  the kernel uses: a lane per column, no carry between lanes.  An edge has an event in column c exactly when
  min(xs, xe) <= 5 c + 2 and 5 c + 3 <= max(xs, xe).

  One object is a list of parts; its mask is the OR of the parts' decoded bitmaps (what the reference hands on, since it decodes the
  merged RLE at once) and its RLE is rle.rle_encode of that bitmap.

PolygonBatch holds the polygons of a padded batch in buffers of a fixed shape, the polygon counterpart of detector.PaddedTargets and
rle.RleMasks.  It takes polygon objects only: objects given as RLE dicts (COCO's crowds) keep going through rle.RleMasks.from_lists, and
putting both kinds into one RleMasks is out of scope, as are geometric transforms of the vertices (the project augments bitmaps).
"""
import ctypes
import math

import numpy as np
import torch

from ._lib import PswinError
from . import rle as _rle

SCALE = 5.0
COORD_LIMIT = float(1 << 20)
MAX_SIDE = 4096


# ------------------------------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------------------------------
def _check_part(xy, who="rle_from_polygon"):
    a = np.asarray(xy, dtype=np.float64).reshape(-1)
    if a.size < 6 or a.size % 2:
        raise PswinError(f"{who}: a polygon part is x0, y0, x1, y1, ... with at least 3 points, got {a.size} numbers")
    if not np.isfinite(a).all() or float(np.abs(a).max()) > COORD_LIMIT:
        raise PswinError(f"{who}: coordinates must be finite with |x|, |y| <= 2^20")
    return a


def polygon_points(xy):
    """steps 1 and 2 of the rule: the lists u, v (v is None for the point of a zero-length edge)"""
    a = _check_part(xy)
    k = a.size // 2
    X = [int(SCALE * float(a[2 * j]) + 0.5) for j in range(k)]
    Y = [int(SCALE * float(a[2 * j + 1]) + 0.5) for j in range(k)]
    X.append(X[0])
    Y.append(Y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ye - ys)
        if dx == 0 and dy == 0:
            u.append(xs)
            v.append(None)
            continue
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = float(ye - ys) / dx
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(xs + t)
                v.append(int(ys + s * t + 0.5))
        else:
            s = float(xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(ys + t)
                u.append(int(xs + s * t + 0.5))
    return u, v


def polygon_events(xy, h, w):
    """step 3 of the rule: the event positions, in list order"""
    u, v = polygon_points(xy)
    events = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = (min(u[j], u[j - 1]) + 0.5) / SCALE - 0.5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = (min(v[j], v[j - 1]) + 0.5) / SCALE - 0.5
        yd = math.ceil(min(max(yd, 0.0), float(h)))
        events.append(int(xd) * h + int(yd))
    return events


def rle_from_polygon(xy, h, w):
    """One polygon part -> its counts (a uint32 array), by the rule of the module docstring"""
    h, w = int(h), int(w)
    if h < 1 or w < 1 or h * w >= 1 << 32:
        raise PswinError(f"rle_from_polygon: an image of {h} x {w}")
    a = sorted(polygon_events(xy, h, w) + [h * w])
    diffs, p = [], 0
    for t in a:
        diffs.append(t - p)
        p = t
    b = [diffs[0]]
    j = 1
    while j < len(diffs):
        if diffs[j] > 0:
            b.append(diffs[j])
            j += 1
        else:
            j += 1
            if j < len(diffs):
                b[-1] += diffs[j]
                j += 1
    return np.asarray(b, dtype=np.uint32)


def object_mask(parts, h, w):
    """One object (a list of parts) -> uint8 [h, w] of 0 / 1: the OR of the parts' decoded bitmaps"""
    m = np.zeros((h, w), dtype=np.uint8)
    for part in parts:
        m |= _rle.rle_decode(rle_from_polygon(part, h, w), h, w)
    return m


# ------------------------------------------------------------------------------------------------------------------------
# the polygons of a batch
# ------------------------------------------------------------------------------------------------------------------------
def poly_supported(B, K, H, W):
    """Whether the polygon kernels take the shape: H, W <= 4096 (a column's bits live in the workgroup's LDS), H W < 2^32, fewer than
    2^31 objects.  The number of vertices of a part is limited by the buffers alone."""
    return 1 <= int(B) and 1 <= int(K) and int(B) * int(K) < 1 << 31 and 1 <= int(H) <= MAX_SIDE and 1 <= int(W) <= MAX_SIDE


class PolygonBatch:
    """The polygon objects of B images, K rows each, in fixed-shape buffers: xy float64 [Vcap, 2] (x, y of every vertex, part after part),
    part_offsets int32 [Pcap + 1] (part p owns the vertices part_offsets[p] .. part_offsets[p + 1]), obj_offsets int32 [B K + 1] (object
    n = b K + k owns the parts obj_offsets[n] .. obj_offsets[n + 1]; flat across the rows past count[b]) and count int32 [B].  The unused
    tails of part_offsets and xy are flat / zero.  Only polygon objects are taken: an RLE dict (a crowd) is refused -- those go through
    rle.RleMasks.from_lists, and mixing both kinds in one RleMasks is out of scope.
    Checked on the host (PswinError): every part has an even number of at least 6 coordinates (the reference's process_polygons rule),
    all finite with |x|, |y| <= 2^20 so that every int(.) of the rule is defined; at most K objects per image; the capacities."""

    def __init__(self, xy, part_offsets, obj_offsets, count, height, width, B, K):
        self.xy, self.part_offsets, self.obj_offsets, self.count = xy, part_offsets, obj_offsets, count
        self.height, self.width, self.B, self.K = int(height), int(width), int(B), int(K)

    @property
    def max_vertices(self):
        return int(self.xy.shape[0])

    @property
    def max_parts(self):
        return int(self.part_offsets.numel()) - 1

    @property
    def device(self):
        return self.xy.device

    @classmethod
    def allocate(cls, B, K, max_parts, max_vertices, height, width, device):
        """Zeroed buffers (an empty batch: count = 0 everywhere) for copy_from to fill"""
        B, K, P, V = int(B), int(K), int(max_parts), int(max_vertices)
        if B < 1 or K < 1 or P < 1 or V < 1 or int(height) < 1 or int(width) < 1:
            raise PswinError(f"PolygonBatch.allocate: B = {B}, K = {K}, max_parts = {P}, max_vertices = {V}, {height} x {width}")
        return cls(torch.zeros(V, 2, dtype=torch.float64, device=device), torch.zeros(P + 1, dtype=torch.int32, device=device),
                   torch.zeros(B * K + 1, dtype=torch.int32, device=device), torch.zeros(B, dtype=torch.int32, device=device),
                   height, width, B, K)

    @staticmethod
    def _host(annotations, B, K, max_parts, max_vertices, who):
        """the four host arrays for `annotations` (per image a list of objects, each a list of flat coordinate sequences)"""
        if len(annotations) != B:
            raise PswinError(f"{who}: {len(annotations)} images, the batch has {B}")
        counts = [len(per) for per in annotations]
        if max(counts) > K:
            raise PswinError(f"{who}: an image has {max(counts)} objects, K = {K}")
        verts, part_off, obj_off = [], [0], [0]
        for per in annotations:
            for obj in per:
                if isinstance(obj, dict) or isinstance(obj, (bytes, str)):
                    raise PswinError(f"{who}: objects are lists of polygon parts; RLE objects (crowds) go through RleMasks.from_lists")
                for part in obj:
                    a = _check_part(part, who)
                    verts.append(a.reshape(-1, 2))
                    part_off.append(part_off[-1] + a.size // 2)
                obj_off.append(len(part_off) - 1)
            obj_off += [obj_off[-1]] * (K - len(per))
        n_parts, n_verts = len(part_off) - 1, part_off[-1]
        P = max(n_parts, 1) if max_parts is None else max_parts
        V = max(n_verts, 1) if max_vertices is None else max_vertices
        if n_parts > P or n_verts > V:
            raise PswinError(f"{who}: {n_parts} parts and {n_verts} vertices do not fit max_parts = {P}, max_vertices = {V}")
        xy = np.zeros((V, 2), dtype=np.float64)
        if n_verts:
            xy[:n_verts] = np.concatenate(verts)
        po = np.full(P + 1, n_verts, dtype=np.int32)
        po[:n_parts + 1] = part_off
        return xy, po, np.asarray(obj_off, dtype=np.int32), np.asarray(counts, dtype=np.int32)

    @classmethod
    def from_lists(cls, annotations, height, width, device, K=None):
        """annotations: per image a list of objects, each object a list of flat coordinate sequences [x0, y0, x1, y1, ...] -- what
        ann_info['masks'] holds for non-crowd instances.  K defaults to the largest count (at least 1); the buffers hold exactly the
        batch's parts and vertices (at least 1)."""
        B = len(annotations)
        K = max([1] + [len(per) for per in annotations]) if K is None else int(K)
        if B < 1 or K < 1 or int(height) < 1 or int(width) < 1:
            raise PswinError(f"PolygonBatch.from_lists: {B} images, K = {K}, {height} x {width}")
        xy, po, oo, cnt = cls._host(annotations, B, K, None, None, "PolygonBatch.from_lists")
        return cls(torch.from_numpy(xy).to(device), torch.from_numpy(po).to(device), torch.from_numpy(oo).to(device),
                   torch.from_numpy(cnt).to(device), height, width, B, K)

    def copy_from(self, annotations):
        """Fill the buffers in place with another batch of the same B (four copies, nothing else): for a captured step that is replayed
        on new batches, like PaddedTargets.copy_from.  The same checks as from_lists, against this batch's K and capacities."""
        xy, po, oo, cnt = self._host(annotations, self.B, self.K, self.max_parts, self.max_vertices, "PolygonBatch.copy_from")
        self.xy.copy_(torch.from_numpy(xy))
        self.part_offsets.copy_(torch.from_numpy(po))
        self.obj_offsets.copy_(torch.from_numpy(oo))
        self.count.copy_(torch.from_numpy(cnt))
        return self

    def to_lists(self):
        """the inverse of from_lists (reads back: not for a captured step)"""
        xy, po, oo = self.xy.cpu().numpy(), self.part_offsets.cpu().numpy(), self.obj_offsets.cpu().numpy()
        out = []
        for b, n in enumerate(self.count.tolist()):
            n = max(0, min(int(n), self.K))
            out.append([[xy[po[p]:po[p + 1]].reshape(-1).tolist() for p in range(oo[b * self.K + k], oo[b * self.K + k + 1])]
                        for k in range(n)])
        return out


def _check_batch(polys, who):
    if not isinstance(polys, PolygonBatch):
        raise PswinError(f"{who}: polys must be a PolygonBatch, got {type(polys).__name__}")
    N = polys.B * polys.K
    dev = polys.xy.device
    if polys.xy.dtype != torch.float64 or polys.xy.dim() != 2 or polys.xy.shape[1] != 2 or polys.xy.shape[0] < 1 or \
            polys.part_offsets.dtype != torch.int32 or polys.part_offsets.numel() < 2 or polys.obj_offsets.dtype != torch.int32 or \
            polys.obj_offsets.numel() != N + 1 or polys.count.dtype != torch.int32 or tuple(polys.count.shape) != (polys.B,) or \
            any(t.device != dev or not t.is_contiguous() for t in (polys.xy, polys.part_offsets, polys.obj_offsets, polys.count)):
        raise PswinError(f"{who}: a PolygonBatch holds contiguous xy float64 [Vcap, 2], part_offsets int32 [Pcap + 1], obj_offsets int32 "
                         f"[B K + 1] and count int32 [B] on one device")
    if polys.height < 1 or polys.width < 1 or polys.height * polys.width >= 1 << 32:
        raise PswinError(f"{who}: an image of {polys.height} x {polys.width}")
    return N


def _masks_out(out, polys, who):
    shape = (polys.B, polys.K, polys.height, polys.width)
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=polys.xy.device)
    if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != polys.xy.device:
        raise PswinError(f"{who}: out must be a contiguous uint8 {list(shape)} tensor on the device of the polygons")
    return out


def polygons_to_masks_definition(polys, out=None):
    """polygons_to_masks on the CPU: object_mask of every object inside its image's count, zeros in the rows past it"""
    _check_batch(polys, "polygons_to_masks")
    out = _masks_out(out, polys, "polygons_to_masks")
    out.zero_()
    for b, per in enumerate(polys.to_lists()):
        for k, obj in enumerate(per):
            out[b, k] = torch.from_numpy(object_mask(obj, polys.height, polys.width))
    return out


def polygons_to_rle_definition(polys, capacity=None, out=None):
    """polygons_to_rle on the CPU: rle.rle_encode of every object's mask, laid out as RleMasks lays them out"""
    N = _check_batch(polys, "polygons_to_rle")
    H, W = polys.height, polys.width
    out = _rle._out_for(out, N, H, W, polys.xy.device, capacity, polys.B, polys.K, polys.count, "polygons_to_rle")
    per_mask = []
    for per in polys.to_lists():
        per_mask += [_rle.rle_encode(object_mask(obj, H, W)) for obj in per] + [np.zeros(0, dtype=np.uint32)] * (polys.K - len(per))
    return _rle._fill(out, per_mask)


_CACHE = {}


def _scratch(polys, what, nbytes_or_shape):
    """per (shape, device) buffers of the GPU route: the bit-plane workspace and, for polygons_to_rle, the bitmaps"""
    key = (what, polys.B, polys.K, polys.height, polys.width, str(polys.xy.device))
    if key not in _CACHE:
        _CACHE[key] = torch.empty(nbytes_or_shape, dtype=torch.uint8, device=polys.xy.device)
    return _CACHE[key]


def poly_workspace(polys):
    from . import _poly_lib
    nbytes = ctypes.c_longlong(0)
    _poly_lib.check(_poly_lib.load().pswin_poly_workspace(polys.B, polys.K, polys.height, polys.width, ctypes.byref(nbytes)),
                    "pswin_poly_workspace")
    return _scratch(polys, "planes", int(nbytes.value))


def _masks_hip(polys, out, who):
    from . import _poly_lib
    _check_batch(polys, who)
    if not poly_supported(polys.B, polys.K, polys.height, polys.width):
        raise PswinError(f"{who}: outside the kernels' limits (H, W <= 4096, B K < 2^31): B = {polys.B}, K = {polys.K}, "
                         f"{polys.height} x {polys.width}")
    out = _masks_out(out, polys, who)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    _poly_lib.call("pswin_poly_masks", polys.xy, ptr(polys.xy), ptr(polys.part_offsets), ptr(polys.obj_offsets), ptr(polys.count),
                   polys.max_parts, polys.max_vertices, polys.B, polys.K, polys.height, polys.width, ptr(out), ptr(poly_workspace(polys)))
    return out


def polygons_to_masks(polys, out=None):
    """PolygonBatch -> uint8 [B, K, H, W] of 0 / 1, every byte written, zeros in the rows past count[b].  HIP tensors: pswin_poly_masks
    of libpswin_poly_hip.so (two launches, no atomics, no host synchronisation: capturable; the bit-planes live in one workspace per
    shape and device, written by a call before the call reads it; limits: poly_supported, beyond them PswinError); CPU tensors: the
    definition."""
    if isinstance(polys, PolygonBatch) and polys.xy.is_cuda:
        return _masks_hip(polys, out, "polygons_to_masks")
    return polygons_to_masks_definition(polys, out)


def polygons_to_rle(polys, capacity=None, out=None):
    """PolygonBatch -> RleMasks carrying B, K and count, with the overflow contract of rle.encode_masks: what PaddedTargets.rle holds
    for CocoAccumulator / MapAccumulator(iou="segm").  HIP tensors: pswin_poly_masks into a bitmap buffer kept per shape and device,
    then rle.encode_masks of it (six launches, capturable); CPU tensors: the definition."""
    if isinstance(polys, PolygonBatch) and polys.xy.is_cuda:
        _check_batch(polys, "polygons_to_rle")
        masks = _masks_hip(polys, _scratch(polys, "bitmaps", (polys.B, polys.K, polys.height, polys.width)), "polygons_to_rle")
        return _rle.encode_masks(masks, polys.count, capacity, out)
    return polygons_to_rle_definition(polys, capacity, out)
