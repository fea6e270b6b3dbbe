"""Cases for the polygon tests and a SECOND restatement of pycocotools' rleFrPoly, written independently of
panoswintransformerobjectdetection_amd/polygons.py (which follows the C code's point list, sort and zero-dropping loop).

The restatement works column by column.  An edge's points are a function t -> (u, v); column c has an event wherever two consecutive
points of ONE edge have u = 5 c + 2 and 5 c + 3 (pairs across two edges never count: they share u, or lie left of column 0).  The event's
row is ceil((min(v) - 2) / 5) in INTEGER arithmetic, clamped to [0, h] -- (m + 0.5) / 5 - 0.5 is (m - 2) / 5, and the double expression is
exact where that is an integer.  The mask is "toggle one bit at every event position x h + y, then take the prefix XOR in scan order",
and the counts are a plain loop over the scanned bits.  If pycocotools ever becomes available, this is where a pin attaches.

`defect=` plants one wrong reading of the rule (tests/test_polygons.py shows that the cases notice each)."""
import math

import numpy as np

DEFECTS = ("floor_for_trunc", "no_flip", "max_for_min", "floor_for_ceil", "clamp_h_minus_1", "keep_outside_columns", "xor_parts",
           "no_half_in_v", "row_major")
UNOBSERVABLE = ("gt_for_ge",)


def _edge_points(xs, ys, xe, ye, defect):
    """the points of one edge in the arithmetic's own order (the order does not matter to min(.)): integer arrays u, v"""
    rnd = np.floor if defect == "floor_for_trunc" else np.trunc
    dx, dy = abs(xe - xs), abs(ye - ys)
    x_major = dx > dy if defect == "gt_for_ge" else dx >= dy
    if x_major:
        if xs > xe and defect != "no_flip":
            xs, ys, xe, ye = xe, ye, xs, ys
        t = np.arange(dx + 1, dtype=np.float64)
        s = float(ye - ys) / dx
        half = 0.0 if defect == "no_half_in_v" else 0.5
        return (xs + t).astype(np.int64), rnd(ys + s * t + half).astype(np.int64)
    if ys > ye and defect != "no_flip":
        xs, ys, xe, ye = xe, ye, xs, ys
    t = np.arange(dy + 1, dtype=np.float64)
    s = float(xe - xs) / dy
    return rnd(xs + s * t + 0.5).astype(np.int64), (ys + t).astype(np.int64)


def column_events(xy, h, w, defect=None):
    """per column c (a dict; columns outside the image too) the list of event rows 0 .. h of one part"""
    rnd = math.floor if defect == "floor_for_trunc" else math.trunc
    a = [float(z) for z in xy]
    k = len(a) // 2
    X = [rnd(5.0 * a[2 * j] + 0.5) for j in range(k)]
    Y = [rnd(5.0 * a[2 * j + 1] + 0.5) for j in range(k)]
    out = {}
    for j in range(k):
        xs, ys, xe, ye = X[j], Y[j], X[(j + 1) % k], Y[(j + 1) % k]
        if xs == xe:
            continue                                                            # u is constant along the edge (zero-length edges too)
        u, v = _edge_points(xs, ys, xe, ye, defect)
        lo = np.minimum(u[1:], u[:-1])
        step = np.flatnonzero((u[1:] != u[:-1]) & ((lo - 2) % 5 == 0))
        for i in step:
            c = int(lo[i] - 2) // 5
            pick = max if defect == "max_for_min" else min
            m = int(pick(v[i], v[i + 1])) - 2
            y = m // 5 if defect == "floor_for_ceil" else -((-m) // 5)
            y = max(0, min(y, h - 1 if defect == "clamp_h_minus_1" else h))
            out.setdefault(c, []).append(y)
    return out


def part_mask(xy, h, w, defect=None):
    """uint8 [h, w]: toggle at the event positions, prefix XOR in scan order"""
    toggles = np.zeros(h * w + 1 + (h if defect == "keep_outside_columns" else 0), dtype=bool)
    for c, rows in column_events(xy, h, w, defect).items():
        if defect == "keep_outside_columns":
            c = min(max(c, 0), w)                                               # an event left or right of the image lands on its rim
        elif c < 0 or c > w - 1:
            continue
        for y in rows:
            p = y * w + c if defect == "row_major" and y < h else c * h + y
            toggles[p] ^= True
    filled = np.logical_xor.accumulate(toggles[:h * w])
    if defect == "row_major":
        return np.ascontiguousarray(filled.reshape(h, w)).astype(np.uint8)
    return np.ascontiguousarray(filled.reshape(w, h).T).astype(np.uint8)


def loop_encode(mask):
    """counts of a [h, w] mask, column-major, as a list of ints"""
    h, w = mask.shape
    counts, run, cur = [], 0, 0
    for x in range(w):
        for y in range(h):
            if int(mask[y, x] != 0) != cur:
                counts.append(run)
                run, cur = 0, 1 - cur
            run += 1
    counts.append(run)
    return counts


def restated_counts(xy, h, w, defect=None):
    return loop_encode(part_mask(xy, h, w, defect))


def restated_object_mask(parts, h, w, defect=None):
    m = np.zeros((h, w), dtype=np.uint8)
    for p in parts:
        m = (m ^ part_mask(p, h, w, defect)) if defect == "xor_parts" else (m | part_mask(p, h, w, defect))
    return m


# ---- named cases: (name, object = list of parts, h, w) ---------------------------------------------------------------------------
def star(n, cx, cy, r_out, r_in, phase=0.0):
    """a star polygon of n vertices (n edges), alternating radii"""
    out = []
    for i in range(n):
        r = r_out if i % 2 == 0 else r_in
        a = phase + 2.0 * math.pi * i / n
        out += [cx + r * math.cos(a), cy + r * math.sin(a)]
    return out


HAND = [
    ([1, 1, 4, 1, 4, 4, 1, 4], 6, 6, [7, 3, 3, 3, 3, 3, 14]),
    ([0.5, 0.5, 3.5, 0.5, 3.5, 3.5, 0.5, 3.5], 5, 5, [6, 3, 2, 3, 2, 3, 6]),
    ([2, 0, 4, 4, 0, 4], 5, 5, [3, 1, 2, 3, 2, 3, 4, 1, 6]),
]

NAMED = [
    ("hand_square", [[1, 1, 4, 1, 4, 4, 1, 4]], 6, 6),
    ("hand_half_square", [[0.5, 0.5, 3.5, 0.5, 3.5, 3.5, 0.5, 3.5]], 5, 5),
    ("hand_triangle", [[2, 0, 4, 4, 0, 4]], 5, 5),
    ("negative_trunc_not_floor", [[-0.25, -0.25, 6.3, -0.12, 6.7, 5.9, -0.3, 7.1]], 9, 8),
    ("negative_slope_from_outside", [[-2.26, 1.3, 5.1, 0.4, 7.3, 6.2, -1.14, 7.9]], 9, 8),
    ("wholly_left", [[-9, 1, -2, 1, -2, 6, -9, 6]], 8, 8),
    ("wholly_right", [[12, 1, 19, 1, 19, 6, 12, 6]], 8, 8),
    ("wholly_above", [[1, -9, 6, -9, 6, -2, 1, -2]], 8, 8),
    ("wholly_below", [[1, 11, 6, 11, 6, 17, 1, 17]], 8, 8),
    ("covers_everything", [[-3, -3, 11, -3, 11, 12, -3, 12]], 8, 8),
    ("clamp_to_0_and_h", [[2, -4, 6, -4, 6, 13, 2, 13]], 8, 8),
    ("wrap_into_next_column", [[1.5, 3, 4.5, 3, 4.5, 30, 1.5, 30]], 7, 6),
    ("wrap_at_last_column", [[3.5, 2, 9, 2, 9, 30, 3.5, 30]], 7, 6),
    ("bottom_row_only", [[0, 6.6, 6, 6.6, 6, 9, 0, 9]], 7, 6),
    ("repeated_vertices", [[1, 1, 1, 1, 5, 1, 5, 1, 5, 1, 5, 6, 1, 6, 1, 6]], 8, 8),
    ("repeated_first_last", [[1, 1, 5, 2, 3, 6, 1, 1]], 8, 8),
    ("dx_equals_dy", [[1, 1, 6, 6, 1, 6]], 8, 8),
    ("dx_equals_dy_other_way", [[6, 1, 1, 6, 6, 6]], 8, 8),
    ("diamond", [[4, 0.4, 7.6, 4, 4, 7.6, 0.4, 4]], 8, 8),
    ("horizontal_and_vertical", [[0.6, 2.2, 7.4, 2.2, 7.4, 5.8, 0.6, 5.8]], 8, 8),
    ("flip_x_major", [[7, 1, 1, 2.6, 2, 6.2, 7.4, 5]], 8, 8),
    ("flip_y_major", [[2, 7, 3.4, 1, 6.2, 0.6, 5, 7.4]], 8, 8),
    ("clockwise", [[1, 1, 1, 6.4, 6.4, 6.4, 6.4, 1]], 8, 8),
    ("bow_tie", [[1, 1, 7, 7, 7, 1, 1, 7]], 8, 8),
    ("collinear", [[1, 1, 4, 4, 7, 7]], 8, 8),
    ("collinear_horizontal", [[1, 3, 4, 3, 7, 3]], 8, 8),
    ("k3_sliver", [[0.2, 0.3, 7.7, 3.1, 0.9, 3.9]], 8, 8),
    ("steep_sliver", [[3.1, -2.0, 3.9, 20.0, 4.6, -1.0]], 16, 8),
    ("one_pixel_image", [[-1, -1, 2, -1, 2, 2, -1, 2]], 1, 1),
    ("one_row", [[0.4, -2, 11.6, -2, 11.6, 3, 0.4, 3]], 1, 13),
    ("one_column", [[-1, 2.4, 3, 2.4, 3, 9.6, -1, 9.6]], 13, 1),
    ("shared_events_cancel", [[1, 1, 4, 1, 4, 5, 1, 5], [4, 1, 7, 1, 7, 5, 4, 5]], 8, 8),
    ("same_part_twice", [[1, 1, 6, 1, 6, 6, 1, 6], [1, 1, 6, 1, 6, 6, 1, 6]], 8, 8),
    ("parts_disjoint", [[0, 0, 3, 0, 3, 3, 0, 3], [5, 5, 8, 5, 8, 8, 5, 8]], 9, 9),
    ("parts_nested", [[0, 0, 8, 0, 8, 8, 0, 8], [2, 2, 6, 2, 6, 6, 2, 6]], 9, 9),
    ("parts_overlapping", [[0, 0, 5, 0, 5, 5, 0, 5], [3, 3, 8, 3, 8, 8, 3, 8]], 9, 9),
    ("five_parts", [[0, 0, 3, 0, 3, 3, 0, 3], [2, 2, 6, 2, 6, 6, 2, 6], [5, 0.5, 9, 1, 7, 4], [1, 6, 4, 9, 0.5, 9.5],
                    [8, 8, 3, 8.4, 8.6, 4.2]], 10, 10),
]
NAMED_BY_NAME = {name: (parts, h, w) for name, parts, h, w in NAMED}


# ---- seeded random polygons: (family, xy, h, w) ------------------------------------------------------------------------------------
RANDOM_H = (1, 3, 7, 20, 64, 65)
RANDOM_W = (1, 2, 5, 17, 33)
FAMILIES = ("real", "integer", "grid")


def random_polygons(n, seed=0):
    """n polygons, the three families in turn; every family reaches 3 pixels outside the image on every side"""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        fam = FAMILIES[i % 3]
        h, w = RANDOM_H[rng.randint(len(RANDOM_H))], RANDOM_W[rng.randint(len(RANDOM_W))]
        k = int(rng.randint(3, 9))
        if fam == "real":
            x, y = rng.uniform(-3, w + 3, k), rng.uniform(-3, h + 3, k)
        elif fam == "integer":
            x, y = rng.randint(-3, w + 4, k).astype(np.float64), rng.randint(-3, h + 4, k).astype(np.float64)
        else:
            x, y = rng.randint(-15, 5 * (w + 3) + 1, k) / 5.0, rng.randint(-15, 5 * (h + 3) + 1, k) / 5.0
            shift = np.array([0.0, 0.1, 0.5, -0.1])
            x, y = x + shift[rng.randint(4, size=k)], y + shift[rng.randint(4, size=k)]
        out.append((fam, np.stack([x, y], 1).reshape(-1).tolist(), h, w))
    return out
