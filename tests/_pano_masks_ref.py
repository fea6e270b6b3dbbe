"""Checker of pswin_pano_masks and of pano_aug.transform_masks_one, written from the statement in include/pswin.h with explicit loops
over the nearest-neighbour rule, on top of _pano_ref.warp at C = 1.  Not a copy of the package's definition: that one indexes whole
planes with arrays and samples the stretch itself.

    out[r][y][x] = 0 outside oh x ow, else max over the sources a of rows[r] with 0 <= a < n_in of Wm[a][sy][sx]
    nn(d, n_in, n_out) = min(int(floor(d * (1.0 / (float(n_out) / float(n_in))))), n_in - 1)
    h1 == 0: sy = nn(y, H, oh), sx = nn(x, W, ow)
    h1 >  0: sy = nn(cy + nn(y, ch, oh), H, h1), sx = nn(cx + nn(x, cw, ow), W, w1)
    Wm[a] = _pano_ref.warp of the one-channel image (src[a] != 0)

The keyword arguments plant one defect each; the tests show that every one of them changes the result on their inputs."""
import math

import numpy as np

import _pano_ref as R


def nn(d, n_in, n_out):
    return min(int(math.floor(d * (1.0 / (float(n_out) / float(n_in))))), n_in - 1)


def nn_ratio(d, n_in, n_out):
    """DEFECT: n_in / n_out in the place of 1 / (n_out / n_in)."""
    return min(int(math.floor(d * (float(n_in) / float(n_out)))), n_in - 1)


def warped(plane, stretch, kx, ky, shift, flip, flip_first=False):
    img = (np.asarray(plane) != 0).astype(np.uint8)[:, :, None]
    if flip_first:                                               # DEFECT: flip before roll
        out = R.stretch(img, kx, ky) if stretch else img.copy()
        return np.ascontiguousarray(np.roll(out[:, ::-1] if flip else out, shift, axis=1))[:, :, 0]
    return R.warp(img, bool(stretch), kx, ky, int(shift), bool(flip))[:, :, 0]


def source_index(y, x, H, W, plan, nn=nn, crop_late=False):
    h1, w1, cy, cx, ch, cw, oh, ow = plan
    if h1 == 0:
        return nn(y, H, oh), nn(x, W, ow)
    if crop_late:                                                # DEFECT: the crop offset applied after the second resize
        return min(cy + nn(nn(y, ch, oh), H, h1), H - 1), min(cx + nn(nn(x, cw, ow), W, w1), W - 1)
    return nn(cy + nn(y, ch, oh), H, h1), nn(cx + nn(x, cw, ow), W, w1)


def masks(src, stretch, kx, ky, shift, flip, plan, rows, pad_hw, nn=nn, crop_late=False, flip_first=False, merge_and=False):
    src = np.asarray(src)
    n_in, H, W = src.shape
    plan = tuple(int(v) for v in plan)
    oh, ow = plan[6], plan[7]
    Wm = [warped(src[a], stretch, kx, ky, shift, flip, flip_first) for a in range(n_in)]
    out = np.zeros((len(rows), int(pad_hw[0]), int(pad_hw[1])), np.uint8)
    index = [[source_index(y, x, H, W, plan, nn, crop_late) for x in range(ow)] for y in range(oh)]
    for r, pair in enumerate(rows):
        srcs = [int(a) for a in pair if 0 <= int(a) < n_in]
        for y in range(oh):
            for x in range(ow):
                sy, sx = index[y][x]
                vals = [int(Wm[a][sy, sx]) for a in srcs]
                if vals:
                    out[r, y, x] = min(vals) if merge_and else max(vals)       # DEFECT (merge_and): the merge as AND
    return out


def blobs(n, H, W, seed):
    """n bitmaps uint8 [n, H, W]: a rectangle and an ellipse each, set bytes 1, 255 or 7, never empty and never full."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        y0, x0 = rng.randint(0, H // 2), rng.randint(0, W // 2)
        out[i, y0:y0 + rng.randint(2, H // 2), x0:x0 + rng.randint(2, W // 2)] = (1, 255, 7)[i % 3]
        cy, cx, ry, rx = rng.randint(H), rng.randint(W), rng.randint(2, H // 3 + 2), rng.randint(2, W // 3 + 2)
        out[i][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = (255, 1, 255)[i % 3]
        out[i, (3 * i) % H, (5 * i) % W] = 0
    return out


def sample_strict(plane, refy, refx):
    """DEFECT: `>` in the place of `>=` at a blend of exactly 0.5.  The taps and the sum are _pano_ref.bilinear_wrap_u8's."""
    p = (np.asarray(plane) != 0).astype(np.float64)
    y0, y1, wy0, wy1 = R._taps(refy, p.shape[0])
    x0, x1, wx0, wx1 = R._taps(refx, p.shape[1])
    t = 0.0 + p[y0, x0] * wy0 * wx0
    t = t + p[y0, x1] * wy0 * wx1
    t = t + p[y1, x0] * wy1 * wx0
    t = t + p[y1, x1] * wy1 * wx1
    return (t > 0.5).astype(np.uint8)
