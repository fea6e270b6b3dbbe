"""numpy restatement of pswin_pano_resize_crop_resize_normalize_pad (include/pswin.h), the checker of the device kernel: the two-stage
contract built on _pano_ref.resize_u8_f32, written from the header's statement."""
import numpy as np

import _pano_ref as R


def resize_crop_resize_u8(img, plan):
    """img uint8 [H, W, 3], plan (h1, w1, cy, cx, ch, cw, oh, ow) -> float32 [oh, ow, 3] holding integers, source channel order."""
    h1, w1, cy, cx, ch, cw, oh, ow = (int(v) for v in plan)
    if h1 == 0:
        return R.resize_u8_f32(img, oh, ow)
    inter = R.resize_u8_f32(img, h1, w1).astype(np.uint8)
    crop = inter[cy:cy + ch, cx:cx + cw]
    assert crop.shape[:2] == (ch, cw), "the plan's crop leaves the intermediate image"
    return R.resize_u8_f32(crop, oh, ow)                                        # clamps inside the crop


def normalize_pad(u, mean, inv_std, to_rgb, Hp, Wp):
    """float32 [oh, ow, 3] -> float32 [3, Hp, Wp]: channel swap, (u - mean) * inv_std in float32, zeros outside."""
    f = np.float32
    if to_rgb:
        u = u[..., ::-1]
    out = np.zeros((3, Hp, Wp), f)
    oh, ow = u.shape[:2]
    v = (u.astype(f) - np.asarray(mean, f)) * np.asarray(inv_std, f)
    out[:, :oh, :ow] = v.astype(f).transpose(2, 0, 1)
    return out


def batch(imgs, plans, norm6, to_rgb, Hp, Wp):
    """imgs uint8 [B, H, W, 3]; norm6 float32 [6] (mean, 1/std per output channel) -> float32 [B, 3, Hp, Wp]."""
    return np.stack([normalize_pad(resize_crop_resize_u8(im, p), norm6[:3], norm6[3:], to_rgb, Hp, Wp) for im, p in zip(imgs, plans)])
