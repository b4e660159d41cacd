"""Numpy mirror of the pixel arithmetic of colour jitter (csrc/color_jitter.hip): torchvision's ColorJitter on a PIL image is
Pillow's `convert("L")`, `Image.blend` (ImageEnhance), RGB <-> HSV conversion and an 8-bit hue shift.  Every form here is checked
against the installed Pillow where there is one (tests/test_host_color_jitter.py); on the GPU machine this module is the expected
value.  Channels are taken by POSITION (Pillow is handed the array as it is, whatever INPUT.FORMAT says).

Ops: 0 brightness, 1 contrast, 2 saturation, 3 hue (torchvision's ids)."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


def all_colours():
    """Every 8-bit colour once, as a [4096, 4096, 3] uint8 image (48 MB)."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], 1).astype(np.uint8).reshape(4096, 4096, 3)


def grey(img):
    """Pillow convert("L") of an RGB-mode image: [..., 3] uint8 -> [...] uint8."""
    c = img.astype(np.uint32)
    return ((c[..., 0] * 19595 + c[..., 1] * 38470 + c[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(in1, in2, f):
    """Image.blend(im1, im2, f): in1 + f * (in2 - in1) in fp32, clipped to [0, 255], truncated."""
    f = np.float32(f)
    a, b = np.asarray(in1).astype(np.float32), np.asarray(in2).astype(np.float32)
    t = a + f * (b - a)
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.uint8)


def mean_grey(img):
    """ImageEnhance.Contrast's grey level: int(mean(L) + 0.5), the mean a float64 division."""
    L = grey(img)
    return int(float(int(L.astype(np.int64).sum())) / float(L.size) + 0.5)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def saturation(img, f):
    return blend(grey(img)[..., None], img, f)


def contrast(img, f, m=None):
    m = mean_grey(img) if m is None else m
    return blend(np.full_like(img, m), img, f)


def rgb_to_hsv(img):
    c0, c1, c2 = (img[..., i].astype(np.int32) for i in range(3))
    mx, mn = np.maximum(np.maximum(c0, c1), c2), np.minimum(np.minimum(c0, c1), c2)
    grey_px = mx == mn
    cr = np.where(grey_px, 1, mx - mn).astype(np.float32)
    mxf = np.where(grey_px, 1, mx).astype(np.float32)
    s = cr / mxf
    rc, gc, bc = ((mx - c).astype(np.float32) / cr for c in (c0, c1, c2))
    h0 = bc - gc                                                                       # fp32
    h1 = ((2.0 + rc.astype(np.float64)) - bc.astype(np.float64)).astype(np.float32)     # fp64, rounded once
    h2 = ((4.0 + gc.astype(np.float64)) - rc.astype(np.float64)).astype(np.float32)
    h = np.where(c0 == mx, h0, np.where(c1 == mx, h1, h2))
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    H = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    S = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    H, S = np.where(grey_px, 0, H), np.where(grey_px, 0, S)
    return np.stack([H, S, mx], -1).astype(np.uint8)


def _round_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


def hsv_to_rgb(hsv):
    H, S, V = (hsv[..., i].astype(np.float64) for i in range(3))
    hf = H * 6.0 / 255.0
    i = np.floor(hf)
    f = (hf - i).astype(np.float32).astype(np.float64)
    fs = (S.astype(np.float32) / np.float32(255.0)).astype(np.float64)
    p = np.clip(_round_away(V * (1.0 - fs)), 0, 255)
    q = np.clip(_round_away(V * (1.0 - fs * f)), 0, 255)
    t = np.clip(_round_away(V * (1.0 - fs * (1.0 - f))), 0, 255)
    k = i.astype(np.int64) % 6
    table = [(V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)]
    out = np.empty(hsv.shape, np.uint8)
    for ch in range(3):
        out[..., ch] = np.select([k == j for j in range(6)], [table[j][ch] for j in range(6)]).astype(np.uint8)
    grey_px = hsv[..., 1] == 0
    out[grey_px] = hsv[..., 2][grey_px][:, None]
    return out


def hue_shift(f):
    """torchvision adjust_hue: np.uint8(hue_factor * 255), the product in float64, truncated toward zero, mod 256."""
    return int(float(f) * 255.0) % 256


def hue(img, f):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + hue_shift(f)).astype(np.uint8)      # 8-bit wrap-around
    return hsv_to_rgb(hsv)


def jitter(img, ops, factors):
    """The steps in the given order on a [H, W, 3] uint8 image; the contrast step blends with the mean grey of the image as the steps
    before it left it."""
    for op, f in zip(ops, factors):
        f = np.float32(f)
        img = (brightness, contrast, saturation, hue)[int(op)](img, f)
    return img
