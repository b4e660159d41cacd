"""Generate tests/golden/color_jitter.npz: the reference's own training input with INPUT.COLOR_JITTER True run on CPU --
DatasetMapperIgnore (crop -> ColorJitterPIL -> resize -> flip) and DatasetMapperMosaic (the same on the painted composite).  Runs
only where the reference tree exists; only data goes into the fixture.  TEST INFRASTRUCTURE ONLY.

The reference's ColorJitterPIL is `torchvision.transforms.ColorJitter` on a PIL image, and this image has no torchvision.  As
make_golden_train_input.py does for fvcore, the piece is installed from its published source: `ColorJitter` below is torchvision
0.8.2's (the version the reference's README pins) -- `forward` draws `torch.randperm(4)` and, walking the permutation, one
`torch.tensor(1.0).uniform_(lo, hi).item()` per step at the moment the step is reached -- over functional_pil's adjust_brightness /
contrast / saturation (Pillow's ImageEnhance) and adjust_hue (convert("HSV"), an 8-bit shift of H, convert back).  It must be in
place before detectron2.data is imported (augmentation_impl.py binds the name at import).  The instance also remembers its last draw,
which goes into the fixture.

Consumers: tests/test_host_color_jitter.py, tests/test_gpu_color_jitter.py.

  per case cK_*: as train_input_*.npz (plain cases) or train_mosaic.npz (mosaic cases: tiles tT_*, canvas / source / trim,
      fill_in_window), plus torch_seed, jitter_ops (the step ids in the order applied: 0 brightness, 1 contrast, 2 saturation, 3 hue)
      and jitter_factors (float64 holding the fp32 draws).  The numpy seed (crop, size, flip) is searched as in those scripts, the
      torch seed is 1000 + the numpy seed; each case's name says what the pair shows, and the script asserts it.

    python scripts/make_golden_color_jitter.py
"""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import refshim  # noqa: E402

refshim.install()

LAST = {}      # the last draw of the installed ColorJitter


def _install_color_jitter():
    import numbers

    import torchvision.transforms as tvt
    from PIL import Image, ImageEnhance

    def adjust_hue(img, hue_factor):
        if not (-0.5 <= hue_factor <= 0.5):
            raise ValueError("hue_factor ({}) is not in [-0.5, 0.5].".format(hue_factor))
        input_mode = img.mode
        if input_mode in {"L", "1", "I", "F"}:
            return img
        h, s, v = img.convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        # 0.8.2 adds np.uint8(hue_factor * 255) under errstate(over="ignore"): the C cast of a negative double, which wraps on the
        # hosts the reference ran on; spelled out so that a newer numpy cannot refuse it
        shift = int(hue_factor * 255) % 256
        with np.errstate(over="ignore"):
            np_h += np.uint8(shift)
        h = Image.fromarray(np_h, "L")
        return Image.merge("HSV", (h, s, v)).convert(input_mode)

    class ColorJitter(torch.nn.Module):
        def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
            super().__init__()
            self.brightness = self._check_input(brightness, "brightness")
            self.contrast = self._check_input(contrast, "contrast")
            self.saturation = self._check_input(saturation, "saturation")
            self.hue = self._check_input(hue, "hue", center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)

        @torch.jit.unused
        def _check_input(self, value, name, center=1, bound=(0, float("inf")), clip_first_on_zero=True):
            if isinstance(value, numbers.Number):
                if value < 0:
                    raise ValueError("If {} is a single number, it must be non negative.".format(name))
                value = [center - float(value), center + float(value)]
                if clip_first_on_zero:
                    value[0] = max(value[0], 0.0)
            elif isinstance(value, (tuple, list)) and len(value) == 2:
                if not bound[0] <= value[0] <= value[1] <= bound[1]:
                    raise ValueError("{} values should be between {}".format(name, bound))
            else:
                raise TypeError("{} should be a single number or a list/tuple with length 2.".format(name))
            if value[0] == value[1] == center:
                value = None
            return value

        def forward(self, img):
            fn_idx = torch.randperm(4)
            ops, factors = [], []
            for fn_id in fn_idx:
                if fn_id == 0 and self.brightness is not None:
                    brightness = self.brightness
                    brightness_factor = torch.tensor(1.0).uniform_(brightness[0], brightness[1]).item()
                    img = ImageEnhance.Brightness(img).enhance(brightness_factor)
                    ops.append(0), factors.append(brightness_factor)
                if fn_id == 1 and self.contrast is not None:
                    contrast = self.contrast
                    contrast_factor = torch.tensor(1.0).uniform_(contrast[0], contrast[1]).item()
                    img = ImageEnhance.Contrast(img).enhance(contrast_factor)
                    ops.append(1), factors.append(contrast_factor)
                if fn_id == 2 and self.saturation is not None:
                    saturation = self.saturation
                    saturation_factor = torch.tensor(1.0).uniform_(saturation[0], saturation[1]).item()
                    img = ImageEnhance.Color(img).enhance(saturation_factor)
                    ops.append(2), factors.append(saturation_factor)
                if fn_id == 3 and self.hue is not None:
                    hue = self.hue
                    hue_factor = torch.tensor(1.0).uniform_(hue[0], hue[1]).item()
                    img = adjust_hue(img, hue_factor)
                    ops.append(3), factors.append(hue_factor)
            LAST["ops"], LAST["factors"] = ops, factors
            return img

    tvt.ColorJitter = ColorJitter


_install_color_jitter()

import make_golden_train_input as base  # noqa: E402  (installs the other third-party pieces)
import make_golden_train_mosaic as mos  # noqa: E402

import detectron2.data.transforms.augmentation_impl as _impl  # noqa: E402
import torchvision.transforms as _tvt  # noqa: E402

assert _impl.ColorJitter is _tvt.ColorJitter and isinstance(_impl.ColorJitterPIL().aug, torch.nn.Module)

_plain_ref_cfg = base.ref_cfg


def ref_cfg(min_sizes, max_size, sampling, crop):
    cfg = _plain_ref_cfg(min_sizes, max_size, sampling, crop)
    cfg.defrost()
    cfg.INPUT.COLOR_JITTER = True
    cfg.freeze()
    return cfg


def torch_seed(seed):
    return 1000 + int(seed)


def drawn_params(mapper, image, seed):
    """base.drawn_params for a list that holds the jitter; leaves torch's generator seeded for the mapper call that follows."""
    from detectron2.data import transforms as T

    np.random.seed(seed)
    torch.manual_seed(torch_seed(seed))
    inp = T.StandardAugInput(image.copy())
    tfms = inp.apply_augmentations(mapper.augmentations)
    h, w = image.shape[:2]
    crop, size, flip, seen = (0, 0, w, h), (h, w), 0, []
    for t in tfms.transforms:
        n = type(t).__name__
        seen.append(n)
        if n == "CropTransform":
            crop, size = (int(t.x0), int(t.y0), int(t.w), int(t.h)), (int(t.h), int(t.w))
        elif n == "ResizeTransform":
            size = (int(t.new_h), int(t.new_w))
        elif n == "HFlipTransform":
            flip = 1
        elif n not in ("NoOpTransform", "PILColorTransform"):
            raise TypeError(n)
    order = [n for n in seen if n in ("CropTransform", "PILColorTransform", "ResizeTransform")]
    assert order in (["CropTransform", "PILColorTransform", "ResizeTransform"], ["PILColorTransform", "ResizeTransform"],
                     ["CropTransform", "PILColorTransform"], ["PILColorTransform"]), order      # behind the crop, before the resize
    torch.manual_seed(torch_seed(seed))
    return crop, size, flip


base.ref_cfg = mos.ref_cfg = ref_cfg
base.drawn_params = drawn_params


def hue_factor():
    return LAST["factors"][LAST["ops"].index(3)]


def record(d, k):
    p = "c%d_" % k
    d[p + "torch_seed"] = np.int64(torch_seed(int(d[p + "seed"])))
    d[p + "jitter_ops"] = np.array(LAST["ops"], np.int64)
    d[p + "jitter_factors"] = np.array(LAST["factors"], np.float64)
    assert sorted(LAST["ops"]) == [0, 1, 2, 3] and all(float(np.float32(f)) == f for f in LAST["factors"])
    print("          torch seed %d: steps %s factors %s" % (torch_seed(int(d[p + "seed"])), LAST["ops"], ["%.4f" % f for f in LAST["factors"]]))


def gen():
    from make_golden_train_input import XYXY, ann

    rng = np.random.default_rng(2026)
    boxes = [ann([4.3, 6.7, 30.2, 20.9], 3, id=11), ann([40.5, 5.25, 30.0, 40.5], 17, ignore=1, id=12),
             ann([10.0, 20.0, 65.5, 51.25], 5, mode=XYXY), ann([5.0, 5.0, 20.0, 20.0], 9, iscrowd=1, id=14)]
    rr = ("relative_range", (0.7, 0.7))
    plain = [
        ("contrast_first_hue_negative", (64, 80), boxes, (56,), 1333, "choice", rr,
         lambda c, s, f, n: LAST["ops"][0] == 1 and hue_factor() < 0),
        ("contrast_second_hue_positive_flip", (75, 100), boxes, (64,), 1333, "choice", rr,
         lambda c, s, f, n: LAST["ops"][1] == 1 and hue_factor() > 0 and f == 1),
        ("contrast_third_after_hue", (37, 53), boxes[:2], (40,), 1333, "choice", rr,
         lambda c, s, f, n: LAST["ops"][2] == 1 and LAST["ops"].index(3) < 2),
        ("contrast_last_noflip", (96, 120), boxes, (48, 64), 1333, "range", rr, lambda c, s, f, n: LAST["ops"][3] == 1 and f == 0),
        ("hue_first_bright", (53, 37), boxes[:2], (48,), 1333, "choice", ("absolute", (40, 30)),
         lambda c, s, f, n: LAST["ops"][0] == 3 and LAST["factors"][LAST["ops"].index(0)] > 1.25),
        ("saturation_first_dark_hue_negative", (120, 160), boxes, (64,), 100, "choice", ("relative", (0.5, 0.6)),
         lambda c, s, f, n: LAST["ops"][0] == 2 and LAST["factors"][LAST["ops"].index(0)] < 0.75 and hue_factor() < 0),
        ("nocrop_same_size", (48, 70), boxes[:3], (48,), 1333, "choice", None, lambda c, s, f, n: True),
    ]
    d = {}
    k = 0
    for c in plain:
        base.run_case(d, k, c[0], rng, *c[1:])
        d["c%d_n_tiles" % k] = np.int64(1)
        record(d, k)
        k += 1
    sizes4 = [(40, 56), (60, 30), (28, 64), (52, 44)]
    sizes9 = [(30, 42), (34, 60), (58, 22), (48, 36), (24, 46), (60, 60), (20, 31), (40, 52), (56, 20)]
    mosaics = [
        ("m4_fill_in_window_flip", sizes4, (64, 72), 1333, "choice", rr, lambda i: i["fill"] and i["flip"] == 1 and i["n"] > 0),
        ("m9_fill_in_window_contrast_first", sizes9, (96,), 1333, "choice", rr,
         lambda i: i["fill"] and i["n"] > 0 and LAST["ops"][0] == 1),
    ]
    for c in mosaics:
        mos.run_case(d, k, c[0], rng, c[1], mos.tile_anns(rng, c[1], 1000 * (k + 1)), *c[2:])
        assert int(d["c%d_fill_in_window" % k]) == 1
        record(d, k)
        k += 1
    d["n"] = np.int64(k)
    d["n_plain"] = np.int64(len(plain))
    ops = [d["c%d_jitter_ops" % i].tolist() for i in range(len(plain))]
    assert {o.index(1) for o in ops} == {0, 1, 2, 3}
    hues = [float(d["c%d_jitter_factors" % i][o.index(3)]) for i, o in enumerate(ops)]
    assert min(hues) < 0 < max(hues)
    base.save("color_jitter", d)


if __name__ == "__main__":
    gen()
