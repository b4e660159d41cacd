"""ResizeShortestEdge / ResizeTransform for uint8 images, on the device.

Mirrors the reference's test-time input transform (detectron2/data/transforms/augmentation_impl.py:184-234
`ResizeShortestEdge`, transform.py:83-134 `ResizeTransform`; built by `build_augmentation`, data/detection_utils.py:
563-595, from INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST).  `apply_image` of the reference hands a uint8 HWC array to Pillow's
`Image.resize(..., BILINEAR)`; here the same fixed-point resample runs as two HIP kernels (csrc/resize.hip) on a
device tensor, bit for bit, and can write straight into the detector's normalised, padded NHWC4 batch slot.

Only the host part of Pillow's algorithm lives here: the per-output coefficient table (Resample.c precompute_coeffs
+ normalize_coeffs_8bpc for the bilinear filter over the whole image), computed in float64 with the same operation
order as the C code and cached per (input size, output size).
"""
import collections
import functools
import math

import numpy as np
import torch

from .. import kernels as K

PRECISION_BITS = 32 - 8 - 2


@functools.lru_cache(maxsize=256)
def _coeffs_np(in_size, out_size):
    scale = float(np.float32(in_size) - np.float32(0.0)) / out_size     # Pillow keeps the box in float
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale                                         # bilinear: support 1
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xx = np.arange(out_size, dtype=np.float64)
    center = 0.0 + (xx + 0.5) * scale
    xmin = np.trunc(center - support + 0.5).astype(np.int64)
    xmin = np.maximum(xmin, 0)
    xmax = np.trunc(center + support + 0.5).astype(np.int64)
    xmax = np.minimum(xmax, in_size) - xmin
    k = np.zeros((out_size, ksize), np.float64)
    ww = np.zeros(out_size, np.float64)
    for x in range(ksize):                                              # ww accumulates tap by tap, as the C loop does
        v = np.abs(((x + xmin).astype(np.float64) - center + 0.5) * ss)
        w = np.where(v < 1.0, 1.0 - v, 0.0)
        w = np.where(x < xmax, w, 0.0)
        k[:, x] = w
        ww = ww + w
    nz = ww != 0.0
    k[nz] = k[nz] / ww[nz, None]
    p = k * float(1 << PRECISION_BITS)
    kk = np.where(k < 0, np.trunc(-0.5 + p), np.trunc(0.5 + p)).astype(np.int32)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    return bounds, kk, ksize


_DEV_COEFFS = collections.OrderedDict()
_DEV_COEFFS_MAX = 512       # (in, out, device) tables kept on the device: a dataset of many image sizes (x 9 under the default
                            # TEST.AUG) would otherwise grow this without bound; least recently used first out


def resample_coeffs(in_size, out_size, device=None):
    """(bounds [out,2] int32, coefficients [out,ksize] int32, ksize); on `device` when given (cached, bounded)."""
    b, k, ks = _coeffs_np(int(in_size), int(out_size))
    if device is None:
        return b, k, ks
    key = (int(in_size), int(out_size), str(device))
    hit = _DEV_COEFFS.get(key)
    if hit is None:
        hit = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), ks)
        _DEV_COEFFS[key] = hit
        while len(_DEV_COEFFS) > _DEV_COEFFS_MAX:     # an evicted table may still be read by a queued launch: the caching allocator
            _DEV_COEFFS.popitem(last=False)           # only hands its block to later work of the same stream
    else:
        _DEV_COEFFS.move_to_end(key)
    return hit


def _box_corners(box):
    """fvcore Transform.apply_box: the 4 corners of each box as [4N, 2] coordinates (a copy), for numpy arrays and tensors."""
    idxs = [0, 1, 2, 1, 0, 3, 2, 3]
    if isinstance(box, torch.Tensor):
        return box.reshape(-1, 4)[:, idxs].reshape(-1, 2).clone()
    return np.asarray(box).reshape(-1, 4)[:, idxs].reshape(-1, 2).copy()


def _corners_to_box(coords):
    c = coords.reshape(-1, 4, 2)
    if isinstance(c, torch.Tensor):
        return torch.cat([c.min(dim=1).values, c.max(dim=1).values], 1)
    return np.concatenate([c.min(axis=1), c.max(axis=1)], axis=1)


def _scale(col, factor):
    """col * factor in the column's own precision, the way numpy multiplies an fp32 array by a Python float (the factor is rounded
    to fp32 first)."""
    if isinstance(col, torch.Tensor):
        return col * torch.tensor(factor, dtype=col.dtype, device=col.device)
    return col * np.asarray(factor, dtype=col.dtype)


class NoOpTransform:
    """fvcore NoOpTransform: every apply_* returns its input."""

    def apply_image(self, img):
        return img

    def apply_coords(self, coords):
        return coords

    def apply_box(self, box):
        return box

    def inverse(self):
        return self


class HFlipTransform:
    """fvcore HFlipTransform(width): x -> width - x on coordinates (fp32 for fp32 input), the image mirrored along its width."""

    def __init__(self, width):
        self.width = int(width)

    def apply_image(self, img):
        """HWC (or NHWC) array / tensor mirrored along W, as fvcore does for numpy images."""
        if isinstance(img, torch.Tensor):
            return img.flip(1 if img.dim() <= 3 else -2)
        return np.flip(img, axis=1) if img.ndim <= 3 else np.flip(img, axis=-2)

    def apply_coords(self, coords):
        coords[:, 0] = self.width - coords[:, 0]
        return coords

    def apply_box(self, box):
        return _corners_to_box(self.apply_coords(_box_corners(box)))

    def inverse(self):
        return self


class TransformList:
    """fvcore TransformList: a flat sequence of transforms; `apply_*` runs them in order (each transform's own apply_box, so every
    step maps corners and takes min / max), `inverse` is the reversed list of inverses, `+` concatenates."""

    def __init__(self, transforms):
        flat = []
        for t in transforms:
            flat.extend(t.transforms if isinstance(t, TransformList) else [t])
        self.transforms = flat

    def _apply(self, x, meth):
        for t in self.transforms:
            x = getattr(t, meth)(x)
        return x

    def apply_image(self, img):
        return self._apply(img, "apply_image")

    def apply_coords(self, coords):
        return self._apply(coords, "apply_coords")

    def apply_box(self, box):
        return self._apply(box, "apply_box")

    def __add__(self, other):
        return TransformList(self.transforms + (other.transforms if isinstance(other, TransformList) else [other]))

    def __radd__(self, other):
        return TransformList((other.transforms if isinstance(other, TransformList) else [other]) + self.transforms)

    def __len__(self):
        return len(self.transforms)

    def inverse(self):
        return TransformList([t.inverse() for t in self.transforms[::-1]])


class ResizeTransform:
    """reference transform.py:83-134 for uint8 images and coordinates."""

    def __init__(self, h, w, new_h, new_w, interp=None):
        if interp not in (None, 2, "bilinear"):     # PIL.Image.BILINEAR == 2
            raise NotImplementedError("only the bilinear resize of the shipped configs is implemented")
        self.h, self.w, self.new_h, self.new_w = int(h), int(w), int(new_h), int(new_w)

    def apply_image(self, img, out_slot=None, mean=None, std=None):
        """img: uint8 [H,W,3] tensor (moved to the device if it is not there).  Returns the resized uint8 [new_h,new_w,3]
        device tensor; with `out_slot` ([Hp,Wp,4] fp32 view of the batch) also writes (resized - mean) / std zero-padded
        into it (GeneralizedRCNN.preprocess_image fused in)."""
        assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3
        assert tuple(img.shape[:2]) == (self.h, self.w)
        return K.resize_bilinear_u8(img, self.new_h, self.new_w, resample_coeffs, out_slot=out_slot, mean=mean, std=std)

    def apply_coords(self, coords):
        coords[:, 0] = coords[:, 0] * (self.new_w * 1.0 / self.w)
        coords[:, 1] = coords[:, 1] * (self.new_h * 1.0 / self.h)
        return coords

    def apply_box(self, box):
        if not isinstance(box, torch.Tensor):     # numpy, as fvcore: corners through apply_coords, then min / max
            coords = _box_corners(box)
            coords[:, 0] = _scale(coords[:, 0], self.new_w * 1.0 / self.w)
            coords[:, 1] = _scale(coords[:, 1], self.new_h * 1.0 / self.h)
            return _corners_to_box(coords)
        box = box.clone().reshape(-1, 4)
        box[:, 0::2] = box[:, 0::2] * (self.new_w * 1.0 / self.w)
        box[:, 1::2] = box[:, 1::2] * (self.new_h * 1.0 / self.h)
        return box

    def inverse(self):
        return ResizeTransform(self.new_h, self.new_w, self.h, self.w)


class ResizeShortestEdge:
    """reference augmentation_impl.py:184-234.  Test time uses sample_style "choice" with one length
    (detection_utils.py:577-581), so no random draw is involved on the path; "range" draws with numpy as the
    reference does."""

    def __init__(self, short_edge_length, max_size=2 ** 63 - 1, sample_style="range", interp=None):
        assert sample_style in ["range", "choice"], sample_style
        self.is_range = sample_style == "range"
        if isinstance(short_edge_length, int):
            short_edge_length = (short_edge_length, short_edge_length)
        if self.is_range:
            assert len(short_edge_length) == 2, "short_edge_length must be two values using 'range' sample style."
        self.short_edge_length, self.max_size, self.interp = tuple(short_edge_length), max_size, interp

    @classmethod
    def from_config(cls, cfg, is_train=False):
        """build_augmentation (detection_utils.py:563-595)."""
        I = cfg.INPUT
        if is_train:
            return cls(I.MIN_SIZE_TRAIN, I.MAX_SIZE_TRAIN, I.MIN_SIZE_TRAIN_SAMPLING)
        return cls(I.MIN_SIZE_TEST, I.MAX_SIZE_TEST, "choice")

    def output_size(self, h, w, size):
        scale = size * 1.0 / min(h, w)
        if h < w:
            newh, neww = size, scale * w
        else:
            newh, neww = scale * h, size
        if max(newh, neww) > self.max_size:
            scale = self.max_size * 1.0 / max(newh, neww)
            newh = newh * scale
            neww = neww * scale
        return int(newh + 0.5), int(neww + 0.5)

    def get_transform(self, img):
        h, w = int(img.shape[0]), int(img.shape[1])
        if self.is_range:
            size = np.random.randint(self.short_edge_length[0], self.short_edge_length[1] + 1)
        else:
            size = np.random.choice(self.short_edge_length)
        if size == 0:
            return None     # NoOpTransform
        newh, neww = self.output_size(h, w, int(size))
        return ResizeTransform(h, w, newh, neww, self.interp)


# ------------------------------------------------------------------------------------------------ training input
# RandomCrop -> ResizeShortestEdge -> RandomFlip: the training augmentation of the shipped yamls (reference DatasetMapperIgnore.
# from_config, lvc/data/dataset_mapper.py:90-126).  Only the POLICY lives here -- which window, which size, flip or not, and the
# matching coordinate transforms; the pixels of a whole batch are produced by one kernel call (csrc/train_input.hip).  Every random
# number comes from numpy's global generator through the reference's own calls in the reference's order, so `np.random.seed(s)`
# before a draw gives the reference's window, size and flip decision.


class CropTransform:
    """fvcore CropTransform(x0, y0, w, h): the window img[y0:y0+h, x0:x0+w]; coordinates shift by (-x0, -y0)."""

    def __init__(self, x0, y0, w, h, orig_w=None, orig_h=None):
        self.x0, self.y0, self.w, self.h = int(x0), int(y0), int(w), int(h)
        self.orig_w, self.orig_h = orig_w, orig_h      # fvcore keeps them for `inverse` only

    def apply_image(self, img):
        """HWC array / tensor: a view of the window, as fvcore's slicing."""
        return img[self.y0:self.y0 + self.h, self.x0:self.x0 + self.w]

    def apply_coords(self, coords):
        coords[:, 0] -= self.x0
        coords[:, 1] -= self.y0
        return coords

    def apply_box(self, box):
        return _corners_to_box(self.apply_coords(_box_corners(box)))


class _Shape:
    """What an augmentation policy needs of an image: its shape."""

    def __init__(self, h, w):
        self.shape = (int(h), int(w), 3)


class RandomCrop:
    """reference augmentation_impl.py:291-340, all four INPUT.CROP.TYPE values."""

    def __init__(self, crop_type, crop_size):
        assert crop_type in ["relative_range", "relative", "absolute", "absolute_range"], crop_type
        self.crop_type, self.crop_size = crop_type, tuple(crop_size)

    def get_transform(self, img):
        h, w = int(img.shape[0]), int(img.shape[1])
        croph, cropw = self.get_crop_size((h, w))
        assert h >= croph and w >= cropw, "Shape computation in {} has bugs.".format(self)
        h0 = np.random.randint(h - croph + 1)
        w0 = np.random.randint(w - cropw + 1)
        return CropTransform(w0, h0, cropw, croph)

    def get_crop_size(self, image_size):
        h, w = image_size
        if self.crop_type == "relative":
            ch, cw = self.crop_size
            return int(h * ch + 0.5), int(w * cw + 0.5)
        if self.crop_type == "relative_range":
            crop_size = np.asarray(self.crop_size, dtype=np.float32)
            ch, cw = crop_size + np.random.rand(2) * (1 - crop_size)
            return int(h * ch + 0.5), int(w * cw + 0.5)
        if self.crop_type == "absolute":
            return (min(self.crop_size[0], h), min(self.crop_size[1], w))
        assert self.crop_size[0] <= self.crop_size[1]      # absolute_range
        ch = np.random.randint(min(h, self.crop_size[0]), min(h, self.crop_size[1]) + 1)
        cw = np.random.randint(min(w, self.crop_size[0]), min(w, self.crop_size[1]) + 1)
        return ch, cw

    def __repr__(self):
        return "RandomCrop(crop_type={!r}, crop_size={!r})".format(self.crop_type, self.crop_size)


class RandomFlip:
    """reference augmentation_impl.py:91-120, horizontal flips (the only kind build_augmentation creates)."""

    def __init__(self, prob=0.5, *, horizontal=True, vertical=False):
        if horizontal and vertical:
            raise ValueError("Cannot do both horiz and vert. Please use two Flip instead.")
        if not horizontal and not vertical:
            raise ValueError("At least one of horiz or vert has to be True!")
        if vertical:
            raise NotImplementedError("RandomFlip(vertical=True): only the horizontal flip of the shipped configs is implemented")
        self.prob = prob

    def get_transform(self, img):
        w = int(img.shape[1])
        do = np.random.uniform(0, 1.0, []) < self.prob      # Augmentation._rand_range()
        return HFlipTransform(w) if do else NoOpTransform()


class PadTransform:
    """fvcore PadTransform(x0, y0, x1, y1, orig_w, orig_h, pad_value): `np.pad` of the image with the constant on its four sides
    (left, top, right, bottom); coordinates shift by (x0, y0)."""

    def __init__(self, x0, y0, x1, y1, orig_w=None, orig_h=None, pad_value=0):
        self.x0, self.y0, self.x1, self.y1 = int(x0), int(y0), int(x1), int(y1)
        self.orig_w, self.orig_h, self.pad_value = orig_w, orig_h, pad_value

    def apply_image(self, img):
        """HWC numpy array, as fvcore (the device path pads inside csrc/train_input.hip)."""
        padding = ((self.y0, self.y1), (self.x0, self.x1)) + (((0, 0),) if img.ndim == 3 else ())
        return np.pad(img, padding, mode="constant", constant_values=self.pad_value)

    def apply_coords(self, coords):
        coords[:, 0] += self.x0
        coords[:, 1] += self.y0
        return coords

    def apply_box(self, box):
        return _corners_to_box(self.apply_coords(_box_corners(box)))


class ResizeScale:
    """reference augmentation_impl.py:391-431: one `np.random.uniform(min_scale, max_scale)` draw s; the image is resized WHOLE by
    k = min(s * target_height / h, s * target_width / w) to round(h * k) x round(w * k), halves to even (`np.round`).  Float64
    scalars in that order of operations: the sizes are the reference's, bit for bit."""

    def __init__(self, min_scale, max_scale, target_height, target_width, interp=None):
        self.min_scale, self.max_scale = min_scale, max_scale
        self.target_height, self.target_width, self.interp = int(target_height), int(target_width), interp

    def get_transform(self, img):
        h, w = int(img.shape[0]), int(img.shape[1])
        s = float(np.random.uniform(self.min_scale, self.max_scale))
        k = min(self.target_height * s / h, self.target_width * s / w)
        return ResizeTransform(h, w, _round_half_even(h * k), _round_half_even(w * k), self.interp)

    def __repr__(self):
        return "ResizeScale(min_scale={}, max_scale={}, target_height={}, target_width={})".format(
            self.min_scale, self.max_scale, self.target_height, self.target_width)


def _round_half_even(x):
    """np.round of a float64 scalar as an int: Python's round is the same IEEE round-half-to-even."""
    return int(round(float(x)))


class FixedSizeCropTransform(TransformList):
    """What one draw of FixedSizeCrop decided: [CropTransform, PadTransform], with the numbers the batch kernel needs -- `window`
    (ox, oy, ow, oh) inside the image it was drawn for, `target` (th, tw) and the `fill` byte."""

    def __init__(self, crop, pad, window, target, fill):
        super().__init__([crop, pad])
        self.window, self.target, self.fill = tuple(int(v) for v in window), (int(target[0]), int(target[1])), int(fill)


class FixedSizeCrop:
    """reference augmentation_impl.py:123-161: ONE scalar `np.random.uniform(0, 1)` draw u for both axes; where the image is larger
    than crop_size (th, tw) the window starts at round(excess * u), halves to even, and where it is smaller the right and bottom
    are padded with pad_value up to crop_size."""

    def __init__(self, crop_size, pad_value=128.0):
        self.crop_size, self.pad_value = (int(crop_size[0]), int(crop_size[1])), pad_value
        if not (0 <= float(pad_value) <= 255 and float(pad_value) == int(pad_value)):      # np.pad writes it into a uint8 image
            raise ValueError("FixedSizeCrop: pad_value {} is not a uint8 value".format(pad_value))
        self.fill = int(pad_value)

    def get_transform(self, img):
        h, w = int(img.shape[0]), int(img.shape[1])
        th, tw = self.crop_size
        u = float(np.random.uniform(0.0, 1.0))
        oy, ox = _round_half_even(max(h - th, 0) * u), _round_half_even(max(w - tw, 0) * u)
        kept_h, kept_w = min(h, th), min(w, tw)      # what slicing leaves of a th x tw window at that offset
        crop = CropTransform(ox, oy, tw, th, w, h)
        pad = PadTransform(0, 0, tw - kept_w, th - kept_h, kept_w, kept_h, self.pad_value)
        return FixedSizeCropTransform(crop, pad, (ox, oy, kept_w, kept_h), (th, tw), self.fill)

    def __repr__(self):
        return "FixedSizeCrop(crop_size={}, pad_value={})".format(self.crop_size, self.pad_value)


class LargeScaleJitter:
    """INPUT.LSJ: the pair build_augmentation puts in ResizeShortestEdge's place (detection_utils.py:589-593) -- ResizeScale then
    FixedSizeCrop; the defaults are the reference's.  `augmentations()` -> the two policies, in order."""

    def __init__(self, min_scale=0.5, max_scale=1.6, target_height=800, target_width=800, pad_value=128.0):
        self.min_scale, self.max_scale, self.pad_value = min_scale, max_scale, pad_value
        self.target_height, self.target_width = int(target_height), int(target_width)
        self.resize = ResizeScale(min_scale, max_scale, target_height, target_width)
        self.crop = FixedSizeCrop((target_height, target_width), pad_value)

    def augmentations(self):
        return [self.resize, self.crop]

    def __repr__(self):
        return "LargeScaleJitter(min_scale={}, max_scale={}, target_height={}, target_width={}, pad_value={})".format(
            self.min_scale, self.max_scale, self.target_height, self.target_width, self.pad_value)


class ColorJitterTransform(NoOpTransform):
    """What one draw of ColorJitter decided: `ops`, the step ids in the order they are applied (0 brightness, 1 contrast, 2
    saturation, 3 hue), and `factors`, their fp32 factors as Python floats.  Coordinates and boxes pass unchanged; the pixels are
    csrc/color_jitter.hip's (`kernels.color_jitter_tiles_u8`), applied to the crop window in front of the resize."""

    def __init__(self, ops, factors):
        self.ops, self.factors = tuple(int(o) for o in ops), tuple(float(f) for f in factors)

    def apply_image(self, img):
        raise NotImplementedError("the colour jitter of an image is computed for a whole batch by kernels.color_jitter_tiles_u8")


class ColorJitter:
    """reference ColorJitterPIL (augmentation_impl.py:589-617): torchvision 0.8.2's `ColorJitter(brightness=0.4, contrast=0.4,
    saturation=0.4, hue=0.2)`, the version the reference pins.  The draws are that version's `forward`: `torch.randperm(4)`, then,
    walking the permutation, one `torch.tensor(1.0).uniform_(lo, hi).item()` per step AT THE MOMENT the step is reached -- so the
    order of the draws follows the permutation.  generator=None is torch's default CPU generator: `torch.manual_seed(s)` before a
    draw gives the reference's permutation and factors.  numpy's generator (crop, size, flip) is not touched."""

    def __init__(self, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.2, generator=None):
        self.ranges = [self._range(brightness, "brightness"), self._range(contrast, "contrast"), self._range(saturation, "saturation"),
                       self._range(hue, "hue", center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)]
        self.generator = generator

    @staticmethod
    def _range(value, name, center=1, bound=(0, float("inf")), clip_first_on_zero=True):
        """torchvision's ColorJitter._check_input: a number v means [center - v, center + v]; None where the step does nothing."""
        if isinstance(value, (int, float)):
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
        return None if value[0] == value[1] == center else (float(value[0]), float(value[1]))

    def get_transform(self, img):
        ops, factors = [], []
        for fn_id in torch.randperm(4, generator=self.generator).tolist():
            r = self.ranges[fn_id]
            if r is not None:
                ops.append(fn_id)
                factors.append(torch.tensor(1.0).uniform_(r[0], r[1], generator=self.generator).item())
        return ColorJitterTransform(ops, factors)

    def __repr__(self):
        return "ColorJitter(ranges={})".format(self.ranges)


class TrainInputParams:
    """What one draw of the training augmentations decided, as the integers the batch kernel needs: the crop window (x0, y0, w, h)
    in the source image (the whole image without a crop), the size after the resize, and the flip decision; `jitter`: None, or the
    (ops, factors) of a ColorJitter draw, applied to the crop window in front of the resize."""

    def __init__(self, h, w):
        self.crop = (0, 0, int(w), int(h))
        self.new_size = (int(h), int(w))
        self.flip = False
        self.jitter = None
        self.scaled = None      # with INPUT.LSJ: the (h, w) the crop window is resized to, WHOLE
        self.lsj = None         # and ((ox, oy, ow, oh), (th, tw), fill): the window of it that is kept, the canvas, the fill byte

    def lsj_item(self, tiles, window=None):
        """The job of kernels.train_input_lsj_u8 on `tiles` (default window: the crop; a jittered crop is its own whole window)."""
        return (tiles, tuple(self.crop if window is None else window), self.scaled) + self.lsj + (self.flip,)

    def crop_job(self):
        """The job of kernels.train_input_u8 on the jittered crop, a plain image of the window's size."""
        return (0, 0, self.crop[2], self.crop[3]) + self.new_size + (self.flip,)

    def job(self):
        return self.crop + self.new_size + (self.flip,)

    def __repr__(self):
        lsj = "" if self.lsj is None else ", scaled={}, lsj={}".format(self.scaled, self.lsj)
        return "TrainInputParams(crop={}, new_size={}, flip={}{})".format(self.crop, self.new_size, self.flip, lsj)


class AugmentationList:
    """AugInput.apply_augmentations (reference augmentation.py:212-245) for images known by their size alone: asks each policy in
    turn for its transform, handing the next one the size the previous transform leaves.  `draw(h, w)` -> (TransformList,
    TrainInputParams).  A crop is only understood in front of the resize and a flip behind it, a colour jitter between the crop and
    the resize (the order from_config builds); a LargeScaleJitter stands for its two policies, and its fixed-size crop is only
    understood between the resize and the flip."""

    def __init__(self, augmentations):
        self.augmentations = []
        for a in augmentations:
            self.augmentations.extend(a.augmentations() if isinstance(a, LargeScaleJitter) else [a])

    def draw(self, h, w):
        p = TrainInputParams(h, w)
        tfms = []
        for aug in self.augmentations:
            t = aug.get_transform(_Shape(h, w))
            if t is None:
                t = NoOpTransform()
            if isinstance(t, FixedSizeCropTransform):
                assert p.lsj is None and not p.flip, "the fixed-size crop comes once, behind the resize and in front of the flip"
                p.scaled, p.lsj, p.new_size = p.new_size, (t.window, t.target, t.fill), t.target
                h, w = t.target
            elif isinstance(t, CropTransform):
                assert (not tfms or all(isinstance(u, NoOpTransform) for u in tfms)) and p.jitter is None, "a crop must come first"
                p.crop = (t.x0, t.y0, t.w, t.h)
                p.new_size = (t.h, t.w)
                h, w = t.h, t.w
            elif isinstance(t, ResizeTransform):
                assert not p.flip and p.lsj is None, "a resize must come before the flip"
                p.new_size = (t.new_h, t.new_w)
                h, w = t.new_h, t.new_w
            elif isinstance(t, HFlipTransform):
                p.flip = not p.flip
            elif isinstance(t, ColorJitterTransform):
                assert p.jitter is None and not p.flip and p.new_size == (p.crop[3], p.crop[2]), \
                    "the colour jitter comes once, behind the crop and in front of the resize"
                p.jitter = (t.ops, t.factors)
            elif not isinstance(t, NoOpTransform):
                raise NotImplementedError("transform {} is not part of the device training input".format(type(t).__name__))
            tfms.append(t)
        return TransformList(tfms), p
