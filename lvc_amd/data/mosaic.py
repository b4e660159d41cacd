"""Mosaic training input (reference lvc/data/mosaic.py: `get_mosaic`, `get_mosaic9`, `MapDatasetMosaic`, `DatasetMapperMosaic`;
INPUT.MOSAIC / INPUT.MOSAIC49SPLIT), with the pixels on the device.

The reference pastes 4 or 9 images into a 2s x 2s / 3s x 3s canvas filled with 114 (s = the longer side of the FIRST image), trims
the canvas to the painted extent and hands the composite to the usual crop -> resize -> flip.  Here the same split as in
dataset_mapper.py: the host half computes the integer geometry (`mosaic4_layout` / `mosaic9_layout`), maps the annotations and draws
the augmentations on the composite's size; the pixels come from `kernels.train_input_tiles_u8` (csrc/train_input.hip), which reads
the tiles in place -- neither the canvas nor the composite is ever written to memory.  With a colour jitter (INPUT.COLOR_JITTER,
opted into with `color_jitter=True`) the jittered crop window of the canvas is written once (`kernels.color_jitter_tiles_u8`) and
`kernels.train_input_u8` resizes it as a plain image.

What is reproduced, quirks included:
  * s comes from tile 0 only, later tiles may be larger; source rectangles go through numpy's slice rules (an end past the image is
    clamped, a negative start wraps); a source whose shape differs from its canvas rectangle's raises ValueError, as the reference's
    assignment does (the reference would broadcast a 1-pixel-wide source; that is refused here too);
  * tiles are painted in order: where canvas rectangles overlap the later tile wins; what no tile covers is 114;
  * 4 tiles: a box has bbox[0] / bbox[1] shifted by the canvas origin (x1a, y1a) -- not by x1a - x1b -- whatever its bbox_mode, and
    is not clipped; 9 tiles: a box is read as x, y, w, h whatever its mode, clipped to the source rectangle, shifted by
    (x1a - x1b, y1a - y1b); both then lose the trim origin;
  * the output dict is the LAST tile's (its image_id, and its width / height, stale for the composite), the annotations of all tiles
    in tile order;
  * `MapDatasetMosaic` draws from Python's `random` module in the reference's order.
"""
import copy
import math
import random

import torch

from .. import kernels as K
from .dataset_mapper import MOSAIC_KEYS, DatasetMapper, _raw_of, jitter_item, mapped_instances, plain_tiles
from .transforms import TrainInputParams, resample_coeffs

FILL = 114      # the canvas colour, all three channels


class MosaicLayout:
    """Integer geometry of one mosaic.  Per tile: `canvas` (x1a, y1a, x2a, y2a) and `source` (x1b, y1b, x2b, y2b) as the reference
    computes them (the annotations use these), and what numpy's slice rules make of them for the pixels: `rect`, the canvas
    rectangle that is painted, and `origin` (x, y), where in the tile its first pixel is read.  `trim` (minx1, miny1, maxx2,
    maxy2): the part of the canvas that is kept (`trim_origin` after the slice rules); `size` (h, w) of the composite; `side`: the
    canvas is side x side."""

    def __init__(self, canvas, source, sizes, trim, side):
        self.canvas, self.source, self.trim, self.side = canvas, source, trim, side
        self.rect, self.origin = _resolve(canvas, source, sizes, side)
        ys, xs = slice(trim[1], trim[3]).indices(side), slice(trim[0], trim[2]).indices(side)
        self.trim_origin = (xs[0], ys[0])
        self.size = (max(0, ys[1] - ys[0]), max(0, xs[1] - xs[0]))


def _resolve(canvas, source, sizes, side):
    """numpy's `image_out[y1a:y2a, x1a:x2a] = img[y1b:y2b, x1b:x2b]` for every tile: the canvas rectangles and source origins after
    the slice rules; ValueError where the two shapes differ."""
    rects, origins = [], []
    for i, ((x1a, y1a, x2a, y2a), (x1b, y1b, x2b, y2b), (h, w)) in enumerate(zip(canvas, source, sizes)):
        cx, cy = slice(x1a, x2a).indices(side), slice(y1a, y2a).indices(side)
        sx, sy = slice(x1b, x2b).indices(w), slice(y1b, y2b).indices(h)
        cshape = (max(0, cy[1] - cy[0]), max(0, cx[1] - cx[0]))
        sshape = (max(0, sy[1] - sy[0]), max(0, sx[1] - sx[0]))
        if cshape != sshape:
            raise ValueError("mosaic tile {}: could not broadcast input array from shape {} into shape {} (tile sizes {})".format(
                i, sshape + (3,), cshape + (3,), list(sizes)))
        rects.append((cx[0], cy[0], cx[0] + cshape[1], cy[0] + cshape[0]))
        origins.append((sx[0], sy[0]))
    return rects, origins


def mosaic4_layout(sizes):
    """get_mosaic (mosaic.py:23-67) for tile sizes [(h, w)] * 4 -> MosaicLayout."""
    assert len(sizes) == 4
    sizes = [(int(h), int(w)) for h, w in sizes]
    s = max(sizes[0])
    yc = xc = s
    maxx2, minx1 = 0, 1000000000
    maxy2, miny1 = 0, 1000000000
    canvas, source = [], []
    for i, (h, w) in enumerate(sizes):
        if i == 0:      # top left
            x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
            x1b, y1b, x2b, y2b = w - (x2a - x1a), h - (y2a - y1a), w, h
        elif i == 1:    # top right
            x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
            x1b, y1b, x2b, y2b = 0, h - (y2a - y1a), min(w, x2a - x1a), h
        elif i == 2:    # bottom left
            x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
            x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, max(xc, w), min(y2a - y1a, h)
        else:           # bottom right
            x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
            x1b, y1b, x2b, y2b = 0, 0, min(w, x2a - x1a), min(y2a - y1a, h)
        if i in (0, 2):
            minx1 = min(minx1, x1a)
        if i in (0, 1):
            miny1 = min(miny1, y1a)
        if i in (1, 3):
            maxx2 = max(maxx2, x2a)
        if i in (2, 3):
            maxy2 = max(maxy2, y2a)
        canvas.append((x1a, y1a, x2a, y2a))
        source.append((x1b, y1b, x2b, y2b))
    return MosaicLayout(canvas, source, sizes, (minx1, miny1, maxx2, maxy2), 2 * s)


def mosaic9_layout(sizes):
    """get_mosaic9 (mosaic.py:70-129) for tile sizes [(h, w)] * 9 -> MosaicLayout."""
    assert len(sizes) == 9
    sizes = [(int(h), int(w)) for h, w in sizes]
    s = max(sizes[0])
    H = W = 3 * s
    yc = xc = (3 * s) // 2
    fl, ce = (lambda v: int(math.floor(v / 2))), (lambda v: int(math.ceil(v / 2)))
    ltrb, source = [], []
    for i, (h, w) in enumerate(sizes):
        if i == 0:
            x1a, y1a, x2a, y2a = xc - fl(w), yc - fl(h), xc + ce(w), yc + ce(h)
            x1b, y1b, x2b, y2b = 0, 0, w, h
        elif i == 1:    # top
            x1a, y1a, x2a, y2a = max(0, xc - fl(w)), max(0, ltrb[0][1] - h), min(W, xc + ce(w)), ltrb[0][1]
            x1b, y1b, x2b, y2b = w // 2 - fl(x2a - x1a), h - (y2a - y1a), w // 2 + ce(x2a - x1a), h
        elif i == 2:    # top left
            x1a, y1a, x2a, y2a = max(0, ltrb[1][0] - w), max(0, ltrb[1][3] - h), ltrb[1][0], ltrb[1][3]
            x1b, y1b, x2b, y2b = w - (x2a - x1a), h - (y2a - y1a), w, h
        elif i == 3:    # left
            x1a, y1a, x2a, y2a = max(0, ltrb[0][0] - w), ltrb[2][3], ltrb[0][0], min(ltrb[0][3], ltrb[2][3] + h)
            x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, w, y2a - y1a
        elif i == 4:    # bottom left
            x1a, y1a, x2a, y2a = max(0, ltrb[0][0] - w), ltrb[3][3], ltrb[0][0], min(H, ltrb[3][3] + h)
            x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, w, y2a - y1a
        elif i == 5:    # bottom
            x1a, y1a, x2a, y2a = ltrb[0][0], ltrb[0][3], min(W, ltrb[0][0] + w), min(H, ltrb[0][3] + h)
            x1b, y1b, x2b, y2b = 0, 0, x2a - x1a, y2a - y1a
        elif i == 6:    # bottom right: the reference bounds this x coordinate by the canvas HEIGHT
            x1a, y1a, x2a, y2a = ltrb[5][2], ltrb[0][3], min(H, ltrb[5][2] + w), min(H, ltrb[0][3] + h)
            x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, w, y2a - y1a
        elif i == 7:    # right
            x1a, y1a, x2a, y2a = ltrb[0][2], ltrb[2][3], min(W, ltrb[0][2] + w), min(ltrb[0][3], ltrb[2][3] + h)
            x1b, y1b, x2b, y2b = w - (x2a - x1a), h // 2 - fl(y2a - y1a), w, h // 2 + ce(y2a - y1a)
        else:           # top right
            x1a, y1a, x2a, y2a = ltrb[1][2], max(0, ltrb[1][3] - h), min(ltrb[1][2] + w, W), ltrb[1][3]
            x1b, y1b, x2b, y2b = w - (x2a - x1a), h - (y2a - y1a), w, h
        ltrb.append((x1a, y1a, x2a, y2a))
        source.append((x1b, y1b, x2b, y2b))
    x1s, y1s, x2s, y2s = zip(*ltrb)
    return MosaicLayout(ltrb, source, sizes, (min(x1s), min(y1s), max(x2s), max(y2s)), 3 * s)


def mosaic_layout(sizes):
    if len(sizes) == 4:
        return mosaic4_layout(sizes)
    if len(sizes) == 9:
        return mosaic9_layout(sizes)
    raise ValueError("a mosaic has 4 or 9 tiles, got {}".format(len(sizes)))


def compose(images, layout):
    """The composite as the reference builds it, in numpy on the host (tests, tools; the training path never builds it)."""
    import numpy as np

    out = np.full((layout.side, layout.side, 3), FILL, np.uint8)
    for img, (x1a, y1a, x2a, y2a), (x1b, y1b) in zip(images, layout.rect, layout.origin):
        out[y1a:y2a, x1a:x2a] = np.asarray(img)[y1b:y1b + (y2a - y1a), x1b:x1b + (x2a - x1a)]
    minx1, miny1, maxx2, maxy2 = layout.trim
    return out[miny1:maxy2, minx1:maxx2]


def mosaic_annotations(annotation_lists, layout):
    """The annotation list of the composite from the tiles' lists (copies; Python float / int arithmetic as the reference's)."""
    nine = len(annotation_lists) == 9
    minx1, miny1 = layout.trim[0], layout.trim[1]
    out = []
    for annos, (x1a, y1a, _, _), (x1b, y1b, x2b, y2b) in zip(annotation_lists, layout.canvas, layout.source):
        for a in annos:
            a = copy.deepcopy(a)
            if nine:
                x1, y1, w, h = a["bbox"]
                x2, y2 = x1 + w, y1 + h
                y2, x2 = min(y2, y2b), min(x2, x2b)
                y1, x1 = max(y1, y1b), max(x1, x1b)
                h, w = max(0.0, y2 - y1), max(0.0, x2 - x1)
                x1 += x1a - x1b
                y1 += y1a - y1b
                a["bbox"] = [x1, y1, w, h]
            else:
                a["bbox"] = list(a["bbox"])
                a["bbox"][0] += x1a
                a["bbox"][1] += y1a
            a["bbox"][0] -= minx1
            a["bbox"][1] -= miny1
            out.append(a)
    return out


class MosaicInputParams(TrainInputParams):
    """TrainInputParams of a composite (crop in the composite's coordinates) with the layout that places its tiles."""

    def __init__(self, h, w, layout=None):
        super().__init__(h, w)
        self.layout = layout

    def tiles_item(self, tiles):
        """The job of kernels.train_input_tiles_u8: the crop window moves into canvas coordinates by the trim origin."""
        x0, y0, cw, ch = self.crop
        tx, ty = self.layout.trim_origin
        return ([(t, r, o) for t, r, o in zip(tiles, self.layout.rect, self.layout.origin)], (x0 + tx, y0 + ty, cw, ch),
                self.new_size[0], self.new_size[1], self.flip)


def plain_tiles_item(raw, params):
    """A plain image as a one-tile job."""
    h, w = int(raw.shape[0]), int(raw.shape[1])
    return ([(raw, (0, 0, w, h), (0, 0))], tuple(params.crop), params.new_size[0], params.new_size[1], params.flip)


class DatasetMapperMosaic(DatasetMapper):
    """reference DatasetMapperMosaic: `mapper([dict] * 4 or 9)` -> the reference's dict ("image": uint8 CHW on the device,
    "normalized" as DatasetMapper.__call__).  `draw(list)` is the host half: (dict, tile images, MosaicInputParams)."""

    @classmethod
    def from_config(cls, cfg, is_train=True, *, color_jitter=None, lsj=None):
        return cls._from_config(cfg, is_train, allow=MOSAIC_KEYS, color_jitter=color_jitter, lsj=lsj)

    def draw(self, dataset_dicts):
        raws = [_raw_of(d) for d in dataset_dicts]
        dicts = [{k: v for k, v in d.items() if k != "raw"} for d in dataset_dicts]
        for d, raw in zip(dicts, raws):      # detection_utils.check_image_size on every tile
            h, w = int(raw.shape[0]), int(raw.shape[1])
            if "width" in d and "height" in d and (d["width"], d["height"]) != (w, h):
                raise ValueError("Mismatched image shape: got {}, expect {}".format((w, h), (d["width"], d["height"])))
            d.setdefault("width", w)
            d.setdefault("height", h)
        layout = mosaic_layout([(int(r.shape[0]), int(r.shape[1])) for r in raws])
        out = dict(dicts[-1])
        if "sem_seg_file_name" in out:
            raise NotImplementedError("sem_seg_file_name: semantic segmentation is not implemented by the device training input")
        annos = mosaic_annotations([d.get("annotations", []) for d in dicts], layout)
        h, w = layout.size
        transforms, drawn = self.augmentations.draw(h, w)
        params = MosaicInputParams(h, w, layout)
        params.crop, params.new_size, params.flip, params.jitter = drawn.crop, drawn.new_size, drawn.flip, drawn.jitter
        params.scaled, params.lsj = drawn.scaled, drawn.lsj
        out.pop("annotations", None)
        out["instances"] = mapped_instances(annos, transforms, params.new_size)
        return out, raws, params

    def __call__(self, dataset_dicts):
        d, raws, params = self.draw(dataset_dicts)
        tiles = [r.to(self.device, non_blocking=True) for r in raws]
        nh, nw = params.new_size
        slot = torch.empty(1, nh, nw, 4, dtype=torch.float32, device=self.device)
        item = params.tiles_item(tiles)
        if params.lsj is not None:      # the window of the painted canvas (or its jittered copy) through the large-scale jitter
            lsj_item = params.lsj_item(item[0], item[1])
            if params.jitter is not None:
                crop = K.color_jitter_tiles_u8([jitter_item(item[0], item[1], params)])[0]
                lsj_item = params.lsj_item(plain_tiles(crop), params.crop_job()[0:4])
            u8 = K.train_input_lsj_u8([lsj_item], slot, self.pixel_mean, self.pixel_std, resample_coeffs, want_u8=True)[0]
        elif params.jitter is not None:      # the jittered window of the painted canvas (114 fill included) is the image the resize reads
            crop = K.color_jitter_tiles_u8([jitter_item(item[0], item[1], params)])[0]
            u8 = K.train_input_u8([crop], [params.crop_job()], slot, self.pixel_mean, self.pixel_std, resample_coeffs, want_u8=True)[0]
        else:
            u8 = K.train_input_tiles_u8([item], slot, self.pixel_mean, self.pixel_std, resample_coeffs, want_u8=True)[0]
        d["image"] = u8.permute(2, 0, 1).contiguous()
        d["normalized"] = slot[0]
        return d


class MapDatasetMosaic:
    """reference MapDatasetMosaic (mosaic.py:132-169): item idx is, with probability INPUT.MOSAIC, a mosaic of idx and 3 (with
    probability INPUT.MOSAIC49SPLIT) or 8 other items drawn by `random.sample`, else the plain item.  The draws come from Python's
    `random` module in the reference's order; a dataset shorter than the sample raises ValueError, as `random.sample` does."""

    def __init__(self, dataset, map_func_mosaic, map_func, cfg):
        self._dataset, self._map_func_mosaic, self._map_func = dataset, map_func_mosaic, map_func
        self._mos, self._mos49 = cfg.INPUT.MOSAIC, cfg.INPUT.MOSAIC49SPLIT

    def __len__(self):
        return len(self._dataset)

    def draw_indices(self, idx):
        """The dataset indices of item idx's tiles: [idx] for a plain item."""
        idx = int(idx)
        if random.random() < self._mos:
            k = 3 if random.random() < self._mos49 else 8
            return [idx] + random.sample(range(len(self)), k=k)
        return [idx]

    def __getitem__(self, idx):
        idxs = self.draw_indices(idx)
        if len(idxs) > 1:
            return self._map_func_mosaic([self._dataset[i] for i in idxs])
        return self._map_func(self._dataset[idxs[0]])
