"""Generate tests/golden/train_input_*.npz: the reference's own training input run on CPU -- DatasetMapperIgnore
(lvc/data/dataset_mapper.py:24-209: RandomCrop -> ResizeShortestEdge -> RandomFlip, annotations, filter_empty_instances) and
TrainingSampler + AspectRatioGroupedDataset (the order of images).  Runs only where the reference tree exists (as
oracle/make_golden.py); only data goes into the fixtures.  TEST INFRASTRUCTURE ONLY.

Consumers: tests/test_host_train_input.py, tests/test_gpu_train_input.py.

  train_input_nocrop.npz / train_input_crop.npz   per case cK_*: the input image (uint8 HWC, INPUT.FORMAT order), the annotation
      lists (bbox float64, bbox_mode, category_id, iscrowd, ignore_qe (-1: key absent), id (-1000: key absent)), the cfg values
      (min sizes, max size, sampling, crop enabled / type / size), the numpy seed, and the reference's outputs: image (uint8 CHW),
      gt_boxes fp32, gt_classes, gt_ignores, ids, and the transform parameters it drew: crop (x0, y0, w, h), new size (h, w), flip.
      The reference reads files: each image goes through a temporary PNG (lossless).  Seeds are searched (first of 0..399) so that
      each case shows what its name says (flip or not, a box dropped, nothing left, ...).
  train_input_order.npz   a toy dataset's widths / heights, the sampler seed, and for world sizes 1 and 2 the batches of indices
      that leave the reference's sampler + grouping (and its plain BatchSampler) while the first 3 x len(dataset) indices of each
      rank go in.

    python scripts/make_golden_train_input.py
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import refshim  # noqa: E402

refshim.install()
GOLD = os.path.join(ROOT, "tests", "golden")


def _install_third_party():
    """Third-party pieces the data path of the reference executes and this image lacks, from their published sources: fvcore's
    HFlipTransform / CropTransform / TransformList, and iopath's PathManager.open for local files.  Must run before anything under
    detectron2.data is imported (it binds these names at import)."""
    import fvcore.transforms.transform as fvt

    class HFlipTransform(fvt.Transform):
        def __init__(self, width):
            self.width = width

        def apply_image(self, img):
            return np.flip(img, axis=1) if img.ndim <= 3 else np.flip(img, axis=-2)

        def apply_coords(self, coords):
            coords[:, 0] = self.width - coords[:, 0]
            return coords

    class CropTransform(fvt.Transform):
        def __init__(self, x0, y0, w, h, orig_w=None, orig_h=None):
            self.x0, self.y0, self.w, self.h = x0, y0, w, h

        def apply_image(self, img):
            if len(img.shape) <= 3:
                return img[self.y0:self.y0 + self.h, self.x0:self.x0 + self.w]
            return img[..., self.y0:self.y0 + self.h, self.x0:self.x0 + self.w, :]

        def apply_coords(self, coords):
            coords[:, 0] -= self.x0
            coords[:, 1] -= self.y0
            return coords

    class TransformList(fvt.Transform):
        def __init__(self, transforms):
            flat = []
            for t in transforms:
                flat.extend(t.transforms if isinstance(t, TransformList) else [t])
            self.transforms = flat

        def _apply(self, x, meth):
            for t in self.transforms:
                x = getattr(t, meth)(x)
            return x

        def __getattribute__(self, name):
            if name.startswith("apply_"):
                return lambda x: self._apply(x, name)
            return super().__getattribute__(name)

    fvt.HFlipTransform, fvt.CropTransform, fvt.TransformList = HFlipTransform, CropTransform, TransformList
    import fvcore.transforms as fvts

    fvts.HFlipTransform, fvts.CropTransform, fvts.TransformList, fvts.NoOpTransform = (HFlipTransform, CropTransform, TransformList,
                                                                                      fvt.NoOpTransform)
    from detectron2.utils.file_io import PathManager

    PathManager.open = lambda path, mode="r", **kw: open(path, mode)


_install_third_party()

XYXY, XYWH = 0, 1


def ann(bbox, cat, mode=XYWH, iscrowd=None, ignore=None, id=None):
    return {"bbox": [float(v) for v in bbox], "mode": mode, "cat": cat, "iscrowd": iscrowd, "ignore": ignore, "id": id}


def ref_annotations(anns):
    from detectron2.structures import BoxMode

    out = []
    for a in anns:
        d = {"bbox": list(a["bbox"]), "bbox_mode": BoxMode(a["mode"]), "category_id": a["cat"]}
        if a["iscrowd"] is not None:
            d["iscrowd"] = a["iscrowd"]
        if a["ignore"] is not None:
            d["ignore_qe"] = a["ignore"]
        if a["id"] is not None:
            d["id"] = a["id"]
        out.append(d)
    return out


def ref_cfg(min_sizes, max_size, sampling, crop):
    from lvc.config import get_cfg

    cfg = get_cfg()
    opts = ["MODEL.DEVICE", "cpu", "INPUT.MIN_SIZE_TRAIN", tuple(min_sizes), "INPUT.MAX_SIZE_TRAIN", max_size,
            "INPUT.MIN_SIZE_TRAIN_SAMPLING", sampling]
    if crop is not None:
        opts += ["INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", crop[0], "INPUT.CROP.SIZE", list(crop[1])]
    cfg.merge_from_list(opts)
    cfg.freeze()
    return cfg


def drawn_params(mapper, image, seed):
    """The transforms the mapper will draw for this seed: the same augmentation list on the same image from the same seed."""
    from detectron2.data import transforms as T

    np.random.seed(seed)
    inp = T.StandardAugInput(image.copy())
    tfms = inp.apply_augmentations(mapper.augmentations)
    h, w = image.shape[:2]
    crop, size, flip = (0, 0, w, h), (h, w), 0
    for t in tfms.transforms:
        n = type(t).__name__
        if n == "CropTransform":
            crop, size = (int(t.x0), int(t.y0), int(t.w), int(t.h)), (int(t.h), int(t.w))
        elif n == "ResizeTransform":
            size = (int(t.new_h), int(t.new_w))
        elif n == "HFlipTransform":
            flip = 1
        elif n != "NoOpTransform":
            raise TypeError(n)
    return crop, size, flip


def run_case(d, k, name, rng, hw, anns, min_sizes, max_size, sampling, crop, want):
    """want(crop, size, flip, n_instances) -> bool: what the case must show; the first seed of 0..399 that shows it is used."""
    from PIL import Image

    from lvc.data.dataset_mapper import DatasetMapperIgnore

    h, w = hw
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)      # in INPUT.FORMAT (BGR) order
    mapper = DatasetMapperIgnore(ref_cfg(min_sizes, max_size, sampling, crop), True)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "image.png")
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(path)      # the file holds RGB
        dic = {"file_name": path, "height": h, "width": w, "image_id": k, "annotations": ref_annotations(anns)}
        for seed in range(400):
            params = drawn_params(mapper, img, seed)
            np.random.seed(seed)
            out = mapper(dic)
            if want(params[0], params[1], params[2], len(out["instances"])):
                break
        else:
            raise RuntimeError("no seed shows case " + name)
    inst = out["instances"]
    p = "c%d_" % k
    d[p + "name"] = np.array(name)
    d[p + "image"] = img
    d[p + "ann_bbox"] = np.array([a["bbox"] for a in anns], np.float64).reshape(-1, 4)
    d[p + "ann_mode"] = np.array([a["mode"] for a in anns], np.int64)
    d[p + "ann_cat"] = np.array([a["cat"] for a in anns], np.int64)
    d[p + "ann_iscrowd"] = np.array([-1 if a["iscrowd"] is None else a["iscrowd"] for a in anns], np.int64)
    d[p + "ann_ignore"] = np.array([-1 if a["ignore"] is None else a["ignore"] for a in anns], np.int64)
    d[p + "ann_id"] = np.array([-1000 if a["id"] is None else a["id"] for a in anns], np.int64)
    d[p + "min_sizes"] = np.array(min_sizes, np.int64)
    d[p + "max_size"] = np.int64(max_size)
    d[p + "sampling"] = np.array(sampling)
    d[p + "crop_enabled"] = np.int64(crop is not None)
    d[p + "crop_type"] = np.array(crop[0] if crop else "relative_range")
    d[p + "crop_size"] = np.array(crop[1] if crop else (0.9, 0.9), np.float64)
    d[p + "seed"] = np.int64(seed)
    d[p + "out_image"] = out["image"].numpy()
    d[p + "gt_boxes"] = inst.gt_boxes.tensor.numpy()
    d[p + "gt_classes"] = inst.gt_classes.numpy()
    d[p + "gt_ignores"] = inst.gt_ignores.numpy()
    d[p + "ids"] = inst.ids.numpy()
    d[p + "crop"] = np.array(params[0], np.int64)
    d[p + "new_size"] = np.array(params[1], np.int64)
    d[p + "flip"] = np.int64(params[2])
    assert tuple(out["image"].shape[1:]) == tuple(params[1]) and inst.gt_boxes.tensor.dtype == torch.float32
    print("  case %2d %-28s %s seed %3d crop %s -> %s flip %d, %d of %d annotations kept" %
          (k, name, hw, seed, params[0], params[1], params[2], len(inst), len(anns)))


def gen_cases():
    rng = np.random.default_rng(2024)
    base = [ann([12.3, 20.7, 50.2, 30.9], 3, id=11), ann([70.5, 5.25, 40.0, 60.5], 17, ignore=1, id=12),
            ann([30.0, 40.0, 95.5, 71.25], 5, mode=XYXY), ann([5.0, 5.0, 20.0, 20.0], 9, iscrowd=1, id=14),
            ann([100.2, 50.1, 30.3, 25.6], 0, iscrowd=0, ignore=0)]
    corner = [ann([1.5, 2.5, 14.0, 12.0], 2, id=3), ann([3.0, 1.0, 9.5, 10.5], 4, iscrowd=1)]
    nocrop = [
        ("nocrop_down_noflip", (120, 200), base, (64,), 1333, "choice", None, lambda c, s, f, n: f == 0),
        ("nocrop_up_flip", (60, 90), base[:2], (100,), 1333, "choice", None, lambda c, s, f, n: f == 1),
        ("nocrop_max_clamp", (80, 250), base, (100,), 200, "choice", None, lambda c, s, f, n: max(s) == 200),
        ("nocrop_choice_tuple", (110, 150), base, (64, 72, 80, 96), 1333, "choice", None, lambda c, s, f, n: min(s) not in (64, 96)),
        ("nocrop_range_flip", (150, 100), base[:3], (64, 96), 1333, "range", None, lambda c, s, f, n: f == 1 and min(s) not in (64, 96)),
        ("nocrop_same_size", (64, 100), base[:2], (64,), 1333, "choice", None, lambda c, s, f, n: f == 0),
        ("nocrop_no_annotations", (70, 90), [], (80,), 1333, "choice", None, lambda c, s, f, n: n == 0),
    ]
    crop = [
        ("crop_relative_range_flip", (120, 200), base, (80,), 1333, "choice", ("relative_range", (0.5, 0.5)),
         lambda c, s, f, n: f == 1 and 0 < n < 4),
        ("crop_relative_noflip", (130, 170), base, (100,), 120, "choice", ("relative", (0.5, 0.7)), lambda c, s, f, n: f == 0 and n < 4),
        ("crop_absolute_flip", (100, 160), base, (64, 80), 1333, "range", ("absolute", (50, 70)), lambda c, s, f, n: f == 1 and 0 < n < 4),
        ("crop_absolute_range_noflip", (140, 120), base, (96,), 1333, "choice", ("absolute_range", (40, 90)),
         lambda c, s, f, n: f == 0 and n > 0),
        ("crop_nothing_left", (100, 160), corner, (60,), 1333, "choice", ("absolute", (40, 40)), lambda c, s, f, n: n == 0),
        ("crop_larger_than_image", (60, 75), base[:2], (60,), 1333, "choice", ("absolute", (200, 200)), lambda c, s, f, n: f == 1),
    ]
    for fname, cases in (("train_input_nocrop", nocrop), ("train_input_crop", crop)):
        d = {"n": np.int64(len(cases))}
        for k, c in enumerate(cases):
            run_case(d, k, c[0], rng, *c[1:])
        save(fname, d)


def gen_order():
    from detectron2.data.common import AspectRatioGroupedDataset
    from detectron2.data.samplers import TrainingSampler

    rng = np.random.default_rng(5)
    N, seed, bs = 11, 7, 2
    wide = rng.integers(0, 2, N).astype(bool)
    width = np.where(wide, 200, 120).astype(np.int64)
    height = np.where(wide, 120, 200).astype(np.int64)
    width[3] = height[3] = 150      # square: w > h is false
    d = {"width": width, "height": height, "seed": np.int64(seed), "batch_size": np.int64(bs)}
    for world in (1, 2):
        for rank in range(world):
            for grouped in (1, 0):
                s = TrainingSampler(N, seed=seed)
                s._rank, s._world_size = rank, world
                it = iter(s)
                idx = [int(next(it)) for _ in range(3 * N)]
                rows = [{"index": i, "width": int(width[i]), "height": int(height[i])} for i in idx]
                if grouped:
                    batches = [[r["index"] for r in b] for b in AspectRatioGroupedDataset(rows, bs)]
                else:
                    sampler = torch.utils.data.sampler.BatchSampler(idx, bs, drop_last=True)
                    batches = [list(b) for b in sampler]
                d["w%d_r%d_g%d" % (world, rank, grouped)] = np.array(batches, np.int64)
                print("  order world %d rank %d grouped %d: %d batches" % (world, rank, grouped, len(batches)))
    save("train_input_order", d)


def save(name, d):
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **d)
    print("wrote %-32s %8.1f KB" % (name + ".npz", os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    gen_cases()
    gen_order()
