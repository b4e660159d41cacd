"""Generate tests/golden/tta_*.npz: the reference's test-time augmentation (detectron2/modeling/test_time_augmentation.py,
DatasetMapperTTA + GeneralizedRCNNWithTTA) run on CPU around the reference GeneralizedRCNN.  Runs only where the
reference tree exists (as oracle/make_golden.py).  Only outputs are stored; the inputs are regenerated in the tests from
their seeds and pinned by a checksum.  TEST INFRASTRUCTURE ONLY.

Contents (consumers: tests/test_host_tta.py, tests/test_gpu_tta.py), with the conditioned R50-FPN weights of the e2e fixtures and
fvcore's HFlipTransform / TransformList set on the import shim first:
  tta_small.npz    map*: DatasetMapperTTA on small uint8 inputs (a pre-transform, an unchanged axis, the MAX_SIZE clamp, FLIP
                   False); small_bs{3,2}_i{0,1}_*: 240x320 (height/width 480x640) and 352x200 with MIN_SIZES (200, 240, 320) and
                   flip, batch sizes 3 and 2 -- every augmentation's raw detections, the union after the inverse transforms
                   (before the merge's in-place clip), the merged Instances; crafted*: _merge_detections on crafted unions
  tta_default.npz  default_i0_*: the same for one 240x320 image at the default TEST.AUG

    python scripts/make_golden_tta.py            # about a minute on 8 cores (the default TEST.AUG case is most of it)
"""
import copy
import hashlib
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import make_golden as mg  # noqa: E402  (installs the import shim)


def _install_fvcore_transforms():
    """fvcore.transforms.transform (third-party) as published: HFlipTransform, TransformList and NoOpTransform.inverse.
    Must run before anything under detectron2.data is imported (it binds these names at import)."""
    import fvcore.transforms.transform as fvt

    class HFlipTransform(fvt.Transform):
        def __init__(self, width):
            self.width = width

        def apply_image(self, img):
            return np.flip(img, axis=1) if img.ndim <= 3 else np.flip(img, axis=-2)

        def apply_coords(self, coords):
            coords[:, 0] = self.width - coords[:, 0]
            return coords

        def inverse(self):
            return self

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

        def __add__(self, other):
            others = other.transforms if isinstance(other, TransformList) else [other]
            return TransformList(self.transforms + others)

        def __radd__(self, other):
            others = other.transforms if isinstance(other, TransformList) else [other]
            return TransformList(others + self.transforms)

        def inverse(self):
            return TransformList([t.inverse() for t in self.transforms[::-1]])

    fvt.HFlipTransform = HFlipTransform
    fvt.TransformList = TransformList
    fvt.NoOpTransform.inverse = lambda self: self
    import fvcore.transforms as fvts

    fvts.HFlipTransform, fvts.TransformList, fvts.NoOpTransform = HFlipTransform, TransformList, fvt.NoOpTransform


_install_fvcore_transforms()

from lvc_amd.utils import synthetic as syn  # noqa: E402


def uint8_image(seed, h, w):
    return syn.synthetic_image(seed, h, w).round().clamp(0, 255).to(torch.uint8)


def checksum(t):
    return hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).hexdigest()


def tfm_rows(tfms):
    """Each transform of a TransformList as a row (kind, a, b, c, d): 0 no-op, 1 resize (h, w, new_h, new_w), 2 hflip (width)."""
    rows = []
    for t in tfms.transforms:
        n = type(t).__name__
        if n == "NoOpTransform":
            rows.append([0, 0, 0, 0, 0])
        elif n == "ResizeTransform":
            rows.append([1, t.h, t.w, t.new_h, t.new_w])
        elif n == "HFlipTransform":
            rows.append([2, t.width, 0, 0, 0])
        else:
            raise TypeError(n)
    return np.array(rows, np.int64)


def tta_cfg(cfg, min_sizes, max_size, flip):
    c = cfg.clone()
    c.defrost()
    c.TEST.AUG.MIN_SIZES = tuple(min_sizes)
    c.TEST.AUG.MAX_SIZE = max_size
    c.TEST.AUG.FLIP = flip
    c.freeze()
    return c


def gen_mapper(cfg, d):
    """(a) DatasetMapperTTA on small uint8 inputs: a pre-transform, an unchanged axis, the MAX_SIZE clamp, FLIP False."""
    from detectron2.modeling.test_time_augmentation import DatasetMapperTTA

    rng = np.random.default_rng(11)
    cases = [((20, 200), (20, 200), (21, 10), 201, True),      # (20, 201): height unchanged, width resampled; 10 -> down-scale
             ((37, 53), (74, 106), (24, 37, 64), 1000, False),  # pre_tfm; 37 leaves both axes unchanged; no flip
             ((60, 45), (60, 45), (30, 90), 100, True)]         # portrait; 90 clamped by MAX_SIZE
    for i, ((h, w), (oh, ow), mins, mx, flip) in enumerate(cases):
        img = torch.from_numpy(rng.integers(0, 256, (3, h, w), dtype=np.uint8))
        out = DatasetMapperTTA(tta_cfg(cfg, mins, mx, flip))({"image": img, "height": oh, "width": ow})
        d["map%d_in" % i] = img.numpy()
        d["map%d_cfg" % i] = np.array([oh, ow, mx, int(flip)] + list(mins), np.int64)
        d["map%d_n" % i] = np.int64(len(out))
        for j, o in enumerate(out):
            d["map%d_img%d" % (i, j)] = o["image"].numpy()
            d["map%d_tfm%d" % (i, j)] = tfm_rows(o["transforms"])
        print("  mapper case", i, (h, w), "->", [tuple(o["image"].shape[1:]) for o in out])
    d["map_n"] = np.int64(len(cases))


def run_tta(cfg, model, inputs, min_sizes, max_size, flip, batch_size, d, tag):
    """(b) per-augmentation raw detections, (c) the union after the inverse transforms, (d) the merged Instances."""
    from detectron2.modeling.test_time_augmentation import GeneralizedRCNNWithTTA

    tta = GeneralizedRCNNWithTTA(tta_cfg(cfg, min_sizes, max_size, flip), model, batch_size=batch_size)
    for i, inp in enumerate(inputs):
        aug_inputs, tfms = tta._get_augmented_inputs(copy.copy(inp))
        seen = []
        run = tta._batch_inference
        tta._batch_inference = lambda x: seen.append(run(x)) or seen[-1]     # keep the per-augmentation outputs
        with torch.no_grad():
            all_boxes, all_scores, all_classes = tta._get_augmented_boxes(aug_inputs, tfms)
            union = all_boxes.clone()      # Boxes.clip in the merge clamps all_boxes in place
            merged = tta._merge_detections(all_boxes, all_scores, all_classes, (inp["height"], inp["width"]))
        del tta._batch_inference
        outputs = seen[0]
        p = "%s_i%d_" % (tag, i)
        d[p + "naug"] = np.int64(len(outputs))
        d[p + "sizes"] = np.array([list(a["image"].shape[1:]) for a in aug_inputs], np.int64)
        for a, (o, t) in enumerate(zip(outputs, tfms)):
            d[p + "aug%d_boxes" % a] = o.pred_boxes.tensor.numpy()
            d[p + "aug%d_scores" % a] = o.scores.numpy()
            d[p + "aug%d_classes" % a] = o.pred_classes.numpy().astype(np.int32)
            d[p + "aug%d_tfm" % a] = tfm_rows(t)
        d[p + "union_boxes"] = union.numpy()
        d[p + "union_scores"] = torch.stack(all_scores).numpy() if all_scores else np.zeros(0, np.float32)
        d[p + "union_classes"] = torch.stack(all_classes).numpy().astype(np.int32) if all_classes else np.zeros(0, np.int32)
        d[p + "det_boxes"] = merged.pred_boxes.tensor.numpy()
        d[p + "det_scores"] = merged.scores.numpy()
        d[p + "det_classes"] = merged.pred_classes.numpy().astype(np.int32)
        print("  %s image %d: %d augmentations, union %d, merged %d" % (tag, i, len(outputs), len(union), len(merged)))


def gen_crafted(cfg, model, d):
    """(e) _merge_detections on crafted unions (boxes already in the original image's coordinates)."""
    from detectron2.modeling.test_time_augmentation import GeneralizedRCNNWithTTA

    tta = GeneralizedRCNNWithTTA(cfg, model)
    rng = np.random.default_rng(5)
    H, W = 120, 160
    cases = []
    # 0: exact score ties (same class and across classes), a NaN box, an inf score, scores at and below 1e-8, boxes off the image
    b = np.array([[10, 10, 50, 50], [12, 11, 52, 49], [10, 10, 50, 50], [100, 20, 140, 60], [101, 21, 139, 61], [-20, -5, 30, 40],
                  [150, 100, 200, 150], [np.nan, 1, 5, 5], [1, 1, 9, 9], [2, 2, 8, 8], [60, 60, 90, 90], [61, 61, 91, 91]], np.float32)
    s = np.array([0.5, 0.5, 0.5, 0.7, 0.7, 0.9, 0.6, 0.8, 1e-8, 2e-8, 0.3, 0.3], np.float32)
    c = np.array([3, 3, 4, 3, 3, 1, 1, 2, 5, 5, 7, 8], np.int32)
    s2 = s.copy()
    s2[6] = np.inf
    cases.append([(b[:6], s[:6], c[:6]), (b[:0], s[:0], c[:0]), (b[6:], s2[6:], c[6:])])
    # 1: heavy same-class overlap: 300 jittered copies of 3 boxes, two classes
    base = np.array([[20, 20, 80, 70], [30, 25, 90, 80], [70, 40, 150, 110]], np.float32)
    k = rng.integers(0, 3, 300)
    bb = (base[k] + rng.normal(0, 3, (300, 4))).astype(np.float32)
    ss = rng.uniform(0.05, 1.0, 300).astype(np.float32)
    ss[::7] = ss[3]     # ties inside the overlap clusters
    cc = rng.integers(0, 2, 300).astype(np.int32)
    cases.append([(bb[:100], ss[:100], cc[:100]), (bb[100:100], ss[100:100], cc[100:100]), (bb[100:200], ss[100:200], cc[100:200]),
                  (bb[200:], ss[200:], cc[200:])])
    # 2: more than DETECTIONS_PER_IMAGE survivors: 250 disjoint small boxes over many classes
    xy = np.stack(np.meshgrid(np.arange(25) * 6.0, np.arange(10) * 11.0), -1).reshape(-1, 2).astype(np.float32)
    bb = np.concatenate([xy, xy + 4.0], 1).astype(np.float32)
    ss = rng.uniform(0.05, 1.0, 250).astype(np.float32)
    cc = rng.integers(0, 80, 250).astype(np.int32)
    cases.append([(bb[:125], ss[:125], cc[:125]), (bb[:0], ss[:0], cc[:0]), (bb[125:], ss[125:], cc[125:])])
    for i, augs in enumerate(cases):
        p = "crafted%d_" % i
        d[p + "naug"] = np.int64(len(augs))
        for a, (bx, sc, cl) in enumerate(augs):
            d[p + "aug%d_boxes" % a], d[p + "aug%d_scores" % a], d[p + "aug%d_classes" % a] = bx, sc, cl
        boxes = torch.from_numpy(np.concatenate([x[0] for x in augs]))
        scores = [torch.tensor(v) for x in augs for v in x[1]]
        classes = [torch.tensor(int(v)) for x in augs for v in x[2]]
        with torch.no_grad():
            m = tta._merge_detections(boxes, scores, classes, (H, W))
        d[p + "hw"] = np.array([H, W], np.int64)
        d[p + "det_boxes"] = m.pred_boxes.tensor.numpy()
        d[p + "det_scores"] = m.scores.numpy()
        d[p + "det_classes"] = m.pred_classes.numpy().astype(np.int32)
        print("  crafted case", i, "union", len(boxes), "merged", len(m))


def main():
    import helpers

    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    cfg, model = mg.build_ref_model("COCO-detection/faster_rcnn_R_50_FPN_base.yaml", ["MODEL.ROI_HEADS.NUM_CLASSES", 80])
    import detectron2.modeling.test_time_augmentation as ref_tta
    import lvc.modeling

    ref_tta.GeneralizedRCNN = lvc.modeling.GeneralizedRCNN     # the reference wrapper asserts detectron2's own class
    model.load_state_dict(helpers.r50_state_dict(), strict=True)

    d = {}
    gen_mapper(cfg, d)
    a, b = uint8_image(3, 240, 320), uint8_image(4, 352, 200)
    d["small_checksums"] = np.array([checksum(a), checksum(b)])
    small = [{"image": a, "height": 480, "width": 640}, {"image": b, "height": 352, "width": 200}]
    for bs in (3, 2):
        run_tta(cfg, model, small, (200, 240, 320), 4000, True, bs, d, "small_bs%d" % bs)
    gen_crafted(cfg, model, d)
    mg.save("tta_small", **d)

    d = {}
    c = uint8_image(5, 240, 320)
    d["default_checksums"] = np.array([checksum(c)])
    aug = cfg.TEST.AUG
    d["default_cfg"] = np.array([aug.MAX_SIZE, int(aug.FLIP)] + list(aug.MIN_SIZES), np.int64)
    run_tta(cfg, model, [{"image": c, "height": 240, "width": 320}], aug.MIN_SIZES, aug.MAX_SIZE, aug.FLIP, 3, d, "default")
    mg.save("tta_default", **d)


if __name__ == "__main__":
    main()
