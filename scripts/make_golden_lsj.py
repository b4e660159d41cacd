"""Generate tests/golden/train_lsj.npz: the reference's own training input with the large-scale jitter run on CPU --
DatasetMapperIgnore and DatasetMapperMosaic over an explicit augmentation list ([RandomCrop] -> [ColorJitterPIL] -> ResizeScale ->
FixedSizeCrop -> RandomFlip, the order build_augmentation and the mappers' from_config give) with a SMALL target, 72 x 100: not
square and no multiple of 32, so that the canvas fill (128) and the batch's zero padding stay apart; and one case through the
reference's build_augmentation with INPUT.LSJ True (800 x 800).  Runs only where the reference tree exists; only data goes into the
fixture.  TEST INFRASTRUCTURE ONLY.

Third-party pieces the reference imports and this image lacks, restated from fvcore's published behaviour as in
make_golden_train_input.py (restated, unpinned): `PadTransform(x0, y0, x1, y1, orig_w, orig_h, pad_value)` below -- `np.pad` of the
image with the constant, coordinates shifted by (x0, y0) -- and `CropTransform` with its optional orig_w / orig_h (that script's).
ColorJitterPIL's torchvision piece is make_golden_color_jitter.py's.

Consumers: tests/test_host_lsj.py, tests/test_gpu_lsj.py.

  per case cK_*: as train_input_*.npz (plain cases: image, ann_*) or train_mosaic.npz (mosaic cases: tiles tT_*, canvas / source /
      trim, composite_size), plus target (h, w), scale_range, pad_value, seed, torch_seed, and what the reference drew, read from the
      TransformList of the same list on the same image under the same seeds: crop (the RandomCrop window, the whole image without
      one), scale (the ResizeScale draw), scaled (h, w), u (the FixedSizeCrop draw), offset (x, y), window (ox, oy, ow, oh: what
      numpy's slicing leaves), flip, jitter_ops / jitter_factors; and its outputs: out_image (the uint8 canvas, CHW), gt_boxes fp32,
      gt_classes, gt_ignores, ids.  The numpy seed is searched (first of 0..19999) so that each case shows what its name says; the
      script asserts it.
  forced_u: no seed can land `max_offset * u` on .5 (u is one of 2^53 values), so the half-to-even case replaces the VALUE of the
      FixedSizeCrop draw by 0.5 (the generator is still advanced by the call): the reference's own np.round then rounds 2.5 / 3.5
      style products.  -1 where the draw is the generator's.
  cfg_*: the 800 x 800 case through build_augmentation; its image is stored only if the file stays under the 1 MiB limit of a
      committed file, its SHA-256 (of the CHW bytes) always.  What is restated and what is forced is also said in
      tests/golden/README_train_lsj.md.

    python scripts/make_golden_lsj.py
"""
import hashlib
import os
import sys
import tempfile

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import refshim  # noqa: E402

refshim.install()


def _install_pad_transform():
    """Before anything under detectron2.data is imported (augmentation_impl.py binds the name at import)."""
    import fvcore.transforms.transform as fvt

    class PadTransform(fvt.Transform):
        def __init__(self, x0, y0, x1, y1, orig_w=None, orig_h=None, pad_value=0, seg_pad_value=0):
            self.x0, self.y0, self.x1, self.y1, self.pad_value = x0, y0, x1, y1, pad_value

        def apply_image(self, img):
            padding = ((self.y0, self.y1), (self.x0, self.x1), (0, 0)) if img.ndim == 3 else ((self.y0, self.y1), (self.x0, self.x1))
            return np.pad(img, padding, mode="constant", constant_values=self.pad_value)

        def apply_coords(self, coords):
            coords[:, 0] += self.x0
            coords[:, 1] += self.y0
            return coords

    fvt.PadTransform = PadTransform


_install_pad_transform()

import make_golden_color_jitter as cj  # noqa: E402  (installs torchvision's ColorJitter, the shim's other pieces, imports the two below)
import make_golden_train_input as base  # noqa: E402
import make_golden_train_mosaic as mos  # noqa: E402
from make_golden_train_input import XYXY, ann, ref_annotations  # noqa: E402

TARGET = (72, 100)
SCALES = (0.5, 1.6)
MAX_SEED = 20000


class ForcedUniform:
    """np.random.uniform with the VALUE of its call number `which` (0-based) replaced by `value`; every call still advances the
    generator.  which=None: only records the draws."""

    def __init__(self, which=None, value=None):
        self.which, self.value, self.drawn = which, value, []

    def __enter__(self):
        self.real = np.random.uniform

        def uniform(*a, **k):
            v = self.real(*a, **k)
            if self.which is not None and len(self.drawn) == self.which:
                v = type(v)(self.value) if np.ndim(v) == 0 else np.full_like(v, self.value)
            self.drawn.append(v)
            return v

        np.random.uniform = uniform
        return self

    def __exit__(self, *exc):
        np.random.uniform = self.real


def ref_augs(spec):
    from detectron2.data import transforms as T

    augs = []
    if spec.get("crop"):
        augs.append(T.RandomCrop(*spec["crop"]))
    if spec.get("jitter"):
        augs.append(T.ColorJitterPIL())
    augs += [T.ResizeScale(min_scale=SCALES[0], max_scale=SCALES[1], target_height=TARGET[0], target_width=TARGET[1]),
             T.FixedSizeCrop(crop_size=TARGET), T.RandomFlip()]
    return augs


def torch_seed(seed):
    return 1000 + int(seed)


def draw(augs, image, seed, forced):
    """What the list draws on this image under this seed: a dict of the numbers, from the transforms themselves."""
    from detectron2.data import transforms as T

    np.random.seed(seed)
    torch.manual_seed(torch_seed(seed))
    # the uniform calls of the list, in order: ResizeScale, FixedSizeCrop, RandomFlip (RandomCrop draws with randint / rand)
    with ForcedUniform(1 if forced else None, 0.5) as fu:
        tfms = T.StandardAugInput(image.copy()).apply_augmentations(augs)
    names = [type(t).__name__ for t in tfms.transforms]
    core = [n for n in names if n not in ("NoOpTransform", "HFlipTransform")]
    assert core[-3:] == ["ResizeTransform", "CropTransform", "PadTransform"] and core[:-3] in (
        [], ["CropTransform"], ["PILColorTransform"], ["CropTransform", "PILColorTransform"]), names
    h, w = image.shape[:2]
    info = {"crop": (0, 0, w, h), "flip": int("HFlipTransform" in names)}
    ts = [t for t in tfms.transforms if type(t).__name__ not in ("NoOpTransform", "HFlipTransform", "PILColorTransform")]
    if len(ts) == 4:
        t = ts[0]
        info["crop"] = (int(t.x0), int(t.y0), int(t.w), int(t.h))
    rs, cr, pd = ts[-3:]
    assert (int(rs.h), int(rs.w)) == (info["crop"][3], info["crop"][2])
    info["scaled"] = (int(rs.new_h), int(rs.new_w))
    info["offset"] = (int(cr.x0), int(cr.y0))
    sh, sw = info["scaled"]
    info["window"] = (int(cr.x0), int(cr.y0), min(sw, TARGET[1]), min(sh, TARGET[0]))
    assert (int(pd.x1), int(pd.y1)) == (TARGET[1] - info["window"][2], TARGET[0] - info["window"][3]) and (pd.x0, pd.y0) == (0, 0)
    assert len(fu.drawn) == 3
    info["scale"], info["u"] = float(fu.drawn[0]), float(fu.drawn[1])
    return info


def record_draw(d, p, info, seed, forced, spec):
    d[p + "target"] = np.array(TARGET, np.int64)
    d[p + "scale_range"] = np.array(SCALES, np.float64)
    d[p + "pad_value"] = np.float64(128.0)
    d[p + "seed"] = np.int64(seed)
    d[p + "torch_seed"] = np.int64(torch_seed(seed))
    d[p + "forced_u"] = np.float64(0.5 if forced else -1.0)
    d[p + "crop"] = np.array(info["crop"], np.int64)
    d[p + "scale"] = np.float64(info["scale"])
    d[p + "u"] = np.float64(info["u"])
    d[p + "scaled"] = np.array(info["scaled"], np.int64)
    d[p + "offset"] = np.array(info["offset"], np.int64)
    d[p + "window"] = np.array(info["window"], np.int64)
    d[p + "flip"] = np.int64(info["flip"])
    d[p + "new_size"] = np.array(TARGET, np.int64)
    crop = spec.get("crop")
    d[p + "crop_enabled"] = np.int64(crop is not None)
    d[p + "crop_type"] = np.array(crop[0] if crop else "relative_range")
    d[p + "crop_size"] = np.array(crop[1] if crop else (0.9, 0.9), np.float64)
    d[p + "min_sizes"], d[p + "max_size"], d[p + "sampling"] = np.array((64,), np.int64), np.int64(1333), np.array("choice")
    d[p + "jitter"] = np.int64(bool(spec.get("jitter")))
    d[p + "jitter_ops"] = np.array(cj.LAST["ops"] if spec.get("jitter") else [], np.int64)
    d[p + "jitter_factors"] = np.array(cj.LAST["factors"] if spec.get("jitter") else [], np.float64)


def record_out(d, p, out):
    inst = out["instances"]
    d[p + "out_image"] = out["image"].numpy()
    d[p + "gt_boxes"] = inst.gt_boxes.tensor.numpy()
    d[p + "gt_classes"] = inst.gt_classes.numpy()
    d[p + "gt_ignores"] = inst.gt_ignores.numpy()
    d[p + "ids"] = inst.ids.numpy()
    assert tuple(out["image"].shape[1:]) == TARGET and inst.gt_boxes.tensor.dtype == torch.float32


def record_anns(d, q, anns):
    d[q + "ann_bbox"] = np.array([a["bbox"] for a in anns], np.float64).reshape(-1, 4)
    d[q + "ann_mode"] = np.array([a["mode"] for a in anns], np.int64)
    d[q + "ann_cat"] = np.array([a["cat"] for a in anns], np.int64)
    d[q + "ann_iscrowd"] = np.array([-1 if a["iscrowd"] is None else a["iscrowd"] for a in anns], np.int64)
    d[q + "ann_ignore"] = np.array([-1 if a["ignore"] is None else a["ignore"] for a in anns], np.int64)
    d[q + "ann_id"] = np.array([-1000 if a["id"] is None else a["id"] for a in anns], np.int64)


def boxes_for(h, w):
    """A large central box (kept by every window), a small box in each of two opposite corners (a crop removes one), a crowd."""
    return [ann([0.2 * w, 0.2 * h, 0.6 * w, 0.6 * h], 3, id=11), ann([0.5, 0.5, 0.12 * w, 0.12 * h], 17, ignore=1, id=12),
            ann([0.86 * w, 0.86 * h, w - 0.5, h - 0.5], 5, mode=XYXY), ann([0.3 * w, 0.3 * h, 0.2 * w, 0.2 * h], 9, iscrowd=1, id=14)]


def run_plain(d, k, name, rng, hw, spec, want, forced=False):
    from PIL import Image

    from lvc.data.dataset_mapper import DatasetMapperIgnore

    h, w = hw
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)      # in INPUT.FORMAT (BGR) order
    anns = boxes_for(h, w)
    augs = ref_augs(spec)
    mapper = DatasetMapperIgnore(is_train=True, augmentations=augs, image_format="BGR")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "image.png")
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(path)
        dic = {"file_name": path, "height": h, "width": w, "image_id": k, "annotations": ref_annotations(anns)}
        for seed in range(MAX_SEED):
            info = draw(augs, img, seed, forced)
            info["hw"], info["n"], info["candidates"] = hw, -1, 3
            if not want(info):
                continue
            np.random.seed(seed)
            torch.manual_seed(torch_seed(seed))
            with ForcedUniform(1 if forced else None, 0.5):
                out = mapper(dic)
            info["n"] = len(out["instances"])
            if info["n"] >= 1 and want(info):
                break
        else:
            raise RuntimeError("no seed shows case " + name)
    p = "c%d_" % k
    d[p + "name"] = np.array(name)
    d[p + "n_tiles"] = np.int64(1)
    d[p + "image"] = img
    record_anns(d, p, anns)
    record_draw(d, p, info, seed, forced, spec)
    record_out(d, p, out)
    print("  case %2d %-28s %s seed %5d crop %s scale %.4f -> %s u %.4f window %s flip %d, %d of 3 boxes kept" %
          (k, name, hw, seed, info["crop"], info["scale"], info["scaled"], info["u"], info["window"], info["flip"], info["n"]))
    return info


def run_mosaic(d, k, name, rng, sizes, spec, want):
    import copy

    from PIL import Image

    from lvc.data import mosaic as ref_mosaic

    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    anns = mos.tile_anns(rng, sizes, 1000 * (k + 1))
    augs = ref_augs(spec)
    mapper = ref_mosaic.DatasetMapperMosaic(is_train=True, augmentations=augs, image_format="BGR")
    with tempfile.TemporaryDirectory() as tmp:
        dicts = []
        for t, (img, a) in enumerate(zip(imgs, anns)):
            path = os.path.join(tmp, "tile%d.png" % t)
            Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(path)
            dicts.append({"file_name": path, "height": img.shape[0], "width": img.shape[1], "image_id": 100 * k + t,
                          "annotations": ref_annotations(a)})
        tr = mos.Traced()
        composite, merged = tr((ref_mosaic.get_mosaic if len(sizes) == 4 else ref_mosaic.get_mosaic9), copy.deepcopy(dicts), imgs)
        composite = composite.copy()
        canvas = np.array([tr.tiles[t][:4] for t in range(len(sizes))], np.int64)
        source = np.array([tr.tiles[t][4:] for t in range(len(sizes))], np.int64)
        trim = np.array(tr.trim, np.int64)
        side = (2 if len(sizes) == 4 else 3) * max(sizes[0])
        count = mos.paint_count(canvas, side)[trim[1]:trim[3], trim[0]:trim[2]]
        assert count.shape == composite.shape[:2]
        for seed in range(MAX_SEED):
            info = draw(augs, composite, seed, False)
            # the composite pixels well inside what the window shows: the window mapped back, shrunk by one source pixel a side
            x0, y0, cw, ch = info["crop"]
            ox, oy, ow, oh = info["window"]
            fx, fy = cw / info["scaled"][1], ch / info["scaled"][0]
            xa, xb = int(np.ceil(ox * fx)) + 1, int(np.floor((ox + ow) * fx)) - 1
            ya, yb = int(np.ceil(oy * fy)) + 1, int(np.floor((oy + oh) * fy)) - 1
            win = count[y0 + ya:y0 + yb, x0 + xa:x0 + xb]
            info["fill"] = bool(win.size and (win == 0).any())
            info["n"] = -1
            if not want(info):
                continue
            np.random.seed(seed)
            torch.manual_seed(torch_seed(seed))
            out = mapper(dicts)
            info["n"] = len(out["instances"])
            if info["n"] >= 1 and want(info):
                break
        else:
            raise RuntimeError("no seed shows case " + name)
    p = "c%d_" % k
    d[p + "name"] = np.array(name)
    d[p + "n_tiles"] = np.int64(len(sizes))
    for t, (img, a) in enumerate(zip(imgs, anns)):
        q = p + "t%d_" % t
        d[q + "image"] = img
        d[q + "image_id"] = np.int64(100 * k + t)
        record_anns(d, q, a)
    d[p + "canvas"], d[p + "source"], d[p + "trim"] = canvas, source, trim
    d[p + "composite_size"] = np.array(composite.shape[:2], np.int64)
    d[p + "fill_in_window"] = np.int64(info["fill"])
    d[p + "out_image_id"] = np.int64(out["image_id"])
    record_draw(d, p, info, seed, False, spec)
    record_out(d, p, out)
    assert info["fill"] and (out["image"].numpy() == 114).all(axis=0).any()
    print("  case %2d %-28s %d tiles composite %s seed %5d crop %s scale %.4f -> %s window %s flip %d, %d boxes kept" %
          (k, name, len(sizes), tuple(composite.shape[:2]), seed, info["crop"], info["scale"], info["scaled"], info["window"],
           info["flip"], info["n"]))
    return info


def gen_cfg_case(d, rng):
    """The reference's own list: build_augmentation with INPUT.LSJ True, through DatasetMapperIgnore(cfg, True)."""
    from PIL import Image

    from lvc.config import get_cfg
    from lvc.data.dataset_mapper import DatasetMapperIgnore

    global TARGET
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "INPUT.LSJ", True])
    cfg.freeze()
    mapper = DatasetMapperIgnore(cfg, True)
    names = [type(a).__name__ for a in mapper.augmentations]
    assert names == ["ResizeScale", "FixedSizeCrop", "RandomFlip"], names
    rs, fc = mapper.augmentations[:2]
    assert (rs.min_scale, rs.max_scale, rs.target_height, rs.target_width, tuple(fc.crop_size), fc.pad_value) == (0.5, 1.6, 800, 800,
                                                                                                                 (800, 800), 128.0)
    h, w = 96, 128
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    anns = boxes_for(h, w)
    small, TARGET = TARGET, (800, 800)
    try:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "image.png")
            Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(path)
            dic = {"file_name": path, "height": h, "width": w, "image_id": 7, "annotations": ref_annotations(anns)}
            for seed in range(MAX_SEED):      # cropped on x, padded on y, flipped
                info = draw(mapper.augmentations, img, seed, False)
                if info["scaled"][1] > 800 and info["offset"][0] > 0 and info["flip"] == 1:
                    break
            np.random.seed(seed)
            out = mapper(dic)
        p = "cfg_"
        d[p + "image"] = img
        record_anns(d, p, anns)
        record_draw(d, p, info, seed, False, {})
        chw = out["image"].numpy()
        assert chw.shape == (3, 800, 800)
        d[p + "sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(chw).tobytes()).hexdigest())
        inst = out["instances"]
        d[p + "gt_boxes"], d[p + "gt_classes"] = inst.gt_boxes.tensor.numpy(), inst.gt_classes.numpy()
        d[p + "gt_ignores"], d[p + "ids"] = inst.gt_ignores.numpy(), inst.ids.numpy()
        print("  cfg case: %s seed %d scale %.4f -> %s window %s flip %d, %d boxes kept, sha256 %s..." %
              ((h, w), seed, info["scale"], info["scaled"], info["window"], info["flip"], len(inst), str(d[p + "sha256"])[:12]))
        return chw
    finally:
        TARGET = small


def gen():
    rng = np.random.default_rng(2027)
    Th, Tw = TARGET
    rr = ("relative_range", (0.7, 0.7))
    sc, of, wi = (lambda i: i["scaled"]), (lambda i: i["offset"]), (lambda i: i["window"])
    plain = [
        ("crop_both_box_removed", (90, 120), {}, lambda i: sc(i)[0] > Th and sc(i)[1] > Tw and min(of(i)) > 0 and i["n"] in (-1, 1, 2)),
        ("pad_both_noflip", (90, 120), {}, lambda i: sc(i)[0] < Th and sc(i)[1] < Tw and i["flip"] == 0),
        ("pad_both_flip", (88, 117), {}, lambda i: sc(i)[0] < Th and sc(i)[1] < Tw and i["flip"] == 1),
        ("crop_x_pad_y", (40, 120), {}, lambda i: sc(i)[0] < Th and sc(i)[1] > Tw and of(i)[0] > 0),
        ("crop_y_pad_x_flip", (120, 40), {}, lambda i: sc(i)[0] > Th and sc(i)[1] < Tw and of(i)[1] > 0 and i["flip"] == 1),
        ("scaled_equals_target_on_x", (40, 120), {}, lambda i: sc(i)[1] == Tw and sc(i)[0] != Th),
        ("width_unchanged", (60, 20), {}, lambda i: sc(i)[1] == 20 and sc(i)[0] != 60),
        ("height_unchanged", (20, 60), {}, lambda i: sc(i)[0] == 20 and sc(i)[1] != 60),
        ("random_crop_in_front", (110, 150), {"crop": rr}, lambda i: sc(i)[1] > Tw and of(i)[0] > 0 and i["crop"][0] > 0),
        ("colour_jitter_in_front", (64, 90), {"jitter": True}, lambda i: sc(i)[1] > Tw and sc(i)[0] < Th),
        ("crop_and_jitter_in_front_flip", (100, 140), {"crop": rr, "jitter": True},
         lambda i: sc(i)[0] > Th and sc(i)[1] > Tw and i["flip"] == 1),
    ]
    d = {}
    k = 0
    infos = {}
    for name, hw, spec, want in plain:
        infos[name] = run_plain(d, k, name, rng, hw, spec, want)
        k += 1
    # half to even: max offsets 2 * odd + 1 apart in parity, u forced to 0.5 -> products k + .5, one rounded down and one up
    def half(i):
        mx, my = i["scaled"][1] - Tw, i["scaled"][0] - Th
        return mx > 0 and my > 0 and mx % 2 == 1 and my % 2 == 1 and (mx // 2) % 2 != (my // 2) % 2
    infos["offset_half_to_even"] = i = run_plain(d, k, "offset_half_to_even", rng, (90, 120), {}, half, forced=True)
    mx, my = i["scaled"][1] - Tw, i["scaled"][0] - Th
    assert i["u"] == 0.5 and {i["offset"][0] - mx // 2, i["offset"][1] - my // 2} == {0, 1} and all(v % 2 == 0 for v in i["offset"])
    k += 1
    n_plain = k
    sizes4 = [(40, 56), (60, 30), (28, 64), (52, 44)]
    sizes9 = [(30, 42), (34, 60), (58, 22), (48, 36), (24, 46), (60, 60), (20, 31), (40, 52), (56, 20)]
    run_mosaic(d, k, "m4_fill_in_window", rng, sizes4, {}, lambda i: i["fill"] and i["scaled"][1] > Tw)
    k += 1
    run_mosaic(d, k, "m9_fill_in_window_crop_flip", rng, sizes9, {"crop": rr}, lambda i: i["fill"] and i["flip"] == 1)
    k += 1
    d["n"], d["n_plain"] = np.int64(k), np.int64(n_plain)
    assert len(d["c0_gt_classes"]) < 3      # the crop removed a box entirely
    chw = gen_cfg_case(d, rng)
    d["cfg_has_image"] = np.int64(0)
    path = os.path.join(base.GOLD, "train_lsj.npz")
    np.savez_compressed(path, **dict(d, cfg_out_image=chw, cfg_has_image=np.int64(1)))
    if os.path.getsize(path) >= 900 * 1024:      # over the limit of a committed file: the digest alone
        print("  the 800 x 800 image would make the file %.1f KB: its SHA-256 is stored instead" % (os.path.getsize(path) / 1024))
        np.savez_compressed(path, **d)
    print("wrote train_lsj.npz %8.1f KB" % (os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    gen()
