"""Test-time augmentation, host side (lvc_amd/modeling/test_time_augmentation.py, lvc_amd/data/transforms.py) against the reference's
DatasetMapperTTA / GeneralizedRCNNWithTTA (tests/golden/tta_*.npz, scripts/make_golden_tta.py).  No GPU needed."""
import hashlib
import os
import tempfile

import numpy as np
import pytest
import torch

from helpers import gold


def _tfm_rows(tl):
    rows = []
    for t in tl.transforms:
        n = type(t).__name__
        rows.append({"NoOpTransform": [0, 0, 0, 0, 0], "HFlipTransform": [2, getattr(t, "width", 0), 0, 0, 0]}.get(n)
                    or [1, t.h, t.w, t.new_h, t.new_w])
    return np.array(rows, np.int64)


def _uint8_image(seed, h, w):
    from lvc_amd.utils import synthetic as syn

    return syn.synthetic_image(seed, h, w).round().clamp(0, 255).to(torch.uint8)


def _plan(h, w, height, width, mins, mx, flip):
    from lvc_amd.modeling.test_time_augmentation import _Plan

    return _Plan(h, w, height, width, mins, mx, flip)


def test_input_images_match_the_fixture_checksums():
    g = gold("tta_small")
    for img, ref in zip((_uint8_image(3, 240, 320), _uint8_image(4, 352, 200)), g["small_checksums"]):
        assert hashlib.sha256(img.numpy().tobytes()).hexdigest() == str(ref)
    d = gold("tta_default")
    assert hashlib.sha256(_uint8_image(5, 240, 320).numpy().tobytes()).hexdigest() == str(d["default_checksums"][0])


def test_mapper_augmentations_and_transforms_match_the_reference():
    g = gold("tta_small")
    for i in range(int(g["map_n"])):
        cfg = g["map%d_cfg" % i].tolist()
        oh, ow, mx, flip, mins = cfg[0], cfg[1], cfg[2], bool(cfg[3]), cfg[4:]
        _, h, w = g["map%d_in" % i].shape
        p = _plan(h, w, oh, ow, mins, mx, flip)
        assert len(p.augs) == int(g["map%d_n" % i])
        for k, (j, fl) in enumerate(p.augs):
            assert tuple(p.sizes[j]) == tuple(g["map%d_img%d" % (i, k)].shape[1:])
            assert np.array_equal(_tfm_rows(p.transforms(k)), g["map%d_tfm%d" % (i, k)].numpy()), (i, k)
    for tag in ("small_bs3", "small_bs2"):
        for i, (h, w, oh, ow) in enumerate(((240, 320, 480, 640), (352, 200, 352, 200))):
            pre = "%s_i%d_" % (tag, i)
            p = _plan(h, w, oh, ow, (200, 240, 320), 4000, True)
            assert [list(p.sizes[j]) for j, _ in p.augs] == g[pre + "sizes"].tolist()
            for k in range(len(p.augs)):
                assert np.array_equal(_tfm_rows(p.transforms(k)), g[pre + "aug%d_tfm" % k].numpy())
    d = gold("tta_default")
    c = d["default_cfg"].tolist()
    p = _plan(240, 320, 240, 320, c[2:], c[0], bool(c[1]))
    assert [list(p.sizes[j]) for j, _ in p.augs] == d["default_i0_sizes"].tolist()


def _union_cases():
    for name, tags in (("tta_small", ("small_bs3_i0", "small_bs3_i1", "small_bs2_i0", "small_bs2_i1")), ("tta_default", ("default_i0",))):
        g = gold(name)
        for tag in tags:
            yield g, tag


def test_inverse_apply_box_is_bit_exact_to_the_reference_union():
    from lvc_amd.data import TransformList

    for g, tag in _union_cases():
        p = tag + "_"
        n = int(g[p + "naug"])
        hw = {"small_bs3_i0": (240, 320, 480, 640), "small_bs2_i0": (240, 320, 480, 640), "default_i0": (240, 320, 240, 320)}.get(
            tag, (352, 200, 352, 200))
        c = (200, 240, 320) if tag.startswith("small") else tuple(gold("tta_default")["default_cfg"].tolist()[2:])
        plan = _plan(*hw, c, 4000, True)
        got = []
        for k in range(n):
            tl = plan.transforms(k)
            assert isinstance(tl, TransformList)
            got.append(tl.inverse().apply_box(g[p + "aug%d_boxes" % k].numpy()))
        got = np.concatenate(got)
        assert got.dtype == np.float32
        assert np.array_equal(got, g[p + "union_boxes"].numpy()), tag


def _emulate_merge_union(boxes, row):
    """The merge kernel's inverse-transform arithmetic (csrc/tta.hip tta_inverse_box) restated in numpy fp32."""
    b = boxes.astype(np.float32).copy()
    for s in range(int(row[0])):
        kind, a, bb = int(row[1 + 3 * s]), np.float32(row[2 + 3 * s]), np.float32(row[3 + 3 * s])
        if kind == 1:
            u0, u1, v0, v1 = a - b[:, 0], a - b[:, 2], b[:, 1], b[:, 3]
        else:
            u0, u1, v0, v1 = b[:, 0] * a, b[:, 2] * a, b[:, 1] * bb, b[:, 3] * bb
        b = np.stack([np.minimum(u0, u1), np.minimum(v0, v1), np.maximum(u0, u1), np.maximum(v0, v1)], 1).astype(np.float32)
    return b


def test_merge_parameter_rows_reproduce_the_union():
    from lvc_amd.modeling.test_time_augmentation import _inverse_steps

    for g, tag in _union_cases():
        p = tag + "_"
        n = int(g[p + "naug"])
        hw = {"small_bs3_i0": (240, 320, 480, 640), "small_bs2_i0": (240, 320, 480, 640), "default_i0": (240, 320, 240, 320)}.get(
            tag, (352, 200, 352, 200))
        c = (200, 240, 320) if tag.startswith("small") else tuple(gold("tta_default")["default_cfg"].tolist()[2:])
        plan = _plan(*hw, c, 4000, True)
        got = np.concatenate([_emulate_merge_union(g[p + "aug%d_boxes" % k].numpy(), _inverse_steps(plan.transforms(k))) for k in range(n)])
        assert np.array_equal(got, g[p + "union_boxes"].numpy()), tag


def test_transform_list_semantics():
    from lvc_amd.data import HFlipTransform, NoOpTransform, ResizeTransform, TransformList

    t = NoOpTransform() + TransformList([ResizeTransform(10, 20, 30, 40), HFlipTransform(40)])      # TransformList.__radd__
    assert [type(x).__name__ for x in t.transforms] == ["NoOpTransform", "ResizeTransform", "HFlipTransform"]
    assert len(TransformList([t]) + HFlipTransform(40)) == 4                                         # flattened, then __add__
    box = np.array([[1.0, 2.0, 5.0, 7.0]], np.float32)
    fwd = t.apply_box(box)
    assert fwd.dtype == np.float32 and np.array_equal(fwd, np.array([[30.0, 6.0, 38.0, 21.0]], np.float32))
    assert np.array_equal(t.inverse().apply_box(fwd), box)
    tb = t.apply_box(torch.from_numpy(box))
    assert torch.equal(tb, torch.from_numpy(fwd))
    img = np.arange(2 * 3 * 3).reshape(2, 3, 3)
    assert np.array_equal(HFlipTransform(3).apply_image(img), img[:, ::-1])


def test_test_aug_keys_merge_from_yaml():
    from lvc_amd.config import get_cfg

    cfg = get_cfg()
    assert not cfg.TEST.AUG.ENABLED and cfg.TEST.AUG.FLIP and cfg.TEST.AUG.MAX_SIZE == 4000
    assert list(cfg.TEST.AUG.MIN_SIZES) == [400, 500, 600, 700, 800, 900, 1000, 1100, 1200]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "tta.yaml")
        with open(path, "w") as f:
            f.write("VERSION: 2\nTEST:\n  AUG:\n    ENABLED: true\n    MIN_SIZES: [200, 240]\n    MAX_SIZE: 1000\n    FLIP: false\n")
        cfg.merge_from_file(path)
    assert cfg.TEST.AUG.ENABLED and not cfg.TEST.AUG.FLIP and cfg.TEST.AUG.MAX_SIZE == 1000
    assert tuple(cfg.TEST.AUG.MIN_SIZES) == (200, 240)


def test_mapper_refuses_float_images():
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.modeling import DatasetMapperTTA

    m = DatasetMapperTTA(base_rcnn_fpn(device="cpu"))
    with pytest.raises(NotImplementedError):
        m({"image": torch.zeros(3, 20, 30), "height": 20, "width": 30})


def test_device_coefficient_cache_stays_bounded():
    from lvc_amd.data import transforms as T

    for n in range(T._DEV_COEFFS_MAX + 100):
        T.resample_coeffs(240, 100 + n, "cpu")
    assert len(T._DEV_COEFFS) <= T._DEV_COEFFS_MAX
    b, k, ks = T.resample_coeffs(240, 100 + T._DEV_COEFFS_MAX + 99, "cpu")     # the most recent one is still cached
    assert (240, 100 + T._DEV_COEFFS_MAX + 99, "cpu") in T._DEV_COEFFS
