"""Colour jitter, host side: the numpy mirror of the pixel arithmetic (tests/color_ref.py) against the installed Pillow, the draws of
lvc_amd.data.ColorJitter against the reference's recorded ones (tests/golden/color_jitter.npz, scripts/make_golden_color_jitter.py),
and how a caller opts in.  No GPU needed.  Every comparison is for equality."""
import os
import re

import numpy as np
import pytest
import torch

import color_ref as R
from test_host_train_input import case_cfg, case_dict, gold
from test_host_train_mosaic import mosaic_cfg, tile_dicts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def jitter_cases():
    """Every fixture case as a dict of its arrays (prefix stripped); a mosaic case has its tiles under "tiles"."""
    g = gold("color_jitter")
    out = []
    for k in range(int(g["n"])):
        p = "c%d_" % k
        c = {key[len(p):]: g[key] for key in g if key.startswith(p)}
        c["tiles"] = []
        for t in range(int(c["n_tiles"]) if int(c["n_tiles"]) > 1 else 0):
            q = "t%d_" % t
            c["tiles"].append({key[len(q):]: c[key] for key in c if isinstance(key, str) and key.startswith(q)})
        out.append(c)
    return out


def jitter_cfg(c, device="cpu", key=True):
    cfg = mosaic_cfg(c, device) if c["tiles"] else case_cfg(c, device)
    cfg.defrost()
    cfg.INPUT.COLOR_JITTER = bool(key)
    cfg.freeze()
    return cfg


def seed_case(c):
    np.random.seed(int(c["seed"]))
    torch.manual_seed(int(c["torch_seed"]))


def case_mapper(c, device="cpu"):
    from lvc_amd.data import DatasetMapper, DatasetMapperMosaic

    cls = DatasetMapperMosaic if c["tiles"] else DatasetMapper
    return cls.from_config(jitter_cfg(c, device), True, color_jitter=True)


def case_input(c):
    return tile_dicts(c) if c["tiles"] else case_dict(c)


# ------------------------------------------------------------------------------------------------ the mirror against Pillow
@pytest.fixture(scope="module")
def colours():
    return R.all_colours()


def test_mirror_grey_and_both_hsv_directions_equal_pillow_on_every_input(colours):
    Image = pytest.importorskip("PIL.Image")
    im = Image.fromarray(colours)
    assert np.array_equal(np.asarray(im.convert("L")), R.grey(colours))
    assert np.array_equal(np.asarray(im.convert("HSV")), R.rgb_to_hsv(colours))
    hsv = Image.merge("HSV", [Image.fromarray(np.ascontiguousarray(colours[..., i])) for i in range(3)])
    assert np.array_equal(np.asarray(hsv.convert("RGB")), R.hsv_to_rgb(colours))


def test_mirror_blend_equals_pillow_on_every_pair():
    Image = pytest.importorskip("PIL.Image")
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rng = np.random.default_rng(3)
    factors = [0.6, 1.0, 1.4] + [float(np.float32(v)) for v in rng.uniform(0.6, 1.4, 2)]
    for f in factors:
        got = np.asarray(Image.blend(Image.fromarray(a), Image.fromarray(b), f))
        assert np.array_equal(got, R.blend(a, b, f)), f


def test_mirror_contrast_mean_rounds_half_up_as_pillow():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance

    img = np.array([[[10, 10, 10], [11, 11, 11]]], np.uint8)      # L = 10, 11: the mean is 10.5
    assert R.grey(img).tolist() == [[10, 11]] and R.mean_grey(img) == 11
    deg = np.asarray(ImageEnhance.Contrast(Image.fromarray(img)).degenerate)
    assert (deg == 11).all()


def _pillow_jitter(img, ops, factors):
    """torchvision 0.8.2 functional_pil's four adjustments over the installed Pillow."""
    from PIL import Image, ImageEnhance

    im = Image.fromarray(img)
    for op, f in zip(ops, factors):
        if op == 3:
            h, s, v = im.convert("HSV").split()
            h = Image.fromarray((np.asarray(h).astype(np.int32) + int(f * 255) % 256).astype(np.uint8), "L")
            im = Image.merge("HSV", (h, s, v)).convert("RGB")
        else:
            im = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op](im).enhance(f)
    return np.asarray(im)


def test_mirror_composition_equals_pillow():
    pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    for ops in ([1, 0, 3, 2], [3, 2, 0, 1], [0, 3, 1, 2], [2, 1], [3], []):
        factors = [float(np.float32(rng.uniform(-0.2, 0.2) if o == 3 else rng.uniform(0.6, 1.4))) for o in ops]
        assert np.array_equal(R.jitter(img, ops, factors), _pillow_jitter(img, ops, factors)), ops
    assert R.hue_shift(-0.1) == 231 and R.hue_shift(0.0) == 0
    assert not np.array_equal(R.hue(img, 0.0), img)      # no identity shortcut: the round trip through HSV is lossy


def test_fixture_images_are_the_mirror_of_their_recorded_draws():
    """The reference's output of every plain case whose resize is a copy is the mirror on its crop: ties the fixture to the mirror
    without Pillow."""
    n = 0
    for c in jitter_cases():
        x0, y0, cw, ch = c["crop"].tolist()
        if c["tiles"] or c["new_size"].tolist() != [ch, cw]:
            continue
        exp = R.jitter(c["image"][y0:y0 + ch, x0:x0 + cw], c["jitter_ops"].tolist(), c["jitter_factors"].tolist())
        exp = exp[:, ::-1] if int(c["flip"]) else exp
        assert np.array_equal(exp.transpose(2, 0, 1), c["out_image"]), str(c["name"])
        n += 1
    assert n >= 1


# ------------------------------------------------------------------------------------------------ the draws
def test_fixture_covers_the_cases_the_feature_names():
    cs = jitter_cases()
    plain = [c for c in cs if not c["tiles"]]
    assert len(plain) >= 6 and sum(int(c["crop_enabled"]) for c in plain) >= 6
    assert {c["jitter_ops"].tolist().index(1) for c in plain} == {0, 1, 2, 3}      # contrast first, in the middle, last
    hues = [float(c["jitter_factors"][c["jitter_ops"].tolist().index(3)]) for c in plain]
    assert min(hues) < 0 < max(hues)
    assert {len(c["tiles"]) for c in cs} == {0, 4, 9}
    assert all(int(c["fill_in_window"]) == 1 for c in cs if c["tiles"])
    for c in cs:
        assert sorted(c["jitter_ops"].tolist()) == [0, 1, 2, 3]
        f = c["jitter_factors"]
        assert (f.astype(np.float32).astype(np.float64) == f).all()      # fp32 draws
        for img in ([t["image"] for t in c["tiles"]] or [c["image"]]):
            assert max(img.shape[:2]) <= 160
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "color_jitter.npz")) < (1 << 20)


def test_seeded_draws_equal_the_reference_bit_for_bit():
    for c in jitter_cases():
        name = str(c["name"])
        seed_case(c)
        out, _, p = case_mapper(c).draw(case_input(c))
        assert p.jitter is not None, name
        ops, factors = p.jitter
        assert list(ops) == c["jitter_ops"].tolist(), name
        assert np.array(factors, np.float64).tobytes() == c["jitter_factors"].tobytes(), name
        assert list(p.crop) == c["crop"].tolist() and list(p.new_size) == c["new_size"].tolist() and int(p.flip) == int(c["flip"]), name
        assert out["instances"].gt_boxes.tensor.numpy().tobytes() == c["gt_boxes"].tobytes(), name


def test_jitter_draws_leave_numpy_alone_and_follow_the_permutation():
    from lvc_amd.data import ColorJitter
    from lvc_amd.data.transforms import _Shape

    c = jitter_cases()[0]
    seed_case(c)
    with_jitter = case_mapper(c).draw(case_input(c))[2]
    from lvc_amd.data import DatasetMapper

    np.random.seed(int(c["seed"]))
    without = DatasetMapper.from_config(jitter_cfg(c, key=False), True, color_jitter=True).draw(case_input(c))[2]
    assert without.jitter is None and (with_jitter.crop, with_jitter.new_size, with_jitter.flip) == (without.crop, without.new_size, without.flip)
    # torchvision 0.8.2's forward: randperm(4), then one uniform_ per step in the permutation's order
    g = torch.Generator().manual_seed(77)
    t = ColorJitter(generator=g).get_transform(_Shape(4, 4))
    g.manual_seed(77)
    perm = torch.randperm(4, generator=g).tolist()
    lo_hi = [(0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.2, 0.2)]
    factors = [torch.tensor(1.0).uniform_(*lo_hi[i], generator=g).item() for i in perm]
    assert list(t.ops) == perm and list(t.factors) == factors
    # a step whose range is a single point is left out, the permutation is still drawn
    g.manual_seed(77)
    t = ColorJitter(hue=0, generator=g).get_transform(_Shape(4, 4))
    assert list(t.ops) == [i for i in perm if i != 3]


# ------------------------------------------------------------------------------------------------ opting in
def _loader_calls(cfg, **kw):
    from lvc_amd.data import DatasetMapper, DatasetMapperMosaic, build_detection_train_loader, build_detection_train_mosaic_loader

    data = [{"raw": torch.zeros(8, 8, 3, dtype=torch.uint8), "width": 8, "height": 8}]
    return [lambda: DatasetMapper.from_config(cfg, True, **kw), lambda: DatasetMapperMosaic.from_config(cfg, True, **kw),
            lambda: build_detection_train_loader(cfg, data, seed=0, **kw), lambda: build_detection_train_mosaic_loader(cfg, data, seed=0, **kw)]


def test_default_arguments_still_raise_and_say_how_to_opt_in():
    c = jitter_cases()[0]
    for call in _loader_calls(jitter_cfg(c)):
        with pytest.raises(NotImplementedError, match=r"INPUT\.COLOR_JITTER.*color_jitter=True"):
            call()


def test_blur_and_lsj_raise_whatever_is_passed():
    from lvc_amd.data import ColorJitter

    c = jitter_cases()[0]
    for key in ("BLUR", "LSJ"):
        cfg = jitter_cfg(c)
        cfg.defrost()
        setattr(cfg.INPUT, key, True)
        cfg.freeze()
        for kw in ({"color_jitter": True}, {"color_jitter": ColorJitter()}):
            for call in _loader_calls(cfg, **kw):
                with pytest.raises(NotImplementedError, match="INPUT." + key):
                    call()


def test_color_jitter_true_follows_the_key_and_an_instance_overrides_it():
    from lvc_amd.data import ColorJitter, DatasetMapper, build_augmentation

    c = jitter_cases()[0]
    on, off = jitter_cfg(c), jitter_cfg(c, key=False)
    names = lambda augs: [type(a).__name__ for a in augs]      # noqa: E731
    assert names(build_augmentation(on, True, color_jitter=True)) == ["RandomCrop", "ColorJitter", "ResizeShortestEdge", "RandomFlip"]
    assert names(build_augmentation(off, True, color_jitter=True)) == ["RandomCrop", "ResizeShortestEdge", "RandomFlip"]
    assert names(build_augmentation(off, True)) == ["RandomCrop", "ResizeShortestEdge", "RandomFlip"]
    assert names(build_augmentation(on, False, color_jitter=True)) == ["ResizeShortestEdge"]
    mine = ColorJitter(brightness=0.1, contrast=0, saturation=0, hue=0)
    augs = build_augmentation(off, True, color_jitter=mine)
    assert augs[1] is mine
    np.random.seed(0)
    p = DatasetMapper.from_config(off, True, color_jitter=mine).draw(case_dict(c))[2]
    assert p.jitter[0] == (0,) and 0.9 <= p.jitter[1][0] <= 1.1
    np.random.seed(0)
    assert DatasetMapper.from_config(off, True, color_jitter=True).draw(case_dict(c))[2].jitter is None
    with pytest.raises(TypeError):
        build_augmentation(on, True, color_jitter="yes")


def test_header_declares_the_entry_and_kernels_binds_it():
    from lvc_amd import _lib
    from lvc_amd import kernels as K

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvc_amd.h")).read(), flags=re.S)
    assert "int lvc_color_jitter_tiles_u8(" in txt
    assert hasattr(_lib.lib(), "lvc_color_jitter_tiles_u8")
    assert callable(K.color_jitter_tiles_u8) and K.COLOR_JITTER_FIELDS == 128 and K.COLOR_JITTER_LAUNCHES == K.COLOR_JITTER_LAUNCHES[:64]
    assert K.COLOR_JITTER_OPS == ("brightness", "contrast", "saturation", "hue")
    assert (R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE) == (0, 1, 2, 3)
