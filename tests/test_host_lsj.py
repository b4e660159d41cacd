"""Large-scale jitter, host side (lvc_amd/data/transforms.py ResizeScale / FixedSizeCrop / LargeScaleJitter, dataset_mapper.py,
build.py, kernels.train_input_lsj_blob) against the reference's recorded draws and boxes (tests/golden/train_lsj.npz,
scripts/make_golden_lsj.py), how a caller opts in, and the library's refusal of a corrupted job table.  No GPU needed.  Every
comparison is for equality."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_host_train_input import case_cfg, case_dict, gold
from test_host_train_mosaic import mosaic_cfg, tile_dicts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lsj_cases():
    """Every fixture case as a dict of its arrays (prefix stripped); a mosaic case has its tiles under "tiles"."""
    g = gold("train_lsj")
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


def cfg_case():
    g = gold("train_lsj")
    return {key[4:]: g[key] for key in g if key.startswith("cfg_")}


def lsj_of(c):
    from lvc_amd.data import LargeScaleJitter

    return LargeScaleJitter(float(c["scale_range"][0]), float(c["scale_range"][1]), int(c["target"][0]), int(c["target"][1]),
                            float(c["pad_value"]))


def lsj_cfg(c, device="cpu", key=False):
    cfg = mosaic_cfg(c, device) if c["tiles"] else case_cfg(c, device)
    cfg.defrost()
    cfg.INPUT.COLOR_JITTER = bool(int(c["jitter"]))
    cfg.INPUT.LSJ = bool(key)
    cfg.freeze()
    return cfg


def case_mapper(c, device="cpu"):
    from lvc_amd.data import DatasetMapper, DatasetMapperMosaic

    cls = DatasetMapperMosaic if c["tiles"] else DatasetMapper
    return cls.from_config(lsj_cfg(c, device), True, color_jitter=True, lsj=lsj_of(c))


def case_input(c):
    return tile_dicts(c) if c["tiles"] else case_dict(c)


@contextlib.contextmanager
def seeded(c):
    """The seeds of a case; where the fixture forced the VALUE of FixedSizeCrop's draw (the second np.random.uniform call of the
    list: no seed lands a product on .5), the same here -- the generator is still advanced by the call."""
    np.random.seed(int(c["seed"]))
    torch.manual_seed(int(c["torch_seed"]))
    forced = float(c["forced_u"])
    real, calls = np.random.uniform, []

    def uniform(*a, **k):
        v = real(*a, **k)
        calls.append(v)
        return forced if forced >= 0 and len(calls) == 2 else v

    np.random.uniform = uniform
    try:
        yield calls
    finally:
        np.random.uniform = real


def test_fixture_covers_the_cases_the_feature_names():
    cs = {str(c["name"]): c for c in lsj_cases()}
    Th, Tw = 72, 100
    assert all(c["target"].tolist() == [Th, Tw] and c["out_image"].shape == (3, Th, Tw) for c in cs.values())
    assert Th % 32 and Tw % 32 and Th != Tw
    sc, of = (lambda c: c["scaled"].tolist()), (lambda c: c["offset"].tolist())
    c = cs["crop_both_box_removed"]
    assert sc(c)[0] > Th and sc(c)[1] > Tw and min(of(c)) > 0 and 0 < len(c["gt_classes"]) < 3
    assert all(sc(cs[n])[0] < Th and sc(cs[n])[1] < Tw for n in ("pad_both_noflip", "pad_both_flip"))
    assert int(cs["pad_both_flip"]["flip"]) == 1 and int(cs["pad_both_noflip"]["flip"]) == 0
    c = cs["crop_x_pad_y"]
    assert sc(c)[0] < Th and sc(c)[1] > Tw and of(c)[0] > 0
    c = cs["crop_y_pad_x_flip"]
    assert sc(c)[0] > Th and sc(c)[1] < Tw and of(c)[1] > 0
    assert sc(cs["scaled_equals_target_on_x"])[1] == Tw != sc(cs["scaled_equals_target_on_x"])[0]
    c = cs["width_unchanged"]
    assert sc(c)[1] == c["image"].shape[1] and sc(c)[0] != c["image"].shape[0]
    c = cs["height_unchanged"]
    assert sc(c)[0] == c["image"].shape[0] and sc(c)[1] != c["image"].shape[1]
    c = cs["offset_half_to_even"]
    mx, my = sc(c)[1] - Tw, sc(c)[0] - Th
    assert float(c["forced_u"]) == 0.5 and mx % 2 == 1 and my % 2 == 1      # products k + .5: one rounds down, one up, both to even
    assert sorted([of(c)[0] - mx // 2, of(c)[1] - my // 2]) == [0, 1] and all(v % 2 == 0 for v in of(c))
    assert int(cs["random_crop_in_front"]["crop_enabled"]) and cs["random_crop_in_front"]["crop"][0] > 0
    assert int(cs["colour_jitter_in_front"]["jitter"]) and len(cs["colour_jitter_in_front"]["jitter_ops"]) == 4
    assert {len(c["tiles"]) for c in cs.values()} == {0, 4, 9}
    for c in cs.values():
        assert len(c["gt_classes"]) >= 1
        if c["tiles"]:
            assert int(c["fill_in_window"]) == 1 and (c["out_image"] == 114).all(axis=0).any()
        for img in ([t["image"] for t in c["tiles"]] or [c["image"]]):
            assert max(img.shape[:2]) <= 160
    g = cfg_case()
    assert g["target"].tolist() == [800, 800] and len(str(g["sha256"])) == 64
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "train_lsj.npz")) < (1 << 20)


def test_seeded_draws_and_boxes_equal_the_reference_bit_for_bit():
    for c in lsj_cases():
        name = str(c["name"])
        mapper = case_mapper(c)
        with seeded(c) as calls:
            out, _, p = mapper.draw(case_input(c))
        assert len(calls) == 3 and float(calls[0]) == float(c["scale"]), name      # ResizeScale, FixedSizeCrop, RandomFlip
        if float(c["forced_u"]) < 0:
            assert float(calls[1]) == float(c["u"]), name
        assert list(p.crop) == c["crop"].tolist() and list(p.scaled) == c["scaled"].tolist(), name
        window, target, fill = p.lsj
        assert list(window) == c["window"].tolist() and list(window[:2]) == c["offset"].tolist(), name
        assert list(target) == c["target"].tolist() == list(p.new_size) and fill == 128 and int(p.flip) == int(c["flip"]), name
        if int(c["jitter"]):
            assert list(p.jitter[0]) == c["jitter_ops"].tolist(), name
            assert np.array(p.jitter[1], np.float64).tobytes() == c["jitter_factors"].tobytes(), name
        else:
            assert p.jitter is None, name
        inst = out["instances"]
        assert inst.gt_boxes.tensor.dtype == torch.float32 and inst.gt_boxes.tensor.numpy().tobytes() == c["gt_boxes"].tobytes(), name
        assert inst.gt_classes.tolist() == c["gt_classes"].tolist() and inst.ids.tolist() == c["ids"].tolist(), name
        assert inst.gt_ignores.tolist() == c["gt_ignores"].tolist() and inst.image_size == (72, 100), name


def test_cfg_key_builds_the_references_defaults_and_draws_its_case():
    from lvc_amd.data import DatasetMapper, FixedSizeCrop, LargeScaleJitter, ResizeScale, build_augmentation

    g = cfg_case()
    g["tiles"], g["jitter"] = [], 0
    on, off = lsj_cfg(g, key=True), lsj_cfg(g, key=False)
    augs = build_augmentation(on, True, lsj=True)
    assert [type(a).__name__ for a in augs] == ["ResizeScale", "FixedSizeCrop", "RandomFlip"]
    rs, fc = augs[:2]
    assert isinstance(rs, ResizeScale) and isinstance(fc, FixedSizeCrop)
    assert (rs.min_scale, rs.max_scale, rs.target_height, rs.target_width, fc.crop_size, fc.pad_value) == (0.5, 1.6, 800, 800, (800, 800), 128.0)
    d = LargeScaleJitter()
    assert (d.min_scale, d.max_scale, d.target_height, d.target_width, d.pad_value) == (0.5, 1.6, 800, 800, 128.0)
    names = lambda a: [type(x).__name__ for x in a]      # noqa: E731
    assert names(build_augmentation(off, True, lsj=True)) == ["ResizeShortestEdge", "RandomFlip"]      # True follows the key
    assert names(build_augmentation(on, False, lsj=True)) == ["ResizeShortestEdge"]                    # never at test time
    mine = LargeScaleJitter(0.8, 1.2, 72, 100)
    augs = build_augmentation(off, True, lsj=mine)      # an instance is used whatever the key says
    assert augs[0] is mine.resize and augs[1] is mine.crop
    crop_on = lsj_cfg(dict(g, crop_enabled=np.int64(1)), key=True)
    crop_on.defrost()
    crop_on.INPUT.COLOR_JITTER = True
    crop_on.freeze()      # the reference's order: crop, colour jitter, resize scale, fixed-size crop, flip
    assert names(build_augmentation(crop_on, True, color_jitter=True, lsj=True)) == ["RandomCrop", "ColorJitter", "ResizeScale", "FixedSizeCrop",
                                                                                     "RandomFlip"]
    with pytest.raises(TypeError):
        build_augmentation(on, True, lsj="yes")
    with pytest.raises(ValueError):
        LargeScaleJitter(pad_value=128.5)
    np.random.seed(int(g["seed"]))
    out, _, p = DatasetMapper.from_config(on, True, lsj=True).draw(case_dict(g))
    assert list(p.scaled) == g["scaled"].tolist() and list(p.lsj[0]) == g["window"].tolist() and int(p.flip) == int(g["flip"])
    assert p.lsj[1:] == ((800, 800), 128) and p.new_size == (800, 800)
    assert out["instances"].gt_boxes.tensor.numpy().tobytes() == g["gt_boxes"].tobytes()


def _loader_calls(cfg, **kw):
    from lvc_amd.data import DatasetMapper, DatasetMapperMosaic, build_detection_train_loader, build_detection_train_mosaic_loader

    data = [{"raw": torch.zeros(8, 8, 3, dtype=torch.uint8), "width": 8, "height": 8}]
    return [lambda: DatasetMapper.from_config(cfg, True, **kw), lambda: DatasetMapperMosaic.from_config(cfg, True, **kw),
            lambda: build_detection_train_loader(cfg, data, seed=0, **kw), lambda: build_detection_train_mosaic_loader(cfg, data, seed=0, **kw)]


def test_lsj_none_still_raises_and_says_how_to_opt_in():
    c = lsj_cases()[0]
    for kw in ({}, {"lsj": None}, {"lsj": False}, {"color_jitter": True}):
        for call in _loader_calls(lsj_cfg(c, key=True), **kw):
            with pytest.raises(NotImplementedError, match=r"INPUT\.LSJ.*lsj=True"):
                call()


def test_blur_raises_under_every_lsj_setting():
    from lvc_amd.data import LargeScaleJitter

    c = lsj_cases()[0]
    for key in (False, True):
        cfg = lsj_cfg(c, key=key)
        cfg.defrost()
        cfg.INPUT.BLUR = True
        cfg.freeze()
        for kw in ({}, {"lsj": True}, {"lsj": LargeScaleJitter(0.5, 1.6, 72, 100)}, {"lsj": True, "color_jitter": True}):
            if key and not kw:
                continue      # that one names INPUT.LSJ or INPUT.BLUR, whichever the list has first
            for call in _loader_calls(cfg, **kw):
                with pytest.raises(NotImplementedError, match=r"INPUT\.BLUR"):
                    call()


# ------------------------------------------------------------------------------------------------ the job table
FAKE = 0x10000      # a non-null "device pointer": nothing below launches


def _case_item(c, p=None):
    """The job of a fixture case from its own numbers, over tile descriptors in place of device tensors."""
    from lvc_amd.data.mosaic import mosaic_layout

    geom = (tuple(c["scaled"].tolist()), tuple(c["window"].tolist()), tuple(c["target"].tolist()), 128, bool(c["flip"]))
    x0, y0, cw, ch = c["crop"].tolist()
    if int(c["jitter"]):      # the jittered crop is a packed image of the window's size
        return ([((FAKE, ch, cw, cw * 3, 3, 1), (0, 0, cw, ch), (0, 0))], (0, 0, cw, ch)) + geom
    if c["tiles"]:
        shapes = [t["image"].shape[:2] for t in c["tiles"]]
        lay = mosaic_layout(shapes)
        tiles = [((FAKE, h, w, w * 3, 3, 1), r, o) for (h, w), r, o in zip(shapes, lay.rect, lay.origin)]
        return (tiles, (x0 + lay.trim_origin[0], y0 + lay.trim_origin[1], cw, ch)) + geom
    h, w = c["image"].shape[:2]
    return ([((FAKE, h, w, w * 3, 3, 1), (0, 0, w, h), (0, 0))], (x0, y0, cw, ch)) + geom


def _blob(items):
    from lvc_amd import kernels as K
    from lvc_amd.data import resample_coeffs

    tab, tables, off, tmp = K.train_input_lsj_blob(items, resample_coeffs)
    blob = np.zeros(off // 8 + 1, np.int64)      # 8-byte aligned
    raw = blob.view(np.uint8)
    raw[:tab.nbytes] = tab.reshape(-1).view(np.uint8)
    at = tab.nbytes
    for t in tables:
        raw[at:at + t.nbytes] = np.ascontiguousarray(t, np.int32).reshape(-1).view(np.uint8)
        at += t.nbytes
    assert at == off
    return tab, blob, off, tmp


def test_windows_bands_and_taps_of_every_fixture_case_lie_inside_their_sources():
    from lvc_amd import kernels as K
    from lvc_amd.data import resample_coeffs

    cs = lsj_cases()
    items = [_case_item(c) for c in cs]
    tab, blob, off, tmp = _blob(items)
    assert tab.shape == (len(cs), K.TRAIN_INPUT_LSJ_FIELDS) and K.TRAIN_INPUT_LSJ_FIELDS == 140
    for c, row in zip(cs, tab):
        name = str(c["name"])
        X0, Y0, cw, ch, sh, sw = row[0:6].tolist()
        ox, oy, ow, oh, th, tw, fill, by0, bh = row[17:26].tolist()
        assert 0 <= ox and ox + ow <= sw and 0 <= oy and oy + oh <= sh and ow <= tw and oh <= th and fill == 128, name
        assert 0 <= by0 and bh > 0 and by0 + bh <= ch, name
        assert (row[6] < 0) == (sw == cw) and (row[9] < 0) == (sh == ch), name
        if sw != cw:      # column taps of the window inside the crop window
            b = resample_coeffs(cw, sw)[0][ox:ox + ow]
            assert b[:, 0].min() >= 0 and (b[:, 0] + b[:, 1]).max() <= cw, name
        if sh != ch:      # row taps of the window inside the band, and the band is tight
            b = resample_coeffs(ch, sh)[0][oy:oy + oh]
            assert b[:, 0].min() == by0 and (b[:, 0] + b[:, 1]).max() == by0 + bh, name
            if oh < sh:
                assert bh < ch, name      # a cropped axis reads fewer source rows than the crop window has
        else:
            assert (by0, bh) == (oy, oh), name
    # bytes of the intermediates: the bands, not the scaled images
    assert tmp == sum((int(r[25]) * int(r[19]) * 3 + 255) & ~255 for r in tab)
    full = sum(int(r[3]) * int(r[5]) * 3 for r in tab)
    assert sum(int(r[25]) * int(r[19]) * 3 for r in tab) < full


def _call(blob, nbytes, B, tmp_bytes, Hp=96, Wp=128, n_slots=None):
    from lvc_amd import _lib

    m, s, n = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), ctypes.c_int(-1)
    rc = _lib.lib().lvc_train_input_lsj_u8(ctypes.c_void_p(blob.ctypes.data), ctypes.c_void_p(FAKE), ctypes.c_longlong(nbytes),
                                           ctypes.c_int(B), ctypes.c_void_p(FAKE), ctypes.c_longlong(tmp_bytes), ctypes.c_void_p(FAKE),
                                           ctypes.c_int(n_slots or B), ctypes.c_int(Hp), ctypes.c_int(Wp), m, s, ctypes.byref(n),
                                           ctypes.c_void_p(0))
    return rc, n.value, _lib.lib().lvc_last_error().decode()


def test_the_entry_refuses_a_corrupted_blob_with_its_error_code_before_any_launch():
    """Every field the kernels index with is checked on the host copy: a hand-corrupted table comes back as LVC_ERR_INVALID (1) with
    no launch counted.  The pointers are fake: a launch would not survive them, and none is made (the good table is NOT sent)."""
    from lvc_amd import kernels as K

    HEAD = K.TRAIN_INPUT_LSJ_HEAD
    cs = {str(c["name"]): c for c in lsj_cases()}
    good = [_case_item(cs["crop_both_box_removed"]), _case_item(cs["height_unchanged"])]
    tab, blob, off, tmp = _blob(good)
    words = blob[:tab.size].reshape(tab.shape)
    yb = int(tab[0, 9])
    bad = [
        ("window past the scaled width", (0, 17), int(tab[0, 5] - tab[0, 19] + 1), "output window"),
        ("window past the scaled height", (0, 18), int(tab[0, 4] - tab[0, 20] + 1), "output window"),
        ("negative window origin", (0, 17), -1, "output window"),
        ("window wider than the canvas", (0, 22), int(tab[0, 19] - 1), "canvas"),
        ("canvas taller than the padded batch", (0, 21), 97, "canvas"),
        ("fill that is no byte", (0, 23), 256, "fill"),
        ("band past the crop window", (0, 25), int(tab[0, 3] + 1), "band"),
        ("band that misses the first tap", (0, 24), int(tab[0, 24] + 1), "band|row taps"),
        ("band one row short", (0, 25), int(tab[0, 25] - 1), "row taps"),
        ("rows outside the band where the height stays", (1, 24), int(tab[1, 24] + 1), "band|output rows"),
        ("scaled size that contradicts the tables", (0, 5), int(tab[0, 2]), "coefficients|output window"),
        ("no tiles", (0, 16), 0, "tiles"),
        ("null tile pointer", (0, HEAD), 0, "tile"),
        ("two jobs on one slot", (1, 13), 0, "slot"),
        ("slot outside the batch", (1, 13), 2, "slot"),
        ("intermediate outside the scratch buffer", (1, 15), 1 << 40, "intermediate"),
        ("table offset outside the blob", (0, 10), off, "row tables"),
        ("two intermediates on the same bytes", (1, 15), int(tab[0, 15]), "intermediate"),
        ("an intermediate that begins inside another", (1, 15), int(tab[1, 15]) - 256, "intermediate"),
    ]
    for what, (job, word), value, msg in bad:
        keep = int(words[job, word])
        words[job, word] = value
        rc, launches, err = _call(blob, off, 2, tmp)
        words[job, word] = keep
        assert rc == 1 and launches == 0, (what, rc, launches)
        assert "lvc_train_input_lsj_u8" in err and re.search(msg, err), (what, err)
    # a tap range edited inside the tables themselves, and buffers that are too small
    b = blob.view(np.int32)
    r = yb // 4 + 2 * int(tab[0, 18])
    keep, b[r] = int(b[r]), int(tab[0, 24]) - 1
    assert _call(blob, off, 2, tmp)[:2] == (1, 0)
    b[r] = keep
    assert _call(blob, off, 2, tmp - 256)[:2] == (1, 0)
    assert _call(blob, tab.nbytes - 8, 2, tmp)[:2] == (1, 0)
    assert _call(blob, off, 2, tmp, n_slots=1)[:2] == (1, 0)
    assert _call(blob, off, 2, tmp, Hp=71)[:2] == (1, 0)
    assert words.tolist() == tab.tolist()      # every edit was undone: what was refused differs from an accepted table by one word


def test_header_declares_the_entry_and_kernels_binds_it():
    from lvc_amd import _lib
    from lvc_amd import kernels as K

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvc_amd.h")).read(), flags=re.S)
    assert "int lvc_train_input_lsj_u8(" in txt
    assert hasattr(_lib.lib(), "lvc_train_input_lsj_u8")
    assert callable(K.train_input_lsj_u8) and K.TRAIN_INPUT_LSJ_HEAD == 32 and K.TRAIN_INPUT_LSJ_LAUNCHES == K.TRAIN_INPUT_LSJ_LAUNCHES[:64]
    import lvc_amd.data as D

    assert "LargeScaleJitter" in D.__all__ and D.LargeScaleJitter is not None
