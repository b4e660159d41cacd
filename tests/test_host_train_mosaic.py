"""Mosaic training input, host side (lvc_amd/data/mosaic.py, build.py) against the reference's get_mosaic / get_mosaic9,
DatasetMapperMosaic and MapDatasetMosaic + AspectRatioGroupedDataset (tests/golden/train_mosaic.npz, scripts/
make_golden_train_mosaic.py).  No GPU needed."""
import ctypes
import itertools
import os
import random

import numpy as np
import pytest
import torch

from helpers import GOLD
from test_host_train_input import case_cfg, gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mosaic_cases():
    """Every fixture case as a dict of its arrays (prefix stripped), its tiles under "tiles" as dicts of theirs."""
    g = gold("train_mosaic")
    out = []
    for k in range(int(g["n"])):
        p = "c%d_" % k
        c = {key[len(p):]: g[key] for key in g if key.startswith(p)}
        c["tiles"] = []
        for t in range(int(c["n_tiles"])):
            q = "t%d_" % t
            c["tiles"].append({key[len(q):]: c[key] for key in c if isinstance(key, str) and key.startswith(q)})
        out.append(c)
    return out


def tile_dicts(c):
    """The dataset dicts the reference's mapper was given, with the images under "raw" instead of files."""
    out = []
    for t in c["tiles"]:
        annos = []
        for bbox, mode, cat, crowd, ign, id_ in zip(t["ann_bbox"], t["ann_mode"], t["ann_cat"], t["ann_iscrowd"], t["ann_ignore"],
                                                    t["ann_id"]):
            a = {"bbox": [float(v) for v in bbox], "bbox_mode": int(mode), "category_id": int(cat)}
            if crowd >= 0:
                a["iscrowd"] = int(crowd)
            if ign >= 0:
                a["ignore_qe"] = int(ign)
            if id_ != -1000:
                a["id"] = int(id_)
            annos.append(a)
        h, w = t["image"].shape[:2]
        out.append({"raw": torch.from_numpy(t["image"]), "height": h, "width": w, "image_id": int(t["image_id"]), "annotations": annos})
    return out


def mosaic_cfg(c, device="cpu", mosaic=0.5, split=1.0):
    cfg = case_cfg(c, device)
    cfg.defrost()
    cfg.INPUT.MOSAIC, cfg.INPUT.MOSAIC49SPLIT = mosaic, split
    cfg.freeze()
    return cfg


def test_fixture_covers_the_cases_the_feature_names():
    cs = {str(c["name"]): c for c in mosaic_cases()}
    assert {int(c["n_tiles"]) for c in cs.values()} == {4, 9}
    c = cs["m4_equal_noresample_noflip"]
    assert len({t["image"].shape for t in c["tiles"]}) == 1 and not int(c["crop_enabled"]) and not int(c["flip"])
    assert c["new_size"].tolist() == c["composite_size"].tolist() == list(c["out_image"].shape[1:])
    c = cs["m4_mixed_crop_flip"]
    shapes = [t["image"].shape[:2] for t in c["tiles"]]
    assert any(h > w for h, w in shapes) and any(w > h for h, w in shapes) and int(c["flip"]) == 1
    assert any(h > shapes[0][0] or w > shapes[0][1] for h, w in shapes[1:])
    assert str(c["crop_type"]) == "relative_range" and c["crop_size"].tolist() == [0.7, 0.7]
    c = cs["m4_tile0_smallest"]
    shapes = [t["image"].shape[:2] for t in c["tiles"]]
    assert all(h * w > shapes[0][0] * shapes[0][1] for h, w in shapes[1:])
    c = cs["m9_mixed_crop_noflip"]
    assert int(c["crop_enabled"]) and not int(c["flip"]) and int(c["fill_in_window"]) and int(c["clipped_to_nothing"]) > 0
    assert len(c["gt_classes"]) < int(c["candidates"])
    c = cs["m9_width_unchanged"]
    assert c["new_size"][1] == c["crop"][2] and c["new_size"][0] != c["crop"][3]
    for c in cs.values():      # every annotation flavour in every case
        modes = np.concatenate([t["ann_mode"] for t in c["tiles"]])
        crowd = np.concatenate([t["ann_iscrowd"] for t in c["tiles"]])
        ign = np.concatenate([t["ann_ignore"] for t in c["tiles"]])
        ids = np.concatenate([t["ann_id"] for t in c["tiles"]])
        assert (modes == 0).sum() == 1 and (crowd == 1).sum() == 1
        assert (ign >= 0).any() and (ign < 0).any() and (ids != -1000).any() and (ids == -1000).any()
        for t in c["tiles"]:
            assert all(20 <= v <= 90 for v in t["image"].shape[:2])
    g = gold("train_mosaic")      # the reference's geometry never overlaps two canvas rectangles (see the generator's docstring)
    assert int(g["overlap_lists"]) >= 400 and int(g["overlap_found"]) == 0


def test_layouts_equal_the_reference():
    from lvc_amd.data import mosaic4_layout, mosaic9_layout

    for c in mosaic_cases():
        sizes = [t["image"].shape[:2] for t in c["tiles"]]
        lay = (mosaic4_layout if len(sizes) == 4 else mosaic9_layout)(sizes)
        name = str(c["name"])
        assert [list(r) for r in lay.canvas] == c["canvas"].tolist(), name
        assert [list(r) for r in lay.source] == c["source"].tolist(), name
        assert list(lay.trim) == c["trim"].tolist(), name
        assert list(lay.size) == c["composite_size"].tolist(), name
        for v in itertools.chain(*lay.canvas, *lay.source, lay.trim):
            assert type(v) is int, name


def test_numpy_composite_equals_the_reference():
    """The no-resample case's reference output IS the composite (no crop, no flip, neither axis resampled)."""
    from lvc_amd.data.mosaic import compose, mosaic_layout

    c = [c for c in mosaic_cases() if str(c["name"]) == "m4_equal_noresample_noflip"][0]
    imgs = [t["image"] for t in c["tiles"]]
    got = compose(imgs, mosaic_layout([i.shape[:2] for i in imgs]))
    assert np.array_equal(got, c["out_image"].transpose(1, 2, 0))
    # a 9-tile composite holds every tile's source rectangle where the layout says, and 114 where no tile is
    c = [c for c in mosaic_cases() if int(c["n_tiles"]) == 9][0]
    imgs = [t["image"] for t in c["tiles"]]
    lay = mosaic_layout([i.shape[:2] for i in imgs])
    comp = compose(imgs, lay)
    covered = np.zeros(comp.shape[:2], bool)
    for img, (x1a, y1a, x2a, y2a), (x1b, y1b, x2b, y2b) in zip(imgs, c["canvas"].tolist(), c["source"].tolist()):
        ox, oy = x1a - lay.trim[0], y1a - lay.trim[1]
        assert np.array_equal(comp[oy:oy + y2a - y1a, ox:ox + x2a - x1a], img[y1b:y2b, x1b:x2b])
        covered[oy:oy + y2a - y1a, ox:ox + x2a - x1a] = True
    assert (~covered).any() and bool((comp[~covered] == 114).all())


def test_annotations_equal_the_reference_bit_for_bit():
    from lvc_amd.data import DatasetMapperMosaic

    for c in mosaic_cases():
        mapper = DatasetMapperMosaic.from_config(mosaic_cfg(c), True)
        dicts = tile_dicts(c)
        keep = [[a["bbox"][:] for a in d["annotations"]] for d in dicts]
        np.random.seed(int(c["seed"]))
        out, tiles, p = mapper.draw(dicts)
        name = str(c["name"])
        assert list(p.crop) == c["crop"].tolist() and list(p.new_size) == c["new_size"].tolist() and int(p.flip) == int(c["flip"]), name
        assert len(tiles) == int(c["n_tiles"]) and all(torch.equal(t, d["raw"]) for t, d in zip(tiles, dicts)), name
        inst = out["instances"]
        assert inst.image_size == tuple(c["new_size"].tolist()), name
        b = inst.gt_boxes.tensor
        assert b.dtype == torch.float32 and tuple(b.shape) == c["gt_boxes"].shape, name
        assert b.numpy().tobytes() == c["gt_boxes"].tobytes(), name
        assert inst.gt_classes.tolist() == c["gt_classes"].tolist(), name
        assert inst.gt_ignores.tolist() == c["gt_ignores"].tolist(), name
        assert inst.ids.tolist() == c["ids"].tolist(), name
        assert (out["image_id"], out["width"], out["height"]) == (int(c["out_image_id"]), int(c["out_width"]), int(c["out_height"])), name
        assert "annotations" not in out and "raw" not in out
        assert [[a["bbox"] for a in d["annotations"]] for d in dicts] == keep, "the caller's dicts were modified"


def test_tile_index_stream_and_grouped_batches_equal_the_reference():
    from lvc_amd.data import MapDatasetMosaic, TrainingSampler
    from lvc_amd.data.build import MosaicTrainInputLoader

    g = gold("train_mosaic")
    N, bs = len(g["order_width"]), int(g["order_batch_size"])
    dicts = [{"width": int(w), "height": int(h)} for w, h in zip(g["order_width"], g["order_height"])]
    c = dict(mosaic_cases()[0])
    cfg = mosaic_cfg(c, mosaic=float(g["order_mosaic"]), split=float(g["order_split"]))
    for world in (1, 2):
        for rank in range(world):
            ref_tiles = [[int(v) for v in row if v >= 0] for row in g["order_w%d_r%d_tiles" % (world, rank)]]
            ref_batches = g["order_w%d_r%d_batches" % (world, rank)].tolist()
            mds = MapDatasetMosaic(dicts, lambda ds: [d for d in ds], lambda d: [d], cfg)
            random.seed(int(g["order_pyseed"]))
            idx = itertools.islice(TrainingSampler(N, seed=int(g["order_seed"]), rank=rank, world_size=world), len(ref_tiles))
            assert [mds.draw_indices(i) for i in idx] == ref_tiles, (world, rank)
            # and through the loader's own batching: the mosaic draws in sampler order, then the grouping by the LAST tile's size
            loader = MosaicTrainInputLoader.__new__(MosaicTrainInputLoader)
            loader.dataset_dicts, loader.batch_size, loader.grouping = dicts, bs, True
            loader.map_dataset = MapDatasetMosaic(dicts, None, None, cfg)
            loader.sampler = TrainingSampler(N, seed=int(g["order_seed"]), rank=rank, world_size=world)
            random.seed(int(g["order_pyseed"]))
            got = list(itertools.islice(loader.index_batches(), len(ref_batches)))
            assert got == [[ref_tiles[r] for r in b] for b in ref_batches], (world, rank)
    # through __getitem__: the map functions get what the reference's get
    mds = MapDatasetMosaic(list(range(100, 111)), lambda ds: ("mosaic", ds), lambda d: ("plain", d), cfg)
    random.seed(3)
    kinds = [mds[i] for i in range(11)]
    random.seed(3)
    again = [mds.draw_indices(i) for i in range(11)]
    assert [len(k[1]) if k[0] == "mosaic" else 1 for k in kinds] == [len(a) for a in again]
    assert all((k[1] if k[0] == "mosaic" else [k[1]]) == [100 + i for i in a] for k, a in zip(kinds, again))


def test_short_dataset_raises_as_random_sample_does():
    from lvc_amd.data import MapDatasetMosaic

    cfg = mosaic_cfg(dict(mosaic_cases()[0]), mosaic=1.0, split=0.0)      # always 9 tiles
    mds = MapDatasetMosaic(list(range(7)), None, None, cfg)
    with pytest.raises(ValueError):
        mds.draw_indices(0)


def test_rejected_shapes_raise_value_error():
    """numpy refuses `canvas[rect] = tile[source]` when the two shapes differ; so does the layout.  Random search (the generator's,
    and the one below) finds no tile-size list for which the reference's own rectangles disagree, so the mismatch is made by hand:
    a layout whose source rectangle is one pixel short, and a tile whose image is not the size its dict says."""
    from lvc_amd.data import DatasetMapperMosaic
    from lvc_amd.data.mosaic import MosaicLayout, mosaic_layout

    rng = random.Random(0)
    for _ in range(300):
        n = rng.choice([4, 9])
        lo, hi = rng.choice([(20, 90), (1, 8), (1, 200)])
        mosaic_layout([(rng.randint(lo, hi), rng.randint(lo, hi)) for _ in range(n)])
    with pytest.raises(ValueError, match="shape"):
        MosaicLayout([(0, 0, 10, 10)], [(0, 0, 9, 10)], [(10, 10)], (0, 0, 10, 10), 20)
    with pytest.raises(ValueError, match="shape"):      # a source end past the image is clamped: 8 columns for a 10-column rectangle
        MosaicLayout([(0, 0, 10, 10)], [(2, 0, 12, 10)], [(10, 10)], (0, 0, 10, 10), 20)
    lay = MosaicLayout([(5, 5, 9, 9)], [(-4, -4, 10, 10)], [(10, 10)], (5, 5, 9, 9), 20)      # a negative start wraps
    assert lay.origin == [(6, 6)] and lay.rect == [(5, 5, 9, 9)]
    c = mosaic_cases()[0]
    dicts = tile_dicts(c)
    dicts[2]["width"] += 1
    with pytest.raises(ValueError, match="Mismatched image shape"):
        DatasetMapperMosaic.from_config(mosaic_cfg(c), True).draw(dicts)
    with pytest.raises(ValueError, match="4 or 9"):
        DatasetMapperMosaic.from_config(mosaic_cfg(c), True).draw(tile_dicts(c)[:3])


def test_unbuilt_keys_still_raise_and_the_plain_entry_points_point_here():
    from lvc_amd.data import DatasetMapper, build_detection_train_loader, build_detection_train_mosaic_loader

    data = [{"raw": torch.zeros(4, 4, 3, dtype=torch.uint8), "width": 4, "height": 4}]
    c = dict(mosaic_cases()[0])
    for key in ("COLOR_JITTER", "BLUR", "LSJ"):
        cfg = mosaic_cfg(c)
        cfg.defrost()
        setattr(cfg.INPUT, key, True)
        cfg.freeze()
        with pytest.raises(NotImplementedError, match=r"INPUT\.%s" % key):
            build_detection_train_mosaic_loader(cfg, data, seed=0)
    cfg = mosaic_cfg(c)
    cfg.defrost()
    cfg.DATALOADER.SAMPLER_TRAIN = "RepeatFactorTrainingSampler"
    cfg.freeze()
    with pytest.raises(NotImplementedError, match="SAMPLER_TRAIN"):
        build_detection_train_mosaic_loader(cfg, data, seed=0)
    for call in (lambda: DatasetMapper.from_config(mosaic_cfg(c), True), lambda: build_detection_train_loader(mosaic_cfg(c), data, seed=0)):
        with pytest.raises(NotImplementedError, match=r"INPUT\.MOSAIC.*build_detection_train_mosaic_loader"):
            call()


def test_header_declares_the_new_symbol():
    text = open(os.path.join(ROOT, "include", "lvc_amd.h")).read()
    assert "int lvc_train_input_tiles_u8(" in text and "int lvc_train_input_u8(" in text
    from lvc_amd import kernels as K

    assert K.TRAIN_INPUT_TILES_FIELDS == 128 and K.TRAIN_INPUT_FIELDS == 24
    assert "[B][128]" in text


def test_the_three_tiled_entries_refuse_the_same_tile_lists_under_their_own_names():
    """lvc_train_input_tiles_u8, lvc_train_input_lsj_u8 and lvc_color_jitter_tiles_u8 check a crop window and its tiles alike: one
    40 x 50 tile under the window (10, 10, 50, 40), the same word of the tile list corrupted for each entry, comes back as
    LVC_ERR_INVALID (1) with no launch counted and the same message under the entry's own name.  The pointers are fake: a launch
    would not survive them, and none is made (the good table is NOT sent)."""
    from lvc_amd import _lib
    from lvc_amd import kernels as K

    FAKE = 0x10000
    window, tile = (10, 10, 50, 40), (FAKE, 40, 50, 150, 3, 1, 10, 10, 60, 50, 0, 0)
    lib = _lib.lib()
    v, ll, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    m, s = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)

    def resample_entry(fn):
        return lambda blob, n: fn(v(blob.ctypes.data), v(FAKE), ll(blob.nbytes), ci(1), v(FAKE), ll(40 * 50 * 3), v(FAKE), ci(1), ci(40),
                                  ci(50), m, s, ctypes.byref(n), v(0))

    tiles = np.zeros((1, K.TRAIN_INPUT_TILES_FIELDS), np.int64)
    tiles[0, 0:6], tiles[0, 6], tiles[0, 9], tiles[0, 16] = window + (40, 50), -1, -1, 1
    lsj = K.train_input_lsj_blob([([(tile[:6], tile[6:10], tile[10:12])], window, (40, 50), (0, 0, 50, 40), (40, 50), 128, False)],
                                 None)[0]
    jitter = np.zeros((1, K.COLOR_JITTER_FIELDS), np.int64)
    jitter[0, 0:4], jitter[0, 14] = window, 1
    entries = [
        ("lvc_train_input_tiles_u8", tiles, K.TRAIN_INPUT_TILES_HEAD, 16, resample_entry(lib.lvc_train_input_tiles_u8)),
        ("lvc_train_input_lsj_u8", lsj, K.TRAIN_INPUT_LSJ_HEAD, 16, resample_entry(lib.lvc_train_input_lsj_u8)),
        ("lvc_color_jitter_tiles_u8", jitter, K.TRAIN_INPUT_TILES_HEAD, 14,
         lambda blob, n: lib.lvc_color_jitter_tiles_u8(v(blob.ctypes.data), v(FAKE), ll(blob.nbytes), ci(1), v(FAKE), ll(40 * 50 * 3),
                                                       ctypes.byref(n), v(0))),
    ]
    bad = [      # (what, word of the tile (None: the tile count), value, message)
        ("null source", 0, 0, "bad tile image"),
        ("zero row stride", 3, 0, "strides must be positive"),
        ("negative channel stride", 5, -1, "strides must be positive"),
        ("rectangle of negative extent", 8, 9, "negative extent"),
        ("a coordinate at 2^30", 6, 1 << 30, "coordinate out of range"),
        ("the window reads above the tile", 11, -1, "a tile is read outside its image"),
        ("no tile", None, 0, "1 to 9 tiles"),
        ("ten tiles", None, 10, "1 to 9 tiles"),
    ]
    for what, word, value, msg in bad:
        said = set()
        for name, tab, head, nt_word, call in entries:
            tab[0, head:head + 12] = tile
            good = tab.copy()
            at = nt_word if word is None else head + word
            tab[0, at] = value
            n = ctypes.c_int(-1)
            rc = call(tab, n)
            err = lib.lvc_last_error().decode()
            tab[0, at] = good[0, at]
            assert rc == 1 and n.value == 0, (what, name, rc, n.value)
            assert err.startswith(name + ": ") and msg in err, (what, name, err)
            assert tab.tolist() == good.tolist()      # the edit was undone: what was refused differs from the good table by one word
            said.add(err[len(name):])
        assert len(said) == 1, (what, said)      # one checker: the same words from all three
