"""Training input, host side (lvc_amd/data/transforms.py, dataset_mapper.py, build.py) against the reference's DatasetMapperIgnore and
TrainingSampler + AspectRatioGroupedDataset (tests/golden/train_input_*.npz, scripts/make_golden_train_input.py).  No GPU needed."""
import itertools

import numpy as np
import pytest
import torch

from helpers import GOLD

FIXTURES = ("train_input_nocrop", "train_input_crop")


def gold(name):
    import os

    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def cases():
    """Every fixture case as a dict of its arrays (prefix stripped)."""
    out = []
    for f in FIXTURES:
        g = gold(f)
        for k in range(int(g["n"])):
            p = "c%d_" % k
            out.append({key[len(p):]: g[key] for key in g if key.startswith(p)})
    return out


def case_cfg(c, device="cpu"):
    from lvc_amd.config.presets import base_rcnn_fpn

    cfg = base_rcnn_fpn()
    cfg.defrost()
    cfg.MODEL.DEVICE = device
    cfg.INPUT.MIN_SIZE_TRAIN = tuple(int(v) for v in c["min_sizes"])
    cfg.INPUT.MAX_SIZE_TRAIN = int(c["max_size"])
    cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING = str(c["sampling"])
    cfg.INPUT.CROP.ENABLED = bool(c["crop_enabled"])
    cfg.INPUT.CROP.TYPE = str(c["crop_type"])
    cfg.INPUT.CROP.SIZE = [float(v) for v in c["crop_size"]]
    cfg.freeze()
    return cfg


def case_dict(c):
    """The dataset dict the reference's mapper was given, with the image under "raw" instead of a file."""
    annos = []
    for bbox, mode, cat, crowd, ign, id_ in zip(c["ann_bbox"], c["ann_mode"], c["ann_cat"], c["ann_iscrowd"], c["ann_ignore"], c["ann_id"]):
        a = {"bbox": [float(v) for v in bbox], "bbox_mode": int(mode), "category_id": int(cat)}
        if crowd >= 0:
            a["iscrowd"] = int(crowd)
        if ign >= 0:
            a["ignore_qe"] = int(ign)
        if id_ != -1000:
            a["id"] = int(id_)
        annos.append(a)
    h, w = c["image"].shape[:2]
    return {"raw": torch.from_numpy(c["image"]), "height": h, "width": w, "image_id": 0, "annotations": annos}


def test_fixture_covers_the_cases_the_feature_names():
    cs = cases()
    names = {str(c["name"]) for c in cs}
    assert len(cs) == len(names) >= 12
    assert {str(c["crop_type"]) for c in cs if c["crop_enabled"]} == {"relative_range", "relative", "absolute", "absolute_range"}
    for crop in (0, 1):
        assert {int(c["flip"]) for c in cs if int(c["crop_enabled"]) == crop} == {0, 1}
    assert any(int(c["crop_enabled"]) == 0 and c["new_size"][0] > c["image"].shape[0] for c in cs)      # up-scaling
    assert any(int(c["crop_enabled"]) == 0 and c["new_size"][0] < c["image"].shape[0] for c in cs)      # down-scaling
    assert any(max(c["new_size"]) == int(c["max_size"]) for c in cs)                                   # MAX_SIZE_TRAIN clamp
    assert any(str(c["sampling"]) == "choice" and len(c["min_sizes"]) > 2 for c in cs)
    assert any(str(c["sampling"]) == "range" for c in cs)
    assert any(len(c["ann_cat"]) > 0 and len(c["gt_classes"]) == 0 for c in cs)                         # nothing left
    assert any((c["ann_iscrowd"] == 1).any() for c in cs) and any((c["ann_ignore"] == 1).any() for c in cs)
    cut = False
    for c in cs:      # a box the crop cuts: a kept box that touches the border of a cropped image
        if int(c["crop_enabled"]) and len(c["gt_boxes"]):
            h, w = c["new_size"]
            b = c["gt_boxes"]
            cut = cut or bool(((b[:, 0] == 0) | (b[:, 1] == 0) | (b[:, 2] == w) | (b[:, 3] == h)).any())
    assert cut


def test_seeded_draws_equal_the_reference():
    from lvc_amd.data import AugmentationList, build_augmentation

    for c in cases():
        aug = AugmentationList(build_augmentation(case_cfg(c), True))
        h, w = c["image"].shape[:2]
        np.random.seed(int(c["seed"]))
        _, p = aug.draw(h, w)
        name = str(c["name"])
        assert list(p.crop) == c["crop"].tolist(), name
        assert list(p.new_size) == c["new_size"].tolist(), name
        assert int(p.flip) == int(c["flip"]), name


def test_annotations_equal_the_reference_bit_for_bit():
    from lvc_amd.data import DatasetMapper

    for c in cases():
        mapper = DatasetMapper.from_config(case_cfg(c), True)
        d = case_dict(c)
        keep = [a["bbox"][:] for a in d["annotations"]]
        np.random.seed(int(c["seed"]))
        out, raw, p = mapper.draw(d)
        name = str(c["name"])
        inst = out["instances"]
        assert inst.image_size == tuple(c["new_size"].tolist()), name
        b = inst.gt_boxes.tensor
        assert b.dtype == torch.float32 and tuple(b.shape) == c["gt_boxes"].shape, name
        assert b.numpy().tobytes() == c["gt_boxes"].tobytes(), name
        assert inst.gt_classes.dtype == torch.int64 and inst.gt_classes.tolist() == c["gt_classes"].tolist(), name
        assert inst.gt_ignores.dtype == torch.int64 and inst.gt_ignores.tolist() == c["gt_ignores"].tolist(), name
        assert inst.ids.tolist() == c["ids"].tolist(), name
        assert "annotations" not in out and "raw" not in out and out["height"] == c["image"].shape[0]
        assert [a["bbox"] for a in d["annotations"]] == keep, "the caller's dict was modified"


def test_transforms_compose_through_transform_list():
    from lvc_amd.data import CropTransform, HFlipTransform, ResizeTransform, TransformList

    tl = TransformList([CropTransform(10, 20, 100, 50), ResizeTransform(50, 100, 100, 200), HFlipTransform(200)])
    box = np.array([[30.0, 30.0, 60.0, 50.0]])
    assert tl.apply_box(box).tolist() == [[200 - 100.0, 20.0, 200 - 40.0, 60.0]]
    pts = np.array([[10.0, 20.0], [110.0, 70.0]])
    assert tl.apply_coords(pts).tolist() == [[200.0, 0.0], [0.0, 100.0]]
    img = np.arange(80 * 120 * 3, dtype=np.uint8).reshape(80, 120, 3)
    assert np.array_equal(CropTransform(10, 20, 100, 50).apply_image(img), img[20:70, 10:110])
    t = torch.from_numpy(img)
    assert torch.equal(CropTransform(10, 20, 100, 50).apply_image(t), t[20:70, 10:110])


def test_loader_order_equals_the_reference():
    from lvc_amd.data import AspectRatioGrouper, TrainingSampler
    from lvc_amd.data.build import TrainInputLoader

    g = gold("train_input_order")
    N, bs, seed = len(g["width"]), int(g["batch_size"]), int(g["seed"])
    dicts = [{"width": int(w), "height": int(h)} for w, h in zip(g["width"], g["height"])]
    for world in (1, 2):
        for rank in range(world):
            idx = list(itertools.islice(TrainingSampler(N, seed=seed, rank=rank, world_size=world), 3 * N))
            rows = [dict(dicts[i], index=i) for i in idx]
            got = [[r["index"] for r in b] for b in AspectRatioGrouper(rows, bs)]
            assert got == g["w%d_r%d_g1" % (world, rank)].tolist(), (world, rank)
            for grouped in (1, 0):      # and through the loader's own batching of the infinite stream
                ref = g["w%d_r%d_g%d" % (world, rank, grouped)].tolist()
                loader = TrainInputLoader.__new__(TrainInputLoader)
                loader.dataset_dicts, loader.batch_size, loader.grouping = dicts, bs, bool(grouped)
                loader.sampler = TrainingSampler(N, seed=seed, rank=rank, world_size=world)
                assert list(itertools.islice(loader.index_batches(), len(ref))) == ref, (world, rank, grouped)


@pytest.mark.parametrize("key,value", [("INPUT.COLOR_JITTER", True), ("INPUT.BLUR", True), ("INPUT.LSJ", True), ("INPUT.MOSAIC", 0.5),
                                       ("MODEL.MASK_ON", True), ("MODEL.KEYPOINT_ON", True), ("MODEL.LOAD_PROPOSALS", True)])
def test_out_of_scope_keys_raise(key, value):
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.data import DatasetMapper, build_detection_train_loader

    cfg = base_rcnn_fpn()
    cfg.defrost()
    node = cfg
    parts = key.split(".")
    for p in parts[:-1]:
        node = getattr(node, p)
    setattr(node, parts[-1], value)
    cfg.MODEL.DEVICE = "cpu"
    cfg.freeze()
    with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")):
        DatasetMapper.from_config(cfg, True)
    with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")):
        build_detection_train_loader(cfg, [{"raw": torch.zeros(4, 4, 3, dtype=torch.uint8), "width": 4, "height": 4}], seed=0)


def test_file_name_only_dicts_and_vertical_flips_raise():
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.data import DatasetMapper, DatasetMapperIgnore, RandomFlip

    assert DatasetMapperIgnore is DatasetMapper
    cfg = base_rcnn_fpn()
    cfg.defrost()
    cfg.MODEL.DEVICE = "cpu"
    cfg.freeze()
    mapper = DatasetMapper.from_config(cfg, True)
    with pytest.raises(ValueError, match="file_name"):
        mapper({"file_name": "a.jpg", "height": 4, "width": 4, "annotations": []})
    with pytest.raises(NotImplementedError):
        RandomFlip(horizontal=False, vertical=True)
