"""Large-scale jitter on the device (csrc/train_input.hip lvc_train_input_lsj_u8, lvc_amd/data) against the installed Pillow's
Image.resize -> numpy crop -> pad 128 -> flip, against the reference's mappers (tests/golden/train_lsj.npz, scripts/make_golden_lsj.py)
and against the path every batch without the jitter takes.  No tolerances: the path is Pillow's integer resample and copies (byte
identity), and the normaliser is held to bit identity with torch's fp32 (v - mean) / std."""
import hashlib

import numpy as np
import pytest
import torch
from PIL import Image      # the oracle of the hand-set cases: a machine without it fails here, it does not skip

from test_host_lsj import case_input, case_mapper, cfg_case, lsj_cases, lsj_cfg, lsj_of, seeded
from test_host_train_input import case_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEAN, STD = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]
T = (72, 100)      # not square, no multiple of 32: the canvas fill and the batch's zero padding stay apart


def _normalised(u8_hwc, mean=MEAN, std=STD):
    m = torch.tensor(mean, dtype=torch.float32, device=u8_hwc.device)
    s = torch.tensor(std, dtype=torch.float32, device=u8_hwc.device)
    return (u8_hwc.to(torch.float32) - m) / s


def _pillow_canvas(img, scaled, ox, oy, target, flip, fill=128):
    """The CPU chain of the reference: Pillow's bilinear resize of the WHOLE image, numpy crop, pad right and bottom, flip."""
    sh, sw = scaled
    full = np.asarray(Image.fromarray(img).resize((sw, sh), Image.BILINEAR))
    win = full[oy:oy + target[0], ox:ox + target[1]]
    out = np.pad(win, ((0, target[0] - win.shape[0]), (0, target[1] - win.shape[1]), (0, 0)), mode="constant", constant_values=fill)
    return np.ascontiguousarray(out[:, ::-1] if flip else out)


def _item(raw, scaled, ox, oy, target, flip, fill=128):
    h, w = raw.shape[:2]
    window = (ox, oy, min(scaled[1], target[1]), min(scaled[0], target[0]))
    return ([(raw, (0, 0, w, h), (0, 0))], (0, 0, w, h), tuple(scaled), window, tuple(target), fill, flip)


def _run(items, Hp=None, Wp=None, **kw):
    from lvc_amd import kernels as K
    from lvc_amd.data import resample_coeffs
    from lvc_amd.structures import ImageList

    hp, wp = ImageList.padded_size([it[4] for it in items], 32)
    buf = torch.full((len(items), Hp or hp, Wp or wp, 4), float("nan"), device=DEV)
    u8 = K.train_input_lsj_u8(items, buf, MEAN, STD, resample_coeffs, want_u8=True, **kw)
    return u8, buf, K.TRAIN_INPUT_LSJ_LAUNCHES[-1]


def _check_slot(buf_i, u8_i, target):
    th, tw = target
    assert torch.equal(buf_i[:th, :tw, :3], _normalised(u8_i))      # bit-identical inside the canvas
    rest = buf_i.clone()
    rest[:th, :tw, :3] = 0
    assert bool((rest == 0).all())                                  # exactly 0 in the fourth channel and outside the canvas


# (name, source (h, w), scaled (h, w), ox, oy, target, flip)
HAND = [
    ("crop both", (90, 120), (113, 150), 27, 22, T, False),
    ("crop both at the far corner", (90, 120), (113, 150), 50, 41, T, True),
    ("crop both at the origin", (90, 120), (113, 150), 0, 0, T, False),
    ("pad both", (90, 120), (71, 94), 0, 0, T, False),
    ("pad both, flipped: the fill on the left", (88, 117), (69, 92), 0, 0, T, True),
    ("crop x, pad y", (40, 120), (37, 110), 7, 0, T, False),
    ("crop y, pad x, flipped", (120, 40), (80, 27), 0, 6, T, True),
    ("scaled == target on x", (40, 120), (33, 100), 0, 0, T, True),
    ("scaled == target on both", (50, 70), (72, 100), 0, 0, T, False),
    ("width unchanged: no horizontal pass", (60, 20), (59, 20), 0, 0, T, True),
    ("height unchanged: no vertical pass", (20, 60), (20, 61), 0, 0, T, False),
    ("height unchanged and cropped on it", (80, 60), (80, 61), 0, 5, T, False),
    ("nothing changes", (72, 80), (72, 80), 0, 0, T, True),
    ("down-scaling by 2.3: wide kernels", (200, 260), (87, 113), 9, 11, T, False),
    ("two workgroups a row", (30, 200), (60, 400), 57, 11, (40, 300), True),
    ("a single pixel a side", (1, 1), (3, 3), 0, 0, (5, 7), True),
]


@pytest.fixture(scope="module")
def hand():
    """Sources, jobs and Pillow's canvases of the hand-set cases, computed once."""
    rng = np.random.default_rng(41)
    out = []
    for name, hw, scaled, ox, oy, target, flip in HAND:
        img = rng.integers(0, 256, hw + (3,), dtype=np.uint8)
        out.append((name, torch.from_numpy(img).to(DEV), (scaled, ox, oy, target, flip), _pillow_canvas(img, scaled, ox, oy, target, flip)))
    return out


def test_every_hand_set_case_is_byte_identical_to_pillow(hand):
    for name, raw, job, ref in hand:
        u8, buf, launches = _run([_item(raw, *job)])
        diff = int((u8[0].cpu().numpy() != ref).sum())
        print("%-44s %d of %d bytes differ from Pillow's chain" % (name, diff, ref.size))
        assert u8[0].shape == ref.shape and diff == 0, name
        _check_slot(buf[0], u8[0], job[3])
        assert launches == 2, name


def test_mixed_batch_of_five_equals_pillow_and_single_calls_in_two_launches(hand):
    pick = [0, 4, 6, 10, 15]      # crop both; pad both flipped; crop y pad x flipped; height unchanged; a 5 x 7 canvas
    items = [_item(hand[i][1], *hand[i][2]) for i in pick]
    assert len({tuple(it[0][0][0].shape) for it in items}) == 5      # five source sizes
    u8, buf, launches = _run(items)
    assert launches == 2 and tuple(buf.shape[1:3]) == (96, 128)
    for s, i in enumerate(pick):
        assert np.array_equal(u8[s].cpu().numpy(), hand[i][3]), hand[i][0]
        _check_slot(buf[s], u8[s], hand[i][2][3])
        one_u8, one_buf, one_launches = _run([items[s]], Hp=96, Wp=128)
        assert torch.equal(one_u8[0], u8[s]) and torch.equal(one_buf[0], buf[s]) and one_launches == 2


def test_strided_and_tiled_sources(hand):
    """An HWC view of a CHW tensor is read in place; a source cut into two tiles (with a hole that shows the mosaic's 114) equals
    Pillow on the painted canvas."""
    name, raw, job, ref = hand[0]
    view = raw.permute(2, 0, 1).contiguous().permute(1, 2, 0)
    assert not view.is_contiguous()
    assert np.array_equal(_run([_item(view, *job)])[0][0].cpu().numpy(), ref)
    h, w = raw.shape[:2]
    canvas = np.full((h, w, 3), 114, np.uint8)
    canvas[:, :50] = raw.cpu().numpy()[:, :50]
    canvas[10:, 60:] = raw.cpu().numpy()[10:, 60:]
    scaled, ox, oy, target, flip = job
    tiles = [(raw, (0, 0, 50, h), (0, 0)), (raw, (60, 10, w, h), (60, 10))]
    item = (tiles, (0, 0, w, h), scaled, (ox, oy, target[1], target[0]), target, 128, flip)
    assert np.array_equal(_run([item])[0][0].cpu().numpy(), _pillow_canvas(canvas, scaled, ox, oy, target, flip))


def test_mappers_are_byte_identical_to_the_reference_on_every_fixture_case():
    for c in lsj_cases():
        name = str(c["name"])
        mapper = case_mapper(c, DEV)
        with seeded(c):
            out = mapper(case_input(c))
        got, ref = out["image"], torch.from_numpy(c["out_image"])
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == tuple(ref.shape) == (3,) + T, name
        diff = int((got.cpu() != ref).sum())
        print("%-32s %d of %d bytes differ from the reference" % (name, diff, ref.numel()))
        assert diff == 0, name
        slot = out["normalized"]
        assert torch.equal(slot[:, :, :3], _normalised(got.permute(1, 2, 0), mapper.pixel_mean, mapper.pixel_std)), name
        assert bool((slot[:, :, 3] == 0).all()), name
        assert out["instances"].gt_boxes.tensor.numpy().tobytes() == c["gt_boxes"].tobytes(), name


def _one_item_cfg(c, key=False):
    cfg = lsj_cfg(c, DEV, key=key)
    cfg.defrost()
    cfg.SOLVER.IMS_PER_BATCH = 1
    cfg.freeze()
    return cfg


def _check_loader_item(batch, c, mean, std):
    name = str(c["name"])
    assert len(batch) == 1
    pb = batch[0]["prepared"]
    pb.ready.synchronize()
    assert tuple(pb.buffer.shape) == (1, 96, 128, 4) and list(pb.sizes) == [T], name      # the target padded to the divisibility
    ref = torch.from_numpy(c["out_image"]).permute(1, 2, 0).to(DEV)
    assert torch.equal(pb.buffer[0, :T[0], :T[1], :3], _normalised(ref, mean, std)), name      # one fp32 per byte: the bytes are the reference's
    rest = pb.buffer[0].clone()
    rest[:T[0], :T[1], :3] = 0
    assert bool((rest == 0).all()), name
    assert batch[0]["instances"].gt_boxes.tensor.numpy().tobytes() == c["gt_boxes"].tobytes(), name
    assert batch[0]["instances"].image_size == T, name


def test_plain_loader_reproduces_the_fixtures():
    from lvc_amd import kernels as K
    from lvc_amd.data import build_detection_train_loader

    for c in [c for c in lsj_cases() if not c["tiles"]]:
        cfg = _one_item_cfg(c)
        loader = build_detection_train_loader(cfg, [case_dict(c)], seed=0, size_divisibility=32, sync=True, color_jitter=True, lsj=lsj_of(c))
        del K.TRAIN_INPUT_LAUNCHES[:], K.TRAIN_INPUT_LSJ_LAUNCHES[:]      # the logs keep the last 64 calls only: counted from empty
        with seeded(c):
            batch = next(loader)
        _check_loader_item(batch, c, cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD)
        assert K.TRAIN_INPUT_LSJ_LAUNCHES == [2] and K.TRAIN_INPUT_LAUNCHES == []
        loader.close()


def test_mosaic_loader_reproduces_the_fixtures_plain_and_mosaic_items():
    from lvc_amd.data import DatasetMapper, DatasetMapperMosaic
    from lvc_amd.data.build import MosaicTrainInputLoader
    from lvc_amd.data.dataset_mapper import MOSAIC_KEYS

    cs = lsj_cases()
    cs = [c for c in cs if c["tiles"]] + [c for c in cs if not c["tiles"]][:2] + [c for c in cs if not c["tiles"] and int(c["jitter"])]
    for c in cs:
        cfg = _one_item_cfg(c)
        data = case_input(c) if c["tiles"] else [case_input(c)]
        plain = DatasetMapper._from_config(cfg, True, allow=MOSAIC_KEYS, color_jitter=True, lsj=lsj_of(c))
        mosaic = DatasetMapperMosaic.from_config(cfg, True, color_jitter=True, lsj=lsj_of(c))
        loader = MosaicTrainInputLoader(data, plain, mosaic, None, 1, None, 32, device=DEV, sync=True)
        loader.index_batches = lambda n=len(data): iter([[list(range(n))]])      # the fixture's tiles in the fixture's order
        it = iter(loader)
        with seeded(c):
            batch = next(it)
        _check_loader_item(batch, c, cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD)
        assert batch[0]["tile_indices"] == list(range(len(data)))
        it.close()


def test_cfg_key_through_the_loader_gives_the_references_800_square_batch():
    from lvc_amd.data import build_detection_train_loader

    g = cfg_case()
    g["tiles"], g["jitter"] = [], 0
    cfg = _one_item_cfg(g, key=True)
    loader = build_detection_train_loader(cfg, [case_dict(g)], seed=0, sync=True, lsj=True)
    np.random.seed(int(g["seed"]))
    batch = next(loader)
    pb = batch[0]["prepared"]
    pb.ready.synchronize()
    assert tuple(pb.buffer.shape) == (1, 800, 800, 4) and list(pb.sizes) == [(800, 800)]      # no padding waste at all
    m = torch.tensor(cfg.MODEL.PIXEL_MEAN, dtype=torch.float32, device=DEV)
    s = torch.tensor(cfg.MODEL.PIXEL_STD, dtype=torch.float32, device=DEV)
    u8 = torch.round(pb.buffer[0, :, :, :3] * s + m).clamp(0, 255).to(torch.uint8)
    assert torch.equal(pb.buffer[0, :, :, :3], _normalised(u8, cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD))      # u8 is what was normalised
    assert bool((pb.buffer[0, :, :, 3] == 0).all())
    digest = hashlib.sha256(u8.permute(2, 0, 1).contiguous().cpu().numpy().tobytes()).hexdigest()
    assert digest == str(g["sha256"])
    if int(g["has_image"]):
        assert np.array_equal(u8.permute(2, 0, 1).cpu().numpy(), g["out_image"])
    ox, oy, ow, oh = g["window"].tolist()
    assert bool((u8[oh:] == 128).all()) and oh < 800 and int(g["flip"]) == 1      # padded below
    assert batch[0]["instances"].gt_boxes.tensor.numpy().tobytes() == g["gt_boxes"].tobytes()
    loader.close()


def test_two_calls_are_bit_identical_and_the_path_without_lsj_is_the_old_one():
    from lvc_amd import kernels as K
    from lvc_amd.data import DatasetMapper, build_detection_train_loader
    from test_gpu_train_input import _loader_cfg, _toy_dataset

    cs = lsj_cases()
    c = cs[0]
    outs = []
    for _ in range(2):
        with seeded(c):
            outs.append(case_mapper(c, DEV)(case_input(c)))
    assert torch.equal(outs[0]["image"], outs[1]["image"]) and torch.equal(outs[0]["normalized"], outs[1]["normalized"])
    # a cfg without the key, lsj=None (and lsj=True, which follows the key): the entry that was always called, the batch it always gave
    data, cfg = _toy_dataset(4, 6), _loader_cfg()
    got = []
    for kw in ({}, {"lsj": None}, {"lsj": True}):
        n_plain, n_lsj = len(K.TRAIN_INPUT_LAUNCHES), list(K.TRAIN_INPUT_LSJ_LAUNCHES)
        del K.TRAIN_INPUT_LAUNCHES[:]
        np.random.seed(13)
        loader = build_detection_train_loader(cfg, data, seed=2, size_divisibility=32, sync=True, **kw)
        batch = next(loader)
        batch[0]["prepared"].ready.synchronize()
        assert K.TRAIN_INPUT_LAUNCHES == [2] and K.TRAIN_INPUT_LSJ_LAUNCHES == n_lsj      # lvc_train_input_u8, once; the new entry never
        assert all(b["train_input_params"].lsj is None for b in batch)
        got.append(([b["index"] for b in batch], batch[0]["prepared"].buffer.clone(), [b["train_input_params"].job() for b in batch]))
        loader.close()
    assert all(g[0] == got[0][0] and g[2] == got[0][2] and torch.equal(g[1], got[0][1]) for g in got[1:])
    # and that batch is what the entry gives when it is called directly with the drawn jobs
    from lvc_amd.data import resample_coeffs

    ref = torch.full_like(got[0][1], float("nan"))
    K.train_input_u8([data[i]["raw"].to(DEV) for i in got[0][0]], got[0][2], ref, cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD, resample_coeffs)
    assert torch.equal(ref, got[0][1])


def test_mosaic_builder_mixes_plain_mosaic_and_jittered_items_in_one_call():
    """build_detection_train_mosaic_loader(..., lsj=...) on batches of four: plain items, 4- and 9-tile mosaics share a call of the
    new entry, and -- with a plain mapper of the caller's that has no colour jitter beside a mosaic mapper that has one -- only a
    SUBSET of a batch goes through the jitter first.  Every slot equals what the item's own mapper gives alone under the same
    generator states (and the mappers equal the reference, above)."""
    import itertools
    import random

    from lvc_amd import kernels as K
    from lvc_amd.data import DatasetMapper, DatasetMapperMosaic, LargeScaleJitter, build_detection_train_mosaic_loader
    from lvc_amd.data.dataset_mapper import MOSAIC_KEYS
    from test_gpu_train_input import _loader_cfg, _toy_dataset

    cfg = _loader_cfg()
    cfg.defrost()
    cfg.INPUT.MOSAIC, cfg.INPUT.MOSAIC49SPLIT, cfg.INPUT.COLOR_JITTER, cfg.INPUT.LSJ = 0.5, 0.5, True, True
    cfg.INPUT.CROP.SIZE = [0.7, 0.7]
    cfg.SOLVER.IMS_PER_BATCH = 4
    cfg.freeze()
    data = _toy_dataset(11, 3)
    lsj = LargeScaleJitter(0.5, 1.6, T[0], T[1])
    for own_plain in (False, True):
        plain = DatasetMapper._from_config(cfg, True, allow=MOSAIC_KEYS + ("INPUT.COLOR_JITTER",), lsj=lsj) if own_plain else None
        np.random.seed(31), random.seed(17), torch.manual_seed(23)
        loader = build_detection_train_mosaic_loader(cfg, data, mapper=plain, seed=5, size_divisibility=32, sync=True, color_jitter=True, lsj=lsj)
        for log in (K.TRAIN_INPUT_LSJ_LAUNCHES, K.TRAIN_INPUT_LAUNCHES, K.TRAIN_INPUT_TILES_LAUNCHES):
            del log[:]      # the logs keep the last 64 calls only: counted from empty
        rows = []
        for batch in itertools.islice(loader, 5):
            pb = batch[0]["prepared"]
            pb.ready.synchronize()
            assert tuple(pb.buffer.shape) == (4, 96, 128, 4) and list(pb.sizes) == [T] * 4
            rows.append(([b["tile_indices"] for b in batch], [b["train_input_params"].jitter is not None for b in batch], pb.buffer.clone(),
                         [b["instances"].gt_boxes.tensor.clone() for b in batch]))
        loader.close()
        assert K.TRAIN_INPUT_LSJ_LAUNCHES == [2] * 5      # one call of the new entry a batch, none of the others
        assert K.TRAIN_INPUT_LAUNCHES == [] and K.TRAIN_INPUT_TILES_LAUNCHES == []
        kinds = [[len(t) for t in r[0]] for r in rows]
        print("tiles per item:", kinds, "jittered:", [r[1] for r in rows])
        assert {k for ks in kinds for k in ks} == {1, 4, 9} and any(len(set(ks)) > 1 for ks in kinds)
        if own_plain:      # the jittered items are a proper subset of some batch, and not its first items only
            assert all(j == (len(t) > 1) for r in rows for t, j in zip(r[0], r[1]))
            assert any(0 < sum(r[1]) < 4 and not r[1][0] for r in rows)
        else:
            assert all(all(r[1]) for r in rows)
        one_plain = plain or DatasetMapper._from_config(cfg, True, allow=MOSAIC_KEYS, color_jitter=True, lsj=lsj)
        one_mosaic = DatasetMapperMosaic.from_config(cfg, True, color_jitter=True, lsj=lsj)
        np.random.seed(31), torch.manual_seed(23)      # the loader draws item by item in batch order: so does the replay
        for tiles, _, buf, boxes in rows:
            for s, idxs in enumerate(tiles):
                out = one_plain(data[idxs[0]]) if len(idxs) == 1 else one_mosaic([data[i] for i in idxs])
                assert tuple(out["image"].shape) == (3,) + T
                assert torch.equal(buf[s, :T[0], :T[1]], out["normalized"]), (own_plain, tiles, s)
                assert bool((buf[s, T[0]:] == 0).all()) and bool((buf[s, :, T[1]:] == 0).all())
                assert torch.equal(out["instances"].gt_boxes.tensor, boxes[s])
