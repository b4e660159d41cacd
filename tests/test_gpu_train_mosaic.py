"""Mosaic training input on the device (csrc/train_input.hip lvc_train_input_tiles_u8, lvc_amd/data/mosaic.py, build.py) against
the reference's DatasetMapperMosaic (tests/golden/train_mosaic.npz), against lvc_train_input_u8 on plain images, and against a numpy
painting of the canvas.  No tolerances: the path is copies and Pillow's integer resample (byte identity), and the normaliser is held
to bit identity."""
import itertools
import random

import numpy as np
import pytest
import torch

from test_host_train_input import case_cfg, case_dict, cases
from test_host_train_mosaic import mosaic_cases, mosaic_cfg, tile_dicts

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEAN, STD = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]


def _expected_slot(u8_hwc, mean, std):
    m = torch.tensor(mean, dtype=torch.float32, device=u8_hwc.device)
    s = torch.tensor(std, dtype=torch.float32, device=u8_hwc.device)
    return (u8_hwc.to(torch.float32) - m) / s


def _run(items, Hp=None, Wp=None, n_slots=None, **kw):
    """One call of the new entry: (uint8 results, the batch buffer, launches)."""
    from lvc_amd import kernels as K
    from lvc_amd.data import resample_coeffs
    from lvc_amd.structures import ImageList

    hp, wp = ImageList.padded_size([it[2:4] for it in items], 32)
    buf = torch.full((n_slots or len(items), Hp or hp, Wp or wp, 4), float("nan"), device=DEV)
    u8 = K.train_input_tiles_u8(items, buf, MEAN, STD, resample_coeffs, want_u8=True, **kw)
    return u8, buf, K.TRAIN_INPUT_TILES_LAUNCHES[-1]


def _fixture_item(c):
    """The job of a fixture case from its own numbers (the reference's rectangles, crop, size and flip)."""
    from lvc_amd.data.mosaic import MosaicInputParams, mosaic_layout

    tiles = [torch.from_numpy(t["image"]).to(DEV) for t in c["tiles"]]
    lay = mosaic_layout([t.shape[:2] for t in tiles])
    p = MosaicInputParams(*lay.size, lay)
    p.crop, p.new_size, p.flip = tuple(c["crop"].tolist()), tuple(c["new_size"].tolist()), bool(c["flip"])
    return p.tiles_item(tiles)


def _plain_item(raw, job):
    x0, y0, cw, ch, nh, nw, flip = job
    return ([(raw, (0, 0, raw.shape[1], raw.shape[0]), (0, 0))], (x0, y0, cw, ch), nh, nw, flip)


def test_every_fixture_case_is_byte_identical_to_the_reference():
    from lvc_amd.data import DatasetMapperMosaic

    for c in mosaic_cases():
        name = str(c["name"])
        mapper = DatasetMapperMosaic.from_config(mosaic_cfg(c, DEV), True)
        np.random.seed(int(c["seed"]))
        out = mapper(tile_dicts(c))
        ref = torch.from_numpy(c["out_image"])
        got = out["image"]
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == tuple(ref.shape), name
        diff = int((got.cpu() != ref).sum())
        print("%s: %d of %d bytes differ from the reference" % (name, diff, ref.numel()))
        assert diff == 0, name
        slot = out["normalized"]
        exp = _expected_slot(got.permute(1, 2, 0), mapper.pixel_mean, mapper.pixel_std)
        assert torch.equal(slot[:, :, :3], exp) and bool((slot[:, :, 3] == 0).all()), name
        assert out["instances"].gt_boxes.tensor.numpy().tobytes() == c["gt_boxes"].tobytes(), name
        assert out["image_id"] == int(c["out_image_id"]) and "raw" not in out
    # the same cases as ONE batch: every slot is (u8 - mean) / std inside its image and exactly 0 in the padding
    cs = mosaic_cases()
    u8, buf, _ = _run([_fixture_item(c) for c in cs])
    for i, c in enumerate(cs):
        nh, nw = c["new_size"].tolist()
        assert torch.equal(u8[i].cpu(), torch.from_numpy(c["out_image"]).permute(1, 2, 0)), i
        assert torch.equal(buf[i, :nh, :nw, :3], _expected_slot(u8[i], MEAN, STD)), i
        pad = buf[i].clone()
        pad[:nh, :nw, :3] = 0
        assert bool((pad == 0).all()), i


def test_single_tile_jobs_equal_the_plain_entry():
    from lvc_amd import kernels as K
    from lvc_amd.data import resample_coeffs

    cs = cases()
    raws = [torch.from_numpy(c["image"]).to(DEV) for c in cs]
    jobs = [tuple(c["crop"].tolist()) + tuple(c["new_size"].tolist()) + (bool(c["flip"]),) for c in cs]
    assert any(j[2] == j[5] for j in jobs) and any(j[3] == j[4] for j in jobs)      # an unchanged width and an unchanged height
    u8, buf, _ = _run([_plain_item(r, j) for r, j in zip(raws, jobs)])
    ref_buf = torch.full_like(buf, float("nan"))
    ref_u8 = K.train_input_u8(raws, jobs, ref_buf, MEAN, STD, resample_coeffs, want_u8=True)
    assert torch.equal(buf, ref_buf)
    assert all(torch.equal(a, b) for a, b in zip(u8, ref_u8))


def test_mixed_batch_equals_single_calls_and_launch_count_is_constant():
    cs = mosaic_cases()
    plain = cases()[0]
    raw = torch.from_numpy(plain["image"]).to(DEV)
    items = [_plain_item(raw, tuple(plain["crop"].tolist()) + tuple(plain["new_size"].tolist()) + (bool(plain["flip"]),)),
             _fixture_item(cs[1]), _fixture_item(cs[3]), _fixture_item(cs[4]), _fixture_item(cs[2])]
    assert [len(it[0]) for it in items] == [1, 4, 9, 9, 4]
    u8, buf, launches5 = _run(items)
    Hp, Wp = buf.shape[1:3]
    for i, it in enumerate(items):
        one_u8, one_buf, launches1 = _run([it], Hp=Hp, Wp=Wp)
        assert torch.equal(one_u8[0], u8[i]) and torch.equal(one_buf[0], buf[i]), i
    print("kernel launches per call: batch of 5 (1, 4, 9, 9, 4 tiles): %d, batch of 1: %d" % (launches5, launches1))
    assert launches5 == launches1 <= 3


def test_strided_tiles_are_read_in_place():
    """Tiles given as HWC views of CHW tensors (strides (W, 1, H*W)) give what their contiguous copies give."""
    c = mosaic_cases()[3]
    item = _fixture_item(c)
    views = [(t.permute(2, 0, 1).contiguous().permute(1, 2, 0), r, o) for t, r, o in item[0]]
    assert all(not v[0].is_contiguous() for v in views)
    a = _run([item])
    b = _run([(views,) + item[1:]])
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0][0].cpu(), torch.from_numpy(c["out_image"]).permute(1, 2, 0))


def test_later_tiles_win_and_uncovered_pixels_are_114():
    """The reference's own rectangles never overlap (see scripts/make_golden_train_mosaic.py), so the painting rule is checked on
    hand-made rectangles against numpy: overlaps of two and three tiles, a tile inside another, a hole, tiles reaching past the
    window, a tile outside it and an empty rectangle -- copied (no resample), then resampled in both axes and flipped."""
    from lvc_amd.data.transforms import ResizeTransform

    g = torch.Generator().manual_seed(12)
    rects = [(0, 0, 40, 30), (25, 10, 70, 45), (30, 20, 50, 28), (60, 0, 90, 20), (-10, 40, 20, 70), (200, 200, 230, 230),
             (50, 50, 50, 60), (15, 25, 35, 50)]
    origins = [(3, 2), (0, 0), (5, 5), (1, 0), (12, 0), (0, 0), (0, 0), (2, 3)]
    tiles = [torch.randint(0, 256, (80, 75, 3), generator=g, dtype=torch.uint8) for _ in rects]
    canvas = np.full((260, 260, 3), 114, np.uint8)
    for t, (x1a, y1a, x2a, y2a), (x1b, y1b) in zip(tiles, rects, origins):
        lx, ly = max(x1a, 0), max(y1a, 0)      # the canvas starts at 0: the part of a rectangle left of it does not exist
        canvas[ly:y2a, lx:x2a] = t.numpy()[y1b + ly - y1a:y1b + y2a - y1a, x1b + lx - x1a:x1b + x2a - x1a]
    X0, Y0, cw, ch = 2, 1, 93, 71
    window = torch.from_numpy(canvas[Y0:Y0 + ch, X0:X0 + cw].copy())
    assert bool((window == 114).all(dim=2).any())
    spec = [(t.to(DEV), r, o) for t, r, o in zip(tiles, rects, origins)]
    u8, _, _ = _run([(spec, (X0, Y0, cw, ch), ch, cw, False)])
    assert torch.equal(u8[0].cpu(), window)
    u8, _, _ = _run([(spec, (X0, Y0, cw, ch), 100, 131, True)])
    ref = ResizeTransform(ch, cw, 100, 131).apply_image(window.to(DEV)).flip(1)
    assert torch.equal(u8[0], ref)


def test_bad_jobs_are_refused_before_any_launch():
    from lvc_amd import kernels as K
    from lvc_amd.data import resample_coeffs

    F, HEAD, TILE = K.TRAIN_INPUT_TILES_FIELDS, K.TRAIN_INPUT_TILES_HEAD, K.TRAIN_INPUT_TILES_TILE
    raw = torch.zeros(40, 50, 3, dtype=torch.uint8, device=DEV)
    tile = (raw, (10, 10, 60, 50), (0, 0))
    good = ([tile], (10, 10, 50, 40), 40, 50, False)

    def edit(word, value, job=0):
        def hook(tab):
            tab[job, word] = value
        return hook

    def two(tab):
        tab[1, 13] = 0

    bad = [
        ("no tiles", [good], edit(16, 0)),
        ("ten tiles", [good], edit(16, 10)),
        ("null tile pointer", [good], edit(HEAD + 0, 0)),
        ("zero row stride", [good], edit(HEAD + 3, 0)),
        ("negative channel stride", [good], edit(HEAD + 5, -1)),
        ("rectangle with negative extent", [good], edit(HEAD + 8, 9)),
        ("window reaches past the tile's right edge", [([(raw, (10, 10, 70, 50), (0, 0))], (10, 10, 60, 40), 40, 60, False)], None),
        ("window reaches above the tile's source", [([(raw, (10, 10, 60, 50), (0, -1))], (10, 10, 50, 40), 40, 50, False)], None),
        ("source origin past the bottom", [([(raw, (10, 10, 60, 50), (0, 1))], (10, 10, 50, 40), 40, 50, False)], None),
        ("taps outside the window", [([tile], (10, 10, 50, 40), 40, 25, False)], edit(2, 49)),
        ("row taps outside the window", [([tile], (10, 10, 50, 40), 20, 50, False)], edit(3, 39)),
        ("output wider than the padded batch", [([tile], (10, 10, 50, 40), 40, 100, False)], None),
        ("output taller than the padded batch", [([tile], (10, 10, 50, 40), 80, 50, False)], None),
        ("two jobs on one slot", [good, good], two),
        ("slot outside the batch", [good], edit(13, 5)),
        ("intermediate outside the scratch buffer", [good], edit(15, 1 << 40)),
        ("negative intermediate offset", [good], edit(15, -256)),
    ]
    for what, items, hook in bad:
        buf = torch.full((2, 64, 64, 4), -7.0, device=DEV)
        with pytest.raises(RuntimeError, match="lvc_train_input_tiles_u8"):
            K.train_input_tiles_u8(items, buf, [0, 0, 0], [1, 1, 1], resample_coeffs, table_hook=hook)
        torch.cuda.synchronize()
        assert bool((buf == -7.0).all()), what
    buf = torch.full((2, 64, 64, 4), -7.0, device=DEV)      # and the job they were all made from is accepted
    K.train_input_tiles_u8([good], buf, [0, 0, 0], [1, 1, 1], resample_coeffs)
    assert bool((buf[0] == 0).all()) and bool((buf[1] == -7.0).all())


def _mosaic_loader_cfg(split=0.5):
    from test_gpu_train_input import _loader_cfg

    cfg = _loader_cfg()
    cfg.defrost()
    cfg.INPUT.MOSAIC, cfg.INPUT.MOSAIC49SPLIT = 0.5, split
    cfg.INPUT.CROP.SIZE = [0.7, 0.7]
    cfg.freeze()
    return cfg


@pytest.fixture(scope="module")
def train_model():
    from test_gpu_train import _train_model

    return _train_model()


def test_loader_pipelined_equals_sync_equals_the_mappers_and_trains(train_model):
    from lvc_amd.data import DatasetMapper, DatasetMapperMosaic, build_detection_train_mosaic_loader
    from lvc_amd.data.dataset_mapper import MOSAIC_KEYS
    from test_gpu_train_input import _step, _toy_dataset

    model = train_model
    data = _toy_dataset(11, 3)
    cfg = _mosaic_loader_cfg()
    seen = {}
    for sync in (True, False):
        np.random.seed(31)
        random.seed(17)
        loader = build_detection_train_mosaic_loader(cfg, data, seed=5, size_divisibility=model.backbone.size_divisibility, sync=sync)
        rows = []
        for batch in itertools.islice(loader, 6):
            pb = batch[0]["prepared"]
            pb.ready.synchronize()
            rows.append(([b["tile_indices"] for b in batch], list(pb.sizes), pb.buffer.clone(),
                         [b["instances"].gt_boxes.tensor.clone() for b in batch], batch))
        torch.cuda.synchronize()
        seen[sync] = rows
    kinds = sorted({len(t) for r in seen[True] for t in r[0]})
    print("tiles per item over 6 batches:", [[len(t) for t in r[0]] for r in seen[True]])
    assert kinds == [1, 4, 9]
    for k, (a, b) in enumerate(zip(seen[True], seen[False])):
        assert a[0] == b[0] and a[1] == b[1], k
        assert a[2].shape == b[2].shape and torch.equal(a[2], b[2]), k
        assert all(torch.equal(x, y) for x, y in zip(a[3], b[3])), k
    # each item is what the mappers give for the same tiles under the same numpy seed (the loader draws in batch order)
    plain, mosaic = DatasetMapper._from_config(cfg, True, allow=MOSAIC_KEYS), DatasetMapperMosaic.from_config(cfg, True)
    np.random.seed(31)
    for tiles, sizes, buf, boxes, batch in seen[True]:
        for s, idxs in enumerate(tiles):
            out = plain(data[idxs[0]]) if len(idxs) == 1 else mosaic([data[i] for i in idxs])
            nh, nw = sizes[s]
            assert tuple(out["image"].shape[1:]) == (nh, nw)
            assert torch.equal(buf[s, :nh, :nw], out["normalized"])
            assert torch.equal(out["instances"].gt_boxes.tensor, boxes[s])
            assert batch[s]["image_id"] == data[idxs[-1]]["image_id"] and batch[s]["index"] == idxs[0]
    # one training step on a loader batch that holds a mosaic equals the step on the same batch passed as "image" tensors
    np.random.seed(31)
    k = [i for i, r in enumerate(seen[True]) if max(len(t) for t in r[0]) > 1][0]
    outs = []
    for tiles, *_ in seen[True][:k + 1]:
        outs = [plain(data[idxs[0]]) if len(idxs) == 1 else mosaic([data[i] for i in idxs]) for idxs in tiles]
    from lvc_amd.data.build import PreparedBatch

    fixed = PreparedBatch(seen[True][k][2], seen[True][k][1], None)      # the sync loader's one buffer has moved on: the kept copy
    batch = [dict(b, prepared=fixed) for b in seen[True][k][4]]
    as_images = [{"image": o["image"], "instances": b["instances"], "height": b["height"], "width": b["width"]} for o, b in zip(outs, batch)]
    images, ref = model.preprocess_image(batch), model.preprocess_image(as_images)      # the model's input is the same, bit for bit
    assert images.image_sizes == ref.image_sizes and torch.equal(images.tensor, ref.tensor)
    runs = [_step(model, as_images), _step(model, as_images), _step(model, batch)]
    for losses in runs:
        assert all(bool(torch.isfinite(v).all()) for v in losses.values())
    repeatable = all(torch.equal(runs[0][n], runs[1][n]) for n in runs[0])
    print("two steps of the image path on identical inputs bit-identical:", repeatable)
    print({n: (float(runs[0][n].detach()), float(runs[2][n].detach())) for n in runs[0]})
    if repeatable:      # as test_gpu_train_input: the step is compared where the step itself repeats
        for n in runs[0]:
            assert torch.equal(runs[0][n], runs[2][n]), n


def test_fine_tune_settings_produce_batches_and_train_a_step(train_model):
    """What the two shipped fine-tune yamls set for the input (INPUT.MOSAIC 0.5, MOSAIC49SPLIT 1.0, CROP relative_range 0.7) with
    INPUT.COLOR_JITTER False; and MOSAIC 0 is the plain loader."""
    from lvc_amd.data import build_detection_train_loader, build_detection_train_mosaic_loader
    from test_gpu_train_input import _loader_cfg, _step, _toy_dataset

    model = train_model
    data = _toy_dataset(11, 4)
    np.random.seed(2)
    random.seed(2)
    loader = build_detection_train_mosaic_loader(_mosaic_loader_cfg(split=1.0), data, seed=1, size_divisibility=model.backbone.size_divisibility)
    batches = list(itertools.islice(loader, 4))
    assert {len(b["tile_indices"]) for batch in batches for b in batch} == {1, 4}
    batch = [b for b in batches if max(len(x["tile_indices"]) for x in b) == 4][0]
    losses = _step(model, batch)
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"}
    assert all(bool(torch.isfinite(v).all()) for v in losses.values())
    got = []
    for build in (build_detection_train_mosaic_loader, build_detection_train_loader):
        np.random.seed(9)
        batch = next(build(_loader_cfg(), data, seed=1, size_divisibility=model.backbone.size_divisibility, sync=True))
        got.append(([b["index"] for b in batch], batch[0]["prepared"].buffer.clone()))
    assert got[0][0] == got[1][0] and torch.equal(got[0][1], got[1][1])
