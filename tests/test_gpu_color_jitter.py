"""Colour jitter on the device (csrc/color_jitter.hip lvc_color_jitter_tiles_u8, lvc_amd/data) against the numpy mirror of Pillow's
arithmetic (tests/color_ref.py, itself held to the installed Pillow by tests/test_host_color_jitter.py) and against the reference's
DatasetMapperIgnore / DatasetMapperMosaic with INPUT.COLOR_JITTER True (tests/golden/color_jitter.npz).  No tolerances: the path is
uint8 and short float arithmetic, every comparison is for equality."""
import itertools
import random

import numpy as np
import pytest
import torch

import color_ref as R
from test_host_color_jitter import case_input, case_mapper, jitter_cases, jitter_cfg, seed_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _plain(img):
    return [(img, (0, 0, int(img.shape[1]), int(img.shape[0])), (0, 0))]


def _jitter(img, ops, factors, window=None, **kw):
    """One job of the entry on a plain device image -> the jittered window (a view of the call's scratch)."""
    from lvc_amd import kernels as K

    h, w = img.shape[:2]
    return K.color_jitter_tiles_u8([(_plain(img), window or (0, 0, w, h), ops, factors)], **kw)[0]


def _expected_slot(u8_hwc, mean, std):
    m = torch.tensor(mean, dtype=torch.float32, device=u8_hwc.device)
    s = torch.tensor(std, dtype=torch.float32, device=u8_hwc.device)
    return (u8_hwc.to(torch.float32) - m) / s


# ------------------------------------------------------------------------------------------------ single steps, every colour
class _Colours:
    """The all-colours image, on the host and the device, with the factor-independent halves of the mirror's hue step computed once:
    HSV of every colour, and RGB of every HSV triple (the image read as HSV)."""

    def __init__(self):
        self.host = R.all_colours()
        self.dev = torch.from_numpy(self.host).to(DEV)
        self._hsv = self._rgb_of = None

    def hue(self, f):
        if self._hsv is None:
            self._hsv, self._rgb_of = R.rgb_to_hsv(self.host), R.hsv_to_rgb(self.host)
        h = (self._hsv[..., 0].astype(np.int32) + R.hue_shift(f)) & 255
        # the image holds triple (a, b, c) at flat index a << 16 | b << 8 | c
        return self._rgb_of.reshape(-1, 3)[(h << 16) | (self._hsv[..., 1].astype(np.int32) << 8) | self._hsv[..., 2]]


@pytest.fixture(scope="module")
def colours():
    return _Colours()


_RANDOM = np.random.default_rng(17)
_SINGLE = [(R.HUE, -0.2), (R.HUE, 0.2), (R.HUE, float(np.float32(_RANDOM.uniform(-0.2, 0.2)))),
           (R.SATURATION, 0.6), (R.SATURATION, 1.4), (R.SATURATION, float(np.float32(_RANDOM.uniform(0.6, 1.4)))),
           (R.BRIGHTNESS, 0.6), (R.BRIGHTNESS, 1.4), (R.BRIGHTNESS, float(np.float32(_RANDOM.uniform(0.6, 1.4))))]


@pytest.mark.parametrize("op,factor", _SINGLE)
def test_single_step_on_every_colour_equals_the_mirror(colours, op, factor):
    got = _jitter(colours.dev, [op], [factor]).cpu().numpy()
    if op == R.HUE:
        exp = colours.hue(factor)
        small = colours.host[:8, :64]      # and the memoised form is the mirror's own
        assert np.array_equal(colours.hue(factor)[:8, :64], R.hue(small, factor))
    else:
        exp = R.jitter(colours.host, [op], [factor])
    diff = int((got != exp).any(-1).sum())
    print("step %d factor %r: %d of %d colours differ" % (op, factor, diff, 1 << 24))
    assert diff == 0


# ------------------------------------------------------------------------------------------------ the mean
def test_contrast_mean_rounds_half_up():
    img = np.array([[[10, 10, 10], [11, 11, 11]]], np.uint8)      # L = 10, 11: the mean is 10.5, m = 11
    dev = torch.from_numpy(img).to(DEV)
    assert _jitter(dev, [R.CONTRAST], [0.0]).cpu().tolist() == [[[11] * 3, [11] * 3]]
    got = _jitter(dev, [R.CONTRAST], [0.6]).cpu().numpy()
    assert np.array_equal(got, R.contrast(img, 0.6)) and not np.array_equal(got, R.contrast(img, 0.6, m=10))


def test_contrast_sum_does_not_overflow_32_bits():
    h, w = 4200, 4100
    assert h * w * 255 > 1 << 32
    img = torch.full((h, w, 3), 255, dtype=torch.uint8, device=DEV)
    out = _jitter(img, [R.CONTRAST], [0.0])      # factor 0: every byte is m
    assert tuple(out.shape) == (h, w, 3) and bool((out == 255).all())


def test_contrast_mean_is_taken_after_the_steps_before_it():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    dev = torch.from_numpy(img).to(DEV)
    for ops, factors in (([R.BRIGHTNESS, R.CONTRAST], [0.6, 1.3]), ([R.HUE, R.SATURATION, R.CONTRAST, R.BRIGHTNESS], [0.1, 1.4, 0.7, 1.2])):
        factors = [float(np.float32(f)) for f in factors]
        got = _jitter(dev, ops, factors).cpu().numpy()
        assert np.array_equal(got, R.jitter(img, ops, factors))
        k = ops.index(R.CONTRAST)
        before = R.jitter(img, ops[:k], factors[:k])
        assert R.mean_grey(before) != R.mean_grey(img)      # the source's mean would give another image
        wrong = R.jitter(R.contrast(before, factors[k], m=R.mean_grey(img)), ops[k + 1:], factors[k + 1:])
        assert not np.array_equal(got, wrong)
    # a window of a larger image, odd sizes, more than one workgroup, no steps at all: a copy
    big = rng.integers(0, 256, (91, 77, 3), dtype=np.uint8)
    win = (5, 7, 61, 70)
    got = _jitter(torch.from_numpy(big).to(DEV), [], [], window=win).cpu().numpy()
    assert np.array_equal(got, big[7:77, 5:66])
    ops, factors = [R.SATURATION, R.CONTRAST, R.HUE], [float(np.float32(f)) for f in (0.7, 1.4, -0.2)]
    got = _jitter(torch.from_numpy(big).to(DEV), ops, factors, window=win).cpu().numpy()
    assert np.array_equal(got, R.jitter(big[7:77, 5:66], ops, factors))
    # an HWC view of a CHW tensor is read in place
    chw = torch.from_numpy(big).to(DEV).permute(2, 0, 1).contiguous().permute(1, 2, 0)
    assert not chw.is_contiguous() and np.array_equal(_jitter(chw, ops, factors, window=win).cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------ the reference's cases
def test_every_fixture_case_through_its_mapper_is_byte_identical_to_the_reference():
    for c in jitter_cases():
        name = str(c["name"])
        mapper = case_mapper(c, DEV)
        seed_case(c)
        out = mapper(case_input(c))
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


class _Script:
    """Stands where a loader's mapper stands: item k of a batch is drawn by the k-th (mapper, case) pair, seeded as the case says."""

    def __init__(self, plan):
        self.plan, self.at = plan, 0
        self.pixel_mean, self.pixel_std = plan[0][0].pixel_mean, plan[0][0].pixel_std

    def draw(self, d):
        mapper, c = self.plan[self.at % len(self.plan)]
        self.at += 1
        seed_case(c)
        return mapper.draw(d)


def _batch(loader_cls, picks, runs=2):
    """`picks`: (case, jitter on?) per batch item.  The batch through `loader_cls`'s own _prepare, `runs` times:
    [(items, buffer copy)], and the launches of the new entry."""
    from lvc_amd import kernels as K
    from lvc_amd.data import DatasetMapper, DatasetMapperMosaic
    from lvc_amd.data.build import MosaicTrainInputLoader, TrainingSampler, _Slot
    from lvc_amd.data.mosaic import MapDatasetMosaic

    data, indices, plan = [], [], []
    for c, on in picks:
        dicts = case_input(c)
        dicts = dicts if isinstance(dicts, list) else [dicts]
        indices.append(list(range(len(data), len(data) + len(dicts))))
        data += dicts
        cls = DatasetMapperMosaic if c["tiles"] else DatasetMapper
        plan.append((cls.from_config(jitter_cfg(c, DEV, key=on), True, color_jitter=True), c))
    script = _Script(plan)
    sampler = TrainingSampler(len(data), seed=0)
    if loader_cls is MosaicTrainInputLoader:
        cfg = jitter_cfg(picks[0][0], DEV)
        loader = loader_cls(data, script, script, MapDatasetMosaic(data, script, script, cfg), len(picks), sampler, 32, device=DEV)
    else:
        loader = loader_cls(data, script, len(picks), sampler, 32, device=DEV)
        indices = [i[0] for i in indices]
    out, launches = [], []
    slot = _Slot(loader.device)
    for _ in range(runs):
        del K.COLOR_JITTER_LAUNCHES[:]
        items = loader._prepare(indices, slot, torch.cuda.current_stream())
        items[0]["prepared"].ready.synchronize()
        out.append((items, items[0]["prepared"].buffer.clone()))
        launches.append(list(K.COLOR_JITTER_LAUNCHES))
    return out, launches, plan


def _check_batch(picks, out, plan):
    from lvc_amd.data import DatasetMapper

    items, buf = out
    for s, ((c, on), b) in enumerate(zip(picks, items)):
        name = str(c["name"])
        nh, nw = b["prepared"].sizes[s]
        p = b["train_input_params"]
        if on:
            ref = torch.from_numpy(c["out_image"]).to(DEV).permute(1, 2, 0)
            assert list(p.jitter[0]) == c["jitter_ops"].tolist(), name      # the permutation is as recorded
        else:      # the same draw without the key: what the standing path gives
            assert p.jitter is None, name
            seed_case(c)
            ref = plan[s][0](case_input(c))["image"].permute(1, 2, 0)
        assert (nh, nw) == tuple(ref.shape[:2]), name
        assert torch.equal(buf[s, :nh, :nw, :3], _expected_slot(ref, plan[s][0].pixel_mean, plan[s][0].pixel_std)), name
        pad = buf[s].clone()
        pad[:nh, :nw, :3] = 0
        assert bool((pad == 0).all()), name
        if on:
            assert b["instances"].gt_boxes.tensor.numpy().tobytes() == c["gt_boxes"].tobytes(), name


def test_fixture_cases_through_both_loaders_mixed_batches_two_launches_bit_identical_runs():
    from lvc_amd import kernels as K
    from lvc_amd.data.build import MosaicTrainInputLoader, TrainInputLoader

    cs = jitter_cases()
    plain, mosaic = [c for c in cs if not c["tiles"]], [c for c in cs if c["tiles"]]
    assert {len(c["tiles"]) for c in mosaic} == {4, 9}
    batches = [
        (TrainInputLoader, [(c, True) for c in plain]),                                                  # every plain case
        (TrainInputLoader, [(plain[0], True), (plain[1], False), (plain[3], True)]),                     # jitter and none, mixed
        (MosaicTrainInputLoader, [(mosaic[0], True), (plain[2], True), (mosaic[1], True)]),              # every item jittered
        (MosaicTrainInputLoader, [(plain[0], True), (mosaic[0], True), (plain[1], False), (mosaic[1], True), (mosaic[0], False)]),
    ]
    for loader_cls, picks in batches:
        out, launches, plan = _batch(loader_cls, picks)
        for run in out:
            _check_batch(picks, run, plan)
        print("%s, %d items (%d jittered): launches of the jitter entry per batch %s" %
              (loader_cls.__name__, len(picks), sum(on for _, on in picks), launches))
        assert launches == [[2], [2]]      # one call of the entry per batch, two launches whatever the batch
        assert torch.equal(out[0][1], out[1][1])      # two runs, bit for bit
    # a batch without a jitter item: the calls it always made, and none of the new entry
    for loader_cls in (TrainInputLoader, MosaicTrainInputLoader):
        del K.TRAIN_INPUT_LAUNCHES[:], K.TRAIN_INPUT_TILES_LAUNCHES[:]
        picks = [(plain[0], False), (plain[4], False)]
        out, launches, plan = _batch(loader_cls, picks, runs=1)
        _check_batch(picks, out[0], plan)
        assert launches == [[]]
        if loader_cls is TrainInputLoader:
            assert len(K.TRAIN_INPUT_LAUNCHES) >= 1 and K.TRAIN_INPUT_TILES_LAUNCHES == []
        else:
            assert len(K.TRAIN_INPUT_TILES_LAUNCHES) == 1


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_jobs_are_refused_before_any_launch():
    from lvc_amd import kernels as K

    raw = torch.zeros(40, 50, 3, dtype=torch.uint8, device=DEV)
    ws = K.ColorJitterWorkspace(DEV)
    ws.reserve(1 << 14, 1 << 16)
    good = (_plain(raw), (5, 4, 40, 30), [R.BRIGHTNESS, R.CONTRAST], [1.2, 0.8])

    def edit(word, value):
        def hook(tab):
            tab[0, word] = value
        return hook

    bad = [
        ("window past the right edge of the canvas' only tile", ([(raw, (0, 0, 60, 40), (0, 0))], (20, 4, 40, 30), [R.HUE], [0.1]), None),
        ("window below it", ([(raw, (0, 0, 50, 60), (0, 0))], (0, 20, 40, 30), [], []), None),
        ("window at a negative corner", (_plain(raw), (-1, 0, 40, 30), [], []), None),
        ("step id 7", good, edit(6, 7)),
        ("five steps", good, edit(5, 5)),
        ("negative step count", good, edit(5, -1)),
        ("two contrast steps", good, edit(6, R.CONTRAST)),
        ("hue factor outside [-0.5, 0.5]", (_plain(raw), (5, 4, 40, 30), [R.HUE], [0.7]), None),
        ("no tiles", good, edit(14, 0)),
        ("ten tiles", good, edit(14, 10)),
        ("null tile pointer", good, edit(K.TRAIN_INPUT_TILES_HEAD, 0)),
        ("zero row stride", good, edit(K.TRAIN_INPUT_TILES_HEAD + 3, 0)),
        ("output outside the scratch", good, edit(4, 1 << 40)),
        ("misaligned output", good, edit(4, 2)),
        ("sum word not zero", good, edit(19, 1)),
    ]
    for what, item, hook in bad:
        ws.scratch.fill_(7)
        with pytest.raises(RuntimeError, match="lvc_color_jitter_tiles_u8"):
            K.color_jitter_tiles_u8([item], workspace=ws, table_hook=hook)
        torch.cuda.synchronize()
        assert bool((ws.scratch == 7).all()), what
    def overlap(tab):
        tab[1, 4] = tab[0, 4]
    with pytest.raises(RuntimeError, match="lvc_color_jitter_tiles_u8"):
        K.color_jitter_tiles_u8([good, good], workspace=ws, table_hook=overlap)
    out = K.color_jitter_tiles_u8([good], workspace=ws)[0]      # and the job they were all made from is accepted
    assert tuple(out.shape) == (30, 40, 3) and bool((out == 0).all())


# ------------------------------------------------------------------------------------------------ the shipped settings
@pytest.fixture(scope="module")
def train_model():
    from test_gpu_train import _train_model

    return _train_model()


def test_fine_tune_settings_with_color_jitter_produce_batches_and_train_a_step(train_model):
    """What the two shipped fine-tune yamls set for the input: INPUT.MOSAIC 0.5, MOSAIC49SPLIT 1.0, CROP relative_range 0.7 and
    INPUT.COLOR_JITTER True, opted into with color_jitter=True."""
    from lvc_amd import kernels as K
    from lvc_amd.data import build_detection_train_mosaic_loader
    from test_gpu_train_input import _step, _toy_dataset
    from test_gpu_train_mosaic import _mosaic_loader_cfg

    model = train_model
    data = _toy_dataset(11, 4)
    cfg = _mosaic_loader_cfg(split=1.0)
    cfg.defrost()
    cfg.INPUT.COLOR_JITTER = True
    cfg.freeze()
    assert cfg.INPUT.CROP.TYPE == "relative_range" and list(cfg.INPUT.CROP.SIZE) == [0.7, 0.7]
    with pytest.raises(NotImplementedError, match="INPUT.COLOR_JITTER"):
        build_detection_train_mosaic_loader(cfg, data, seed=1)
    seen = []
    for sync in (True, False):
        np.random.seed(2)
        random.seed(2)
        torch.manual_seed(2)
        del K.COLOR_JITTER_LAUNCHES[:]
        loader = build_detection_train_mosaic_loader(cfg, data, seed=1, size_divisibility=model.backbone.size_divisibility, sync=sync,
                                                     color_jitter=True)
        batches = list(itertools.islice(loader, 4))
        torch.cuda.synchronize()
        assert {len(b["tile_indices"]) for batch in batches for b in batch} == {1, 4}
        for batch in batches:
            for b in batch:
                ops, factors = b["train_input_params"].jitter
                assert sorted(ops) == [0, 1, 2, 3] and all(0.6 <= f <= 1.4 for o, f in zip(ops, factors) if o != 3)
        assert set(K.COLOR_JITTER_LAUNCHES) == {2} and len(K.COLOR_JITTER_LAUNCHES) >= 4
        seen.append(batches)
    for a, b in zip(*seen):      # the pipelined loader draws what the plain order draws
        assert [x["tile_indices"] for x in a] == [x["tile_indices"] for x in b]
        assert [x["train_input_params"].jitter for x in a] == [x["train_input_params"].jitter for x in b]
    last = [batches[-1][0]["prepared"] for batches in seen]      # the one batch whose buffer neither loader has reused yet
    assert last[0].sizes == last[1].sizes and torch.equal(last[0].buffer, last[1].buffer)
    losses = _step(model, seen[1][-1])
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"}
    assert all(bool(torch.isfinite(v).all()) for v in losses.values())
