"""Training input on the device (csrc/train_input.hip, lvc_amd/data/dataset_mapper.py, build.py) against the reference's
DatasetMapperIgnore (tests/golden/train_input_*.npz) and against the composition of the pieces other tests already pin
(ResizeTransform.apply_image, HFlipTransform.apply_image, the model's normalise-and-pad)."""
import itertools

import numpy as np
import pytest
import torch

from test_host_train_input import FIXTURES, case_cfg, case_dict, cases, gold  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _expected_slot(u8_hwc, mean, std):
    """(u8 - mean) / std in fp32 by torch, as [h,w,3]."""
    m = torch.tensor(mean, dtype=torch.float32, device=u8_hwc.device)
    s = torch.tensor(std, dtype=torch.float32, device=u8_hwc.device)
    return (u8_hwc.to(torch.float32) - m) / s


def _pieces(raw, p):
    """One image through the pinned pieces: crop (a copy), ResizeTransform.apply_image, HFlipTransform.apply_image -> uint8 HWC."""
    from lvc_amd.data import HFlipTransform, ResizeTransform

    x0, y0, w, h = p.crop
    img = raw.to(DEV)[y0:y0 + h, x0:x0 + w].contiguous()
    nh, nw = p.new_size
    if (nh, nw) != (h, w):
        img = ResizeTransform(h, w, nh, nw).apply_image(img)
    if p.flip:
        img = HFlipTransform(nw).apply_image(img).contiguous()
    return img


def test_every_fixture_case_is_byte_identical_to_the_reference():
    from lvc_amd import kernels as K
    from lvc_amd.data import DatasetMapper, resample_coeffs
    from lvc_amd.structures import ImageList

    for f in FIXTURES:
        g = gold(f)
        cs = [{key[len("c%d_" % k):]: g[key] for key in g if key.startswith("c%d_" % k)} for k in range(int(g["n"]))]
        raws, jobs, u8s = [], [], []
        for c in cs:
            name = str(c["name"])
            mapper = DatasetMapper.from_config(case_cfg(c, DEV), True)
            np.random.seed(int(c["seed"]))
            out = mapper(case_dict(c))
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
            raws.append(torch.from_numpy(c["image"]).to(DEV))
            jobs.append(tuple(c["crop"].tolist()) + tuple(c["new_size"].tolist()) + (bool(c["flip"]),))
            u8s.append(got.permute(1, 2, 0))
        # the same cases as ONE batch: every slot equals (u8 - mean) / std inside its image and is exactly 0 in the padding
        Hp, Wp = ImageList.padded_size([j[4:6] for j in jobs], 32)
        buf = torch.full((len(jobs), Hp, Wp, 4), float("nan"), device=DEV)
        K.train_input_u8(raws, jobs, buf, mapper.pixel_mean, mapper.pixel_std, resample_coeffs)
        for i, (j, u8) in enumerate(zip(jobs, u8s)):
            nh, nw = j[4:6]
            assert torch.equal(buf[i, :nh, :nw, :3], _expected_slot(u8, mapper.pixel_mean, mapper.pixel_std)), i
            pad = buf[i].clone()
            pad[:nh, :nw, :3] = 0
            assert bool((pad == 0).all()), i


def _full_size_draws():
    """8 images of mixed sizes and orientations with seeded random crops, sizes and flips; the first numpy seed whose draws hold a
    flipped and an unflipped image, an image whose long side hits MAX_SIZE_TRAIN and an 800 x 1333-class output."""
    from lvc_amd.data import AugmentationList, RandomCrop, RandomFlip, ResizeShortestEdge

    sizes = [(480, 640), (640, 480), (427, 640), (500, 375), (600, 1400), (900, 1500), (768, 1024), (1200, 800)]
    aug = AugmentationList([RandomCrop("relative_range", (0.8, 0.8)), ResizeShortestEdge((640, 672, 704, 736, 768, 800), 1333, "choice"),
                            RandomFlip()])
    for seed in range(100):
        np.random.seed(seed)
        ps = [aug.draw(h, w)[1] for h, w in sizes]
        if ({p.flip for p in ps} == {False, True} and any(max(p.new_size) == 1333 for p in ps)
                and any(min(p.new_size) == 800 and max(p.new_size) >= 1200 for p in ps)):
            return sizes, ps
    raise AssertionError("no seed shows the wanted draws")


def test_full_size_batch_equals_the_pinned_pieces_and_launch_count_is_constant():
    from lvc_amd import kernels as K
    from lvc_amd.data import resample_coeffs
    from lvc_amd.structures import ImageList

    mean, std = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]
    sizes, ps = _full_size_draws()
    g = torch.Generator().manual_seed(8)
    raws = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(DEV) for h, w in sizes]
    launches = {}
    for B in (8, 2):
        Hp, Wp = ImageList.padded_size([p.new_size for p in ps[:B]], 32)
        buf = torch.full((B, Hp, Wp, 4), float("nan"), device=DEV)
        u8 = K.train_input_u8(raws[:B], [p.job() for p in ps[:B]], buf, mean, std, resample_coeffs, want_u8=True)
        launches[B] = K.TRAIN_INPUT_LAUNCHES[-1]
        refs = [_pieces(r, p) for r, p in zip(raws[:B], ps[:B])]
        ref_buf = torch.full((B, Hp, Wp, 4), float("nan"), device=DEV)
        K.preprocess_batch_into([r.permute(2, 0, 1) for r in refs], ref_buf, mean, std)
        for i in range(B):
            assert tuple(u8[i].shape) == tuple(refs[i].shape) and torch.equal(u8[i], refs[i]), (B, i, ps[i])
            assert torch.equal(buf[i], ref_buf[i]), (B, i, ps[i])
    print("kernel launches per call: batch of 8: %d, batch of 2: %d" % (launches[8], launches[2]))
    assert launches[8] == launches[2] == 2


def test_strided_source_is_read_in_place():
    """A CHW tensor viewed as HWC (strides (W, 1, H*W)) gives what its contiguous copy gives."""
    from lvc_amd import kernels as K
    from lvc_amd.data import resample_coeffs

    g = torch.Generator().manual_seed(4)
    chw = torch.randint(0, 256, (3, 90, 130), generator=g, dtype=torch.uint8).to(DEV)
    view = chw.permute(1, 2, 0)
    job = (7, 11, 100, 60, 90, 150, True)
    outs = []
    for src in (view, view.contiguous()):
        buf = torch.empty(1, 96, 160, 4, device=DEV)
        outs.append((K.train_input_u8([src], [job], buf, [1.0, 2.0, 3.0], [2.0, 4.0, 8.0], resample_coeffs, want_u8=True)[0], buf))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_bad_jobs_are_refused_before_any_launch():
    from lvc_amd import kernels as K
    from lvc_amd.data import resample_coeffs

    raw = torch.zeros(40, 50, 3, dtype=torch.uint8, device=DEV)
    buf = torch.empty(1, 64, 64, 4, device=DEV)
    for job in ((20, 0, 40, 40, 40, 40, False),      # window past the right edge
                (0, 0, 50, 40, 80, 100, False)):     # output larger than the padded batch
        with pytest.raises(RuntimeError, match="lvc_train_input_u8"):
            K.train_input_u8([raw], [job], buf, [0, 0, 0], [1, 1, 1], resample_coeffs)


def _toy_dataset(n, seed):
    """n dataset dicts with pinned uint8 images of mixed orientation and a few boxes each."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        h, w = ((200, 300), (300, 210), (180, 320), (260, 190))[i % 4]
        h, w = h + 7 * (i // 4), w + 5 * (i // 4)
        raw = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).pin_memory()
        annos = []
        for k in range(3):
            x, y = float(torch.rand((), generator=g)) * w * 0.5, float(torch.rand((), generator=g)) * h * 0.5
            annos.append({"bbox": [x, y, 30 + 0.3 * w, 30 + 0.3 * h], "bbox_mode": 1, "category_id": (3 * i + k) % 20, "id": 10 * i + k})
        out.append({"raw": raw, "height": h, "width": w, "image_id": i, "annotations": annos})
    return out


def _loader_cfg():
    from lvc_amd.config.presets import base_rcnn_fpn

    cfg = base_rcnn_fpn(num_classes=20)
    cfg.defrost()
    cfg.MODEL.DEVICE = DEV
    cfg.INPUT.MIN_SIZE_TRAIN = (224, 240, 256)
    cfg.INPUT.MAX_SIZE_TRAIN = 360
    cfg.INPUT.CROP.ENABLED = True
    cfg.SOLVER.IMS_PER_BATCH = 2
    cfg.freeze()
    return cfg


@pytest.fixture(scope="module")
def train_model():
    from test_gpu_train import _train_model

    return _train_model()


def _step(model, batch):
    from lvc_amd.utils.events import EventStorage

    for p in model.parameters():
        p.grad = None
    torch.manual_seed(5)
    with EventStorage(0):
        losses = model(batch)
        sum(losses.values()).backward()
    return losses


def test_model_sees_what_the_image_path_builds(train_model):
    from lvc_amd.data import build_detection_train_loader

    model = train_model
    data = _toy_dataset(6, 1)
    np.random.seed(11)
    loader = build_detection_train_loader(_loader_cfg(), data, seed=3, size_divisibility=model.backbone.size_divisibility)
    batch = next(loader)
    assert len(batch) == 2 and all("image" not in b for b in batch)
    images = model.preprocess_image(batch)
    plain = [{"image": _pieces(data[b["index"]]["raw"], b["train_input_params"]).permute(2, 0, 1).contiguous(),
              "instances": b["instances"], "height": b["height"], "width": b["width"]} for b in batch]
    ref = model.preprocess_image(plain)
    assert images.image_sizes == ref.image_sizes and images.tensor.shape == ref.tensor.shape
    assert images.tensor.stride() == ref.tensor.stride() and torch.equal(images.tensor, ref.tensor)
    for b, q in zip(batch, plain):      # _forward_train moves x["instances"] of either batch: the same objects' fields
        assert b["instances"].image_size == tuple(b["train_input_params"].new_size)
        assert torch.equal(b["instances"].gt_boxes.tensor, q["instances"].gt_boxes.tensor) and len(b["instances"]) > 0
    runs = [_step(model, plain), _step(model, plain), _step(model, batch)]
    for losses in runs:
        assert set(losses) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"}
        assert all(bool(torch.isfinite(v).all()) for v in losses.values())
    repeatable = all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    print("two steps of the image path on identical inputs bit-identical:", repeatable)
    print({k: (float(runs[0][k].detach()), float(runs[2][k].detach())) for k in runs[0]})
    if repeatable:
        for k in runs[0]:
            assert torch.equal(runs[0][k], runs[2][k]), k


def test_two_buffers_in_flight_equal_one_batch_at_a_time(train_model):
    """20 consecutive loader batches, each read AFTER the training step that consumed it, equal the same batches prepared one at a
    time on the step's own stream with a wait after each: a buffer overwritten before its step had finished would differ."""
    from lvc_amd.data import build_detection_train_loader

    model = train_model
    data = _toy_dataset(8, 2)
    seen = {}
    for sync in (True, False):
        np.random.seed(21)
        loader = build_detection_train_loader(_loader_cfg(), data, seed=9, size_divisibility=model.backbone.size_divisibility, sync=sync)
        rows = []
        for batch in itertools.islice(loader, 20):
            losses = _step(model, batch)
            assert all(bool(torch.isfinite(v).all()) for v in losses.values())
            pb = batch[0]["prepared"]
            rows.append(([b["index"] for b in batch], list(pb.sizes), pb.buffer.clone(),
                         [b["instances"].gt_boxes.tensor.clone() for b in batch]))
        torch.cuda.synchronize()
        seen[sync] = rows
    assert len(seen[True]) == len(seen[False]) == 20
    for k, (a, b) in enumerate(zip(seen[True], seen[False])):
        assert a[0] == b[0] and a[1] == b[1], k
        assert a[2].shape == b[2].shape and torch.equal(a[2], b[2]), k
        assert all(torch.equal(x, y) for x, y in zip(a[3], b[3])), k
