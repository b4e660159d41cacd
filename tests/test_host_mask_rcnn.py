"""Mask R-CNN (MODEL.MASK_ON) on the host: the model builds with the reference's state_dict (tests/golden/mask_rcnn_r50_fpn_keys.npz,
scripts/make_golden_mask_rcnn.py), a box-only model is untouched, the two new entries are declared and exported, what is not built says
so under its config key, and tests/mask_ref.py -- the restatement the GPU tests measure the kernels against -- agrees with torch's own
operators and with the reference's masks.  No kernel is launched."""
import ast
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mask_ref
from helpers import ROOT, gold


def _cfg(**kw):
    from lvc_amd.config.presets import mask_rcnn_fpn

    return mask_rcnn_fpn(device="cpu", **kw)


@pytest.fixture(scope="module")
def model():
    from lvc_amd.modeling import build_model

    return build_model(_cfg())


def test_mask_model_has_the_reference_state_dict(model):
    g = gold("mask_rcnn_r50_fpn_keys")
    want = dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
    got = {k: str(tuple(v.shape)) for k, v in model.state_dict().items()}
    assert got == want
    assert list(got) == list(want)
    assert any(k.startswith("roi_heads.mask_head.deconv") for k in got)
    sd = {k: torch.full(ast.literal_eval(s), 0.5) for k, s in want.items()}
    missing, unexpected = model.load_state_dict(sd, strict=True)
    assert not missing and not unexpected


def test_box_only_model_is_the_parents(model):
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.modeling import build_model

    base = build_model(base_rcnn_fpn(device="cpu"))
    g = gold("r50_fpn_state_dict_keys")
    got = {k: str(tuple(v.shape)) for k, v in base.state_dict().items()}
    assert got == dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
    assert not hasattr(base.roi_heads, "mask_head") and not hasattr(base.roi_heads, "mask_pooler") and base.roi_heads.mask_on is False
    assert "mask" not in repr(base).lower()
    # the mask model adds the mask modules and nothing else
    assert [k for k in model.state_dict() if ".mask_head." not in k] == list(base.state_dict())


def test_header_declares_and_library_exports_the_entries():
    from lvc_amd import _lib

    text = open(os.path.join(ROOT, "include", "lvc_amd.h")).read()
    L = _lib.lib()
    for name in ("lvc_mask_deconv_predict", "lvc_paste_masks"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert getattr(L, name) is not None
    assert L.lvc_abi_version() == 1


def test_preset_and_refusals_name_their_keys():
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.evaluation import GraphedInference, PipelinedInference
    from lvc_amd.modeling import GeneralizedRCNNWithTTA, build_model

    cfg = _cfg()
    assert cfg.MODEL.MASK_ON is True and cfg.MODEL.ROI_MASK_HEAD.NUM_CONV == 4 and cfg.MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION == 14
    assert base_rcnn_fpn().MODEL.MASK_ON is False
    for key, value, pat in (("MODEL.ROI_MASK_HEAD.NORM", "GN", "MODEL.ROI_MASK_HEAD.NORM"), ("MODEL.ROI_MASK_HEAD.CONV_DIM", 96, "MODEL.ROI_MASK_HEAD.CONV_DIM")):
        bad = _cfg()
        bad.merge_from_list([key, value])
        with pytest.raises(NotImplementedError, match=pat):
            build_model(bad)
    m = build_model(cfg)
    m.train()
    with pytest.raises(NotImplementedError, match="training the mask branch"):
        m([{"image": torch.zeros(3, 32, 32)}])
    m.eval()
    with pytest.raises(NotImplementedError, match="MODEL.MASK_ON"):
        GeneralizedRCNNWithTTA(cfg, m)
    with pytest.raises(NotImplementedError, match="MODEL.MASK_ON"):
        GraphedInference(m, [{"image": torch.zeros(3, 32, 32)}])
    with pytest.raises(NotImplementedError, match="MODEL.MASK_ON"):
        PipelinedInference.__new__(PipelinedInference).__init__(m)
    with pytest.raises(NotImplementedError):
        m.roi_heads.mask_head.layers(torch.zeros(1, 256, 14, 14))
    from lvc_amd import kernels as K

    with pytest.raises(NotImplementedError, match="threshold"):      # only the reference's visualisation branch; 0 is a threshold
        K.paste_masks(torch.zeros(1, 28, 28), np.zeros((0, 8), np.int64), 0, threshold=-1.0)


def test_packed_deconv_operand_layout():
    from lvc_amd import kernels as K

    w = torch.arange(64 * 128 * 4, dtype=torch.float32).view(64, 128, 2, 2)
    p = K.pack_mask_deconv(w)
    assert p.shape == (4 * 128, 64)
    for dy, dx, co, ci in ((0, 0, 0, 0), (1, 0, 5, 63), (0, 1, 127, 1), (1, 1, 64, 17)):
        assert float(p[(dy * 2 + dx) * 128 + co, ci]) == float(w[ci, co, dy, dx])


@pytest.mark.parametrize("shape", [(1, 1, 64, 64, 1), (3, 7, 64, 128, 3), (4, 5, 128, 64, 6)])
def test_mask_ref_tail_is_torchs(shape):
    from lvc_amd.utils import synthetic as syn

    x, wd, bd, wp, bp, classes = syn.mask_tail_case(*shape)
    want = F.conv2d(F.relu(F.conv_transpose2d(x.double(), wd.double(), bd.double(), stride=2)), wp.double(), bp.double())
    want = want[torch.arange(len(classes)), classes].sigmoid()
    got = mask_ref.tail(x, wd, bd, wp, bp, classes)
    assert got.shape == want.shape and float((got - want).abs().max()) < 1e-12
    agn = mask_ref.tail(x, wd, bd, wp, bp, None)
    assert float((agn - F.conv2d(F.relu(F.conv_transpose2d(x.double(), wd.double(), bd.double(), stride=2)), wp.double(), bp.double())[:, 0].sigmoid()).abs().max()) < 1e-12


def test_mask_ref_tail_against_the_fixture():
    from lvc_amd.utils import synthetic as syn

    g = gold("mask_head_small")
    for i, case in enumerate(g["cases"].tolist()):
        x, wd, bd, wp, bp, classes = syn.mask_tail_case(*case)
        assert torch.equal(classes.to(torch.int32), g["classes_%d" % i])
        got = mask_ref.tail(x, wd, bd, wp, bp, classes)
        assert float((got - g["prob32_%d" % i].double()).abs().max()) <= float(g["err64_%d" % i]) + 1e-12


def test_mask_ref_paste_is_grid_sample():
    p, b, (H, W) = mask_ref.paste_inputs()
    soft = mask_ref.paste_soft(p, b, H, W)
    x0, y0, x1, y1 = [b[:, i:i + 1].double() for i in range(4)]
    gx = ((torch.arange(W, dtype=torch.float64)[None] + 0.5 - x0) / (x1 - x0) * 2 - 1)[:, None, :].expand(len(p), H, W)
    gy = ((torch.arange(H, dtype=torch.float64)[None] + 0.5 - y0) / (y1 - y0) * 2 - 1)[:, :, None].expand(len(p), H, W)
    want = F.grid_sample(p[:, None].double(), torch.stack([gx, gy], 3), align_corners=False)[:, 0]
    assert float((soft - want).abs().max()) < 1e-12
    assert soft[1].min() > 0 and not soft[6][10:].any()      # the whole-image box covers every pixel; the 1 x 1 box nothing far away


def test_mask_ref_paste_gives_the_fixtures_masks():
    """The reference model's own soft masks and boxes through mask_ref.paste (fp64) are the reference's bits outside the band."""
    g = gold("mask_rcnn_small")
    compared = aside = 0
    for i, (h, w) in enumerate(((128, 160), (120, 176))):
        n = len(g["det32_scores_%d" % i])
        bits = torch.from_numpy(np.unpackbits(g["masks32_%d" % i].numpy())[: n * h * w].reshape(n, h, w)).bool()
        band = torch.from_numpy(np.unpackbits(g["band_%d" % i].numpy())[: n * h * w].reshape(n, h, w)).bool()
        assert bits.any() and len(g["match_%d" % i]) == n and g["raw32_boxes_%d" % i].shape == (n, 4)
        twin = g["match_%d" % i] >= 0
        got = mask_ref.paste(g["prob32_%d" % i], g["det32_boxes_%d" % i], h, w)
        assert not ((got != bits) & ~band)[twin].any()
        compared += int(twin.sum()) * h * w
        aside += int(band[twin].sum())
    assert aside <= 1e-3 * compared
    assert float(g["share_compared"]) <= 1e-3 and 2.0 <= float(g["logit_std"]) <= 3.0


def test_wire_refuses_instances_with_masks():
    from lvc_amd.structures import Boxes, Instances
    from lvc_amd.wire import instances_to_coco_json

    inst = Instances((8, 8))
    inst.pred_boxes = Boxes(torch.tensor([[1.0, 1.0, 4.0, 4.0]]))
    inst.scores = torch.tensor([0.9])
    inst.pred_classes = torch.tensor([2])
    assert len(instances_to_coco_json(inst, 7)) == 1
    inst.pred_masks = torch.zeros(1, 8, 8, dtype=torch.bool)
    with pytest.raises(NotImplementedError, match="MODEL.MASK_ON"):
        instances_to_coco_json(inst, 7)
