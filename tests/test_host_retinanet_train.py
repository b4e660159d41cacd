"""RetinaNet training on the host: tests/retinanet_loss_ref.py -- the expected value of the GPU tests -- reproduces the labels and the
normaliser the reference's own training step produced (tests/golden/retinanet_train.npz, scripts/make_golden_retinanet_train.py), the
loss entries are declared and exported, and training is opt-in with its refusals naming their keys.  No kernel is launched."""
import ctypes
import os
import re

import pytest
import torch

import retinanet_loss_ref as lref
from helpers import ROOT, gold

SHAPES = ((16, 24), (8, 12), (4, 6), (2, 3), (1, 2))
STRIDES = (8, 16, 32, 64, 128)
K = 20


def _cfg(**kw):
    from lvc_amd.config.presets import retinanet_r_fpn

    return retinanet_r_fpn(device="cpu", **kw)


def _anchors():
    from lvc_amd.modeling.anchor_generator import DefaultAnchorGenerator

    out = []
    for (h, w), s, x in zip(SHAPES, STRIDES, (32, 64, 128, 256, 512)):
        cell = DefaultAnchorGenerator.generate_cell_anchors([x, x * 2 ** (1.0 / 3), x * 2 ** (2.0 / 3)], (0.5, 1.0, 2.0)).float()
        sx = torch.arange(0, w * s, step=s, dtype=torch.float32)
        sy = torch.arange(0, h * s, step=s, dtype=torch.float32)
        yy, xx = torch.meshgrid(sy, sx, indexing="ij")
        shifts = torch.stack((xx.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1)), 1)
        out.append((shifts.view(-1, 1, 4) + cell.view(1, -1, 4)).reshape(-1, 4))
    return torch.cat(out)


def cases():
    g = gold("retinanet_train")
    a = ([g["a_gt_boxes0"], g["a_gt_boxes1"]], [g["a_gt_classes0"], g["a_gt_classes1"]], g["a_gt_labels"], g["a_matched"])
    b = ([g["b_gt_boxes0"], torch.zeros(0, 4)], [g["b_gt_classes0"], torch.zeros(0, dtype=torch.int64)], g["b_gt_labels"], g["b_matched"])
    return {"a": a, "b": b}


@pytest.mark.parametrize("case", ["a", "b"])
def test_mirror_label_anchors_reproduces_the_reference_exactly(case):
    boxes, classes, want_labels, want_matched = cases()[case]
    anchors = _anchors()
    assert anchors.shape == (4608, 4)
    labels, matched, _ = lref.label_anchors(anchors, boxes, classes, K)
    assert torch.equal(labels, want_labels.long())
    pos = (want_labels >= 0) & (want_labels != K)
    assert torch.equal(matched[pos], want_matched.long()[pos])
    if case == "b":
        assert int(pos[0].sum()) == 120 and int(pos[1].sum()) == 0 and bool((labels[1] == K).all())
    else:
        assert pos.sum(1).tolist() == [82, 96] and (want_labels < 0).sum(1).tolist() == [141, 116]


def test_mirror_ema_reproduces_the_reference_normaliser_bit_for_bit():
    g = gold("retinanet_train")
    n = int(g["num_pos"].sum())
    n1 = lref.ema(100, n)
    n2 = lref.ema(n1, n)
    assert [n1, n2] == [float(v) for v in g["normalizer"]]
    assert (1 - 0.9) == 0.09999999999999998          # the factor the reference multiplies by: not 0.1


def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "lvc_amd.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "lvc_amd", "liblvc_amd.so"))
    for name in ("lvc_retinanet_loss", "lvc_retinanet_loss_grad"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert getattr(lib, name) is not None


def test_training_is_opt_in():
    from lvc_amd.modeling import build_model

    model = build_model(_cfg())
    assert model.enable_training() is model
    model.enable_training(False)
    model.train()
    with pytest.raises(NotImplementedError, match="RetinaNet training") as e:
        model([{"image": torch.zeros(3, 32, 32)}])
    assert "enable_training" in str(e.value)
    assert model.loss_normalizer == 100
    model.loss_normalizer = 107.8
    assert model.loss_normalizer == 107.8


def test_unbuilt_training_settings_name_their_key():
    from lvc_amd.modeling import build_model

    cfg = _cfg()
    cfg.MODEL.RETINANET.FOCAL_LOSS_GAMMA = 0.5
    with pytest.raises(NotImplementedError, match="MODEL.RETINANET.FOCAL_LOSS_GAMMA"):
        build_model(cfg).enable_training()
    cfg = _cfg()
    cfg.VIS_PERIOD = 1
    with pytest.raises(NotImplementedError, match="VIS_PERIOD"):
        build_model(cfg).enable_training()
    cfg = _cfg()
    cfg.MODEL.RETINANET.NORM = "GN"
    with pytest.raises(NotImplementedError, match="MODEL.RETINANET.NORM"):
        build_model(cfg)


def test_state_dict_keys_are_the_reference_after_enable_training():
    from lvc_amd.modeling import build_model

    model = build_model(_cfg()).enable_training()
    g = gold("retinanet_r50_fpn_keys")
    assert list(model.state_dict()) == g["keys"].tolist()
    assert {k: str(tuple(v.shape)) for k, v in model.state_dict().items()} == dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
