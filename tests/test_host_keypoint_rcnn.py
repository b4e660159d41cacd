"""Keypoint R-CNN without a GPU: the restatements of tests/keypoint_ref.py against torch and the reference's stored outputs, the
model's state_dict against detectron2's, the refusals and the wire format."""
import ast
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import keypoint_ref as kr
from helpers import ROOT, gold

TRAIN_REFUSAL = "training the keypoint branch (MODEL.KEYPOINT_ON: keypoint_rcnn_loss, gt_keypoints) is not built"


def _cfg(**kw):
    from lvc_amd.config.presets import keypoint_rcnn_fpn

    return keypoint_rcnn_fpn(device="cpu", **kw)


@pytest.fixture(scope="module")
def model():
    from lvc_amd.modeling import build_model

    return build_model(_cfg())


def test_keypoint_model_has_the_reference_state_dict(model):
    g = gold("keypoint_rcnn_r50_fpn_keys")
    want = dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
    got = {k: str(tuple(v.shape)) for k, v in model.state_dict().items()}
    assert got == want
    assert list(got) == list(want)
    assert got["roi_heads.keypoint_head.score_lowres.weight"] == "(512, 17, 4, 4)"
    assert sum(1 for k in got if k.startswith("roi_heads.keypoint_head.conv_fcn")) == 16
    sd = {k: torch.full(ast.literal_eval(s), 0.5) for k, s in want.items()}
    missing, unexpected = model.load_state_dict(sd, strict=True)
    assert not missing and not unexpected


def test_keypoint_head_init_is_the_references():
    from lvc_amd.modeling import build_model

    torch.manual_seed(0)
    head = build_model(_cfg()).roi_heads.keypoint_head
    for name, p in head.named_parameters():
        if name.endswith("bias"):
            assert float(p.detach().abs().max()) == 0.0, name
    # kaiming_normal_(fan_out, relu): std = sqrt(2 / (size(0) * receptive field)) for conv and transposed conv alike
    w = head.conv_fcn2.weight
    assert abs(float(w.detach().std()) / (2.0 / (512 * 9)) ** 0.5 - 1) < 0.02
    w = head.score_lowres.weight
    assert abs(float(w.detach().std()) / (2.0 / (512 * 16)) ** 0.5 - 1) < 0.02


def test_box_only_model_is_the_parents(model):
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.modeling import build_model

    base = build_model(base_rcnn_fpn(device="cpu"))
    g = gold("r50_fpn_state_dict_keys")
    got = {k: str(tuple(v.shape)) for k, v in base.state_dict().items()}
    assert got == dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
    assert list(got) == g["keys"].tolist()
    assert not hasattr(base.roi_heads, "keypoint_head") and not hasattr(base.roi_heads, "keypoint_pooler")
    assert base.roi_heads.keypoint_on is False
    assert "keypoint" not in repr(base).lower()
    # the keypoint model adds the keypoint modules and nothing else (one class: the predictor's shapes differ, the names do not)
    assert [k for k in model.state_dict() if ".keypoint_head." not in k] == list(base.state_dict())


def test_header_declares_and_library_exports_the_entries():
    from lvc_amd import _lib

    text = open(os.path.join(ROOT, "include", "lvc_amd.h")).read()
    L = _lib.lib()
    for name in ("lvc_keypoint_deconv", "lvc_keypoint_deconv_pack", "lvc_keypoint_deconv_packed_rows", "lvc_heatmaps_to_keypoints"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert getattr(L, name) is not None
    assert L.lvc_keypoint_deconv_packed_rows(17) == 16 * 32 and L.lvc_keypoint_deconv_packed_rows(33) == 16 * 64
    assert "lowest" in text[text.index("lvc_heatmaps_to_keypoints"):].lower()      # the tie rule is stated in the header


def test_preset_and_refusals_name_their_keys(model):
    from lvc_amd import kernels as K
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.evaluation import GraphedInference, PipelinedInference, inference_on_dataset
    from lvc_amd.layers import ConvTranspose2d
    from lvc_amd.modeling import build_model

    cfg = _cfg()
    assert cfg.MODEL.KEYPOINT_ON is True and cfg.MODEL.ROI_HEADS.NUM_CLASSES == 1 and cfg.MODEL.MASK_ON is False
    assert base_rcnn_fpn().MODEL.KEYPOINT_ON is False
    for pairs, pat in (((("MODEL.MASK_ON", True),), "MODEL.KEYPOINT_ON together with MODEL.MASK_ON"),
                       ((("MODEL.ROI_HEADS.NAME", "CascadeROIHeads"),), "MODEL.KEYPOINT_ON with MODEL.ROI_HEADS.NAME"),
                       ((("MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS", [512, 200]),), "MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS"),
                       ((("MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS", 65),), "MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS")):
        bad = _cfg()
        for key, value in pairs:
            bad.merge_from_list([key, value])
        with pytest.raises(NotImplementedError, match=re.escape(pat)):
            build_model(bad)
    model.train()
    try:
        with pytest.raises(NotImplementedError, match=re.escape(TRAIN_REFUSAL)):
            model([{"image": torch.zeros(3, 32, 32)}])
        with pytest.raises(NotImplementedError, match=re.escape(TRAIN_REFUSAL)):
            model.roi_heads(None, {}, [], None)
        with pytest.raises(NotImplementedError, match=re.escape(TRAIN_REFUSAL)):
            model.roi_heads.keypoint_head(torch.zeros(1, 256, 14, 14), [])
    finally:
        model.eval()
    with pytest.raises(NotImplementedError, match="MODEL.KEYPOINT_ON"):
        GraphedInference(model, [{"image": torch.zeros(3, 32, 32)}])
    with pytest.raises(NotImplementedError, match="MODEL.KEYPOINT_ON"):
        PipelinedInference.__new__(PipelinedInference).__init__(model)
    with pytest.raises(NotImplementedError, match="MODEL.KEYPOINT_ON"):
        inference_on_dataset(model, [])
    for cin, k, pat in ((8, 17, "CONV_DIMS"), (40, 17, "CONV_DIMS"), (64, 0, "NUM_KEYPOINTS"), (64, 65, "NUM_KEYPOINTS")):
        with pytest.raises(NotImplementedError, match=pat):
            K.keypoint_deconv_check(cin, k)
    K.keypoint_deconv_check(K.KEYPOINT_DECONV_CIN, 1)
    K.keypoint_deconv_check(512, 17)
    # the wrapper takes the two triples on the path and keeps refusing the others
    assert ConvTranspose2d(32, 5, 4, stride=2, padding=1).weight.shape == (32, 5, 4, 4)
    assert ConvTranspose2d(64, 64, 2, stride=2, padding=0).weight.shape == (64, 64, 2, 2)
    for triple in ((3, 2, 1), (4, 2, 0), (4, 4, 1), (2, 2, 1)):
        with pytest.raises(NotImplementedError, match="only the mask head's ConvTranspose2d"):
            ConvTranspose2d(64, 64, triple[0], stride=triple[1], padding=triple[2])
    with pytest.raises(NotImplementedError):
        ConvTranspose2d(32, 5, 4, stride=2, padding=1)(torch.zeros(1, 32, 4, 4))


# ------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("shape", [(2, 5, 8, 3), (1, 1, 4, 1), (2, 14, 16, 17)])
def test_ref_deconv_is_torchs(shape):
    M, S, cin, k = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(M, S, S, cin, generator=g, dtype=torch.float64)
    w = torch.randn(cin, k, 4, 4, generator=g, dtype=torch.float64)
    b = torch.randn(k, generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(x.permute(0, 3, 1, 2), w, b, stride=2, padding=1)
    assert float((kr.deconv4x4_s2_p1(x, w, b) - want).abs().max()) < 1e-12


def test_ref_bilinear_and_bicubic_are_atens():
    maps = kr.smooth_maps(2, 3, 5).double()
    want = F.interpolate(maps, scale_factor=2, mode="bilinear", align_corners=False)
    assert float((kr.bilinear_up2(maps) - want).abs().max()) < 1e-13
    m56 = kr.bilinear_up2(kr.bilinear_up2(maps))[0]
    for oh, ow in ((1, 1), (123, 1), (56, 56), (13, 31), (130, 199), (7, 300), (112, 112)):
        assert float((kr.bicubic_resize(m56, oh, ow) - kr.interpolate_bicubic(m56, oh, ow)).abs().max()) < 1e-12, (oh, ow)
    assert torch.equal(kr.bicubic_resize(m56, 56, 56), m56)      # the identity resize is exact


def test_ref_lowest_index_rule():
    flat = torch.tensor([[1.0, 5.0, 5.0, 2.0], [7.0, 7.0, 7.0, 7.0], [0.0, 1.0, 2.0, 3.0]])
    assert kr.lowest_argmax(flat).tolist() == [1, 0, 3]
    assert kr.lowest_argmax(flat).tolist() == flat.argmax(1).tolist()      # torch.argmax on the CPU takes the first maximum
    const = torch.full((1, 2, 56, 56), 4.0, dtype=torch.float64)
    out, pos = kr.heatmaps_to_keypoints(const, torch.tensor([[10.0, 20.0, 66.0, 76.0]]))
    assert pos.tolist() == [[[0, 0], [0, 0]]] and out[0, :, :2].tolist() == [[10.5, 20.5]] * 2


@pytest.mark.parametrize("case", [0, 1])
def test_ref_decode_gives_the_references_keypoints(case):
    """The restatement on the reference head's own maps (small case), or on maps the restated deconv and upsampling make from the
    seeded operands (both cases), against detectron2's stored heatmaps_to_keypoints in fp64."""
    from lvc_amd.utils import synthetic as syn

    g = gold("keypoint_head_small")
    M, S, cin, k = [int(v) for v in g["cases"][case]]
    x, w, b, boxes = syn.keypoint_head_case(M, S, cin, k)
    assert torch.equal(boxes, g["boxes_%d" % case])
    maps = kr.bilinear_up2(kr.deconv4x4_s2_p1(x.permute(0, 2, 3, 1).double(), w.double(), b.double()))
    if "maps64_%d" % case in g:
        assert float((maps - g["maps64_%d" % case]).abs().max()) < 1e-10
        assert float((g["maps32_%d" % case].double() - maps).abs().max()) < 1e-4
    out, _pos = kr.heatmaps_to_keypoints(maps, boxes)
    want = g["kp64_%d" % case]
    assert float((out[:, :, :2] - want[:, :, :2]).abs().max()) < 1e-4      # (our boxes stay fp32 in the position expression)
    assert float((out[:, :, 2:] - want[:, :, 2:]).abs().max()) < 1e-9


def test_xy_expression_is_the_references_fp32_bits():
    """At the reference's own positions, the numpy fp32 expression gives the reference's fp32 (x, y) bit for bit."""
    g = gold("keypoint_head_small")
    for case in (0, 1):
        kp32, boxes = g["kp32_%d" % case], g["boxes_%d" % case]
        for i in range(kp32.shape[0]):
            oh, ow, h, w = kr.box_out_size(boxes[i].numpy())
            for k in range(kp32.shape[1]):
                xi = int(np.floor((float(kp32[i, k, 0]) - float(boxes[i, 0])) / (float(w) / ow)))
                yi = int(np.floor((float(kp32[i, k, 1]) - float(boxes[i, 1])) / (float(h) / oh)))
                cands = [kr.xy_from_position(boxes[i].numpy(), a, c) for a in (xi - 1, xi, xi + 1) for c in (yi - 1, yi, yi + 1)]
                assert (np.float32(kp32[i, k, 0]), np.float32(kp32[i, k, 1])) in cands, (case, i, k)


# ------------------------------------------------------------------ wire, postprocess
def test_wire_writes_the_keypoints_field():
    from lvc_amd.structures import Boxes, Instances
    from lvc_amd.wire import instances_to_coco_json

    inst = Instances((100, 120))
    inst.pred_boxes = Boxes(torch.tensor([[10.0, 20.0, 50.0, 80.0], [1.0, 2.0, 3.0, 4.0]]))
    inst.scores = torch.tensor([0.75, 0.5])
    inst.pred_classes = torch.tensor([0, 0])
    inst.pred_keypoints = torch.tensor([[[12.5, 30.5, 0.25], [40.0, 70.25, 0.125]], [[1.5, 2.5, 0.5], [2.0, 3.0, 0.0625]]])
    rows = instances_to_coco_json(inst, 7)
    assert rows[0] == {"image_id": 7, "category_id": 0, "bbox": [10.0, 20.0, 40.0, 60.0], "score": 0.75,
                       "keypoints": [12.0, 30.0, 0.25, 39.5, 69.75, 0.125]}
    assert rows[1]["keypoints"] == [1.0, 2.0, 0.5, 1.5, 2.5, 0.0625]
    assert inst.pred_keypoints[0, 0, 0] == 12.5      # the instances keep their values
    del inst._fields["pred_keypoints"]
    assert "keypoints" not in instances_to_coco_json(inst, 7)[0]


def test_detector_postprocess_scales_keypoints_and_does_not_clip_them():
    from lvc_amd.modeling import detector_postprocess
    from lvc_amd.structures import Boxes, Instances

    inst = Instances((50, 100))
    inst.pred_boxes = Boxes(torch.tensor([[10.0, 20.0, 50.0, 45.0], [5.0, 5.0, 5.0, 9.0]]))      # the second is empty: dropped
    inst.scores = torch.tensor([0.75, 0.5])
    inst.pred_classes = torch.tensor([0, 0])
    inst.pred_keypoints = torch.tensor([[[12.5, 30.5, 0.25], [120.0, -3.0, 0.125]], [[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]])
    out = detector_postprocess(inst, 75, 300)
    assert len(out) == 1
    sx, sy = np.float32(300 / 100), np.float32(75 / 50)
    want = [[float(np.float32(12.5) * sx), float(np.float32(30.5) * sy), 0.25], [float(np.float32(120.0) * sx), float(np.float32(-3.0) * sy), 0.125]]
    assert out.pred_keypoints.tolist() == [want]
