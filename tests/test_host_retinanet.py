"""RetinaNet on the host: the preset builds, its state_dict is the reference's (tests/golden/retinanet_r50_fpn_keys.npz), training
refuses, and tests/retinanet_ref.py -- the expected value of the GPU tests -- reproduces the candidates the reference's own
`inference_single_image` hands to its NMS (tests/golden/retinanet_r50_fpn_small.npz, scripts/make_golden_retinanet.py).  No kernel is
launched."""
import pytest
import torch

import retinanet_ref as ref
from helpers import gold

LEVELS = ("p3", "p4", "p5", "p6", "p7")
STRIDES = (8, 16, 32, 64, 128)


def _cfg(**kw):
    from lvc_amd.config.presets import retinanet_r_fpn

    return retinanet_r_fpn(device="cpu", **kw)


@pytest.fixture(scope="module")
def model():
    from lvc_amd.modeling import build_model

    return build_model(_cfg())


def test_preset_builds_with_the_reference_state_dict(model):
    from lvc_amd.modeling import LastLevelP6P7, RetinaNet, RetinaNetHead

    g = gold("retinanet_r50_fpn_keys")
    want = dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
    got = {k: str(tuple(v.shape)) for k, v in model.state_dict().items()}
    assert got == want
    assert list(got) == list(want)
    assert isinstance(model, RetinaNet) and isinstance(model.head, RetinaNetHead) and isinstance(model.backbone.top_block, LastLevelP6P7)
    assert tuple(model.head.cls_score.weight.shape) == (720, 256, 3, 3) and tuple(model.head.bbox_pred.weight.shape) == (36, 256, 3, 3)
    assert abs(float(model.head.cls_score.bias.detach()[0]) + 4.59512) < 1e-4          # -log((1 - 0.01) / 0.01)
    assert float(model.head.cls_subnet[0].weight.std()) < 0.011 and float(model.head.bbox_pred.bias.abs().max()) == 0.0
    assert [len(c) for c in model.anchor_generator.cell_anchors] == [9] * 5


def test_reference_shaped_state_dict_loads_strictly(model):
    g = gold("retinanet_r50_fpn_keys")
    sd = {k: torch.full(eval(s), 0.5) for k, s in zip(g["keys"].tolist(), g["shapes"].tolist())}
    sd["pixel_mean"] = torch.tensor([1.0, 2.0, 3.0]).view(3, 1, 1)
    sd["pixel_std"] = torch.tensor([4.0, 5.0, 6.0]).view(3, 1, 1)
    missing, unexpected = model.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    assert float(model.head.cls_subnet[6].weight.detach().mean()) == 0.5 and float(model.backbone.top_block.p7.bias.detach().mean()) == 0.5
    assert model._mean_std() == ([1.0, 2.0, 3.0], [4.0, 5.0, 6.0])      # the preprocess kernels' host copies follow the checkpoint


def test_output_shape_is_p3_to_p7(model):
    shapes = model.backbone.output_shape()
    assert list(shapes) == list(LEVELS)
    assert [shapes[k].stride for k in LEVELS] == list(STRIDES) and all(shapes[k].channels == 256 for k in LEVELS)
    assert model.in_features == list(LEVELS) and model.backbone.size_divisibility == 32


def test_training_forward_refuses(model):
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="RetinaNet training"):
            model([{"image": torch.zeros(3, 32, 32)}])
    finally:
        model.eval()


def test_unbuilt_settings_name_their_key():
    from lvc_amd.modeling import GeneralizedRCNNWithTTA, build_model

    cfg = _cfg()
    cfg.MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS = [[0.5, 1.0, 2.0], [1.0], [1.0], [1.0], [1.0]]
    with pytest.raises(NotImplementedError, match="ANCHOR_GENERATOR"):
        build_model(cfg)
    with pytest.raises(AssertionError):
        GeneralizedRCNNWithTTA(_cfg(), build_model(_cfg()))


def test_preset_keys_and_the_r50_rcnn_tree_is_unchanged():
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.modeling import build_model

    M = _cfg(num_classes=20).MODEL
    assert M.META_ARCHITECTURE == "RetinaNet" and M.BACKBONE.NAME == "build_retinanet_resnet_fpn_backbone"
    assert M.RESNETS.OUT_FEATURES == M.FPN.IN_FEATURES == ["res3", "res4", "res5"] and M.RETINANET.NUM_CLASSES == 20
    assert [[round(v, 4) for v in s] for s in M.ANCHOR_GENERATOR.SIZES][:2] == [[32, 40.3175, 50.7968], [64, 80.6349, 101.5937]]
    rcnn = build_model(base_rcnn_fpn(device="cpu"))
    g = gold("r50_fpn_state_dict_keys")
    assert {k: str(tuple(v.shape)) for k, v in rcnn.state_dict().items()} == dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
    assert rcnn._mean_std() == (rcnn.pixel_mean, rcnn.pixel_std)


def test_ref_selection_reproduces_the_reference_candidates():
    """retinanet_ref on the fixture's fp32 logits and deltas against the candidates the reference's inference_single_image handed to
    its NMS: the same entries per (image, level), the same order up to permutations inside groups of equal fp32 score (the reference
    sorts the probabilities, the restatement the logits), equal scores, bit-equal boxes.  Entries whose membership rounding may decide
    (tied with the cut, or within 1e-6 of the threshold) are set aside: at most 1 % of a level's candidates."""
    from lvc_amd.modeling.anchor_generator import DefaultAnchorGenerator

    # (the restatement's shortcut -- everything above the k-th value, then the lowest indices equal to it -- is the head of a stable sort)
    x = (torch.randn(5000, generator=torch.Generator().manual_seed(5)) * 2).round() / 2          # many equal values
    full = torch.sort(x, descending=True, stable=True)[1]
    for k in (1, 7, 100, 1000, 4999, 5000, 6000):
        assert torch.equal(ref.stable_topk(x, k), full[:k])
    g = gold("retinanet_r50_fpn_small")
    K, topk, thresh = 20, 1000, 0.05
    sizes = [[x, x * 2 ** (1.0 / 3), x * 2 ** (2.0 / 3)] for x in (32, 64, 128, 256, 512)]
    cells = [DefaultAnchorGenerator.generate_cell_anchors(s, (0.5, 1.0, 2.0)).float() for s in sizes]
    ours = ref.select_pyramid([g["logits_" + k] for k in LEVELS], [g["deltas_" + k] for k in LEVELS], cells, STRIDES, 0.0, K, topk, thresh)
    checked = 0
    for b in range(2):
        for l in range(5):
            m = (g["cand_image"] == b) & (g["cand_level"] == l)
            want_i, want_s, want_c, want_b = g["cand_index"][m].long(), g["cand_score"][m], g["cand_class"][m].long(), g["cand_box"][m]
            got_i, got_s, got_c, got_b = ours[b][l]
            n = max(len(want_i), len(got_i))
            aside = set(want_i.tolist()) ^ set(got_i.tolist())
            assert len(aside) <= 0.01 * n, (b, l, len(aside), n)
            for scores, index in ((want_s, want_i), (got_s, got_i)):
                for i in aside & set(index.tolist()):
                    s = float(scores[index == i])
                    assert s == float(scores.min()) or abs(s - thresh) <= 1e-6, (b, l, i, s)
            kw, kg = [torch.tensor([i not in aside for i in idx.tolist()], dtype=torch.bool) for idx in (want_i, got_i)]
            want_i, want_s, want_c, want_b = want_i[kw], want_s[kw], want_c[kw], want_b[kw]
            got_i, got_s, got_c, got_b = got_i[kg], got_s[kg], got_c[kg], got_b[kg]
            assert torch.equal(got_s, want_s), (b, l)                      # both descending: equal as sequences
            # canonical order inside equal-score groups: by index
            ow = torch.tensor(sorted(range(len(want_i)), key=lambda r: (-float(want_s[r]), int(want_i[r]))), dtype=torch.long)
            og = torch.tensor(sorted(range(len(got_i)), key=lambda r: (-float(got_s[r]), int(got_i[r]))), dtype=torch.long)
            assert torch.equal(got_i[og], want_i[ow]) and torch.equal(got_c[og], want_c[ow]), (b, l)
            assert torch.equal(got_b[og], want_b[ow]), (b, l, float((got_b[og] - want_b[ow]).abs().max()))
            checked += len(want_i)
    assert checked > 2000
