"""Panoptic FPN on the host: tests/seg_ref.py -- the restatement the GPU tests compare bits against -- agrees with torch's own
operators and with the reference's outputs (tests/golden, scripts/make_golden_panoptic.py); the models build with the reference's
state_dict; what is not built says so under its config key; a box-only and a mask model are the parent's.  No kernel is launched."""
import ast
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_ref
from helpers import gold

K_BAR = 3.0


# ------------------------------------------------------------------------------------------------ seg_ref against torch and the fixtures
@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 3, 5, 128), (1, 7, 2, 64)])
def test_seg_ref_upsample2_against_torch(shape, with_acc):
    g = torch.Generator().manual_seed(sum(shape) + with_acc)
    N, H, W, C = shape
    x = torch.randn(shape, generator=g) * 3
    acc = torch.randn(N, 2 * H, 2 * W, C, generator=g) * 3 if with_acc else None
    got = torch.from_numpy(seg_ref.upsample2(x.numpy(), None if acc is None else acc.numpy()))

    def torch_ref(dtype):
        y = F.interpolate(x.to(dtype).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        return y if acc is None else acc.to(dtype) + y

    y64 = torch_ref(torch.float64)
    dev32 = float((torch_ref(torch.float32).double() - y64).abs().max())
    assert got.dtype == torch.float32 and float((got.double() - y64).abs().max()) <= K_BAR * dev32
    # the weights are 0.25 / 0.75 / 1 and the far taps clamp to the edge
    ty = seg_ref.tap(0.5, 2 * H, H)
    assert set(np.unique(ty[3]).tolist()) <= {0.0, 0.25, 0.75} and ty[1].max() == H - 1 and ty[0][0] == 0 and ty[3][0] == 0


def _band(bits, shape):
    return np.unpackbits(bits.numpy())[: shape[0] * shape[1]].reshape(shape).astype(bool)


def test_seg_ref_postprocess_against_the_reference_head_outputs():
    """The reference head's stride-4 logits through seg_ref's two stages: soft values within 3 x the reference's own |fp32 - fp64|,
    labels equal outside the band."""
    z = gold("sem_seg_head_small")
    image = tuple(int(v) for v in z["image"])
    low = np.ascontiguousarray(z["low6"].numpy().transpose(1, 2, 0))
    low = np.concatenate([low, np.full(low.shape[:2] + (2,), 1e30, np.float32)], axis=2)      # padding channels, never read
    for j, out in enumerate(tuple(int(v) for v in o) for o in z["outs"]):
        soft, labels = seg_ref.postprocess(low, 6, 4, image, out)
        assert soft.dtype == np.float32 and soft.shape == (6,) + out
        band = _band(z["band6_%d" % j], out)
        assert band.mean() <= 1e-3
        assert np.array_equal(labels[~band], z["labels6_%d" % j].numpy()[~band])
        if "soft6_%d" % j in z:
            err = float(np.abs(soft.astype(np.float64) - z["soft6_%d" % j].numpy()).max())
            assert err <= K_BAR * float(z["err64_6_%d" % j]), (out, err)


def test_seg_ref_postprocess_takes_the_lowest_class_on_ties_as_torch_does():
    low = np.zeros((3, 4, 5), np.float32)
    low[:, :, 3] = low[:, :, 1] = 2.0
    soft, labels = seg_ref.postprocess(low, 5, 4, (11, 15), (7, 9))
    assert (labels == 1).all()
    assert bool((torch.from_numpy(soft).argmax(0) == 1).all())


def _cases():
    z = gold("panoptic_combine_cases")
    for i, name in enumerate(z["names"].tolist()):
        H, W = (int(v) for v in z["shape_%d" % i])
        n = len(z["scores_%d" % i])
        masks = np.unpackbits(z["masks_%d" % i].numpy())[: n * H * W].reshape(n, H, W) if n else np.zeros((0, H, W), np.uint8)
        yield name, z, i, masks


def test_seg_ref_combine_gives_the_references_results_exactly():
    names = []
    for name, z, i, masks in _cases():
        thr, limit, conf = (float(v) for v in z["params"])
        scores = z["scores_%d" % i].numpy()
        above = scores[scores >= conf]
        assert len(set(above.tolist())) == len(above), "equal scores above the threshold: the reference's argsort is not stable"
        pan, info = seg_ref.combine(masks, scores, z["classes_%d" % i].numpy(), z["labels_%d" % i].numpy(), thr, limit, conf)
        assert np.array_equal(pan, z["pan_%d" % i].numpy()), name
        want = z["seg_%d" % i].numpy().reshape(-1, 5).tolist()
        assert [[s["id"], int(s["isthing"]), s["category_id"], s.get("instance_id", -1), s.get("area", -1)] for s in info] == want, name
        assert [s.get("score", 0.0) for s in info] == z["segscore_%d" % i].numpy().tolist(), name
        names.append(name)
    assert {"overlap_at_threshold", "overlap_over_threshold", "zero_area", "low_score_in_the_middle", "stuff_area_limits", "no_instances",
            "all_rejected", "small_canvas"} == set(names)


# ------------------------------------------------------------------------------------------------ the modules
def _cfg(**kw):
    from lvc_amd.config.presets import panoptic_fpn

    return panoptic_fpn(device="cpu", **kw)


@pytest.fixture(scope="module")
def model():
    from lvc_amd.modeling import build_model

    return build_model(_cfg())


def test_panoptic_model_has_the_reference_state_dict(model):
    g = gold("panoptic_fpn_keys")
    want = dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
    got = {k: str(tuple(v.shape)) for k, v in model.state_dict().items()}
    assert got == want
    for k in ("sem_seg_head.p2.0.weight", "sem_seg_head.p2.0.norm.weight", "sem_seg_head.p4.2.weight", "sem_seg_head.p5.4.norm.bias",
              "sem_seg_head.predictor.weight", "sem_seg_head.predictor.bias"):
        assert k in got
    assert not any(k.startswith(("sem_seg_head.p2.1", "sem_seg_head.p3.1.", "sem_seg_head.p5.1.")) for k in got)      # the upsample slots
    sd = {k: torch.full(ast.literal_eval(s), 0.5) for k, s in want.items()}
    missing, unexpected = model.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    assert model.sem_seg_head.logits_ld == 64 and model.sem_seg_head.common_stride == 4
    assert (model.combine_overlap_threshold, model.combine_stuff_area_limit, model.combine_instances_confidence_threshold) == (0.5, 4096.0, 0.5)


def test_the_head_starts_from_the_references_initialisation():
    from lvc_amd.modeling import build_model

    head = build_model(_cfg()).sem_seg_head      # (a fresh one: the module's model holds the loaded constants)
    for name, p in head.named_parameters():
        if name.endswith(".norm.weight"):
            assert bool((p == 1).all())
        elif name.endswith("bias"):
            assert bool((p == 0).all()), name
    w = head.p5[2].weight.detach()      # c2_msra_fill: normal, std sqrt(2 / fan_out)
    assert abs(float(w.std()) - (2.0 / (128 * 9)) ** 0.5) < 0.1 * (2.0 / (128 * 9)) ** 0.5
    assert head.p2[0].bias is None and [type(m).__name__ for m in head.p4] == ["Conv2d", "Upsample2", "Conv2d", "Upsample2"]


def test_semantic_segmentor_is_registered_and_holds_trunk_and_head_only():
    from lvc_amd.modeling import META_ARCH_REGISTRY, SEM_SEG_HEADS_REGISTRY, build_model

    assert SEM_SEG_HEADS_REGISTRY.get("SemSegFPNHead").__name__ == "SemSegFPNHead"
    assert META_ARCH_REGISTRY.get("PanopticFPN").__name__ == "PanopticFPN"
    cfg = _cfg()
    cfg.MODEL.META_ARCHITECTURE = "SemanticSegmentor"
    seg = build_model(cfg)
    assert all(k.startswith(("backbone.", "sem_seg_head.")) for k in seg.state_dict())
    assert not hasattr(seg, "roi_heads") and seg.keep_sem_seg_logits is True


def test_every_refusal_names_its_key(model):
    from lvc_amd.evaluation import GraphedInference, PipelinedInference, inference_on_dataset
    from lvc_amd.modeling import GeneralizedRCNNWithTTA, build_model

    cfg = _cfg()
    cfg.MODEL.SEM_SEG_HEAD.NORM = "BN"
    with pytest.raises(NotImplementedError, match="MODEL.SEM_SEG_HEAD.NORM"):
        build_model(cfg)
    cfg = _cfg()
    cfg.MODEL.SEM_SEG_HEAD.CONVS_DIM = 96
    with pytest.raises(NotImplementedError, match="MODEL.SEM_SEG_HEAD.CONVS_DIM"):
        build_model(cfg)
    cfg = _cfg()
    cfg.MODEL.SEM_SEG_HEAD.IN_FEATURES = ["p3", "p2"]
    with pytest.raises(NotImplementedError, match="MODEL.SEM_SEG_HEAD.IN_FEATURES"):
        build_model(cfg)
    cfg = _cfg()
    cfg.MODEL.MASK_ON = False
    with pytest.raises(NotImplementedError, match="MODEL.MASK_ON"):
        build_model(cfg)
    cfg = _cfg()
    cfg.MODEL.SEM_SEG_HEAD.NORM = ""
    plain = build_model(cfg)
    assert plain.sem_seg_head.p2[0].norm is None and plain.sem_seg_head.p2[0].bias is not None
    model.train()
    try:
        with pytest.raises(NotImplementedError, match=r"training the semantic branch \(loss_sem_seg\) is not built"):
            model([{"image": torch.zeros(3, 32, 32)}])
    finally:
        model.eval()
    for make in (lambda: PipelinedInference(model), lambda: GraphedInference(model, [{"image": torch.zeros(3, 32, 32)}]),
                 lambda: inference_on_dataset(model, []), lambda: GeneralizedRCNNWithTTA(_cfg(), model)):
        with pytest.raises(NotImplementedError, match="MODEL.META_ARCHITECTURE = PanopticFPN"):
            make()
    seg_cfg = _cfg()
    seg_cfg.MODEL.META_ARCHITECTURE = "SemanticSegmentor"
    seg = build_model(seg_cfg)
    with pytest.raises(NotImplementedError, match="MODEL.META_ARCHITECTURE = SemanticSegmentor"):
        PipelinedInference(seg)
    seg.train()
    with pytest.raises(NotImplementedError, match="loss_sem_seg"):
        seg([{"image": torch.zeros(3, 32, 32)}])


def test_box_only_and_mask_models_are_the_parents():
    from lvc_amd.config.presets import base_rcnn_fpn, mask_rcnn_fpn
    from lvc_amd.modeling import build_model

    for preset, keys in ((base_rcnn_fpn, "r50_fpn_state_dict_keys"), (mask_rcnn_fpn, "mask_rcnn_r50_fpn_keys")):
        m = build_model(preset(device="cpu"))
        g = gold(keys)
        got = {k: str(tuple(v.shape)) for k, v in m.state_dict().items()}
        assert got == dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
        assert type(m).__name__ == "GeneralizedRCNN" and not hasattr(m, "sem_seg_head")
        assert "sem_seg" not in repr(m).lower() and "upsample2" not in repr(m).lower()


def test_the_padded_predictor_takes_an_mfma_route():
    from lvc_amd import kernels as K

    def route(k):
        pc = types.SimpleNamespace(R=1, S=1, C=128, K=k, stride=1, pad=0, mode=0, two_acc=True, state={"tier": 0})
        return K.conv_route(pc, 8, 200, 336)

    assert route(54).entry == "lvc_conv2d_nhwc_f32"      # 54 % 4 != 0: the generic fp32 entry
    padded = route(64)
    assert padded.entry != "lvc_conv2d_nhwc_f32" and padded.engine != "f32", padded
    print("predictor 128 -> 64 at 8 x 200 x 336:", padded)


def test_the_table_builders_lay_out_what_the_header_states():
    from lvc_amd import kernels as K

    jobs, soft, labels = K.sem_seg_jobs([(32, 44), (9, 13)], [(125, 173), (33, 50)], [(97, 131), (66, 100)], 54, 64)
    assert jobs.shape == (2, K.SEG_POST_FIELDS) and jobs.dtype == np.int64
    assert jobs[1].tolist() == [32 * 44 * 64, 9, 13, 33, 50, 66, 100, 54 * 97 * 131, 97 * 131]
    assert (soft, labels) == (54 * (97 * 131 + 66 * 100), 97 * 131 + 66 * 100)
    rows = np.array([[1, 1, 7, 3, np.float32(0.75).view(np.int32), 40, 0, 0], [2, 0, 11, -1, 0, 500, 0, 0]], dtype=np.int32)
    assert K.segments_info(rows) == [{"id": 1, "isthing": True, "score": 0.75, "category_id": 7, "instance_id": 3},
                                     {"id": 2, "isthing": False, "category_id": 11, "area": 500}]
    text = open(__import__("os").path.join(__import__("helpers").ROOT, "include", "lvc_amd_seg.h")).read()
    for name, value in (("LVCSEG_POST_FIELDS", K.SEG_POST_FIELDS), ("LVCSEG_COMBINE_FIELDS", K.SEG_COMBINE_FIELDS),
                        ("LVCSEG_SEGMENT_FIELDS", K.SEG_SEGMENT_FIELDS)):
        assert "#define {} {}\n".format(name, value) in text
