"""ResNeXt trunks (RESNETS.NUM_GROUPS / WIDTH_PER_GROUP) on the host: the model builds, its state_dict is the reference's (tests/golden/
resnext_x50_fpn_keys.npz, scripts/make_golden_resnext.py), what is not built says so under its config key.  No kernel is launched."""
import pytest
import torch

from helpers import gold


def _cfg(depth=50, groups=32, width=4, **kw):
    from lvc_amd.config.presets import resnext_rcnn_fpn

    return resnext_rcnn_fpn(depth=depth, num_groups=groups, width_per_group=width, device="cpu", **kw)


@pytest.fixture(scope="module")
def x50():
    from lvc_amd.modeling import build_model

    return build_model(_cfg())


def test_x50_builds_with_the_reference_state_dict(x50):
    g = gold("resnext_x50_fpn_keys")
    want = dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
    got = {k: str(tuple(v.shape)) for k, v in x50.state_dict().items()}
    assert got == want
    assert list(got) == list(want)
    c2 = x50.backbone.bottom_up.res2[0].conv2
    assert c2.groups == 32 and tuple(c2.weight.shape) == (128, 4, 3, 3) and c2.stride == 1
    assert x50.backbone.bottom_up.res3[0].conv2.stride == 2 and x50.backbone.bottom_up.res3[0].conv1.stride == 1      # STRIDE_IN_1X1 False


def test_reference_shaped_state_dict_loads_strictly(x50):
    g = gold("resnext_x50_fpn_keys")
    sd = {k: torch.full(eval(s), 0.5) for k, s in zip(g["keys"].tolist(), g["shapes"].tolist())}
    missing, unexpected = x50.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    assert float(x50.backbone.bottom_up.res5[2].conv2.weight.detach().mean()) == 0.5


def test_conv2d_groups_weight_shape_and_refusals():
    from lvc_amd.layers import Conv2d

    conv = Conv2d(256, 256, kernel_size=3, padding=1, groups=32)
    assert tuple(conv.weight.shape) == (256, 8, 3, 3) and "groups=32" in repr(conv)
    assert tuple(Conv2d(256, 256, kernel_size=3, padding=1).weight.shape) == (256, 256, 3, 3)
    for kw in (dict(kernel_size=1), dict(kernel_size=7, padding=3), dict(kernel_size=3, padding=0), dict(kernel_size=3, padding=1, stride=3)):
        with pytest.raises(NotImplementedError, match="grouped"):
            Conv2d(256, 256, groups=32, **kw)
    with pytest.raises(NotImplementedError):
        Conv2d(256, 256, kernel_size=3, padding=1, groups=32, dilation=2)
    with pytest.raises(NotImplementedError, match="NUM_GROUPS"):
        Conv2d(96, 96, kernel_size=3, padding=1, groups=32)


@pytest.mark.parametrize("groups,width", [(32, 4), (32, 8), (64, 4)])
@pytest.mark.parametrize("stride_in_1x1", (False, True))
def test_trunk_widths_build(groups, width, stride_in_1x1):
    from lvc_amd.layers import ShapeSpec
    from lvc_amd.modeling.backbone.resnet import build_resnet_backbone

    cfg = _cfg(50, groups, width)
    cfg.MODEL.RESNETS.STRIDE_IN_1X1 = stride_in_1x1
    net = build_resnet_backbone(cfg, ShapeSpec(channels=3))
    for i, stage in enumerate((net.res2, net.res3, net.res4, net.res5)):
        for j, blk in enumerate(stage):
            w = groups * width * 2 ** i
            assert blk.conv2.groups == groups and tuple(blk.conv2.weight.shape) == (w, w // groups, 3, 3)
            assert blk.conv2.stride == (2 if (i > 0 and j == 0 and not stride_in_1x1) else 1)
            assert not blk.fused_eligible()      # the one-launch block bakes in a dense conv2


def test_unsupported_settings_name_their_key():
    from lvc_amd.modeling import build_model

    cfg = _cfg(50, 32, 3)
    with pytest.raises(NotImplementedError, match="NUM_GROUPS.*WIDTH_PER_GROUP"):
        build_model(cfg)
    cfg = _cfg()
    cfg.MODEL.RESNETS.RES5_DILATION = 2
    with pytest.raises(NotImplementedError, match="RES5_DILATION"):
        build_model(cfg)


def test_preset_keys_and_the_r50_tree_is_unchanged():
    from lvc_amd.config.presets import base_rcnn_fpn, resnext_rcnn_fpn
    from lvc_amd.modeling import build_model

    R = resnext_rcnn_fpn().MODEL.RESNETS
    assert (R.DEPTH, R.NUM_GROUPS, R.WIDTH_PER_GROUP, R.STRIDE_IN_1X1) == (101, 32, 8, False)
    model = build_model(base_rcnn_fpn(device="cpu"))
    g = gold("r50_fpn_state_dict_keys")
    assert {k: str(tuple(v.shape)) for k, v in model.state_dict().items()} == dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
    assert all(getattr(m, "groups", 1) == 1 for m in model.modules())
    assert "groups" not in repr(model)


def test_grouped_layers_route_to_the_grouped_kernel_only():
    import types

    from lvc_amd import kernels as K

    for tier in (0, 1, 2):
        pc = types.SimpleNamespace(R=3, S=3, C=256, K=256, stride=1, pad=1, mode=0, two_acc=False, state={"tier": tier}, groups=32)
        assert K.conv_route(pc, 8, 200, 336) == K.ConvRoute("f32_grouped", "lvc_conv3x3_grouped_nhwc", False, False)
    dense = types.SimpleNamespace(R=3, S=3, C=256, K=256, stride=1, pad=1, mode=0, two_acc=False, state={"tier": 0})
    assert K.conv_route(dense, 8, 200, 336).entry != "lvc_conv3x3_grouped_nhwc"
    assert "lvc_conv3x3_grouped_nhwc" in K._CONV_ARGS
