"""The ResNet-D trunk (RESNETS.D: DeepStem, BottleneckBlockCLIP) on the host: the model builds, its state_dict is the reference's (tests/golden/
resnet_d_r50_fpn_keys.npz, scripts/make_golden_resnet_d.py), what is not built says so under its config keys, and the D: False tree is
what it was.  No kernel is launched."""
import re
import types

import pytest
import torch

from helpers import gold


def _cfg(depth=50, **kw):
    from lvc_amd.config.presets import resnet_d_rcnn_fpn

    return resnet_d_rcnn_fpn(depth=depth, device="cpu", **kw)


@pytest.fixture(scope="module")
def r50d():
    from lvc_amd.modeling import build_model

    return build_model(_cfg())


def test_r50_d_builds_with_the_reference_state_dict(r50d):
    from lvc_amd.modeling.backbone.resnet import BottleneckBlockCLIP, DeepStem

    g = gold("resnet_d_r50_fpn_keys")
    want = dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
    got = {k: str(tuple(v.shape)) for k, v in r50d.state_dict().items()}
    assert got == want
    assert list(got) == list(want)
    trunk = r50d.backbone.bottom_up
    assert isinstance(trunk.stem, DeepStem) and trunk.stem.stride == 4
    assert [tuple(c.weight.shape) for c in (trunk.stem.conv1, trunk.stem.conv2, trunk.stem.conv3)] == [(32, 3, 3, 3), (32, 32, 3, 3), (64, 32, 3, 3)]
    assert (trunk.stem.conv1.stride, trunk.stem.conv2.stride, trunk.stem.conv3.stride) == (2, 1, 1)
    assert [len(s) for s in (trunk.res2, trunk.res3, trunk.res4, trunk.res5)] == [3, 4, 6, 3]
    for i, stage in enumerate((trunk.res2, trunk.res3, trunk.res4, trunk.res5)):
        for j, blk in enumerate(stage):
            assert isinstance(blk, BottleneckBlockCLIP)
            assert blk.stride == (2 if (i > 0 and j == 0) else 1)
            assert (blk.conv1.stride, blk.conv2.stride, blk.conv3.stride) == (1, 1, 1)      # the stride is the pools'
            assert (blk.shortcut is not None) == (j == 0) and (blk.shortcut is None or blk.shortcut.stride == 1)
    assert {k: v.stride for k, v in trunk.output_shape().items()} == {"res2": 4, "res3": 8, "res4": 16, "res5": 32}
    # FREEZE_AT 2: the stem and res2 do not train, res3.. do
    assert not any(p.requires_grad for p in trunk.stem.parameters()) and not any(p.requires_grad for p in trunk.res2.parameters())
    assert all(p.requires_grad for p in trunk.res3.parameters())


def test_reference_shaped_state_dict_loads_strictly(r50d):
    g = gold("resnet_d_r50_fpn_keys")
    sd = {k: torch.full(eval(s), 0.5) for k, s in zip(g["keys"].tolist(), g["shapes"].tolist())}
    missing, unexpected = r50d.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    assert float(r50d.backbone.bottom_up.stem.conv2.weight.detach().mean()) == 0.5
    assert float(r50d.backbone.bottom_up.res5[0].shortcut.weight.detach().mean()) == 0.5


def test_stride_in_1x1_is_ignored_and_depths_build():
    from lvc_amd.layers import ShapeSpec
    from lvc_amd.modeling.backbone.resnet import build_resnet_backbone

    for flag in (True, False):
        cfg = _cfg()
        cfg.MODEL.RESNETS.STRIDE_IN_1X1 = flag
        net = build_resnet_backbone(cfg, ShapeSpec(channels=3))
        assert all(b.conv1.stride == 1 and b.conv2.stride == 1 for s in (net.res2, net.res3, net.res4, net.res5) for b in s)
    net = build_resnet_backbone(_cfg(depth=101), ShapeSpec(channels=3))
    assert len(net.res4) == 23


def test_refused_combinations_name_their_keys():
    from lvc_amd.modeling import build_model

    cfg = _cfg()
    cfg.MODEL.RESNETS.NUM_GROUPS = 32
    cfg.MODEL.RESNETS.WIDTH_PER_GROUP = 4
    with pytest.raises(NotImplementedError, match=r"RESNETS\.D.*NUM_GROUPS"):
        build_model(cfg)
    for depth in (18, 34):
        cfg = _cfg()
        cfg.MODEL.RESNETS.DEPTH = depth
        cfg.MODEL.RESNETS.RES2_OUT_CHANNELS = 64
        with pytest.raises(NotImplementedError, match=r"RESNETS\.D.*DEPTH = %d" % depth):
            build_model(cfg)
    cfg = _cfg()
    cfg.MODEL.RESNETS.RES5_DILATION = 2
    with pytest.raises(NotImplementedError, match=r"RESNETS\.D.*RES5_DILATION"):
        build_model(cfg)
    cfg = _cfg()
    cfg.MODEL.RESNETS.DROPOUT = 0.1      # (in the reference D wins over DROPOUT; here DROPOUT keeps raising)
    with pytest.raises(NotImplementedError, match=r"RESNETS\.DROPOUT"):
        build_model(cfg)
    cfg = _cfg()
    cfg.MODEL.RESNETS.NORM = "BN"
    with pytest.raises(NotImplementedError, match=r"RESNETS\.NORM"):
        build_model(cfg)


def test_block_and_stem_refusals():
    from lvc_amd.modeling.backbone.resnet import BottleneckBlockCLIP, DeepStem

    with pytest.raises(NotImplementedError, match="NUM_GROUPS"):
        BottleneckBlockCLIP(256, 256, bottleneck_channels=128, num_groups=32, norm="FrozenBN")
    with pytest.raises(NotImplementedError, match="RES5_DILATION"):
        BottleneckBlockCLIP(256, 256, bottleneck_channels=64, dilation=2, norm="FrozenBN")
    with pytest.raises(NotImplementedError, match="stride"):
        BottleneckBlockCLIP(256, 512, bottleneck_channels=128, stride=3, norm="FrozenBN")
    with pytest.raises(NotImplementedError, match="STEM_OUT_CHANNELS"):
        DeepStem(3, 48, "FrozenBN")


def test_d_false_tree_and_routes_are_unchanged(monkeypatch):
    from lvc_amd import kernels as K
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.modeling.backbone.resnet import BasicStem, BottleneckBlock

    cfg = base_rcnn_fpn(device="cpu")
    assert cfg.MODEL.RESNETS.D is False
    model = build_model(cfg)
    g = gold("r50_fpn_state_dict_keys")
    got = {k: str(tuple(v.shape)) for k, v in model.state_dict().items()}
    assert got == dict(zip(g["keys"].tolist(), g["shapes"].tolist())) and list(got) == g["keys"].tolist()
    trunk = model.backbone.bottom_up
    assert type(trunk.stem) is BasicStem and all(type(b) is BottleneckBlock for s in (trunk.res2, trunk.res3, trunk.res4, trunk.res5) for b in s)
    assert "AvgPool" not in repr(model) and "CLIP" not in repr(model)
    # conv_route's answers for the trunk's layer shapes at 8 x 800 x 1344 (pure: no tensor, no library call)
    def pc(R, C, Kc, stride=1, two_acc=False):
        return types.SimpleNamespace(R=R, S=R, C=C, K=Kc, stride=stride, pad=R // 2, mode=0, two_acc=two_acc, state={"tier": 0})

    want = {      # (recorded on the commit before RESNETS.D was built; `conv_route` is not touched by it)
        (1, 256, 64, 200, 336): "lvc_conv1x1_nhwc_f16s1",
        (3, 64, 64, 200, 336): "lvc_conv3x3_nhwc_f16s1",
        (1, 64, 256, 200, 336): "lvc_conv1x1_nhwc_f16x2_pipe",
        (3, 128, 128, 100, 168): "lvc_conv3x3_nhwc_wino",
        (1, 128, 512, 100, 168): "lvc_conv1x1_nhwc_f16x2_pipe",
        (3, 256, 256, 50, 84): "lvc_conv3x3_nhwc_f16s1",
        (1, 1024, 256, 50, 84): "lvc_conv1x1_nhwc_f16s1",
        (1, 512, 2048, 25, 42): "lvc_conv1x1_nhwc_f16s1",
    }
    # the table holds for the kernel switches' defaults: set them, so that an environment override cannot make this part vacuous
    for name, value in (("CONV_ENGINE", "bf16x3"), ("CONV_SPLIT", "f16x2"), ("HALO_S1", 2), ("PW_S1", 2), ("CONV_WINO", True), ("PW_W2", True)):
        monkeypatch.setattr(K, name, value)
    got = {k: K.conv_route(pc(k[0], k[1], k[2]), 8, k[3], k[4]).entry for k in want}
    assert got == want


def test_clip_blocks_decline_the_fused_paths():
    from lvc_amd.modeling.backbone.resnet import BottleneckBlock, BottleneckBlockCLIP, ResNet

    res2_0 = BottleneckBlockCLIP(64, 256, bottleneck_channels=64, stride=1, norm="FrozenBN").eval()
    ident = BottleneckBlockCLIP(256, 256, bottleneck_channels=64, stride=1, norm="FrozenBN").eval()
    proj = BottleneckBlockCLIP(256, 512, bottleneck_channels=128, stride=2, norm="FrozenBN").eval()
    dense = BottleneckBlock(256, 256, bottleneck_channels=64, stride=1, norm="FrozenBN").eval()
    with torch.no_grad():
        for blk in (res2_0, ident, proj):
            assert not isinstance(blk, BottleneckBlock)      # ResNet.forward_nhwc walks it with forward_nhwc, never forward_chained
            assert not blk.fused_eligible() and blk.fused() is None
            assert blk.chain_to(dense, False) is None and blk.chain_to(dense, True) is None
            assert not hasattr(blk, "forward_chained")
        # the one-GEMM conv3 + shortcut: stride-2 blocks, gradient-free passes only
        assert not res2_0.can_fuse_projection() and not ident.can_fuse_projection()
        assert res2_0.shortcut is not None and ident.shortcut is None
    import lvc_amd.modeling.backbone.resnet as R
    from lvc_amd import kernels as K

    assert R.FUSE_POOLED_PROJECTION is True
    if K.FUSE_PROJECTION and K.CONV_ENGINE == "bf16x3":
        with torch.no_grad():
            assert proj.can_fuse_projection()
        with torch.enable_grad():
            assert not proj.can_fuse_projection()      # trainable parameters under autograd: two pools, two convs, a residual add
            assert proj.freeze().can_fuse_projection()
    assert [n for n, _ in proj.named_children()] == ["shortcut", "conv1", "conv2", "conv3"]      # the pools own no parameters or buffers
    assert ResNet.forward_nhwc.__code__.co_names.count("forward_chained") == 1


def test_wrapper_value_errors():
    from lvc_amd import kernels as K

    for shape in ((1, 1, 8, 4), (1, 8, 1, 4)):
        with pytest.raises(ValueError, match="at least 2 x 2"):
            K.avgpool2_into(torch.zeros(shape))
    for c in (3, 6, 30):
        with pytest.raises(ValueError, match="multiples of 4"):
            K.avgpool2_into(torch.zeros(1, 4, 4, c))
    buf = torch.zeros(1, 2, 2, 38)
    with pytest.raises(ValueError, match="multiples of 4"):      # ldo = 38
        K.avgpool2_into(torch.zeros(1, 4, 4, 4), buf[..., :4])
    buf = torch.zeros(1, 2, 2, 40)
    with pytest.raises(ValueError, match="multiples of 4"):      # a slice that starts at channel 2
        K.avgpool2_into(torch.zeros(1, 4, 4, 4), buf[..., 2:6])
    with pytest.raises(ValueError, match="output"):
        K.avgpool2_into(torch.zeros(1, 4, 4, 4), torch.zeros(1, 2, 3, 4))
    with pytest.raises(ValueError, match="gradient"):
        K.avgpool2_backward(torch.zeros(1, 2, 2, 4), 7, 4)
    with pytest.raises(ValueError, match="multiples of 4"):
        K.avgpool2_backward(torch.zeros(1, 2, 2, 6), 4, 4)
    # well-formed arguments on the host: there is no CPU path
    with pytest.raises(RuntimeError, match="device tensors"):
        K.avgpool2_into(torch.zeros(1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="device tensors"):
        K.avgpool2_nhwc(torch.zeros(1, 5, 7, 8))


def test_header_declares_the_entries_and_the_library_exports_them():
    import os

    from helpers import ROOT
    from lvc_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvc_amd.h")).read(), flags=re.S)
    for name in ("lvc_avgpool2_nhwc", "lvc_avgpool2_bwd_nhwc"):
        assert "int %s(" % name in txt and hasattr(_lib.lib(), name)
