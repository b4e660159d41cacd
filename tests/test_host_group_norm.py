"""GroupNorm (NORM: "GN") without a GPU: what `get_norm` builds, the state_dict contract of the GN variant of R50-FPN (pyramid +
4conv1fc head; tests/golden/gn_state_dict_keys.npz from the reference, scripts/make_golden_gn.py), the solver's norm group, the
trunk's refusal, and the C ABI of csrc/group_norm.hip."""
import os
import re

import pytest
import torch

from helpers import ROOT, gold


def _gn_model(**over):
    from lvc_amd.config.presets import gn_rcnn_fpn
    from lvc_amd.modeling import build_model

    cfg = gn_rcnn_fpn(device="cpu")
    for k, v in over.items():
        node = cfg
        parts = k.split(".")
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = v
    return cfg, build_model(cfg)


def test_get_norm_gn_and_the_norms_that_stay_unimplemented():
    from lvc_amd.layers import GroupNorm, get_norm

    m = get_norm("GN", 256)
    assert isinstance(m, torch.nn.GroupNorm) and isinstance(m, GroupNorm)
    assert m.num_groups == 32 and m.num_channels == 256 and m.eps == 1e-5
    assert sorted(k for k, _ in m.named_parameters()) == ["bias", "weight"]
    assert get_norm("", 8) is None
    for name in ("BN", "SyncBN", "nnSyncBN", "naiveSyncBN"):
        with pytest.raises(NotImplementedError, match=name):
            get_norm(name, 8)


def test_gn_model_state_dict_matches_reference_and_loads_strictly():
    _, model = _gn_model()
    g = gold("gn_state_dict_keys")
    mine = {k: str(tuple(v.shape)) for k, v in model.state_dict().items()}
    assert list(mine) == g["keys"].tolist()
    assert list(mine.values()) == g["shapes"].tolist()
    sd = {k: torch.full(eval(s), 0.5) for k, s in zip(g["keys"].tolist(), g["shapes"].tolist())}
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert float(model.backbone.fpn_output3.norm.bias.detach()[7]) == 0.5 and float(model.roi_heads.box_head.conv4.norm.weight.detach()[0]) == 0.5
    # GN drops the conv bias (reference fpn.py:70-74, box_head.py:30-35)
    assert model.backbone.fpn_lateral2.bias is None and model.roi_heads.box_head.conv1.bias is None
    assert len(model.roi_heads.box_head.conv_norm_relus) == 4 and len(model.roi_heads.box_head.fcs) == 1


def test_gn_parameters_decay_by_weight_decay_norm():
    from lvc_amd import solver

    cfg, model = _gn_model()
    cfg.SOLVER.WEIGHT_DECAY = 1e-4
    cfg.SOLVER.WEIGHT_DECAY_NORM = 0.25
    gn = {id(p) for m in model.modules() if isinstance(m, torch.nn.GroupNorm) for p in m.parameters()}
    assert len(gn) == 24
    seen = 0
    for grp in solver.parameter_groups(cfg, model):
        for p in grp["params"]:
            if id(p) in gn:
                seen += 1
                assert grp["weight_decay"] == 0.25
            else:
                assert grp["weight_decay"] != 0.25
    assert seen == 24


def test_gn_in_the_trunk_is_refused_with_the_key():
    with pytest.raises(NotImplementedError, match=r"RESNETS\.NORM"):
        _gn_model(**{"MODEL.RESNETS.NORM": "GN"})


def test_group_norm_abi_is_declared_and_exported():
    from lvc_amd import _lib

    txt = open(os.path.join(ROOT, "include", "lvc_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(lvc_[a-z0-9_]+)\s*\(", txt))
    L = _lib.lib()
    for s in ("lvc_group_norm_fwd_nhwc", "lvc_group_norm_bwd_nhwc", "lvc_group_norm_workspace_bytes", "lvc_upsample2_add_grad_nhwc"):
        assert s in declared, s
        assert hasattr(L, s), s
    # the workspace query is host arithmetic: none for whole samples in the forward, slabs for row tiles and for every backward
    q = L.lvc_group_norm_workspace_bytes
    assert q(2, 7, 7, 256, 32, 0, 0) == 0
    assert q(2, 64, 64, 256, 32, 16, 0) >= 2 * 4 * 32 * 2 * 4
    assert q(2, 7, 7, 256, 32, 0, 1) >= 2 * 2 * 256 * 4
    assert q(2, 64, 64, 256, 32, 16, 1) > q(2, 64, 64, 256, 32, 64, 1)


def test_group_norm_needs_the_device():
    from lvc_amd.layers import GroupNorm

    with pytest.raises(RuntimeError):
        GroupNorm(32, 64)(torch.zeros(1, 64, 4, 4))
