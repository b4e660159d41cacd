"""The grouped 3x3 convolution of the ResNeXt trunk on the device (csrc/conv_grouped.hip, `Conv2d(groups=)`, RESNETS.NUM_GROUPS).

Kernel tests: the oracle is F.conv2d(..., groups=G) on the CPU in float64.  The bar of every comparison is measured, not set (the
GroupNorm tests' rule): 3 x max |torch CPU fp32 - fp64| over the tensor, on the same inputs.  Every (ours, noise, bar, ratio) row is
written to profiles/grouped_conv_parity.json (LVC_GROUPED_PARITY_OUT: another path).

Model tests: the reference's own ResNeXt modules on the CPU (tests/golden/resnext_*.npz; scripts/make_golden_resnext.py)."""
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

from helpers import ROOT, gold

pytestmark = pytest.mark.gpu

K_NOISE = 3.0
_PARITY = {}

WIDTHS = ((32, 4), (32, 8), (32, 16), (32, 32), (32, 64), (64, 4))      # (groups, channels per group)
MAPS = ((1, 1, 1), (2, 5, 3), (2, 13, 17), (1, 33, 70))      # smaller than a tile; odd; ragged last tile both ways; several workgroups
OPTIONS = ("plain", "affine", "affine_relu", "affine_res_relu")


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    yield
    if not _PARITY:
        return
    path = os.environ.get("LVC_GROUPED_PARITY_OUT") or os.path.join(ROOT, "profiles", "grouped_conv_parity.json")
    try:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.update(_PARITY)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def _dev():
    return torch.device("cuda:0")


def _record(key, ours, noise):
    bar = K_NOISE * noise
    _PARITY[key] = {"ours": ours, "noise": noise, "bar": bar, "ratio": ours / bar if bar > 0 else (0.0 if ours == 0 else float("inf"))}
    print("%-64s ours %.3e  noise %.3e  bar %.3e" % (key, ours, noise, bar))
    return bar


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _case(G, cg, shape, stride):
    """Seeded inputs and the CPU convolution in float32 and float64 (computed once, never modified).  NHWC tensors."""
    N, H, W = shape
    C = G * cg
    g = torch.Generator().manual_seed(10000 * cg + 100 * G + 10 * H + stride)
    x = torch.randn(N, H, W, C, generator=g)
    w = torch.randn(C, cg, 3, 3, generator=g) / (9 * cg) ** 0.5
    scale = 1.0 + 0.3 * torch.randn(C, generator=g)
    shift = 0.2 * torch.randn(C, generator=g)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = torch.randn(N, Ho, Wo, C, generator=g)
    y32 = _nhwc(F.conv2d(_nchw(x), w, None, stride, 1, 1, G))
    y64 = _nhwc(F.conv2d(_nchw(x.double()), w.double(), None, stride, 1, 1, G))
    assert y64.shape == (N, Ho, Wo, C)
    return {"x": x, "w": w, "scale": scale, "shift": shift, "res": res, "y32": y32, "y64": y64}


def _epilogue(y, c, option):
    dt = y.dtype
    if option != "plain":
        y = y * c["scale"].to(dt) + c["shift"].to(dt)
    if option == "affine_res_relu":
        y = y + c["res"].to(dt)
    if option.endswith("relu"):
        y = F.relu(y)
    return y


@pytest.mark.parametrize("shape", MAPS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("G,cg", WIDTHS)
def test_kernel_parity(G, cg, shape):
    from lvc_amd import kernels as K

    dev = _dev()
    for stride in (1, 2):
        c = _case(G, cg, shape, stride)
        x = c["x"].to(dev)
        for option in OPTIONS:
            affine = (None, None) if option == "plain" else (c["scale"].to(dev), c["shift"].to(dev))
            pc = K.pack_conv(c["w"].to(dev), stride=stride, pad=1, affine=affine, groups=G)
            assert K.conv_route(pc, *shape).entry == "lvc_conv3x3_grouped_nhwc"
            res = c["res"].to(dev) if option == "affine_res_relu" else None
            y = K.conv2d_nhwc(x, pc, relu=option.endswith("relu"), residual=res, res_mode=1 if res is not None else 0).cpu()
            ref64 = _epilogue(c["y64"], c, option)
            noise = float((_epilogue(c["y32"], c, option).double() - ref64).abs().max())
            ours = float((y.double() - ref64).abs().max())
            bar = _record("fwd G%d cg%d %s s%d %s" % (G, cg, "x".join(map(str, shape)), stride, option), ours, noise)
            assert y.shape == ref64.shape and ours <= bar, (option, stride, ours, bar)


@functools.lru_cache(maxsize=None)
def _grad_case(cg, stride):
    G, (N, H, W) = 32, (2, 13, 17)
    c = _case(G, cg, (N, H, W), stride)
    g = torch.Generator().manual_seed(77 + cg + stride)
    bias = 0.2 * torch.randn(G * cg, generator=g)
    dy = torch.randn(c["y64"].shape, generator=g)
    # no gradient is fed where the fp64 pre-activation is within 1e-3 of the ReLU's kink: a mask flipped there by an fp32 evaluation
    # (torch's or ours) moves dx by a whole dy (the GroupNorm tests' guard)
    pre64 = c["y64"] + bias.double()
    dy = torch.where(pre64.abs() < 1e-3, torch.zeros_like(dy), dy)
    out = {"bias": bias, "dy": dy}
    for dt in (torch.float32, torch.float64):
        x = c["x"].detach().clone().to(dt).requires_grad_(True)      # (copies: the cached case is never modified)
        w = c["w"].detach().clone().to(dt).requires_grad_(True)
        b = bias.detach().clone().to(dt).requires_grad_(True)
        y = F.relu(_nhwc(F.conv2d(_nchw(x), w, b, stride, 1, 1, G)))
        (y * dy.to(dt)).sum().backward()
        out[dt] = {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": b.grad}
    return c, out


def _conv_module(c, cg, stride, bias, dev):
    from lvc_amd.layers import Conv2d

    C = 32 * cg
    conv = Conv2d(C, C, kernel_size=3, stride=stride, padding=1, bias=True, activation=F.relu_, groups=32).to(dev)
    with torch.no_grad():
        conv.weight.copy_(c["w"])
        conv.bias.copy_(bias)
    assert tuple(conv.weight.shape) == (C, cg, 3, 3)
    return conv


def _backward(conv, c, dy, dev):
    x = c["x"].detach().to(dev).requires_grad_(True)
    conv.weight.grad = conv.bias.grad = None
    y = conv.forward_nhwc(x)
    (y * dy.to(dev)).sum().backward()
    return y.detach().cpu(), x.grad.cpu(), conv.weight.grad.cpu().clone(), conv.bias.grad.cpu().clone()


@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("cg", (4, 16, 64))
def test_gradients_under_autograd(cg, stride):
    c, r = _grad_case(cg, stride)
    dev = _dev()
    conv = _conv_module(c, cg, stride, r["bias"], dev)
    y, dx, dw, db = _backward(conv, c, r["dy"], dev)
    r32, r64 = r[torch.float32], r[torch.float64]
    for name, got in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
        noise = float((r32[name].double() - r64[name]).abs().max())
        ours = float((got.double() - r64[name]).abs().max())
        bar = _record("bwd cg%d s%d %s" % (cg, stride, name), ours, noise)
        assert got.shape == r64[name].shape and ours <= bar, (name, ours, bar)


@pytest.mark.parametrize("stride", (1, 2))
def test_forward_dx_dw_are_bit_identical_across_calls(stride):
    c, r = _grad_case(16, stride)
    dev = _dev()
    conv = _conv_module(c, 16, stride, r["bias"], dev)
    a = _backward(conv, c, r["dy"], dev)
    b = _backward(conv, c, r["dy"], dev)
    for name, u, v in zip(("y", "dx", "dw", "db"), a, b):
        if name != "db":      # (the bias gradient is the dense layers' column sum, which uses atomics)
            assert torch.equal(u, v), name


def test_large_activations_stay_exact():
    """A planted 5000 and a planted 1e5 in one group: beyond the one- and two-accumulator ranges of the fp16-split kernels.  The grouped
    kernel multiplies fp32 operands, so nothing is raised and nothing re-routed; the output meets the bar, and so does the next call."""
    from lvc_amd import kernels as K
    from lvc_amd.layers import Conv2d
    from lvc_amd.modeling.roi_heads.roi_heads import run_with_fallbacks

    dev = _dev()
    G, cg, (N, H, W) = 32, 8, (2, 13, 17)
    c = _case(G, cg, (N, H, W), 1)
    conv = Conv2d(G * cg, G * cg, kernel_size=3, padding=1, bias=False, groups=G).to(dev)
    with torch.no_grad():
        conv.weight.copy_(c["w"])
    K.clear_conv_error_word(dev)

    def run(x):
        def once():
            y = conv.forward_nhwc(x.to(dev))
            K.check_conv_error_word(dev)
            return y
        with torch.no_grad():
            return run_with_fallbacks(conv, once).cpu()

    xb = c["x"].clone()
    xb[0, 6, 8, 3 * cg + 1] = 5000.0
    xb[1, 2, 3, 3 * cg + 5] = 1e5
    for tag, x in (("planted", xb), ("ordinary", c["x"])):
        y64 = _nhwc(F.conv2d(_nchw(x.double()), c["w"].double(), None, 1, 1, 1, G))
        y32 = _nhwc(F.conv2d(_nchw(x), c["w"], None, 1, 1, 1, G))
        noise = float((y32.double() - y64).abs().max())
        ours = float((run(x).double() - y64).abs().max())
        bar = _record("range %s" % tag, ours, noise)
        assert ours <= bar, (tag, ours, bar, float(y64.abs().max()))
    assert conv._range_state["tier"] == 0


def _block(groups, dev, cin=256, width=128, cout=256, stride=1, stride_in_1x1=False):
    from lvc_amd.modeling.backbone.resnet import BottleneckBlock

    torch.manual_seed(5)
    blk = BottleneckBlock(cin, cout, bottleneck_channels=width, stride=stride, num_groups=groups, norm="FrozenBN",
                          stride_in_1x1=stride_in_1x1)
    return blk.to(dev).eval()


def test_grouped_block_declines_the_dense_conv2_paths(monkeypatch):
    from lvc_amd import kernels as K

    dev = _dev()
    N, H, W = 8, 200, 336      # the trunk's res2 map: large enough for the Winograd and the fused-block routes of a dense layer
    # res2's own shape (64 mid channels): the dense block is one fused launch, the 64x1d grouped one is not
    dense, grouped = _block(1, dev, 256, 64, 256), _block(64 // 4, dev, 256, 64, 256)
    with torch.no_grad():
        assert dense.fused_eligible() and dense.fused() is not None
        assert not grouped.fused_eligible() and grouped.fused() is None
    wide_d, wide_g = _block(1, dev), _block(32, dev)
    rd = K.conv_route(wide_d.conv2.packed(), N, H, W)
    rg = K.conv_route(wide_g.conv2.packed(), N, H, W)
    assert rd.entry in ("lvc_conv3x3_nhwc_wino", "lvc_conv3x3_nhwc_f16s1") and rd.slotted      # a dense layer's routes, as before
    assert rg == K.ConvRoute("f32_grouped", "lvc_conv3x3_grouped_nhwc", False, False)
    assert wide_g.conv2.packed().groups == 32 and wide_d.conv2.packed().groups == 1
    assert wide_g.conv2.packed().w.dim() == 1 and wide_d.conv2.packed().w.dim() == 2      # the packed operand's type
    monkeypatch.setattr(K, "PRESPLIT", True)
    x = torch.empty(N, 50, 84, 128, device=dev)
    assert not K.presplit_pair_ok(x, wide_g.conv2.packed(), wide_g.conv3.packed())
    # the pointwise layers of a grouped block route as the dense block's do
    for name in ("conv1", "conv3"):
        assert K.conv_route(getattr(wide_g, name).packed(), N, H, W) == K.conv_route(getattr(wide_d, name).packed(), N, H, W)


def test_batch_of_one_and_empty_batch():
    from lvc_amd import kernels as K

    dev = _dev()
    c = _case(32, 8, (1, 1, 1), 1)
    pc = K.pack_conv(c["w"].to(dev), stride=1, pad=1, groups=32)
    y = K.conv2d_nhwc(c["x"].to(dev), pc).cpu()
    assert float((y.double() - c["y64"]).abs().max()) <= K_NOISE * max(float((c["y32"].double() - c["y64"]).abs().max()), 1e-7)
    empty = K.conv2d_nhwc(torch.empty(0, 5, 3, 256, device=dev), pc)      # no launch: an empty result
    assert tuple(empty.shape) == (0, 5, 3, 256)
    dw = K.conv_wgrad_grouped(torch.empty(0, 5, 3, 256, device=dev), torch.empty(0, 5, 3, 256, device=dev), None, 32, 1)
    assert tuple(dw.shape) == (256, 8, 3, 3) and float(dw.abs().max()) == 0.0
    with pytest.raises(NotImplementedError, match="NUM_GROUPS"):
        K.pack_conv(torch.zeros(96, 3, 3, 3, device=dev), stride=1, pad=1, groups=32)


# ----------------------------------------------------------------------------------------------------------------- reference fixtures
@pytest.mark.parametrize("name,cin,width,cout,stride,seed", [("resnext_block_identity", 256, 128, 256, 1, 61),
                                                             ("resnext_block_proj", 256, 256, 512, 2, 62)])
def test_reference_block(name, cin, width, cout, stride, seed):
    """The reference's BottleneckBlock(num_groups=32) with seeded weights and non-trivial FrozenBN buffers (the generator's recipe)."""
    from lvc_amd.utils import synthetic as syn

    g = gold(name)
    dev = _dev()
    blk = _block(32, torch.device("cpu"), cin, width, cout, stride, stride_in_1x1=False)
    blk.load_state_dict(syn.seeded_module_state_dict(blk.state_dict(), seed=seed), strict=True)
    blk = blk.to(dev).eval()
    x = torch.randn(2, 256, 9, 11, generator=torch.Generator().manual_seed(seed)).relu_()
    with torch.no_grad():
        y = blk(x.to(dev)).cpu()
    noise = float((g["out32"].double() - g["out64"]).abs().max())
    ours = float((y.double() - g["out64"]).abs().max())
    bar = _record("block %s" % name, ours, noise)
    assert y.shape == g["out64"].shape and ours <= bar, (ours, bar)


def _x50_model(train=False):
    from lvc_amd.config.presets import resnext_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    cfg = resnext_rcnn_fpn(depth=50, num_groups=32, width_per_group=4, num_classes=60 if train else 80)
    model = build_model(cfg)
    model.load_state_dict(syn.conditioned_resnext_state_dict(model.state_dict(), seed=0), strict=True)
    return model.train() if train else model.eval()


_X50_SIZES = ((128, 160, 3), (120, 176, 4))
_X50_SAMPLE = {"p2": (16, 2), "p3": (8, 1), "p4": (8, 1), "p5": (8, 1), "p6": (8, 1)}      # the fixture's [:, ::channels, ::rows, ::columns]


def _x50_inputs():
    from lvc_amd.utils import synthetic as syn

    return [{"image": syn.synthetic_image(seed, h, w), "height": h, "width": w} for h, w, seed in _X50_SIZES]


@pytest.mark.parametrize("grad", (False, True), ids=("eval", "autograd"))
def test_reference_x50_pyramid(grad):
    g = gold("resnext_x50_fpn_small")
    model = _x50_model()
    if grad:
        for p in model.backbone.parameters():
            p.requires_grad_(True)
    with torch.set_grad_enabled(grad):
        x = model.preprocess_image(_x50_inputs()).tensor
        feats = model.backbone(x)
    for k in ("p2", "p3", "p4", "p5", "p6"):
        cs, ss = _X50_SAMPLE[k]
        got = feats[k].detach()[:, ::cs, ::ss, ::ss].cpu()
        noise = float((g["feat32_" + k].double() - g["feat64_" + k]).abs().max())
        ours = float((got.double() - g["feat64_" + k]).abs().max())
        bar = _record("x50 %s %s" % (k, "autograd" if grad else "eval"), ours, noise)
        assert got.shape == g["feat64_" + k].shape and ours <= bar, (k, ours, bar)


def test_reference_x50_training_step(monkeypatch):
    """One step of the X-50-32x4d-FPN detector with FREEZE_AT 2 (res3..res5 train through the grouped dgrad / wgrad) against the
    reference's CPU step (tests/golden/resnext_train.npz), held to the bars of test_gpu_train.py's base-detector step."""
    from lvc_amd.structures import Boxes, Instances
    from lvc_amd.utils import synthetic as syn
    from lvc_amd.utils.events import EventStorage

    g = gold("resnext_train")
    model = _x50_model(train=True)
    assert [n for n, p in model.named_parameters() if not p.requires_grad] == g["frozen_names"].tolist()
    batch = []
    for i, (h, w, seed) in enumerate(_X50_SIZES):
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(g["gt_boxes%d" % i])
        inst.gt_classes = g["gt_classes%d" % i]
        batch.append({"image": syn.synthetic_image(seed, h, w), "instances": inst, "height": h, "width": w})
    monkeypatch.setattr(torch, "randperm", lambda n, **kw: torch.arange(n, **{k: v for k, v in kw.items() if k in ("device", "dtype")}))
    with EventStorage(0):
        losses = model(batch)
        sum(losses.values()).backward()
    for k in ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"):
        ref, got = float(g["loss." + k]), float(losses[k].detach())
        print(k, got, ref)
        assert abs(got - ref) <= 2e-4 * max(1.0, abs(ref)), k
    bad = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, name
            continue
        assert p.grad is not None, name
        gflat = p.grad.flatten().cpu()
        s, nrm, stride = [float(v) for v in g["grad_stats." + name]]
        sample = gflat[:: int(stride)][:2048].double()
        ref = g["grad_sample." + name].double()
        if nrm == 0.0:
            assert float(gflat.abs().max()) == 0.0, name
            continue
        cos = float((sample * ref).sum() / (sample.norm() * ref.norm()).clamp_min(1e-30))
        nerr = abs(float(gflat.double().norm()) - nrm) / max(nrm, 1e-12)
        print("%-52s cos %.6f  norm err %.2e" % (name, cos, nerr))
        if not (cos >= 0.998 and nerr <= 1e-2):
            bad[name] = (cos, nerr)
    assert not bad, bad
