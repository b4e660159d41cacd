"""The ResNet-D trunk on the device (RESNETS.D: `DeepStem`, `BottleneckBlockCLIP`, presets.resnet_d_rcnn_fpn) against the reference's own
modules run on the CPU (tests/golden/resnet_d_*.npz; scripts/make_golden_resnet_d.py, whose seeds these tests repeat).

The bar of every comparison is measured, not set: 3 x the fixture's own max |out32 - out64| (the grouped-conv tests' rule); the training
step is held to the bars of test_gpu_train.py's base-detector step.  Rows go to profiles/avgpool_parity.json with the kernel's."""
import pytest
import torch
import torch.nn.functional as F

from avgpool_rows import dev as _dev, record as _record, write_parity  # noqa: F401  (the fixture writes this module's rows)
from helpers import gold

pytestmark = pytest.mark.gpu

STEM_SEED = 70
BLOCKS = {"res2_0": (64, 64, 256, 1, 71), "identity": (256, 64, 256, 1, 72), "proj": (256, 128, 512, 2, 73)}      # in, width, out, stride, seed
_SIZES = ((128, 160, 3), (120, 176, 4))
_SAMPLE = {"p2": (16, 2), "p3": (8, 1), "p4": (8, 1), "p5": (8, 1), "p6": (8, 1)}      # the fixture's [:, ::channels, ::rows, ::columns]


def _check(key, got, g):
    noise = float((g["out32"].double() - g["out64"]).abs().max())
    ours = float((got.double() - g["out64"]).abs().max())
    bar = _record(key, ours, noise)
    assert got.shape == g["out64"].shape and ours <= bar, (key, ours, bar)


def _block(name, dev):
    from lvc_amd.modeling.backbone.resnet import BottleneckBlockCLIP
    from lvc_amd.utils import synthetic as syn

    cin, width, cout, stride, seed = BLOCKS[name]
    blk = BottleneckBlockCLIP(cin, cout, bottleneck_channels=width, stride=stride, norm="FrozenBN")
    blk.load_state_dict(syn.seeded_module_state_dict(blk.state_dict(), seed=seed), strict=True)
    x = torch.randn(2, cin, 9, 11, generator=torch.Generator().manual_seed(seed)).relu_()
    return blk.to(dev).eval(), x


def test_reference_stem():
    from lvc_amd.modeling.backbone.resnet import DeepStem
    from lvc_amd.utils import synthetic as syn

    dev = _dev()
    stem = DeepStem(3, 64, "FrozenBN")
    stem.load_state_dict(syn.seeded_module_state_dict(stem.state_dict(), seed=STEM_SEED), strict=True)
    stem = stem.to(dev).eval()
    x = torch.randn(2, 3, 37, 53, generator=torch.Generator().manual_seed(STEM_SEED))
    with torch.no_grad():
        y = stem(x.to(dev)).cpu()
        again = stem(x.to(dev)).cpu()
    _check("stem", y, gold("resnet_d_stem"))
    assert torch.equal(y, again)
    # a trainable conv1 raises, as BasicStem's does (MODEL.BACKBONE.FREEZE_AT >= 1)
    with pytest.raises(NotImplementedError, match="stem"):
        stem(x.to(dev))


@pytest.mark.parametrize("name", ("res2_0", "identity", "proj"))
def test_reference_block(name):
    g = gold("resnet_d_block_" + name)
    blk, x = _block(name, _dev())
    with torch.no_grad():
        y = blk(x.to(_dev())).cpu()
        again = blk(x.to(_dev())).cpu()
    _check("block %s" % name, y, g)
    assert torch.equal(y, again)      # two identical forwards are bit-identical


@pytest.mark.parametrize("fuse", (True, False), ids=("one_gemm", "two_convs"))
def test_stride2_block_with_and_without_the_pooled_projection_gemm(fuse, monkeypatch):
    import lvc_amd.modeling.backbone.resnet as R
    from lvc_amd import kernels as K

    monkeypatch.setattr(R, "FUSE_POOLED_PROJECTION", fuse)
    blk, x = _block("proj", _dev())
    calls = []
    real = K.avgpool2_into
    monkeypatch.setattr(K, "avgpool2_into", lambda x_, out=None: (calls.append(None if out is None else out.stride(2)), real(x_, out))[1])
    with torch.no_grad():
        assert blk.can_fuse_projection() == (fuse and K.FUSE_PROJECTION and K.CONV_ENGINE == "bf16x3")
        y = blk(x.to(_dev())).cpu()
    _check("block proj %s" % ("one GEMM" if fuse else "two convs"), y, gold("resnet_d_block_proj"))
    # two pool launches either way: into the two slices of the [N,4,5,128 + 256] buffer, or into tensors of their own
    assert calls == ([384, 384] if (fuse and K.FUSE_PROJECTION and K.CONV_ENGINE == "bf16x3") else [None, None])


@pytest.mark.parametrize("name", ("identity", "proj"))
def test_block_under_autograd(name):
    """y and dx with trainable parameters: both pools, the three (four) convs and the residual add on the autograd path, against the
    reference block's own CPU autograd in float32 and float64 (the module is rebuilt in torch from the same seeded state_dict)."""
    cin, width, cout, stride, seed = BLOCKS[name]
    dev = _dev()
    blk, x = _block(name, dev)
    sd = {k: v.cpu() for k, v in blk.state_dict().items()}

    def torch_block(xx, dt):
        def cbn(t, p, pad=0):
            t = F.conv2d(t, sd[p + ".weight"].to(dt), None, 1, pad)
            return F.batch_norm(t, sd[p + ".norm.running_mean"].to(dt), sd[p + ".norm.running_var"].to(dt), sd[p + ".norm.weight"].to(dt),
                                sd[p + ".norm.bias"].to(dt), False, 0.0, 1e-5)
        pool = (lambda t: F.avg_pool2d(t, 2)) if stride == 2 else (lambda t: t)
        out = F.relu(cbn(xx, "conv1"))
        out = F.relu(cbn(out, "conv2", 1))
        out = cbn(pool(out), "conv3")
        sc = cbn(pool(xx), "shortcut") if "shortcut.weight" in sd else xx
        return out + sc

    with torch.no_grad():
        pre64 = torch_block(x.double(), torch.float64)
    dy = torch.randn(pre64.shape, generator=torch.Generator().manual_seed(seed + 100))
    # no gradient is fed where the fp64 pre-activation is within 1e-3 of the final ReLU's kink (the grouped-conv tests' guard)
    dy = torch.where(pre64.abs() < 1e-3, torch.zeros_like(dy), dy)
    out = {}
    for dt in (torch.float32, torch.float64):
        xx = x.clone().to(dt).requires_grad_(True)
        y = F.relu(torch_block(xx, dt))
        (y * dy.to(dt)).sum().backward()
        out[dt] = {"y": y.detach(), "dx": xx.grad}
    for p in blk.parameters():
        p.requires_grad_(True)
    xd = x.to(dev).requires_grad_(True)
    with torch.enable_grad():
        assert not blk.can_fuse_projection()
        y = blk(xd)
        (y * dy.to(dev)).sum().backward()
    assert all(p.grad is not None for p in blk.parameters())
    for key, got in (("y", y.detach().cpu()), ("dx", xd.grad.cpu())):
        noise = float((out[torch.float32][key].double() - out[torch.float64][key]).abs().max())
        ours = float((got.double() - out[torch.float64][key]).abs().max())
        bar = _record("autograd %s %s" % (name, key), ours, noise)
        assert got.shape == out[torch.float64][key].shape and ours <= bar, (key, ours, bar)


def _r50d_model(train=False):
    from lvc_amd.config.presets import resnet_d_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    model = build_model(resnet_d_rcnn_fpn(depth=50, num_classes=60 if train else 80))
    # (no FrozenBN calibration is stored for this trunk either: the ResNeXt recipe, conv3's norm scales its branch by 0.25)
    model.load_state_dict(syn.conditioned_resnext_state_dict(model.state_dict(), seed=0), strict=True)
    return model.train() if train else model.eval()


def _inputs():
    from lvc_amd.utils import synthetic as syn

    return [{"image": syn.synthetic_image(seed, h, w), "height": h, "width": w} for h, w, seed in _SIZES]


@pytest.mark.parametrize("grad", (False, True), ids=("eval", "autograd"))
def test_reference_r50_d_pyramid(grad):
    g = gold("resnet_d_r50_fpn_small")
    model = _r50d_model()
    if grad:
        for name, p in model.backbone.named_parameters():
            if ".stem.conv1." not in name:      # (a trainable stem conv1 raises)
                p.requires_grad_(True)
    with torch.set_grad_enabled(grad):
        x = model.preprocess_image(_inputs()).tensor
        feats = model.backbone(x)
        again = feats if grad else model.backbone(x)
    for k in ("p2", "p3", "p4", "p5", "p6"):
        cs, ss = _SAMPLE[k]
        got = feats[k].detach()[:, ::cs, ::ss, ::ss].cpu()
        noise = float((g["feat32_" + k].double() - g["feat64_" + k]).abs().max())
        ours = float((got.double() - g["feat64_" + k]).abs().max())
        bar = _record("r50-d %s %s" % (k, "autograd" if grad else "eval"), ours, noise)
        assert got.shape == g["feat64_" + k].shape and ours <= bar, (k, ours, bar)
        assert torch.equal(feats[k].detach(), again[k].detach()), k      # two identical forwards are bit-identical


def test_reference_r50_d_training_step(monkeypatch):
    """One step of the R50-D-FPN detector with FREEZE_AT 2 (res3..res5 train through both pools' backward) against the reference's CPU
    step (tests/golden/resnet_d_train.npz), held to the bars of test_gpu_train.py's base-detector step."""
    from lvc_amd.structures import Boxes, Instances
    from lvc_amd.utils import synthetic as syn
    from lvc_amd.utils.events import EventStorage

    g = gold("resnet_d_train")
    model = _r50d_model(train=True)
    assert [n for n, p in model.named_parameters() if not p.requires_grad] == g["frozen_names"].tolist()
    batch = []
    for i, (h, w, seed) in enumerate(_SIZES):
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
