"""GroupNorm on the device (csrc/group_norm.hip, lvc_amd.layers.GroupNorm, NORM: "GN" in the pyramid and the 4conv1fc box head).

Kernel tests: the oracle is torch.nn.functional.group_norm on the CPU in float64 (what the reference's nn.GroupNorm calls).  The bar
of every comparison is measured, not set (oracle/noise.py's convention): 3 x max |torch CPU fp32 - fp64| on the same input.  Every
(ours, reference noise, bar) triple is written to profiles/group_norm_parity.json (LVC_GN_PARITY_OUT: another path).

Model tests: the reference's GN model on CPU (tests/golden/gn_*.npz, train_gn.npz; scripts/make_golden_gn.py)."""
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

SHAPES = {            # shape -> (groups, forced tile height with >= 3 row tiles and a ragged last one)
    (2, 7, 7, 256): (32, 3),          # the box head's regime
    (1, 5, 3, 256): (32, 2),
    (3, 37, 53, 256): (32, 16),       # odd sizes, several workgroups per sample
    (2, 9, 11, 96): (32, 4),          # C/G = 3: the scalar-load instance
}
MODES = ("plain", "relu", "res1", "res2")
INPUTS = ("offset", "wide")           # x = 100 + randn (|mean| >> std), x = 50 * randn
REGIMES = ("whole", "split", "split_tiles")
RELU_GUARD = 1e-3                     # see _case: dy is zero where the fp64 pre-activation is within this of the ReLU's kink


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    yield
    if not _PARITY:
        return
    path = os.environ.get("LVC_GN_PARITY_OUT") or os.path.join(ROOT, "profiles", "group_norm_parity.json")
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
    _PARITY[key] = {"ours": ours, "noise": noise, "bar": bar}
    print("%-64s ours %.3e  noise %.3e  bar %.3e" % (key, ours, noise, bar))
    return bar


def _up2(res, H, W):
    return res.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :H, :W]


def _compose(x, gamma, beta, res, dy, G, mode):
    """The reference composition on the CPU in x's dtype, NHWC in / out: (y, mean, rstd, dx, dgamma, dbeta, dres)."""
    x = x.clone().requires_grad_(True)
    gamma, beta = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    res = res.clone().requires_grad_(True) if res is not None else None
    N, H, W, C = x.shape
    xc = x.permute(0, 3, 1, 2)
    y = F.group_norm(xc, G, gamma, beta, 1e-5).permute(0, 2, 3, 1)
    with torch.no_grad():
        _, mean, rstd = torch.native_group_norm(xc.detach().contiguous(), gamma.detach(), beta.detach(), N, C, H * W, G, 1e-5)
    pre = y.detach()
    if mode == "relu":
        y = F.relu(y)
    elif mode == "res1":
        y = y + res
    elif mode == "res2":
        y = y + _up2(res, H, W)
    (y * dy).sum().backward()
    return {"y": y.detach(), "pre": pre, "mean": mean.reshape(N, G), "rstd": rstd.reshape(N, G), "dx": x.grad, "dgamma": gamma.grad,
            "dbeta": beta.grad, "dres": res.grad if res is not None else None}


@functools.lru_cache(maxsize=None)
def _case(shape, kind, mode):
    """Seeded inputs and the CPU references in float32 and float64 (computed once per case, never modified)."""
    N, H, W, C = shape
    G = SHAPES[shape][0]
    g = torch.Generator().manual_seed(1000 * H + 10 * C + INPUTS.index(kind) + 100 * MODES.index(mode))
    x = torch.randn(shape, generator=g)
    x = 100.0 + x if kind == "offset" else 50.0 * x
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    res = None
    if mode == "res1":
        res = torch.randn(shape, generator=g)
    elif mode == "res2":
        res = torch.randn(N, (H + 1) // 2, (W + 1) // 2, C, generator=g)
    dy = torch.randn(shape, generator=g)
    if mode == "relu":
        # the ReLU's gradient is undefined to within rounding where the pre-activation is ~0: a mask flipped there by an fp32
        # evaluation (torch's or ours) would move dx by a whole dy.  No gradient is fed into those few elements.
        xd = x.double().permute(0, 3, 1, 2)
        pre64 = F.group_norm(xd, G, gamma.double(), beta.double(), 1e-5).permute(0, 2, 3, 1)
        dy = torch.where(pre64.abs() < RELU_GUARD, torch.zeros_like(dy), dy)
    r32 = _compose(x, gamma, beta, res, dy, G, mode)
    r64 = _compose(x.double(), gamma.double(), beta.double(), res.double() if res is not None else None, dy.double(), G, mode)
    return {"x": x, "gamma": gamma, "beta": beta, "res": res, "dy": dy, "G": G, "r32": r32, "r64": r64}


def _run_ours(c, mode):
    from lvc_amd.layers.batch_norm import _GroupNormFn

    d = _dev()
    x = c["x"].to(d).requires_grad_(True)
    gamma, beta = c["gamma"].to(d).requires_grad_(True), c["beta"].to(d).requires_grad_(True)
    res = c["res"].to(d).requires_grad_(True) if c["res"] is not None else None
    res_mode = {"plain": 0, "relu": 0, "res1": 1, "res2": 2}[mode]
    from lvc_amd import kernels as K

    with torch.no_grad():
        y0, mean, rstd = K.group_norm_nhwc(x.detach(), gamma.detach(), beta.detach(), c["G"], 1e-5, relu=mode == "relu",
                                           residual=res.detach() if res is not None else None, res_mode=res_mode)
    y = _GroupNormFn.apply(x, gamma, beta, res, c["G"], 1e-5, mode == "relu", res_mode)
    assert torch.equal(y.detach(), y0)                  # the autograd path launches the same forward
    y.backward(c["dy"].to(d))
    torch.cuda.synchronize()
    return {"y": y0, "mean": mean, "rstd": rstd, "dx": x.grad, "dgamma": gamma.grad, "dbeta": beta.grad,
            "dres": res.grad if res is not None else None}


def _set_regime(monkeypatch, regime, shape):
    from lvc_amd import kernels as K

    monkeypatch.setattr(K, "GN_SPLIT_MIN_HW", 1 << 40 if regime == "whole" else 1)
    monkeypatch.setattr(K, "GN_TILE_ROWS", SHAPES[shape][1] if regime == "split_tiles" else None)
    if regime == "split_tiles":
        H = shape[1]
        rows = SHAPES[shape][1]
        assert -(-H // rows) >= 3 and H % rows != 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forward_and_backward_match_torch_float64(shape, mode, monkeypatch):
    """y, mean, rstd, dx, dgamma, dbeta and the residual's gradient in every regime (one workgroup per sample, row tiles chosen by
    the host, row tiles forced small), each against float64 at 3 x torch's own fp32 deviation; the regimes agree within that bar."""
    failures = []
    for kind in INPUTS:
        c = _case(shape, kind, mode)
        outs = {}
        for regime in REGIMES:
            _set_regime(monkeypatch, regime, shape)
            outs[regime] = _run_ours(c, mode)
        for name in ("y", "mean", "rstd", "dx", "dgamma", "dbeta", "dres"):
            ref32, ref64 = c["r32"][name], c["r64"][name]
            if ref64 is None:
                continue
            noise = float((ref32.double() - ref64).abs().max())
            for regime in REGIMES:
                got = outs[regime][name].cpu().double()
                assert got.shape == ref64.shape
                ours = float((got - ref64).abs().max())
                key = "%s/%s/%s/%s/%s" % ("x".join(map(str, shape)), kind, mode, regime, name)
                bar = _record(key, ours, noise)
                if not ours <= bar:
                    failures.append((key, ours, bar))
            for regime in REGIMES[1:]:
                apart = float((outs[regime][name].double() - outs["whole"][name].double()).abs().max())
                if not apart <= K_NOISE * noise:
                    failures.append(("%s vs whole, %s %s %s" % (regime, kind, mode, name), apart, K_NOISE * noise))
    assert not failures, failures


def test_two_runs_are_bit_identical(monkeypatch):
    shape = (3, 37, 53, 256)
    for mode in ("relu", "res2"):
        c = _case(shape, "offset", mode)
        for regime in ("split", "split_tiles"):
            _set_regime(monkeypatch, regime, shape)
            a, b = _run_ours(c, mode), _run_ours(c, mode)
            for name, v in a.items():
                if v is not None:
                    assert torch.equal(v, b[name]), (mode, regime, name)


def test_bad_arguments_raise_through_the_abi():
    from lvc_amd import kernels as K
    from lvc_amd._lib import LvcNativeError

    d = _dev()
    assert issubclass(LvcNativeError, RuntimeError)
    w, b = torch.ones(48, device=d), torch.zeros(48, device=d)
    with pytest.raises(LvcNativeError, match="divisible"):
        K.group_norm_nhwc(torch.randn(1, 4, 4, 48, device=d), w, b, 32)
    w, b = torch.ones(64, device=d), torch.zeros(64, device=d)
    wide = torch.randn(2, 4, 4, 128, device=d)
    with pytest.raises(LvcNativeError, match="contiguous"):
        K.group_norm_nhwc(wide[..., :64], w, b, 32)
    with pytest.raises(LvcNativeError, match="contiguous"):
        K.group_norm_nhwc(torch.randn(2, 64, 4, 4, device=d).permute(0, 2, 3, 1), w, b, 32)
    x = torch.randn(2, 4, 4, 64, device=d)
    with pytest.raises(LvcNativeError, match="residual"):
        K.group_norm_nhwc(x, w, b, 32, relu=True, residual=torch.zeros_like(x), res_mode=1)
    y, mean, rstd = K.group_norm_nhwc(x, w, b, 32)           # and the same tensors are fine without the fault
    assert y.shape == x.shape and mean.shape == (2, 32) and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("shape", [(2, 6, 8, 64), (2, 7, 8, 64), (1, 6, 5, 96), (2, 9, 11, 6)])
def test_upsampled_residual_gradient_at_even_and_odd_sizes(shape):
    """The coarser map's gradient of a res_mode-2 add: sums of at most four addends, exact against float64 up to fp32 rounding of
    three additions (3 x 2^-24 relative to the sum of magnitudes); even sizes go through lvc_downsum2x2_nhwc, odd ones and channel
    counts that are no multiple of 4 through lvc_upsample2_add_grad_nhwc."""
    from lvc_amd import kernels as K

    N, H, W, C = shape
    g = torch.randn(shape, generator=torch.Generator().manual_seed(H * 100 + W))
    coarse = torch.zeros(N, (H + 1) // 2, (W + 1) // 2, C, dtype=torch.float64, requires_grad=True)
    (_up2(coarse, H, W) * g.double()).sum().backward()
    mag = torch.zeros_like(coarse)
    mag = torch.autograd.grad((_up2(coarse, H, W) * g.double().abs()).sum(), coarse)[0]
    got = K.upsample2_residual_grad(g.to(_dev()), coarse.shape).cpu().double()
    assert bool(((got - coarse.grad).abs() <= 3 * 2.0 ** -24 * mag).all())


def test_module_is_an_nchw_drop_in():
    from lvc_amd.layers import GroupNorm

    m = GroupNorm(32, 64).to(_dev())
    with torch.no_grad():
        m.weight.uniform_(0.5, 1.5)
        m.bias.uniform_(-0.5, 0.5)
    x = torch.randn(2, 64, 6, 5, device=_dev())
    ref = F.group_norm(x.cpu().double(), 32, m.weight.detach().cpu().double(), m.bias.detach().cpu().double(), 1e-5)
    noise = float((F.group_norm(x.cpu(), 32, m.weight.detach().cpu(), m.bias.detach().cpu(), 1e-5).double() - ref).abs().max())
    with torch.no_grad():
        got = m(x)
    assert got.shape == x.shape
    assert float((got.cpu().double() - ref).abs().max()) <= _record("module_nchw/y", float((got.cpu().double() - ref).abs().max()), noise)


# ------------------------------------------------------------------------------------------------ the GN model
def _gn_model(num_classes=80, fuse="sum"):
    from lvc_amd.config.presets import gn_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    cfg = gn_rcnn_fpn(num_classes=num_classes)
    cfg.MODEL.FPN.FUSE_TYPE = fuse
    return syn.conditioned_gn_r50_fpn_(build_model(cfg))


def _small_inputs():
    from lvc_amd.utils import synthetic as syn

    return [{"image": syn.synthetic_image(3, 240, 320), "height": 480, "width": 640},
            {"image": syn.synthetic_image(4, 200, 352), "height": 200, "width": 352}]


def _watch_branch(monkeypatch):
    """Counts the launches that tell the two walks of FPN.forward_nhwc apart."""
    from lvc_amd import kernels as K
    from lvc_amd.layers import GroupNorm

    seen = {"merged": 0, "gn": 0}
    real_levels, real_gn = K.conv3x3_levels, GroupNorm.forward_nhwc

    def levels(*a, **k):
        seen["merged"] += 1
        return real_levels(*a, **k)

    def gn(self, *a, **k):
        seen["gn"] += 1
        return real_gn(self, *a, **k)

    monkeypatch.setattr(K, "conv3x3_levels", levels)
    monkeypatch.setattr(GroupNorm, "forward_nhwc", gn)
    return seen


@pytest.mark.parametrize("training", [False, True])
def test_gn_pyramid_matches_reference(training, monkeypatch):
    """p2..p6 of the two small images against the reference backbone with GN (tests/golden/gn_fpn_small.npz), per level at 3 x the
    reference's own fp32-vs-fp64 deviation; in eval, and under autograd with the FPN's parameters trainable.  Both walk the
    level-by-level branch (eight GroupNorm launches, no merged output-conv launch)."""
    g = gold("gn_fpn_small")
    model = _gn_model()
    seen = _watch_branch(monkeypatch)
    inputs = _small_inputs()
    if training:
        model.train()
        assert all(p.requires_grad for n, p in model.backbone.named_parameters() if n.startswith("fpn_"))
        feats = model.backbone(model.preprocess_image(inputs).tensor)
        assert all(v.requires_grad for v in feats.values())
    else:
        model.eval()
        with torch.no_grad():
            feats = model.backbone(model.preprocess_image(inputs).tensor)
    assert seen == {"merged": 0, "gn": 8}
    bad = []
    for k in ("p2", "p3", "p4", "p5", "p6"):
        got = feats[k].detach()[:, ::16, ::2, ::2].cpu()
        assert got.shape == g["feat_" + k].shape
        ours = float((got - g["feat_" + k]).abs().max())
        bar = _record("pyramid/%s/%s" % ("train" if training else "eval", k), ours, float(g["noise_" + k]))
        if not ours <= bar:
            bad.append((k, ours, bar))
    assert not bad, bad


@pytest.mark.parametrize("training", [False, True])
def test_gn_pyramid_with_avg_fusion_walks_the_level_branch(training, monkeypatch):
    avg, summed = _gn_model(fuse="avg"), _gn_model(fuse="sum")
    seen = _watch_branch(monkeypatch)
    x = avg.preprocess_image(_small_inputs()).tensor
    with torch.set_grad_enabled(training):
        fa, fs = avg.train(training).backbone(x), summed.train(training).backbone(x)
    assert seen == {"merged": 0, "gn": 16}
    assert torch.equal(fa["p5"], fs["p5"]) and not torch.equal(fa["p2"], fs["p2"])      # the coarsest level has no top-down term
    assert bool(torch.isfinite(fa["p2"]).all())


def test_gn_box_head_matches_reference():
    g = gold("gn_box_head")
    head = _gn_model().roi_heads.box_head.eval()
    with torch.no_grad():
        # the fixture's input (scripts/make_golden_gn.py box_head_input, BOX_HEAD_SEED)
        got = head(torch.randn(5, 256, 7, 7, generator=torch.Generator().manual_seed(21)).to(_dev())).cpu()
    assert got.shape == g["out32"].shape == (5, 1024)
    noise = float((g["out32"].double() - g["out64"]).abs().max())
    ours = float((got.double() - g["out32"].double()).abs().max())
    assert ours <= _record("box_head/out", ours, noise)


def test_empty_head_input_launches_nothing(monkeypatch):
    from lvc_amd import kernels as K

    head = _gn_model().roi_heads.box_head.eval()

    def boom(*a, **k):
        raise AssertionError("a kernel was launched for an empty batch")

    for name in ("conv2d_nhwc", "group_norm_nhwc", "linear"):
        monkeypatch.setattr(K, name, boom)
    with torch.no_grad():
        out = head.forward_nhwc(torch.zeros(0, 7, 7, 256, device=_dev()))
    assert tuple(out.shape) == (0, 1024)


def test_gn_training_step_matches_reference(monkeypatch):
    """One training step of the GN model against the reference's (tests/golden/train_gn.npz), at the bars
    tests/test_gpu_train.py::test_base_detector_training_step_matches_reference applies to train_base.npz: losses to 2e-4,
    gradients by direction (cosine >= 0.998 on the stored sample) and size (norm within 1e-2)."""
    from lvc_amd.structures import Boxes, Instances
    from lvc_amd.utils import synthetic as syn
    from lvc_amd.utils.events import EventStorage

    LOSS_TOL, COS_MIN, NORM_TOL = 2e-4, 0.998, 1e-2
    g = gold("train_gn")
    model = _gn_model(num_classes=60).train()
    batch = []
    for i, (h, w, seed) in enumerate(((240, 320, 3), (200, 352, 4))):
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(g["gt_boxes%d" % i])
        inst.gt_classes = g["gt_classes%d" % i]
        batch.append({"image": syn.synthetic_image(seed, h, w), "instances": inst, "height": h, "width": w})
    monkeypatch.setattr(torch, "randperm", lambda n, **kw: torch.arange(n, **{k: v for k, v in kw.items() if k in ("device", "dtype")}))
    with EventStorage(0) as storage:
        losses = model(batch)
        sum(losses.values()).backward()
    bad = {}
    for k in ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"):
        ref, got = float(g["loss." + k]), float(losses[k].detach())
        print(k, got, ref)
        if not abs(got - ref) <= LOSS_TOL * max(1.0, abs(ref)):
            bad[k] = (got, ref)
    lat = storage.latest()
    assert lat["rpn/num_pos_anchors"] == float(g["scalar.rpn.num_pos_anchors"])
    assert lat["roi_head/num_fg_samples"] == float(g["scalar.roi_head.num_fg_samples"])
    params = dict(model.named_parameters())
    names = g["grad_names"].tolist()
    assert len(names) == 27
    for name in names:
        p = params[name]
        assert p.requires_grad and p.grad is not None, name
        gflat = p.grad.flatten().cpu()
        s, nrm, stride = [float(v) for v in g["grad_stats." + name]]
        sample = gflat[:: int(stride)][:2048].double()
        ref = g["grad_sample." + name].double()
        if nrm == 0.0:   # (as in test_gpu_train.py) identity randperm samples the first anchors (all on p2) and no RoI is pooled from p5
            assert float(gflat.abs().max()) == 0.0, name
            continue
        cos = float((sample * ref).sum() / (sample.norm() * ref.norm()).clamp_min(1e-30))
        nerr = abs(float(gflat.double().norm()) - nrm) / max(nrm, 1e-12)
        print("%-52s cos %.6f  norm err %.2e" % (name, cos, nerr))
        if not (cos >= COS_MIN and nerr <= NORM_TOL):
            bad[name] = (cos, nerr)
    assert not bad, bad


def test_gn_model_end_to_end_is_deterministic():
    from lvc_amd.structures import Instances

    model = _gn_model().eval()
    inputs = _small_inputs()
    with torch.no_grad():
        a, b = model(inputs), model(inputs)
    assert len(a) == 2
    for ra, rb in zip(a, b):
        ia, ib = ra["instances"], rb["instances"]
        assert isinstance(ia, Instances)
        assert torch.equal(ia.pred_boxes.tensor, ib.pred_boxes.tensor) and torch.equal(ia.scores, ib.scores)
        assert torch.equal(ia.pred_classes, ib.pred_classes)
        assert bool(torch.isfinite(ia.pred_boxes.tensor).all())
