"""RetinaNet training, model level: `label_anchors` and one training step against the reference's CPU step
(tests/golden/retinanet_train.npz, scripts/make_golden_retinanet_train.py), the normaliser state, the single host read, an optimizer
step, loss scaling, and inference afterwards.

The step is held to the bars tests/test_gpu_resnet_d.py::test_reference_r50_d_training_step takes from the base-detector step: both
losses within 2e-4 * max(1, |ref|); on every trainable parameter cosine >= 0.998 on the sampled gradient and gradient-norm error <= 1e-2;
frozen parameters without a gradient."""
import json
import os

import pytest
import torch

from helpers import ROOT, gold

pytestmark = pytest.mark.gpu

_SIZES = ((128, 160, 3), (120, 176, 4))
K = 20
_PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def write_parity():
    yield
    if not _PARITY:
        return
    path = os.environ.get("LVC_RETINANET_LOSS_PARITY_OUT") or os.path.join(ROOT, "profiles", "retinanet_loss_parity.json")
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


def _model():
    from lvc_amd.config.presets import retinanet_r_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    cfg = retinanet_r_fpn(num_classes=K)
    m = build_model(cfg)
    syn.conditioned_retinanet_(m, seed=0)
    return cfg, m.enable_training().train()


@pytest.fixture(scope="module")
def trained():
    """One model for the tests that only read it or run further passes on it."""
    return _model()


def _instances(boxes, classes, hw, dev=None):
    from lvc_amd.structures import Boxes, Instances

    inst = Instances(hw)
    inst.gt_boxes = Boxes(boxes.to(dev) if dev is not None else boxes)
    inst.gt_classes = classes.to(dev) if dev is not None else classes
    return inst


def _batch(case="a", dev=None):
    from lvc_amd.utils import synthetic as syn

    g = gold("retinanet_train")
    if case == "a":
        gts = [(g["a_gt_boxes0"], g["a_gt_classes0"]), (g["a_gt_boxes1"], g["a_gt_classes1"])]
    else:
        gts = [(g["b_gt_boxes0"], g["b_gt_classes0"]), (torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64))]
    out = []
    for (h, w, seed), (b, c) in zip(_SIZES, gts):
        im = syn.synthetic_image(seed, h, w)
        out.append({"image": im.to(dev) if dev is not None else im, "instances": _instances(b, c, (h, w), dev), "height": h, "width": w})
    return out


def _check_grads(model, g, tag, scale=1.0):
    bad, worst_cos, worst_nerr = {}, 1.0, 0.0
    for name, p in model.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, name
            continue
        assert p.grad is not None, name
        gflat = p.grad.flatten().cpu() / scale
        _s, nrm, stride = [float(v) for v in g["grad_stats." + name]]
        sample = gflat[:: int(stride)][:2048].double()
        ref = g["grad_sample." + name].double()
        if nrm == 0.0:
            assert float(gflat.abs().max()) == 0.0, name
            continue
        cos = float((sample * ref).sum() / (sample.norm() * ref.norm()).clamp_min(1e-30))
        nerr = abs(float(gflat.double().norm()) - nrm) / max(nrm, 1e-12)
        print("%-52s cos %.6f  norm err %.2e" % (name, cos, nerr))
        worst_cos, worst_nerr = min(worst_cos, cos), max(worst_nerr, nerr)
        if not (cos >= 0.998 and nerr <= 1e-2):
            bad[name] = (cos, nerr)
    _PARITY["train_step/%s/grad_cosine_min" % tag] = {"ours": worst_cos, "bar": 0.998}
    _PARITY["train_step/%s/grad_norm_err_max" % tag] = {"ours": worst_nerr, "bar": 1e-2}
    assert not bad, bad


@pytest.mark.parametrize("case", ["a", "b"])
def test_label_anchors_equals_the_reference(trained, case):
    _cfg, model = trained
    g = gold("retinanet_train")
    batch = _batch(case)
    images = model.preprocess_image(batch)
    Hp, Wp = images.tensor.shape[-2:]
    grids = [(-(-Hp // s), -(-Wp // s)) for s in model.anchor_generator.strides]
    from lvc_amd.structures import Boxes

    anchors = [Boxes(t) for t in model.anchor_generator._grid_anchors(grids)]
    labels, boxes = model.label_anchors(anchors, [b["instances"] for b in batch])
    want = g[case + "_gt_labels"].long()
    got = torch.stack(labels).cpu()
    assert got.dtype == torch.int64 and torch.equal(got, want)
    pos = (want >= 0) & (want != K)
    for i, b in enumerate(batch):
        gtb = b["instances"].gt_boxes.tensor
        assert tuple(boxes[i].shape) == (want.shape[1], 4)
        if len(gtb):
            assert torch.equal(boxes[i].cpu()[pos[i]], gtb[g[case + "_matched"][i].long()[pos[i]]])


def test_reference_training_step():
    from lvc_amd.utils.events import EventStorage

    g = gold("retinanet_train")
    _cfg, model = _model()
    assert [n for n, p in model.named_parameters() if not p.requires_grad] == g["frozen_names"].tolist()
    batch = _batch("a")
    with EventStorage(0) as storage:
        losses = model(batch)
        assert set(losses) == {"loss_cls", "loss_box_reg"} and all(v.is_cuda and v.dim() == 0 for v in losses.values())
        n1 = model.loss_normalizer
        sum(losses.values()).backward()
        with torch.no_grad():
            model(batch)
        n2 = model.loss_normalizer
        logged = storage.latest()["num_pos_anchors"]
    logged = logged[0] if isinstance(logged, (tuple, list)) else logged
    assert float(logged) == float(g["num_pos"].sum()) / 2
    assert [n1, n2] == [float(v) for v in g["normalizer"]]
    for k in ("loss_cls", "loss_box_reg"):
        ref, got = float(g["loss." + k]), float(losses[k].detach())
        print(k, got, ref, "fp64", float(g["loss64." + k]))
        _PARITY["train_step/%s" % k] = {"ours": abs(got - ref), "bar": 2e-4 * max(1.0, abs(ref)), "reference_fp32_vs_fp64": abs(ref - float(g["loss64." + k]))}
        assert abs(got - ref) <= 2e-4 * max(1.0, abs(ref)), k
    _check_grads(model, g, "plain")


def test_repeated_pass_advances_the_normaliser_once(trained, monkeypatch):
    """A pass that `run_with_fallbacks` repeats (a layer re-routed to a wider form) must not advance the EMA twice.  The condition is
    a Python exception raised in place of the range check; nothing on the device is provoked."""
    from lvc_amd import kernels as Kn
    from lvc_amd.utils.events import EventStorage

    _cfg, model = trained
    g = gold("retinanet_train")
    model.loss_normalizer = 100.0
    calls = {"n": 0, "summary": 0}
    real_summary = Kn.range_summary

    def summary(device):
        calls["summary"] += 1
        return torch.ones(1, dtype=torch.int32, device=device) if calls["summary"] == 1 else real_summary(device)

    def check(device):
        calls["n"] += 1
        e = Kn.Fp16RangeError("a layer was re-routed (test)")
        e.rerouted = True
        raise e

    monkeypatch.setattr(Kn, "range_summary", summary)
    monkeypatch.setattr(Kn, "check_conv_error_word", check)
    with EventStorage(0), torch.no_grad():
        model(_batch("a"))
    assert calls["n"] == 1 and calls["summary"] == 2
    assert model.loss_normalizer == float(g["normalizer"][0])


def test_training_forward_reads_the_device_once(trained, monkeypatch):
    """Everything up to the forward's one read (num_pos + the range summary) runs under torch's sync-debug mode "error"."""
    from lvc_amd import kernels as Kn
    from lvc_amd.utils.events import EventStorage

    _cfg, model = trained
    batch = _batch("a", _dev())
    with EventStorage(0):
        model(batch)                    # packs the weights, fills the caches
        torch.cuda.synchronize()
        real = Kn.range_summary
        reads = []

        def summary(device):            # the last thing queued before the read: sync-debug goes back to "default" here
            out = real(device)
            torch.cuda.set_sync_debug_mode("default")
            reads.append(1)
            return out

        monkeypatch.setattr(Kn, "range_summary", summary)
        torch.cuda.set_sync_debug_mode("error")
        try:
            losses = model(batch)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert reads == [1] and bool(torch.isfinite(losses["loss_cls"]))


def test_optimizer_step_then_next_forward_then_inference():
    from lvc_amd.solver import build_optimizer
    from lvc_amd.utils.events import EventStorage

    cfg, model = _model()
    opt = build_optimizer(cfg, model)
    batch = _batch("a")
    w0 = model.head.cls_score.weight.detach().clone()
    with EventStorage(0):
        l0 = model(batch)
        sum(l0.values()).backward()
        opt.step()
        opt.zero_grad()
        assert not torch.equal(model.head.cls_score.weight.detach(), w0)
        l1 = model(batch)
    assert all(bool(torch.isfinite(v)) for v in l1.values())
    assert float(l1["loss_cls"]) != float(l0["loss_cls"])
    model.eval()
    with torch.no_grad():
        out = model([{k: v for k, v in b.items() if k != "instances"} for b in batch])
    assert len(out) == 2 and all(len(o["instances"]) >= 0 and o["instances"].pred_boxes.tensor.shape[-1] == 4 for o in out)


def test_loss_scaler_step_matches_after_unscaling():
    from lvc_amd.solver import LossScaler
    from lvc_amd.utils.events import EventStorage

    g = gold("retinanet_train")
    _cfg, model = _model()
    scaler = LossScaler()
    with EventStorage(0):
        losses = model(_batch("a"))
        scaler.backward(sum(losses.values()))
    _check_grads(model, g, "loss_scaler", scale=scaler.scale_value)
