"""Mask R-CNN training on the device: lvc_mask_deconv_logits, lvc_mask_loss and lvc_mask_deconv_grad (csrc/mask_deconv.hip,
csrc/mask_train.hip) against tests/mask_train_ref.py in fp64, each bar 3 x what an fp32 torch-CPU run of the same expression deviates
from fp64 on the same input; then a whole training step of a mask model against the reference's own recorded step.  Every ratio goes
to profiles/mask_train_parity.json (LVC_MASK_TRAIN_PARITY_OUT: another path)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mask_train_ref as R
from helpers import ROOT, gold

pytestmark = pytest.mark.gpu

_PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def write_parity():
    yield
    if not _PARITY:
        return
    path = os.environ.get("LVC_MASK_TRAIN_PARITY_OUT") or os.path.join(ROOT, "profiles", "mask_train_parity.json")
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


def _record(key, ours, noise, bar=None):
    bar = 3.0 * noise if bar is None else bar
    _PARITY[key] = {"ours": ours, "noise": noise, "bar": bar, "ratio": ours / bar if bar > 0 else float("inf") if ours > 0 else 0.0}
    print("%-52s ours %.3e  fp32 reference's own %.3e  bar %.3e" % (key, ours, noise, bar))
    return bar


# ------------------------------------------------------------------ cases
# name -> ((M, S, Cin, Cmid, K), options): classes "own" = synthetic.mask_tail_case's, "sparse" = repeated classes with absent ones
# between and above them, None = class-agnostic; num_valid (rows past it hold NaN); upstream scalar g; plant: logits overwritten
CASES = {
    "1x1": ((1, 1, 64, 64, 1), dict()),
    "3x7": ((3, 7, 64, 128, 3), dict()),                       # 49 pixels: fewer than one tile
    "3x7-g1024": ((3, 7, 64, 128, 3), dict(g=1024.0)),
    "5x14": ((5, 14, 192, 256, 20), dict()),                   # the last tile of a RoI has 4 rows
    "37x14-sparse-g1024": ((37, 14, 256, 256, 20), dict(classes="sparse", g=1024.0)),
    "agnostic": ((3, 7, 64, 128, 1), dict(classes=None)),
    "num_valid": ((5, 7, 64, 128, 3), dict(num_valid=3)),
    "num_valid-0": ((3, 7, 64, 128, 3), dict(num_valid=0)),
    "planted": ((3, 7, 64, 128, 3), dict(plant=True)),
}
PLANTED = (0.0, 30.0, -30.0, 90.0, -90.0)
_REF = {}


def _operands(name):
    from lvc_amd.utils import synthetic as syn

    shape, opt = CASES[name]
    x, wd, bd, wp, bp, classes = syn.mask_tail_case(*shape)
    mode = opt.get("classes", "own")
    if mode == "sparse":
        classes = (torch.arange(shape[0]) % 7) * 2          # 0, 2, .. 12 several times each; the odd classes and 13 .. 19 are absent
    elif mode is None:
        classes = None
    M, S = shape[0], shape[1]
    g = torch.Generator().manual_seed(4242 + M + S)
    t = torch.rand(M, 2 * S, 2 * S, generator=g) > 0.6
    nv = opt.get("num_valid", M)
    if nv < M:
        x = x.clone()
        x[nv:] = float("nan")
    plant = None
    if opt.get("plant"):
        idx = torch.randperm(M * 4 * S * S, generator=g)[: 10 * len(PLANTED)]
        plant = (idx, torch.tensor(PLANTED).repeat(10))
    return (x, wd, bd, wp, bp, classes), t, nv, float(opt.get("g", 1.0)), plant


def _torch_autograd(ops, t, nv, g, dtype, planted_z=None):
    """torch's own operators and autograd on the CPU: (logits, loss, the five gradients) of the first nv rows."""
    x, wd, bd, wp, bp, classes = ops
    ps = [p[:nv].to(dtype).clone().requires_grad_() if i == 0 else p.to(dtype).clone().requires_grad_() for i, p in enumerate((x, wd, bd, wp, bp))]
    c = torch.zeros(nv, dtype=torch.int64) if classes is None else classes[:nv]
    z = F.conv2d(F.relu(F.conv_transpose2d(ps[0], ps[1], ps[2], stride=2)), ps[3], ps[4])[torch.arange(nv), c]
    logits = z.detach().clone()
    if planted_z is not None:
        z = planted_z.to(dtype) + (z - z.detach())          # the planted values, with the graph of the computed ones
    loss = F.binary_cross_entropy_with_logits(z, t[:nv].to(dtype)) if nv else z.sum() * 0
    (loss * g).backward()
    grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in ps]
    dx = torch.zeros(x.shape, dtype=dtype)
    dx[:nv] = grads[0]
    return logits, loss.detach(), {"dx": dx, "dWd": grads[1], "dbd": grads[2], "dWp": grads[3].reshape(wp.shape[0], -1), "dbp": grads[4]}


def _reference(name):
    """The fp64 restatement and torch's fp32 deviation from it, computed once per case and shared."""
    if name in _REF:
        return _REF[name]
    ops, t, nv, g, plant = _operands(name)
    x, wd, bd, wp, bp, classes = ops
    sl = (x[:nv], wd, bd, wp, bp, None if classes is None else classes[:nv])
    z64 = R.tail_logits(*sl)[0]
    zp = None
    if plant is not None:
        zp = z64.clone().view(-1)
        zp[plant[0]] = plant[1].double()
        zp = zp.view_as(z64)
    exact = R.grads(*sl, t[:nv], upstream=g, z=zp)
    dx = torch.zeros(x.shape, dtype=torch.float64)
    dx[:nv] = exact["dx"]
    exact["dx"] = dx
    z32, _l32, g32 = _torch_autograd(ops, t, nv, g, torch.float32, None if zp is None else zp.float())
    noise = {k: float((g32[k].double() - exact[k]).abs().max()) for k in exact}
    noise["z"] = float((z32.double() - z64).abs().max()) if nv else 0.0
    _REF[name] = (ops, t, nv, g, plant, z64, exact, noise)
    return _REF[name]


def _run(name, corrupt_class=False):
    """-> dict of the kernels' results on the case (CPU tensors)."""
    from lvc_amd import kernels as K

    ops, t, nv, g, plant, _z64, _exact, _noise = _reference(name)
    x, wd, bd, wp, bp, classes = ops
    dev = _dev()
    M, S = x.shape[0], x.shape[2]
    xn = x.permute(0, 2, 3, 1).contiguous().to(dev)
    packed = K.pack_mask_deconv(wd.to(dev))
    wp2 = wp.reshape(wp.shape[0], -1).contiguous().to(dev)
    cls = None if classes is None else classes.to(torch.int32).to(dev)
    if corrupt_class:
        cls = cls.clone()
        cls[0] = wp.shape[0]
    num_valid = None if nv == M else torch.tensor([nv], dtype=torch.int32, device=dev)
    status = K.new_status(dev)
    z = torch.full((M, 2 * S, 2 * S), float("nan"), device=dev)
    K.mask_deconv_logits(xn, packed, bd.to(dev), wp2, bp.to(dev), classes=cls, num_valid=num_valid, status=status, out=z)
    prob = K.mask_deconv_predict(xn, packed, bd.to(dev), wp2, bp.to(dev), classes=cls, num_valid=num_valid)
    if plant is not None:
        z.view(-1)[plant[0].to(dev)] = plant[1].to(dev)
    tb = t.to(dev).to(torch.uint8)
    loss, total, counts = K.mask_loss(z, tb, num_valid)
    up = torch.tensor([g], dtype=torch.float32, device=dev)
    dx, dwd, dbd, dwp, dbp = K.mask_deconv_grad(xn, packed, bd.to(dev), wp2, cls, z, tb, num_valid, up, status=status)
    torch.cuda.synchronize()
    return {"z": z.cpu(), "prob": prob.cpu(), "sig": (1.0 / (1.0 + torch.exp(-z))).cpu(), "loss": loss.cpu(), "sum": total.cpu(),
            "counts": counts.cpu(), "status": int(status.item()), "dx": dx.permute(0, 3, 1, 2).cpu(), "dWd": dwd.cpu(), "dbd": dbd.cpu(),
            "dWp": dwp.cpu(), "dbp": dbp.cpu()}


_OUT = {}


def _out(name):
    if name not in _OUT:
        _OUT[name] = _run(name)
    return _OUT[name]


@pytest.mark.parametrize("name", list(CASES))
def test_logits(name):
    ops, t, nv, g, plant, z64, exact, noise = _reference(name)
    o = _out(name)
    assert o["status"] == 0
    if nv == 0:
        assert bool(torch.isnan(o["z"]).all())          # nothing is written
        return
    z = o["z"][:nv]
    if plant is not None:
        zf = z.reshape(-1)
        assert torch.equal(zf[plant[0]], plant[1])
        keep = torch.ones(zf.numel(), dtype=torch.bool)
        keep[plant[0]] = False
        err = float((zf.double() - z64.reshape(-1))[keep].abs().max())
    else:
        err = float((z.double() - z64).abs().max())
        # the inference entry with the same classes: the same pass, then the sigmoid
        assert torch.equal(o["sig"][:nv], o["prob"][:nv]), "sigmoid(logits) differs from lvc_mask_deconv_predict in %d values" % int((o["sig"][:nv] != o["prob"][:nv]).sum())
    assert bool(torch.isnan(o["z"][nv:]).all()), "rows past num_valid were written"
    bar = _record("logits/%s" % name, err, noise["z"])
    assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_counts(name):
    ops, t, nv, g, plant, z64, exact, noise = _reference(name)
    o = _out(name)
    z = o["z"][:nv]
    s64, mean64, counts = R.loss(z, t[:nv])                  # the formula in fp64 on the kernel's own logits
    _s32, mean32, _ = R.loss(z, t[:nv], torch.float32)
    if nv == 0:
        assert float(o["loss"]) == 0.0 and float(o["sum"]) == 0.0 and o["counts"].tolist() == [0, 0, 0]
        return
    rel = abs(float(o["sum"]) - float(s64)) / abs(float(s64))
    _PARITY["loss_sum/%s" % name] = {"relative": rel, "bar": 1e-12}
    assert rel <= 1e-12, (name, rel)
    dev32 = abs(float(mean32.double() - mean64))
    bar = _record("loss_mean/%s" % name, abs(float(o["loss"].double() - mean64)), dev32)
    assert abs(float(o["loss"].double() - mean64)) <= bar, (name, float(o["loss"]), float(mean64))
    # the counts: exact on the kernel's own logits; against the fp64 logits once the pixels with |z| below the logit bar are set aside
    assert o["counts"].tolist() == list(counts), (o["counts"].tolist(), counts)
    if plant is None:
        near = z64.abs() <= 3 * noise["z"]
        _, _, c64 = R.loss(z64, t[:nv])
        share = float(near.sum()) / near.numel()
        _PARITY["counts/%s" % name] = {"set_aside": int(near.sum()), "pixels": near.numel(), "share": share}
        print("counts/%s: %d of %d pixels set aside (|z| <= %.2e)" % (name, int(near.sum()), near.numel(), 3 * noise["z"]))
        assert abs(counts[0] - c64[0]) <= int(near.sum()) and counts[1] == c64[1] and abs(counts[2] - c64[2]) <= int(near.sum())
    else:
        assert math_isfinite(o["loss"]) and math_isfinite(o["sum"])


def math_isfinite(t):
    return bool(torch.isfinite(t).all())


@pytest.mark.parametrize("name", list(CASES))
def test_gradients(name):
    ops, t, nv, g, plant, z64, exact, noise = _reference(name)
    o = _out(name)
    classes = ops[5]
    K_ = ops[3].shape[0]
    for key in ("dx", "dWd", "dbd", "dWp", "dbp"):
        got = o[key].reshape(exact[key].shape)
        assert math_isfinite(got), key
        err = float((got.double() - exact[key]).abs().max())
        bar = _record("%s/%s" % (key, name), err, noise[key])
        assert err <= bar, (name, key, err, bar)
    present = set([0] if classes is None else classes[:nv].tolist()) if nv else set()
    absent = [k for k in range(K_) if k not in present]
    if absent:
        assert not bool(o["dWp"][absent].any()) and not bool(o["dbp"][absent].any()), "rows of absent classes are not exactly zero"
    if name == "37x14-sparse-g1024":
        assert len(absent) == 13 and all(bool(o["dWp"][k].any()) for k in present)
    assert not bool(o["dx"][nv:].any())


@pytest.mark.parametrize("name", ["3x7", "3x7-g1024", "5x14", "37x14-sparse-g1024"])
def test_dx_with_the_fp16_split_meets_the_same_bar(monkeypatch, name):
    """`dx = dh Wd` runs on the forward GEMM under `kernels.DGRAD_SPLIT`: bf16x3 (range-free) by default, the two-way fp16 split under a
    LossScaler.  Both ratios go to the parity file; both must meet the bar of the default."""
    from lvc_amd import kernels as K

    exact, noise = _reference(name)[6], _reference(name)[7]
    assert K.DGRAD_SPLIT == "bf16x3"
    errs = {"bf16x3": float((_out(name)["dx"].double() - exact["dx"]).abs().max())}
    monkeypatch.setattr(K, "DGRAD_SPLIT", "f16x2")
    o = _run(name)
    assert math_isfinite(o["dx"]) and K.conv_error_word(_dev()) == 0
    errs["f16x2"] = float((o["dx"].double() - exact["dx"]).abs().max())
    for split, err in errs.items():
        bar = _record("dx_%s/%s" % (split, name), err, noise["dx"])
        assert err <= bar, (name, split, err, bar)


@pytest.mark.parametrize("name", ["5x14", "37x14-sparse-g1024", "num_valid"])
def test_two_runs_give_the_same_bits(name):
    a, b = _out(name), _run(name)
    nv = _reference(name)[2]
    for key in ("loss", "sum", "counts", "dx", "dWd", "dbd", "dWp", "dbp"):
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(a["z"][:nv], b["z"][:nv])


def test_a_class_out_of_range_sets_the_status_bit():
    from lvc_amd import kernels as K

    assert _out("3x7")["status"] == 0
    assert _run("3x7", corrupt_class=True)["status"] & K.MASK_BAD_CLASS


def test_autograd_function_is_the_kernels():
    """`MaskTailLoss` (what the head's training forward is built on): the same loss and gradients through torch's autograd, with the
    upstream scalar a device tensor."""
    from lvc_amd.modeling.roi_heads.mask_head import MaskTailLoss

    ops, t, nv, g, plant, z64, exact, noise = _reference("3x7-g1024")
    o = _out("3x7-g1024")
    x, wd, bd, wp, bp, classes = ops
    dev = _dev()
    ps = [p.to(dev).requires_grad_() for p in (x.permute(0, 2, 3, 1).contiguous(), wd, bd, wp, bp)]
    loss, total, counts = MaskTailLoss.apply(*ps, classes.to(torch.int32).to(dev), t.to(dev).to(torch.uint8), None, None, None)
    (loss * torch.tensor(g, device=dev)).backward()
    assert loss.dim() == 0 and torch.equal(loss.detach().cpu().view(1), o["loss"]) and torch.equal(counts.cpu(), o["counts"])
    for key, p in zip(("dx", "dWd", "dbd", "dWp", "dbp"), ps):
        got = p.grad.permute(0, 3, 1, 2).cpu() if key == "dx" else p.grad.cpu()
        assert torch.equal(got.reshape(o[key].shape), o[key]), key


# ------------------------------------------------------------------ the model step
_SIZES = ((128, 160, 3), (120, 176, 4))
BATCH_SIZE_PER_IMAGE = 128          # as scripts/make_golden_mask_train.py
LOSSES = ("loss_cls", "loss_box_reg", "loss_mask", "loss_rpn_cls", "loss_rpn_loc")


def _identity_randperm(monkeypatch):
    monkeypatch.setattr(torch, "randperm", lambda n, **kw: torch.arange(n, **{k: v for k, v in kw.items() if k in ("device", "dtype")}))


def _mask_model(mask_on=True):
    from lvc_amd.config.presets import base_rcnn_fpn, mask_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    cfg = (mask_rcnn_fpn if mask_on else base_rcnn_fpn)(num_classes=20)
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = BATCH_SIZE_PER_IMAGE
    m = build_model(cfg)
    m = syn.conditioned_mask_head_(m) if mask_on else syn.conditioned_r50_fpn_(m)
    m.train()
    return m.enable_mask_training() if mask_on else m


def _gt_masks(g, i):
    h, w, _ = _SIZES[i]
    n = len(g["gt_classes%d" % i])
    return torch.from_numpy(np.unpackbits(g["gt_masks%d" % i].numpy())[: n * h * w].reshape(n, h, w)).bool()


def _step_batch(g, masks=True, device=None):
    from lvc_amd.structures import BitMasks, Boxes, Instances
    from lvc_amd.utils import synthetic as syn

    batch = []
    for i, (h, w, seed) in enumerate(_SIZES):
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(g["gt_boxes%d" % i])
        inst.gt_classes = g["gt_classes%d" % i]
        if masks:
            inst.gt_masks = BitMasks(_gt_masks(g, i))
        image = syn.synthetic_image(seed, h, w)
        if device is not None:
            inst, image = inst.to(device), image.to(device)
        batch.append({"image": image, "instances": inst, "height": h, "width": w})
    return batch


def _check_step(g, model, losses, scalars, tag):
    for k in LOSSES:
        ref, got = float(g["loss." + k]), float(losses[k].detach())
        _PARITY["step/%s/%s" % (tag, k)] = {"ours": got, "reference": ref, "relative": abs(got - ref) / max(1.0, abs(ref)),
                                            "reference_fp32_vs_fp64": float(g["loss_dev." + k])}
        print("%-14s ours %.7f  reference %.7f (its own fp32-vs-fp64 deviation %.2e)" % (k, got, ref, float(g["loss_dev." + k])))
        assert abs(got - ref) <= 2e-4 * max(1.0, abs(ref)), k
    if scalars is not None:
        for name in ("rpn/num_pos_anchors", "roi_head/num_fg_samples", "roi_head/num_bg_samples"):
            assert scalars[name] == float(g["scalar." + name.replace("/", ".")]), name
        # the three logged scalars are ratios of pixel counts: equal to the reference's but for pixels whose logit the step cannot tell
        # from 0 -- those of the reference's own logits within the losses' bar (2e-4 of the largest logit) of 0; each may move a count by one
        n = sum(len(g["fg_classes%d" % i]) for i in range(2)) * 28 * 28
        pos = sum(int(np.unpackbits(g["targets%d" % i].numpy())[: len(g["fg_classes%d" % i]) * 784].sum()) for i in range(2))
        z_ref = g["fg_logits"]
        aside = int((z_ref.abs() <= 2e-4 * float(z_ref.abs().max())).sum())
        print("logged scalars: %d of %d pixels set aside" % (aside, n))
        _PARITY["step/%s/scalars" % tag] = {"set_aside": aside, "pixels": n}
        for name, denom in (("mask_rcnn/accuracy", n), ("mask_rcnn/false_positive", n - pos), ("mask_rcnn/false_negative", pos)):
            ref = float(g["scalar." + name.replace("/", ".")])
            print("%-26s ours %.6f  reference %.6f" % (name, scalars[name], ref))
            assert abs(scalars[name] - ref) <= aside / max(denom, 1) + 1e-15, name
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
        if "mask_head" in name:
            print("%-52s cos %.6f  norm err %.2e" % (name, cos, nerr))
            _PARITY["step/%s/grad/%s" % (tag, name)] = {"cosine": cos, "norm_error": nerr}
        if not (cos >= 0.998 and nerr <= 1e-2):
            bad[name] = (cos, nerr)
    assert not bad, bad


@pytest.fixture(scope="module")
def step_model():
    return _mask_model()


def _latest(storage):
    return {k: (v[0] if isinstance(v, tuple) else v) for k, v in storage.latest().items()}


def test_mask_training_step_matches_reference(monkeypatch, step_model):
    """One step of the reference's Mask R-CNN (tests/golden/mask_train.npz: FREEZE_AT 2, 20 classes, two small images, identity
    randperm) at the bars of train_base.npz: losses within 2e-4 relative, every trainable gradient with cosine >= 0.998 and norm
    error <= 1e-2; the deferred path, which must make exactly one device->host read."""
    from lvc_amd import kernels as Kn
    from lvc_amd.utils.events import EventStorage

    g = gold("mask_train")
    model = step_model
    assert [n for n, p in model.named_parameters() if not p.requires_grad] == g["frozen_names"].tolist()
    _identity_randperm(monkeypatch)
    batch = _step_batch(g, device=_dev())
    with EventStorage(0):
        model(batch)      # (routes, packed operands and range words settle in a first pass)
    for p in model.parameters():
        p.grad = None
    torch.cuda.synchronize()
    real, reads = Kn.range_summary, []

    def summary(device):      # the last thing queued before the step's one read: sync-debug goes back to "default" here
        out = real(device)
        torch.cuda.set_sync_debug_mode("default")
        reads.append(1)
        return out

    monkeypatch.setattr(Kn, "range_summary", summary)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with EventStorage(0) as storage:
            losses = model(batch)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    monkeypatch.setattr(Kn, "range_summary", real)
    assert reads == [1], reads
    sum(losses.values()).backward()
    _check_step(g, model, losses, _latest(storage), "deferred")


def test_mask_training_step_under_loss_scaler(monkeypatch, step_model):
    from lvc_amd.solver import LossScaler
    from lvc_amd.utils.events import EventStorage

    g = gold("mask_train")
    model = step_model
    params = [p for p in model.parameters() if p.requires_grad]
    for p in params:
        p.grad = None
    _identity_randperm(monkeypatch)
    scaler = LossScaler(init_scale=2.0 ** 10)
    with EventStorage(0) as storage:
        losses = model(_step_batch(g))
        scaler.backward(sum(losses.values()))
    assert scaler.step(torch.optim.SGD(params, lr=0.0)) is True
    _check_step(g, model, losses, _latest(storage), "loss_scaler")


def test_mask_targets_of_the_step_are_the_references(step_model):
    """The recorded foreground rows through the model's own batched helper inputs: targets equal outside the fixture's band."""
    from lvc_amd import kernels as K

    g = gold("mask_train")
    dev = _dev()
    n = [len(g["fg_classes%d" % i]) for i in range(2)]
    R_ = max(n)
    boxes = torch.zeros(2, R_, 4)
    matched = torch.zeros(2, R_, dtype=torch.int64)
    for i in range(2):
        boxes[i, : n[i]] = g["fg_boxes%d" % i]
        matched[i, : n[i]] = g["fg_matched%d" % i].long()
    got = K.mask_targets(boxes.to(dev), matched.to(dev), torch.tensor(n, dtype=torch.int32, device=dev), [_gt_masks(g, i).to(dev) for i in range(2)], 28).cpu()
    aside = total = 0
    for i in range(2):
        want = torch.from_numpy(np.unpackbits(g["targets%d" % i].numpy())[: n[i] * 784].reshape(n[i], 28, 28)).bool()
        band = torch.from_numpy(np.unpackbits(g["band%d" % i].numpy())[: n[i] * 784].reshape(n[i], 28, 28)).bool()
        mine = got[i * R_: i * R_ + n[i]] != 0
        assert not bool(((mine != want) & ~band).any())
        aside += int(band.sum())
        total += band.numel()
    assert aside <= 1e-3 * total and float(g["band_share"]) <= 1e-3


def test_per_image_path_gives_the_same_loss_mask(monkeypatch, step_model):
    from lvc_amd.modeling.meta_arch.rcnn import GeneralizedRCNN
    from lvc_amd.utils.events import EventStorage

    g = gold("mask_train")
    _identity_randperm(monkeypatch)
    res = {}
    for fast in (True, False):
        monkeypatch.setattr(GeneralizedRCNN, "deferred_reads", fast)
        with EventStorage(0) as st:
            losses = step_model(_step_batch(g))
            res[fast] = ({k: float(v.detach()) for k, v in losses.items()}, _latest(st))
    print(res)
    assert set(res[True][0]) == set(res[False][0]) == set(LOSSES)
    assert res[True][0]["loss_mask"] == res[False][0]["loss_mask"]
    for k in LOSSES:
        assert abs(res[True][0][k] - res[False][0][k]) <= 2e-6 * max(1.0, abs(res[False][0][k])), k
    for k in ("mask_rcnn/accuracy", "mask_rcnn/false_positive", "mask_rcnn/false_negative"):
        assert res[True][1][k] == res[False][1][k], k


def test_sampled_instances_carry_no_full_size_planes(monkeypatch, step_model):
    """The per-image sampler of a mask model keeps the matched index, not gathered planes; a non-BitMasks gt_masks is refused by key."""
    from lvc_amd.modeling.meta_arch.rcnn import GeneralizedRCNN
    from lvc_amd.utils.events import EventStorage

    g = gold("mask_train")
    _identity_randperm(monkeypatch)
    monkeypatch.setattr(GeneralizedRCNN, "deferred_reads", False)
    seen = []
    orig = type(step_model.roi_heads)._branch_loss_batched

    def spy(self, name, feats, s_boxes, s_cls, s_m, fg_count, gt_masks, status):
        assert name == "mask"
        seen.append((s_boxes.shape, [tuple(getattr(m, "tensor", m).shape) for m in gt_masks]))
        return orig(self, name, feats, s_boxes, s_cls, s_m, fg_count, gt_masks, status)

    monkeypatch.setattr(type(step_model.roi_heads), "_branch_loss_batched", spy)
    heads = step_model.roi_heads
    sample = heads.label_and_sample_proposals
    for batched in (True, False):      # the one-read sampler and the per-image loop
        sampled = []

        def spy_sampler(proposals, targets, *a, **kw):
            out = sample(proposals, targets, *a, **kw)
            sampled.append((out, targets))
            return out

        monkeypatch.setattr(heads, "label_and_sample_proposals", spy_sampler)
        monkeypatch.setattr(type(heads), "batched_sampling", batched)
        with EventStorage(0):
            step_model(_step_batch(g))
        assert len(sampled) == 1
        for inst, tgt in zip(*sampled[0]):
            assert tgt.has("gt_masks") and not inst.has("gt_masks"), "a sampled Instances carries gathered full-size planes"
            assert inst.has("gt_boxes") and inst.has("gt_classes") and len(inst) == BATCH_SIZE_PER_IMAGE
            matched = inst._lvc_matched
            assert matched.shape == (len(inst),) and matched.dtype == torch.int64
            assert torch.equal(tgt.gt_boxes.tensor[matched], inst.gt_boxes.tensor)
    assert len(seen) == 2 and seen[0][1] == [(3, 128, 160), (4, 120, 176)]
    bad = _step_batch(g)
    bad[0]["instances"].gt_masks = _gt_masks(g, 0)          # a plain tensor, as a polygon-format loader might hand over
    with EventStorage(0), pytest.raises(NotImplementedError, match="INPUT.MASK_FORMAT"):
        step_model(bad)


def test_box_only_model_gives_the_mask_models_box_and_rpn_losses(monkeypatch, step_model):
    """MODEL.MASK_ON False on the same batch: the box and RPN losses are bit-equal to the mask model's (the mask branch adds a loss and
    changes nothing else), there is no loss_mask, and ground-truth masks in the batch are ignored."""
    from lvc_amd.utils.events import EventStorage

    g = gold("mask_train")
    _identity_randperm(monkeypatch)
    base = _mask_model(mask_on=False)
    with EventStorage(0):
        a = base(_step_batch(g, masks=False))
        b = step_model(_step_batch(g))
    assert set(a) == set(LOSSES) - {"loss_mask"}
    for k in a:
        assert torch.equal(a[k].detach(), b[k].detach()), (k, float(a[k]), float(b[k]))


def test_step_with_an_image_without_ground_truth(step_model):
    """An image without ground truth has background rows only: it adds no mask row, the step goes through the per-image path and the
    mask loss is that of the other image's rows."""
    from lvc_amd.structures import BitMasks, Boxes
    from lvc_amd.utils.events import EventStorage

    g = gold("mask_train")
    batch = _step_batch(g)
    h, w, _ = _SIZES[1]
    inst = batch[1]["instances"]
    inst = type(inst)((h, w))
    inst.gt_boxes = Boxes(torch.zeros(0, 4))
    inst.gt_classes = torch.zeros(0, dtype=torch.int64)
    inst.gt_masks = BitMasks(torch.zeros(0, h, w, dtype=torch.bool))
    batch[1]["instances"] = inst
    for p in step_model.parameters():
        p.grad = None
    with EventStorage(0) as storage:
        losses = step_model(batch)
        sum(losses.values()).backward()
    assert set(losses) == set(LOSSES) and all(bool(torch.isfinite(v)) for v in losses.values())
    assert float(losses["loss_mask"]) > 0 and 0.0 <= _latest(storage)["mask_rcnn/accuracy"] <= 1.0
    grad = step_model.roi_heads.mask_head.deconv.weight.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0


def test_box_only_step_gives_the_parent_commits_bits(monkeypatch):
    """MODEL.MASK_ON False on the fixture's batch against what the commit before the mask branch's training computed on an MI355X
    (tests/golden/mask_train_parent_box.npz: that tree's box-only step -- 20 classes, 128 rows per image, identity randperm, the
    fixture's boxes and classes): the four losses and the bias gradients of the box predictor bit for bit.  The bias gradients of the
    RPN head's three convs are held to 1e-6 of their largest entry instead: that tree did not reproduce them between its own runs (a conv's
    bias gradient is a column sum that joins slabs with float atomics; five runs gave values one ulp apart in single elements of
    `objectness_logits.bias` and `conv.bias`)."""
    from lvc_amd.utils.events import EventStorage

    g, want = gold("mask_train"), gold("mask_train_parent_box")
    _identity_randperm(monkeypatch)
    base = _mask_model(mask_on=False)
    with EventStorage(0):
        losses = base(_step_batch(g, masks=False))
        sum(losses.values()).backward()
    assert set(losses) == set(LOSSES) - {"loss_mask"}
    for k, v in losses.items():
        assert torch.equal(v.detach().cpu().reshape(1), want["loss." + k]), (k, float(v), float(want["loss." + k]))
    grads = {n: p.grad.cpu() for n, p in base.named_parameters() if p.grad is not None}
    names = [k[len("bias_grad."):] for k in want if k.startswith("bias_grad.")]
    assert len(names) == 5
    for n in names:
        ref = want["bias_grad." + n]
        if "rpn_head" in n:
            assert float((grads[n] - ref).abs().max()) <= 1e-6 * float(ref.abs().max()), n
        else:
            assert torch.equal(grads[n], ref), n
