"""Keypoint R-CNN training on the device: lvc_keypoint_loss, lvc_keypoint_loss_grad, lvc_keypoint_deconv_dx and lvc_keypoint_deconv_wgrad
(csrc/keypoint_train.hip) against tests/keypoint_train_ref.py in fp64, each bar 3 x what an fp32 torch-CPU run of the same expression
deviates from fp64 on the same input; then a whole training step of a keypoint model against the reference's own recorded step
(tests/golden/keypoint_train.npz).  Every ratio goes to profiles/keypoint_train_parity.json (LVC_KEYPOINT_TRAIN_PARITY_OUT: another path)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import keypoint_train_ref as R
from helpers import ROOT, gold

pytestmark = pytest.mark.gpu

_PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def write_parity():
    yield
    if not _PARITY:
        return
    path = os.environ.get("LVC_KEYPOINT_TRAIN_PARITY_OUT") or os.path.join(ROOT, "profiles", "keypoint_train_parity.json")
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
# name -> ((M, S, Cin, K), options): num_valid (rows past it hold NaN; it falls in the middle of a 64-row tile of M S^2), upstream
# scalar g, fixed normaliser (None: the valid entries), LOSS_WEIGHT
CASES = {
    "1x3": ((1, 3, 16, 3), dict()),                                       # every pixel of the odd map is a border
    "5x3-k17-fixed": ((5, 3, 48, 17), dict(fixed=37.0, weight=0.7)),      # K pads to 20: a contraction that is no multiple of 16
    "5x14-g1024": ((5, 14, 16, 3), dict(g=1024.0)),
    "9x14-k17-nv": ((9, 14, 48, 17), dict(num_valid=6)),                  # 6 * 196 = 18 * 64 + 24 rows
    "70x3-k17-nv": ((70, 3, 48, 17), dict(num_valid=41, weight=2.0)),     # 41 * 9 = 5 * 64 + 49 rows
}
_REF = {}


def _operands(name):
    from lvc_amd.utils import synthetic as syn

    (M, S, cin, K), opt = CASES[name]
    x, w, b, _boxes = syn.keypoint_head_case(M, S, cin, K)
    g = torch.Generator().manual_seed(977 + 31 * M + S + K)
    target = torch.randint(0, 16 * S * S, (M, K), generator=g)
    valid = torch.rand(M, K, generator=g) < 0.7
    valid.view(-1)[0] = True
    if M > 2:
        valid[1] = False          # a row that was not selected
    # the corners and an edge of the map among the targets
    corners = torch.tensor([0, 4 * S - 1, 16 * S * S - 4 * S, 16 * S * S - 1, 2 * S])
    target.view(-1)[: min(5, M * K)] = corners[: min(5, M * K)]
    target = target * valid.long()
    nv = opt.get("num_valid", M)
    if nv < M:
        x = x.clone()
        x[nv:] = float("nan")
    return (x, w, b), target, valid, nv, float(opt.get("g", 1.0)), opt.get("fixed"), float(opt.get("weight", 1.0))


def _torch_autograd(ops, target, valid, nv, g, fixed, weight, dtype):
    """torch's own operators and autograd on the CPU on the first nv rows -> (low, terms [nv, K], loss, gradients)."""
    x, w, b = ops
    ps = [x[:nv].to(dtype).clone().requires_grad_(), w.to(dtype).clone().requires_grad_(), b.to(dtype).clone().requires_grad_()]
    K = w.shape[1]
    low = F.conv_transpose2d(ps[0], ps[1], ps[2], stride=2, padding=1)
    low.retain_grad()
    z = F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=False)
    v = valid[:nv].reshape(-1)
    terms = F.cross_entropy(z.view(nv * K, -1), target[:nv].reshape(-1), reduction="none") * v.to(dtype)
    n = float(v.sum())
    loss = terms.sum() / (n if fixed is None else fixed) * weight if n else terms.sum() * 0
    (loss * g).backward()
    dx = torch.zeros(x.shape, dtype=dtype)
    dx[:nv] = ps[0].grad
    return low.detach(), terms.detach().view(nv, K), loss.detach(), {"dlow": low.grad, "dx": dx, "dW": ps[1].grad, "db": ps[2].grad}


def _reference(name):
    """The fp64 restatement and torch's fp32 deviation from it, computed once per case and shared."""
    if name in _REF:
        return _REF[name]
    ops, target, valid, nv, g, fixed, weight = _operands(name)
    x, w, b = ops
    exact = R.grads(x[:nv].double(), w.double(), b.double(), target[:nv], valid[:nv], fixed=fixed, weight=weight, upstream=g)
    dx = torch.zeros(x.shape, dtype=torch.float64)
    dx[:nv] = exact["dx"]
    exact["dx"] = dx
    low32, terms32, loss32, g32 = _torch_autograd(ops, target, valid, nv, g, fixed, weight, torch.float32)
    noise = {k: float((g32[k].double() - exact[k]).abs().max()) for k in ("dlow", "dx", "dW", "db")}
    noise["low"] = float((low32.double() - exact["low"]).abs().max())
    noise["terms"] = float((terms32.double() - exact["terms"]).abs().max())
    _REF[name] = (ops, target, valid, nv, g, fixed, weight, exact, noise)
    return _REF[name]


SENTINEL = -7.5


def _run(name, bad_target=None):
    """-> dict of the kernels' results on the case (CPU tensors).  Every output starts as SENTINEL (low: NaN)."""
    from lvc_amd import kernels as K

    ops, target, valid, nv, g, fixed, weight = _reference(name)[:7]
    x, w, b = ops
    dev = _dev()
    M, cin, S, _ = x.shape
    k = w.shape[1]
    kc = K.keypoint_dlow_channels(k)
    xn = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd = w.to(dev)
    num_valid = None if nv == M else torch.tensor([nv], dtype=torch.int32, device=dev)
    status = K.new_status(dev)
    low = torch.full((M, k, 2 * S, 2 * S), float("nan"), device=dev)
    K.keypoint_deconv(xn, K.pack_keypoint_deconv(wd), b.to(dev), k, num_valid=num_valid, out=low)
    tg = target.to(torch.int32).to(dev)
    if bad_target is not None:
        tg = tg.clone()
        tg.view(-1)[bad_target] = 16 * S * S
    vd = valid.to(torch.uint8).to(dev)
    outs = (torch.full((M, k), SENTINEL, dtype=torch.float64, device=dev), torch.full((M, k), SENTINEL, dtype=torch.float32, device=dev),
            torch.full((M, k), SENTINEL, dtype=torch.float64, device=dev))
    loss, total, count, term, pmax, plse = K.keypoint_loss(low, tg, vd, num_valid=num_valid, normalizer=fixed, loss_weight=weight,
                                                           status=status, out=outs)
    up = torch.tensor([g], dtype=torch.float32, device=dev)
    dlow = K.keypoint_loss_grad(low, tg, vd, pmax, plse, count, up, num_valid=num_valid, normalizer=fixed, loss_weight=weight,
                                out=torch.full((M, 2 * S, 2 * S, kc), SENTINEL, device=dev))
    dx = K.keypoint_deconv_dx(dlow, K.pack_keypoint_deconv_dx(wd), k, num_valid=num_valid, out=torch.full((M, S, S, cin), SENTINEL, device=dev))
    dW, db = K.keypoint_deconv_wgrad(xn, dlow, k, num_valid=num_valid)
    torch.cuda.synchronize()
    return {"low": low.cpu(), "loss": loss.cpu(), "sum": total.cpu(), "count": count.cpu(), "term": term.cpu(), "pmax": pmax.cpu(),
            "plse": plse.cpu(), "status": int(status.item()), "dlow_raw": dlow.cpu(), "dlow": dlow[..., :k].permute(0, 3, 1, 2).cpu(),
            "dx": dx.permute(0, 3, 1, 2).cpu(), "dW": dW.cpu(), "db": db.cpu()}


_OUT = {}


def _out(name):
    if name not in _OUT:
        _OUT[name] = _run(name)
    return _OUT[name]


def _finite(t):
    return bool(torch.isfinite(t).all())


@pytest.mark.parametrize("name", list(CASES))
def test_terms_and_loss(name):
    ops, target, valid, nv, g, fixed, weight, exact, noise = _reference(name)
    o = _out(name)
    assert o["status"] == 0
    low = o["low"][:nv]
    err = float((low.double() - exact["low"]).abs().max())
    assert err <= _record("low/%s" % name, err, noise["low"]), name
    v = valid[:nv]
    # the formula in fp64, and in fp32, on the kernel's own planes
    t64, _ = R.loss_terms(low.double(), target[:nv], v)
    t32, _ = R.loss_terms(low.float(), target[:nv], v)
    got = o["term"][:nv]
    assert torch.equal(got[~v], torch.full_like(got[~v], SENTINEL)), "an invalid entry's term was written"
    err = float((got - t64)[v].abs().max())
    assert err <= _record("terms_own/%s" % name, err, float((t32.double() - t64)[v].abs().max())), name
    err = float((got - exact["terms"])[v].abs().max())
    assert err <= _record("terms/%s" % name, err, noise["terms"]), name
    # pmax + plse is the plane's logsumexp
    z = R.upsample(low.double()).flatten(2)
    assert float((o["pmax"][:nv].double() + o["plse"][:nv] - torch.logsumexp(z, 2))[v].abs().max()) <= 1e-5
    own = float(got[v].sum())
    rel = abs(float(o["sum"]) - own) / abs(own)
    _PARITY["loss_sum/%s" % name] = {"relative": rel, "bar": 1e-12}
    print("loss_sum/%s relative %.3e" % (name, rel))
    assert rel <= 1e-12, (name, rel)
    assert int(o["count"]) == int(v.sum())
    n = float(v.sum()) if fixed is None else fixed
    mean64 = float(t64.sum()) / n * weight
    mean32 = float((t32.sum() / n * weight).float())
    err = abs(float(o["loss"].double()) - mean64)
    assert err <= _record("loss/%s" % name, err, abs(mean32 - mean64)), (name, float(o["loss"]), mean64)


@pytest.mark.parametrize("name", list(CASES))
def test_gradients(name):
    ops, target, valid, nv, g, fixed, weight, exact, noise = _reference(name)
    o = _out(name)
    bad = {}
    for key in ("dlow", "dx", "dW", "db"):
        got = o[key][:nv] if key == "dlow" else o[key]
        ref = exact[key]
        if key == "dx":
            got, ref = got[:nv], ref[:nv]
        assert _finite(got), key
        err = float((got.double() - ref).abs().max())
        bar = _record("%s/%s" % (key, name), err, noise[key])
        if err > bar:
            bad[key] = (err, bar)
    assert not bad, (name, bad)
    k = ops[1].shape[1]
    assert not bool(o["dlow_raw"][:nv][..., k:].any()), "the padding channels of dlow are not zero"
    inv = ~valid[:nv]
    assert not bool(o["dlow"][:nv][inv].any()), "an invalid entry's plane is not zero"


@pytest.mark.parametrize("name", ["9x14-k17-nv", "70x3-k17-nv"])
def test_rows_past_num_valid_keep_their_bytes(name):
    nv = _reference(name)[3]
    o = _out(name)
    assert bool(torch.isnan(o["low"][nv:]).all())
    for key in ("term", "pmax", "plse", "dlow_raw", "dx"):
        rest = o[key][nv:]
        assert rest.numel() and torch.equal(rest, torch.full_like(rest, SENTINEL)), key
    assert _finite(o["dW"]) and _finite(o["db"]) and _finite(o["loss"])      # the NaN rows of x were not read


@pytest.mark.parametrize("name", ["5x3-k17-fixed", "9x14-k17-nv", "70x3-k17-nv"])
def test_two_runs_give_the_same_bits(name):
    a, b = _out(name), _run(name)
    for key in ("loss", "sum", "count", "term", "pmax", "plse", "dlow_raw", "dx", "dW", "db"):
        assert torch.equal(a[key], b[key]), key
    nv = _reference(name)[3]
    assert torch.equal(a["low"][:nv], b["low"][:nv])


def test_a_target_out_of_range_sets_the_status_bit_and_is_skipped():
    from lvc_amd import kernels as K

    name = "5x3-k17-fixed"          # the fixed normaliser: skipping an entry changes no other entry's scale
    ops, target, valid, nv = _reference(name)[:4]
    e = int(valid.view(-1).nonzero()[3])
    a, b = _out(name), _run(name, bad_target=e)
    assert a["status"] == 0 and b["status"] & K.KEYPOINT_BAD_TARGET and K.KEYPOINT_BAD_TARGET != K.MASK_BAD_CLASS
    keep = torch.ones(valid.numel(), dtype=torch.bool)
    keep[e] = False
    for key in ("term", "pmax", "plse"):
        assert torch.equal(a[key].view(-1)[keep], b[key].view(-1)[keep]), key
        assert float(b[key].view(-1)[e]) == SENTINEL
    assert int(b["count"]) == int(a["count"]) - 1
    assert abs(float(b["sum"]) - (float(a["sum"]) - float(a["term"].view(-1)[e]))) <= 1e-12 * abs(float(a["sum"]))
    k = ops[1].shape[1]
    da, db_ = a["dlow"].reshape(valid.numel(), -1), b["dlow"].reshape(valid.numel(), -1)
    assert torch.equal(da[keep], db_[keep]) and not bool(db_[e].any()) and bool(da[e].any())
    assert _finite(b["dx"]) and _finite(b["dW"]) and _finite(b["loss"]) and k == 17


def _tail_apply(x, w, b, target, valid, num_valid=None, normalizer=None, weight=1.0, g=1.0, status=None):
    from lvc_amd.modeling.roi_heads.keypoint_head import KeypointTailLoss

    loss, total, count = KeypointTailLoss.apply(x, w, b, target, valid, num_valid, status, normalizer, weight, None, None)
    (loss * torch.tensor(g, device=x.device)).backward()
    return loss, total, count


def test_nothing_valid_and_no_rows_give_exact_zeros():
    dev = _dev()
    ops, target, valid = _reference("5x3-k17-fixed")[:3]
    x, w, b = ops
    for rows, fixed in ((5, None), (5, 37.0), (0, None)):
        ps = [x[:rows].permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(), w.to(dev).requires_grad_(), b.to(dev).requires_grad_()]
        tg = target[:rows].to(torch.int32).to(dev)
        loss, total, count = _tail_apply(*ps, tg, torch.zeros(rows, 17, dtype=torch.uint8, device=dev), normalizer=fixed)
        assert float(loss.detach()) == 0.0 and float(total) == 0.0 and int(count) == 0
        for p in ps:
            assert p.grad is not None and p.grad.shape == p.shape and not bool(p.grad.any()) and _finite(p.grad)
    # num_valid = 0 with NaN rows: nothing is read
    ps = [torch.full((3, 3, 3, 48), float("nan"), device=dev).requires_grad_(), w.to(dev).requires_grad_(), b.to(dev).requires_grad_()]
    loss, _t, count = _tail_apply(*ps, target[:3].to(torch.int32).to(dev), valid[:3].to(torch.uint8).to(dev),
                                  num_valid=torch.zeros(1, dtype=torch.int32, device=dev))
    assert float(loss.detach()) == 0.0 and int(count) == 0
    for p in ps:
        assert not bool(p.grad.any()) and _finite(p.grad)


def test_autograd_function_is_the_kernels(monkeypatch):
    """`KeypointTailLoss` (what the head's training forward is built on): the same loss and gradients through torch's autograd, with the
    upstream scalar a device tensor; an input that needs no gradient costs no launch."""
    from lvc_amd import kernels as K

    name = "9x14-k17-nv"
    ops, target, valid, nv, g, fixed, weight = _reference(name)[:7]
    o = _out(name)
    x, w, b = ops
    dev = _dev()
    calls = []
    real_dx, real_dw = K.keypoint_deconv_dx, K.keypoint_deconv_wgrad
    monkeypatch.setattr(K, "keypoint_deconv_dx", lambda *a, **k: (calls.append("dx"), real_dx(*a, **k))[1])
    monkeypatch.setattr(K, "keypoint_deconv_wgrad", lambda *a, **k: (calls.append("dw"), real_dw(*a, **k))[1])

    def operands(need_x, need_w):
        return [x.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(need_x), w.to(dev).requires_grad_(need_w), b.to(dev).requires_grad_(need_w)]

    tg, vd = target.to(torch.int32).to(dev), valid.to(torch.uint8).to(dev)
    num_valid = torch.tensor([nv], dtype=torch.int32, device=dev)
    ps = operands(True, True)
    loss, total, count = _tail_apply(*ps, tg, vd, num_valid=num_valid, normalizer=fixed, weight=weight, g=g)
    assert calls == ["dx", "dw"]
    assert loss.dim() == 0 and torch.equal(loss.detach().cpu().view(1), o["loss"]) and torch.equal(count.cpu(), o["count"])
    assert torch.equal(total.cpu(), o["sum"])
    assert torch.equal(ps[0].grad.permute(0, 3, 1, 2).cpu()[:nv], o["dx"][:nv]) and not bool(ps[0].grad[nv:].any())
    assert torch.equal(ps[1].grad.cpu(), o["dW"]) and torch.equal(ps[2].grad.cpu(), o["db"])
    del calls[:]
    ps = operands(False, True)
    _tail_apply(*ps, tg, vd, num_valid=num_valid, normalizer=fixed, weight=weight, g=g)
    assert calls == ["dw"] and ps[0].grad is None and torch.equal(ps[1].grad.cpu(), o["dW"])
    del calls[:]
    ps = operands(True, False)
    _tail_apply(*ps, tg, vd, num_valid=num_valid, normalizer=fixed, weight=weight, g=g)
    assert calls == ["dx"] and ps[1].grad is None and ps[2].grad is None
    assert torch.equal(ps[0].grad.permute(0, 3, 1, 2).cpu()[:nv], o["dx"][:nv])


# ------------------------------------------------------------------ the model step
_SIZES = ((128, 160, 3), (120, 176, 4))
BATCH_SIZE_PER_IMAGE = 128          # as scripts/make_golden_keypoint_train.py
BOX_LOSSES = ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc")
LOSSES = BOX_LOSSES + ("loss_keypoint",)
ZERO_SUM_GRAD = "roi_heads.keypoint_head.score_lowres.bias"


def _identity_randperm(monkeypatch):
    monkeypatch.setattr(torch, "randperm", lambda n, **kw: torch.arange(n, **{k: v for k, v in kw.items() if k in ("device", "dtype")}))


def _keypoint_model(keypoint_on=True, enable=True):
    from lvc_amd.config.presets import base_rcnn_fpn, keypoint_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    cfg = (keypoint_rcnn_fpn if keypoint_on else base_rcnn_fpn)(num_classes=1)
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = BATCH_SIZE_PER_IMAGE
    m = build_model(cfg)
    m = syn.conditioned_keypoint_head_(m) if keypoint_on else syn.conditioned_r50_fpn_(m)
    m.train()
    return m.enable_keypoint_training() if keypoint_on and enable else m


def _step_batch(g, keypoints=True, device=None, hide=False):
    from lvc_amd.structures import Boxes, Instances, Keypoints
    from lvc_amd.utils import synthetic as syn

    batch = []
    for i, (h, w, seed) in enumerate(_SIZES):
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(g["gt_boxes%d" % i])
        inst.gt_classes = g["gt_classes%d" % i]
        if keypoints:
            kp = g["gt_keypoints%d" % i].clone()
            if hide:
                kp[:, :, 2] = 0
            inst.gt_keypoints = Keypoints(kp)
        image = syn.synthetic_image(seed, h, w)
        if device is not None:
            inst, image = inst.to(device), image.to(device)
        batch.append({"image": image, "instances": inst, "height": h, "width": w})
    return batch


def _latest(storage):
    return {k: (v[0] if isinstance(v, tuple) else v) for k, v in storage.latest().items()}


def _check_step(g, model, losses, scalars, tag):
    """The bars of train_base.npz, as test_mask_training_step_matches_reference uses them: losses within 2e-4 relative, every
    trainable gradient with cosine >= 0.998 and norm error <= 1e-2 -- but for the one gradient that is analytically zero (see
    ZERO_SUM_GRAD below), which is held to the rounding bound of its sum instead."""
    assert set(losses) == set(LOSSES)
    for k in LOSSES:
        ref, got = float(g["loss." + k]), float(losses[k].detach())
        _PARITY["step/%s/%s" % (tag, k)] = {"ours": got, "reference": ref, "relative": abs(got - ref) / max(1.0, abs(ref)),
                                            "reference_fp32_vs_fp64": float(g["loss_dev." + k])}
        print("%-14s ours %.7f  reference %.7f (its own fp32-vs-fp64 deviation %.2e)" % (k, got, ref, float(g["loss_dev." + k])))
        assert abs(got - ref) <= 2e-4 * max(1.0, abs(ref)), k
    if scalars is not None:
        for name in ("rpn/num_pos_anchors", "roi_head/num_fg_samples", "roi_head/num_bg_samples", "keypoint_head/num_fg_samples"):
            assert scalars[name] == float(g["scalar." + name.replace("/", ".")]), name
        assert "kpts_num_skipped_batches" not in scalars
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
        if name == ZERO_SUM_GRAD:
            # d loss / d score_lowres.bias[k] = sum of dlow[:, k]: analytically 0 -- a valid entry's softmax - onehot sums to 0 and the
            # x2 adjoint's weights keep sums -- so what either side holds is the residue of its own roundings, and a cosine between two
            # residues says nothing.  The bound is the format's: sum |dlow[:, k]| <= 2 (each of the n valid entries carries at most 2 / n),
            # every element is rounded to fp32 once (relative 2^-24) and the sum itself is formed in fp64: |db[k]| <= 2^-23.  The
            # reference's recorded residue obeys it too.
            ours, theirs = float(gflat.abs().max()), float(ref.abs().max())
            print("%-52s |residue| ours %.3e  reference %.3e  bound %.3e" % (name, ours, theirs, 2.0 ** -23))
            _PARITY["step/%s/grad/%s" % (tag, name)] = {"ours_max": ours, "reference_max": theirs, "bound": 2.0 ** -23}
            assert ours <= 2.0 ** -23 and theirs <= 2.0 ** -23, name
            continue
        cos = float((sample * ref).sum() / (sample.norm() * ref.norm()).clamp_min(1e-30))
        nerr = abs(float(gflat.double().norm()) - nrm) / max(nrm, 1e-12)
        if "keypoint_head" in name:
            print("%-52s cos %.6f  norm err %.2e" % (name, cos, nerr))
            _PARITY["step/%s/grad/%s" % (tag, name)] = {"cosine": cos, "norm_error": nerr}
        if not (cos >= 0.998 and nerr <= 1e-2):
            bad[name] = (cos, nerr)
    assert not bad, bad


@pytest.fixture(scope="module")
def step_model():
    return _keypoint_model()


def test_keypoint_training_step_matches_reference(monkeypatch, step_model):
    """One step of the reference's Keypoint R-CNN (tests/golden/keypoint_train.npz) on the deferred path, which must make exactly one
    device->host read."""
    from lvc_amd import kernels as Kn
    from lvc_amd.utils.events import EventStorage

    g = gold("keypoint_train")
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


def test_keypoint_training_step_on_the_per_image_path(monkeypatch, step_model):
    from lvc_amd.modeling.meta_arch.rcnn import GeneralizedRCNN
    from lvc_amd.utils.events import EventStorage

    g = gold("keypoint_train")
    _identity_randperm(monkeypatch)
    monkeypatch.setattr(GeneralizedRCNN, "deferred_reads", False)
    for p in step_model.parameters():
        p.grad = None
    with EventStorage(0) as storage:
        losses = step_model(_step_batch(g))
        sum(losses.values()).backward()
    _check_step(g, step_model, losses, _latest(storage), "per_image")


def test_keypoint_training_step_under_loss_scaler(monkeypatch, step_model):
    from lvc_amd.solver import LossScaler
    from lvc_amd.utils.events import EventStorage

    g = gold("keypoint_train")
    params = [p for p in step_model.parameters() if p.requires_grad]
    for p in params:
        p.grad = None
    _identity_randperm(monkeypatch)
    scaler = LossScaler(init_scale=2.0 ** 10)
    with EventStorage(0) as storage:
        losses = step_model(_step_batch(g))
        scaler.backward(sum(losses.values()))
    assert scaler.step(torch.optim.SGD(params, lr=0.0)) is True
    _check_step(g, step_model, losses, _latest(storage), "loss_scaler")


def test_targets_and_logits_of_the_step(monkeypatch, step_model):
    """The step's targets are the reference's exactly, and the planes its loss reads are bit-equal to `head.lowres_nhwc` in eval mode
    on the same pooled rows."""
    from lvc_amd import kernels as K
    from lvc_amd.utils.events import EventStorage

    g = gold("keypoint_train")
    _identity_randperm(monkeypatch)
    seen = {}
    real_t, real_l = K.keypoint_targets, K.keypoint_loss
    head = step_model.roi_heads.keypoint_head
    real_loss_nhwc = head.loss_nhwc

    def targets(*a, **k):
        seen["targets"] = real_t(*a, **k)
        return seen["targets"]

    def loss(low, *a, **k):
        seen["low"], seen["num_valid"] = low.clone(), k.get("num_valid")
        return real_l(low, *a, **k)

    def loss_nhwc(pooled, *a, **k):
        seen["pooled"] = pooled.detach().clone()
        return real_loss_nhwc(pooled, *a, **k)

    monkeypatch.setattr(K, "keypoint_targets", targets)
    monkeypatch.setattr(K, "keypoint_loss", loss)
    monkeypatch.setattr(head, "loss_nhwc", loss_nhwc)
    with EventStorage(0):
        step_model(_step_batch(g))
    target, valid, selected, sel = [t.cpu() for t in seen["targets"]]
    R_ = target.shape[0] // 2
    assert R_ == 32          # int(128 * 0.25) foreground rows at most
    for i in range(2):
        n = len(g["fg_matched%d" % i])
        keep = g["selected%d" % i].bool()
        rows = slice(i * R_, i * R_ + n)
        want_v = g["valid%d" % i].bool() & keep[:, None]
        assert torch.equal(selected[rows].bool(), keep) and int(sel[i]) == int(keep.sum())
        assert torch.equal(valid[rows].bool(), want_v)
        assert torch.equal(target[rows].long(), g["targets%d" % i].long() * want_v.long())
        assert not bool(valid[i * R_ + n: (i + 1) * R_].any())
    total = int(seen["num_valid"])
    assert total == sum(len(g["fg_matched%d" % i]) for i in range(2))
    head.eval()
    try:
        with torch.no_grad():
            low = head.lowres_nhwc(seen["pooled"], num_valid=seen["num_valid"])
    finally:
        head.train()
    assert torch.equal(low[:total], seen["low"][:total])


def test_step_with_an_image_without_ground_truth(step_model):
    from lvc_amd.structures import Boxes
    from lvc_amd.utils.events import EventStorage

    g = gold("keypoint_train")
    for with_field in (True, False):
        batch = _step_batch(g)
        h, w, _ = _SIZES[1]
        inst = type(batch[1]["instances"])((h, w))
        inst.gt_boxes = Boxes(torch.zeros(0, 4))
        inst.gt_classes = torch.zeros(0, dtype=torch.int64)
        if with_field:
            inst.gt_keypoints = batch[1]["instances"].gt_keypoints[:0]
        batch[1]["instances"] = inst
        for p in step_model.parameters():
            p.grad = None
        with EventStorage(0) as storage:
            losses = step_model(batch)
            sum(losses.values()).backward()
        assert set(losses) == set(LOSSES) and all(bool(torch.isfinite(v)) for v in losses.values())
        assert float(losses["loss_keypoint"].detach()) > 0
        # the image without foreground rows does not enter the mean
        assert _latest(storage)["keypoint_head/num_fg_samples"] == float(g["selected0"].sum())
        grad = step_model.roi_heads.keypoint_head.score_lowres.weight.grad
        assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    bad = _step_batch(g)
    bad[0]["instances"].remove("gt_keypoints")
    with EventStorage(0), pytest.raises(ValueError, match="gt_keypoints"):
        step_model(bad)


def test_step_without_a_visible_keypoint(monkeypatch, step_model):
    """Every v = 0: loss_keypoint is exactly 0 with exactly zero gradients in the keypoint head, kpts_num_skipped_batches is logged on
    both read paths, and the box and RPN losses are those of the ordinary step."""
    from lvc_amd.modeling.meta_arch.rcnn import GeneralizedRCNN
    from lvc_amd.modeling.roi_heads import keypoint_head as kh
    from lvc_amd.utils.events import EventStorage

    g = gold("keypoint_train")
    _identity_randperm(monkeypatch)
    with EventStorage(0):
        ordinary = step_model(_step_batch(g))
    for fast in (True, False):
        monkeypatch.setattr(GeneralizedRCNN, "deferred_reads", fast)
        for p in step_model.parameters():
            p.grad = None
        before = kh._TOTAL_SKIPPED
        with EventStorage(0) as storage:
            losses = step_model(_step_batch(g, hide=True))
            sum(losses.values()).backward()
        assert float(losses["loss_keypoint"].detach()) == 0.0
        assert kh._TOTAL_SKIPPED == before + 1 and _latest(storage)["kpts_num_skipped_batches"] == before + 1
        assert _latest(storage)["keypoint_head/num_fg_samples"] == 0.0
        for name, p in step_model.roi_heads.keypoint_head.named_parameters():
            assert p.grad is not None and not bool(p.grad.any()) and bool(torch.isfinite(p.grad).all()), name
        for k in BOX_LOSSES:
            assert abs(float(losses[k]) - float(ordinary[k])) <= 2e-6 * max(1.0, abs(float(ordinary[k]))), k


def test_box_only_model_gives_the_keypoint_models_box_and_rpn_losses(monkeypatch, step_model):
    """MODEL.KEYPOINT_ON False on the same batch: the box and RPN losses are bit-equal to the keypoint model's (the branch adds a loss
    and changes nothing else), there is no loss_keypoint, and ground-truth keypoints in the batch are ignored."""
    from lvc_amd.utils.events import EventStorage

    g = gold("keypoint_train")
    _identity_randperm(monkeypatch)
    base = _keypoint_model(keypoint_on=False)
    with EventStorage(0):
        a = base(_step_batch(g))
        b = step_model(_step_batch(g))
    assert set(a) == set(BOX_LOSSES) and set(b) == set(LOSSES)
    for k in a:
        assert torch.equal(a[k].detach(), b[k].detach()), (k, float(a[k]), float(b[k]))


def test_training_without_the_switch_still_refuses():
    from lvc_amd.modeling.roi_heads.keypoint_head import TRAIN_REFUSAL
    from lvc_amd.utils.events import EventStorage

    g = gold("keypoint_train")
    model = _keypoint_model(enable=False)
    with EventStorage(0), pytest.raises(NotImplementedError) as e:
        model(_step_batch(g))
    assert str(e.value) == TRAIN_REFUSAL == "training the keypoint branch (MODEL.KEYPOINT_ON: keypoint_rcnn_loss, gt_keypoints) is not built"
    with pytest.raises(NotImplementedError, match="not built"):
        model.roi_heads.keypoint_head(torch.zeros(1, 256, 14, 14, device=_dev()), [])


def test_head_forward_with_the_reference_signature(step_model):
    """`KRCNNConvDeconvUpsampleHead.forward(x, instances)` in training mode, as the reference calls it -- pooled features [M, C, S, S] of
    the SELECTED foreground instances, each with `proposal_boxes` and `gt_keypoints` -- against `loss_nhwc` on the same rows with the
    fixture's targets: the same bits; instances without a valid keypoint give 0 and count as a skipped batch."""
    from lvc_amd.layers.layout import to_nhwc
    from lvc_amd.modeling.roi_heads import keypoint_head as kh
    from lvc_amd.structures import Boxes, Instances, Keypoints
    from lvc_amd.utils.events import EventStorage

    g = gold("keypoint_train")
    dev = _dev()
    head = step_model.roi_heads.keypoint_head
    instances, targets, valids = [], [], []
    for i, (h, w, _seed) in enumerate(_SIZES):
        keep = g["selected%d" % i].bool()
        inst = Instances((h, w))
        inst.proposal_boxes = Boxes(g["fg_boxes%d" % i][keep])
        inst.gt_keypoints = Keypoints(g["gt_keypoints%d" % i][g["fg_matched%d" % i].long()][keep])
        instances.append(inst.to(dev))
        targets.append(g["targets%d" % i][keep])
        valids.append(g["valid%d" % i][keep])
    M = sum(len(i) for i in instances)
    x = torch.randn(M, 256, 14, 14, generator=torch.Generator().manual_seed(5)).relu_().to(dev)
    with EventStorage(0) as storage:
        out = head(x, instances)
    assert set(out) == {"loss_keypoint"} and "kpts_num_skipped_batches" not in _latest(storage)
    with torch.no_grad():
        want, _total, count = head.loss_nhwc(to_nhwc(x).contiguous(), torch.cat(targets).to(torch.int32).to(dev),
                                             torch.cat(valids).to(torch.uint8).to(dev), num_images=2)
    assert int(count) == int(torch.cat(valids).sum()) and torch.equal(out["loss_keypoint"].detach(), want)
    out["loss_keypoint"].backward()
    grad = head.score_lowres.weight.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    for inst in instances:
        inst.gt_keypoints.tensor[:, :, 2] = 0
    before = kh._TOTAL_SKIPPED
    with EventStorage(0) as storage:
        out = head(x, instances)
    assert float(out["loss_keypoint"].detach()) == 0.0 and _latest(storage)["kpts_num_skipped_batches"] == before + 1
    with EventStorage(0) as storage:
        out = head(x[:0], [i[:0] for i in instances])
    assert float(out["loss_keypoint"].detach()) == 0.0 and _latest(storage)["kpts_num_skipped_batches"] == before + 2
