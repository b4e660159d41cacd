"""lvcst_sem_seg_loss_fwd / lvcst_sem_seg_loss_bwd on the device: F.interpolate(x scale, bilinear) + F.cross_entropy(mean, ignore_index)
and its gradient from the stride-`scale` logits, against torch's own float64 evaluation on the CPU.  The bar of every quantity is
3 x the deviation of torch's fp32 CPU evaluation from that float64 one on the same input (one fp32 ulp of the quantity's magnitude
where that deviation is zero).

The per-pixel loss is not an output of the kernel, so its consistency with lvcseg_sem_seg_postprocess is tested through the soft
planes: the kernel's fp64 sum equals the float64 sum of fp32(lse - soft[t]) over the valid pixels to 1e-12 (which holds only if the
kernel's z_t are the soft planes' bits), and lse recomputed from the soft planes in float64 meets the kernel's lse at the bar."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

K_BAR = 3.0
GUARD = 64
IGNORE = 255
# (h, w, K, ld, scale): one pixel; a small odd map; the head's classes on one tile; scale 2; scale 1 (the identity interpolation);
# several workgroups per image with a tile edge in both axes, forward (16 x 64) and backward (8 x 8); scale 64 (the backward's
# outputs of one low-resolution pixel no longer fit the LDS and are read from memory)
CASES = [(1, 1, 1, 4, 4), (2, 3, 5, 8, 4), (5, 7, 54, 64, 4), (9, 13, 3, 64, 2), (4, 6, 7, 8, 1), (19, 37, 54, 64, 4), (2, 2, 3, 4, 64)]
IDS = ["%dx%d_K%d_ld%d_s%d" % c for c in CASES]
MEASURED = {}


def _kernels():
    from lvc_amd import kernels as K

    return K


def _ulp32(magnitude):
    return math.ldexp(1.0, math.frexp(magnitude)[1] - 24) if magnitude > 0 else 0.0


def _bar(dev32, magnitude):
    """3 x torch's fp32 deviation from float64, with a floor of one fp32 ulp of the quantity's magnitude: where torch's fp32 result
    happens to round to the float64 one (a deviation of zero, or of a small part of an ulp), an fp32 result cannot be asked to."""
    return max(K_BAR * dev32, _ulp32(magnitude))


def _record(name, case, ours, torchs):
    MEASURED.setdefault(name, []).append({"case": list(case), "ours": ours, "torch": torchs, "ratio": ours / torchs if torchs else 0.0})
    out = os.environ.get("LVC_PARITY_JSON")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1)


def _label_sizes(H, W):
    """Two images whose own maps are smaller than the padded size, and differ."""
    return [(max(H - 1, 1), W), (H, max(W - 2, 1))]


@functools.lru_cache(maxsize=None)
def _inputs(case, mode):
    """-> (low [2,h,w,ld] fp32 with 1e30 in the padding channels and planted values, labels: two int64 maps).
    mode "mixed": about a fifth of the labels ignored; "one_ignored": image 1 wholly ignored; "none_valid": both."""
    h, w, K, ld, scale = case
    g = torch.Generator().manual_seed(1000 * h + 10 * w + K + scale)
    low = torch.full((2, h, w, ld), 1e30)
    low[..., :K] = torch.randn(2, h, w, K, generator=g) * 3
    plant = [0.0, 30.0, -30.0, 90.0, -90.0]
    for i, v in enumerate(plant):      # single classes of single pixels, then a whole pixel at +90 and one at -90
        low[i % 2, (i * 3) % h, (i * 5) % w, (i * 7) % K] = v
    if h * w > 4:
        low[0, h - 1, w - 1, :K] = 90.0
        low[1, 0, w - 1, :K] = -90.0
    labels = []
    for i, (lh, lw) in enumerate(_label_sizes(scale * h, scale * w)):
        t = torch.randint(0, K, (lh, lw), generator=g)
        t[torch.rand(lh, lw, generator=g) < 0.2] = IGNORE
        if mode == "none_valid" or (mode == "one_ignored" and i == 1):
            t[:] = IGNORE
        labels.append(t)
    return low, labels


@functools.lru_cache(maxsize=None)
def _reference(case, mode):
    """torch on the CPU, float64 and fp32: lse map, mean loss, the gradient for upstream 1.  Computed once per case."""
    import seg_train_ref

    h, w, K, ld, scale = case
    low, labels = _inputs(case, mode)
    target = seg_train_ref.padded_labels(labels, scale * h, scale * w, IGNORE)
    out = {}
    for dtype in (torch.float64, torch.float32):
        x = low[..., :K].permute(0, 3, 1, 2).to(dtype).requires_grad_()
        z = F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False)
        loss = F.cross_entropy(z, target, reduction="mean", ignore_index=IGNORE)
        count = int((target != IGNORE).sum())
        grad = torch.autograd.grad(loss, x)[0].permute(0, 2, 3, 1) if count else None
        out[dtype] = (torch.logsumexp(z.detach(), 1), loss.detach(), grad)
    return out, target


def _run(case, mode, label_dtype, upstreams=(1.0,)):
    """One forward and one backward per upstream, into guarded buffers -> dict of host tensors."""
    K = _kernels()
    h, w, Kc, ld, scale = case
    low, labels = _inputs(case, mode)
    H, W = scale * h, scale * w
    # the label maps lie in one buffer with junk (a valid class) in front of, between and behind them
    offsets, at = [], GUARD
    for t in labels:
        offsets.append(at)
        at += t.numel() + GUARD
    buf = torch.zeros(at, dtype=label_dtype)
    for off, t in zip(offsets, labels):
        buf[off: off + t.numel()] = t.reshape(-1).to(label_dtype)
    jobs, _ = K.sem_seg_loss_jobs([tuple(t.shape) for t in labels], offsets=offsets)
    logits, d_labels = low.cuda(), buf.cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    n_lse, n_low = 2 * H * W, low.numel()
    lse_buf = torch.full((n_lse + 2 * GUARD,), float("nan"), device="cuda")
    lse = lse_buf[GUARD: GUARD + n_lse].view(2, H, W)
    loss, maps, total, count, d_jobs = K.sem_seg_loss_fwd(logits, d_labels, jobs, Kc, scale, IGNORE, status, lse=lse)
    assert torch.equal(maps[0] + maps[1], lse), "lse is not the fp32 sum of the two maps the backward takes"
    res = {"dlow": {}}
    for up in upstreams:
        dl_buf = torch.full((n_low + 2 * GUARD,), float("nan"), device="cuda")
        dlow = dl_buf[GUARD: GUARD + n_low].view(2, h, w, ld)
        g = torch.tensor([up], device="cuda")
        got = K.sem_seg_loss_bwd(logits, d_labels, jobs, d_jobs, Kc, scale, IGNORE, maps, g, count, out=dlow)
        assert got is dlow
        host = dl_buf.cpu()
        assert bool(torch.isnan(host[:GUARD]).all()) and bool(torch.isnan(host[GUARD + n_low:]).all()), "elements outside dlow were written"
        res["dlow"][up] = host[GUARD: GUARD + n_low].view(2, h, w, ld).clone()
    torch.cuda.synchronize()
    host = lse_buf.cpu()
    assert bool(torch.isnan(host[:GUARD]).all()) and bool(torch.isnan(host[GUARD + n_lse:]).all()), "elements outside lse were written"
    res.update(lse=host[GUARD: GUARD + n_lse].view(2, H, W).clone(), loss=loss.cpu(), sum=total.cpu(), count=int(count.cpu()),
               status=int(status.cpu()), logits=logits)
    assert torch.equal(logits.cpu().view(torch.int32), low.view(torch.int32)), "the logits were written"
    return res


def _soft_planes(case, logits):
    """lvcseg_sem_seg_postprocess' soft logits at the equal size: [2, K, H, W] on the host."""
    K = _kernels()
    h, w, Kc, ld, scale = case
    H, W = scale * h, scale * w
    jobs, soft_numel, labels_numel = K.sem_seg_jobs([(h, w)] * 2, [(H, W)] * 2, [(H, W)] * 2, Kc, ld)
    soft, _ = K.sem_seg_postprocess(logits, jobs, Kc, scale, soft_numel, labels_numel, want_soft=True, want_labels=False)
    return soft.view(2, Kc, H, W).cpu()


@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64], ids=["uint8", "int64"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_loss_lse_and_gradient_against_float64(case, label_dtype):
    h, w, Kc, ld, scale = case
    ref, target = _reference(case, "mixed")
    (lse64, loss64, grad64), (lse32, loss32, grad32) = ref[torch.float64], ref[torch.float32]
    res = _run(case, "mixed", label_dtype, upstreams=(1.0, 1024.0))
    again = _run(case, "mixed", label_dtype, upstreams=(1.0, 1024.0))
    valid = target != IGNORE
    assert res["status"] == 0 and res["count"] == int(valid.sum()) > 0

    def check(name, ours, r64, r32):
        dev32 = float((r32.double() - r64).abs().max())
        err = float((ours.double() - r64).abs().max())
        bar = _bar(dev32, float(r64.abs().max()))
        print("%s %s: |hip - fp64| %.3e, torch fp32 deviation %.3e, bar %.3e" % (name, case, err, dev32, bar))
        _record(name, case, err, dev32)
        assert err <= bar, (name, err, bar)

    check("lse", res["lse"], lse64, lse32)
    check("loss", res["loss"].view(()), loss64, loss32)
    for up in (1.0, 1024.0):
        d = res["dlow"][up]
        assert not d[..., Kc:].any(), "dlow: a channel past K is not an exact zero"
        check("dlow_x%g" % up, d[..., :Kc], grad64 * up, grad32 * up)
        assert torch.equal(d.view(torch.int32), again["dlow"][up].view(torch.int32)), "two runs differ (dlow)"
    assert torch.equal(res["lse"].view(torch.int32), again["lse"].view(torch.int32)) and res["count"] == again["count"]
    assert torch.equal(res["loss"].view(torch.int32), again["loss"].view(torch.int32)) and torch.equal(res["sum"], again["sum"])
    assert float(res["loss"]) == float(np.float32(float(res["sum"]) / res["count"]))

    # the kernel's own per-pixel terms, recomputed from its lse and the postprocess kernel's soft planes (its z in the equal-size case)
    soft = _soft_planes(case, res["logits"])
    tt = torch.where(valid, target, torch.zeros_like(target))
    zt = soft.gather(1, tt[:, None])[:, 0]
    terms = (res["lse"] - zt)[valid]      # fp32 subtraction, as the kernel's
    want_sum = float(terms.double().sum())
    rel = abs(float(res["sum"]) - want_sum) / max(abs(want_sum), 1e-300)
    print("  fp64 sum %.15e against its own terms %.15e: relative %.2e" % (float(res["sum"]), want_sum, rel))
    assert rel <= 1e-12
    lse_soft = torch.logsumexp(soft.double(), 1)
    dev32 = float((lse32.double() - lse64).abs().max())
    assert float((res["lse"].double() - lse_soft).abs().max()) <= _bar(dev32, float(lse64.abs().max()))


@pytest.mark.parametrize("case", [CASES[1], CASES[5]], ids=[IDS[1], IDS[5]])
def test_an_image_with_every_label_ignored(case):
    ref, target = _reference(case, "one_ignored")
    (lse64, loss64, grad64), (lse32, loss32, grad32) = ref[torch.float64], ref[torch.float32]
    res = _run(case, "one_ignored", torch.uint8)
    Kc = case[2]
    assert res["count"] == int((target[0] != IGNORE).sum()) and res["status"] == 0
    assert float((res["loss"].double() - loss64).abs()) <= _bar(float((loss32.double() - loss64).abs()), float(loss64.abs()))
    d = res["dlow"][1.0]
    assert not d[1].any(), "the ignored image's gradient is not zero"
    dev32 = float((grad32.double() - grad64).abs().max())
    assert float((d[..., :Kc].double() - grad64).abs().max()) <= _bar(dev32, float(grad64.abs().max()))


def test_no_valid_pixel_gives_nan_as_torch_does():
    case = CASES[1]
    ref, _ = _reference(case, "none_valid")
    assert bool(torch.isnan(ref[torch.float32][1])) and bool(torch.isnan(ref[torch.float64][1]))      # the installed torch, on the CPU
    res = _run(case, "none_valid", torch.int64)
    assert res["count"] == 0 and float(res["sum"]) == 0.0 and bool(torch.isnan(res["loss"]).all()) and res["status"] == 0
    lse64, lse32 = ref[torch.float64][0], ref[torch.float32][0]
    assert float((res["lse"].double() - lse64).abs().max()) <= _bar(float((lse32.double() - lse64).abs().max()), float(lse64.abs().max()))


@pytest.mark.parametrize("bad, label_dtype", [(54, torch.uint8), (200, torch.uint8), (-1, torch.int64), (1 << 40, torch.int64)])
def test_a_label_out_of_range_sets_the_status_bit_and_the_host_raises(bad, label_dtype):
    from lvc_amd.config import get_cfg
    from lvc_amd.layers import ShapeSpec
    from lvc_amd.modeling import build_sem_seg_head

    K = _kernels()
    case = CASES[2]
    h, w, Kc, ld, scale = case
    low, labels = _inputs(case, "mixed")
    labels = [t.clone() for t in labels]
    labels[1][3, 5] = bad
    buf = torch.cat([t.reshape(-1) for t in labels]).to(label_dtype).cuda()
    jobs, _ = K.sem_seg_loss_jobs([tuple(t.shape) for t in labels])
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    loss, _maps, total, count, _ = K.sem_seg_loss_fwd(low.cuda(), buf, jobs, Kc, scale, IGNORE, status)
    assert int(status.cpu()) == K.SEGTRAIN_STATUS_LABEL_RANGE
    # the pixel adds nothing: count and sum are those of the map with that pixel ignored
    labels[1][3, 5] = IGNORE
    buf2 = torch.cat([t.reshape(-1) for t in labels]).to(label_dtype).cuda()
    status2 = torch.zeros(1, dtype=torch.int32, device="cuda")
    _, _, total2, count2, _ = K.sem_seg_loss_fwd(low.cuda(), buf2, jobs, Kc, scale, IGNORE, status2)
    assert int(status2.cpu()) == 0 and int(count.cpu()) == int(count2.cpu()) and torch.equal(total.cpu(), total2.cpu())
    head = build_sem_seg_head(get_cfg(), {"p%d" % l: ShapeSpec(channels=256, stride=2 ** l) for l in (2, 3, 4, 5)})
    head.check_loss_status(0)
    with pytest.raises(IndexError, match="sem_seg.*IGNORE_VALUE.*NUM_CLASSES"):
        head.check_loss_status(int(status.cpu()))


def test_the_autograd_function_and_the_uint8_ignore_refusal():
    from lvc_amd.modeling.meta_arch.semantic_seg import sem_seg_loss

    K = _kernels()
    case = CASES[3]
    h, w, Kc, ld, scale = case
    ref, _ = _reference(case, "mixed")
    low, labels = _inputs(case, "mixed")
    buf = torch.cat([t.reshape(-1) for t in labels]).to(torch.uint8).cuda()
    jobs, _ = K.sem_seg_loss_jobs([tuple(t.shape) for t in labels])
    x = low.cuda().requires_grad_()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    loss = sem_seg_loss(x, buf, jobs, Kc, scale, IGNORE, status)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss * 0.5).backward()
    direct = _run(case, "mixed", torch.uint8, upstreams=(0.5,))
    assert torch.equal(x.grad.cpu(), direct["dlow"][0.5]) and torch.equal(loss.detach().cpu().view(1), direct["loss"])
    with pytest.raises(ValueError, match="MODEL.SEM_SEG_HEAD.IGNORE_VALUE"):
        sem_seg_loss(x.detach(), buf, jobs, Kc, scale, -1, status)
