"""csrc/sem_seg.hip on the device: the x2 upsample of the scale heads and the semantic postprocess, bit for bit against tests/seg_ref.py
and to a measured bar against torch on the CPU; the semantic head against the reference's own output (tests/golden)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_ref
from helpers import gold

pytestmark = pytest.mark.gpu

K_BAR = 3.0          # bars are K_BAR x the deviation of torch's own fp32 CPU evaluation from float64 on the same input
CAP = 1e-3           # share of label pixels that may be set aside as undecided at that bar


def _kernels():
    from lvc_amd import kernels as K

    return K


# ------------------------------------------------------------------------------------------------ x2 upsample
@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 3, 5, 128), (1, 7, 2, 64)])
def test_upsample2_bits_bar_and_repeat(shape, with_acc):
    K = _kernels()
    g = torch.Generator().manual_seed(sum(shape) + with_acc)
    N, H, W, C = shape
    x = torch.randn(shape, generator=g) * 3
    acc = torch.randn(N, 2 * H, 2 * W, C, generator=g) * 3 if with_acc else None
    want = seg_ref.upsample2(x.numpy(), None if acc is None else acc.numpy())
    xd, ad = x.cuda(), None if acc is None else acc.cuda()
    got = K.upsample2_bilinear_nhwc(xd, ad)
    again = K.upsample2_bilinear_nhwc(xd, ad)
    assert got.shape == (N, 2 * H, 2 * W, C)
    assert torch.equal(got, again)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), "bits differ from seg_ref.upsample2"

    def torch_ref(dtype):
        y = F.interpolate(x.to(dtype).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        return y if acc is None else acc.to(dtype) + y

    y64 = torch_ref(torch.float64)
    dev32 = float((torch_ref(torch.float32).double() - y64).abs().max())
    err = float((got.cpu().double() - y64).abs().max())
    print("upsample2 %s acc=%s: |hip - fp64| %.3e, torch fp32 deviation %.3e" % (shape, with_acc, err, dev32))
    assert err <= K_BAR * dev32
    if with_acc:      # in place on the accumulator, as the head runs it
        out = K.upsample2_bilinear_nhwc(xd, ad, out=ad)
        assert out is ad and torch.equal(ad, got)


# ------------------------------------------------------------------------------------------------ postprocess
GUARD = 64
POST_SMALL = dict(low=(2, 3), K=5, ld=8, image=(7, 11), outs=((7, 11), (13, 5), (3, 29)))
POST_LARGE = dict(low=(32, 44), K=54, ld=64, image=(125, 173), outs=((125, 173), (97, 131), (250, 346)))


def _low(h, w, K, ld, seed, std=3.0):
    g = torch.Generator().manual_seed(seed)
    low = torch.full((h, w, ld), 1e30)      # the padding channels would win every argmax and poison every sum if they were read
    low[:, :, :K] = torch.randn(h, w, K, generator=g) * std
    return low


def _torch_post(low, K, scale, image, out, dtype):
    x = low[:, :, :K].permute(2, 0, 1)[None].to(dtype)
    y = F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False)[:, :, : image[0], : image[1]]
    return F.interpolate(y, size=out, mode="bilinear", align_corners=False)[0]


def _run_post(lows, K, scale, images, outs, want_soft, want_labels, int32=False):
    """One launch over the images, into buffers with guard elements in front of, between and behind the planes.
    -> per image (soft [K,oh,ow] or None, labels [oh,ow] or None) on the host."""
    Kn = _kernels()
    ld = lows[0].shape[-1]
    jobs, _, _ = Kn.sem_seg_jobs([l.shape[:2] for l in lows], images, outs, K, ld)
    soft_off, lab_off, s, l = [], [], GUARD, GUARD
    for (oh, ow) in outs:
        soft_off.append(s)
        lab_off.append(l)
        s += K * oh * ow + GUARD
        l += oh * ow + GUARD
    jobs[:, 7], jobs[:, 8] = soft_off, lab_off
    logits = torch.cat([t.reshape(-1) for t in lows]).cuda()
    soft = torch.full((s,), float("nan"), device="cuda") if want_soft else None
    labels = torch.full((l,), 171, device="cuda", dtype=torch.int32 if int32 else torch.uint8) if want_labels else None
    rs, rl = Kn.sem_seg_postprocess(logits, jobs, K, scale, 0, 0, want_soft=want_soft, want_labels=want_labels, soft=soft, labels=labels,
                                    ld=ld)
    assert rs is soft and rl is labels
    torch.cuda.synchronize()
    out = []
    soft_h = soft.cpu() if want_soft else None
    lab_h = labels.cpu() if want_labels else None
    smask = torch.ones(s, dtype=torch.bool)
    lmask = torch.ones(l, dtype=torch.bool)
    for i, (oh, ow) in enumerate(outs):
        a = b = None
        if want_soft:
            a = soft_h[soft_off[i]: soft_off[i] + K * oh * ow].view(K, oh, ow)
            smask[soft_off[i]: soft_off[i] + K * oh * ow] = False
        if want_labels:
            b = lab_h[lab_off[i]: lab_off[i] + oh * ow].view(oh, ow).long()
            lmask[lab_off[i]: lab_off[i] + oh * ow] = False
        out.append((a, b))
    if want_soft:
        assert bool(torch.isnan(soft_h[smask]).all()), "soft: elements outside the planes were written"
    if want_labels:
        assert bool((lab_h[lmask] == 171).all()), "labels: elements outside the maps were written"
    return out


def _check_post(low, K, scale, image, out, soft, labels, stats):
    """One image's outputs against seg_ref (bits) and against torch in float64 (bar, band)."""
    ref_soft, ref_labels = seg_ref.postprocess(low.numpy(), K, scale, image, out)
    if soft is not None:
        assert np.array_equal(soft.numpy().view(np.uint32), ref_soft.view(np.uint32)), "soft bits differ from seg_ref.postprocess"
    if labels is not None:
        assert np.array_equal(labels.numpy(), ref_labels), "labels differ from seg_ref.postprocess"
    y64 = _torch_post(low, K, scale, image, out, torch.float64)
    dev32 = float((_torch_post(low, K, scale, image, out, torch.float32).double() - y64).abs().max())
    if soft is not None:
        err = float((soft.double() - y64).abs().max())
        print("postprocess low %s -> %s -> %s: |hip - fp64| %.3e, torch fp32 deviation %.3e" % (tuple(low.shape), image, out, err, dev32))
        assert err <= K_BAR * dev32
    if labels is not None:
        top2 = y64.topk(2, dim=0).values
        band = (top2[0] - top2[1]) < 2 * K_BAR * dev32
        assert torch.equal(labels[~band], y64.argmax(0)[~band]), "labels differ from the float64 argmax outside the band"
        stats[0] += int(band.sum())
        stats[1] += band.numel()


@pytest.mark.parametrize("form", ["both", "labels", "soft"])
@pytest.mark.parametrize("case", [POST_SMALL, POST_LARGE], ids=["small", "large"])
def test_postprocess_each_output_size(case, form):
    K, ld, scale = case["K"], case["ld"], 4
    low = _low(*case["low"], K, ld, seed=K)
    stats = [0, 0]
    for out in case["outs"]:
        (soft, labels), = _run_post([low], K, scale, [case["image"]], [out], form != "labels", form != "soft")
        _check_post(low, K, scale, case["image"], out, soft, labels, stats)
    if form != "soft":
        share = stats[0] / stats[1]
        print("set aside %d of %d label pixels (%.4f %%)" % (stats[0], stats[1], 100 * share))
        assert share <= CAP


def test_postprocess_batch_of_two_images_of_different_sizes():
    K, ld, scale = 54, 64, 4
    lows = [_low(32, 44, K, ld, seed=1), _low(9, 13, K, ld, seed=2)]
    images, outs = [(125, 173), (33, 50)], [(97, 131), (66, 100)]
    res = _run_post(lows, K, scale, images, outs, True, True)
    again = _run_post(lows, K, scale, images, outs, True, True)
    stats = [0, 0]
    for low, image, out, (soft, labels), (soft2, labels2) in zip(lows, images, outs, res, again):
        _check_post(low, K, scale, image, out, soft, labels, stats)
        assert torch.equal(soft, soft2) and torch.equal(labels, labels2)
    assert stats[0] / stats[1] <= CAP


def test_postprocess_a_strong_downscale_shrinks_the_tile():
    """(200, 280) -> (5, 7): an output tile's footprint is the whole low-resolution map; the host must pick a smaller tile."""
    K, ld, scale = 54, 64, 4
    low = _low(50, 70, K, ld, seed=3)
    (soft, labels), = _run_post([low], K, scale, [(200, 280)], [(5, 7)], True, True)
    _check_post(low, K, scale, (200, 280), (5, 7), soft, labels, [0, 0])


def test_postprocess_planted_ties_take_the_lower_class():
    K, ld, scale = 54, 64, 4
    low = _low(32, 44, K, ld, seed=4)
    low[4:20, 6:30, 41] = low[4:20, 6:30, 17] = 40.0 + torch.rand(16, 24, generator=torch.Generator().manual_seed(5))
    low[20:, :, 53] = low[20:, :, 0] = 50.0
    for out in ((125, 173), (97, 131)):
        (_, labels), = _run_post([low], K, scale, [(125, 173)], [out], False, True)
        ref_soft, ref_labels = seg_ref.postprocess(low.numpy(), K, scale, (125, 173), out)
        assert np.array_equal(labels.numpy(), ref_labels)
        tie17 = (ref_soft[17] == ref_soft[41]) & (ref_soft[17] == ref_soft.max(0))
        tie0 = (ref_soft[0] == ref_soft[53]) & (ref_soft[0] == ref_soft.max(0))
        assert tie17.sum() > 1000 and tie0.sum() > 1000
        assert bool((labels.numpy()[tie17] == 17).all()) and bool((labels.numpy()[tie0] == 0).all())


def test_postprocess_int32_labels_above_256_classes():
    K, ld, scale = 300, 300, 2
    low = _low(5, 6, K, ld, seed=6)
    (soft, labels), = _run_post([low], K, scale, [(9, 11)], [(9, 11)], True, True, int32=True)
    _check_post(low, K, scale, (9, 11), (9, 11), soft, labels, [0, 0])
    assert int(labels.max()) > 255
    from lvc_amd._lib import LvcNativeError

    with pytest.raises(LvcNativeError, match="int32"):
        _run_post([low], K, scale, [(9, 11)], [(9, 11)], False, True, int32=False)


# ------------------------------------------------------------------------------------------------ head
def _head(num_classes):
    from lvc_amd.config import get_cfg
    from lvc_amd.layers import ShapeSpec
    from lvc_amd.modeling import build_sem_seg_head
    from lvc_amd.utils import synthetic as syn

    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.SEM_SEG_HEAD.NUM_CLASSES", num_classes])
    head = build_sem_seg_head(cfg, {"p%d" % l: ShapeSpec(channels=256, stride=2 ** l) for l in (2, 3, 4, 5)}).eval()
    sd = syn.conditioned_sem_seg_head_state_dict({k: v.detach().cpu() for k, v in head.state_dict().items()}, seed=0)
    head.load_state_dict(sd, strict=True)
    feats = {k: v.cuda().permute(0, 2, 3, 1).contiguous() for k, v in syn.sem_seg_pyramid(seed=0).items()}
    return head.cuda(), feats


def test_head_logits_and_postprocess_against_the_reference_head():
    """tests/golden/sem_seg_head_small.npz: the reference SemSegFPNHead (fp32, and as .double() for its own error) on the seeded
    pyramid.  Stride-4 logits and soft values within 3 x the reference's |fp32 - fp64|; labels equal outside the band."""
    z = gold("sem_seg_head_small")
    image = tuple(int(v) for v in z["image"])
    outs = [tuple(int(v) for v in o) for o in z["outs"]]
    head, feats = _head(6)
    logits = head.forward_nhwc(feats)
    assert logits.shape == (1, 32, 48, 64) and not logits[..., 6:].any()
    low = logits[0, :, :, :6].permute(2, 0, 1).cpu()
    err = float((low.double() - z["low6"].double()).abs().max())
    print("stride-4 logits: |hip - reference| %.3e, reference |fp32 - fp64| %.3e" % (err, float(z["low6_err64"])))
    assert err <= K_BAR * float(z["low6_err64"])
    res, _, _ = head.postprocess(logits.expand(3, -1, -1, -1).contiguous(), [image] * 3, outs)
    for j, (soft, labels) in enumerate(res):
        band = torch.from_numpy(np.unpackbits(z["band6_%d" % j].numpy())[: labels.numel()].reshape(labels.shape).astype(bool))
        assert torch.equal(labels.cpu()[~band], z["labels6_%d" % j][~band])
        if "soft6_%d" % j in z:
            e = float((soft.cpu().double() - z["soft6_%d" % j].double()).abs().max())
            print("  -> %s: |hip - reference| %.3e, reference |fp32 - fp64| %.3e" % (outs[j], e, float(z["err64_6_%d" % j])))
            assert e <= K_BAR * float(z["err64_6_%d" % j])
    head, feats = _head(54)
    logits = head.forward_nhwc(feats)
    res, _, _ = head.postprocess(logits.expand(3, -1, -1, -1).contiguous(), [image] * 3, outs, want_soft=False)
    for j, (soft, labels) in enumerate(res):
        assert soft is None and labels.dtype == torch.uint8
        band = torch.from_numpy(np.unpackbits(z["band54_%d" % j].numpy())[: labels.numel()].reshape(labels.shape).astype(bool))
        assert torch.equal(labels.cpu()[~band], z["labels54_%d" % j][~band])
