"""Keypoint R-CNN inference on the device: the keypoint head's transposed convolution (csrc/keypoint.hip), the heatmap decode
(csrc/keypoint_decode.hip) and the model, against fp64 restatements (tests/keypoint_ref.py), torch's own fp32 result on the CPU and
detectron2's stored outputs (tests/golden/keypoint_head_small.npz, keypoint_rcnn_small.npz).

The bar of every comparison against fp64 is 3 x torch's own CPU fp32 deviation from fp64 on the same case; every (ours, torch's,
ratio) triple goes to profiles/keypoint_rcnn_parity.json."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import keypoint_ref as kr
from helpers import ROOT, found_bar, gold, match_fraction

pytestmark = pytest.mark.gpu

_SIZES = ((128, 160, 3), (120, 176, 4))
_PARITY = {}
K17 = 17


@pytest.fixture(scope="module", autouse=True)
def write_parity():
    yield
    if not _PARITY:
        return
    path = os.environ.get("LVC_KEYPOINT_RCNN_PARITY_OUT") or os.path.join(ROOT, "profiles", "keypoint_rcnn_parity.json")
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
    bar = 3.0 * noise
    _PARITY[key] = {"ours": ours, "torch": noise, "bar": bar, "ratio": ours / bar if bar > 0 else float("inf") if ours > 0 else 0.0}
    print("%-44s ours %.3e  torch's own %.3e  bar %.3e" % (key, ours, noise, bar))
    return bar


# ------------------------------------------------------------------ the transposed convolution
def _K():
    from lvc_amd import kernels

    return kernels


def _deconv_case(M, S, cin, k, plant=None):
    g = torch.Generator().manual_seed(7919 * M + 131 * S + cin + 3 * k)
    x = torch.randn(M, S, S, cin, generator=g).relu_()
    w = torch.randn(cin, k, 4, 4, generator=g) * math.sqrt(2.0 / (4 * cin))
    b = torch.randn(k, generator=g) * 0.5
    if plant is not None:
        x.view(-1)[x.numel() // 3] = plant
    return x, w, b


def _deconv_refs(x, w, b):
    xc = x.permute(0, 3, 1, 2).contiguous()
    exact = F.conv_transpose2d(xc.double(), w.double(), b.double(), stride=2, padding=1)
    noise = float((F.conv_transpose2d(xc, w, b, stride=2, padding=1).double() - exact).abs().max())
    return exact, noise


def _run_deconv(x, w, b, **kw):
    K = _K()
    dev = _dev()
    return K.keypoint_deconv(x.to(dev), K.pack_keypoint_deconv(w.to(dev)), b.to(dev), w.shape[1], **kw)


def _cin_min():
    return _K().KEYPOINT_DECONV_CIN


DECONV_SHAPES = ((1, 1, None, 1), (3, 7, 64, 17), (5, 14, 512, 17), (2, 14, 192, 5), (2, 3, 64, 33))


@pytest.mark.parametrize("shape", DECONV_SHAPES)
def test_deconv_against_fp64(shape):
    """Measured on an MI355X (ours, torch's own, bar): 1x1x16x1 1.5e-08 / 1.5e-08 / 4.5e-08; 3x7x64x17 3.5e-07 / 1.7e-06 / 5.0e-06;
    5x14x512x17 7.5e-07 / 1.9e-06 / 5.6e-06; 2x14x192x5 3.9e-07 / 1.4e-06 / 4.2e-06; 2x3x64x33 2.7e-07 / 7.2e-07 / 2.1e-06.
    The first case has four outputs of 16 products each, so its bar is a fraction of an ulp: a kernel that ran the 16 products through
    one fp32 accumulator and added the bias in fp32 came out at 5.18e-08 there (0.87 ulp) and missed it; the chains are now a quarter
    as long and are joined, with the bias, in fp64 (csrc/keypoint.hip)."""
    M, S, cin, k = shape
    cin = _cin_min() if cin is None else cin
    x, w, b = _deconv_case(M, S, cin, k)
    exact, noise = _deconv_refs(x, w, b)
    out = _run_deconv(x, w, b).cpu()
    assert out.shape == (M, k, 2 * S, 2 * S)
    err = float((out.double() - exact).abs().max())
    bar = _record("deconv/%s" % "x".join(map(str, (M, S, cin, k))), err, noise)
    assert err <= bar, (err, bar)


def test_deconv_num_valid_leaves_the_rest_alone():
    M, S, cin, k = 5, 7, 64, 17
    x, w, b = _deconv_case(M, S, cin, k)
    exact, noise = _deconv_refs(x, w, b)
    dev = _dev()
    nv = M - 2
    out = torch.full((M, k, 2 * S, 2 * S), -7.25, device=dev)
    xs = x.clone()
    xs[nv:] = float("nan")      # rows past num_valid are not read: a NaN there reaches nothing
    _run_deconv(xs, w, b, num_valid=torch.tensor([nv], dtype=torch.int32, device=dev), out=out)
    out = out.cpu()
    assert torch.equal(out[nv:], torch.full_like(out[nv:], -7.25))
    err = float((out[:nv].double() - exact[:nv]).abs().max())
    bar = _record("deconv/num_valid_%d" % nv, err, noise)
    assert err <= bar, (err, bar)
    none = torch.full((M, k, 2 * S, 2 * S), -7.25, device=dev)
    _run_deconv(x, w, b, num_valid=torch.tensor([0], dtype=torch.int32, device=dev), out=none)
    assert torch.equal(none.cpu(), torch.full((M, k, 2 * S, 2 * S), -7.25))
    assert _run_deconv(x[:0], w, b).shape == (0, k, 2 * S, 2 * S)


def test_deconv_is_range_free():
    M, S, cin, k = 3, 7, 64, 17
    x, w, b = _deconv_case(M, S, cin, k, plant=1e5)
    exact, noise = _deconv_refs(x, w, b)
    out = _run_deconv(x, w, b).cpu()
    err = float((out.double() - exact).abs().max())
    bar = _record("deconv/planted_1e5", err, noise)
    assert float(exact.abs().max()) > 1e3      # the planted value reaches the outputs
    assert err <= bar, (err, bar)


def test_deconv_two_runs_are_bit_identical():
    x, w, b = _deconv_case(5, 14, 512, 17)
    assert torch.equal(_run_deconv(x, w, b), _run_deconv(x, w, b))


def test_deconv_refuses_other_channel_counts():
    K = _K()
    for cin, k in ((8, 17), (72, 17), (64, 0), (64, 65)):
        with pytest.raises(NotImplementedError, match="MODEL.ROI_KEYPOINT_HEAD"):
            K.keypoint_deconv_check(cin, k)
    dev = _dev()
    with pytest.raises(NotImplementedError, match="CONV_DIMS"):
        K.pack_keypoint_deconv(torch.zeros(72, 17, 4, 4, device=dev))
    with pytest.raises(NotImplementedError, match="NUM_KEYPOINTS"):
        K.keypoint_deconv(torch.zeros(1, 2, 2, 64, device=dev), torch.zeros(16 * 96, 64, device=dev), None, 65)


# ------------------------------------------------------------------ the decode
# the kernel tiles a box in strips of 64 columns; its four waves walk the rows.  One box is wider than a strip, one taller than wide,
# the last at least 700 x 500
DECODE_BOXES = {
    "subpixel": (3.3, 4.1, 4.0, 4.6),
    "1x123": (10.0, 5.0, 11.0, 128.0),
    "identity56": (10.0, 20.0, 66.0, 76.0),
    "fractional": (2.25, 3.5, 32.75, 16.25),
    "198x129": (5.25, 7.5, 203.95, 136.7),
    "wide": (1.5, 2.0, 301.0, 40.0),
    "tall": (4.0, 1.0, 45.5, 311.25),
    "700x500": (1.0, 2.0, 720.5, 515.25),
}
_M = 3


def _maps56(seed):
    """[M, 17, 56, 56]: seeded 3 * randn [M, 17, 14, 14], upsampled twice so that neighbouring values correlate."""
    return kr.bilinear_up2(kr.bilinear_up2(kr.smooth_maps(_M, K17, seed)))


_DECODE_CACHE = {}


def _decode_case(name):
    if name not in _DECODE_CACHE:
        maps = _maps56(sorted(DECODE_BOXES).index(name))
        rois = torch.tensor([DECODE_BOXES[name]] * _M, dtype=torch.float32)
        r64, p64, full64 = kr.heatmaps_to_keypoints(maps.double(), rois, return_maps=True)
        r32, _p32 = kr.heatmaps_to_keypoints(maps, rois, resize=kr.interpolate_bicubic)      # torch's own fp32 run
        _DECODE_CACHE[name] = (maps, rois, r64, p64, full64, r32)
    return _DECODE_CACHE[name]


def _check_decode(key, got, rois, r64, p64, full64, r32):
    """got [M, K, 4] from the kernel against the fp64 restatement: logit and score within 3 x torch's fp32 deviation; (x, y) bit-equal
    to the numpy fp32 expression at the position ours reports; the position the fp64 argmax, except for keypoints whose position of
    ours holds an fp64 value within 2 x the logit bar of the fp64 maximum (at most 1 % of the case's keypoints)."""
    M, K = got.shape[:2]
    noise_logit = float((r32[:, :, 2].double() - r64[:, :, 2]).abs().max())
    noise_score = float((r32[:, :, 3].double() - r64[:, :, 3]).abs().max())
    err_logit = float((got[:, :, 2].double() - r64[:, :, 2]).abs().max())
    err_score = float((got[:, :, 3].double() - r64[:, :, 3]).abs().max())
    bar_logit = _record("decode/%s/logit" % key, err_logit, noise_logit)
    bar_score = _record("decode/%s/score" % key, err_score, noise_score)
    aside = 0
    for i in range(M):
        oh, ow, h, w = kr.box_out_size(rois[i].numpy())
        for k in range(K):
            # the position ours reports, recovered from its (x, y): the index whose fp32 expression gives these bits
            gx, gy = np.float32(got[i, k, 0]), np.float32(got[i, k, 1])
            xi = int(np.floor((float(gx) - float(rois[i, 0])) / (float(w) / ow)))
            yi = int(np.floor((float(gy) - float(rois[i, 1])) / (float(h) / oh)))
            cand = [(a, b) for a in (xi - 1, xi, xi + 1) for b in (yi - 1, yi, yi + 1) if 0 <= a < ow and 0 <= b < oh
                    and kr.xy_from_position(rois[i].numpy(), a, b) == (gx, gy)]
            assert cand, ("no position gives ours' (x, y) bits", key, i, k, gx, gy)
            want = (int(p64[i, k, 0]), int(p64[i, k, 1]))
            if want in cand:
                continue
            a, b = cand[0]
            gap = float(r64[i, k, 2] - full64[i][k, b, a])
            assert gap <= 2 * bar_logit, ("position differs from the fp64 argmax beyond a near-tie", key, i, k, cand, want, gap)
            aside += 1
    _PARITY["decode/%s/set_aside" % key] = {"keypoints": M * K, "set_aside": aside}
    assert aside <= 0.01 * M * K, (aside, M * K)
    assert err_logit <= bar_logit, (err_logit, bar_logit)
    assert err_score <= bar_score, (err_score, bar_score)


@pytest.mark.parametrize("name", sorted(DECODE_BOXES))
def test_decode_against_fp64(name):
    from lvc_amd.structures import heatmaps_to_keypoints

    maps, rois, r64, p64, full64, r32 = _decode_case(name)
    dev = _dev()
    got = heatmaps_to_keypoints(maps.to(dev), rois.to(dev))
    again = heatmaps_to_keypoints(maps.to(dev), rois.to(dev))
    assert torch.equal(got, again)      # two runs are bit-identical
    _check_decode(name, got.cpu(), rois, r64, p64, full64, r32)


def test_decode_exact_ties_take_the_lowest_flat_index():
    K = _K()
    dev = _dev()
    # a constant integer map: every resized value is the constant (identity resize, and the x2 resize whose coefficients are dyadic)
    const = torch.full((2, 3, 56, 56), 5.0)
    rois = torch.tensor([[10.0, 20.0, 66.0, 76.0], [0.0, 0.0, 112.0, 112.0]])
    got = K.heatmaps_to_keypoints(const.to(dev), rois.to(dev)).cpu()
    for i in range(2):
        x, y = kr.xy_from_position(rois[i].numpy(), 0, 0)
        assert torch.equal(got[i, :, 0], torch.full((3,), float(x))) and torch.equal(got[i, :, 1], torch.full((3,), float(y))), got[i]
        assert torch.equal(got[i, :, 2], torch.full((3,), 5.0))
        assert torch.allclose(got[i, :, 3], torch.full((3,), 1.0 / (56 * 56)), rtol=1e-6, atol=0)
    # two equal peaks under the identity resize: the lower flat index y * w + x wins, whichever lane or wave finds the other
    peaks = torch.zeros(1, 4, 56, 56)
    pairs = (((3, 40), (30, 2)), ((30, 2), (31, 1)), ((7, 9), (7, 50)), ((55, 55), (54, 0)))      # (y, x) pairs
    for k, ((ya, xa), (yb, xb)) in enumerate(pairs):
        peaks[0, k, ya, xa] = peaks[0, k, yb, xb] = 9.0
    got = K.heatmaps_to_keypoints(peaks.to(dev), rois[:1].to(dev)).cpu()
    for k, pair in enumerate(pairs):
        y, x = min(pair, key=lambda p: p[0] * 56 + p[1])
        wx, wy = kr.xy_from_position(rois[0].numpy(), x, y)
        assert (float(got[0, k, 0]), float(got[0, k, 1]), float(got[0, k, 2])) == (float(wx), float(wy), 9.0), (k, got[0, k])


def test_decode_up2_forms_the_bilinear_map_and_decodes_it():
    K = _K()
    dev = _dev()
    low = kr.bilinear_up2(kr.smooth_maps(_M, K17, 11))      # [M, 17, 28, 28], as score_lowres leaves it
    rois = torch.tensor([DECODE_BOXES["198x129"], DECODE_BOXES["fractional"], DECODE_BOXES["identity56"]])
    maps_out = torch.zeros(_M, K17, 56, 56, device=dev)
    got = K.heatmaps_to_keypoints(low.to(dev), rois.to(dev), up=2, maps_out=maps_out)
    exact = F.interpolate(low.double(), scale_factor=2, mode="bilinear", align_corners=False)
    noise = float((F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=False).double() - exact).abs().max())
    err = float((maps_out.cpu().double() - exact).abs().max())
    bar = _record("decode/up2_map", err, noise)
    assert err <= bar, (err, bar)
    assert float((kr.bilinear_up2(low.double()) - exact).abs().max()) < 1e-12      # (the restatement is ATen's rule)
    # the same decode as an up = 1 call on that map, bit for bit; and without maps_out
    assert torch.equal(got, K.heatmaps_to_keypoints(maps_out, rois.to(dev), up=1))
    assert torch.equal(got, K.heatmaps_to_keypoints(low.to(dev), rois.to(dev), up=2))


def test_decode_num_valid_and_empty():
    K = _K()
    dev = _dev()
    maps, rois, r64, p64, full64, r32 = _decode_case("fractional")
    nv = _M - 2
    out = torch.full((_M, K17, 4), -7.25, device=dev)
    mo = torch.full((_M, K17, 56, 56), -7.25, device=dev)
    K.heatmaps_to_keypoints(maps.to(dev), rois.to(dev), num_valid=torch.tensor([nv], dtype=torch.int32, device=dev), maps_out=mo, out=out)
    full = K.heatmaps_to_keypoints(maps.to(dev), rois.to(dev))
    assert torch.equal(out[:nv], full[:nv]) and torch.equal(mo[:nv].cpu(), maps[:nv])
    assert torch.equal(out[nv:].cpu(), torch.full((_M - nv, K17, 4), -7.25)) and torch.equal(mo[nv:].cpu(), torch.full((_M - nv, K17, 56, 56), -7.25))
    assert K.heatmaps_to_keypoints(maps[:0].to(dev), rois[:0].to(dev)).shape == (0, K17, 4)
    with pytest.raises(NotImplementedError, match="side"):
        K.heatmaps_to_keypoints(torch.zeros(1, 1, 40, 40, device=dev), rois[:1].to(dev), up=2)


def _head(cin, k, S):
    from lvc_amd.config import get_cfg
    from lvc_amd.layers import ShapeSpec
    from lvc_amd.modeling.roi_heads import build_keypoint_head

    cfg = get_cfg()
    cfg.MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS = []
    cfg.MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS = k
    return build_keypoint_head(cfg, ShapeSpec(channels=cin, width=S, height=S)).to(_dev()).eval()


@pytest.mark.parametrize("case", [0, 1])
def test_head_against_the_reference_head(case):
    """`score_lowres` + x2 + decode on the fixture's seeded operands against detectron2's own fp32 bits and its fp64 run."""
    from lvc_amd.structures import Boxes, Instances
    from lvc_amd.utils import synthetic as syn

    g = gold("keypoint_head_small")
    M, S, cin, k = [int(v) for v in g["cases"][case]]
    x, w, b, boxes = syn.keypoint_head_case(M, S, cin, k)
    assert torch.equal(boxes, g["boxes_%d" % case])
    head = _head(cin, k, S)
    head.load_state_dict({"score_lowres.weight": w, "score_lowres.bias": b}, strict=True)
    dev = _dev()
    kp32, kp64 = g["kp32_%d" % case], g["kp64_%d" % case]
    with torch.no_grad():
        maps = head.layers(x.to(dev)).cpu()
        inst = Instances((400, 400))
        inst.pred_boxes = Boxes(boxes.to(dev))
        head(x.to(dev), [inst])
        xyls = head.forward_nhwc(x.permute(0, 2, 3, 1).contiguous().to(dev), boxes.to(dev)).cpu()
    assert maps.shape == (M, k, 4 * S, 4 * S)
    assert torch.equal(inst.pred_keypoints.cpu(), xyls[:, :, [0, 1, 3]])
    if "maps64_%d" % case in g:
        noise = float((g["maps32_%d" % case].double() - g["maps64_%d" % case]).abs().max())
        err = float((maps.double() - g["maps64_%d" % case]).abs().max())
        bar = _record("head/%d/maps" % case, err, noise)
        assert err <= bar, (err, bar)
    for col, name in ((2, "logit"), (3, "score")):
        noise = float((kp32[:, :, col].double() - kp64[:, :, col]).abs().max())
        err = float((xyls[:, :, col].double() - kp64[:, :, col]).abs().max())
        bar = _record("head/%d/%s" % (case, name), err, noise)
        assert err <= bar, (err, bar)
    # positions: the reference's fp64 ones, except where the reference's own fp32 run moved too (at most 1 %)
    moved = (xyls[:, :, :2].double() - kp64[:, :, :2]).abs().amax(2) > 1e-3
    moved_ref = (kp32[:, :, :2].double() - kp64[:, :, :2]).abs().amax(2) > 1e-3
    _PARITY["head/%d/moved" % case] = {"ours": int(moved.sum()), "reference_fp32": int(moved_ref.sum()), "keypoints": moved.numel()}
    assert int(moved.sum()) <= max(3 * int(moved_ref.sum()), math.ceil(0.01 * moved.numel())), (int(moved.sum()), int(moved_ref.sum()))
    same = ~moved & ~moved_ref
    assert torch.equal(xyls[:, :, :2][same], kp32[:, :, :2][same])      # at the same position, the reference's fp32 bits


def test_head_refuses_training():
    head = _head(64, 17, 14).train()
    with pytest.raises(NotImplementedError, match="training the keypoint branch"):
        head(torch.zeros(1, 64, 14, 14, device=_dev()), [])


# ------------------------------------------------------------------ the model
def _inputs(device=None):
    from lvc_amd.utils import synthetic as syn

    out = []
    for h, w, seed in _SIZES:
        im = syn.synthetic_image(seed, h, w)
        out.append({"image": im.to(device) if device is not None else im, "height": h, "width": w})
    return out


@pytest.fixture(scope="module")
def model():
    from lvc_amd.config.presets import keypoint_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    cfg = keypoint_rcnn_fpn()
    cfg.TEST.DETECTIONS_PER_IMAGE = 20
    m = build_model(cfg).eval()
    g = gold("keypoint_rcnn_r50_fpn_keys")
    sd = syn.conditioned_keypoint_rcnn_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, seed=0)
    assert list(sd.keys()) == g["keys"].tolist()
    m.load_state_dict(sd, strict=True)      # a state_dict with the fixture's names loads strictly
    return m


@pytest.fixture(scope="module")
def outputs(model):
    with torch.no_grad():
        out = model(_inputs())
    torch.cuda.synchronize()
    return out


def _compare_keypoints(g, tag, per_image, box_tol):
    """per_image: [(boxes, classes, keypoints [n, K, 3], logits [n, K] or None)] of ours.  Every reference fp32 detection with an
    fp64 twin and one of ours within box_tol: the logits within 3 x band_logit of the fp64 twin's, and the count of keypoints whose
    position differs from the fp64 twin's (by more than 0.5 px, the fixture's rule: the twins' boxes differ by ~0.01 px)."""
    matched = kps = moved = 0
    worst = 0.0
    for i in range(2):
        boxes, classes, kp, logit = per_image[i]
        wb, wc, twin = g["det32_boxes_%d" % i], g["det32_classes_%d" % i].long(), g["match_%d" % i]
        for a in range(len(wc)):
            t = int(twin[a])
            if t < 0:
                continue
            d = (boxes - wb[a]).abs().max(dim=1)[0] + (classes != wc[a]).float() * 1e6
            j = int(d.argmin()) if len(d) else -1
            if j < 0 or float(d[j]) > box_tol:
                continue
            matched += 1
            kps += kp.shape[1]
            moved += int(((kp[j][:, :2].double() - g["kp64_%d" % i][t][:, :2]).abs().amax(1) > 0.5).sum())
            if logit is not None:
                worst = max(worst, float((logit[j].double() - g["logit64_%d" % i][t]).abs().max()))
    print("%s: %d detections matched, %d keypoints, %d moved, worst logit deviation %.3e" % (tag, matched, kps, moved, worst))
    _PARITY["model/" + tag] = {"matched": matched, "keypoints": kps, "moved": moved, "logit": worst,
                               "band_logit": float(g["band_logit"]), "moved_ref": int(g["moved_ref"])}
    return matched, kps, moved, worst


def _moved_bar(g, kps):
    return max(3 * int(g["moved_ref"]), math.ceil(0.01 * kps))


def test_model_detections_and_keypoints_vs_reference(model, outputs):
    from oracle import noise as onoise

    g = gold("keypoint_rcnn_small")
    nz = dict(zip(g["noise_keys"].tolist(), [float(v) for v in g["noise_vals"].tolist()]))
    nz["counts_equal"] = bool(nz["counts_equal"])
    ours = [(o["instances"].pred_boxes.tensor.cpu(), o["instances"].scores.cpu(), o["instances"].pred_classes.cpu()) for o in outputs]
    want = [(g["det32_boxes_%d" % i], g["det32_scores_%d" % i], g["det32_classes_%d" % i].long()) for i in range(2)]
    dev = onoise.deviation(ours, want, nz["box_tol"], nz["score_tol"])
    ok, bars, msg = onoise.gate(dev, nz)
    print("deviation", dev, "bars", bars)
    _PARITY["model/deviation"] = {k: (float(v) if not isinstance(v, bool) else v) for k, v in dev.items()}
    assert ok, msg
    for (b, s, c), (gb, gs, gc) in zip(ours, want):
        frac, _, _ = match_fraction(b, s, c, gb, gs, gc, nz["box_tol"], nz["score_tol"])
        assert frac >= found_bar(nz["matched_fraction"], len(gs)), (frac, len(gs))
    assert outputs[0]["instances"].image_size == (128, 160) and outputs[1]["instances"].image_size == (120, 176)
    # the logits do not leave forward(): the device part hands them out
    with torch.no_grad():
        ob, osc, ocl, cnt, kps, status, out_sizes = model._keypoints_device(_inputs(_dev()), True)
        logits = _forward_logits(model)
    per_image = []
    for i, ((b, _s, c), o) in enumerate(zip(ours, outputs)):
        kp = o["instances"].pred_keypoints.cpu()
        assert kp.shape == (len(b), K17, 3) and torch.equal(kp, kps[i, : len(b)].cpu())
        per_image.append((b, c, kp, logits[i]))
    matched, n, moved, worst = _compare_keypoints(g, "forward", per_image, nz["box_tol"])
    total_twins = sum(int((g["match_%d" % i] >= 0).sum()) for i in range(2))
    assert matched >= found_bar(nz["matched_fraction"], total_twins) * total_twins, (matched, total_twins)
    assert worst <= 3 * float(g["band_logit"]), (worst, float(g["band_logit"]))
    assert moved <= _moved_bar(g, n), (moved, _moved_bar(g, n))


def _forward_logits(model):
    """The logits of the forward's detections, per image and in the detections' order: the same device steps as `_keypoints_device`
    without the postprocess scaling (a detection's logit does not depend on it), gathered through the survivors' rows."""
    from lvc_amd import kernels as K

    inputs = _inputs(_dev())
    x4, sizes = model.preprocess_nhwc(inputs)
    sizes_dev = model._dev_const(sizes, torch.int32)
    feats = model.backbone.forward_nhwc(x4)
    pboxes, _pl, pcount = model.proposal_generator.predict_proposals_batched(feats, sizes_dev)
    heads = model.roi_heads
    ob, osc, ocl, _orow, cnt = heads.forward_batched(feats, pboxes, pcount, sizes_dev, post=None)
    kp, rows = heads.forward_keypoints_batched(feats, ob, cnt)
    B, T = osc.shape
    keep = torch.arange(T, dtype=torch.int32, device=_dev()).repeat(B, 1).contiguous()
    post = model._dev_const([[1.0, 1.0, float(h), float(w)] for h, w in sizes], torch.float32)
    _b, _s, _c, rows, cnt = K.gather_detections(ob, osc, ocl, rows, keep, cnt, T, post=post)
    out = []
    for i, n in enumerate(cnt.tolist()):
        out.append(kp[rows[i, :n].long()][:, :, 2].cpu())
    return out


def test_given_boxes_give_the_references_keypoints(model):
    from lvc_amd.structures import Boxes, Instances

    g = gold("keypoint_rcnn_small")
    dev = _dev()
    det = []
    for i, (h, w, _) in enumerate(_SIZES):
        inst = Instances((h, w))
        inst.pred_boxes = Boxes(g["raw32_boxes_%d" % i].to(dev))
        inst.pred_classes = g["det32_classes_%d" % i].long().to(dev)
        inst.scores = g["det32_scores_%d" % i].to(dev)
        det.append(inst)
    if any(len(g["raw32_boxes_%d" % i]) != len(g["det32_scores_%d" % i]) for i in range(2)):
        pytest.fail("the fixture's raw boxes and detections differ in number: regenerate it")
    with torch.no_grad():
        out = model.inference(_inputs(), detected_instances=det)
        feats = model.backbone(model.preprocess_image(_inputs()).tensor)
        heads = model.roi_heads
        nhwc = {f: feats[f].permute(0, 2, 3, 1) for f in heads.keypoint_in_features}
        R = max(len(d) for d in det)
        boxes = torch.zeros(2, R, 4, device=dev)
        for i, d in enumerate(det):
            boxes[i, : len(d)] = d.pred_boxes.tensor
        xyls, rows = heads.forward_keypoints_batched(nhwc, boxes, torch.tensor([len(d) for d in det], dtype=torch.int32, device=dev))
    per_image = []
    for i, o in enumerate(out):
        r = o["instances"]
        assert len(r) == len(g["det32_scores_%d" % i])
        assert float((r.pred_boxes.tensor.cpu() - g["det32_boxes_%d" % i]).abs().max()) <= 1e-4
        logit = xyls[rows[i, : len(r)].long()][:, :, 2].cpu()
        per_image.append((r.pred_boxes.tensor.cpu(), r.pred_classes.cpu(), r.pred_keypoints.cpu(), logit))
    matched, n, moved, worst = _compare_keypoints(g, "given_boxes", per_image, 1e-3)
    assert matched == sum(int((g["match_%d" % i] >= 0).sum()) for i in range(2))
    assert worst <= 3 * float(g["band_logit"]), (worst, float(g["band_logit"]))
    assert moved <= _moved_bar(g, n), (moved, _moved_bar(g, n))
    with torch.no_grad():
        raw = model.inference(_inputs(), detected_instances=det, do_postprocess=False)
    assert raw[0].pred_keypoints.shape == (len(det[0]), K17, 3) and raw[0].pred_keypoints.dtype == torch.float32


def test_forward_reads_the_device_once(model, outputs):
    """The device part runs under torch's sync-debug mode "error" (a host read inside raises); the whole inference under "warn":
    exactly one synchronising operation, the read of counts and status."""
    import warnings

    inputs = _inputs(_dev())
    with torch.no_grad():
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            ob, osc, ocl, cnt, kps, status, out_sizes = model._keypoints_device(inputs, True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert cnt.tolist() == [len(o["instances"]) for o in outputs] and int(status.item()) == 0
        assert out_sizes == [(128, 160), (120, 176)] and kps.shape[2:] == (K17, 3)
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                out = model._inference_keypoints(inputs, True)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower()]
        print("synchronising operations in _inference_keypoints:", syncs)
        assert len(syncs) == 1, syncs
    for a, b in zip(out, outputs):
        assert torch.equal(a["instances"].pred_keypoints, b["instances"].pred_keypoints)


def test_box_only_model_gives_the_same_detections(outputs):
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    cfg = base_rcnn_fpn(num_classes=1)
    cfg.TEST.DETECTIONS_PER_IMAGE = 20
    base = syn.conditioned_r50_fpn_(build_model(cfg).eval())
    with torch.no_grad():
        out = base(_inputs())
    for a, b in zip(out, outputs):
        a, b = a["instances"], b["instances"]
        assert not a.has("pred_keypoints") and b.has("pred_keypoints")
        assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor) and torch.equal(a.scores, b.scores)
        assert torch.equal(a.pred_classes, b.pred_classes)


def test_train_mode_refuses_before_the_device(model):
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="training the keypoint branch"):
            model(_inputs())
        with pytest.raises(NotImplementedError, match="training the keypoint branch"):
            model.roi_heads(None, {}, [], None)
    finally:
        model.eval()
