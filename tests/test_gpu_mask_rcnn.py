"""Mask R-CNN inference on the device: the mask head's tail kernel (csrc/mask_deconv.hip) and the paste kernel (csrc/mask_paste.hip)
against tests/mask_ref.py in fp64, and the whole model against detectron2's Mask R-CNN run on the CPU (tests/golden/mask_head_small.npz,
mask_rcnn_small.npz, scripts/make_golden_mask_rcnn.py, whose seeds these tests repeat).

Bars are measured or derived, not set.  The tail may deviate from the fp64 value by 3 x what torch's own CPU fp32 evaluation
(conv_transpose2d + conv2d + index + sigmoid) deviates on the same input.  Pasted masks are bits: pixels whose fp64 soft value lies
within 3 x the reference arithmetic's own max |fp32 - fp64| of the threshold are set aside (never more than 0.1 % of the compared
pixels), every other pixel must be equal.  Rows go to profiles/mask_rcnn_parity.json (LVC_MASK_RCNN_PARITY_OUT: another path)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mask_ref
from helpers import ROOT, found_bar, gold, match_fraction

pytestmark = pytest.mark.gpu

_SIZES = ((128, 160, 3), (120, 176, 4))
_PARITY = {}
CAP = 1e-3      # largest share of compared pixels a mask comparison may set aside


@pytest.fixture(scope="module", autouse=True)
def write_parity():
    yield
    if not _PARITY:
        return
    path = os.environ.get("LVC_MASK_RCNN_PARITY_OUT") or os.path.join(ROOT, "profiles", "mask_rcnn_parity.json")
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
    _PARITY[key] = {"ours": ours, "noise": noise, "bar": bar, "ratio": ours / bar if bar > 0 else float("inf") if ours > 0 else 0.0}
    print("%-44s ours %.3e  reference's own %.3e  bar %.3e" % (key, ours, noise, bar))
    return bar


# ------------------------------------------------------------------ the tail kernel
def _torch_tail32(x, wd, bd, wp, bp, classes):
    z = F.conv2d(F.relu(F.conv_transpose2d(x, wd, bd, stride=2)), wp, bp)
    c = torch.zeros(len(x), dtype=torch.int64) if classes is None else classes
    return z[torch.arange(len(x)), c].sigmoid()


def _run_tail(x, wd, bd, wp, bp, classes, **kw):
    from lvc_amd import kernels as K

    dev = _dev()
    xn = x.permute(0, 2, 3, 1).contiguous().to(dev)
    cls = None if classes is None else classes.to(torch.int32).to(dev)
    return K.mask_deconv_predict(xn, K.pack_mask_deconv(wd.to(dev)), bd.to(dev), wp.reshape(wp.shape[0], -1).contiguous().to(dev), bp.to(dev),
                                 classes=cls, **kw)


def _case(shape):
    from lvc_amd.utils import synthetic as syn

    return syn.mask_tail_case(*shape)


_REF = {}


def _tail_ref(key, ops):
    """(fp64 value, torch's CPU fp32 deviation from it), computed once per case and shared."""
    if key not in _REF:
        exact = mask_ref.tail(*ops)
        _REF[key] = (exact, float((_torch_tail32(*ops).double() - exact).abs().max()))
    return _REF[key]


TAIL_SHAPES = ((1, 1, 64, 64, 1), (3, 7, 64, 128, 3), (37, 14, 256, 256, 20), (5, 14, 192, 256, 80))


@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_tail_against_fp64(shape):
    ops = _case(shape)
    exact, noise = _tail_ref(shape, ops)
    got = _run_tail(*ops).cpu()
    assert got.shape == exact.shape
    err = float((got.double() - exact).abs().max())
    bar = _record("tail/%s" % "x".join(map(str, shape)), err, noise)
    assert err <= bar, (shape, err, bar)


def test_tail_class_agnostic():
    shape = (3, 7, 64, 128, 3)
    x, wd, bd, wp, bp, _ = _case(shape)
    ops = (x, wd, bd, wp, bp, None)
    exact, noise = _tail_ref(shape + ("agnostic",), ops)
    err = float((_run_tail(*ops).cpu().double() - exact).abs().max())
    bar = _record("tail/class_agnostic", err, noise)
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("keep", ["none", "all_but_two"])
def test_tail_num_valid_leaves_the_rest_alone(keep):
    shape = (37, 14, 256, 256, 20)
    ops = _case(shape)
    exact, noise = _tail_ref(shape, ops)
    M = shape[0]
    nv = 0 if keep == "none" else M - 2
    out = torch.full((M, 28, 28), -7.0, device=_dev())
    got = _run_tail(*ops, num_valid=torch.tensor([nv], dtype=torch.int32, device=_dev()), out=out).cpu()
    assert bool((got[nv:] == -7.0).all())
    if nv:
        err = float((got[:nv].double() - exact[:nv]).abs().max())
        bar = _record("tail/num_valid_%d" % nv, err, noise)
        assert err <= bar, (err, bar)


def test_tail_is_range_free():
    shape = (3, 7, 64, 128, 3)
    x, wd, bd, wp, bp, classes = _case(shape)
    x = x.clone()
    x[0, 5, 3, 3] = 1e5
    ops = (x, wd, bd, wp, bp, classes)
    exact, noise = _tail_ref(shape + ("1e5",), ops)
    got = _run_tail(*ops).cpu()
    assert bool(torch.isfinite(got).all())
    err = float((got.double() - exact).abs().max())
    bar = _record("tail/planted_1e5", err, noise)
    assert err <= bar, (err, bar)


def test_tail_two_runs_are_bit_identical():
    ops = _case((37, 14, 256, 256, 20))
    a, b = _run_tail(*ops), _run_tail(*ops)
    assert torch.equal(a, b)


def test_tail_flags_a_class_out_of_range():
    from lvc_amd import kernels as K

    shape = (3, 7, 64, 128, 3)
    x, wd, bd, wp, bp, classes = _case(shape)
    for bad in (3, -1):
        c = classes.clone()
        c[1] = bad
        status = K.new_status(_dev())
        got = _run_tail(x, wd, bd, wp, bp, c, status=status)
        assert int(status.item()) & K.MASK_BAD_CLASS
        assert bool(torch.isfinite(got).all())
    status = K.new_status(_dev())
    _run_tail(x, wd, bd, wp, bp, classes, status=status)
    assert int(status.item()) == 0


def test_tail_refuses_other_channel_counts():
    from lvc_amd import kernels as K

    with pytest.raises(NotImplementedError, match="MODEL.ROI_MASK_HEAD.CONV_DIM"):
        K.pack_mask_deconv(torch.zeros(96, 96, 2, 2, device=_dev()))


def test_tail_against_the_reference_head():
    g = gold("mask_head_small")
    for i, case in enumerate(g["cases"].tolist()):
        ops = _case(tuple(case))
        got = _run_tail(*ops).cpu()
        err = float((got - g["prob32_%d" % i]).abs().max())
        bar = _record("tail/fixture_%d" % i, err, float(g["err64_%d" % i]))
        assert err <= bar, (case, err, bar)


# ------------------------------------------------------------------ the paste kernel
def _grid_sample_soft(p, b, H, W, dtype):
    """The reference's expression (mask_ops.py _do_paste_mask, skip_empty=False) through torch's own grid_sample, in `dtype`."""
    p, b = p.to(dtype), b.to(dtype)
    x0, y0, x1, y1 = [b[:, i:i + 1] for i in range(4)]
    img_y = torch.arange(0, H, dtype=torch.float32).to(dtype) + 0.5
    img_x = torch.arange(0, W, dtype=torch.float32).to(dtype) + 0.5
    img_y = (img_y - y0) / (y1 - y0) * 2 - 1
    img_x = (img_x - x0) / (x1 - x0) * 2 - 1
    gx = img_x[:, None, :].expand(len(p), H, W)
    gy = img_y[:, :, None].expand(len(p), H, W)
    return F.grid_sample(p[:, None], torch.stack([gx, gy], dim=3), align_corners=False)[:, 0]


def _paste_case():
    p, b, (H, W) = mask_ref.paste_inputs()
    H2, W2 = 40, 57
    rows2 = torch.tensor([4, 0, 9])
    b2 = torch.tensor([[2.5, 3.5, 30.5, 39.5], [0., 0., 57., 40.], [50.2, 10.1, 56.9, 12.4]])
    return (p, b, H, W), (rows2, b2, H2, W2)


def test_paste_against_fp64_and_the_reference_expression():
    from lvc_amd import kernels as K

    (p, b, H, W), (rows2, b2, H2, W2) = _paste_case()
    n1, n2 = len(b), len(b2)
    total = n1 * H * W + n2 * H2 * W2
    jobs = K.paste_jobs(list(range(n1)) + rows2.tolist(), torch.cat([b, b2]).numpy(), [(H, W)] * n1 + [(H2, W2)] * n2,
                        [i * H * W for i in range(n1)] + [n1 * H * W + i * H2 * W2 for i in range(n2)])
    padded = (total + 15) // 16 * 16
    assert padded > total and (H * W) % 16      # planes share 16-byte chunks with their neighbours; the buffer ends in padding
    out = torch.full((padded,), 0xAB, dtype=torch.uint8, device=_dev())
    buf = K.paste_masks(p.to(_dev()), jobs, total, threshold=0.5, out=out).cpu()
    assert bool((buf[total:] == 0xAB).all())
    compared = aside = 0
    for tag, got, pp, bb, hh, ww in (("image0", buf[: n1 * H * W].view(n1, H, W), p, b, H, W),
                                     ("image1", buf[n1 * H * W: total].view(n2, H2, W2), p[rows2], b2, H2, W2)):
        assert bool((got <= 1).all())
        soft64 = mask_ref.paste_soft(pp, bb, hh, ww)
        ref32, ref64 = _grid_sample_soft(pp, bb, hh, ww, torch.float32), _grid_sample_soft(pp, bb, hh, ww, torch.float64)
        noise = float((ref32.double() - ref64).abs().max())
        band = (soft64 - 0.5).abs() <= 3.0 * noise
        want = soft64 >= 0.5
        bad = (got.bool() != want) & ~band
        bad_ref = (got.bool() != (ref32 >= 0.5)) & ~band
        ys, xs = torch.arange(hh)[None, :, None] + 0.5, torch.arange(ww)[None, None, :] + 0.5
        outside = (xs < bb[:, 0, None, None]) | (xs > bb[:, 2, None, None]) | (ys < bb[:, 1, None, None]) | (ys > bb[:, 3, None, None])
        print("paste %s: reference's own max |fp32 - fp64| %.3e, %d of %d pixels within the band, %d differ outside it (%d from the "
              "reference's fp32 bits), %d set" % (tag, noise, int(band.sum()), band.numel(), int(bad.sum()), int(bad_ref.sum()), int(got.sum())))
        _PARITY["paste/" + tag] = {"noise": noise, "band_pixels": int(band.sum()), "pixels": band.numel(), "differ": int(bad.sum()),
                                   "differ_from_reference_fp32": int(bad_ref.sum())}
        assert int(bad.sum()) == 0 and int(bad_ref.sum()) == 0
        assert not bool(got[outside].any())
        assert int(got.sum()) > 0
        compared += band.numel()
        aside += int(band.sum())
    assert aside <= CAP * compared, (aside, compared)


def test_paste_refuses_empty_boxes_and_the_visualisation_branch():
    from lvc_amd import kernels as K
    from lvc_amd._lib import LvcNativeError

    p = torch.rand(2, 28, 28, device=_dev())
    for box in ([3.0, 3.0, 3.0, 9.0], [3.0, 9.0, 8.0, 9.0]):
        with pytest.raises(LvcNativeError, match="zero width or height"):
            K.paste_masks(p, K.paste_jobs([0], [box], [(16, 16)], [0]), 256)
    with pytest.raises(LvcNativeError, match="outside"):
        K.paste_masks(p, K.paste_jobs([2], [[1.0, 1.0, 5.0, 5.0]], [(16, 16)], [0]), 256)
    with pytest.raises(LvcNativeError, match="outside"):
        K.paste_masks(p, K.paste_jobs([0], [[1.0, 1.0, 5.0, 5.0]], [(16, 16)], [16]), 256)
    with pytest.raises(NotImplementedError, match="threshold"):
        K.paste_masks(p, K.paste_jobs([0], [[1.0, 1.0, 5.0, 5.0]], [(16, 16)], [0]), 256, threshold=-1.0)


def test_paste_threshold_zero_sets_every_pixel():
    """The reference's `soft >= 0` is true everywhere, also where no tap meets the mask (those pixels take the wide-store path)."""
    from lvc_amd import kernels as K

    p, b, (H, W) = mask_ref.paste_inputs()
    n = len(b)
    total = n * H * W
    jobs = K.paste_jobs(range(n), b.numpy(), [(H, W)] * n, [i * H * W for i in range(n)])
    out = torch.full(((total + 15) // 16 * 16,), 0xAB, dtype=torch.uint8, device=_dev())
    buf = K.paste_masks(p.to(_dev()), jobs, total, threshold=0.0, out=out).cpu()
    assert bool((buf[:total] == 1).all()) and bool((buf[total:] == 0xAB).all())


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
    from lvc_amd.config.presets import mask_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    cfg = mask_rcnn_fpn(num_classes=20)
    cfg.TEST.DETECTIONS_PER_IMAGE = 20
    m = build_model(cfg).eval()
    return syn.conditioned_mask_head_(m)


@pytest.fixture(scope="module")
def outputs(model):
    with torch.no_grad():
        out = model(_inputs())
    torch.cuda.synchronize()
    return out


def _bits(g, name, i, n, h, w):
    return torch.from_numpy(np.unpackbits(g["%s_%d" % (name, i)].numpy())[: n * h * w].reshape(n, h, w)).bool()


def _compare_masks(g, tag, per_image, box_tol):
    """per_image: [(boxes, classes, masks)] of ours; every reference fp32 detection that has an fp64 twin and one of ours within box_tol
    must have its mask, bit for bit, outside the fixture's band."""
    compared = aside = differ = matched = 0
    for i, (h, w, _) in enumerate(_SIZES):
        boxes, classes, masks = per_image[i]
        assert masks.dtype == torch.bool and masks.shape[1:] == (h, w), (masks.dtype, masks.shape)
        wb, wc, twin = g["det32_boxes_%d" % i], g["det32_classes_%d" % i].long(), g["match_%d" % i]
        n = len(wc)
        want, band = _bits(g, "masks32", i, n, h, w), _bits(g, "band", i, n, h, w)
        for a in range(n):
            if int(twin[a]) < 0:
                continue
            d = (boxes - wb[a]).abs().max(dim=1)[0] + (classes != wc[a]).float() * 1e6
            j = int(d.argmin()) if len(d) else -1
            if j < 0 or float(d[j]) > box_tol:
                continue
            matched += 1
            compared += h * w
            aside += int(band[a].sum())
            differ += int(((masks[j] != want[a]) & ~band[a]).sum())
    print("%s: %d detections matched, %d of %d pixels set aside, %d differ outside the band" % (tag, matched, aside, compared, differ))
    _PARITY["model/" + tag] = {"matched": matched, "compared": compared, "aside": aside, "differ": differ}
    return matched, compared, aside, differ


def test_model_detections_and_masks_vs_reference(model, outputs):
    from oracle import noise as onoise

    g = gold("mask_rcnn_small")
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
    per_image = [(b, c, o["instances"].pred_masks.cpu()) for (b, _s, c), o in zip(ours, outputs)]
    matched, compared, aside, differ = _compare_masks(g, "forward", per_image, nz["box_tol"])
    total_twins = sum(int((g["match_%d" % i] >= 0).sum()) for i in range(2))
    assert matched >= found_bar(nz["matched_fraction"], total_twins) * total_twins, (matched, total_twins)
    assert aside <= CAP * compared and differ == 0, (aside, compared, differ)


def test_given_boxes_give_the_references_masks(model):
    from lvc_amd.structures import Boxes, Instances

    g = gold("mask_rcnn_small")
    dev = _dev()
    det = []
    for i, (h, w, _) in enumerate(_SIZES):
        inst = Instances((h, w))
        inst.pred_boxes = Boxes(g["raw32_boxes_%d" % i].to(dev))
        inst.pred_classes = g["det32_classes_%d" % i].long().to(dev)
        inst.scores = g["det32_scores_%d" % i].to(dev)
        det.append(inst)
    with torch.no_grad():
        out = model.inference(_inputs(), detected_instances=det)
    per_image = []
    for i, o in enumerate(out):
        r = o["instances"]
        assert len(r) == len(g["det32_scores_%d" % i])
        assert float((r.pred_boxes.tensor.cpu() - g["det32_boxes_%d" % i]).abs().max()) <= 1e-4
        per_image.append((r.pred_boxes.tensor.cpu(), r.pred_classes.cpu(), r.pred_masks.cpu()))
    matched, compared, aside, differ = _compare_masks(g, "given_boxes", per_image, 1e-3)
    assert matched == sum(int((g["match_%d" % i] >= 0).sum()) for i in range(2))
    assert aside <= CAP * compared and differ == 0, (aside, compared, differ)
    with torch.no_grad():
        soft = model.inference(_inputs(), detected_instances=det, do_postprocess=False)
    assert soft[0].pred_masks.shape == (len(det[0]), 1, 28, 28) and soft[0].pred_masks.dtype == torch.float32


def test_forward_reads_the_device_once(model, outputs):
    """The device part runs under torch's sync-debug mode "error" (a host read inside raises); the whole inference, the paste
    included, under "warn": exactly one synchronising operation, the read of counts, status, rows and boxes."""
    import warnings

    inputs = _inputs(_dev())
    with torch.no_grad():
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            ob, osc, ocl, rows, cnt, prob, status, out_sizes = model._masks_device(inputs, True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert cnt.tolist() == [len(o["instances"]) for o in outputs] and int(status.item()) == 0
        assert out_sizes == [(128, 160), (120, 176)] and prob.shape[1:] == (28, 28)
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                out = model._inference_masks(inputs, True)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower()]
        print("synchronising operations in _inference_masks:", syncs)
        assert len(syncs) == 1, syncs
    for a, b in zip(out, outputs):
        assert torch.equal(a["instances"].pred_masks, b["instances"].pred_masks)


def test_box_only_model_gives_the_same_detections(outputs):
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    cfg = base_rcnn_fpn(num_classes=20)
    cfg.TEST.DETECTIONS_PER_IMAGE = 20
    base = syn.conditioned_r50_fpn_(build_model(cfg).eval())
    with torch.no_grad():
        out = base(_inputs())
    for a, b in zip(out, outputs):
        a, b = a["instances"], b["instances"]
        assert not a.has("pred_masks") and b.has("pred_masks")
        assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor) and torch.equal(a.scores, b.scores)
        assert torch.equal(a.pred_classes, b.pred_classes)


def test_train_mode_refuses_before_the_device(model):
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="training the mask branch"):
            model(_inputs())
    finally:
        model.eval()
