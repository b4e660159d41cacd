"""Test-time augmentation on the MI355X (lvc_amd/modeling/test_time_augmentation.py, csrc/tta.hip) against the reference's
DatasetMapperTTA / GeneralizedRCNNWithTTA run on CPU (tests/golden/tta_*.npz, scripts/make_golden_tta.py)."""
import numpy as np
import pytest
import torch

from helpers import found_bar, gold, match_fraction, r50_state_dict

pytestmark = pytest.mark.gpu

BOX_TOL, SCORE_TOL = 0.1, 2e-3      # the R50 identity bars (tests/test_gpu_e2e.py)


def _uint8_image(seed, h, w):
    from lvc_amd.utils import synthetic as syn

    return syn.synthetic_image(seed, h, w).round().clamp(0, 255).to(torch.uint8)


@pytest.fixture(scope="module")
def model():
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.modeling import build_model

    torch.cuda.set_device(0)
    m = build_model(base_rcnn_fpn()).eval()
    m.load_state_dict(r50_state_dict(), strict=True)
    return m


def _cfg(min_sizes, max_size, flip):
    from lvc_amd.config.presets import base_rcnn_fpn

    cfg = base_rcnn_fpn()
    cfg.TEST.AUG.MIN_SIZES = tuple(min_sizes)
    cfg.TEST.AUG.MAX_SIZE = max_size
    cfg.TEST.AUG.FLIP = flip
    return cfg


def _dets(inst):
    inst = inst.to("cpu")
    return inst.pred_boxes.tensor, inst.scores, inst.pred_classes


# ------------------------------------------------------------------ 1. resize / mirror kernel
def test_resize_mirror_kernel_is_byte_exact_and_fills_the_slots_as_preprocess_image(model):
    from lvc_amd.modeling import DatasetMapperTTA
    from lvc_amd.modeling.test_time_augmentation import _Plan
    from lvc_amd.structures import ImageList

    g = gold("tta_small")
    dev = model.device
    for i in range(int(g["map_n"])):
        c = g["map%d_cfg" % i].tolist()
        oh, ow, mx, flip, mins = c[0], c[1], c[2], bool(c[3]), c[4:]
        img = g["map%d_in" % i]
        n = int(g["map%d_n" % i])
        refs = [g["map%d_img%d" % (i, k)] for k in range(n)]
        mapper = DatasetMapperTTA(_cfg(mins, mx, flip))
        for inp in ({"image": img, "height": oh, "width": ow}, {"raw": img.permute(1, 2, 0).contiguous(), "height": oh, "width": ow}):
            out = mapper(inp)
            assert len(out) == n
            for k in range(n):
                assert torch.equal(out[k]["image"].cpu(), refs[k]), (i, k)
                assert out[k]["height"] == oh and out[k]["width"] == ow
        # the NHWC4 slots of groups of 3 (mixed sizes, each group padded to its own size) = preprocess_image of the reference's images
        H, W = img.shape[1:]
        plan = _Plan(H, W, oh, ow, mins, mx, flip)
        slots, bufs = [], []
        for g0 in range(0, n, 3):
            sizes = [plan.sizes[j] for j, _ in plan.augs[g0:g0 + 3]]
            Hp, Wp = ImageList.padded_size(sizes, model.backbone.size_divisibility)
            buf = torch.full((len(sizes), Hp, Wp, 4), float("nan"), device=dev)
            bufs.append(buf)
            slots.extend(buf[s] for s in range(len(sizes)))
        plan.launch(img.to(dev), (img.stride(1), img.stride(2), img.stride(0)), dev, slots=slots, mean=model.pixel_mean,
                    std=model.pixel_std)
        for gi, buf in enumerate(bufs):
            ref = model.preprocess_image([{"image": r.to(dev)} for r in refs[3 * gi:3 * gi + 3]])
            rbuf = ref.tensor.as_strided(buf.shape, (buf.shape[1] * buf.shape[2] * 4, buf.shape[2] * 4, 4, 1), ref.tensor.storage_offset())
            assert rbuf.shape == buf.shape
            assert torch.equal(buf, rbuf), (i, gi)


# ------------------------------------------------------------------ 2. merge kernel
def _merge_inputs(augs, hw_list, params_list, dev):
    """augs: per image a list of (boxes, scores, classes) -> the device tables of K.tta_merge."""
    flat = [a for img in augs for a in img]
    T = max(1, max(len(a[1]) for a in flat))
    A = len(flat)
    boxes = torch.zeros(A, T, 4)
    scores = torch.zeros(A, T)
    classes = torch.zeros(A, T, dtype=torch.int32)
    counts = torch.zeros(A, dtype=torch.int32)
    for k, (b, s, c) in enumerate(flat):
        n = len(s)
        boxes[k, :n], scores[k, :n], classes[k, :n], counts[k] = torch.as_tensor(b), torch.as_tensor(s), torch.as_tensor(c), n
    tab, a = [], 0
    for img, (h, w) in zip(augs, hw_list):
        tab.append([a, a + len(img), h, w])
        a += len(img)
    params = torch.tensor([r for p in params_list for r in p], dtype=torch.float32)
    nmax = max(t[1] - t[0] for t in tab) * T
    return [x.to(dev) for x in (boxes, scores, classes, counts, params, torch.tensor(tab, dtype=torch.int32))], nmax


def _small_augs(g, tag, i):
    from lvc_amd.modeling.test_time_augmentation import _Plan, _inverse_steps

    p = "%s_i%d_" % (tag, i)
    h, w, oh, ow = ((240, 320, 480, 640), (352, 200, 352, 200))[i]
    plan = _Plan(h, w, oh, ow, (200, 240, 320), 4000, True)
    n = int(g[p + "naug"])
    augs = [(g[p + "aug%d_boxes" % k], g[p + "aug%d_scores" % k], g[p + "aug%d_classes" % k]) for k in range(n)]
    return augs, (oh, ow), [_inverse_steps(plan.transforms(k)) for k in range(n)]


def test_merge_of_the_reference_detections_is_bit_exact(model):
    from lvc_amd import kernels as K

    g = gold("tta_small")
    dev = model.device
    for tag in ("small_bs3", "small_bs2"):
        parts = [_small_augs(g, tag, i) for i in range(2)]
        args, nmax = _merge_inputs([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts], dev)
        ob, osc, ocl, cnt = K.tta_merge(*args, 2, nmax, 1e-8, 0.5, 100)
        cnt = cnt.tolist()
        for i in range(2):
            p = "%s_i%d_" % (tag, i)
            n = cnt[i]
            assert n == len(g[p + "det_scores"]), (tag, i)
            assert torch.equal(ob[i, :n].cpu(), g[p + "det_boxes"]), (tag, i)
            assert torch.equal(osc[i, :n].cpu(), g[p + "det_scores"]), (tag, i)
            assert torch.equal(ocl[i, :n].cpu(), g[p + "det_classes"]), (tag, i)
        # the union itself: no suppression (IoU > 1 never holds) and every candidate kept -> the clipped, filtered union in
        # score order, ties by union position
        ob, osc, ocl, cnt = K.tta_merge(*args, 2, nmax, 1e-8, 1.0, nmax)
        cnt = cnt.tolist()
        for i in range(2):
            p = "%s_i%d_" % (tag, i)
            oh, ow = parts[i][1]
            ub = g[p + "union_boxes"].clone()
            us, uc = g[p + "union_scores"], g[p + "union_classes"]
            ok = torch.isfinite(ub).all(1) & torch.isfinite(us) & (us > 1e-8)
            ub[:, 0::2] = ub[:, 0::2].clamp(min=0, max=ow)
            ub[:, 1::2] = ub[:, 1::2].clamp(min=0, max=oh)
            ub, us, uc = ub[ok], us[ok], uc[ok]
            order = torch.from_numpy(np.argsort(-us.numpy(), kind="stable"))
            assert cnt[i] == len(order)
            assert torch.equal(ob[i, :cnt[i]].cpu(), ub[order]) and torch.equal(osc[i, :cnt[i]].cpu(), us[order])
            assert torch.equal(ocl[i, :cnt[i]].cpu(), uc[order])


def test_merge_of_crafted_unions_gives_the_reference_keep_lists(model):
    from lvc_amd import kernels as K

    g = gold("tta_small")
    dev = model.device
    case = 0
    while "crafted%d_naug" % case in g:
        p = "crafted%d_" % case
        n = int(g[p + "naug"])
        augs = [(g[p + "aug%d_boxes" % k], g[p + "aug%d_scores" % k], g[p + "aug%d_classes" % k]) for k in range(n)]
        h, w = g[p + "hw"].tolist()
        identity = [[0.0] * K.TTA_PARAM_STRIDE for _ in range(n)]
        args, nmax = _merge_inputs([augs], [(h, w)], [identity], dev)
        ob, osc, ocl, cnt = K.tta_merge(*args, 1, nmax, 1e-8, 0.5, 100)
        m = int(cnt[0])
        assert m == len(g[p + "det_scores"]), case
        assert torch.equal(ob[0, :m].cpu(), g[p + "det_boxes"]), case
        assert torch.equal(osc[0, :m].cpu(), g[p + "det_scores"]), case
        assert torch.equal(ocl[0, :m].cpu(), g[p + "det_classes"]), case
        case += 1
    assert case == 3


# ------------------------------------------------------------------ 3. small case end to end
def test_small_case_end_to_end_at_the_noise_bars(model):
    from lvc_amd import kernels as K
    from lvc_amd.modeling import GeneralizedRCNNWithTTA
    from oracle import noise as onoise
    from oracle import rcnn as orc

    g = gold("tta_small")
    a, b = _uint8_image(3, 240, 320), _uint8_image(4, 352, 200)
    inputs = [{"image": a, "height": 480, "width": 640}, {"image": b, "height": 352, "width": 200}]
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    cfg = _cfg((200, 240, 320), 4000, True)
    nz = None
    for bs in (3, 2):
        tta = GeneralizedRCNNWithTTA(cfg, model, batch_size=bs)
        tag = "small_bs%d" % bs
        # (b) every augmentation's detections, from the groups the fused path runs
        hip, refd = [], []
        for i, inp in enumerate(inputs):
            outs = []
            with torch.no_grad():
                tta._fused(inp, K.new_status(model.device), outs)
            p = "%s_i%d_" % (tag, i)
            for ob, osc, ocl, cnt in outs:
                for r in range(ob.shape[0]):
                    n = int(cnt[r])
                    hip.append((ob[r, :n].cpu(), osc[r, :n].cpu(), ocl[r, :n].cpu().long()))
            refd += [(g[p + "aug%d_boxes" % k], g[p + "aug%d_scores" % k], g[p + "aug%d_classes" % k].long())
                     for k in range(int(g[p + "naug"]))]
        if nz is None:      # the reference path's own fp32-vs-fp64 noise on the augmented images of image 0, in their groups of 3
            from lvc_amd.modeling import DatasetMapperTTA

            augs = DatasetMapperTTA(cfg)(inputs[0])
            cpu_in = [{"image": x["image"].cpu().float()} for x in augs]
            nz = onoise.fp32_vs_fp64(sd, orc.RCNNSpec(), cpu_in)
        dev = onoise.deviation(hip, refd, nz["box_tol"], nz["score_tol"])
        ok, bars, msg = onoise.gate(dev, nz)
        print("%s per augmentation: found %.2f%% (reference path of its own fp64: %.2f%%), box median %.2e p90 %.2e, score median %.2e "
              "p90 %.2e | bars %s" % (tag, 100 * dev["matched_fraction"], 100 * nz["matched_fraction"], dev["box_median"], dev["box_p90"],
                                      dev["score_median"], dev["score_p90"], {k: "%.1e" % v for k, v in bars.items()}))
        assert ok, msg
        assert dev["matched_fraction"] >= 0.9
        # (d) the merged detections
        with torch.no_grad():
            out = tta(inputs)
        for i in range(2):
            p = "%s_i%d_" % (tag, i)
            assert out[i]["instances"].image_size == (inputs[i]["height"], inputs[i]["width"])
            bx, sc, cl = _dets(out[i]["instances"])
            n = len(g[p + "det_scores"])
            frac, wb, ws = match_fraction(bx, sc, cl, g[p + "det_boxes"], g[p + "det_scores"], g[p + "det_classes"].long(),
                                          nz["box_tol"], nz["score_tol"])
            print("%s image %d merged: %d vs %d detections, found %.0f%% (worst box %.2e, score %.2e)" % (tag, i, len(sc), n, 100 * frac, wb, ws))
            assert len(sc) == n
            assert frac >= max(0.9, found_bar(nz["matched_fraction"], n)), (tag, i, frac)


# ------------------------------------------------------------------ 4. default TEST.AUG end to end (trunk up to 1200 x 1600)
def test_default_test_aug_end_to_end(model):
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.modeling import GeneralizedRCNNWithTTA

    d = gold("tta_default")
    c = d["default_cfg"].tolist()
    cfg = base_rcnn_fpn()
    assert [cfg.TEST.AUG.MAX_SIZE, int(cfg.TEST.AUG.FLIP)] + list(cfg.TEST.AUG.MIN_SIZES) == c
    tta = GeneralizedRCNNWithTTA(cfg, model)
    with torch.no_grad():
        out = tta([{"image": _uint8_image(5, 240, 320), "height": 240, "width": 320}])
    bx, sc, cl = _dets(out[0]["instances"])
    n = len(d["default_i0_det_scores"])
    frac, wb, ws = match_fraction(bx, sc, cl, d["default_i0_det_boxes"], d["default_i0_det_scores"], d["default_i0_det_classes"].long(),
                                  BOX_TOL, SCORE_TOL)
    print("default TEST.AUG: %d vs %d detections, found %.0f%% (worst box %.2e, score %.2e)" % (len(sc), n, 100 * frac, wb, ws))
    assert len(sc) == n and frac >= 0.9


# ------------------------------------------------------------------ 5. one size, no flip = the plain raw-input path
def _iou(a, b):
    lt = torch.max(a[:2], b[:2])
    rb = torch.min(a[2:], b[2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[0] * wh[1]
    area = lambda x: (x[2] - x[0]) * (x[3] - x[1])  # noqa: E731
    return float(inter / (area(a) + area(b) - inter))


def test_single_size_without_flip_reproduces_the_plain_path(model):
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.modeling import GeneralizedRCNNWithTTA

    base = base_rcnn_fpn()
    cfg = _cfg((base.INPUT.MIN_SIZE_TEST,), base.INPUT.MAX_SIZE_TEST, False)
    tta = GeneralizedRCNNWithTTA(cfg, model)
    thr = float(cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST)
    empties = renms = trunc = common = 0
    for seed, (h, w) in ((6, (240, 320)), (7, (300, 200))):
        raw = _uint8_image(seed, h, w).permute(1, 2, 0).contiguous()
        with torch.no_grad():
            plain = _dets(model([{"raw": raw}])[0]["instances"])
            aug = _dets(tta([{"raw": raw}])[0]["instances"])
        key = lambda b, s, c: (tuple(b.tolist()), float(s), int(c))  # noqa: E731
        pk = [key(*x) for x in zip(*plain)]
        tk = [key(*x) for x in zip(*aug)]
        pset, tset = set(pk), set(tk)
        both_p = [k for k in pk if k in tset]
        both_t = [k for k in tk if k in pset]
        assert both_p == both_t, "common detections in a different order"
        common += len(both_p)
        for k in tk:
            if k not in pset:      # kept by the merge, dropped by detector_postprocess as empty
                (x0, y0, x1, y1) = k[0]
                assert x1 <= x0 or y1 <= y0, "TTA detection %s not in the plain output and not empty" % (k,)
                empties += 1
        last = min(range(len(tk)), key=lambda j: tk[j][1]) if tk else None
        for k in pk:
            if k in tset:
                continue
            partners = [t for t in tk if t[2] == k[2] and t[1] >= k[1]]
            if any(abs(_iou(torch.tensor(t[0]), torch.tensor(k[0])) - thr) < 1e-5 for t in partners):
                renms += 1                      # suppressed by the merge's NMS at an IoU within fp32 rounding of the threshold
            else:
                assert len(tk) == int(cfg.TEST.DETECTIONS_PER_IMAGE) and last is not None and k[1] <= tk[last][1], \
                    "plain detection %s missing from the TTA output" % (k,)
                trunc += 1                      # behind the last of a full list (the kept empties took its place)
    print("single size, no flip: %d common detections bit-identical; %d empty boxes kept by the merge, %d re-suppressed at the NMS "
          "threshold, %d past a full list" % (common, empties, renms, trunc))
    assert common > 0


# ------------------------------------------------------------------ 6. pipelined evaluation
def test_inference_on_dataset_equals_direct_calls(model):
    from lvc_amd.evaluation import inference_on_dataset
    from lvc_amd.modeling import GeneralizedRCNNWithTTA

    tta = GeneralizedRCNNWithTTA(_cfg((160, 200), 4000, True), model)
    batches = [[{"image": _uint8_image(20 + i, 120 + 8 * i, 160), "height": 240, "width": 320}] for i in range(4)]
    with torch.no_grad():
        direct = [tta(b) for b in batches]
        piped = [o for _, o in inference_on_dataset(tta, batches, depth=2)]
    assert len(piped) == 4
    for d, p in zip(direct, piped):
        for a, b in zip(_dets(d[0]["instances"]), _dets(p[0]["instances"])):
            assert torch.equal(a, b)
