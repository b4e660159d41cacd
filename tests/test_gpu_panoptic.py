"""lvcseg_panoptic_combine on the device against the reference's own combine_semantic_and_instance_outputs
(tests/golden/panoptic_combine_cases.npz), and the PanopticFPN / SemanticSegmentor models against tests/seg_ref.py."""
import numpy as np
import pytest
import torch

import seg_ref
from helpers import gold

pytestmark = pytest.mark.gpu


def _cases():
    z = gold("panoptic_combine_cases")
    out = []
    for i, name in enumerate(z["names"].tolist()):
        H, W = (int(v) for v in z["shape_%d" % i])
        n = len(z["scores_%d" % i])
        masks = np.unpackbits(z["masks_%d" % i].numpy())[: n * H * W].reshape(n, H, W) if n else np.zeros((0, H, W), np.uint8)
        out.append(dict(name=name, shape=(H, W), masks=masks, scores=z["scores_%d" % i], classes=z["classes_%d" % i],
                        labels=z["labels_%d" % i], pan=z["pan_%d" % i], seg=z["seg_%d" % i].numpy().reshape(-1, 5),
                        segscore=z["segscore_%d" % i].numpy()))
    return out, [float(v) for v in z["params"]]


def _tight_box(m):
    ys, xs = np.nonzero(m)
    if len(ys) == 0:
        return [0.0, 0.0, 1.0, 1.0]
    return [float(xs.min()), float(ys.min()), float(xs.max() + 1), float(ys.max() + 1)]


def _combine(cases, params, use_boxes, int32_labels=False):
    """All `cases` as one batch in one launch -> per case (panoptic [H,W] int32, rows [count, 8] int32), on the host."""
    from lvc_amd import kernels as K

    rows, boxes, sizes, offs, planes, total = [], [], [], [], [], 0
    for c in cases:
        H, W = c["shape"]
        for m in c["masks"]:
            rows.append(len(rows))
            boxes.append(_tight_box(m) if use_boxes else [0.0, 0.0, float(W), float(H)])
            sizes.append((H, W))
            offs.append(total)
            planes.append(torch.from_numpy(m.reshape(-1).copy()))
            total += H * W
    jobs = K.paste_jobs(rows, np.array(boxes, dtype=np.float32).reshape(-1, 4), sizes, offs)
    planes = (torch.cat(planes) if planes else torch.zeros(16, dtype=torch.uint8)).cuda()
    counts = [len(c["masks"]) for c in cases]
    score_off = np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist()
    scores = torch.cat([c["scores"].float() for c in cases] + [torch.zeros(1)]).cuda()
    classes = torch.cat([c["classes"].int() for c in cases] + [torch.zeros(1, dtype=torch.int32)]).cuda()
    labels = torch.cat([c["labels"].reshape(-1) for c in cases]).to(torch.int32 if int32_labels else torch.uint8).cuda()
    label_off = np.concatenate([[0], np.cumsum([c["shape"][0] * c["shape"][1] for c in cases])[:-1]]).tolist()
    pan, seg, cnt, pan_off, seg_off = K.panoptic_combine(planes, jobs, counts, [c["shape"] for c in cases], scores, classes, score_off,
                                                         labels, label_off, 54, params[0], params[1], params[2], use_boxes=use_boxes)
    pan, seg, cnt = pan.cpu(), seg.cpu().numpy(), cnt.cpu().tolist()
    out = []
    for i, c in enumerate(cases):
        H, W = c["shape"]
        table = seg[seg_off[i]: seg_off[i] + counts[i] + 54]
        assert not table[cnt[i]:].any(), "rows past the count are zero"
        out.append((pan[pan_off[i]: pan_off[i] + H * W].view(H, W), table[: cnt[i]]))
    return out


def _check_case(c, pan, rows):
    from lvc_amd import kernels as K

    assert torch.equal(pan, c["pan"]), c["name"]
    info = K.segments_info(rows)
    want = c["seg"]
    assert [(s["id"], int(s["isthing"]), s["category_id"], s.get("instance_id", -1), s.get("area", -1)) for s in info] == [tuple(r) for r in want.tolist()], c["name"]
    assert [s.get("score", 0.0) for s in info] == c["segscore"].tolist(), c["name"]
    for s, r in zip(info, rows):      # the area column: the pixels the segment holds in the map
        assert int(r[5]) == int((pan == s["id"]).sum())
    ref_pan, ref_info = seg_ref.combine(c["masks"], c["scores"].numpy(), c["classes"].numpy(), c["labels"].numpy(), 0.5, 100, 0.5)
    assert np.array_equal(ref_pan, pan.numpy()) and ref_info == info, c["name"]


@pytest.mark.parametrize("use_boxes", [False, True])
def test_combine_every_case_alone(use_boxes):
    cases, params = _cases()
    assert params == [0.5, 100.0, 0.5]
    for c in cases:
        (pan, rows), = _combine([c], params, use_boxes)
        _check_case(c, pan, rows)


def test_combine_all_cases_as_one_batch_twice():
    """Images of two sizes in one call, one workgroup each; a second run gives the same bits."""
    cases, params = _cases()
    assert len({c["shape"] for c in cases}) == 2
    first = _combine(cases, params, True)
    again = _combine(cases, params, True, int32_labels=True)
    for c, (pan, rows), (pan2, rows2) in zip(cases, first, again):
        _check_case(c, pan, rows)
        assert torch.equal(pan, pan2) and np.array_equal(rows, rows2)


def test_combine_equal_scores_take_the_lower_index_first():
    H, W = 24, 40
    masks = np.zeros((3, H, W), np.uint8)
    masks[0, 2:12, 2:22] = 1
    masks[1, 2:12, 12:32] = 1      # half of it under instance 0: kept only if it comes second
    masks[2, 14:20, 5:9] = 1
    c = dict(name="ties", shape=(H, W), masks=masks, scores=torch.tensor([0.75, 0.75, 0.75]), classes=torch.tensor([4, 5, 6], dtype=torch.int32),
             labels=torch.ones(H, W, dtype=torch.uint8))
    (pan, rows), = _combine([c], [0.4, 10.0, 0.5], False)
    ref_pan, ref_info = seg_ref.combine(masks, c["scores"].numpy(), c["classes"].numpy(), c["labels"].numpy(), 0.4, 10.0, 0.5)
    from lvc_amd import kernels as K

    assert np.array_equal(ref_pan, pan.numpy()) and K.segments_info(rows) == ref_info
    assert [s["instance_id"] for s in ref_info if s["isthing"]] == [0, 2]


# ------------------------------------------------------------------------------------------------ the models
_SIZES = ((128, 160, 3), (120, 176, 4))
K_BAR = 3.0


def _inputs(device=None):
    from lvc_amd.utils import synthetic as syn

    out = []
    for h, w, seed in _SIZES:
        im = syn.synthetic_image(seed, h, w)
        out.append({"image": im.to(device) if device is not None else im, "height": h, "width": w})
    return out


def _cfg(arch="PanopticFPN"):
    from lvc_amd.config.presets import panoptic_fpn

    g = gold("panoptic_fpn_small")
    cfg = panoptic_fpn(num_classes=20, num_stuff_classes=54)
    cfg.TEST.DETECTIONS_PER_IMAGE = 20
    cfg.MODEL.META_ARCHITECTURE = arch
    _, limit, conf = (float(v) for v in g["params"])
    cfg.MODEL.PANOPTIC_FPN.COMBINE.STUFF_AREA_LIMIT = int(limit)
    cfg.MODEL.PANOPTIC_FPN.COMBINE.INSTANCES_CONFIDENCE_THRESH = conf
    return cfg


@pytest.fixture(scope="module")
def model():
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    return syn.conditioned_panoptic_(build_model(_cfg()).eval())


@pytest.fixture(scope="module")
def outputs(model):
    with torch.no_grad():
        out = model(_inputs())
    torch.cuda.synchronize()
    return out


def _category_map(pan, info):
    """[H, W] int64: 0 where no segment, else 1 + category_id + 1000 * isthing."""
    out = torch.zeros(pan.shape, dtype=torch.int64)
    for s in info:
        out[pan == s["id"]] = 1 + s["category_id"] + 1000 * int(s["isthing"])
    return out


def test_model_detections_pass_the_mask_models_gate(outputs):
    from oracle import noise as onoise

    g = gold("mask_rcnn_small")      # the instance half of the reference PanopticFPN is that fixture's model (asserted by the script)
    nz = dict(zip(g["noise_keys"].tolist(), [float(v) for v in g["noise_vals"].tolist()]))
    nz["counts_equal"] = bool(nz["counts_equal"])
    ours = [(o["instances"].pred_boxes.tensor.cpu(), o["instances"].scores.cpu(), o["instances"].pred_classes.cpu()) for o in outputs]
    want = [(g["det32_boxes_%d" % i], g["det32_scores_%d" % i], g["det32_classes_%d" % i].long()) for i in range(2)]
    ok, bars, msg = onoise.gate(onoise.deviation(ours, want, nz["box_tol"], nz["score_tol"]), nz)
    assert ok, msg
    assert set(outputs[0]) == {"instances", "sem_seg", "panoptic_seg"}


def test_model_sem_seg_within_the_references_own_error(outputs):
    g = gold("panoptic_fpn_small")
    soft = outputs[0]["sem_seg"]
    assert soft.shape == (54, 128, 160) and soft.dtype == torch.float32
    ours = soft[[int(c) for c in g["soft_classes"]]].cpu()
    err, noise = float((ours.double() - g["soft32_0"].double()).abs().max()), float(g["sem_err64"])
    print("sem_seg: |hip - reference| %.3e, reference |fp32 - fp64| %.3e, bar %.3e" % (err, noise, K_BAR * noise))
    assert err <= K_BAR * noise


def test_model_panoptic_is_seg_refs_combine_of_its_own_outputs(model, outputs):
    for o in outputs:
        inst = o["instances"]
        pan, info = o["panoptic_seg"]
        assert pan.dtype == torch.int32 and tuple(pan.shape) == inst.image_size
        want_pan, want_info = seg_ref.combine(inst.pred_masks.cpu().numpy(), inst.scores.cpu().numpy(), inst.pred_classes.cpu().numpy(),
                                              o["sem_seg"].cpu().argmax(0).numpy(), model.combine_overlap_threshold,
                                              model.combine_stuff_area_limit, model.combine_instances_confidence_threshold)
        assert np.array_equal(pan.cpu().numpy(), want_pan)
        assert info == want_info


def test_model_panoptic_against_the_reference(outputs):
    g, gm = gold("panoptic_fpn_small"), gold("mask_rcnn_small")
    aside = total = 0
    for i, (h, w, _) in enumerate(_SIZES):
        pan, info = outputs[i]["panoptic_seg"]
        want = g["seg32_%d" % i].numpy().reshape(-1, 5)
        assert [(int(s["isthing"]), s["category_id"]) for s in info] == [(int(r[1]), int(r[2])) for r in want]
        assert [s["id"] for s in info] == [int(r[0]) for r in want]
        want_info = [{"id": int(r[0]), "isthing": bool(r[1]), "category_id": int(r[2])} for r in want]
        n = len(gm["det32_scores_%d" % i])
        band = torch.from_numpy(np.unpackbits(gm["band_%d" % i].numpy())[: n * h * w].reshape(n, h, w)).bool().any(0)
        band |= torch.from_numpy(np.unpackbits(g["label_band_%d" % i].numpy())[: h * w].reshape(h, w)).bool()
        ours, ref = _category_map(pan.cpu(), info), _category_map(g["pan32_%d" % i], want_info)
        assert torch.equal(ours[~band], ref[~band]), int((ours != ref)[~band].sum())
        aside += int(band.sum())
        total += h * w
    print("panoptic vs reference: %d of %d pixels set aside (%.4f %%)" % (aside, total, 100.0 * aside / total))


def test_forward_reads_the_device_twice(model, outputs):
    """The device part -- trunk, heads, mask branch, semantic head, semantic postprocess -- under sync-debug "error"; the whole forward
    under "warn": two synchronising operations, the mask model's read and the read of the segment tables."""
    import warnings

    inputs = _inputs(torch.device("cuda:0"))
    with torch.no_grad():
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            model._masks_device(inputs, True)
            sem, labels, _ = model.__dict__.pop("_semantic")
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(sem[0]["sem_seg"], outputs[0]["sem_seg"]) and labels.dtype == torch.uint8
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                out = model(inputs)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower()]
        print("synchronising operations in PanopticFPN.forward:", syncs)
        assert len(syncs) == 2, syncs
    for a, b in zip(out, outputs):
        assert torch.equal(a["panoptic_seg"][0], b["panoptic_seg"][0]) and a["panoptic_seg"][1] == b["panoptic_seg"][1]
        assert torch.equal(a["sem_seg"], b["sem_seg"])


def test_labels_only_form_and_combine_off(model, outputs):
    model.keep_sem_seg_logits = False
    try:
        with torch.no_grad():
            out = model(_inputs())
    finally:
        model.keep_sem_seg_logits = True
    for a, b in zip(out, outputs):
        assert "sem_seg" not in a and a["sem_seg_labels"].dtype == torch.uint8
        assert torch.equal(a["sem_seg_labels"].long(), b["sem_seg"].argmax(0))
        assert torch.equal(a["panoptic_seg"][0], b["panoptic_seg"][0]) and a["panoptic_seg"][1] == b["panoptic_seg"][1]
    model.combine_on = False
    try:
        with torch.no_grad():
            out = model(_inputs())
    finally:
        model.combine_on = True
    assert set(out[0]) == {"instances", "sem_seg"} and torch.equal(out[1]["sem_seg"], outputs[1]["sem_seg"])


def test_mask_model_without_the_semantic_head_gives_the_same_instances(outputs):
    from lvc_amd.config.presets import mask_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    cfg = mask_rcnn_fpn(num_classes=20)
    cfg.TEST.DETECTIONS_PER_IMAGE = 20
    base = syn.conditioned_mask_head_(build_model(cfg).eval())
    assert not hasattr(base, "sem_seg_head")
    with torch.no_grad():
        out = base(_inputs())
    for a, b in zip(out, outputs):
        a, b = a["instances"], b["instances"]
        assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor) and torch.equal(a.scores, b.scores)
        assert torch.equal(a.pred_classes, b.pred_classes) and torch.equal(a.pred_masks, b.pred_masks)


def test_semantic_segmentor_gives_the_panoptic_models_sem_seg(model, outputs):
    from lvc_amd.modeling import build_model

    seg = build_model(_cfg("SemanticSegmentor")).eval()
    own = set(seg.state_dict())
    assert all(k.startswith(("backbone.", "sem_seg_head.")) for k in own)
    seg.load_state_dict({k: v for k, v in model.state_dict().items() if k in own}, strict=True)
    with torch.no_grad():
        out = seg(_inputs())
    for a, b in zip(out, outputs):
        assert set(a) == {"sem_seg"} and torch.equal(a["sem_seg"], b["sem_seg"])
    seg.keep_sem_seg_logits = False
    with torch.no_grad():
        out = seg(_inputs())
    assert torch.equal(out[0]["sem_seg_labels"].long(), outputs[0]["sem_seg"].argmax(0))


def test_train_mode_refuses_before_the_device(model):
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="loss_sem_seg"):
            model([{"image": None}])
    finally:
        model.eval()
