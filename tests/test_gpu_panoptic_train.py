"""Training Panoptic FPN's semantic branch on the device against detectron2's own modules on the CPU (tests/golden,
scripts/make_golden_panoptic_train.py): (a) the head alone, (b) one SemanticSegmentor step, (c) one PanopticFPN step.  Bars are those of
the standing training fixtures (train_base.npz): losses within 2e-4 relative, every gradient with cosine >= 0.998 on the stored samples
and norm error <= 1e-2."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from helpers import gold

pytestmark = pytest.mark.gpu

_SIZES = ((128, 160, 3), (120, 176, 4))
BATCH_SIZE_PER_IMAGE = 128          # as scripts/make_golden_panoptic_train.py
HEAD_LABEL_SEED = 5
MEASURED = {}


def _record(tag, name, value):
    MEASURED.setdefault(tag, {})[name] = value
    out = os.environ.get("LVC_STEP_PARITY_JSON")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1)


def _check_losses(g, losses, tag, keys=None):
    for k in keys or [n[5:] for n in g if n.startswith("loss.")]:
        ref, got = float(g["loss." + k]), float(losses[k].detach())
        rel = abs(got - ref) / max(1.0, abs(ref))
        print("%-14s ours %.7f  reference %.7f (its own fp32-vs-fp64 deviation %.2e)" % (k, got, ref, float(g["loss_dev." + k])))
        _record(tag, "loss/" + k, {"ours": got, "reference": ref, "relative": rel, "reference_fp32_vs_fp64": float(g["loss_dev." + k])})
        assert rel <= 2e-4, k


def _check_grad(g, name, grad, tag, bad):
    gflat = grad.flatten().cpu()
    s, nrm, stride = [float(v) for v in g["grad_stats." + name]]
    sample = gflat[:: int(stride)][:2048].double()
    ref = g["grad_sample." + name].double()
    if nrm == 0.0:
        assert float(gflat.abs().max()) == 0.0, name
        return
    cos = float((sample * ref).sum() / (sample.norm() * ref.norm()).clamp_min(1e-30))
    nerr = abs(float(gflat.double().norm()) - nrm) / max(nrm, 1e-12)
    if "sem_seg_head" in name or tag == "head":
        print("%-52s cos %.6f  norm err %.2e" % (name, cos, nerr))
    _record(tag, "grad/" + name, {"cosine": cos, "norm_error": nerr})
    if not (cos >= 0.998 and nerr <= 1e-2):
        bad[name] = (cos, nerr)


def _check_param_grads(g, model, tag):
    bad = {}
    assert [n for n, p in model.named_parameters() if not p.requires_grad] == g["frozen_names"].tolist()
    for name, p in model.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, name
            continue
        assert p.grad is not None, name
        _check_grad(g, name, p.grad, tag, bad)
    assert not bad, bad


def _count_syncs(fn):
    """-> (fn's result, the synchronising operations torch warned about while it ran)."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return out, sum("synchroniz" in str(w.message).lower() for w in caught)


# ------------------------------------------------------------------------------------------------ (a) the head alone
def _head():
    from lvc_amd.config import get_cfg
    from lvc_amd.layers import ShapeSpec
    from lvc_amd.modeling import build_sem_seg_head
    from lvc_amd.utils import synthetic as syn

    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.SEM_SEG_HEAD.NUM_CLASSES", 54])
    head = build_sem_seg_head(cfg, {"p%d" % l: ShapeSpec(channels=256, stride=2 ** l) for l in (2, 3, 4, 5)})
    sd = syn.conditioned_sem_seg_head_state_dict({k: v.detach().cpu() for k, v in head.state_dict().items()}, seed=0)
    head.load_state_dict(sd, strict=True)
    feats = {k: v.cuda().permute(0, 2, 3, 1).contiguous() for k, v in syn.sem_seg_pyramid(seed=0).items()}
    return head.cuda().train(), feats


def test_head_loss_and_gradients_against_the_reference_head():
    from lvc_amd import kernels as K
    from lvc_amd.utils import synthetic as syn

    g = gold("sem_seg_head_train")
    head, feats = _head()
    with torch.no_grad():
        want_logits = head.forward_nhwc(feats)
    feats = {k: v.requires_grad_() for k, v in feats.items()}
    target = syn.sem_seg_label_map(HEAD_LABEL_SEED, 128, 192, 54, head.ignore_value)
    assert int((target != head.ignore_value).sum()) == int(g["valid"])
    for dtype in (torch.int64, torch.uint8):
        for t in list(head.parameters()) + list(feats.values()):
            t.grad = None
        labels = target.to(dtype).cuda().reshape(-1)
        jobs, _ = K.sem_seg_loss_jobs([(128, 192)])
        logits = head.forward_train_nhwc(feats)
        assert logits.requires_grad and torch.equal(logits.detach(), want_logits), "the training logits are not forward_nhwc's bits"
        losses = head.losses(logits, (labels, jobs))
        assert list(losses) == ["loss_sem_seg"]
        losses["loss_sem_seg"].backward()
        head.check_loss_status(int(head.__dict__["_loss_status"].cpu()))
        tag = "head" if dtype == torch.int64 else "head_uint8"
        _check_losses(g, losses, tag)
        bad = {}
        for name, p in head.named_parameters():
            _check_grad(g, name, p.grad, tag, bad)
        for name, t in feats.items():
            _check_grad(g, "feature." + name, t.grad.permute(0, 3, 1, 2), tag, bad)
        assert not bad, bad
    assert head.predictor.weight.grad.shape == (54, 128, 1, 1) and head.predictor.bias.grad.shape == (54,)


# ------------------------------------------------------------------------------------------------ (b) SemanticSegmentor
def _batch(g=None, device="cuda", label_dtype=torch.int64):
    from lvc_amd.structures import BitMasks, Boxes, Instances
    from lvc_amd.utils import synthetic as syn

    batch = []
    for i, (h, w, seed) in enumerate(_SIZES):
        item = {"image": syn.synthetic_image(seed, h, w).to(device), "height": h, "width": w,
                "sem_seg": syn.sem_seg_label_map(seed, h, w, 54, 255).to(label_dtype).to(device)}
        if g is not None:
            n = len(g["gt_classes%d" % i])
            inst = Instances((h, w))
            inst.gt_boxes = Boxes(g["gt_boxes%d" % i])
            inst.gt_classes = g["gt_classes%d" % i]
            inst.gt_masks = BitMasks(torch.from_numpy(np.unpackbits(g["gt_masks%d" % i].numpy())[: n * h * w].reshape(n, h, w)).bool())
            item["instances"] = inst.to(device)
        batch.append(item)
    return batch


@pytest.fixture(scope="module")
def panoptic_model():
    from lvc_amd.config.presets import panoptic_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    cfg = panoptic_fpn(num_classes=20)
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = BATCH_SIZE_PER_IMAGE
    return syn.conditioned_panoptic_(build_model(cfg)).train()


def test_semantic_segmentor_step_matches_reference(panoptic_model):
    from lvc_amd.config.presets import panoptic_fpn
    from lvc_amd.modeling import build_model

    g = gold("sem_seg_model_train")
    cfg = panoptic_fpn(num_classes=20)
    cfg.MODEL.META_ARCHITECTURE = "SemanticSegmentor"
    model = build_model(cfg).train()
    full = panoptic_model.state_dict()
    model.load_state_dict({k: full[k] for k in model.state_dict()}, strict=True)
    with pytest.raises(NotImplementedError, match="loss_sem_seg"):
        model(_batch())
    assert model.enable_sem_seg_training() is model
    batch = _batch()
    model(batch)      # (routes, packed operands and range words settle in a first pass)
    for p in model.parameters():
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")      # the device part of the step, up to its one read
    try:
        losses, words = model._losses_device(batch)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert words.tolist() == [0, 0]
    losses2 = model(batch)
    assert torch.equal(losses2["loss_sem_seg"].detach(), losses["loss_sem_seg"].detach())
    losses["loss_sem_seg"].backward()
    _check_losses(g, losses, "segmentor")
    _check_param_grads(g, model, "segmentor")
    # a planted label out of range: the step's read raises, as torch's CPU kernel does
    bad = _batch()
    bad[1]["sem_seg"][7, 9] = 54
    with pytest.raises(IndexError, match="sem_seg"):
        model(bad)
    model.enable_sem_seg_training(False)
    with pytest.raises(NotImplementedError, match="loss_sem_seg"):
        model(batch)


# ------------------------------------------------------------------------------------------------ (c) PanopticFPN
LOSSES = ("loss_sem_seg", "loss_cls", "loss_box_reg", "loss_mask", "loss_rpn_cls", "loss_rpn_loc")


def _mask_only_step(model, batch):
    """The same model's mask-only step: the base class's (empty) hooks in place of PanopticFPN's."""
    from lvc_amd.modeling.meta_arch.rcnn import GeneralizedRCNN

    hooks = ("_forward_train", "_on_train_features", "_train_extra_words", "_on_train_extra_words", "_train_losses")
    cls = type(model)
    own = {k: cls.__dict__[k] for k in hooks}
    for k in hooks:
        setattr(cls, k, getattr(GeneralizedRCNN, k))
    try:
        return GeneralizedRCNN.forward(model, batch)
    finally:
        for k in hooks:
            setattr(cls, k, own[k])


def test_panoptic_step_matches_reference(monkeypatch, panoptic_model):
    from lvc_amd.utils.events import EventStorage

    g = gold("panoptic_train")
    model = panoptic_model
    monkeypatch.setattr(torch, "randperm", lambda n, **kw: torch.arange(n, **{k: v for k, v in kw.items() if k in ("device", "dtype")}))
    batch = _batch(g)
    with pytest.raises(NotImplementedError, match=r"training the semantic branch \(loss_sem_seg\) is not built"):
        model(batch)
    assert model.enable_mask_training() is model and model.enable_sem_seg_training() is model
    with EventStorage(0):
        model(batch)      # (routes, packed operands and range words settle in a first pass)
        _mask_only_step(model, batch)
    for p in model.parameters():
        p.grad = None
    torch.cuda.synchronize()
    with EventStorage(0):
        mask_losses, mask_syncs = _count_syncs(lambda: _mask_only_step(model, batch))
        losses, syncs = _count_syncs(lambda: model(batch))
    print("synchronising operations: the panoptic step %d, the same model's mask-only step %d" % (syncs, mask_syncs))
    assert syncs <= mask_syncs and mask_syncs >= 1
    # the keys and the two scalings: the detector losses are the mask-only step's times INSTANCE_LOSS_WEIGHT, the RPN losses are its own
    assert set(losses) == set(LOSSES) and set(mask_losses) == set(LOSSES) - {"loss_sem_seg"}
    wgt = model.instance_loss_weight
    assert wgt == float(g["instance_loss_weight"])
    # (two runs of the detector's own step: equal but for the order of its loss kernels' fp32 sums)
    for k in ("loss_cls", "loss_box_reg", "loss_mask"):
        assert abs(float(losses[k].detach()) - float(mask_losses[k].detach()) * wgt) <= 1e-6 * abs(float(mask_losses[k].detach())), k
    for k in ("loss_rpn_cls", "loss_rpn_loc"):
        assert abs(float(losses[k].detach()) - float(mask_losses[k].detach())) <= 1e-6 * abs(float(mask_losses[k].detach())), k
    sum(losses.values()).backward()
    _check_losses(g, losses, "panoptic", LOSSES)
    _check_param_grads(g, model, "panoptic")
    # uint8 label maps give the same loss bits; a planted label out of range raises at the step's read
    with EventStorage(0):
        again = model(_batch(g, label_dtype=torch.uint8))
        assert torch.equal(again["loss_sem_seg"].detach(), losses["loss_sem_seg"].detach())
        bad = _batch(g)
        bad[0]["sem_seg"][3, 4] = 200
        with pytest.raises(IndexError, match="sem_seg"):
            model(bad)
    model.enable_sem_seg_training(False)
    with pytest.raises(NotImplementedError, match="enable_sem_seg_training"):
        model(batch)
    model.enable_mask_training(False)
    with pytest.raises(NotImplementedError, match=r"training the semantic branch \(loss_sem_seg\) is not built"):
        model(batch)
