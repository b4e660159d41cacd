"""Training Panoptic FPN on the host: tests/seg_train_ref.py -- the plain restatement of the loss and both gradients -- agrees with torch's
float64 autograd of F.interpolate + F.cross_entropy; the opt-in switches; the refusals of the label maps; the reference's loss dict with
its two scalings.  No kernel is launched."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_train_ref

from lvc_amd import _lib

IGNORE = 255


# ------------------------------------------------------------------------------------------------ seg_train_ref against torch's autograd
def _labels(g, sizes, K, ignored=0.2):
    out = []
    for lh, lw in sizes:
        t = torch.randint(0, K, (lh, lw), generator=g)
        t[torch.rand(lh, lw, generator=g) < ignored] = IGNORE
        out.append(t)
    return out


@pytest.mark.parametrize("h, w, K, scale", [(4, 6, 7, 1), (9, 13, 3, 2), (5, 7, 54, 4), (1, 1, 1, 4), (2, 3, 5, 4)])
def test_seg_train_ref_equals_torch_float64_autograd(h, w, K, scale):
    g = torch.Generator().manual_seed(h + w + K + scale)
    H, W = scale * h, scale * w
    low = (torch.randn(2, h, w, K, generator=g, dtype=torch.float64) * 3)
    labels = _labels(g, [(max(H - 1, 1), W), (H, max(W - 2, 1))], K)      # both padded by ignore, differently
    mine = seg_train_ref.loss(low, labels, scale, IGNORE, upstream=1024.0)
    target = seg_train_ref.padded_labels(labels, H, W, IGNORE)
    assert bool((target[0, H - 1:] == IGNORE).all()) or H == 1
    x = low.permute(0, 3, 1, 2).clone().requires_grad_()
    z = F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False)
    loss = F.cross_entropy(z, target, reduction="mean", ignore_index=IGNORE)
    (loss * 1024.0).backward()
    scale_of = lambda t: max(float(t.detach().abs().max()), 1.0)      # noqa: E731
    assert float((mine["z"] - z.detach().permute(0, 2, 3, 1)).abs().max()) <= 1e-12 * scale_of(z)
    assert float((mine["lse"] - torch.logsumexp(z.detach(), 1)).abs().max()) <= 1e-12 * scale_of(z)
    assert abs(float(mine["mean"] - loss.detach())) <= 1e-12 * scale_of(loss)
    assert mine["count"] == int((target != IGNORE).sum())
    grad = x.grad.permute(0, 2, 3, 1)
    assert float((mine["dlow"] - grad).abs().max()) <= 1e-12 * scale_of(grad)
    per = F.cross_entropy(z.detach(), target, reduction="none", ignore_index=IGNORE)
    assert float((mine["pixel"] - per).abs().max()) <= 1e-12 * scale_of(per)


def test_seg_train_ref_upsample2_backward_is_torchs():
    g = torch.Generator().manual_seed(3)
    for shape in [(1, 1, 1, 4), (2, 3, 5, 8), (1, 7, 2, 4), (1, 1, 6, 8), (1, 2, 1, 4)]:
        N, H, W, C = shape
        x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        dy = torch.randn(N, 2 * H, 2 * W, C, generator=g, dtype=torch.float64)
        y = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        assert float((seg_train_ref.upsample2(x.detach().permute(0, 2, 3, 1)) - y.detach().permute(0, 2, 3, 1)).abs().max()) <= 1e-12
        y.backward(dy.permute(0, 3, 1, 2))
        assert float((seg_train_ref.upsample2_backward(dy) - x.grad.permute(0, 2, 3, 1)).abs().max()) <= 1e-12


def test_no_valid_pixel_is_nan_in_the_installed_torch_and_in_the_restatement():
    low = torch.randn(1, 2, 3, 5, dtype=torch.float64)
    labels = [torch.full((8, 12), IGNORE)]
    z = F.interpolate(low.permute(0, 3, 1, 2), scale_factor=4, mode="bilinear", align_corners=False)
    for dtype in (torch.float64, torch.float32):
        assert bool(torch.isnan(F.cross_entropy(z.to(dtype), labels[0][None], reduction="mean", ignore_index=IGNORE)))
    mine = seg_train_ref.loss(low, labels, 4, IGNORE)
    assert mine["count"] == 0 and bool(torch.isnan(mine["mean"]))
    with pytest.raises(IndexError):      # what the device path's IndexError stands for: torch's CPU kernel on a target out of range
        F.cross_entropy(z, torch.full((1, 8, 12), 5), reduction="mean", ignore_index=IGNORE)


# ------------------------------------------------------------------------------------------------ the switches and the refusals
def _cfg(**kw):
    from lvc_amd.config.presets import panoptic_fpn

    return panoptic_fpn(device="cpu", **kw)


def _item(h=32, w=32, **kw):
    from lvc_amd.structures import Boxes, Instances

    inst = Instances((h, w))
    inst.gt_boxes = Boxes(torch.tensor([[2.0, 2.0, 20.0, 20.0]]))
    inst.gt_classes = torch.tensor([1])
    return dict({"image": torch.zeros(3, h, w), "instances": inst}, **kw)


def test_panoptic_switches_exist_return_the_model_and_name_each_other():
    from lvc_amd.modeling import build_model

    m = build_model(_cfg()).train()
    with pytest.raises(NotImplementedError, match=r"training the semantic branch \(loss_sem_seg\) is not built"):
        m([_item()])
    assert m.enable_sem_seg_training() is m
    with pytest.raises(NotImplementedError, match="enable_mask_training"):
        m([_item(sem_seg=torch.zeros(32, 32, dtype=torch.uint8))])
    assert m.enable_sem_seg_training(False) is m and m.enable_mask_training() is m
    with pytest.raises(NotImplementedError, match="enable_sem_seg_training"):
        m([_item(sem_seg=torch.zeros(32, 32, dtype=torch.uint8))])
    m.enable_mask_training(False)
    with pytest.raises(NotImplementedError, match=r"training the semantic branch \(loss_sem_seg\) is not built"):
        m([_item()])


def test_missing_wrong_size_or_non_integer_sem_seg_raises_on_the_host():
    from lvc_amd.modeling import build_model

    pan = build_model(_cfg()).train().enable_mask_training().enable_sem_seg_training()
    cfg = _cfg()
    cfg.MODEL.META_ARCHITECTURE = "SemanticSegmentor"
    seg = build_model(cfg).train()
    assert seg.enable_sem_seg_training() is seg
    for model in (pan, seg):      # (CPU models: anything past these checks would raise for the missing device instead)
        with pytest.raises(ValueError, match='item 0: no "sem_seg"'):
            model([_item()])
        with pytest.raises(ValueError, match=r'item 1: "sem_seg" is \(32, 31\) but the image is \(32, 32\)'):
            model([_item(sem_seg=torch.zeros(32, 32, dtype=torch.uint8)), _item(sem_seg=torch.zeros(32, 31, dtype=torch.uint8))])
        with pytest.raises(ValueError, match='"sem_seg" must be an integer tensor'):
            model([_item(sem_seg=torch.zeros(32, 32))])
        model.sem_seg_head.ignore_value = -1
        try:
            with pytest.raises(ValueError, match="MODEL.SEM_SEG_HEAD.IGNORE_VALUE = -1"):
                model([_item(sem_seg=torch.zeros(32, 32, dtype=torch.uint8))])
        finally:
            model.sem_seg_head.ignore_value = 255
    assert seg.enable_sem_seg_training(False) is seg
    with pytest.raises(NotImplementedError, match="loss_sem_seg"):
        seg([_item(sem_seg=torch.zeros(32, 32, dtype=torch.uint8))])


def test_the_loss_dict_scales_the_detector_losses_and_leaves_the_rpn_losses():
    from lvc_amd.modeling.meta_arch.panoptic_fpn import PanopticFPN, panoptic_losses

    sem = {"loss_sem_seg": torch.tensor(0.5)}
    rpn = {"loss_rpn_cls": torch.tensor(2.0), "loss_rpn_loc": torch.tensor(3.0)}
    det = {"loss_cls": torch.tensor(4.0), "loss_box_reg": torch.tensor(5.0), "loss_mask": torch.tensor(6.0)}
    out = panoptic_losses(sem, rpn, det, 0.25)
    assert {k: float(v) for k, v in out.items()} == {"loss_sem_seg": 0.5, "loss_rpn_cls": 2.0, "loss_rpn_loc": 3.0, "loss_cls": 1.0,
                                                     "loss_box_reg": 1.25, "loss_mask": 1.5}
    # the model's hook is that rule with its own INSTANCE_LOSS_WEIGHT and the semantic loss of the step
    stub = PanopticFPN.__new__(PanopticFPN)
    stub.__dict__.update(instance_loss_weight=0.5, _sem_train={"losses": sem})
    out = PanopticFPN._train_losses(stub, det, rpn)
    assert float(out["loss_mask"]) == 3.0 and float(out["loss_rpn_loc"]) == 3.0 and float(out["loss_sem_seg"]) == 0.5
    # and the base class's is the plain union it always was
    from lvc_amd.modeling.meta_arch.rcnn import GeneralizedRCNN

    base = GeneralizedRCNN._train_losses(stub, det, rpn)
    assert {k: float(v) for k, v in base.items()} == {k: float(v) for k, v in {**det, **rpn}.items()}
    assert GeneralizedRCNN._train_extra_words(stub) == [] and GeneralizedRCNN._on_train_features(stub, None, None, None) is None


# ------------------------------------------------------------------------------------------------ the host checks of csrc/sem_seg_train.hip
def _jobs(rows):
    t = np.ascontiguousarray(rows, dtype=np.int64)
    return t, ctypes.c_void_p(t.ctypes.data)


def test_argument_validation_returns_an_error_without_a_device():
    """Every refusal below is decided on the host, in front of any launch: a status and a text, with pointers that are never followed."""
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)      # (non-null, 16-byte aligned, never dereferenced: each call fails its check first)

    def err():
        return lib.lvc_last_error().decode()

    assert lib.lvcst_upsample2_bilinear_bwd_nhwc(fake, fake, 1, 1, 1, 6, None) == 1 and "multiple of 4" in err()
    assert lib.lvcst_upsample2_bilinear_bwd_nhwc(None, None, 1, 1, 1, 4, None) == 1 and "null pointer" in err()
    assert lib.lvcst_upsample2_bilinear_bwd_nhwc(ctypes.c_void_p(4100), fake, 1, 1, 1, 4, None) == 1 and "16-byte" in err()
    assert lib.lvcst_upsample2_bilinear_bwd_nhwc(None, None, 0, 1, 1, 4, None) == 0      # an empty batch launches nothing

    keep, jobs = _jobs([[0, 8, 12]])
    # (`lse` below: the max map, the first of the two maps the backward takes)
    fwd = lambda logits, K, ld, scale, numel, bytes_, j, lse: lib.lvcst_sem_seg_loss_fwd(      # noqa: E731
        logits, 1, 2, 3, K, ld, scale, fake, numel, bytes_, 255, j, fake, lse, fake, None, fake, 1 << 20, fake, fake, fake, fake, None)
    bwd = lambda logits, K, ld, scale, numel, bytes_, j, lse: lib.lvcst_sem_seg_loss_bwd(      # noqa: E731
        logits, 1, 2, 3, K, ld, scale, fake, numel, bytes_, 255, j, fake, lse, fake, fake, fake, fake, None)
    for call, name in ((fwd, "lvcst_sem_seg_loss_fwd"), (bwd, "lvcst_sem_seg_loss_bwd")):
        assert call(fake, 5, 4, 4, 96, 1, jobs, fake) == 1 and "ld >= K" in err() and name in err()
        assert call(fake, 5, 8, 0, 96, 1, jobs, fake) == 1 and "scale" in err()
        assert call(fake, 5, 8, 65, 96, 1, jobs, fake) == 1 and "scale" in err()
        assert call(fake, 4097, 4100, 4, 96, 1, jobs, fake) == 1 and "K <= 4096" in err()
        assert call(fake, 5, 8, 4, 96, 4, jobs, fake) == 1 and "label_bytes" in err()
        assert call(fake, 5, 8, 4, 95, 1, jobs, fake) == 1 and "a job's label map lies outside the buffer" in err()
        assert call(fake, 5, 8, 4, 96, 1, None, fake) == 1 and "null pointer" in err()
        assert call(None, 5, 8, 4, 96, 1, jobs, fake) == 1 and "null pointer" in err()
        assert call(fake, 5, 8, 4, 96, 1, jobs, None) == 1 and "null pointer" in err()
        keep2, big = _jobs([[0, 9, 12]])      # taller than scale x h = 8
        assert call(fake, 5, 8, 4, 200, 1, big, fake) == 1 and "exceeds scale x the logits" in err()
        keep3, neg = _jobs([[-1, 8, 12]])
        assert call(fake, 5, 8, 4, 200, 1, neg, fake) == 1 and "outside the buffer" in err()
    # the forward's workspace: the query's answer is what the call asks for
    need = lib.lvcst_sem_seg_loss_workspace_bytes(1, 2, 3, 5, 4)
    assert need == 16      # one workgroup: an fp64 sum and an int64 count
    assert lib.lvcst_sem_seg_loss_fwd(fake, 1, 2, 3, 5, 8, 4, fake, 96, 1, 255, jobs, fake, fake, fake, None, fake, need - 1, fake, fake, fake,
                                      fake, None) == 1 and "workspace too small" in err()
    assert lib.lvcst_sem_seg_loss_workspace_bytes(8, 200, 336, 54, 4) == 8 * 50 * 21 * 16      # 16 x 64 tiles of 800 x 1344
    assert lib.lvcst_sem_seg_loss_workspace_bytes(1, 2, 3, 5, 65) == -1 and lib.lvcst_sem_seg_loss_workspace_bytes(1, 0, 3, 5, 4) == -1
    assert lib.lvcst_sem_seg_loss_workspace_bytes(1, 2, 3, 4096, 4) == -1      # one pixel's 2 x 2 footprint of 4097 floats: past the LDS
    del keep, keep2, keep3
