"""Generate the fixtures of tests/test_gpu_panoptic_train.py from detectron2's own modules on the CPU (reference
detectron2/modeling/meta_arch/semantic_seg.py `SemSegFPNHead.losses`, `SemanticSegmentor.forward`, panoptic_fpn.py
`PanopticFPN.forward`).  Runs only where the reference tree exists (as scripts/make_golden_panoptic.py, whose builders it uses).  Only
data is stored; weights, images, pyramids and label maps are regenerated from their seeds (lvc_amd.utils.synthetic).  TEST
INFRASTRUCTURE ONLY.

  sem_seg_head_train.npz     (a) `SemSegFPNHead` (GN, 128 channels, 54 classes) in training mode on `synthetic.sem_seg_pyramid(seed 0)`
                             against `synthetic.sem_seg_label_map(5, 128, 192)`; weights `conditioned_sem_seg_head_state_dict(seed 0)`
  sem_seg_model_train.npz    (b) one `SemanticSegmentor` step (R50-FPN, FREEZE_AT 2) on the two small fixture images (128x160, 120x176)
                             with `sem_seg_label_map(seed, h, w)` of each; weights `conditioned_panoptic_state_dict(seed 0)`, of which
                             the model has the trunk's and the semantic head's
  panoptic_train.npz         (c) one `PanopticFPN` step (20 thing / 54 stuff classes, FREEZE_AT 2, BATCH_SIZE_PER_IMAGE 128, identity
                             randperm) on the same images, the ground truth of mask_train.npz (scripts/make_golden_mask_train.py) and
                             the same label maps
Each holds:
  loss.<name>, loss64.<name>, loss_dev.<name>       the losses of the fp32 model, of the model run as .double(), and |difference|
  frozen_names, grad_sample.<name>, grad_stats.<name>      as tests/golden/mask_train.npz (sum, norm, stride of every trainable gradient);
                             (a) also holds the gradients of the four input features as `grad_sample.feature.p2` .. `feature.p5`
  (c) gt_boxes{i}, gt_classes{i}, gt_masks{i}       the ground truth, as mask_train.npz

    python scripts/make_golden_panoptic_train.py [head] [segmentor] [panoptic]
"""
import copy
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden_panoptic as mgp  # noqa: E402  (installs the import shim through oracle.make_golden)
from oracle import make_golden as mg  # noqa: E402

from lvc_amd.utils import synthetic as syn  # noqa: E402

BATCH_SIZE_PER_IMAGE = 128
HEAD_LABEL_SEED = 5


def _grads(d, named, prefix=""):
    for name, t in named:
        gflat = t.flatten()
        stride = max(1, gflat.numel() // 2048) | 1
        d["grad_sample." + prefix + name] = gflat[::stride][:2048].clone()
        d["grad_stats." + prefix + name] = torch.tensor([float(gflat.double().sum()), float(gflat.double().norm()), float(stride)],
                                                        dtype=torch.float64)


def _param_grads(d, model):
    frozen = []
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None, name
            _grads(d, [(name, p.grad)])
        else:
            frozen.append(name)
    d["frozen_names"] = np.array(frozen)


def _losses(d, losses, losses64):
    for k, v in losses.items():
        d["loss." + k] = v.detach()
        d["loss64." + k] = losses64[k].detach()
        d["loss_dev." + k] = np.float64(abs(float(v.detach()) - float(losses64[k])))
    print("  losses", {k: float(v) for k, v in losses.items()})
    print("  fp64  ", {k: float(v) for k, v in losses64.items()})


def _save(name, d):
    mg.save(name, **d)
    size = os.path.getsize(os.path.join(mg.GOLD, name + ".npz"))
    assert size <= (1 << 20), "fixture of %d bytes: the repository's limit for a committed file is 1 MiB" % size
    print(name + ".npz", size, "bytes")


# ------------------------------------------------------------------------------------------------ (a) the head alone
def gen_head():
    head = mgp.build_head(54).train()
    head.load_state_dict(syn.conditioned_sem_seg_head_state_dict(head.state_dict(), seed=0), strict=True)
    head64 = copy.deepcopy(head).double()
    feats = {k: v.requires_grad_() for k, v in syn.sem_seg_pyramid(seed=0).items()}
    target = syn.sem_seg_label_map(HEAD_LABEL_SEED, 128, 192, 54, head.ignore_value)[None]
    _, losses = head(feats, target)
    sum(losses.values()).backward()
    with torch.no_grad():
        _, losses64 = head64({k: v.detach().double() for k, v in feats.items()}, target)
    d = {}
    _losses(d, losses, losses64)
    _param_grads(d, head)
    _grads(d, [(k, v.grad) for k, v in feats.items()], prefix="feature.")
    d["valid"] = np.int64(int((target != head.ignore_value).sum()))
    _save("sem_seg_head_train", d)


# ------------------------------------------------------------------------------------------------ (b), (c) the models
def _batch(gt=None, dtype=torch.float32, ignore_value=255):
    from detectron2.structures import BitMasks, Boxes, Instances

    batch = []
    for i, (h, w, seed) in enumerate(mgp.SIZES):
        item = {"image": syn.synthetic_image(seed, h, w).to(dtype), "height": h, "width": w,
                "sem_seg": syn.sem_seg_label_map(seed, h, w, 54, ignore_value)}
        if gt is not None:
            boxes, classes, masks = gt[i]
            inst = Instances((h, w))
            inst.gt_boxes = Boxes(boxes.clone())
            inst.gt_classes = classes.clone()
            inst.gt_masks = BitMasks(masks.clone())
            item["instances"] = inst
        batch.append(item)
    return batch


def gen_segmentor():
    from detectron2.modeling.meta_arch.semantic_seg import SemanticSegmentor
    from lvc.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(mg.refshim.REF_ROOT, "configs", mgp.YAML))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.META_ARCHITECTURE", "SemanticSegmentor", "MODEL.SEM_SEG_HEAD.NUM_CLASSES", 54])
    model = SemanticSegmentor(cfg).train()
    pan = mgp.build_panoptic(20, 54, topk=20)
    full = syn.conditioned_panoptic_state_dict(pan.state_dict(), seed=0)
    sd = model.state_dict()
    model.load_state_dict({k: full[k] if k in full else v for k, v in sd.items()}, strict=True)
    assert all(k in full for k in sd if k not in ("pixel_mean", "pixel_std"))
    model64 = copy.deepcopy(model).double()
    losses = model(_batch())
    sum(losses.values()).backward()
    with torch.no_grad():
        losses64 = model64(_batch(dtype=torch.float64))
    d = {}
    _losses(d, losses, losses64)
    _param_grads(d, model)
    _save("sem_seg_model_train", d)


def gen_panoptic():
    import make_golden_mask_train as mgt
    from detectron2.layers.roi_align import ROIAlign
    from detectron2.utils.events import EventStorage

    torch.randperm = lambda n, **kw: torch.arange(n, **{k: v for k, v in kw.items() if k in ("device", "dtype")})
    model = mgp.build_panoptic(20, 54, topk=20)
    model.roi_heads.batch_size_per_image = BATCH_SIZE_PER_IMAGE
    model.load_state_dict(syn.conditioned_panoptic_state_dict(model.state_dict(), seed=0), strict=True)
    model.train()
    model64 = copy.deepcopy(model).double()
    for m in list(model64.modules()):      # the poolers hand ROIAlign fp32 rois whatever the maps' dtype: the native op wants one dtype
        if isinstance(m, ROIAlign):
            m.register_forward_pre_hook(lambda mod, args: (args[0], args[1].to(args[0].dtype)))
    gt = mgt.ground_truth()
    d = {}
    for i, (boxes, classes, masks) in enumerate(gt):
        d["gt_boxes%d" % i], d["gt_classes%d" % i] = boxes, classes
        d["gt_masks%d" % i] = np.packbits(masks.numpy().astype(np.uint8))
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    try:
        with EventStorage(0) as storage:
            losses = model(_batch(gt))
            sum(losses.values()).backward()
            scalars = {k: float(v) for k, v in storage.latest().items()}
        torch.nn.functional.binary_cross_entropy_with_logits = lambda x, t, *a, **k: bce(x, t.to(x.dtype), *a, **k)
        with EventStorage(0), torch.no_grad():
            losses64 = model64(_batch(gt, torch.float64))
    finally:
        torch.nn.functional.binary_cross_entropy_with_logits = bce
    _losses(d, losses, losses64)
    d["instance_loss_weight"] = np.float64(model.instance_loss_weight)
    for k, v in scalars.items():
        d["scalar." + k.replace("/", ".")] = np.float64(v)
    assert scalars["roi_head/num_fg_samples"] + scalars["roi_head/num_bg_samples"] == BATCH_SIZE_PER_IMAGE, "an image missed its RoI quota"
    _param_grads(d, model)
    _save("panoptic_train", d)


if __name__ == "__main__":
    torch.manual_seed(0)
    what = sys.argv[1:] or ["head", "segmentor", "panoptic"]
    if "head" in what:
        gen_head()
    if "segmentor" in what:
        gen_segmentor()
    if "panoptic" in what:
        gen_panoptic()
