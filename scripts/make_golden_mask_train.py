"""Generate tests/golden/mask_train.npz: one training step of detectron2's Mask R-CNN (reference detectron2/modeling/meta_arch/rcnn.py
`GeneralizedRCNN.forward`, roi_heads.py `StandardROIHeads._forward_mask` + `select_foreground_proposals`, mask_head.py `mask_rcnn_loss`,
structures/masks.py `BitMasks.crop_and_resize`) run on the CPU.  Runs only where the reference tree exists (as
scripts/make_golden_mask_rcnn.py, whose import shim it uses).  Only data is stored; images and weights are regenerated from their seeds
(lvc_amd.utils.synthetic).  TEST INFRASTRUCTURE ONLY.

Model: R50-FPN Mask R-CNN, 20 classes, default FREEZE_AT 2, ROI_HEADS.BATCH_SIZE_PER_IMAGE 128 (at most 32 foreground rows per image; both
images fill the quota), weights `conditioned_mask_rcnn_state_dict(seed=0)`, the two images of mask_rcnn_small.npz (128x160, 120x176),
`torch.randperm` patched to arange as in the other step fixtures.

  gt_boxes{i}, gt_classes{i}, gt_masks{i}        the ground truth; gt_masks: np.packbits of [n, H, W] (unions of two ellipses inside the box)
  fg_boxes{i}, fg_classes{i}, fg_matched{i}      the sampled foreground rows of image i, in order: box, class, index of the matched gt
  fg_logits                                      the fp32 step's mask logits of each row's ground-truth class [n_fg0 + n_fg1, 28, 28]
  targets{i}                                     np.packbits of the reference's targets [n_fg, 28, 28] (BitMasks.crop_and_resize, fp32)
  band{i}                                        packbits: pixels whose fp64 average (tests/mask_train_ref.py) lies within 3 x target_dev of 0.5
  target_dev                                     max |fp32 - fp64| of the averages;  band_share: band pixels / target pixels
  loss.<name>, loss64.<name>                     the five losses of the fp32 model, and of the model run as .double()
  loss_dev.<name>                                |loss - loss64|: the reference's own fp32-vs-fp64 deviation
  scalar.<name>                                  the EventStorage scalars of the fp32 step ('/' written as '.')
  frozen_names, grad_sample.<name>, grad_stats.<name>      as tests/golden/retinanet_train.npz (sum, norm, stride of every trainable gradient)
The script fails if the reference's fp32 targets disagree with the fp64 restatement on a pixel outside the band, or if the band holds
more than 0.1 % of the target pixels.

    python scripts/make_golden_mask_train.py
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

import make_golden_mask_rcnn as mgm  # noqa: E402  (installs the import shim through oracle.make_golden)
from oracle import make_golden as mg  # noqa: E402

import mask_train_ref as R  # noqa: E402
from lvc_amd.utils import synthetic as syn  # noqa: E402

BATCH_SIZE_PER_IMAGE = 128
CAP = 1e-3
SIDE = 28


def build():
    from detectron2.modeling.meta_arch.rcnn import GeneralizedRCNN
    from lvc.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(mg.refshim.REF_ROOT, "configs", mgm.YAML))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.META_ARCHITECTURE", "GeneralizedRCNN", "MODEL.MASK_ON", True,
                         "MODEL.ROI_MASK_HEAD.NAME", "MaskRCNNConvUpsampleHead", "MODEL.ROI_MASK_HEAD.NUM_CONV", 4,
                         "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", 14, "MODEL.ROI_HEADS.NUM_CLASSES", mgm.NUM_CLASSES,
                         "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", BATCH_SIZE_PER_IMAGE])
    return GeneralizedRCNN(cfg)


def ground_truth():
    """Per image: boxes (the generator of make_golden_retinanet_train.gt_case_a, seed 9: 3 and 4 boxes), classes, and for every box the
    union of two ellipses inside it."""
    g = torch.Generator().manual_seed(9)
    out = []
    for i, (h, w, _seed) in enumerate(mgm.SIZES):
        n = 3 + i
        x0, y0 = torch.rand(n, generator=g) * (w - 60), torch.rand(n, generator=g) * (h - 60)
        bw, bh = 24 + torch.rand(n, generator=g) * 36, 24 + torch.rand(n, generator=g) * 36
        boxes = torch.stack([x0, y0, x0 + bw, y0 + bh], 1)
        classes = torch.randint(0, mgm.NUM_CLASSES, (n,), generator=g)
        yy, xx = torch.arange(h, dtype=torch.float32)[:, None] + 0.5, torch.arange(w, dtype=torch.float32)[None, :] + 0.5
        masks = torch.zeros(n, h, w, dtype=torch.bool)
        for j in range(n):
            for _ in range(2):
                r = torch.rand(4, generator=g)
                cx, cy = float(x0[j] + bw[j] * (0.3 + 0.4 * r[0])), float(y0[j] + bh[j] * (0.3 + 0.4 * r[1]))
                rx, ry = float(bw[j] * (0.15 + 0.15 * r[2])), float(bh[j] * (0.15 + 0.15 * r[3]))
                masks[j] |= ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0
        out.append((boxes, classes, masks))
    return out


def batch_of(gt, dtype=torch.float32):
    from detectron2.structures import BitMasks, Boxes, Instances

    batch = []
    for (h, w, seed), (boxes, classes, masks) in zip(mgm.SIZES, gt):
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(boxes.clone())
        inst.gt_classes = classes.clone()
        inst.gt_masks = BitMasks(masks.clone())
        batch.append({"image": syn.synthetic_image(seed, h, w).to(dtype), "instances": inst, "height": h, "width": w})
    return batch


def main():
    import detectron2.modeling.roi_heads.mask_head as ref_mh
    from detectron2.layers.roi_align import ROIAlign
    from detectron2.utils.events import EventStorage

    torch.randperm = lambda n, **kw: torch.arange(n, **{k: v for k, v in kw.items() if k in ("device", "dtype")})
    model = build()
    model.load_state_dict(syn.conditioned_mask_rcnn_state_dict(model.state_dict(), seed=0), strict=True)
    model.train()
    model64 = copy.deepcopy(model).double()
    for m in list(model64.modules()):      # the poolers hand ROIAlign fp32 rois whatever the maps' dtype: the native op wants one dtype
        if isinstance(m, ROIAlign):
            m.register_forward_pre_hook(lambda mod, args: (args[0], args[1].to(args[0].dtype)))
    gt = ground_truth()
    d = {}
    for i, (boxes, classes, masks) in enumerate(gt):
        d["gt_boxes%d" % i], d["gt_classes%d" % i] = boxes, classes
        d["gt_masks%d" % i] = np.packbits(masks.numpy().astype(np.uint8))

    seen, logits = [], []
    loss_fn = ref_mh.mask_rcnn_loss

    def spy(pred_mask_logits, instances, vis_period=0):
        seen.append(instances)
        logits.append(pred_mask_logits.detach())
        return loss_fn(pred_mask_logits, instances, vis_period)

    ref_mh.mask_rcnn_loss = spy
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    try:
        with EventStorage(0) as storage:
            losses = model(batch_of(gt))
            sum(losses.values()).backward()
            scalars = {k: float(v) for k, v in storage.latest().items()}
        # the fp64 run: the targets stay the fp32 model's (crop_and_resize converts the planes to fp32 whatever the model's dtype)
        torch.nn.functional.binary_cross_entropy_with_logits = lambda x, t, *a, **k: bce(x, t.to(x.dtype), *a, **k)
        with EventStorage(0), torch.no_grad():
            losses64 = model64(batch_of(gt, torch.float64))
    finally:
        ref_mh.mask_rcnn_loss = loss_fn
        torch.nn.functional.binary_cross_entropy_with_logits = bce

    # ---- the sampled foreground rows and their targets
    instances = seen[0]
    n_band = n_pix = 0
    devs = []
    for i, (inst, (boxes, classes, masks)) in enumerate(zip(instances, gt)):
        fb = inst.proposal_boxes.tensor.detach()
        matched = (inst.gt_boxes.tensor[:, None, :] - boxes[None, :, :]).abs().sum(2).argmin(1)
        assert torch.equal(boxes[matched], inst.gt_boxes.tensor) and torch.equal(classes[matched], inst.gt_classes)
        assert torch.equal(inst.gt_masks.tensor, masks[matched])
        tg = inst.gt_masks.crop_and_resize(fb, SIDE)
        bits, band, dev, bits32 = R.targets(list(masks[matched]), fb, SIDE)
        assert torch.equal(bits32, tg), "the fp32 restatement is not the reference's ROIAlign on image %d" % i
        assert not bool(((bits != tg) & ~band).any()), "fp32 and fp64 targets disagree outside the band on image %d" % i
        devs.append(dev)
        d["fg_boxes%d" % i], d["fg_classes%d" % i], d["fg_matched%d" % i] = fb, inst.gt_classes.clone(), matched.to(torch.int32)
        d["targets%d" % i] = np.packbits(tg.numpy().astype(np.uint8))
        n_pix += tg.numel()
        print("  image %d: %d foreground rows of %d sampled, %d positive target pixels" % (i, len(fb), BATCH_SIZE_PER_IMAGE, int(tg.sum())))
    d["target_dev"] = np.float64(max(devs))
    gcls = torch.cat([inst.gt_classes for inst in instances])
    d["fg_logits"] = logits[0][torch.arange(len(gcls)), gcls].float().clone()      # the ground-truth class's logits of the fp32 step
    for i, (inst, (boxes, classes, masks)) in enumerate(zip(instances, gt)):      # one band for the batch: 3 x the largest deviation
        matched = d["fg_matched%d" % i].long()
        a64 = torch.stack([R.target_average(masks[m], b, SIDE) for m, b in zip(matched, d["fg_boxes%d" % i])])
        band = (a64 - 0.5).abs() <= 3 * float(d["target_dev"])
        n_band += int(band.sum())
        d["band%d" % i] = np.packbits(band.numpy().astype(np.uint8))
    d["band_share"] = np.float64(n_band / max(n_pix, 1))
    print("  targets: deviation %.3e, band %d of %d pixels (%.4f %%)" % (d["target_dev"], n_band, n_pix, 100 * d["band_share"]))
    assert d["band_share"] <= CAP, "band share %.5f above the cap %.5f" % (d["band_share"], CAP)

    # ---- losses, scalars, gradients
    for k, v in losses.items():
        d["loss." + k] = v.detach()
        d["loss64." + k] = losses64[k].detach()
        d["loss_dev." + k] = np.float64(abs(float(v) - float(losses64[k])))
    for k, v in scalars.items():
        d["scalar." + k.replace("/", ".")] = np.float64(v)
    frozen, trainable = [], 0
    for n_, p_ in model.named_parameters():
        if p_.requires_grad:
            trainable += 1
            gflat = p_.grad.flatten()
            stride = max(1, gflat.numel() // 2048) | 1
            d["grad_sample." + n_] = gflat[::stride][:2048].clone()
            d["grad_stats." + n_] = torch.tensor([float(gflat.double().sum()), float(gflat.double().norm()), float(stride)], dtype=torch.float64)
        else:
            frozen.append(n_)
    d["frozen_names"] = np.array(frozen)
    print("  losses", {k: float(v) for k, v in losses.items()})
    print("  fp64  ", {k: float(v) for k, v in losses64.items()})
    print("  scalars", scalars, "trainable", trainable, "frozen", len(frozen))
    assert scalars["roi_head/num_fg_samples"] + scalars["roi_head/num_bg_samples"] == BATCH_SIZE_PER_IMAGE, "an image missed its RoI quota"
    assert all(len(i) >= 4 for i in instances), "too few foreground rows"
    mg.save("mask_train", **d)
    size = os.path.getsize(os.path.join(mg.GOLD, "mask_train.npz"))
    assert size <= (1 << 20), "fixture of %d bytes: the repository's limit for a committed file is 1 MiB" % size
    print("mask_train.npz", size, "bytes")


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
