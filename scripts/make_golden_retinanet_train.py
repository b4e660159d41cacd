"""Generate tests/golden/retinanet_train.npz: one training step of detectron2's RetinaNet (reference
detectron2/modeling/meta_arch/retinanet.py:128-282 `forward`, `losses`, `label_anchors`) run on the CPU.  Runs only where the reference
tree exists (as scripts/make_golden_retinanet.py, whose model builder and import shim it uses).  Only data is stored; images and weights
are regenerated from their seeds (lvc_amd.utils.synthetic).  TEST INFRASTRUCTURE ONLY.

The shim's `fvcore.nn.sigmoid_focal_loss_jit` is a placeholder, so fvcore's published definition of `sigmoid_focal_loss` is restated here
(as scripts/make_golden_lsj.py restates fvcore's transforms) and assigned to the name the reference module calls.

Model: R50, 20 classes, default FREEZE_AT 2, weights `conditioned_retinanet_state_dict(seed=0)`, the inference fixture's two images
(128x160, 120x176; batch padded to 128x192: R = 4608 anchors per image).

  case "a" (one whole step): gt boxes from the generator of make_golden_resnet_d.gen_train (seed 9: 3 and 4 boxes)
      a_gt_boxes{0,1}, a_gt_classes{0,1}      the ground truth
      a_gt_labels int8 [2,4608]               `label_anchors`: -1 ignored, 0..19 class, 20 background
      a_matched int16 [2,4608]                index of the matched gt box on positive rows, -1 elsewhere
      loss.{loss_cls,loss_box_reg}            fp32;  loss64.* the model run as .double()
      normalizer [2] float64                  `loss_normalizer` after the first and after a second forward on the same batch
      num_pos [2]                             positives per image
      frozen_names, grad_sample.<name>, grad_stats.<name>      as tests/golden/resnet_d_train.npz
  case "b" (labels only): image 0 = case a's boxes + three boxes no anchor reaches IoU 0.4 with (positives only through
      allow_low_quality_matches, some of them equal-IoU ties); image 1 without gt
      b_gt_boxes0, b_gt_classes0, b_gt_labels int8 [2,4608], b_matched int16 [2,4608], b_low_quality (positives with best IoU < 0.5)

    python scripts/make_golden_retinanet_train.py
"""
import copy
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden_retinanet as mgr  # noqa: E402  (installs the import shim through oracle.make_golden)
from oracle import make_golden as mg  # noqa: E402

from lvc_amd.utils import synthetic as syn  # noqa: E402

EXTRA_B = [[50.3, 40.2, 56.1, 47.0], [20.5, 90.25, 150.0, 99.0], [100.0, 10.0, 108.0, 110.0]]


def sigmoid_focal_loss(inputs, targets, alpha=-1, gamma=2, reduction="none"):
    """fvcore.nn.sigmoid_focal_loss as published."""
    import torch.nn.functional as F

    p = torch.sigmoid(inputs)
    ce_loss = F.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce_loss * ((1 - p_t) ** gamma)
    if alpha >= 0:
        alpha_t = alpha * targets + (1 - alpha) * (1 - targets)
        loss = alpha_t * loss
    if reduction == "mean":
        loss = loss.mean()
    elif reduction == "sum":
        loss = loss.sum()
    return loss


def gt_case_a():
    from detectron2.structures import Boxes, Instances

    g = torch.Generator().manual_seed(9)
    out = []
    for i, (h, w, _seed) in enumerate(mgr.SIZES):
        n = 3 + i
        x0, y0 = torch.rand(n, generator=g) * (w - 60), torch.rand(n, generator=g) * (h - 60)
        bw, bh = 24 + torch.rand(n, generator=g) * 36, 24 + torch.rand(n, generator=g) * 36
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(torch.stack([x0, y0, x0 + bw, y0 + bh], 1))
        inst.gt_classes = torch.randint(0, 20, (n,), generator=g)
        out.append(inst)
    return out


def batch_of(insts):
    return [{"image": syn.synthetic_image(seed, h, w), "instances": inst, "height": h, "width": w}
            for (h, w, seed), inst in zip(mgr.SIZES, insts)]


def labels_of(model, insts):
    """(gt_labels int8 [N,R], matched gt index int16 [N,R] (-1 off the positives), best IoU per anchor list) by the reference's own
    label_anchors and Matcher."""
    from detectron2.structures import Boxes, pairwise_iou

    images = model.preprocess_image(batch_of(insts))
    with torch.no_grad():
        feats = model.backbone(images.tensor)
    anchors = model.anchor_generator([feats[f] for f in model.in_features])
    gt_labels, _boxes = model.label_anchors(anchors, insts)
    cat = Boxes.cat(anchors)
    matched, best = [], []
    for inst, lab in zip(insts, gt_labels):
        m = torch.full((len(cat),), -1, dtype=torch.int64)
        v = torch.zeros(len(cat))
        if len(inst):
            q = pairwise_iou(inst.gt_boxes, cat)
            idx, _ = model.anchor_matcher(q)
            pos = (lab >= 0) & (lab != model.num_classes)
            m[pos] = idx[pos]
            v = q.max(0)[0]
        matched.append(m)
        best.append(v)
    return torch.stack(gt_labels).to(torch.int8), torch.stack(matched).to(torch.int16), best


def main():
    import detectron2.modeling.meta_arch.retinanet as ref
    from detectron2.structures import Boxes, Instances
    from detectron2.utils.events import EventStorage

    ref.sigmoid_focal_loss_jit = sigmoid_focal_loss
    model = mgr.build(mgr.NUM_CLASSES)
    model.load_state_dict(syn.conditioned_retinanet_state_dict(model.state_dict(), seed=0), strict=True)
    model.train()
    K = model.num_classes
    d = {}

    # ---- case a
    insts = gt_case_a()
    for i, inst in enumerate(insts):
        d["a_gt_boxes%d" % i], d["a_gt_classes%d" % i] = inst.gt_boxes.tensor, inst.gt_classes
    lab, matched, best = labels_of(model, insts)
    d["a_gt_labels"], d["a_matched"] = lab, matched
    pos = (lab >= 0) & (lab != K)
    num_pos = [int(v) for v in pos.sum(1)]
    ignored = [int(v) for v in (lab < 0).sum(1)]
    d["num_pos"] = np.array(num_pos)
    model64 = copy.deepcopy(model).double()
    batch = batch_of(insts)
    with EventStorage(0):
        losses = model(batch)
        n1 = float(model.loss_normalizer)
        sum(losses.values()).backward()
        with torch.no_grad():
            model(batch)
        n2 = float(model.loss_normalizer)
        batch64 = [dict(b, image=b["image"].double()) for b in batch]
        with torch.no_grad():
            losses64 = model64(batch64)
    d["normalizer"] = np.array([n1, n2], dtype=np.float64)
    total = sum(num_pos)
    want1 = 0.9 * 100 + (1 - 0.9) * max(total, 1)
    want2 = 0.9 * want1 + (1 - 0.9) * max(total, 1)
    assert n1 == want1 and n2 == want2, (n1, want1, n2, want2)
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
    for k, v in losses.items():
        d["loss." + k] = v.detach()
    for k, v in losses64.items():
        d["loss64." + k] = v.detach()
    print("case a: positives", num_pos, "ignored", ignored, "losses", {k: float(v) for k, v in losses.items()},
          "fp64", {k: float(v) for k, v in losses64.items()}, "normalizer", n1, n2, "trainable", trainable, "frozen", len(frozen))
    best_pos = torch.cat([b[p] for b, p in zip(best, pos)])
    assert bool((best_pos >= 0.5).any()), "no positive at IoU >= 0.5"
    assert sum(ignored) >= 1, "no ignored anchor"

    # ---- case b
    inst0 = Instances(insts[0].image_size)
    inst0.gt_boxes = Boxes(torch.cat([insts[0].gt_boxes.tensor, torch.tensor(EXTRA_B)], 0))
    inst0.gt_classes = torch.cat([insts[0].gt_classes, torch.tensor([4, 11, 17])])
    inst1 = Instances(insts[1].image_size)
    inst1.gt_boxes = Boxes(torch.zeros(0, 4))
    inst1.gt_classes = torch.zeros(0, dtype=torch.int64)
    lab_b, matched_b, best_b = labels_of(model, [inst0, inst1])
    d["b_gt_boxes0"], d["b_gt_classes0"] = inst0.gt_boxes.tensor, inst0.gt_classes
    d["b_gt_labels"], d["b_matched"] = lab_b, matched_b
    pos_b = (lab_b >= 0) & (lab_b != K)
    low = int((best_b[0][pos_b[0]] < 0.5).sum())          # positive only through allow_low_quality_matches
    below = int((best_b[0][pos_b[0]] < 0.4).sum())
    d["b_low_quality"] = np.array(low)
    print("case b: positives", [int(v) for v in pos_b.sum(1)], "of which only through low-quality matches:", low, "(best IoU < 0.4:", below,
          ") background on image 1:", int((lab_b[1] == K).sum()))
    assert below >= 1, "no positive with best IoU < 0.4"
    assert int(pos_b[1].sum()) == 0 and int((lab_b[1] == K).sum()) == lab_b.shape[1], "image 1 must have no positives"

    mg.save("retinanet_train", **d)
    size = os.path.getsize(os.path.join(mg.GOLD, "retinanet_train.npz"))
    assert size <= (1 << 20), "fixture of %d bytes: the repository's limit for a committed file is 1 MiB" % size
    print("retinanet_train.npz", size, "bytes")


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
