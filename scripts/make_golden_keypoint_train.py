"""Generate tests/golden/keypoint_train.npz: one training step of detectron2's Keypoint R-CNN (reference
detectron2/modeling/meta_arch/rcnn.py `GeneralizedRCNN.forward`, roi_heads.py `StandardROIHeads._forward_keypoint` +
`select_foreground_proposals` + `select_proposals_with_visible_keypoints`, keypoint_head.py `keypoint_rcnn_loss`,
structures/keypoints.py `Keypoints.to_heatmap`) run on the CPU.  Runs only where the reference tree exists (as
scripts/make_golden_keypoint_rcnn.py, whose import shim it uses).  Only data is stored; images and weights are regenerated from their
seeds (lvc_amd.utils.synthetic).  TEST INFRASTRUCTURE ONLY.

Model: R50-FPN Keypoint R-CNN, 1 class, default FREEZE_AT 2, ROI_HEADS.BATCH_SIZE_PER_IMAGE 128 (at most 32 foreground rows per
image), weights `conditioned_keypoint_rcnn_state_dict(seed=0)`, the two images of keypoint_rcnn_small.npz (128x160, 120x176),
`torch.randperm` patched to arange as in the other step fixtures.

  gt_boxes{i}, gt_classes{i}, gt_keypoints{i}    the ground truth; keypoints [n, 17, 3] = (x, y, v) from `synthetic_gt_keypoints`, then
                                                 moved off the bin borders (below)
  fg_boxes{i}, fg_matched{i}                     the sampled foreground rows of image i, in order: box, index of the matched gt
  selected{i}                                    select_proposals_with_visible_keypoints' choice among those rows (bool)
  targets{i}, valid{i}                           the reference's Keypoints.to_heatmap(fg_boxes, 56) of ALL foreground rows [n_fg, 17]
  near_share                                     valid entries within 1e-3 of a bin border / valid entries, over the rows whose box
                                                 the network computed (a row that IS a ground-truth box is an exact input: its clamp
                                                 x == x2 and its x == x1 are decided by equal bits): must be 0
  clamped, v1, v0, dropped                       how often the cases the fixture must hold occur
  loss.<name>, loss64.<name>                     the five losses of the fp32 model, and of the model run as .double()
  loss_dev.<name>                                |loss - loss64|: the reference's own fp32-vs-fp64 deviation
  scalar.<name>                                  the EventStorage scalars of the fp32 step ('/' written as '.')
  frozen_names, grad_sample.<name>, grad_stats.<name>      as tests/golden/mask_train.npz (sum, norm, stride of every trainable gradient)

The proposals do not depend on the keypoints, so a first forward pass records the foreground boxes and every keypoint that would lie
within 1e-3 of a bin border of one of them is redrawn (seeded) before the recorded step.  The script fails -- reseed -- unless every
image fills its quota of 128 rows, a foreground row is dropped by the selection, a valid entry uses the x == x2 or y == y2 clamp,
keypoints with v = 1 and v = 0 exist, near_share is 0 and loss_keypoint differs from ln(56 * 56) by more than 1 %.

    python scripts/make_golden_keypoint_train.py
"""
import copy
import math
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden_keypoint_rcnn as mgk  # noqa: E402  (installs the import shim through oracle.make_golden)
from oracle import make_golden as mg  # noqa: E402

from lvc_amd.utils import synthetic as syn  # noqa: E402

BATCH_SIZE_PER_IMAGE = 128
SIDE = 56
K = 17
SEED = 0
NEAR = 1e-3


def build():
    from detectron2.modeling.meta_arch.rcnn import GeneralizedRCNN
    from lvc.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(mg.refshim.REF_ROOT, "configs", mgk.YAML))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.META_ARCHITECTURE", "GeneralizedRCNN", "MODEL.KEYPOINT_ON", True,
                         "MODEL.MASK_ON", False, "MODEL.ROI_HEADS.NUM_CLASSES", 1,
                         "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", BATCH_SIZE_PER_IMAGE])
    return GeneralizedRCNN(cfg)


def ground_truth():
    """Per image: boxes (the generator of make_golden_mask_train.ground_truth, seed 9: 3 and 4 boxes), class 0, keypoints."""
    g = torch.Generator().manual_seed(9)
    out = []
    for i, (h, w, _seed) in enumerate(mgk.SIZES):
        n = 3 + i
        x0, y0 = torch.rand(n, generator=g) * (w - 60), torch.rand(n, generator=g) * (h - 60)
        bw, bh = 24 + torch.rand(n, generator=g) * 36, 24 + torch.rand(n, generator=g) * 36
        boxes = torch.stack([x0, y0, x0 + bw, y0 + bh], 1)
        out.append((boxes, torch.zeros(n, dtype=torch.int64), syn.synthetic_gt_keypoints(boxes, K, seed=SEED + i)))
    return out


def batch_of(gt, dtype=torch.float32):
    from detectron2.structures import Boxes, Instances, Keypoints

    batch = []
    for (h, w, seed), (boxes, classes, kps) in zip(mgk.SIZES, gt):
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(boxes.clone())
        inst.gt_classes = classes.clone()
        inst.gt_keypoints = Keypoints(kps.clone())
        batch.append({"image": syn.synthetic_image(seed, h, w).to(dtype), "instances": inst, "height": h, "width": w})
    return batch


def near_entries(kps, boxes, fb, matched):
    """(row, k) pairs of the foreground rows `fb` (not themselves ground-truth boxes) whose valid keypoint lies within NEAR of a bin border."""
    own = (fb[:, None, :] == boxes[None, :, :]).all(2).any(1)
    kp = kps[matched]
    sx = SIDE / (fb[:, 2] - fb[:, 0])
    sy = SIDE / (fb[:, 3] - fb[:, 1])
    x = (kp[:, :, 0] - fb[:, 0:1]) * sx[:, None]
    y = (kp[:, :, 1] - fb[:, 1:2]) * sy[:, None]
    inside = (x >= -NEAR) & (x <= SIDE + NEAR) & (y >= -NEAR) & (y <= SIDE + NEAR) & (kp[:, :, 2] > 0)
    near = ((x - x.round()).abs() <= NEAR) | ((y - y.round()).abs() <= NEAR)
    return (inside & near & ~own[:, None]).nonzero(), int((inside & ~own[:, None]).sum())


def main():
    import detectron2.modeling.roi_heads.roi_heads as ref_rh
    from detectron2.layers.roi_align import ROIAlign
    from detectron2.structures.keypoints import _keypoints_to_heatmap
    from detectron2.utils.events import EventStorage

    torch.randperm = lambda n, **kw: torch.arange(n, **{k: v for k, v in kw.items() if k in ("device", "dtype")})
    model = build()
    model.load_state_dict(syn.conditioned_keypoint_rcnn_state_dict(model.state_dict(), seed=0), strict=True)
    model.train()
    model64 = copy.deepcopy(model).double()
    for m in list(model64.modules()):      # the poolers hand ROIAlign fp32 rois whatever the maps' dtype: the native op wants one dtype
        if isinstance(m, ROIAlign):
            m.register_forward_pre_hook(lambda mod, args: (args[0], args[1].to(args[0].dtype)))
    gt = ground_truth()

    seen = []
    select = ref_rh.select_proposals_with_visible_keypoints

    def spy(proposals):
        out = select(proposals)
        seen.append((proposals, out))
        return out

    ref_rh.select_proposals_with_visible_keypoints = spy
    try:
        # ---- first pass: the foreground boxes (they do not depend on the keypoints); keypoints near a bin border are redrawn
        with EventStorage(0):      # (with autograd on, as the recorded step: without it the CPU convs take another path and the boxes' last bits move)
            model(batch_of(gt))
        first = seen.pop()[0]
        g = torch.Generator().manual_seed(1 + SEED)
        for i, (inst, (boxes, classes, kps)) in enumerate(zip(first, gt)):
            fb = inst.proposal_boxes.tensor.detach()
            matched = (inst.gt_boxes.tensor[:, None, :] - boxes[None, :, :]).abs().sum(2).argmin(1)
            for _ in range(200):
                bad, _n = near_entries(kps, boxes, fb, matched)
                if len(bad) == 0:
                    break
                for r, k in bad.tolist():
                    j = int(matched[r])
                    if k < 6:      # the planted edge points: only their free coordinate moves
                        free = 1 if k in (0, 2, 4) else 0
                        lo, hi = float(boxes[j, free]), float(boxes[j, free + 2])
                        kps[j, k, free] = lo + (0.02 + 0.96 * float(torch.rand((), generator=g))) * (hi - lo)
                    else:
                        u = 0.02 + 0.96 * torch.rand(2, generator=g)
                        kps[j, k, 0] = boxes[j, 0] + u[0] * (boxes[j, 2] - boxes[j, 0])
                        kps[j, k, 1] = boxes[j, 1] + u[1] * (boxes[j, 3] - boxes[j, 1])
            else:
                raise AssertionError("image %d: keypoints stay near a bin border; reseed" % i)
        # ---- the recorded step
        with EventStorage(0) as storage:
            losses = model(batch_of(gt))
            sum(losses.values()).backward()
            scalars = {k: float(v) for k, v in storage.latest().items()}
        with EventStorage(0), torch.no_grad():
            losses64 = model64(batch_of(gt, torch.float64))
    finally:
        ref_rh.select_proposals_with_visible_keypoints = select

    d = {}
    fg, chosen = seen[0]
    n_near = n_valid = clamped = dropped = 0
    for i, (inst, sel, (boxes, classes, kps)) in enumerate(zip(fg, chosen, gt)):
        d["gt_boxes%d" % i], d["gt_classes%d" % i], d["gt_keypoints%d" % i] = boxes, classes, kps
        fb = inst.proposal_boxes.tensor.detach()
        assert torch.equal(fb, first[i].proposal_boxes.tensor), "the foreground rows moved between the two passes"
        matched = (inst.gt_boxes.tensor[:, None, :] - boxes[None, :, :]).abs().sum(2).argmin(1)
        assert torch.equal(boxes[matched], inst.gt_boxes.tensor) and torch.equal(inst.gt_keypoints.tensor, kps[matched])
        kept = (fb[:, None, :] == sel.proposal_boxes.tensor[None, :, :]).all(2).any(1)
        assert int(kept.sum()) == len(sel)
        tg, vd = _keypoints_to_heatmap(kps[matched], fb, SIDE)
        bad, n = near_entries(kps, boxes, fb, matched)
        n_near += len(bad)
        n_valid += n
        kp = kps[matched]
        clamped += int((((kp[:, :, 0] == fb[:, 2:3]) | (kp[:, :, 1] == fb[:, 3:4])) & (vd > 0) & kept[:, None]).sum())
        dropped += int((~kept).sum())
        d["fg_boxes%d" % i], d["fg_matched%d" % i], d["selected%d" % i] = fb, matched.to(torch.int32), kept
        d["targets%d" % i], d["valid%d" % i] = tg.to(torch.int32), vd.to(torch.uint8)
        print("  image %d: %d foreground rows of %d sampled, %d selected, %d valid entries" % (i, len(fb), BATCH_SIZE_PER_IMAGE, len(sel), int((vd > 0)[kept].sum())))
    allk = torch.cat([k for _b, _c, k in gt])
    d["near_share"] = np.float64(n_near / max(n_valid, 1))
    d["clamped"], d["dropped"] = np.int64(clamped), np.int64(dropped)
    d["v1"], d["v0"] = np.int64(int((allk[:, :, 2] == 1).sum())), np.int64(int((allk[:, :, 2] == 0).sum()))
    print("  near %d of %d, clamped %d, dropped %d, v1 %d, v0 %d" % (n_near, n_valid, clamped, dropped, d["v1"], d["v0"]))

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
    assert dropped >= 1, "no foreground row is dropped by the selection; reseed"
    assert clamped >= 1, "no valid entry uses the x == x2 / y == y2 clamp; reseed"
    assert d["v1"] >= 1 and d["v0"] >= 1, "the keypoints lack v = 1 or v = 0; reseed"
    assert n_near == 0 and d["near_share"] == 0.0, "valid entries within %g of a bin border" % NEAR
    flat = math.log(SIDE * SIDE)
    assert abs(float(losses["loss_keypoint"]) - flat) > 0.01 * flat, "loss_keypoint %.5f is the flat logits' ln(56^2) = %.5f" % (float(losses["loss_keypoint"]), flat)
    mg.save("keypoint_train", **d)
    size = os.path.getsize(os.path.join(mg.GOLD, "keypoint_train.npz"))
    assert size <= (1 << 20), "fixture of %d bytes: the repository's limit for a committed file is 1 MiB" % size
    print("keypoint_train.npz", size, "bytes")


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
