"""Times of one R50-RetinaNet training step (presets.retinanet_r_fpn, 80 classes, FREEZE_AT 2) for a batch of 8 synthetic 800 x 1333
images with 8 gt boxes each, on one device.  Medians of `--reps`, legs alternated in one process.  None of these is a gate.

  loss_pass / grad_pass   kernels.retinanet_loss (streaming pass + finish) and kernels.retinanet_loss_grad alone on the step's own head
                          outputs: us, against the byte counts at the 6.3 TB/s copy rate (one read of the logits and deltas for the loss;
                          that read plus one write of both gradients for the gradient pass)
  eager                   the same loss and gradient in eager PyTorch as the reference writes them (retinanet.py:184-236: stack, cat,
                          boolean-mask gathers, one_hot, .item(), sigmoid_focal_loss, smooth_l1_loss, autograd backward) on the same device
                          tensors -- the yardstick
  step                    model(batch) + backward of the summed losses (wall clock, synchronised): img/s; and, each alone on the step's
                          tensors: the head forward under autograd, labelling + loss, the head backward (loss gradient included)

Writes profiles/retinanet_train_bench.json and prints it as one JSON line.

    python scripts/bench_retinanet_train.py [--reps 20] [--warmup 3] [--out profiles/retinanet_train_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

COPY_GBPS = 6300.0      # the copy rate the README uses


def _alternate(legs, reps, warmup):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in legs}
    for i in range(warmup + reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            start.record()
            fn()
            end.record()
            end.synchronize()
            if i >= warmup:
                times[k].append(start.elapsed_time(end))
    return {k: statistics.median(v) for k, v in times.items()}


def eager_losses(anchors, pred_logits, gt_labels, pred_anchor_deltas, gt_boxes, num_classes, alpha, gamma, beta, normalizer):
    """RetinaNet.losses as the reference writes it, with fvcore's two losses and Box2BoxTransform.get_deltas (weights 1) inline."""
    gt_labels = torch.stack(gt_labels)
    sw, sh = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    scx, scy = anchors[:, 0] + 0.5 * sw, anchors[:, 1] + 0.5 * sh
    tgt = []
    for k in gt_boxes:
        tw, th = k[:, 2] - k[:, 0], k[:, 3] - k[:, 1]
        tcx, tcy = k[:, 0] + 0.5 * tw, k[:, 1] + 0.5 * th
        tgt.append(torch.stack(((tcx - scx) / sw, (tcy - scy) / sh, torch.log(tw / sw), torch.log(th / sh)), dim=1))
    gt_anchor_deltas = torch.stack(tgt)
    valid_mask = gt_labels >= 0
    pos_mask = (gt_labels >= 0) & (gt_labels != num_classes)
    num_pos = pos_mask.sum().item()
    normalizer = 0.9 * normalizer + (1 - 0.9) * max(num_pos, 1)
    target = F.one_hot(gt_labels[valid_mask], num_classes=num_classes + 1)[:, :-1].to(pred_logits[0].dtype)
    x = torch.cat(pred_logits, dim=1)[valid_mask]
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, target, reduction="none")
    p_t = p * target + (1 - p) * (1 - target)
    loss = ce * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * target + (1 - alpha) * (1 - target)) * loss
    loss_cls = loss.sum()
    d = torch.cat(pred_anchor_deltas, dim=1)[pos_mask]
    n = (d - gt_anchor_deltas[pos_mask]).abs()
    loss_box = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta).sum() if beta >= 1e-5 else n.sum()
    return loss_cls / normalizer, loss_box / normalizer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retinanet_train_bench.json"))
    args = ap.parse_args()

    from lvc_amd import kernels as K
    from lvc_amd.config.presets import retinanet_r_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.modeling.backbone.resnet import _as_nhwc4
    from lvc_amd.structures import Boxes, Instances
    from lvc_amd.utils import synthetic as syn
    from lvc_amd.utils.events import EventStorage

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    B, H, W, G = 8, 800, 1333, 8
    model = syn.conditioned_retinanet_(build_model(retinanet_r_fpn()), seed=0).enable_training().train()
    gen = torch.Generator().manual_seed(3)
    batch = []
    for i in range(B):
        x0, y0 = torch.rand(G, generator=gen) * (W - 420), torch.rand(G, generator=gen) * (H - 420)
        bw, bh = 24 + torch.rand(G, generator=gen) * 380, 24 + torch.rand(G, generator=gen) * 380
        inst = Instances((H, W))
        inst.gt_boxes = Boxes(torch.stack([x0, y0, x0 + bw, y0 + bh], 1).to(dev))
        inst.gt_classes = torch.randint(0, 80, (G,), generator=gen).to(dev)
        batch.append({"image": syn.synthetic_image(10 + i, H, W).to(dev), "instances": inst, "height": H, "width": W})
    result = {"batch": B, "image": [H, W], "classes": 80, "gt_per_image": G, "reps": args.reps, "copy_gbps": COPY_GBPS,
              "freeze_at": 2, "device": torch.cuda.get_device_name(0)}
    A, Kc = model.head.num_anchors, model.num_classes
    params = [p for p in model.parameters() if p.requires_grad]

    def zero_grads():
        for p in params:
            p.grad = None

    with EventStorage(0):
        # ---- (c) the whole step
        times = []
        for i in range(args.warmup + args.reps):
            zero_grads()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses = model(batch)
            sum(losses.values()).backward()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times.append(time.perf_counter() - t0)
        ms = 1e3 * statistics.median(times)
        result["step"] = {"ms_per_batch": ms, "img_per_s": B * 1e3 / ms, "losses": {k: float(v.detach()) for k, v in losses.items()},
                          "loss_normalizer": model.loss_normalizer}
        zero_grads()

        # ---- the step's tensors: pyramid features (detached), head outputs, labels
        with torch.no_grad():
            images = model.preprocess_image(batch)
            feats = model.backbone.forward_nhwc(_as_nhwc4(images.tensor))
        feats = [feats[f].detach() for f in model.in_features]
        gt_instances = [b["instances"] for b in batch]
        anchors = model._cat_anchors([(f.shape[1], f.shape[2]) for f in feats])
        gt, gt_off, _ = K.cat_ground_truth(gt_instances)
        gt_classes = torch.cat([g.gt_classes for g in gt_instances]).to(torch.int64).contiguous()
        matches, labels = K.match_boxes_batched(gt, gt_off, B, anchors, None, model.iou_thresholds, model.iou_labels, True)
        with torch.no_grad():
            logits, deltas = model.head.forward_train_nhwc(feats)
        result["levels"] = {name: list(t.shape[1:3]) for name, t in zip(model.in_features, logits)}
        result["anchors_per_image"] = int(anchors.shape[0])
        result["positives"] = int((labels == 1).sum())
        result["ignored"] = int((labels < 0).sum())
        entries = sum(t.numel() for t in logits)
        dentries = sum(t.numel() for t in deltas)
        result["logit_entries"] = entries

        # ---- (a) the two kernels alone
        pack = model._loss_pack(logits, deltas, anchors, matches, labels, gt, gt_classes, gt_off)
        n_in = torch.full((1,), 100.0, dtype=torch.float64, device=dev)
        n_out = torch.zeros(1, dtype=torch.float64, device=dev)
        one = torch.ones((), device=dev)
        dl = [torch.empty_like(t) for t in logits]
        dd = [torch.empty_like(t) for t in deltas]
        ours = K.retinanet_loss(pack, n_in, n_out)[0].clone()

        def loss_pass():
            K.retinanet_loss(pack, n_in, n_out)

        def grad_pass():
            K.retinanet_loss_grad(pack, n_out, one, one, dl, dd)

        # ---- (b) eager PyTorch, as the reference writes it, on the same tensors
        gt_labels, gt_boxes = model.label_anchors([Boxes(anchors)], gt_instances)
        pl = [t.reshape(B, -1, Kc).detach().requires_grad_(True) for t in logits]
        pd = [t.reshape(B, -1, 4).detach().requires_grad_(True) for t in deltas]
        eager_out = {}

        def eager_forward():
            with torch.no_grad():
                eager_out["l"] = eager_losses(anchors, pl, gt_labels, pd, gt_boxes, Kc, model.focal_loss_alpha, model.focal_loss_gamma,
                                              model.smooth_l1_loss_beta, 100.0)

        def eager_forward_backward():
            for t in pl + pd:
                t.grad = None
            lc, lb = eager_losses(anchors, pl, gt_labels, pd, gt_boxes, Kc, model.focal_loss_alpha, model.focal_loss_gamma,
                                  model.smooth_l1_loss_beta, 100.0)
            (lc + lb).backward()

        def ours_forward_backward():
            loss_pass()
            grad_pass()

        t = _alternate({"loss_pass": loss_pass, "grad_pass": grad_pass, "ours_forward_backward": ours_forward_backward,
                        "eager_forward": eager_forward, "eager_forward_backward": eager_forward_backward}, args.reps, args.warmup)
        read_bytes = 4.0 * (entries + dentries) + float(labels.numel()) * 5.0
        grad_bytes = read_bytes + 4.0 * (entries + dentries)
        result["loss_pass"] = {"us": 1e3 * t["loss_pass"], "bytes": read_bytes, "us_at_copy_rate": read_bytes / COPY_GBPS / 1e3,
                               "of_copy_rate": read_bytes / (t["loss_pass"] * 1e6) / COPY_GBPS, "launches": 2,
                               "loss_terms": "fp64"}
        result["grad_pass"] = {"us": 1e3 * t["grad_pass"], "bytes": grad_bytes, "us_at_copy_rate": grad_bytes / COPY_GBPS / 1e3,
                               "of_copy_rate": grad_bytes / (t["grad_pass"] * 1e6) / COPY_GBPS, "launches": 1, "gradient_terms": "fp32"}
        result["ours_forward_backward"] = {"us": 1e3 * t["ours_forward_backward"]}
        result["eager"] = {"forward_us": 1e3 * t["eager_forward"], "forward_backward_us": 1e3 * t["eager_forward_backward"],
                           "speedup_forward": t["eager_forward"] / t["loss_pass"],
                           "speedup_forward_backward": t["eager_forward_backward"] / t["ours_forward_backward"],
                           "losses": [float(v) for v in eager_out["l"]], "ours_losses": [float(v) for v in ours]}
        del pl, pd, eager_out

        # ---- the step's parts, each alone on the step's tensors
        fl = [f.detach().requires_grad_(True) for f in feats]
        state = {}

        def head_forward():
            state["out"] = model.head.forward_train_nhwc(fl)

        def label_and_loss():
            lg, dt = state["out"]
            m, lab = K.match_boxes_batched(gt, gt_off, B, anchors, None, model.iou_thresholds, model.iou_labels, True)
            pk = model._loss_pack(lg, dt, anchors, m, lab, gt, gt_classes, gt_off)
            from lvc_amd.modeling.meta_arch.retinanet import _RetinaNetLossFn

            lc, lb, _n = _RetinaNetLossFn.apply(pk, n_in, n_out, 0.9, 1 - 0.9, *lg, *dt)
            state["loss"] = lc + lb

        def head_backward():
            zero_grads()
            for f in fl:
                f.grad = None
            state["loss"].backward()

        t2 = _alternate({"head_forward": head_forward, "label_and_loss": label_and_loss, "head_backward": head_backward}, args.reps, args.warmup)
        result["step_parts_ms"] = {"head_forward": t2["head_forward"], "label_and_loss": t2["label_and_loss"],
                                   "head_backward_with_loss_gradient": t2["head_backward"],
                                   "rest_of_step (trunk and pyramid forward + backward, by difference)":
                                       ms - t2["head_forward"] - t2["label_and_loss"] - t2["head_backward"]}
        result["not_measured"] = ["the step under LossScaler / GradientBuckets", "an optimizer step", "the LSJ loader in front of the step",
                                  "bbox_pred under autograd against a padded 64-channel route (not built)"]

    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
