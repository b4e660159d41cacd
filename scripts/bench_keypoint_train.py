"""Times of the keypoint branch of R50-FPN Keypoint R-CNN TRAINING (presets.keypoint_rcnn_fpn) at the workload's own shape: 2 images x
128 foreground RoIs, M = 256 rows, S = 14, Cin = 512, K = 17, on one device.  None of these is a gate; no ratio is fixed in advance.

  tail        `KeypointTailLoss` forward + backward (score_lowres, loss, loss gradient, dx, dW / db) beside PyTorch-ROCm's autograd of
              conv_transpose2d + interpolate(bilinear x2) + cross_entropy(sum) / n on the same GPU and the same operands.  The two legs
              are timed as interleaved PAIRS (ours, torch, ours, torch, ...) with device events after a warm-up; every pair goes to the
              pairs file, and median, minimum and maximum of each leg are reported.
  parts       medians of the single launches of our leg (each timed alone, alternated): forward deconv, loss, loss gradient, dx, wgrad
  targets     lvc_keypoint_targets for the 2 x 128 rows
  step        one training step (forward + backward, wall clock, synchronised) of the keypoint model with enable_keypoint_training() and
              of the box-only model on the same trunk, RPN and box-head weights and the same boxes, alternated in one loop

Writes profiles/keypoint_train_bench.json and profiles/keypoint_train_bench_pairs.txt and prints the result as one JSON line.

    python scripts/bench_keypoint_train.py [--reps 30] [--warmup 5] [--out profiles/keypoint_train_bench.json]
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


def _spread(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def _pairs(legs, reps, warmup):
    """legs: name -> fn, run in turn `warmup + reps` times; device events around each call -> name -> list of ms (the timed reps, in order)."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in legs}
    for i in range(warmup + reps):
        for k, fn in legs.items():
            start.record()
            fn()
            end.record()
            end.synchronize()
            if i >= warmup:
                times[k].append(start.elapsed_time(end))
    return times


def _steps(legs, reps, warmup):
    from lvc_amd.utils.events import EventStorage

    times, last = {k: [] for k in legs}, {}
    with EventStorage(0):
        for i in range(warmup + reps):
            for k, (model, batch) in legs.items():
                for p in model.parameters():
                    p.grad = None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                losses = model(batch)
                sum(losses.values()).backward()
                torch.cuda.synchronize()
                if i >= warmup:
                    times[k].append(1e3 * (time.perf_counter() - t0))
                last[k] = {n: float(v.detach()) for n, v in losses.items()}
    return times, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoint_train_bench.json"))
    args = ap.parse_args()

    from lvc_amd import kernels as K
    from lvc_amd.config.presets import base_rcnn_fpn, keypoint_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.modeling.roi_heads.keypoint_head import KeypointTailLoss
    from lvc_amd.structures import Boxes, Instances, Keypoints
    from lvc_amd.utils import synthetic as syn

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    B, R, H, W, S, C, NK, NG = 2, 128, 800, 1333, 14, 512, 17, 20
    M = B * R
    side = 4 * S
    result = {"batch": B, "rois_per_image": R, "rows": M, "S": S, "Cin": C, "keypoints": NK, "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "not_measured": []}
    g = torch.Generator().manual_seed(0)

    # ---- ground truth and sampled rows
    gts = []
    for b in range(B):
        wh = 32 + 368 * torch.rand(NG, 2, generator=g)
        xy = torch.rand(NG, 2, generator=g) * (torch.tensor([W, H]) - wh)
        gb = torch.cat([xy, xy + wh], 1)
        gts.append((gb, syn.synthetic_gt_keypoints(gb, NK, seed=b)))
    matched = torch.randint(0, NG, (B, R), generator=g)
    boxes = torch.stack([gts[b][0][matched[b]] for b in range(B)])
    boxes = boxes + (torch.rand(B, R, 4, generator=g) - 0.5) * 0.2 * (boxes[:, :, 2:] - boxes[:, :, :2]).repeat(1, 1, 2)
    d_boxes, d_matched = boxes.to(dev).contiguous(), matched.to(dev)
    count = torch.full((B,), R, dtype=torch.int32, device=dev)
    kps = [gts[b][1].to(dev) for b in range(B)]

    def targets():
        return K.keypoint_targets(d_boxes, d_matched, count, kps, side)

    target, valid, _sel, sel_count = targets()
    result["valid_entries"] = int(valid.sum())
    result["selected_rows"] = sel_count.tolist()

    # ---- the tail's operands
    x, w, b_, _ = syn.keypoint_head_case(M, S, C, NK)
    xn = x.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_()
    x_nchw = x.to(dev).requires_grad_()
    wd, bd = w.to(dev).requires_grad_(), b_.to(dev).requires_grad_()
    wt, bt = w.to(dev).requires_grad_(), b_.to(dev).requires_grad_()
    packed, packed_dx = K.pack_keypoint_deconv(wd), K.pack_keypoint_deconv_dx(wd)
    vidx = valid.view(-1).nonzero().squeeze(1)
    tsel = target.view(-1).long()[vidx]
    nvalid = float(len(vidx))

    def ours():
        loss, _t, _c = KeypointTailLoss.apply(xn, wd, bd, target, valid, None, None, None, 1.0, packed, packed_dx)
        return torch.autograd.grad(loss, (xn, wd, bd))

    def theirs():
        z = F.interpolate(F.conv_transpose2d(x_nchw, wt, bt, stride=2, padding=1), scale_factor=2, mode="bilinear", align_corners=False)
        loss = F.cross_entropy(z.view(M * NK, -1)[vidx], tsel, reduction="sum") / nvalid
        return torch.autograd.grad(loss, (x_nchw, wt, bt))

    a, t = ours(), theirs()
    result["tail_max_rel_diff_from_torch"] = {
        k: float((u.reshape(v.shape) - v).abs().max() / v.abs().max().clamp_min(1e-30))
        for k, u, v in zip(("dx", "dW"), (a[0].permute(0, 3, 1, 2), a[1]), t[:2])}
    result["tail_db_abs"] = {"ours": float(a[2].abs().max()), "torch": float(t[2].abs().max()), "note": "analytically zero: rounding residue"}
    del a, t
    pair_times = _pairs({"ours": ours, "torch": theirs}, args.reps, args.warmup)
    result["tail"] = {"ours": _spread(pair_times["ours"]), "torch": _spread(pair_times["torch"]),
                      "ours_over_torch_median": statistics.median(pair_times["ours"]) / statistics.median(pair_times["torch"])}

    # ---- the launches of our leg, each alone
    with torch.no_grad():
        xd = xn.detach()
        low = K.keypoint_deconv(xd, packed, bd.detach(), NK)
        _l, _t, cnt, _term, pmax, plse = K.keypoint_loss(low, target, valid)
        up = torch.ones(1, device=dev)
        dlow = K.keypoint_loss_grad(low, target, valid, pmax, plse, cnt, up)
        parts = _pairs({"targets": targets,
                        "deconv": lambda: K.keypoint_deconv(xd, packed, bd.detach(), NK),
                        "loss": lambda: K.keypoint_loss(low, target, valid),
                        "loss_grad": lambda: K.keypoint_loss_grad(low, target, valid, pmax, plse, cnt, up, out=dlow),
                        "dx": lambda: K.keypoint_deconv_dx(dlow, packed_dx, NK),
                        "wgrad": lambda: K.keypoint_deconv_wgrad(xd, dlow, NK)}, args.reps, args.warmup)
    rows = M * S * S
    flops = 2.0 * rows * C * 16 * NK      # multiply-adds of one of the three products (forward, dx, dW), unpadded
    result["parts"] = {k: _spread(v) for k, v in parts.items()}
    for k in ("deconv", "dx", "wgrad"):
        result["parts"][k]["tflops_unpadded"] = flops / result["parts"][k]["median_ms"] / 1e9
    result["dlow_bytes"] = dlow.numel() * 4
    del low, dlow, xn, x_nchw
    torch.cuda.empty_cache()

    # ---- the whole step, with and without the keypoint branch
    def batch_of(keypoints):
        out = []
        for b in range(B):
            inst = Instances((H, W))
            inst.gt_boxes = Boxes(gts[b][0].to(dev))
            inst.gt_classes = torch.zeros(NG, dtype=torch.int64, device=dev)
            if keypoints:
                inst.gt_keypoints = Keypoints(kps[b])
            out.append({"image": syn.synthetic_image(10 + b, H, W).to(dev), "instances": inst, "height": H, "width": W})
        return out

    model = syn.conditioned_keypoint_head_(build_model(keypoint_rcnn_fpn()), seed=0).train().enable_keypoint_training()
    base = syn.conditioned_r50_fpn_(build_model(base_rcnn_fpn(num_classes=1)), seed=0).train()
    step_times, last = _steps({"step_keypoint_on": (model, batch_of(True)), "step_keypoint_off": (base, batch_of(False))},
                              max(args.reps // 2, 5), args.warmup)
    for k, v in step_times.items():
        result[k] = dict(_spread(v), losses=last[k])
    result["step_note"] = ("the two legs alternate in one loop; trunk, RPN and box-head weights are equal; the samplers draw from the "
                           "global RNG (no identity randperm), so the sampled rows, and with them the losses, differ between legs")
    result["not_measured"] += ["kernel times under a profiler (device events around whole calls only)",
                               "the step at 8 or 16 images per device", "multi-device training"]

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.splitext(args.out)[0] + "_pairs.txt", "w") as f:
        f.write("scripts/bench_keypoint_train.py on %s: the tail's forward + loss + backward at M = %d, S = %d, Cin = %d, K = %d, ours and\n"
                "PyTorch-ROCm's autograd alternated in one process after %d warm-up pairs, device events, ms, in the order run:\n\n"
                % (result["device"], M, S, C, NK, args.warmup))
        for i, (u, v) in enumerate(zip(pair_times["ours"], pair_times["torch"]), 1):
            f.write("ours %d %.4f\ntorch %d %.4f\n" % (i, u, i, v))
        f.write("\nours %.4f - %.4f (median %.4f), torch %.4f - %.4f (median %.4f)\n" % (
            min(pair_times["ours"]), max(pair_times["ours"]), statistics.median(pair_times["ours"]),
            min(pair_times["torch"]), max(pair_times["torch"]), statistics.median(pair_times["torch"])))
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
