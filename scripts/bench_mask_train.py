"""Times of the mask branch of R50-FPN Mask R-CNN TRAINING (presets.mask_rcnn_fpn, 80 classes) at 8 images x 128 foreground RoIs:
M = 1024 rows, S = 14, 256 -> 256 channels, ground-truth planes of 800 x 1333, on one device.  Medians of `--reps`, legs alternated in
one process.  None of these is a gate.

  targets     lvc_mask_targets for the 1024 rows (20 planes per image, boxes of 16 .. 400 px), its bytes (planes under the boxes, boxes,
              output) against the copy rate
  logits      lvc_mask_deconv_logits, beside conv_transpose2d + relu + conv2d + gather through PyTorch-ROCm
  loss        lvc_mask_loss (pass + finish), beside binary_cross_entropy_with_logits and the three logged counts through PyTorch-ROCm
  backward    kernels.mask_deconv_grad: the whole backward of tail + loss, and its parts -- `grad_kernel` (the launch that recomputes the
              hidden tile and writes dh, with its finishing launches), `dx` (the GEMM dh x Wd) and `dWd` (lvc_mask_deconv_wgrad) --
              beside autograd's backward of the PyTorch-ROCm expression
  step        one training step (forward + backward, wall clock, synchronised) of the mask model with enable_mask_training() and of the
              box-only model on the same trunk, RPN and box-head weights and the same batch (20 ground-truth boxes per image), the two
              alternated in one loop; the samplers draw from the global RNG, so the two legs sample different rows

Byte times use the 6.3 TB/s copy rate the README uses.  Writes profiles/mask_train_bench.json and prints it as one JSON line.

    python scripts/bench_mask_train.py [--reps 20] [--warmup 3] [--out profiles/mask_train_bench.json]
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
            start.record()
            fn()
            end.record()
            end.synchronize()
            if i >= warmup:
                times[k].append(start.elapsed_time(end))
    return {k: statistics.median(v) for k, v in times.items()}


def _ellipses(n, H, W, boxes, g):
    yy, xx = torch.arange(H, dtype=torch.float32)[:, None], torch.arange(W, dtype=torch.float32)[None, :]
    out = torch.zeros(n, H, W, dtype=torch.bool)
    for j in range(n):
        x0, y0, x1, y1 = boxes[j].tolist()
        out[j] = ((xx - (x0 + x1) / 2) / ((x1 - x0) / 2)) ** 2 + ((yy - (y0 + y1) / 2) / ((y1 - y0) / 2)) ** 2 <= 1.0
    return out


def _steps(legs, reps, warmup):
    """legs: name -> (model, batch).  One training step (forward + backward, wall clock, synchronised) of each leg in turn, `reps` times."""
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
                    times[k].append(time.perf_counter() - t0)
                last[k] = {n: float(v.detach()) for n, v in losses.items()}
    out = {}
    for k, (_model, batch) in legs.items():
        ms = 1e3 * statistics.median(times[k])
        out[k] = {"ms_per_step": ms, "img_per_s": len(batch) * 1e3 / ms, "losses": last[k]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_train_bench.json"))
    args = ap.parse_args()

    from lvc_amd import kernels as K
    from lvc_amd.config.presets import base_rcnn_fpn, mask_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.structures import BitMasks, Boxes, Instances
    from lvc_amd.utils import synthetic as syn

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    B, R, H, W, S, C, NK, NG = 8, 128, 800, 1333, 14, 256, 80, 20
    M = B * R
    result = {"batch": B, "rois_per_image": R, "rows": M, "image": [H, W], "classes": NK, "reps": args.reps, "copy_gbps": COPY_GBPS,
              "device": torch.cuda.get_device_name(0), "not_measured": []}
    g = torch.Generator().manual_seed(0)

    # ---- ground truth: 20 boxes per image with an ellipse each; 128 sampled boxes per image jittered around them
    gts = []
    for b in range(B):
        wh = 32 + 368 * torch.rand(NG, 2, generator=g)
        xy = torch.rand(NG, 2, generator=g) * (torch.tensor([W, H]) - wh)
        gb = torch.cat([xy, xy + wh], 1)
        gts.append((gb, torch.randint(0, NK, (NG,), generator=g), _ellipses(NG, H, W, gb, g)))
    matched = torch.randint(0, NG, (B, R), generator=g)
    boxes = torch.stack([gts[b][0][matched[b]] for b in range(B)])
    boxes = boxes + (torch.rand(B, R, 4, generator=g) - 0.5) * 0.2 * (boxes[:, :, 2:] - boxes[:, :, :2]).repeat(1, 1, 2)
    boxes[:, :, 0::2] = boxes[:, :, 0::2].clamp(0, W)
    boxes[:, :, 1::2] = boxes[:, :, 1::2].clamp(0, H)
    planes = [gts[b][2].to(dev) for b in range(B)]
    d_boxes, d_matched = boxes.to(dev).contiguous(), matched.to(dev)
    count = torch.full((B,), R, dtype=torch.int32, device=dev)
    classes = torch.stack([gts[b][1][matched[b]] for b in range(B)]).view(-1).to(torch.int32).to(dev)

    def targets():
        return K.mask_targets(d_boxes, d_matched, count, planes, 2 * S)

    tg = targets()
    area = float(((boxes[:, :, 2] - boxes[:, :, 0]).clamp(min=1) * (boxes[:, :, 3] - boxes[:, :, 1]).clamp(min=1)).sum())
    target_bytes = area + M * 16 + M * 8 + tg.numel()
    result["not_measured"].append("targets through PyTorch-ROCm: the reference's expression is its compiled ROIAlign operator, which has no "
                                  "eager PyTorch form here (torchvision is not installed)")

    # ---- the tail's operands: the synthetic case at full size, the model's own parameter layout
    x, wd, bd, wp, bp, _ = syn.mask_tail_case(M, S, C, C, NK)
    xn = x.permute(0, 2, 3, 1).contiguous().to(dev)
    x_nchw = x.to(dev).requires_grad_()
    wd, bd, wp, bp = [t.to(dev).requires_grad_() for t in (wd, bd, wp, bp)]
    packed = K.pack_mask_deconv(wd)
    wp2 = wp.detach().reshape(NK, C).contiguous()
    idx, cls64 = torch.arange(M, device=dev), classes.long()
    up = torch.ones(1, device=dev)

    def logits():
        return K.mask_deconv_logits(xn, packed, bd.detach(), wp2, bp.detach(), classes=classes)

    def logits_torch():
        return F.conv2d(F.relu(F.conv_transpose2d(x_nchw, wd, bd, stride=2)), wp, bp)[idx, cls64]

    z = logits()
    with torch.no_grad():
        result["logits_max_abs_diff_from_torch"] = float((z - logits_torch()).abs().max())

    def loss():
        return K.mask_loss(z, tg)

    tgf, tgb = tg.float(), tg.bool()

    def loss_torch():
        bad = (z > 0.0) != tgb
        return F.binary_cross_entropy_with_logits(z, tgf, reduction="mean"), bad.sum(), tgb.sum(), (bad & ~tgb).sum()

    def backward():
        return K.mask_deconv_grad(xn, packed, bd.detach(), wp2, classes, z, tg, None, up)

    def grad_kernel():
        return K.mask_deconv_grad(xn, packed, bd.detach(), wp2, classes, z, tg, None, up, need_dx=False, need_dw=False)

    def grad_dx():
        return K.mask_deconv_grad(xn, packed, bd.detach(), wp2, classes, z, tg, None, up, need_dx=True, need_dw=False)

    def grad_dw():
        return K.mask_deconv_grad(xn, packed, bd.detach(), wp2, classes, z, tg, None, up, need_dx=False, need_dw=True)

    zt = logits_torch()
    lt = F.binary_cross_entropy_with_logits(zt, tgf, reduction="mean")

    def backward_torch():
        return torch.autograd.grad(lt, (x_nchw, wd, bd, wp, bp), retain_graph=True)

    ours, theirs = backward(), backward_torch()
    result["backward_max_rel_diff_from_torch"] = {
        k: float((a.reshape(b.shape) - b).abs().max() / b.abs().max().clamp_min(1e-30))
        for k, a, b in zip(("dx", "dWd", "dbd", "dWp", "dbp"), (ours[0].permute(0, 3, 1, 2),) + tuple(ours[1:]), theirs)}
    with torch.no_grad():      # the same gradients in fp64 on the device (matmuls in double), relative to each one's largest entry
        rows_, x2, pk = M * S * S, xn.view(M * S * S, C).double(), packed.double()
        pre = (x2 @ pk.t()).view(rows_, 4, C) + bd.detach().double()
        wrow = wp2.double()[cls64].repeat_interleave(S * S, 0)
        z64 = (pre.clamp(min=0) * wrow[:, None, :]).sum(-1) + bp.detach().double()[cls64].repeat_interleave(S * S, 0)[:, None]
        t4 = tgb.view(M, S, 2, S, 2).permute(0, 1, 3, 2, 4).reshape(rows_, 4).double()
        dh64 = ((torch.sigmoid(z64) - t4) / (M * 4 * S * S))[:, :, None] * wrow[:, None, :] * (pre > 0)
        del pre, wrow
        ref64 = {"dx": (dh64.view(rows_, 4 * C) @ pk).view(M, S, S, C).permute(0, 3, 1, 2),
                 "dWd": (dh64.view(rows_, 4 * C).t() @ x2).view(2, 2, C, C).permute(3, 2, 0, 1), "dbd": dh64.sum(dim=(0, 1))}
        del dh64, x2
        result["backward_max_rel_err_vs_fp64"] = {
            who: {k: float((got.double() - ref64[k]).abs().max() / ref64[k].abs().max()) for k, got in zip(("dx", "dWd", "dbd"), gs)}
            for who, gs in (("ours", (ours[0].permute(0, 3, 1, 2), ours[1], ours[2])), ("torch_fp32", theirs[:3]))}
        result["backward_note"] = ("at this size both fp32 evaluations are dominated by hidden units whose pre-activation lies within fp32 "
                                   "noise of 0 and flips its ReLU gate, not by the GEMMs")
        del ref64
        legs = {"targets": targets, "logits": logits, "logits_torch": logits_torch, "loss": loss, "loss_torch": loss_torch}
        t = _alternate(legs, args.reps, args.warmup)
    t.update(_alternate({"backward": backward, "grad_kernel": grad_kernel, "grad_dx": grad_dx, "grad_dw": grad_dw,
                         "backward_torch": backward_torch}, args.reps, args.warmup))
    rows = M * S * S
    flops = 2.0 * rows * C * 4 * C
    dh_bytes, x_bytes = rows * 4 * C * 4.0, rows * C * 4.0

    def entry(ms, nbytes, **kw):
        byte_ms = nbytes / COPY_GBPS / 1e6
        return dict({"ms": ms, "bytes": nbytes, "byte_time_ms": byte_ms, "times_byte_time": ms / byte_ms}, **kw)

    result["targets"] = entry(t["targets"], target_bytes)
    result["logits"] = entry(t["logits"], x_bytes + z.numel() * 4.0, tflops=flops / t["logits"] / 1e9, torch_ms=t["logits_torch"])
    result["loss"] = entry(t["loss"], z.numel() * 5.0, torch_ms=t["loss_torch"])
    # x read, dh written, dh read twice and x once by the two GEMMs, dx written
    result["backward"] = entry(t["backward"], x_bytes + dh_bytes + 2 * dh_bytes + x_bytes + x_bytes, torch_ms=t["backward_torch"],
                               tflops=3 * flops / t["backward"] / 1e9)
    result["backward_parts"] = {"grad_kernel_ms": t["grad_kernel"], "grad_kernel_bytes": x_bytes + dh_bytes,
                                "grad_kernel_gbps": (x_bytes + dh_bytes) / t["grad_kernel"] / 1e6,
                                "dx_ms": t["grad_dx"] - t["grad_kernel"], "dWd_ms": t["grad_dw"] - t["grad_kernel"],
                                "dh_bytes": dh_bytes, "dgrad_split": K.DGRAD_SPLIT}
    del ours, theirs, zt, lt, x_nchw, xn, z
    torch.cuda.empty_cache()

    # ---- the whole step, with and without the mask branch
    def batch_of(masks):
        out = []
        for b in range(B):
            inst = Instances((H, W))
            inst.gt_boxes = Boxes(gts[b][0].to(dev))
            inst.gt_classes = gts[b][1].to(dev)
            if masks:
                inst.gt_masks = BitMasks(planes[b])
            out.append({"image": syn.synthetic_image(10 + b, H, W).to(dev), "instances": inst, "height": H, "width": W})
        return out

    model = syn.conditioned_mask_head_(build_model(mask_rcnn_fpn()), seed=0).train().enable_mask_training()
    base = syn.conditioned_r50_fpn_(build_model(base_rcnn_fpn()), seed=0).train()
    steps = _steps({"step_mask_on": (model, batch_of(True)), "step_mask_off": (base, batch_of(False))}, args.reps, args.warmup)
    result.update(steps)
    result["step_note"] = ("the two legs alternate in one loop; trunk, RPN and box-head weights are equal; the samplers draw from the "
                           "global RNG (no identity randperm), so the sampled anchors and rows, and with them the losses, differ between legs")

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
