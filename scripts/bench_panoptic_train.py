"""Times the training of Panoptic FPN's semantic branch on one MI355X and writes profiles/panoptic_train_bench.json.

8 images of 800 x 1333 (padded batch 800 x 1344, stride-4 maps 200 x 336), 54 stuff classes, logits rows of 64 floats.  Every figure is
the median of REPS device-event timings; the legs of a group alternate inside one process, so they share the machine's state.  Legs:

  loss_fwd / loss_fwd_bwd              lvcst_sem_seg_loss_fwd alone / with lvcst_sem_seg_loss_bwd, from the stride-4 logits and uint8 labels
  loss_torch_fwd / loss_torch_fwd_bwd  the yardstick: PyTorch-ROCm's F.interpolate(x4, bilinear) + F.cross_entropy(mean, ignore_index) with
                                       autograd on an NCHW copy of the same logits; `peak_bytes` of each side is
                                       torch.cuda.max_memory_allocated over one forward + backward, above what was allocated before it
  upsample2_bwd_<H>x<W>                lvcst_upsample2_bilinear_bwd_nhwc at the head's three sizes (128 channels), with the share of the
                                       chip's copy rate by dy read once + dx written once
  head_fwd_bwd                         SemSegFPNHead.forward_train_nhwc + losses + backward, the head's parameters training, on a fixed pyramid
  step_panoptic / step_mask            PanopticFPN's training step (forward + backward) / the same model's mask-only step (the base class's
                                       hooks: no semantic branch), FREEZE_AT 2

    python scripts/bench_panoptic_train.py [--out profiles/panoptic_train_bench.json] [--reps 20] [--batch 8] [--no-step]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

COPY_RATE = 6.3e12      # bytes / s: the chip's measured copy rate the byte counts are held against
IGNORE = 255


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(legs, reps, warmup=3):
    """{name: fn} -> {name: [ms]}: one timing of every leg per round, REPS rounds."""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            out[name].append(timed_once(fn))
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def ground_truth(h, w, seed, num_classes):
    """A few boxes with elliptic masks, and a label map, for one image."""
    from lvc_amd.structures import BitMasks, Boxes, Instances
    from lvc_amd.utils import synthetic as syn

    g = torch.Generator().manual_seed(seed)
    n = 6
    x0, y0 = torch.rand(n, generator=g) * (w - 320), torch.rand(n, generator=g) * (h - 320)
    bw, bh = 60 + torch.rand(n, generator=g) * 240, 60 + torch.rand(n, generator=g) * 240
    yy, xx = torch.arange(h, dtype=torch.float32)[:, None] + 0.5, torch.arange(w, dtype=torch.float32)[None, :] + 0.5
    masks = torch.stack([((xx - (x0[j] + bw[j] / 2)) / (bw[j] / 2)) ** 2 + ((yy - (y0[j] + bh[j] / 2)) / (bh[j] / 2)) ** 2 <= 1.0 for j in range(n)])
    inst = Instances((h, w))
    inst.gt_boxes = Boxes(torch.stack([x0, y0, x0 + bw, y0 + bh], 1))
    inst.gt_classes = torch.randint(0, num_classes, (n,), generator=g)
    inst.gt_masks = BitMasks(masks)
    return inst, syn.sem_seg_label_map(seed, h, w, 54, IGNORE).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panoptic_train_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--no-step", action="store_true", help="leave the two model steps out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_panoptic_train.py measures on the GPU; there is no CPU path"

    from lvc_amd import kernels as K
    from lvc_amd.config.presets import panoptic_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.modeling.meta_arch.rcnn import GeneralizedRCNN
    from lvc_amd.modeling.meta_arch.semantic_seg import sem_seg_loss
    from lvc_amd.utils import synthetic as syn
    from lvc_amd.utils.events import EventStorage

    B, H, W = args.batch, args.height, args.width
    model = syn.conditioned_panoptic_(build_model(panoptic_fpn()))
    head = model.sem_seg_head
    Kc, ld, scale = head.num_classes, head.logits_ld, head.common_stride
    Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    h, w = Hp // scale, Wp // scale
    res = {"batch": B, "image": [H, W], "classes": Kc, "reps": args.reps, "device": torch.cuda.get_device_name(0), "logits": [B, h, w, ld]}
    g = torch.Generator().manual_seed(0)

    # ---- the loss and its yardstick
    logits = torch.zeros(B, h, w, ld, device="cuda")
    logits[..., :Kc] = (torch.randn(B, h, w, Kc, generator=g) * 3).cuda()
    label_maps = [syn.sem_seg_label_map(1 + i, H, W, Kc, IGNORE).to(torch.uint8) for i in range(B)]
    labels = torch.cat([m.reshape(-1) for m in label_maps]).cuda()
    jobs, _ = K.sem_seg_loss_jobs([(H, W)] * B)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    one = torch.ones(1, device="cuda")
    dlow = torch.empty_like(logits)
    maps = (torch.empty(B, Hp, Wp, device="cuda"), torch.empty(B, Hp, Wp, device="cuda"))
    d_jobs = K._upload_table(jobs, logits.device)
    nchw = logits[..., :Kc].permute(0, 3, 1, 2).contiguous()
    target = torch.full((B, Hp, Wp), IGNORE, dtype=torch.int64)
    for i, m in enumerate(label_maps):
        target[i, :H, :W] = m.long()
    target = target.cuda()

    def ours_fwd():
        return K.sem_seg_loss_fwd(logits, labels, jobs, Kc, scale, IGNORE, status, d_jobs=d_jobs, maps=maps)

    def ours_fwd_bwd():
        loss, _, _, count, _ = ours_fwd()
        K.sem_seg_loss_bwd(logits, labels, jobs, d_jobs, Kc, scale, IGNORE, maps, one, count, out=dlow)
        return loss

    def torch_fwd():
        with torch.no_grad():
            return F.cross_entropy(F.interpolate(nchw, scale_factor=scale, mode="bilinear", align_corners=False), target,
                                   reduction="mean", ignore_index=IGNORE)

    def torch_fwd_bwd():
        x = nchw.detach().requires_grad_()
        loss = F.cross_entropy(F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False), target, reduction="mean",
                               ignore_index=IGNORE)
        loss.backward()
        return loss, x.grad

    legs = {"loss_fwd": ours_fwd, "loss_torch_fwd": torch_fwd, "loss_fwd_bwd": ours_fwd_bwd, "loss_torch_fwd_bwd": torch_fwd_bwd}
    res.update({k: summary(v) for k, v in alternate(legs, args.reps).items()})
    ours, (theirs, tgrad) = ours_fwd_bwd(), torch_fwd_bwd()
    res["loss_fwd_bwd"]["loss"], res["loss_torch_fwd_bwd"]["loss"] = float(ours), float(theirs.detach())
    res["loss_fwd_bwd"]["max_abs_gradient_difference_from_torch"] = float((dlow[..., :Kc] - tgrad.permute(0, 2, 3, 1)).abs().max())
    del tgrad

    def ours_autograd():
        x = logits.detach().requires_grad_()
        sem_seg_loss(x, labels, jobs, Kc, scale, IGNORE, status).backward()

    res["loss_fwd_bwd"]["peak_bytes"] = peak_bytes(ours_autograd)
    res["loss_torch_fwd_bwd"]["peak_bytes"] = peak_bytes(lambda: torch_fwd_bwd() and None)
    pixels = B * Hp * Wp
    # per pixel: K bilinear values twice (max, sum) and one exponential forward; backwards every (low pixel, class) walks (2 scale)^2 outputs
    res["loss_fwd"].update(bytes_read=logits.numel() * 4 * Kc // ld + labels.numel(), bytes_written=pixels * 8,
                           exponentials=pixels * Kc, bilinear_values=2 * pixels * Kc)
    taps = B * h * w * Kc * (2 * scale) ** 2
    res["loss_fwd_bwd"].update(backward_bytes_read=logits.numel() * 4 * Kc // ld + labels.numel() + pixels * 8, backward_bytes_written=logits.numel() * 4,
                               backward_exponentials=taps, backward_bilinear_values=taps)
    for name in ("loss_fwd",):
        r = res[name]
        r["share_of_copy_rate"] = (r["bytes_read"] + r["bytes_written"]) / COPY_RATE / (r["median_ms"] * 1e-3)
    bwd_ms = res["loss_fwd_bwd"]["median_ms"] - res["loss_fwd"]["median_ms"]
    res["loss_fwd_bwd"]["backward_ms_by_difference"] = bwd_ms
    res["loss_fwd_bwd"]["backward_share_of_copy_rate"] = ((res["loss_fwd_bwd"]["backward_bytes_read"] + res["loss_fwd_bwd"]["backward_bytes_written"])
                                                          / COPY_RATE / (max(bwd_ms, 1e-6) * 1e-3))
    res["loss_fwd"]["exponentials_per_second"] = pixels * Kc / (res["loss_fwd"]["median_ms"] * 1e-3)
    res["loss_fwd_bwd"]["backward_exponentials_per_second"] = taps / (max(bwd_ms, 1e-6) * 1e-3)
    del nchw, target

    # ---- the x2 upsample backward at the head's three sizes
    ups = {}
    for k in (3, 2, 1):
        uh, uw = h >> k, w >> k
        dy = torch.randn(B, 2 * uh, 2 * uw, 128, device="cuda")
        dx = torch.empty(B, uh, uw, 128, device="cuda")
        ups["upsample2_bwd_%dx%d" % (uh, uw)] = (dy, dx)
    legs = {name: (lambda dy=dy, dx=dx: K.upsample2_bilinear_bwd_nhwc(dy, out=dx)) for name, (dy, dx) in ups.items()}
    for name, ms in alternate(legs, args.reps).items():
        dy, dx = ups[name]
        res[name] = summary(ms)
        res[name]["bytes"] = 4 * (dy.numel() + dx.numel())
        res[name]["GB_per_s"] = res[name]["bytes"] / (res[name]["median_ms"] * 1e-3) / 1e9
        res[name]["share_of_copy_rate"] = res[name]["bytes"] / COPY_RATE / (res[name]["median_ms"] * 1e-3)
    del ups, legs

    # ---- the head as a whole: forward + backward, its parameters training
    model.train()
    feats = {f: torch.randn(B, Hp >> l, Wp >> l, 256, device="cuda") for f, l in zip(("p2", "p3", "p4", "p5"), (2, 3, 4, 5))}
    params = list(head.parameters())

    def head_step():
        for p in params:
            p.grad = None
        out = head.losses(head.forward_train_nhwc(feats), (labels, jobs))
        out["loss_sem_seg"].backward()

    res["head_fwd_bwd"] = summary(alternate({"head_fwd_bwd": head_step}, args.reps)["head_fwd_bwd"])
    res["head_fwd_bwd"]["peak_bytes"] = peak_bytes(head_step)
    del feats

    # ---- the model's step with and without the semantic branch
    if not args.no_step:
        model.enable_mask_training().enable_sem_seg_training()
        batch = []
        for i in range(B):
            inst, sem = ground_truth(H, W, 1 + i, model.roi_heads.num_classes)
            batch.append({"image": syn.synthetic_image(1 + i, H, W).cuda(), "instances": inst.to("cuda"), "sem_seg": sem})
        every = list(model.parameters())

        def step(mask_only):
            for p in every:
                p.grad = None
            with EventStorage(0):
                losses = GeneralizedRCNN.forward(model, batch) if mask_only else model(batch)
            sum(losses.values()).backward()
            return losses

        hooks = ("_forward_train", "_on_train_features", "_train_extra_words", "_on_train_extra_words", "_train_losses")
        cls = type(model)
        own = {k: cls.__dict__[k] for k in hooks}

        def mask_step():
            for k in hooks:
                setattr(cls, k, getattr(GeneralizedRCNN, k))
            try:
                return step(True)
            finally:
                for k in hooks:
                    setattr(cls, k, own[k])

        t = alternate({"step_panoptic": lambda: step(False), "step_mask": mask_step}, args.reps, warmup=2)
        res.update({k: summary(v) for k, v in t.items()})
        res["step_panoptic"]["losses"] = {k: float(v.detach()) for k, v in step(False).items()}
        res["step_mask"]["losses"] = {k: float(v.detach()) for k, v in mask_step().items()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
