"""Times of the mask branch of R50-FPN Mask R-CNN inference (presets.mask_rcnn_fpn, 80 classes) for a batch of 8 synthetic 800 x 1333
images with 100 detections per image, on one device.  Medians of `--reps`, legs alternated in one process.  None of these is a gate.

  pooler      StandardROIHeads.pool_masks_batched, the call the forward makes: the compaction's index arithmetic, level assignment and
              ROIAlign 14 x 14 over p2..p5 for the 800 boxes (`roi_align_only`: its ROIAlign launch alone on the same rois)
  mask_fcn<k> each 3x3 conv of the head on [800, 14, 14, 256], with the route `kernels.conv_route` gives it
  tail        lvc_mask_deconv_predict (deconv + ReLU + predictor of the predicted class + sigmoid), beside the same tail through
              PyTorch-ROCm (conv_transpose2d + relu + conv2d + gather + sigmoid) as a yardstick; TF counts 2 M S^2 Cin 4 Cmid flops
  paste       lvc_paste_masks for the 800 detections into 800 x 1333 planes, its output bytes against the 6.3 TB/s copy rate, beside
              F.grid_sample + threshold in chunks of 100 detections (the reference's GPU path) as a yardstick
  forward     model.forward() img/s with MASK_ON and of the box-only model on the same weights (wall clock, synchronised)

Writes profiles/mask_rcnn_bench.json and prints it as one JSON line.

    python scripts/bench_mask_rcnn.py [--reps 20] [--warmup 3] [--out profiles/mask_rcnn_bench.json]
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


def _wall(model, batch, reps, warmup):
    times = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model(batch)
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    ms = 1e3 * statistics.median(times)
    return {"ms_per_batch": ms, "img_per_s": len(batch) * 1e3 / ms, "detections": [len(o["instances"]) for o in out]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_rcnn_bench.json"))
    args = ap.parse_args()

    from lvc_amd import kernels as K
    from lvc_amd.config.presets import base_rcnn_fpn, mask_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    model = syn.conditioned_mask_head_(build_model(mask_rcnn_fpn()).eval(), seed=0)
    base = syn.conditioned_r50_fpn_(build_model(base_rcnn_fpn()).eval(), seed=0)
    B, T, H, W = 8, 100, 800, 1333
    batch = [{"image": syn.synthetic_image(10 + i, H, W).to(dev), "height": H, "width": W} for i in range(B)]
    result = {"batch": B, "image": [H, W], "classes": 80, "detections_per_image": T, "reps": args.reps, "copy_gbps": COPY_GBPS,
              "device": torch.cuda.get_device_name(0)}
    heads = model.roi_heads
    head, pl = heads.mask_head, heads.mask_pooler

    with torch.no_grad():
        images = model.preprocess_image(batch)
        n, _, hp, wp = images.tensor.shape
        x4 = images.tensor.as_strided((n, hp, wp, 4), (hp * wp * 4, wp * 4, 4, 1), images.tensor.storage_offset())
        feats = model.backbone.forward_nhwc(x4)
        fl = [feats[f] for f in heads.mask_in_features]
        # 100 boxes per image whatever the seeded detector finds: seeded boxes of 16 .. 400 px inside the image
        g = torch.Generator().manual_seed(0)
        wh = 16 + 384 * torch.rand(B, T, 2, generator=g)
        xy = torch.rand(B, T, 2, generator=g) * (torch.tensor([W, H]) - wh)
        boxes = torch.cat([xy, xy + wh], 2).to(dev)
        classes = torch.randint(0, 80, (B, T), generator=g).to(torch.int32).to(dev)
        M = B * T

        count = torch.full((B,), T, dtype=torch.int32, device=dev)

        def pooler():
            return heads.pool_masks_batched(feats, boxes, classes, count)

        levels, rois = K.assign_levels_rois(boxes, pl.min_level, pl.max_level, pl.canonical_box_size, pl.canonical_level)

        def roi_align_only():      # the launch inside `pooler`: no row count, the vectorised NHWC kernel
            return K.roi_align_fpn_nhwc(fl, pl.scales, rois, levels, pl.output_size[0], pl.output_size[1], pl.sampling_ratio, pl.aligned)

        pooled = pooler()[0]
        assert torch.equal(pooled, roi_align_only())      # every image is full: the compaction is the identity
        legs, acts, x = {"pooler": pooler, "roi_align_only": roi_align_only}, [], pooled
        for k, layer in enumerate(head.conv_norm_relus):
            acts.append(x)
            legs["mask_fcn%d" % (k + 1)] = (lambda layer=layer, x=x: layer.forward_nhwc(x))
            x = layer.forward_nhwc(x)
        xin = x.contiguous()
        cls = classes.view(-1).contiguous()
        p = head.predictor
        wdp, wpp = head.deconv.packed(), p.weight.detach().view(p.out_channels, -1)

        def tail():
            return K.mask_deconv_predict(xin, wdp, head.deconv.bias, wpp, p.bias, classes=cls)

        x_nchw = xin.permute(0, 3, 1, 2).contiguous()
        idx = torch.arange(M, device=dev)
        cls64 = cls.long()

        def tail_torch():
            y = F.conv2d(F.relu(F.conv_transpose2d(x_nchw, head.deconv.weight, head.deconv.bias, stride=2)), p.weight, p.bias)
            return y[idx, cls64].sigmoid()

        prob = tail()
        err = float((prob - tail_torch()).abs().max())
        legs["tail"], legs["tail_torch"] = tail, tail_torch

        hb = boxes.view(M, 4).cpu().numpy()
        jobs = K.paste_jobs(range(M), hb, [(H, W)] * M, [i * H * W for i in range(M)])
        total = M * H * W
        buf = torch.empty((total + 15) // 16 * 16, dtype=torch.uint8, device=dev)

        def paste():
            return K.paste_masks(prob, jobs, total, out=buf)

        bx = boxes.view(M, 4)
        ys = torch.arange(H, device=dev, dtype=torch.float32) + 0.5
        xs = torch.arange(W, device=dev, dtype=torch.float32) + 0.5

        def paste_torch():
            outs = []
            for c in range(0, M, 100):
                b = bx[c:c + 100]
                gy = (ys[None] - b[:, 1:2]) / (b[:, 3:4] - b[:, 1:2]) * 2 - 1
                gx = (xs[None] - b[:, 0:1]) / (b[:, 2:3] - b[:, 0:1]) * 2 - 1
                grid = torch.stack([gx[:, None, :].expand(-1, H, W), gy[:, :, None].expand(-1, H, W)], 3)
                outs.append(F.grid_sample(prob[c:c + 100, None], grid, align_corners=False)[:, 0] >= 0.5)
            return outs

        same = paste()[:total].view(M, H, W).bool()
        ref = torch.cat(paste_torch())
        result["paste_bits_differ_from_grid_sample"] = int((same != ref).sum())
        del same, ref
        legs["paste"], legs["paste_torch"] = paste, paste_torch

        t = _alternate(legs, args.reps, args.warmup)
        S, cin, cmid = pooled.shape[1], xin.shape[3], head.deconv.out_channels
        result["pooler"] = {"ms": t["pooler"], "roi_align_only_ms": t["roi_align_only"], "kernel": "roi_align_fwd_nhwc4_kernel", "rois": M,
                            "resolution": S}
        conv_flops = 2.0 * M * S * S * 9 * 256 * 256
        for k, layer in enumerate(head.conv_norm_relus):
            r = K.conv_route(layer.packed(), M, S, S)
            ms = t["mask_fcn%d" % (k + 1)]
            result["mask_fcn%d" % (k + 1)] = {"ms": ms, "route": r[0], "entry": r[1], "tflops": conv_flops / ms / 1e9}
        tail_flops = 2.0 * M * S * S * cin * 4 * cmid
        result["tail"] = {"ms": t["tail"], "tflops": tail_flops / t["tail"] / 1e9, "torch_ms": t["tail_torch"],
                          "max_abs_diff_from_torch": err}
        result["paste"] = {"ms": t["paste"], "bytes": total, "gbps": total / t["paste"] / 1e6, "of_copy_rate": total / t["paste"] / 1e6 / COPY_GBPS,
                           "torch_grid_sample_ms": t["paste_torch"]}
        result["flop_split"] = {"mask_fcn_tflop": 4 * conv_flops / 1e12, "tail_tflop": tail_flops / 1e12,
                                "mask_fcn_ms": sum(t["mask_fcn%d" % (k + 1)] for k in range(len(head.conv_norm_relus))), "tail_ms": t["tail"]}
        del buf
        torch.cuda.empty_cache()
        result["forward_mask_on"] = _wall(model, batch, args.reps, args.warmup)
        result["forward_mask_off"] = _wall(base, batch, args.reps, args.warmup)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
