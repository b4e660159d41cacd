"""Times of the keypoint branch of R50-FPN Keypoint R-CNN inference (presets.keypoint_rcnn_fpn) for a batch of 8 synthetic 800 x 1333
images with 100 seeded boxes per image, on one device.  Medians of `--reps`, legs alternated in one process.  None of these is a gate.

  pooler       the keypoint branch's row compaction, level assignment and ROIAlign 14 x 14 over p2..p5 for the 800 boxes
  conv_fcn<k>  each 3x3 conv of the head on [800, 14, 14, 256 / 512], with the route `kernels.conv_route` gives it
  deconv       lvc_keypoint_deconv (score_lowres: 4x4 stride 2 pad 1, 512 -> 17), beside PyTorch-ROCm's conv_transpose2d on the same
               operands (NCHW) as a yardstick; TF counts 2 M S^2 16 Cin K flops
  decode       lvc_heatmaps_to_keypoints with up = 2 (bilinear x2, bicubic resize to every box, max / argmax / score), beside the
               reference's loop over the RoIs restated in torch on the device (interpolate x2 once, then per RoI interpolate(bicubic),
               max, argmax, two exps and a sum) as a yardstick
  forward      model.forward() img/s with KEYPOINT_ON and of the box-only model on the same weights (wall clock, synchronised)

Writes profiles/keypoint_rcnn_bench.json and prints it as one JSON line.

    python scripts/bench_keypoint_rcnn.py [--reps 20] [--warmup 3] [--out profiles/keypoint_rcnn_bench.json]
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


def decode_torch(low, rois):
    """The reference's heatmaps_to_keypoints (its loop over RoIs) after layers()'s interpolate(scale_factor=2), on the device."""
    maps = F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=False)
    widths = (rois[:, 2] - rois[:, 0]).clamp(min=1)
    heights = (rois[:, 3] - rois[:, 1]).clamp(min=1)
    wc, hc = widths.ceil(), heights.ceil()
    sizes = torch.stack([hc, wc], 1).to(torch.int64).tolist()      # (the reference reads them RoI by RoI)
    M, K = maps.shape[:2]
    out = maps.new_zeros(M, K, 4)
    kidx = torch.arange(K, device=maps.device)
    for i in range(M):
        roi_map = F.interpolate(maps[[i]], size=sizes[i], mode="bicubic", align_corners=False).squeeze(0)
        mx = roi_map.view(K, -1).max(1)[0].view(K, 1, 1)
        full = (roi_map - mx).exp_()
        pool = (maps[i] - mx).exp_()
        scores = full / pool.sum((1, 2), keepdim=True)
        w = roi_map.shape[2]
        pos = roi_map.view(K, -1).argmax(1)
        x_int = pos % w
        y_int = (pos - x_int) // w
        out[i, :, 0] = (x_int.float() + 0.5) * (widths[i] / wc[i]) + rois[i, 0]
        out[i, :, 1] = (y_int.float() + 0.5) * (heights[i] / hc[i]) + rois[i, 1]
        out[i, :, 2] = roi_map[kidx, y_int, x_int]
        out[i, :, 3] = scores[kidx, y_int, x_int]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoint_rcnn_bench.json"))
    args = ap.parse_args()

    from lvc_amd import kernels as K
    from lvc_amd.config.presets import base_rcnn_fpn, keypoint_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.modeling.roi_heads.roi_heads import front_rows
    from lvc_amd.utils import synthetic as syn

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    model = syn.conditioned_keypoint_head_(build_model(keypoint_rcnn_fpn()).eval(), seed=0)
    base = syn.conditioned_r50_fpn_(build_model(base_rcnn_fpn(num_classes=1)).eval(), seed=0)
    B, T, H, W = 8, 100, 800, 1333
    batch = [{"image": syn.synthetic_image(10 + i, H, W).to(dev), "height": H, "width": W} for i in range(B)]
    result = {"batch": B, "image": [H, W], "boxes_per_image": T, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    heads = model.roi_heads
    head, pl = heads.keypoint_head, heads.keypoint_pooler

    with torch.no_grad():
        images = model.preprocess_image(batch)
        n, _, hp, wp = images.tensor.shape
        x4 = images.tensor.as_strided((n, hp, wp, 4), (hp * wp * 4, wp * 4, 4, 1), images.tensor.storage_offset())
        feats = model.backbone.forward_nhwc(x4)
        fl = [feats[f] for f in heads.keypoint_in_features]
        # 100 boxes per image whatever the seeded detector finds: seeded boxes of 16 .. 400 px inside the image
        g = torch.Generator().manual_seed(0)
        wh = 16 + 384 * torch.rand(B, T, 2, generator=g)
        xy = torch.rand(B, T, 2, generator=g) * (torch.tensor([W, H]) - wh)
        boxes = torch.cat([xy, xy + wh], 2).to(dev)
        M = B * T
        count = torch.full((B,), T, dtype=torch.int32, device=dev)

        def pooler():
            rois, levels, _rows, _total, _order = front_rows(boxes, count, pl, len(fl))
            return K.roi_align_fpn_nhwc(fl, pl.scales, rois, levels, pl.output_size[0], pl.output_size[1], pl.sampling_ratio, pl.aligned)

        pooled = pooler()
        legs, x = {"pooler": pooler}, pooled
        shapes = []
        for k, layer in enumerate(head.blocks):
            legs["conv_fcn%d" % (k + 1)] = (lambda layer=layer, x=x: layer.forward_nhwc(x))
            shapes.append((x.shape[3], layer.out_channels))
            x = layer.forward_nhwc(x)
        xin = x.contiguous()
        S, cin, nk = xin.shape[1], xin.shape[3], head.num_keypoints
        packed, bias, weight = head.score_lowres.packed(), head.score_lowres.bias, head.score_lowres.weight

        def deconv():
            return K.keypoint_deconv(xin, packed, bias, nk)

        x_nchw = xin.permute(0, 3, 1, 2).contiguous()

        def deconv_torch():
            return F.conv_transpose2d(x_nchw, weight, bias, stride=2, padding=1)

        low = deconv()
        err = float((low - deconv_torch()).abs().max())
        legs["deconv"], legs["deconv_torch"] = deconv, deconv_torch
        rois = boxes.view(M, 4).contiguous()

        def decode():
            return K.heatmaps_to_keypoints(low, rois, up=2)

        got, ref = decode(), decode_torch(low, rois)
        same_pos = ((got[:, :, :2] - ref[:, :, :2]).abs().amax(2) < 1e-3)
        result["decode_vs_torch_loop"] = {"keypoints": int(same_pos.numel()), "positions_differ": int((~same_pos).sum()),
                                          "max_abs_logit_diff": float((got[:, :, 2] - ref[:, :, 2]).abs().max()),
                                          "max_abs_score_diff": float((got[:, :, 3] - ref[:, :, 3]).abs().max())}
        legs["decode"] = decode
        t = _alternate(legs, args.reps, args.warmup)
        # the torch loop makes hundreds of launches per call: a few repetitions of its own
        t.update(_alternate({"decode_torch_loop": lambda: decode_torch(low, rois)}, max(3, args.reps // 5), 1))
        result["pooler"] = {"ms": t["pooler"], "rois": M, "resolution": S}
        for k, layer in enumerate(head.blocks):
            r = K.conv_route(layer.packed(), M, S, S)
            ms = t["conv_fcn%d" % (k + 1)]
            ci, co = shapes[k]
            result["conv_fcn%d" % (k + 1)] = {"ms": ms, "route": r[0], "entry": r[1], "cin": ci, "cout": co,
                                              "tflops": 2.0 * M * S * S * 9 * ci * co / ms / 1e9}
        flops = 2.0 * M * S * S * 16 * cin * nk
        result["deconv"] = {"ms": t["deconv"], "tflops": flops / t["deconv"] / 1e9, "torch_ms": t["deconv_torch"], "max_abs_diff_from_torch": err}
        pixels = float((rois[:, 2] - rois[:, 0]).clamp(min=1).ceil().mul((rois[:, 3] - rois[:, 1]).clamp(min=1).ceil()).sum()) * nk
        result["decode"] = {"ms": t["decode"], "resized_pixels": pixels, "gpixels_per_s": pixels / t["decode"] / 1e6,
                            "torch_loop_ms": t["decode_torch_loop"]}
        result["branch_ms"] = t["pooler"] + sum(t["conv_fcn%d" % (k + 1)] for k in range(len(head.blocks))) + t["deconv"] + t["decode"]
        torch.cuda.empty_cache()
        result["forward_keypoint_on"] = _wall(model, batch, args.reps, args.warmup)
        result["forward_keypoint_off"] = _wall(base, batch, args.reps, args.warmup)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
