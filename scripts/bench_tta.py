"""Throughput of test-time augmentation (GeneralizedRCNNWithTTA, default TEST.AUG: 9 sizes x flip = 18 augmentations per image) on one
GPU, against its floor: the same augmented groups through the plain fast path (GeneralizedRCNN.inference_nhwc) on buffers built
beforehand, timed the same way.  Prints one JSON line.

    python scripts/bench_tta.py [--images 8] [--reps 3] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    args = ap.parse_args()

    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.modeling import GeneralizedRCNNWithTTA, build_model
    from lvc_amd.modeling.test_time_augmentation import _Plan
    from lvc_amd.structures import ImageList
    from lvc_amd.utils import synthetic as syn

    torch.cuda.set_device(0)
    cfg = base_rcnn_fpn()
    model = build_model(cfg).eval()
    syn.conditioned_r50_fpn_(model)
    tta = GeneralizedRCNNWithTTA(cfg, model)
    dev = model.device
    imgs = [syn.synthetic_image(100 + i, args.height, args.width).round().clamp(0, 255).to(torch.uint8) for i in range(args.images)]
    inputs = [{"image": im} for im in imgs]

    # the floor's operands: every image's augmented groups, built once
    groups = []
    aug = cfg.TEST.AUG
    for im in imgs:
        H, W = im.shape[1:]
        plan = _Plan(H, W, H, W, aug.MIN_SIZES, aug.MAX_SIZE, aug.FLIP)
        slots = []
        for g0 in range(0, len(plan.augs), tta.batch_size):
            sizes = [plan.sizes[j] for j, _ in plan.augs[g0:g0 + tta.batch_size]]
            Hp, Wp = ImageList.padded_size(sizes, model.backbone.size_divisibility)
            buf = torch.empty(len(sizes), Hp, Wp, 4, device=dev)
            groups.append((buf, sizes))
            slots.extend(buf[s] for s in range(len(sizes)))
        d = im.to(dev)
        plan.launch(d, (d.stride(1), d.stride(2), d.stride(0)), dev, slots=slots, mean=model.pixel_mean, std=model.pixel_std)

    def run_tta():
        for inp in inputs:
            tta([inp])            # one device->host read per call

    def run_floor():
        outs = [model.inference_nhwc(buf, sizes) for buf, sizes in groups]
        torch.cuda.synchronize()
        return outs

    def timed(fn):
        with torch.no_grad():
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            best = float("inf")
            for _ in range(args.reps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t0)
        return 1e3 * best / args.images

    ms = timed(run_tta)
    floor = timed(run_floor)
    print(json.dumps({"metric": "tta_images_per_s", "value": round(1e3 / ms, 2), "ms_per_image": round(ms, 2), "floor_ms": round(floor, 2),
                      "diff_ms": round(ms - floor, 2), "ratio": round(ms / floor, 4), "images": args.images,
                      "size": [args.height, args.width], "augmentations": len(aug.MIN_SIZES) * (2 if aug.FLIP else 1),
                      "min_sizes": list(aug.MIN_SIZES), "max_size": aug.MAX_SIZE, "batch_size": tta.batch_size,
                      "timing": "best of %d reps after %d warm-up, wall clock with a device sync" % (args.reps, args.warmup)}))


if __name__ == "__main__":
    main()
