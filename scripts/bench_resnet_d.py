"""Times of what the ResNet-D trunk (RESNETS.D) adds, for a batch of 8 at 800 x 1344.  Per leg: median device time of `--reps` launches,
legs alternated in one process.  None of these is a gate.

  pool    lvc_avgpool2_nhwc (csrc/avgpool.hip) at both pools of the three stride-2 blocks (res3.0 / res4.0 / res5.0: conv2's output and
          the block input), written into their slices of the [pool(conv2 output) | pool(x)] buffer as the trunk does; ms, GB/s counting
          x read once and y written once, and that rate as a fraction of the 6.3 TB/s copy rate
  stem    the three DeepStem convs one by one: the `kernels.conv_route` entry each runs on, ms and TFLOP/s
  block   the stride-2 blocks with resnet.FUSE_POOLED_PROJECTION on (two pools + one GEMM) and off (two pools, two convs, residual add)
  model   (`--model`) forward() of R50-D-FPN beside R50-FPN on 8 images of 800 x 1333, img/s

Writes profiles/resnet_d_bench.json and prints it as one JSON line.

    python scripts/bench_resnet_d.py [--reps 20] [--warmup 3] [--model] [--out profiles/resnet_d_bench.json]
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

COPY_GBPS = 6300.0      # the copy rate the README uses


def _timed(fn, start, end):
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def _alternate(legs, reps, warmup):
    """legs: {name: callable}.  Median ms per leg over `reps` rounds in which every leg runs once, in turn."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in legs}
    for i in range(warmup + reps):
        for k, fn in legs.items():
            t = _timed(fn, start, end)
            if i >= warmup:
                times[k].append(t)
    return {k: statistics.median(v) for k, v in times.items()}


def _model_rates(cfgs, steps, warmup):
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    models = {}
    for name, cfg in cfgs.items():
        m = build_model(cfg).eval()
        # (no FrozenBN calibration is stored for this trunk either: the ResNeXt recipe, conv3's norm scales its branch by 0.25)
        m.load_state_dict(syn.conditioned_resnext_state_dict(m.state_dict(), seed=0), strict=True)
        models[name] = m
    batch = [{"image": syn.synthetic_image(10 + i, 800, 1333), "height": 800, "width": 1333} for i in range(8)]
    times = {k: [] for k in models}
    with torch.no_grad():
        for i in range(warmup + steps):
            for name, m in models.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m(batch)
                torch.cuda.synchronize()
                if i >= warmup:
                    times[name].append(time.perf_counter() - t0)
    return {k: 8.0 / statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_d_bench.json"))
    args = ap.parse_args()

    import lvc_amd.modeling.backbone.resnet as R
    from lvc_amd import kernels as K
    from lvc_amd.utils import synthetic as syn

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    result = {"batch": 8, "image": [800, 1344], "reps": args.reps, "copy_gbps": COPY_GBPS, "device": torch.cuda.get_device_name(0)}

    # ---- the pool kernel: (block, H, W, width, in) of the stride-2 blocks
    blocks = [("res3.0", 200, 336, 128, 256), ("res4.0", 100, 168, 256, 512), ("res5.0", 50, 84, 512, 1024)]
    legs, meta = {}, {}
    for name, H, W, width, cin in blocks:
        buf = torch.empty(8, H // 2, W // 2, width + cin, device=dev)
        for what, C, sl in (("conv2 output", width, slice(0, width)), ("block input", cin, slice(width, width + cin))):
            x = torch.randn(8, H, W, C, device=dev)
            key = "%s %s [8,%d,%d,%d]" % (name, what, H, W, C)
            legs[key] = (lambda x=x, out=buf[..., sl]: K.avgpool2_into(x, out))
            meta[key] = 4.0 * (x.numel() + x.numel() // 4)
    ms = _alternate(legs, args.reps, args.warmup)
    result["pool"] = [{"case": k, "ms": ms[k], "bytes": meta[k], "gbps": meta[k] / ms[k] / 1e6, "of_copy_rate": meta[k] / ms[k] / 1e6 / COPY_GBPS}
                      for k in legs]
    del legs, buf, x

    # ---- the three DeepStem convs
    stem = R.DeepStem(3, 64, "FrozenBN")
    stem.load_state_dict(syn.seeded_module_state_dict(stem.state_dict(), seed=70), strict=True)
    stem = stem.to(dev).eval()
    x4 = torch.zeros(8, 800, 1344, 4, device=dev)
    x4[..., :3] = torch.randn(8, 800, 1344, 3, device=dev)
    with torch.no_grad():
        a1 = stem.conv1.forward_nhwc(x4)
        a2 = stem.conv2.forward_nhwc(a1)
        a3 = stem.conv3.forward_nhwc(a2)
        legs = {"conv1 3->32 3x3 s2": lambda: stem.conv1.forward_nhwc(x4), "conv2 32->32 3x3": lambda: stem.conv2.forward_nhwc(a1),
                "conv3 32->64 3x3": lambda: stem.conv3.forward_nhwc(a2), "maxpool 3x3 s2": lambda: K.maxpool2d_nhwc(a3, 3, 2, 1),
                "whole DeepStem": lambda: stem.forward_nhwc(x4)}
        ms = _alternate(legs, args.reps, args.warmup)
        basic = R.BasicStem(3, 64, "FrozenBN").to(dev).eval()
        ms.update(_alternate({"BasicStem (conv + pool, one launch)": lambda: basic.forward_nhwc(x4)}, args.reps, args.warmup))
    rows = []
    for key, conv, inp in (("conv1 3->32 3x3 s2", stem.conv1, x4), ("conv2 32->32 3x3", stem.conv2, a1), ("conv3 32->64 3x3", stem.conv3, a2)):
        n, h, w, _ = inp.shape
        ho, wo = K._out_hw(conv.packed(), h, w)
        flops = 2.0 * n * ho * wo * conv.out_channels * conv.in_channels * 9
        rows.append({"layer": key, "entry": K.conv_route(conv.packed(), n, h, w).entry, "ms": ms[key], "tflops": flops / ms[key] / 1e9})
    rows += [{"layer": k, "ms": ms[k]} for k in ("maxpool 3x3 s2", "whole DeepStem", "BasicStem (conv + pool, one launch)")]
    result["stem"] = rows
    del x4, a1, a2, a3, legs

    # ---- the stride-2 blocks, conv3 + shortcut as one GEMM or not
    rows = []
    for name, H, W, width, cin in blocks:
        blk = R.BottleneckBlockCLIP(cin, 4 * width, bottleneck_channels=width, stride=2, norm="FrozenBN")
        blk.load_state_dict(syn.seeded_module_state_dict(blk.state_dict(), seed=73), strict=True)
        blk = blk.to(dev).eval()
        x = torch.randn(8, H, W, cin, device=dev).relu_()

        def run(flag, blk=blk, x=x):
            R.FUSE_POOLED_PROJECTION = flag
            return blk.forward_nhwc(x)

        with torch.no_grad():
            ms = _alternate({"one_gemm": lambda: run(True), "two_convs": lambda: run(False)}, args.reps, args.warmup)
        R.FUSE_POOLED_PROJECTION = True
        rows.append({"block": "%s %d->%d->%d at %dx%d" % (name, cin, width, 4 * width, H, W), "one_gemm_ms": ms["one_gemm"],
                     "two_convs_ms": ms["two_convs"]})
        del blk, x
    result["block"] = rows

    if args.model:
        from lvc_amd.config.presets import base_rcnn_fpn, resnet_d_rcnn_fpn

        rates = _model_rates({"R50-D-FPN": resnet_d_rcnn_fpn(), "R50-FPN": base_rcnn_fpn()}, 8, 2)
        result["model_img_per_s"] = rates
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
