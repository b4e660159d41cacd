"""Time of the grouped 3x3 convolution (csrc/conv_grouped.hip) at X-101-32x8d's conv2 shapes for a batch of 8 at 800 x 1333: the four
stride-1 shapes of res2..res5 and the three stride-2 first-block shapes, forward, data gradient and weight gradient.  Per leg: median
device time of `--reps` launches, GB/s by the algorithmic byte count (x once + y once + weights) and that rate as a fraction of the
6.3 TB/s copy rate.  As the yardstick (not a gate): PyTorch-ROCm's F.conv2d(groups=) in fp32 on the same values, NCHW and channels_last,
alternated with ours in the same process; the better of the two counts.  `--model`: X-101-32x8d-FPN and R101-FPN inference through
forward() on 8 images of 800 x 1333 in the same process (img/s).  Writes profiles/grouped_conv_bench.json and prints it as one JSON line.

    python scripts/bench_grouped_conv.py [--reps 20] [--warmup 3] [--model] [--out profiles/grouped_conv_bench.json]
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


def _timed(fn, start, end):
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def _model_rate(cfg, steps, warmup):
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    model = build_model(cfg).eval()
    model.load_state_dict(syn.conditioned_resnext_state_dict(model.state_dict(), seed=0), strict=True)
    batch = [{"image": syn.synthetic_image(10 + i, 800, 1333), "height": 800, "width": 1333} for i in range(8)]
    times = []
    with torch.no_grad():
        for i in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model(batch)
            torch.cuda.synchronize()
            if i >= warmup:
                times.append(time.perf_counter() - t0)
    return 8.0 / statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_conv_bench.json"))
    args = ap.parse_args()

    from lvc_amd import kernels as K

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    G = 32
    cases = [("res2", (8, 200, 336, 256), 1), ("res3", (8, 100, 168, 512), 1), ("res4", (8, 50, 84, 1024), 1), ("res5", (8, 25, 42, 2048), 1),
             ("res3.0", (8, 200, 336, 512), 2), ("res4.0", (8, 100, 168, 1024), 2), ("res5.0", (8, 50, 84, 2048), 2)]
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows = []
    for name, shape, stride in cases:
        N, H, W, C = shape
        cg = C // G
        x = torch.randn(shape, device=dev)
        w = torch.randn(C, cg, 3, 3, device=dev) / (9 * cg) ** 0.5
        scale = (1.0 + 0.3 * torch.randn(C, device=dev)).contiguous()
        shift = (0.2 * torch.randn(C, device=dev)).contiguous()
        pc = K.pack_conv(w, stride=stride, pad=1, affine=(scale, shift), groups=G)
        pcd = K.pack_conv_dgrad(w, scale, 1, groups=G)
        y = K.conv2d_nhwc(x, pc, relu=True)
        dy = torch.randn_like(y)
        x_nchw = x.permute(0, 3, 1, 2).contiguous()
        x_cl = x_nchw.contiguous(memory_format=torch.channels_last)
        w_cl = w.contiguous(memory_format=torch.channels_last)
        legs = {
            "fwd": lambda: K.conv2d_nhwc(x, pc, relu=True),
            "dgrad": lambda: K.conv_dgrad(dy, pcd, x.shape, stride),
            "wgrad": lambda: K.conv_wgrad_grouped(x, dy, scale, G, stride),
            "torch_nchw": lambda: F.conv2d(x_nchw, w, None, stride, 1, 1, G),
            "torch_cl": lambda: F.conv2d(x_cl, w_cl, None, stride, 1, 1, G),
        }
        ms = {k: [] for k in legs}
        for i in range(args.warmup + args.reps):
            for k, fn in legs.items():      # alternated: every leg sees the same clocks and the same neighbours
                t = _timed(fn, start, end)
                if i >= args.warmup:
                    ms[k].append(t)
        nbytes = 4.0 * (x.numel() + y.numel() + w.numel())
        row = {"case": name, "shape": list(shape), "stride": stride, "cg": cg, "bytes": nbytes}
        for k in legs:
            med = statistics.median(ms[k])
            row[k] = {"ms": round(med, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4), "gbps": round(nbytes / med / 1e6, 1),
                      "of_copy_rate": round(nbytes / med / 1e6 / COPY_GBPS, 3)}
        row["torch_best_ms"] = min(row["torch_nchw"]["ms"], row["torch_cl"]["ms"])
        row["fwd_vs_torch"] = round(row["torch_best_ms"] / row["fwd"]["ms"], 3)
        rows.append(row)
        print("%-7s cg %2d s%d  fwd %.3f ms (%.0f GB/s)  dgrad %.3f  wgrad %.3f  torch nchw %.3f  channels_last %.3f" % (
            name, cg, stride, row["fwd"]["ms"], row["fwd"]["gbps"], row["dgrad"]["ms"], row["wgrad"]["ms"], row["torch_nchw"]["ms"],
            row["torch_cl"]["ms"]), file=sys.stderr)
        del x, y, dy, x_nchw, x_cl
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "copy_gbps": COPY_GBPS, "layers": rows}
    if args.model:
        from lvc_amd.config.presets import base_rcnn_fpn, resnext_rcnn_fpn

        out["model_img_per_s"] = {"X-101-32x8d-FPN": round(_model_rate(resnext_rcnn_fpn(), 5, 2), 2),
                                  "R101-FPN": round(_model_rate(base_rcnn_fpn(depth=101), 5, 2), 2)}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
