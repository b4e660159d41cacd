"""Time of one GroupNorm launch (csrc/group_norm.hip) at the workload's shapes: the five pyramid levels of a batch of 8 at 800 x 1333
(p2 .. p6, 256 channels, row-tile regime) and the 4conv1fc head's [8000,7,7,256] (whole-sample regime), forward and backward.
Per case: median device time, bytes moved by the algorithmic count (forward: x read + y written, and x once more where the
statistics are a pass of their own; backward: dy and x read twice in the row-tile regime / once in the whole-sample regime, dx
written) and the fraction of the HBM peak.  As a yardstick (not a gate): PyTorch-ROCm's F.group_norm on the same values (NCHW, its
native layout), alternated with ours in the same process.  Writes profiles/group_norm_bench.json and prints it as one JSON line.

    python scripts/bench_group_norm.py [--reps 20] [--warmup 3] [--out profiles/group_norm_bench.json]
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

PEAK_HBM_GBPS = 8000.0      # as bench.py: HBM3E spec


def _timed(fn, start, end):
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_norm_bench.json"))
    args = ap.parse_args()

    from lvc_amd import kernels as K

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    G, C = 32, 256
    cases = [("p2", (8, 200, 336, C)), ("p3", (8, 100, 168, C)), ("p4", (8, 50, 84, C)), ("p5", (8, 25, 42, C)), ("p6", (8, 13, 21, C)),
             ("head", (8000, 7, 7, C))]
    gamma = (1.0 + 0.3 * torch.randn(C, device=dev)).contiguous()
    beta = (0.2 * torch.randn(C, device=dev)).contiguous()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows = []
    for name, shape in cases:
        N, H, W, _ = shape
        x = torch.randn(shape, device=dev) * 3.0 + 1.0
        dy = torch.randn(shape, device=dev)
        relu = name == "head"
        tile_rows = K._gn_tile_rows(N, H, W)
        y, mean, rstd = K.group_norm_nhwc(x, gamma, beta, G, relu=relu)
        xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)      # torch's own layout
        gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        dyt = dy.permute(0, 3, 1, 2).contiguous()

        def ours_fwd():
            K.group_norm_nhwc(x, gamma, beta, G, relu=relu)

        def ours_bwd():
            K.group_norm_backward_nhwc(dy, x, mean, rstd, gamma, beta, G, relu=relu)

        def torch_fwd():
            with torch.no_grad():
                o = F.group_norm(xt, G, gt, bt, 1e-5)
                if relu:
                    F.relu_(o)

        out_t = F.relu(F.group_norm(xt, G, gt, bt, 1e-5)) if relu else F.group_norm(xt, G, gt, bt, 1e-5)

        def torch_bwd():
            torch.autograd.grad(out_t, (xt, gt, bt), dyt, retain_graph=True)

        legs = {"fwd": (ours_fwd, torch_fwd), "bwd": (ours_bwd, torch_bwd)}
        numel = x.numel()
        passes = {"fwd": (3 if tile_rows else 2), "bwd": (5 if tile_rows else 3)}
        for leg, (ours, theirs) in legs.items():
            for _ in range(args.warmup):
                ours()
                theirs()
            torch.cuda.synchronize()
            t_ours, t_torch = [], []
            for _ in range(args.reps):                       # alternated: both see the same neighbours on the box
                t_ours.append(_timed(ours, start, end))
                t_torch.append(_timed(theirs, start, end))
            ms, ms_t = statistics.median(t_ours), statistics.median(t_torch)
            nbytes = passes[leg] * numel * 4
            rows.append({"case": name, "shape": list(shape), "leg": leg, "regime": "row tiles of %d" % tile_rows if tile_rows else "whole samples",
                         "ms_median": round(ms, 4), "ms_min": round(min(t_ours), 4), "ms_max": round(max(t_ours), 4),
                         "algorithmic_bytes": nbytes, "gbps": round(nbytes / ms / 1e6, 1),
                         "frac_of_hbm_peak": round(nbytes / ms / 1e6 / PEAK_HBM_GBPS, 4),
                         "torch_group_norm_ms_median": round(ms_t, 4), "torch_over_ours": round(ms_t / ms, 3)})
        del x, dy, xt, dyt, out_t, y
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "peak_hbm_gbps": PEAK_HBM_GBPS,
           "note": "torch_group_norm_* is F.group_norm (+ relu for the head) on NCHW-contiguous copies of the same values: a yardstick, not a gate",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
