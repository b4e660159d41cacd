"""Large-scale jitter on the device: what the windowed entry costs beside resizing the whole image.

  lvc_train_input_lsj_u8 on a batch of 8 plain 480 x 640 items with an 800 x 800 target at the scales 0.5, 1.0 and 1.6 of
  ResizeScale's range (scaled sizes 300 x 400, 600 x 800, 960 x 1280; the window in the middle of what can be cropped, no flip),
  beside lvc_train_input_u8 resizing the same items to the same FULL scaled sizes, alternated in one process.  Per leg:
    *_us        time per CALL between two events around `calls` back-to-back calls.  A call builds its job table in numpy, waits for
                the previous upload, copies, and launches: the figure is the larger of the host's and the device's time per call;
    *_host_us   the host's share: wall time per call of the same loop, read before the device is waited for;
    *_blob_us   of which building the job table and picking the coefficient tables (no device involved);
  medians of the rounds and the rounds' own spread, and the bytes each form reads and writes (sources, uint8 intermediate written
  and read, fp32 batch).  The kernels' own times come from a trace, not from here:

    python scripts/bench_lsj.py [--rounds 5] [--calls 50] [--out profiles/lsj_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_lsj.py --only 1.6 --rounds 1 --calls 20 --out DIR/x.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

TARGET = (800, 800)
SOURCE = (480, 640)
SCALES = (0.5, 1.0, 1.6)


def scaled_size(s):
    """ResizeScale's arithmetic for one scale."""
    rs = np.multiply(TARGET, s)
    scale = np.minimum(rs[0] / SOURCE[0], rs[1] / SOURCE[1])
    return tuple(int(v) for v in np.round(np.multiply(SOURCE, scale)).astype(int))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsj_bench.json"))
    ap.add_argument("--only", type=float, default=None, help="one scale only (for a kernel trace)")
    a = ap.parse_args()

    from lvc_amd import kernels as K
    from lvc_amd.data import resample_coeffs
    from lvc_amd.structures import ImageList

    dev = "cuda:0"
    mean, std = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]
    g = torch.Generator().manual_seed(3)
    B = 8
    raws = [torch.randint(0, 256, SOURCE + (3,), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
    h, w = SOURCE
    legs, facts = {}, {}
    keep = []
    blob = {}
    for s in (SCALES if a.only is None else (a.only,)):
        sh, sw = scaled_size(s)
        ow, oh = min(sw, TARGET[1]), min(sh, TARGET[0])
        ox, oy = (sw - ow) // 2, (sh - oh) // 2
        items = [([(r, (0, 0, w, h), (0, 0))], (0, 0, w, h), (sh, sw), (ox, oy, ow, oh), TARGET, 128, False) for r in raws]
        Hp, Wp = ImageList.padded_size([TARGET], 32)
        lbuf = torch.empty(B, Hp, Wp, 4, device=dev)
        FHp, FWp = ImageList.padded_size([(sh, sw)], 32)
        fbuf = torch.empty(B, FHp, FWp, 4, device=dev)
        jobs = [(0, 0, w, h, sh, sw, False)] * B
        lws, fws = K.TrainInputWorkspace(dev), K.TrainInputWorkspace(dev)
        keep.append((items, lbuf, fbuf, lws, fws))
        tag = "%.1f" % s
        legs["lsj_" + tag] = (lambda items=items, lbuf=lbuf, lws=lws:
                              K.train_input_lsj_u8(items, lbuf, mean, std, resample_coeffs, workspace=lws))
        legs["full_" + tag] = (lambda jobs=jobs, fbuf=fbuf, fws=fws:
                               K.train_input_u8(raws, jobs, fbuf, mean, std, resample_coeffs, workspace=fws))
        blob["lsj_" + tag] = (lambda items=items: K.train_input_lsj_blob(items, resample_coeffs))
        by0, bh = K.lsj_band(h, sh, oy, oh, resample_coeffs)
        xb = resample_coeffs(w, sw)[0][ox:ox + ow]
        cols = int((xb[:, 0] + xb[:, 1]).max() - xb[:, 0].min())
        facts[tag] = {
            "scaled": [sh, sw], "window": [ox, oy, ow, oh], "band_rows": bh,
            # per item: source bytes touched, intermediate written + read, fp32 batch written
            "lsj_bytes": B * (bh * cols * 3 + 2 * bh * ow * 3 + Hp * Wp * 16),
            "full_bytes": B * (h * w * 3 + 2 * h * sw * 3 + FHp * FWp * 16),
            "lsj_batch": [B, Hp, Wp, 4], "full_batch": [B, FHp, FWp, 4],
        }
    for f in legs.values():
        f()
    torch.cuda.synchronize()
    us, host, blob_us = {k: [] for k in legs}, {k: [] for k in legs}, {k: [] for k in blob}
    for r in range(a.rounds + 1):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                f()
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            if r:      # round 0 warms up
                us[k].append(e0.elapsed_time(e1) * 1e3 / a.calls)
                host[k].append((t1 - t0) * 1e6 / a.calls)
        for k, f in blob.items():
            t0 = time.perf_counter()
            for _ in range(a.calls):
                f()
            if r:
                blob_us[k].append((time.perf_counter() - t0) * 1e6 / a.calls)
    out = {"workload": "batch of 8 plain 480 x 640 uint8 items; lsj = lvc_train_input_lsj_u8, 800 x 800 target, window centred, no flip; "
                       "full = lvc_train_input_u8 resizing the same items to the whole scaled size; *_us: time per call between events (the larger of host "
                       "and device time per call), *_host_us: host wall time per call, *_blob_us: the numpy job-table builder alone",
           "rounds": a.rounds, "calls_per_round": a.calls, "launches_per_lsj_call": K.TRAIN_INPUT_LSJ_LAUNCHES[-1]}
    for k in legs:
        out[k + "_us"] = [round(v, 1) for v in us[k]]
        out[k + "_us_median"] = round(statistics.median(us[k]), 1)
        out[k + "_us_spread"] = round(max(us[k]) - min(us[k]), 1)
        out[k + "_host_us_median"] = round(statistics.median(host[k]), 1)
    for k in blob:
        out[k + "_blob_us_median"] = round(statistics.median(blob_us[k]), 1)
    out["by_scale"] = facts
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
