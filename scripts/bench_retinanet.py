"""Times of R50-RetinaNet inference (presets.retinanet_r_fpn, 80 classes) for a batch of 8 synthetic 800 x 1333 images on one device.
Medians of `--reps`, legs alternated in one process.  None of these is a gate.

  forward   model.forward() (wall clock, synchronised): img/s and ms per batch; the head weights are the seeded ones of
            lvc_amd.utils.synthetic.conditioned_retinanet_ -- the per-(image, level) counts of entries above SCORE_THRESH_TEST they give on
            this batch are in the file (a PRIOR_PROB-initialised head has none and would flatter the select)
  select    kernels.retinanet_select alone on that batch's head outputs: ms, GB/s counting the logits read once plus the deltas of the kept
            anchors, that rate as a fraction of the 6.3 TB/s copy rate, passes over the logits (one: rn_compact_kernel)
            (`select_sparse`: the same call on those logits shifted by -4, where almost nothing passes the threshold -- the pass over the
            logits by itself)
  nms_post  kernels.batched_nms_batch + kernels.gather_detections on the select's outputs
  layers    p6, p7 and every head layer over the five levels: the C-ABI entries its launches ran on and their summed device time

Writes profiles/retinanet_bench.json and prints it as one JSON line.

    python scripts/bench_retinanet.py [--reps 20] [--warmup 3] [--out profiles/retinanet_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retinanet_bench.json"))
    args = ap.parse_args()

    from lvc_amd import kernels as K
    from lvc_amd.config.presets import retinanet_r_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    model = syn.conditioned_retinanet_(build_model(retinanet_r_fpn()).eval(), seed=0)
    batch = [{"image": syn.synthetic_image(10 + i, 800, 1333).to(dev), "height": 800, "width": 1333} for i in range(8)]
    result = {"batch": 8, "image": [800, 1333], "classes": 80, "reps": args.reps, "copy_gbps": COPY_GBPS, "device": torch.cuda.get_device_name(0)}
    A, Kc, head, ag = model.head.num_anchors, model.num_classes, model.head, model.anchor_generator

    with torch.no_grad():
        # ---- (a) the whole forward
        times = []
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model(batch)
            torch.cuda.synchronize()
            if i >= args.warmup:
                times.append(time.perf_counter() - t0)
        ms = 1e3 * statistics.median(times)
        result["forward"] = {"ms_per_batch": ms, "img_per_s": 8e3 / ms, "detections": [len(o["instances"]) for o in out],
                             "max_survivors": model.max_survivors}

        # ---- the batch's head outputs
        images = model.preprocess_image(batch)
        n, _, hp, wp = images.tensor.shape
        x4 = images.tensor.as_strided((n, hp, wp, 4), (hp * wp * 4, wp * 4, 4, 1), images.tensor.storage_offset())
        feats = model.backbone.forward_nhwc(x4)
        logits, deltas = model.head_outputs(feats)
        thr = model.score_threshold
        cut = float(torch.log(torch.tensor(thr / (1 - thr))))
        result["entries_above_threshold"] = {name: [int(v) for v in (t[..., :A * Kc] > cut).flatten(1).sum(1).tolist()]
                                             for name, t in zip(model.in_features, logits)}
        result["levels"] = {name: list(t.shape[1:3]) for name, t in zip(model.in_features, logits)}

        # ---- (b) the select alone, (c) NMS + postprocess
        lg, dl = [t[..., :A * Kc] for t in logits], [t[..., :4 * A] for t in deltas]
        cells = list(ag.cell_anchors)

        def select():
            return K.retinanet_select(lg, dl, cells, ag.strides, ag.offset, Kc, model.topk_candidates, thr, model.box2box_transform.weights,
                                      max_survivors=model.max_survivors)

        boxes, scores, classes, index, count, status = select()
        IP = ctypes.c_int * len(lg)
        cap = model.max_survivors if model.max_survivors is not None else (1 << 30)
        workspace = int(K._lib.lib().lvc_retinanet_select_workspace_bytes(8, len(lg), A, Kc, IP(*[x.shape[1] for x in lg]), IP(*[x.shape[2] for x in lg]), model.topk_candidates, cap))
        post = torch.tensor([[1.0, 1.0, 800.0, 1333.0]] * 8, device=dev)
        D = model.max_detections_per_image

        def nms_post():
            keep, nk = K.batched_nms_batch(boxes, scores, classes, count, model.nms_threshold, max_keep=D)
            return K.gather_detections(boxes, scores, classes, index, keep, nk, D, post=post)

        # the same call on logits shifted by -4: almost nothing above the threshold, i.e. the pass over the logits by itself
        lg_sparse = [(t - 4.0).contiguous() for t in lg]

        def select_sparse():
            return K.retinanet_select(lg_sparse, dl, cells, ag.strides, ag.offset, Kc, model.topk_candidates, thr, model.box2box_transform.weights,
                                      max_survivors=model.max_survivors)

        sparse_count = select_sparse()[4]
        t = _alternate({"select": select, "select_sparse": select_sparse, "nms_post": nms_post}, args.reps, args.warmup)
        kept = int(count.sum())
        nbytes = 4.0 * sum(x.shape[0] * x.shape[1] * x.shape[2] * A * Kc for x in lg) + 16.0 * kept
        result["select"] = {"ms": t["select"], "bytes": nbytes, "gbps": nbytes / t["select"] / 1e6, "of_copy_rate": nbytes / t["select"] / 1e6 / COPY_GBPS,
                            "passes_over_logits": 1, "workspace_bytes": workspace, "candidates": count.tolist(), "status": int(status)}
        sb = 4.0 * sum(x.numel() for x in lg_sparse) + 16.0 * int(sparse_count.sum())
        result["select_sparse"] = {"ms": t["select_sparse"], "gbps": sb / t["select_sparse"] / 1e6, "of_copy_rate": sb / t["select_sparse"] / 1e6 / COPY_GBPS,
                                   "candidates": sparse_count.tolist(),
                                   "entries_above_threshold": {name: [int(v) for v in (x > cut).flatten(1).sum(1).tolist()] for name, x in zip(model.in_features, lg_sparse)}}
        result["nms_post"] = {"ms": t["nms_post"], "rows_per_image": int(scores.shape[1])}

        # ---- (d) the entry and time of every new layer: p6, p7, the towers, the predictors
        trace = []
        real = K._launch

        def traced(tag, flops, nbytes, slot, what, call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            real(tag, flops, nbytes, slot, what, call)
            e1.record()
            trace.append((what, e0, e1))

        c5 = model.backbone.bottom_up.forward_nhwc(x4)["res5"]
        top = model.backbone.top_block
        p6 = top.p6.forward_nhwc(c5)
        p6r = K.relu_backward(p6, p6)
        flist = [feats[f] for f in model.in_features]
        cls, box = head.towers()
        hidden = K.conv3x3_levels(flist, head.packed_layer(cls[0][0]), relu=True)
        layers = {"p6 (res5 2048->256, 3x3 s2)": lambda: top.p6.forward_nhwc(c5), "p7 (256->256, 3x3 s2)": lambda: top.p7.forward_nhwc(p6r),
                  "tower layer (256->256 + ReLU, 5 levels)": lambda: K.conv3x3_levels(flist, head.packed_layer(cls[0][0]), relu=True),
                  "cls_score (256->%d, 5 levels)" % (A * Kc): lambda: K.conv3x3_levels(hidden, head.packed_layer(head.cls_score)),
                  "bbox_pred (256->%d packed as %d, 5 levels)" % (4 * A, head.packed_bbox_pred().K): lambda: K.conv3x3_levels(hidden, head.packed_bbox_pred())}
        rows = []
        K._launch = traced
        try:
            for name, fn in layers.items():
                per_rep, entries = [], set()
                for i in range(args.warmup + args.reps):
                    del trace[:]
                    fn()
                    torch.cuda.synchronize()
                    entries |= {w for w, _, _ in trace}
                    if i >= args.warmup:
                        per_rep.append(sum(a.elapsed_time(b) for _, a, b in trace))
                rows.append({"layer": name, "entries": sorted(entries), "ms": statistics.median(per_rep), "launches": len(trace)})
        finally:
            K._launch = real
        result["layers"] = rows
        result["not_measured"] = ["bench.py on this commit and on its parent (run separately)", "GraphedInference / inference_on_dataset over this model"]

    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
