"""Training step rate fed by the device training-input loader against the same step on a resident, pre-built batch.

cfg-3 (COCO 30-shot novel fine-tune, R50-FPN, only the box predictor trains; bench.py train_leg) with 8 images per step.  The
loader (lvc_amd.data.build_detection_train_loader) reads uint8 480 x 800 images from pinned host memory and prepares every batch on
the device -- INPUT.CROP relative_range 0.9, resize to 800 (<= 1333), flip, normalise, pad.  The resident leg repeats one batch the
loader has prepared (same shapes, same ground truth, nothing to prepare).  Both legs run in the SAME process, alternated in blocks;
the medians of the blocks and their ratio are reported.  `--mode loader` / `--mode resident` run one leg only (for a kernel trace).

    python scripts/bench_train_input.py [--rounds 5] [--steps 20] [--out profiles/train_input_bench.json]
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


def dataset(n, h=480, w=800):
    g = torch.Generator().manual_seed(1)
    out = []
    for i in range(n):
        raw = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).pin_memory()
        annos = []
        for k in range(8):
            x, y = float(torch.rand((), generator=g)) * (w - 200), float(torch.rand((), generator=g)) * (h - 200)
            bw, bh = 30 + float(torch.rand((), generator=g)) * 150, 30 + float(torch.rand((), generator=g)) * 150
            annos.append({"bbox": [x, y, bw, bh], "bbox_mode": 1, "category_id": int(torch.randint(0, 20, (), generator=g))})
        out.append({"raw": raw, "height": h, "width": w, "image_id": i, "annotations": annos})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--mode", choices=["both", "loader", "resident"], default="both")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    from lvc_amd.config import set_global_cfg
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.data import build_detection_train_loader
    from lvc_amd.data.build import PreparedBatch
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn
    from lvc_amd.utils.events import EventStorage

    cfg = base_rcnn_fpn(num_classes=20, device="cuda:0")
    cfg.MODEL.BACKBONE.FREEZE = True
    cfg.MODEL.PROPOSAL_GENERATOR.FREEZE = True
    cfg.MODEL.ROI_HEADS.FREEZE_FEAT = True
    cfg.INPUT.MIN_SIZE_TRAIN = (800,)
    cfg.INPUT.MAX_SIZE_TRAIN = 1333
    cfg.INPUT.CROP.ENABLED = True
    cfg.INPUT.CROP.TYPE = "relative_range"
    cfg.INPUT.CROP.SIZE = [0.9, 0.9]
    cfg.SOLVER.IMS_PER_BATCH = a.batch
    set_global_cfg(cfg)
    model = build_model(cfg)
    syn.conditioned_r50_fpn_(model)
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=1e-4)
    torch.manual_seed(20)
    np.random.seed(20)
    loader = build_detection_train_loader(cfg, dataset(64), seed=1, size_divisibility=model.backbone.size_divisibility)
    first = next(loader)
    pb = first[0]["prepared"]
    pb.ready.synchronize()
    fixed = PreparedBatch(pb.buffer.clone(), list(pb.sizes), None)
    resident = [dict(b, prepared=fixed) for b in first]

    def step(batch):
        losses = model(batch)
        opt.zero_grad()
        sum(losses.values()).backward()
        opt.step()
        return losses

    def block(get):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            losses = step(get())
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v).all()) for v in losses.values())
        return a.batch * a.steps / (time.perf_counter() - t0)

    legs = {"resident": lambda: resident, "loader": lambda: next(loader)}
    order = ["resident", "loader"] if a.mode == "both" else [a.mode]
    rates = {k: [] for k in order}
    with EventStorage(0):
        for k in order:      # warm-up of either leg
            block(legs[k])
        for _ in range(a.rounds):
            for k in order:
                rates[k].append(block(legs[k]))
    out = {"workload": "cfg3 training step, %d images of 800 x 1333-class per step, 1 GPU" % a.batch, "rounds": a.rounds,
           "steps_per_block": a.steps}
    for k in order:
        out[k + "_img_per_s"] = [round(v, 1) for v in rates[k]]
        out[k + "_img_per_s_median"] = round(statistics.median(rates[k]), 1)
    if a.mode == "both":
        out["loader_over_resident"] = round(out["loader_img_per_s_median"] / out["resident_img_per_s_median"], 4)
        out["per_round_ratio"] = [round(l / r, 4) for l, r in zip(rates["loader"], rates["resident"])]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
