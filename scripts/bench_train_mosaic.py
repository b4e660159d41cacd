"""Mosaic training input: what the tiled entry costs.

  entry   lvc_train_input_tiles_u8 on a batch of 8 PLAIN items (one tile each) against lvc_train_input_u8 on the same items,
          alternated in one process: device time per call (events), medians of the rounds and the rounds' own spread.
  loader  the cfg-3 training step (as scripts/bench_train_input.py: 8 images per step, 480 x 800 sources resized to 800 x 1333-class)
          fed by build_detection_train_mosaic_loader at INPUT.MOSAIC 0.5 with INPUT.MOSAIC49SPLIT 1.0 (4 tiles) and 0.0 (9 tiles),
          against the same step on a resident, pre-built batch of that loader; alternated blocks, medians.
  `--mode loader --split S` runs the loader leg alone (for a kernel trace).

    python scripts/bench_train_mosaic.py [--rounds 5] [--steps 20] [--out profiles/train_mosaic_bench.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_train_input import dataset  # noqa: E402


def bench_entry(rounds, calls=50):
    from lvc_amd import kernels as K
    from lvc_amd.data import AugmentationList, RandomCrop, RandomFlip, ResizeShortestEdge, resample_coeffs
    from lvc_amd.structures import ImageList

    dev = "cuda:0"
    mean, std = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]
    aug = AugmentationList([RandomCrop("relative_range", (0.9, 0.9)), ResizeShortestEdge((800,), 1333, "choice"), RandomFlip()])
    np.random.seed(3)
    raws = [d["raw"].to(dev) for d in dataset(8)]
    ps = [aug.draw(r.shape[0], r.shape[1])[1] for r in raws]
    Hp, Wp = ImageList.padded_size([p.new_size for p in ps], 32)
    bufs = [torch.empty(8, Hp, Wp, 4, device=dev) for _ in range(2)]
    jobs = [p.job() for p in ps]
    items = [([(r, (0, 0, r.shape[1], r.shape[0]), (0, 0))], tuple(p.crop), p.new_size[0], p.new_size[1], p.flip) for r, p in zip(raws, ps)]
    ws = [K.TrainInputWorkspace(dev), K.TrainInputWorkspace(dev)]
    legs = {"plain_entry": lambda: K.train_input_u8(raws, jobs, bufs[0], mean, std, resample_coeffs, workspace=ws[0]),
            "tiles_entry": lambda: K.train_input_tiles_u8(items, bufs[1], mean, std, resample_coeffs, workspace=ws[1])}
    for f in legs.values():
        f()
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[1])
    us = {k: [] for k in legs}
    for r in range(rounds + 1):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            e1.synchronize()
            if r:      # round 0 warms up
                us[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    out = {"entry_workload": "8 plain 480 x 800 images -> crop 0.9, resize to 800 x 1333-class, flip; time per call incl. its upload",
           "entry_calls_per_round": calls}
    for k in legs:
        out[k + "_us"] = [round(v, 1) for v in us[k]]
        out[k + "_us_median"] = round(statistics.median(us[k]), 1)
        out[k + "_us_spread"] = round(max(us[k]) - min(us[k]), 1)
    out["tiles_over_plain"] = round(out["tiles_entry_us_median"] / out["plain_entry_us_median"], 4)
    return out


def bench_loader(a, split, only_loader=False):
    from lvc_amd.config import set_global_cfg
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.data import build_detection_train_mosaic_loader
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
    cfg.INPUT.CROP.SIZE = [0.7, 0.7]
    cfg.INPUT.MOSAIC, cfg.INPUT.MOSAIC49SPLIT = 0.5, split
    cfg.SOLVER.IMS_PER_BATCH = a.batch
    set_global_cfg(cfg)
    model = build_model(cfg)
    syn.conditioned_r50_fpn_(model)
    model.train()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, weight_decay=1e-4)
    torch.manual_seed(20)
    np.random.seed(20)
    random.seed(20)
    loader = build_detection_train_mosaic_loader(cfg, dataset(64), seed=1, size_divisibility=model.backbone.size_divisibility)
    first = next(loader)
    pb = first[0]["prepared"]
    pb.ready.synchronize()
    fixed = PreparedBatch(pb.buffer.clone(), list(pb.sizes), None)
    resident = [dict(b, prepared=fixed) for b in first]
    tiles = []

    def from_loader():
        batch = next(loader)
        tiles.extend(len(b["tile_indices"]) for b in batch)
        return batch

    def block(get):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            losses = model(get())
            opt.zero_grad()
            sum(losses.values()).backward()
            opt.step()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v).all()) for v in losses.values())
        return a.batch * a.steps / (time.perf_counter() - t0)

    legs = {"resident": lambda: resident, "loader": from_loader}
    order = ["loader"] if only_loader else ["resident", "loader"]
    rates = {k: [] for k in order}
    with EventStorage(0):
        for k in order:
            block(legs[k])
        for _ in range(a.rounds):
            for k in order:
                rates[k].append(block(legs[k]))
    out = {"items_plain_4_9": [tiles.count(1), tiles.count(4), tiles.count(9)]}
    for k in order:
        out[k + "_img_per_s"] = [round(v, 1) for v in rates[k]]
        out[k + "_img_per_s_median"] = round(statistics.median(rates[k]), 1)
    if not only_loader:
        out["loader_over_resident"] = round(out["loader_img_per_s_median"] / out["resident_img_per_s_median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--mode", choices=["all", "entry", "loader"], default="all")
    ap.add_argument("--split", type=float, default=1.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {"workload": "cfg3 training step, %d images of 800 x 1333-class per step, 1 GPU; INPUT.MOSAIC 0.5, CROP 0.7" % a.batch,
           "rounds": a.rounds, "steps_per_block": a.steps}
    if a.mode in ("all", "entry"):
        out.update(bench_entry(a.rounds))
    if a.mode == "loader":
        out["split_%g" % a.split] = bench_loader(a, a.split, only_loader=True)
    if a.mode == "all":
        for split in (1.0, 0.0):
            out["split_%g" % split] = bench_loader(a, split)
    print(json.dumps(out))
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
