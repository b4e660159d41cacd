"""Colour jitter on the device: what the extra pass costs.

  entry   lvc_color_jitter_tiles_u8 on a batch of 8 -- plain 480 x 800 items (crop 0.9) and 4-tile mosaics of them (crop 0.7), four
          steps each -- beside lvc_train_input_u8 on the same plain items, alternated in one process: device time per call (events,
          the call's upload included), medians of the rounds and the rounds' own spread; and beside the time the algorithmic byte
          count (two reads and one write of the crop windows) takes at the HBM copy rate of an MI355X (6.3 TB/s measured).
  loader  the cfg-3 training step (as scripts/bench_train_mosaic.py: 8 images per step, 480 x 800 sources resized to
          800 x 1333-class, CROP 0.7) fed by the loader with the jitter off and on, against the same step on a resident, pre-built
          batch; alternated blocks in one process, medians.  Three settings: plain (INPUT.MOSAIC 0), 4-tile and 9-tile mosaics at
          INPUT.MOSAIC 0.5.  `host_draw_us`: the host half of one batch (draws + annotations), timed alone, jitter off and on.

    python scripts/bench_color_jitter.py [--rounds 5] [--steps 20] [--out profiles/color_jitter_bench.json]
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

HBM_BYTES_PER_US = 6.3e6      # 6.3 TB/s: the measured float4 copy rate of an MI355X


def bench_entry(rounds, calls=50):
    from lvc_amd import kernels as K
    from lvc_amd.data import AugmentationList, ColorJitter, RandomCrop, RandomFlip, ResizeShortestEdge, resample_coeffs
    from lvc_amd.data.mosaic import MosaicInputParams, mosaic_layout
    from lvc_amd.structures import ImageList

    dev = "cuda:0"
    mean, std = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]
    np.random.seed(3)
    torch.manual_seed(3)
    raws = [d["raw"].to(dev) for d in dataset(8)]

    def draws(crop, sizes):
        aug = AugmentationList([RandomCrop("relative_range", (crop, crop)), ColorJitter(), ResizeShortestEdge((800,), 1333, "choice"),
                                RandomFlip()])
        return [aug.draw(h, w)[1] for h, w in sizes]

    ps = draws(0.9, [r.shape[:2] for r in raws])
    plain_items = [([(r, (0, 0, r.shape[1], r.shape[0]), (0, 0))], tuple(p.crop), p.jitter[0], p.jitter[1]) for r, p in zip(raws, ps)]
    mosaic_items = []
    for i in range(8):
        tiles = [raws[(i + k) % 8] for k in range(4)]
        lay = mosaic_layout([t.shape[:2] for t in tiles])
        d = draws(0.7, [lay.size])[0]
        p = MosaicInputParams(*lay.size, lay)
        p.crop = d.crop
        item = p.tiles_item(tiles)
        mosaic_items.append((item[0], item[1], d.jitter[0], d.jitter[1]))
    Hp, Wp = ImageList.padded_size([p.new_size for p in ps], 32)
    buf = torch.empty(8, Hp, Wp, 4, device=dev)
    jobs = [p.job() for p in ps]
    ws = K.TrainInputWorkspace(dev)
    jw = [K.ColorJitterWorkspace(dev), K.ColorJitterWorkspace(dev)]
    legs = {"train_input_plain": lambda: K.train_input_u8(raws, jobs, buf, mean, std, resample_coeffs, workspace=ws),
            "jitter_plain": lambda: K.color_jitter_tiles_u8(plain_items, workspace=jw[0]),
            "jitter_mosaic4": lambda: K.color_jitter_tiles_u8(mosaic_items, workspace=jw[1])}
    for f in legs.values():
        f()
    torch.cuda.synchronize()
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
    out = {"entry_workload": "batch of 8, four steps per item: plain 480 x 800 images, crop 0.9; 4-tile mosaics of them, crop 0.7; "
                             "train_input = lvc_train_input_u8 on the plain items (resize to 800 x 1333-class); time per call incl. its upload",
           "entry_calls_per_round": calls}
    for k in legs:
        out[k + "_us"] = [round(v, 1) for v in us[k]]
        out[k + "_us_median"] = round(statistics.median(us[k]), 1)
        out[k + "_us_spread"] = round(max(us[k]) - min(us[k]), 1)
    for name, items in (("plain", plain_items), ("mosaic4", mosaic_items)):
        crop_bytes = sum(it[1][2] * it[1][3] * 3 for it in items)
        out["jitter_%s_crop_bytes" % name] = crop_bytes
        out["jitter_%s_us_at_hbm_rate" % name] = round(3 * crop_bytes / HBM_BYTES_PER_US, 2)
    return out


def bench_loader(a, mosaic, split):
    from lvc_amd.config import set_global_cfg
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.data import build_detection_train_loader, build_detection_train_mosaic_loader
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
    cfg.INPUT.MOSAIC, cfg.INPUT.MOSAIC49SPLIT = mosaic, split
    cfg.SOLVER.IMS_PER_BATCH = a.batch
    set_global_cfg(cfg)
    model = build_model(cfg)
    syn.conditioned_r50_fpn_(model)
    model.train()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, weight_decay=1e-4)
    torch.manual_seed(20)
    np.random.seed(20)
    random.seed(20)
    data = dataset(64)
    build = build_detection_train_mosaic_loader if mosaic > 0 else build_detection_train_loader
    loaders = {}
    for name, key in (("loader_off", False), ("loader_on", True)):
        c = cfg.clone()
        c.INPUT.COLOR_JITTER = key
        loaders[name] = build(c, data, seed=1, size_divisibility=model.backbone.size_divisibility, color_jitter=True)
    first = next(loaders["loader_off"])
    pb = first[0]["prepared"]
    pb.ready.synchronize()
    fixed = PreparedBatch(pb.buffer.clone(), list(pb.sizes), None)
    resident = [dict(b, prepared=fixed) for b in first]

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

    legs = {"resident": lambda: resident, "loader_off": lambda: next(loaders["loader_off"]), "loader_on": lambda: next(loaders["loader_on"])}
    rates = {k: [] for k in legs}
    with EventStorage(0):
        for k in legs:
            block(legs[k])
        for _ in range(a.rounds):
            for k in legs:
                rates[k].append(block(legs[k]))
    out = {}
    for k in legs:
        out[k + "_img_per_s"] = [round(v, 1) for v in rates[k]]
        out[k + "_img_per_s_median"] = round(statistics.median(rates[k]), 1)
    for k in ("loader_off", "loader_on"):
        out[k + "_over_resident"] = round(out[k + "_img_per_s_median"] / out["resident_img_per_s_median"], 4)
    return out


def bench_host_draw(a, reps=40):
    """The host half of a batch of plain items alone: draws and annotations, with and without the jitter's draws."""
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.data import DatasetMapper

    data = dataset(a.batch)
    out = {}
    for name, key in (("off", False), ("on", True)):
        cfg = base_rcnn_fpn(num_classes=20, device="cuda:0")
        cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN = (800,), 1333
        cfg.INPUT.CROP.ENABLED, cfg.INPUT.CROP.TYPE, cfg.INPUT.CROP.SIZE = True, "relative_range", [0.7, 0.7]
        cfg.INPUT.COLOR_JITTER = key
        mapper = DatasetMapper.from_config(cfg, True, color_jitter=True)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for d in data:
                mapper.draw(d)
            ts.append((time.perf_counter() - t0) * 1e6)
        out["host_draw_us_per_batch_jitter_" + name] = round(statistics.median(ts), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--mode", choices=["all", "entry", "loader"], default="all")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {"workload": "cfg3 training step, %d images of 800 x 1333-class per step, 1 GPU; CROP 0.7; INPUT.COLOR_JITTER off / on" % a.batch,
           "rounds": a.rounds, "steps_per_block": a.steps}
    if a.mode in ("all", "entry"):
        out.update(bench_entry(a.rounds))
    if a.mode in ("all", "loader"):
        out.update(bench_host_draw(a))
        for name, mosaic, split in (("plain", 0.0, 0.0), ("mosaic4", 0.5, 1.0), ("mosaic9", 0.5, 0.0)):
            out[name] = bench_loader(a, mosaic, split)
    print(json.dumps(out))
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
