"""Generate tests/golden/train_mosaic.npz: the reference's own mosaic training input run on CPU -- DatasetMapperMosaic (lvc/data/
mosaic.py: get_mosaic / get_mosaic9, then crop -> resize -> flip and the annotations) and MapDatasetMosaic (which items become
mosaics, of which tiles) followed by AspectRatioGroupedDataset.  Runs only where the reference tree exists; only data goes into the
fixture.  TEST INFRASTRUCTURE ONLY.

Consumers: tests/test_host_train_mosaic.py, tests/test_gpu_train_mosaic.py.

  per case cK_*: the tile images tT_image (uint8 HWC, INPUT.FORMAT order; random, 20-90 px a side, through lossless PNGs) and
      annotation lists tT_ann_* (as train_input_*.npz), the tiles' image_id, the cfg values, the numpy seed, what the reference's
      get_mosaic / get_mosaic9 computed -- canvas (x1a, y1a, x2a, y2a) and source (x1b, y1b, x2b, y2b) per tile, trim (minx1, miny1,
      maxx2, maxy2), read from the running function's own variables -- the composite's size, the drawn crop / new size / flip, and
      the reference's outputs: image (uint8 CHW), gt_boxes fp32, gt_classes, gt_ignores, ids, and the output dict's image_id /
      width / height.  Seeds are searched (first of 0..399) so that each case shows what its name says; the script asserts it.
  order_*: a toy dataset of 11 dicts, INPUT.MOSAIC = 0.5, INPUT.MOSAIC49SPLIT = 0.5, random.seed(s), the sampler seed: the tile-index
      lists of the first 40 items of each rank for world sizes 1 and 2, and the batches that leave the grouping.
  overlap_lists / overlap_found: how many random tile-size lists were put through the reference's get_mosaic / get_mosaic9 in
      search of two canvas rectangles that overlap, and how many had one.  The reference's geometry tiles the canvas without
      overlap (none was found here either), so "the later tile wins" cannot be shown by a reference case: the tests check that
      rule of the kernel against a numpy painting of hand-made rectangles instead.

    python scripts/make_golden_train_mosaic.py
"""
import os
import random
import sys
import tempfile

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden_train_input as base  # noqa: E402  (installs the reference shim and the third-party pieces)
from make_golden_train_input import XYWH, XYXY, ann, ref_annotations, ref_cfg  # noqa: E402

GOLD = base.GOLD


class Traced:
    """Runs the reference's get_mosaic / get_mosaic9 and reads, from the running frame, the rectangles it computed."""

    def __init__(self):
        self.tiles, self.trim = {}, None

    def _local(self, frame, event, arg):
        v = frame.f_locals
        if "x2b" in v and "i" in v:
            self.tiles[v["i"]] = tuple(int(v[k]) for k in ("x1a", "y1a", "x2a", "y2a", "x1b", "y1b", "x2b", "y2b"))
        if event == "return":
            self.trim = tuple(int(v[k]) for k in ("minx1", "miny1", "maxx2", "maxy2"))
        return self._local

    def _global(self, frame, event, arg):
        return self._local if frame.f_code.co_name in ("get_mosaic", "get_mosaic9") else None

    def __call__(self, fn, *args):
        sys.settrace(self._global)
        try:
            return fn(*args)
        finally:
            sys.settrace(None)


def drawn_params(mapper, composite, seed):
    return base.drawn_params(mapper, composite, seed)


def paint_count(canvas, side):
    """How many tiles cover each canvas pixel."""
    n = np.zeros((side, side), np.int64)
    for x1a, y1a, x2a, y2a in canvas:
        n[y1a:y2a, x1a:x2a] += 1
    return n


def run_case(d, k, name, rng, sizes, anns, min_sizes, max_size, sampling, crop, want):
    """want(info) -> bool on a dict of what the seed drew; the first seed of 0..399 that shows it is used."""
    from PIL import Image

    from lvc.data import mosaic as ref_mosaic

    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    mapper = ref_mosaic.DatasetMapperMosaic(ref_cfg(min_sizes, max_size, sampling, crop), True)
    with tempfile.TemporaryDirectory() as tmp:
        dicts = []
        for t, (img, a) in enumerate(zip(imgs, anns)):
            path = os.path.join(tmp, "tile%d.png" % t)
            Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(path)
            dicts.append({"file_name": path, "height": img.shape[0], "width": img.shape[1], "image_id": 100 * k + t,
                          "annotations": ref_annotations(a)})
        import copy

        tr = Traced()
        fn = ref_mosaic.get_mosaic if len(sizes) == 4 else ref_mosaic.get_mosaic9
        composite, merged = tr(fn, copy.deepcopy(dicts), imgs)
        composite = composite.copy()
        canvas = np.array([tr.tiles[t][:4] for t in range(len(sizes))], np.int64)
        source = np.array([tr.tiles[t][4:] for t in range(len(sizes))], np.int64)
        trim = np.array(tr.trim, np.int64)
        side = (2 if len(sizes) == 4 else 3) * max(sizes[0])
        count = paint_count(canvas, side)[trim[1]:trim[3], trim[0]:trim[2]]
        assert count.shape == composite.shape[:2]
        n_candidates = sum(1 for a in merged["annotations"] if a.get("iscrowd", 0) == 0)
        n_clipped = sum(1 for a in merged["annotations"] if a.get("iscrowd", 0) == 0 and len(sizes) == 9 and
                        (a["bbox"][2] == 0 or a["bbox"][3] == 0))      # get_mosaic9 left it no area: it cannot survive
        for seed in range(400):
            crop_p, size_p, flip_p = drawn_params(mapper, composite, seed)
            np.random.seed(seed)
            out = mapper(dicts)
            x0, y0, cw, ch = crop_p
            win = count[y0:y0 + ch, x0:x0 + cw]
            info = {"crop": crop_p, "size": size_p, "flip": flip_p, "n": len(out["instances"]), "candidates": n_candidates,
                    "fill": bool((win == 0).any()), "composite": composite.shape[:2]}
            if want(info):
                break
        else:
            raise RuntimeError("no seed shows case " + name)
    inst = out["instances"]
    p = "c%d_" % k
    d[p + "name"] = np.array(name)
    d[p + "n_tiles"] = np.int64(len(sizes))
    for t, (img, a) in enumerate(zip(imgs, anns)):
        q = p + "t%d_" % t
        d[q + "image"] = img
        d[q + "image_id"] = np.int64(100 * k + t)
        d[q + "ann_bbox"] = np.array([x["bbox"] for x in a], np.float64).reshape(-1, 4)
        d[q + "ann_mode"] = np.array([x["mode"] for x in a], np.int64)
        d[q + "ann_cat"] = np.array([x["cat"] for x in a], np.int64)
        d[q + "ann_iscrowd"] = np.array([-1 if x["iscrowd"] is None else x["iscrowd"] for x in a], np.int64)
        d[q + "ann_ignore"] = np.array([-1 if x["ignore"] is None else x["ignore"] for x in a], np.int64)
        d[q + "ann_id"] = np.array([-1000 if x["id"] is None else x["id"] for x in a], np.int64)
    d[p + "min_sizes"] = np.array(min_sizes, np.int64)
    d[p + "max_size"] = np.int64(max_size)
    d[p + "sampling"] = np.array(sampling)
    d[p + "crop_enabled"] = np.int64(crop is not None)
    d[p + "crop_type"] = np.array(crop[0] if crop else "relative_range")
    d[p + "crop_size"] = np.array(crop[1] if crop else (0.9, 0.9), np.float64)
    d[p + "seed"] = np.int64(seed)
    d[p + "canvas"], d[p + "source"], d[p + "trim"] = canvas, source, trim
    d[p + "composite_size"] = np.array(composite.shape[:2], np.int64)
    d[p + "fill_in_window"] = np.int64(info["fill"])
    d[p + "candidates"] = np.int64(n_candidates)
    d[p + "clipped_to_nothing"] = np.int64(n_clipped)
    d[p + "out_image"] = out["image"].numpy()
    d[p + "gt_boxes"] = inst.gt_boxes.tensor.numpy()
    d[p + "gt_classes"] = inst.gt_classes.numpy()
    d[p + "gt_ignores"] = inst.gt_ignores.numpy()
    d[p + "ids"] = inst.ids.numpy()
    d[p + "out_image_id"] = np.int64(out["image_id"])
    d[p + "out_width"], d[p + "out_height"] = np.int64(out["width"]), np.int64(out["height"])
    d[p + "crop"] = np.array(crop_p, np.int64)
    d[p + "new_size"] = np.array(size_p, np.int64)
    d[p + "flip"] = np.int64(flip_p)
    assert tuple(out["image"].shape[1:]) == tuple(size_p) and inst.gt_boxes.tensor.dtype == torch.float32
    assert out["image_id"] == 100 * k + len(sizes) - 1 and (out["height"], out["width"]) == tuple(sizes[-1])
    if tuple(size_p) == tuple(composite.shape[:2]) and not flip_p and crop is None:
        assert np.array_equal(out["image"].numpy().transpose(1, 2, 0), composite)
    print("  case %2d %-26s %d tiles composite %s seed %3d crop %s -> %s flip %d, %d of %d boxes kept, fill in window %d" %
          (k, name, len(sizes), tuple(composite.shape[:2]), seed, crop_p, size_p, flip_p, len(inst), n_candidates, info["fill"]))
    return info


def tile_anns(rng, sizes, first_id):
    """A few boxes per tile; one XYXY box, one crowd, ignore_qe and id present and absent; in a 9-tile list a small box in two
    corners of every tile (where get_mosaic9 cuts a tile, one of them is left with no area)."""
    out = []
    for t, (h, w) in enumerate(sizes):
        a = []
        for j in range(2):
            x, y = float(rng.uniform(0, 0.6 * w)), float(rng.uniform(0, 0.6 * h))
            bw, bh = float(rng.uniform(0.2 * w, 0.7 * w)), float(rng.uniform(0.2 * h, 0.7 * h))
            a.append(ann([round(x, 2), round(y, 2), round(bw, 2), round(bh, 2)], int(rng.integers(0, 20)), id=first_id + 10 * t + j,
                         ignore=(1 if (t + j) % 3 == 0 else None)))
        if len(sizes) == 9:
            a.append(ann([0.5, 0.5, 5.0, 5.0], 11, id=first_id + 10 * t + 5))
            a.append(ann([w - 5.5, h - 5.5, 5.0, 5.0], 12, id=first_id + 10 * t + 6))
        if t == 1:
            a.append(ann([3.5, 4.25, 0.6 * w, 0.7 * h], 7, mode=XYXY))                  # no id, no ignore_qe
            a.append(ann([2.0, 2.0, 10.0, 10.0], 9, iscrowd=1, id=first_id + 900))
            a.append(ann([1.0, 1.5, 8.0, 9.0], 4, iscrowd=0, ignore=0))
        out.append(a)
    return out


def gen_cases(d):
    rng = np.random.default_rng(2025)
    cases = []
    eq = [(48, 64)] * 4                                      # composite 96 x 128: MIN_SIZE 96 keeps it, neither pass resamples
    cases.append(("m4_equal_noresample_noflip", eq, (96,), 1333, "choice", None,
                  lambda i: i["size"] == (96, 128) == tuple(i["composite"]) and i["flip"] == 0))
    mixed4 = [(50, 70), (88, 40), (36, 90), (75, 62)]        # portrait and landscape; tiles 1, 2, 3 exceed tile 0 somewhere
    cases.append(("m4_mixed_crop_flip", mixed4, (64, 72, 80), 1333, "choice", ("relative_range", (0.7, 0.7)),
                  lambda i: i["flip"] == 1 and 0 < i["n"] < i["candidates"]))
    small0 = [(22, 31), (60, 85), (90, 45), (70, 70)]        # tile 0 the smallest: the canvas is 62 x 62, every other tile is cut
    cases.append(("m4_tile0_smallest", small0, (80,), 1333, "choice", ("relative_range", (0.7, 0.7)), lambda i: i["n"] > 0))
    mixed9 = [(40, 56), (45, 90), (85, 30), (70, 52), (33, 66), (90, 90), (24, 41), (58, 77), (81, 20)]
    cases.append(("m9_mixed_crop_noflip", mixed9, (120, 128), 1333, "choice", ("relative_range", (0.7, 0.7)),
                  lambda i: i["flip"] == 0 and i["fill"] and 0 < i["n"] < i["candidates"]))
    # ResizeShortestEdge keeps the width only when MAX_SIZE_TRAIN cuts a window at least twice as tall as wide by one pixel:
    # 120 x 50 -> short edge 50 -> 120 > 119 -> scale 119/120 -> int(49.58 + 0.5) = 50 wide, 119 tall
    rot9 = mixed9[3:] + mixed9[:3]
    cases.append(("m9_width_unchanged", rot9, (50,), 119, "choice", ("absolute", (120, 50)),
                  lambda i: i["crop"][2:] == (50, 120) and i["size"] == (119, 50)))
    infos = []
    for k, c in enumerate(cases):
        sizes = c[1]
        infos.append(run_case(d, k, c[0], rng, sizes, tile_anns(rng, sizes, 1000 * (k + 1)), *c[2:]))
    d["n"] = np.int64(len(cases))
    # what the names say, beyond the per-seed predicates
    assert any(h > mixed4[0][0] or w > mixed4[0][1] for h, w in mixed4[1:])
    assert all(h * w > small0[0][0] * small0[0][1] for h, w in small0[1:])
    assert int(d["c3_clipped_to_nothing"]) > 0 and len(d["c3_gt_classes"]) <= int(d["c3_candidates"]) - int(d["c3_clipped_to_nothing"])


def gen_overlap_search(d, n_lists=400):
    """Canvas rectangles of the reference's own functions on random tile-size lists: do two of them ever overlap?"""
    import copy

    from lvc.data import mosaic as ref_mosaic

    rng = np.random.default_rng(7)
    found = 0
    for it in range(n_lists):
        n = 4 if it % 2 == 0 else 9
        lo, hi = ((20, 90), (1, 8), (1, 200))[it % 3]
        sizes = [(int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))) for _ in range(n)]
        imgs = [np.zeros((h, w, 3), np.uint8) for h, w in sizes]
        dicts = [{"annotations": []} for _ in sizes]
        tr = Traced()
        tr(ref_mosaic.get_mosaic if n == 4 else ref_mosaic.get_mosaic9, copy.deepcopy(dicts), imgs)
        side = (2 if n == 4 else 3) * max(sizes[0])
        found += int((paint_count([tr.tiles[t][:4] for t in range(n)], side) > 1).any())
    d["overlap_lists"], d["overlap_found"] = np.int64(n_lists), np.int64(found)
    print("  overlap search: %d of %d random tile lists have two canvas rectangles that overlap" % (found, n_lists))


def gen_order(d):
    from detectron2.data.common import AspectRatioGroupedDataset
    from detectron2.data.samplers import TrainingSampler
    from lvc.data.mosaic import MapDatasetMosaic

    rng = np.random.default_rng(5)
    N, seed, pyseed, bs, n_items = 11, 7, 13, 2, 40
    wide = rng.integers(0, 2, N).astype(bool)
    width = np.where(wide, 200, 120).astype(np.int64)
    height = np.where(wide, 120, 200).astype(np.int64)
    width[3] = height[3] = 150
    cfg = ref_cfg((64,), 1333, "choice", None)
    cfg.defrost()
    cfg.INPUT.MOSAIC, cfg.INPUT.MOSAIC49SPLIT = 0.5, 0.5
    cfg.freeze()
    dataset = [{"index": i, "width": int(width[i]), "height": int(height[i])} for i in range(N)]
    d.update({"order_width": width, "order_height": height, "order_seed": np.int64(seed), "order_pyseed": np.int64(pyseed),
              "order_batch_size": np.int64(bs), "order_mosaic": np.float64(0.5), "order_split": np.float64(0.5)})

    def mosaic_func(dicts):      # what leaves the reference's mapper: the LAST tile's dict
        return {"tiles": [x["index"] for x in dicts], "width": dicts[-1]["width"], "height": dicts[-1]["height"]}

    def plain_func(x):
        return {"tiles": [x["index"]], "width": x["width"], "height": x["height"]}

    for world in (1, 2):
        for rank in range(world):
            mds = MapDatasetMosaic(dataset, mosaic_func, plain_func, cfg)
            s = TrainingSampler(N, seed=seed)
            s._rank, s._world_size = rank, world
            it = iter(s)
            random.seed(pyseed)
            rows = [mds[int(next(it))] for _ in range(n_items)]
            tiles = np.full((n_items, 9), -1, np.int64)
            for r, row in enumerate(rows):
                tiles[r, :len(row["tiles"])] = row["tiles"]
            pos = {id(x): r for r, x in enumerate(rows)}
            batches = [[pos[id(x)] for x in b] for b in AspectRatioGroupedDataset(rows, bs)]      # by position in the stream
            d["order_w%d_r%d_tiles" % (world, rank)] = tiles
            d["order_w%d_r%d_batches" % (world, rank)] = np.array(batches, np.int64)
            kinds = [len(r["tiles"]) for r in rows]
            assert {1, 4, 9} == set(kinds)
            print("  order world %d rank %d: %d plain, %d of 4, %d of 9; %d batches" %
                  (world, rank, kinds.count(1), kinds.count(4), kinds.count(9), len(batches)))


if __name__ == "__main__":
    d = {}
    gen_cases(d)
    gen_overlap_search(d)
    gen_order(d)
    base.save("train_mosaic", d)
