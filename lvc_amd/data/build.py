"""build_detection_train_loader (reference lvc/data/build.py:165-232) with the images prepared on the device.

The reference maps every image on CPU workers (file decode, crop, Pillow resize, flip) and leaves normalising, padding and batching
to the model.  Here the loader draws the transforms and maps the annotations on the host (dataset_mapper.DatasetMapper.draw), then
prepares the pixels of the WHOLE batch with one kernel call (csrc/train_input.hip: two launches, every table in one upload) on a side
stream, straight into the padded NHWC4 fp32 batch the model's trunk reads.  Two batch buffers rotate: batch k+1 is prepared while
step k runs.  Streams meet through events only -- the model's stream waits for the batch's `ready` event (GeneralizedRCNN.
preprocess_image, through `PreparedBatch.image_list`), and the side stream waits, before it overwrites a buffer, for the event the
consumer's stream recorded when the NEXT batch was asked for (by then the step that read the buffer has been queued in full).

Order of images: the reference's TrainingSampler (detectron2/data/samplers/distributed_sampler.py:12-54: seeded torch.randperm
shuffles, rank-strided) followed by its aspect-ratio grouping (detectron2/data/common.py:115-149: two buckets by w > h, a batch
leaves when its bucket is full) when DATALOADER.ASPECT_RATIO_GROUPING is set (the default).

Mosaic (INPUT.MOSAIC, INPUT.MOSAIC49SPLIT) has a loader of its own, as in the reference, whose trainer picks
build_detection_train_mosaic_loader when the key is set (lvc/engine/defaults.py:518): a sampled index becomes, by MapDatasetMosaic's
draws from Python's `random`, a plain item or a mosaic of 4 or 9 dataset items; the batch -- plain and mosaic items mixed -- is
still one kernel call (lvc_train_input_tiles_u8: the tiles are read in place, no canvas in memory).

Colour jitter (INPUT.COLOR_JITTER; both builders take `color_jitter=True` to follow the key -- without it a cfg that sets the key is
refused, as it always was): the items whose draw carries a jitter go through one more call on the side stream
(lvc_color_jitter_tiles_u8, csrc/color_jitter.hip: two launches for the batch), which writes their jittered crop windows into a
scratch of the rotating buffer; lvc_train_input_u8 then resizes those as plain images.  A batch without a jitter item takes the
calls it always took.

Large-scale jitter (INPUT.LSJ; both builders take `lsj=True` to follow the key, or a transforms.LargeScaleJitter): the batch -- plain
items, mosaics and jittered crops alike -- is one call of lvc_train_input_lsj_u8 on the same side stream, buffers and events, which
computes only the window of each scaled image that FixedSizeCrop keeps.  Without it every call made before is made unchanged.
"""
import itertools
import os

import torch

from .. import distributed as dist
from .. import kernels as K
from ..structures import ImageList
from .dataset_mapper import DatasetMapper, check_supported, jitter_allow, jitter_item, plain_tiles
from .transforms import resample_coeffs


class TrainingSampler:
    """An infinite stream of indices: shuffle(range(size)) + shuffle(range(size)) + ..., every world_size-th one from `rank` on."""

    def __init__(self, size, shuffle=True, seed=None, rank=None, world_size=None):
        assert size > 0
        self._size, self._shuffle = int(size), shuffle
        self._rank = dist.get_rank() if rank is None else int(rank)
        self._world_size = dist.get_world_size() if world_size is None else int(world_size)
        if seed is None:
            if self._world_size > 1:
                raise ValueError("TrainingSampler: every rank must be given the same seed")
            seed = int.from_bytes(os.urandom(4), "little")
        self._seed = int(seed)

    def __iter__(self):
        yield from itertools.islice(self._infinite_indices(), self._rank, None, self._world_size)

    def _infinite_indices(self):
        g = torch.Generator()
        g.manual_seed(self._seed)
        while True:
            if self._shuffle:
                yield from torch.randperm(self._size, generator=g).tolist()
            else:
                yield from range(self._size)


class AspectRatioGrouper:
    """AspectRatioGroupedDataset over anything with "width" / "height": bucket 0 holds w > h, bucket 1 the rest; a bucket that
    reaches batch_size leaves as a batch."""

    def __init__(self, dataset, batch_size):
        self.dataset, self.batch_size = dataset, int(batch_size)
        self._buckets = [[] for _ in range(2)]

    def __iter__(self):
        for d in self.dataset:
            bucket = self._buckets[0 if d["width"] > d["height"] else 1]
            bucket.append(d)
            if len(bucket) == self.batch_size:
                yield bucket[:]
                del bucket[:]


def _plain_batches(dataset, batch_size):
    """BatchSampler(drop_last=True) over an infinite stream."""
    it = iter(dataset)
    while True:
        yield [next(it) for _ in range(batch_size)]


def _lsj_batch(drawn):
    """Whether the batch goes through the large-scale jitter: all of its items or none (one mapper setting draws them all)."""
    n = sum(1 for _, _, p in drawn if p.lsj is not None)
    if n not in (0, len(drawn)):
        raise ValueError("a batch mixes items with and without the large-scale jitter: give both mappers the same `lsj`")
    return n > 0


class PreparedBatch:
    """A training batch whose images are already normalised, padded and batched on the device.  Every item of the loader's
    `batched_inputs` carries the same PreparedBatch under "prepared" (and its own "slot" in it, its dataset "index" and the drawn
    "train_input_params"); GeneralizedRCNN.preprocess_image takes the batch as it is."""

    def __init__(self, buffer, sizes, ready):
        self.buffer, self.sizes, self.ready = buffer, sizes, ready      # [B,Hp,Wp,4] fp32, [(h, w)], the event that ends its kernels

    def image_list(self, device=None):
        """The ImageList preprocess_image would have built; the calling stream waits for the batch first."""
        if self.ready is not None:
            torch.cuda.current_stream(self.buffer.device).wait_event(self.ready)
        return ImageList(self.buffer.permute(0, 3, 1, 2)[:, :3], list(self.sizes))


class _Slot:
    def __init__(self, device):
        self.workspace = K.TrainInputWorkspace(device)
        self.jitter = K.ColorJitterWorkspace(device)     # job table and scratch of the batch's jittered crop windows
        self.storage = None          # flat fp32 storage of the batch buffer, grown on demand
        self.released = None         # recorded on the consumer's stream once the step that read this slot has been queued
        self.images = None           # the uploaded sources of the batch in flight


class TrainInputLoader:
    """Infinite iterator of `batched_inputs` (see the module docstring).  `sync=True` prepares each batch on the calling stream and
    waits for it (one buffer would do): the plain order the pipelined one must reproduce."""

    def __init__(self, dataset_dicts, mapper, batch_size, sampler, size_divisibility, aspect_ratio_grouping=True, device="cuda",
                 sync=False, num_buffers=2):
        assert len(dataset_dicts) > 0 and batch_size > 0
        self.dataset_dicts, self.mapper, self.batch_size, self.sampler = dataset_dicts, mapper, int(batch_size), sampler
        self.size_divisibility, self.grouping, self.sync = int(size_divisibility), bool(aspect_ratio_grouping), bool(sync)
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_buffers = int(num_buffers)
        assert self.num_buffers >= 2

    def index_batches(self):
        """The batches as lists of dataset indices (host only): sampler, then grouping by the dicts' own width / height."""
        def row(i):
            d = self.dataset_dicts[i]
            if "width" in d and "height" in d:
                return {"index": i, "width": d["width"], "height": d["height"]}
            return {"index": i, "width": int(d["raw"].shape[1]), "height": int(d["raw"].shape[0])}

        rows = (row(i) for i in self.sampler)
        batches = AspectRatioGrouper(rows, self.batch_size) if self.grouping else _plain_batches(rows, self.batch_size)
        for b in batches:
            yield [r["index"] for r in b]

    def _draw(self, indices):
        """The host half of a batch: per item (mapped dict, source image(s), params)."""
        return [self.mapper.draw(self.dataset_dicts[i]) for i in indices]

    def _fill(self, drawn, buf, slot):
        """Upload the sources of a batch and queue its kernel call on the current stream."""
        slot.images = [raw.to(self.device, non_blocking=True) for _, raw, _ in drawn]
        images, jobs = list(slot.images), [p.job() for _, _, p in drawn]
        jit = [i for i, (_, _, p) in enumerate(drawn) if p.jitter is not None]
        if jit:      # their jittered crop windows become the images the resize reads
            crops = K.color_jitter_tiles_u8([jitter_item(plain_tiles(images[i]), drawn[i][2].crop, drawn[i][2]) for i in jit],
                                            workspace=slot.jitter)
            for i, crop in zip(jit, crops):
                images[i], jobs[i] = crop, drawn[i][2].crop_job()
        if _lsj_batch(drawn):      # every item through the large-scale jitter: the window of its scaled image on its canvas
            items = [p.lsj_item(plain_tiles(img), job[0:4]) for img, job, (_, _, p) in zip(images, jobs, drawn)]
            K.train_input_lsj_u8(items, buf, self.mapper.pixel_mean, self.mapper.pixel_std, resample_coeffs, workspace=slot.workspace)
            return
        K.train_input_u8(images, jobs, buf, self.mapper.pixel_mean, self.mapper.pixel_std, resample_coeffs, workspace=slot.workspace)

    def _items(self, drawn, indices, batch):
        return [dict(d, prepared=batch, index=i, slot=s, train_input_params=p) for s, ((d, _, p), i) in enumerate(zip(drawn, indices))]

    def _prepare(self, indices, slot, stream):
        drawn = self._draw(indices)
        sizes = [p.new_size for _, _, p in drawn]
        Hp, Wp = ImageList.padded_size(sizes, self.size_divisibility)
        B = len(drawn)
        with torch.cuda.stream(stream):
            if slot.released is not None:
                stream.wait_event(slot.released)
            n = B * Hp * Wp * 4
            if slot.storage is None or slot.storage.numel() < n:
                slot.storage = torch.empty(n * 5 // 4, dtype=torch.float32, device=self.device)
            buf = slot.storage[:n].view(B, Hp, Wp, 4)
            self._fill(drawn, buf, slot)
            ready = torch.cuda.Event()
            ready.record(stream)
        return self._items(drawn, indices, PreparedBatch(buf, sizes, ready))

    def __iter__(self):
        batches = self.index_batches()
        if self.sync:
            slot = _Slot(self.device)
            for indices in batches:
                out = self._prepare(indices, slot, torch.cuda.current_stream(self.device))
                out[0]["prepared"].ready.synchronize()
                yield out
            return
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))      # device-resident sources the caller has just produced
        slots = [_Slot(self.device) for _ in range(self.num_buffers)]
        k = 0
        pending = self._prepare(next(batches), slots[0], side)
        while True:
            current, cur_slot = pending, slots[k % self.num_buffers]
            k += 1
            nxt = slots[k % self.num_buffers]
            # whoever read `nxt` (the batch handed out num_buffers - 1 requests ago) has queued its step: `released` is set
            pending = self._prepare(next(batches), nxt, side)
            yield current
            # the consumer is back for the next batch: everything that reads `cur_slot` is on its stream already
            cur_slot.released = torch.cuda.Event()
            cur_slot.released.record(torch.cuda.current_stream(self.device))


class MosaicTrainInputLoader(TrainInputLoader):
    """TrainInputLoader whose items are MapDatasetMosaic's: a batch entry is a list of dataset indices, [i] for a plain item (through
    `mapper`), [i, ...] of 4 or 9 for a mosaic (through `mosaic_mapper`).  The mosaic draws happen in sampler order, before the
    grouping, which buckets a mosaic by its LAST tile's width / height (what the reference's AspectRatioGroupedDataset sees in the
    mapped dict).  Items carry "tile_indices" next to "index" (the sampled one)."""

    def __init__(self, dataset_dicts, mapper, mosaic_mapper, map_dataset, *args, **kwargs):
        super().__init__(dataset_dicts, mapper, *args, **kwargs)
        self.mosaic_mapper, self.map_dataset = mosaic_mapper, map_dataset

    def index_batches(self):
        def row(i):
            idxs = self.map_dataset.draw_indices(i)
            d = self.dataset_dicts[idxs[-1]]
            if "width" in d and "height" in d:
                return {"index": idxs, "width": d["width"], "height": d["height"]}
            return {"index": idxs, "width": int(d["raw"].shape[1]), "height": int(d["raw"].shape[0])}

        rows = (row(i) for i in self.sampler)
        batches = AspectRatioGrouper(rows, self.batch_size) if self.grouping else _plain_batches(rows, self.batch_size)
        for b in batches:
            yield [r["index"] for r in b]

    def _draw(self, indices):
        out = []
        for idxs in indices:
            if len(idxs) == 1:
                d, raw, p = self.mapper.draw(self.dataset_dicts[idxs[0]])
                out.append((d, [raw], p))
            else:
                out.append(self.mosaic_mapper.draw([self.dataset_dicts[i] for i in idxs]))
        return out

    def _fill(self, drawn, buf, slot):
        from .mosaic import plain_tiles_item

        slot.images = [[r.to(self.device, non_blocking=True) for r in raws] for _, raws, _ in drawn]
        items = [p.tiles_item(tiles) if len(tiles) > 1 else plain_tiles_item(tiles[0], p) for tiles, (_, _, p) in zip(slot.images, drawn)]
        jit = [i for i, (_, _, p) in enumerate(drawn) if p.jitter is not None]
        if _lsj_batch(drawn):      # plain and mosaic items, jittered or not, in one call of the large-scale jitter's entry
            lsj = [p.lsj_item(it[0], it[1]) for it, (_, _, p) in zip(items, drawn)]
            if jit:
                crops = K.color_jitter_tiles_u8([jitter_item(items[i][0], items[i][1], drawn[i][2]) for i in jit], workspace=slot.jitter)
                for i, crop in zip(jit, crops):
                    lsj[i] = drawn[i][2].lsj_item(plain_tiles(crop), drawn[i][2].crop_job()[0:4])
            K.train_input_lsj_u8(lsj, buf, self.mapper.pixel_mean, self.mapper.pixel_std, resample_coeffs, workspace=slot.workspace)
            return
        if jit:      # their jittered crop windows (of the painted canvas, 114 fill included) become plain one-tile items
            crops = K.color_jitter_tiles_u8([jitter_item(items[i][0], items[i][1], drawn[i][2]) for i in jit], workspace=slot.jitter)
            if len(jit) == len(items):      # every item is a plain image now: the plain entry
                K.train_input_u8(crops, [p.crop_job() for _, _, p in drawn], buf, self.mapper.pixel_mean, self.mapper.pixel_std,
                                 resample_coeffs, workspace=slot.workspace)
                return
            for i, crop in zip(jit, crops):
                job = drawn[i][2].crop_job()
                items[i] = (plain_tiles(crop), job[0:4], job[4], job[5], job[6])
        K.train_input_tiles_u8(items, buf, self.mapper.pixel_mean, self.mapper.pixel_std, resample_coeffs, workspace=slot.workspace)

    def _items(self, drawn, indices, batch):
        return [dict(d, prepared=batch, index=idxs[0], tile_indices=list(idxs), slot=s, train_input_params=p)
                for s, ((d, _, p), idxs) in enumerate(zip(drawn, indices))]


def _loader_args(cfg, size_divisibility):
    name = cfg.DATALOADER.SAMPLER_TRAIN
    if name != "TrainingSampler":
        raise NotImplementedError("DATALOADER.SAMPLER_TRAIN = {} is not implemented (TrainingSampler only)".format(name))
    world = dist.get_world_size()
    total = int(cfg.SOLVER.IMS_PER_BATCH)
    assert total > 0 and total % world == 0, "Total batch size ({}) must be divisible by the number of gpus ({}).".format(total, world)
    if size_divisibility is None:
        size_divisibility = 32 if "fpn" in cfg.MODEL.BACKBONE.NAME.lower() else 0
    return total // world, size_divisibility


def build_detection_train_mosaic_loader(cfg, dataset_dicts, mapper=None, seed=None, size_divisibility=None, sync=False, *,
                                        color_jitter=None, lsj=None):
    """build_detection_train_loader for INPUT.MOSAIC > 0 (reference lvc/data/build.py build_detection_train_mosaic_loader): each
    sampled item is, by MapDatasetMosaic's draws from Python's `random` module (seed it with `random.seed`), a plain item or a
    mosaic of 4 / 9 dataset items.  mapper: the plain branch's (default: a DatasetMapper of this cfg); the mosaic branch is
    DatasetMapperMosaic.from_config(cfg).  With INPUT.MOSAIC == 0 this is the plain loader.  Everything else as
    build_detection_train_loader (color_jitter and lsj go to both mappers)."""
    from .dataset_mapper import MOSAIC_KEYS
    from .mosaic import DatasetMapperMosaic, MapDatasetMosaic

    check_supported(cfg, allow=jitter_allow(MOSAIC_KEYS, color_jitter, lsj))
    batch_size, size_divisibility = _loader_args(cfg, size_divisibility)
    if mapper is None:
        mapper = DatasetMapper._from_config(cfg, True, allow=MOSAIC_KEYS, color_jitter=color_jitter, lsj=lsj)
    mosaic_mapper = DatasetMapperMosaic.from_config(cfg, True, color_jitter=color_jitter, lsj=lsj)
    sampler = TrainingSampler(len(dataset_dicts), seed=seed)
    loader = MosaicTrainInputLoader(dataset_dicts, mapper, mosaic_mapper, MapDatasetMosaic(dataset_dicts, mosaic_mapper, mapper, cfg),
                                    batch_size, sampler, size_divisibility, aspect_ratio_grouping=cfg.DATALOADER.ASPECT_RATIO_GROUPING,
                                    device=cfg.MODEL.DEVICE, sync=sync)
    return iter(loader)


def build_detection_train_loader(cfg, dataset_dicts, mapper=None, seed=None, size_divisibility=None, sync=False, *, color_jitter=None,
                                 lsj=None):
    """An infinite iterator of batches of SOLVER.IMS_PER_BATCH // world_size items for `model(batched_inputs)` in training mode.
    dataset_dicts: the reference's dataset format with the decoded image under "raw" (uint8 [H,W,3], pinned host memory makes the
    upload asynchronous).  seed: the sampler's (the same on every rank); the augmentations draw from numpy's global generator.
    size_divisibility: the backbone's (default: 32 for the FPN backbones, else 0).  color_jitter: None -- a cfg that sets
    INPUT.COLOR_JITTER is refused; True -- follow the key; a transforms.ColorJitter -- use it (its draws come from torch's default
    generator: `torch.manual_seed`).  lsj: None -- a cfg that sets INPUT.LSJ is refused; True -- follow the key (the reference's
    ResizeScale(0.5, 1.6, 800, 800) + FixedSizeCrop((800, 800)): every batch is 800 x 800); a transforms.LargeScaleJitter -- use it."""
    check_supported(cfg, jitter_allow((), color_jitter, lsj))
    batch_size, size_divisibility = _loader_args(cfg, size_divisibility)
    if mapper is None:
        mapper = DatasetMapper.from_config(cfg, True, color_jitter=color_jitter, lsj=lsj)
    sampler = TrainingSampler(len(dataset_dicts), seed=seed)
    loader = TrainInputLoader(dataset_dicts, mapper, batch_size, sampler, size_divisibility,
                              aspect_ratio_grouping=cfg.DATALOADER.ASPECT_RATIO_GROUPING, device=cfg.MODEL.DEVICE, sync=sync)
    return iter(loader)
