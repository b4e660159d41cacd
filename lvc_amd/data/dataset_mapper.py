"""DatasetMapper for training (reference lvc/data/dataset_mapper.py:24-209 `DatasetMapperIgnore`), with the pixels on the device.

The reference's mapper reads a file, crops / resizes (Pillow) / flips the image on a CPU worker and transforms the annotations.
Here the mapper is split along the line between policy and pixels:

  * `draw(dataset_dict)` is the host half: it draws the augmentations (numpy's global generator, the reference's calls in the
    reference's order) and maps the annotations through them -- a few dozen float64 numbers per image, rounded to fp32 exactly where
    the reference rounds them (`mapped_instances`);
  * the pixels of a whole batch are produced by ONE kernel call (`kernels.train_input_u8`, csrc/train_input.hip), which the loader
    (build.py) issues for the batch; `__call__` issues it for a single image and returns the reference's dict (`"image"`: uint8 CHW).

The image comes from `"raw"`: a uint8 [H,W,3] tensor or array, on any device, already in INPUT.FORMAT channel order.  Decoding
files is the caller's business, as in `eval_loop_host_inputs`.

Built: INPUT.CROP (all four types), MIN_SIZE_TRAIN / MAX_SIZE_TRAIN / MIN_SIZE_TRAIN_SAMPLING, the horizontal flip, boxes, classes,
ignore flags, ids; INPUT.COLOR_JITTER (transforms.ColorJitter; pixels: `kernels.color_jitter_tiles_u8`, csrc/color_jitter.hip, on the
crop window in front of the resize) for callers that opt in with `color_jitter=True` -- without it the key still raises, as it
always has; INPUT.LSJ (transforms.LargeScaleJitter: ResizeScale -> FixedSizeCrop in ResizeShortestEdge's place; pixels:
`kernels.train_input_lsj_u8`, which computes only the window of the scaled image that survives) for callers that opt in with
`lsj=True`, the same way; INPUT.MOSAIC / INPUT.MOSAIC49SPLIT through entry points of their own, as in the reference (mosaic.py:
`DatasetMapperMosaic`, `MapDatasetMosaic`, build.py `build_detection_train_mosaic_loader`) -- `DatasetMapper.from_config` and
`build_detection_train_loader` never do mosaic and refuse a cfg that asks for it, pointing there.  Not built (NotImplementedError
naming the key): INPUT.BLUR (torchvision's GaussianBlur: an fp32 convolution whose summation order cannot be pinned), MODEL.MASK_ON, MODEL.KEYPOINT_ON, MODEL.LOAD_PROPOSALS,
QUERY_EXPAND.GET_CROPS; "sem_seg_file_name" in an input dict.
"""
import numpy as np
import torch

from .. import kernels as K
from ..structures import Boxes, BoxMode, Instances
from .transforms import (AugmentationList, ColorJitter, LargeScaleJitter, RandomCrop, RandomFlip, ResizeShortestEdge,
                         resample_coeffs)


def _unsupported(cfg):
    """Keys of the training input that are not built: (name, is it switched on)."""
    I = cfg.INPUT
    return [("INPUT.COLOR_JITTER", bool(I.COLOR_JITTER)), ("INPUT.BLUR", bool(I.BLUR)), ("INPUT.LSJ", bool(I.LSJ)),
            ("INPUT.MOSAIC", float(I.MOSAIC) > 0), ("INPUT.MOSAIC49SPLIT", float(I.MOSAIC49SPLIT) > 0),
            ("MODEL.MASK_ON", bool(cfg.MODEL.MASK_ON)), ("MODEL.KEYPOINT_ON", bool(cfg.MODEL.KEYPOINT_ON)),
            ("MODEL.LOAD_PROPOSALS", bool(cfg.MODEL.LOAD_PROPOSALS)), ("QUERY_EXPAND.GET_CROPS", bool(cfg.QUERY_EXPAND.GET_CROPS))]


MOSAIC_KEYS = ("INPUT.MOSAIC", "INPUT.MOSAIC49SPLIT")     # built, but only by the mosaic entry points (mosaic.py)
JITTER_KEY = "INPUT.COLOR_JITTER"                          # built, but only for callers that pass color_jitter
LSJ_KEY = "INPUT.LSJ"                                      # built, but only for callers that pass lsj


def check_supported(cfg, allow=()):
    """allow: keys the caller handles itself (the mosaic entry points pass MOSAIC_KEYS)."""
    for key, on in _unsupported(cfg):
        if on and key not in allow:
            if key in MOSAIC_KEYS:
                raise NotImplementedError("{} is not implemented by this entry point (crop, resize, flip only): mosaic batches come "
                                          "from build_detection_train_mosaic_loader / DatasetMapperMosaic".format(key))
            if key == JITTER_KEY:
                raise NotImplementedError("{} is not applied by default: pass `color_jitter=True` to the loader builder or to the "
                                          "mapper's from_config to get the device colour jitter".format(key))
            if key == LSJ_KEY:
                raise NotImplementedError("{} is not applied by default: pass `lsj=True` to the loader builder or to the mapper's "
                                          "from_config to get the device large-scale jitter".format(key))
            raise NotImplementedError("{} is not implemented by the device training input (crop, colour jitter, resize, large-scale "
                                      "jitter, flip, mosaic only)".format(key))


def jitter_allow(allow, color_jitter, lsj=None):
    """The keys a caller handles, with INPUT.COLOR_JITTER / INPUT.LSJ among them once it has opted in."""
    return (tuple(allow) + ((JITTER_KEY,) if color_jitter is not None and color_jitter is not False else ()) +
            ((LSJ_KEY,) if lsj is not None and lsj is not False else ()))


def build_augmentation(cfg, is_train=True, allow=(), color_jitter=None, lsj=None):
    """detection_utils.build_augmentation (:563-598) with the crop of DatasetMapperIgnore.from_config (:92-99) in front.
    color_jitter: None -- a cfg that sets INPUT.COLOR_JITTER raises; True -- follow the key (ColorJitter() in front of the resize if
    it is set, as the reference's list has it, none if not); a transforms.ColorJitter -- use it whatever the key says.
    lsj: None -- a cfg that sets INPUT.LSJ raises; True -- follow the key (ResizeScale(0.5, 1.6, 800, 800) and FixedSizeCrop((800,
    800)) in ResizeShortestEdge's place if it is set, as the reference's list has it); a transforms.LargeScaleJitter -- use its two
    policies whatever the key says.  INPUT.BLUR raises whatever is passed: it is torchvision's GaussianBlur, an fp32 convolution
    whose summation order cannot be pinned to bytes."""
    check_supported(cfg, jitter_allow(allow, color_jitter, lsj))
    if not (color_jitter is None or color_jitter is True or color_jitter is False or isinstance(color_jitter, ColorJitter)):
        raise TypeError("color_jitter is None, True or a ColorJitter, got {!r}".format(color_jitter))
    if not (lsj is None or lsj is True or lsj is False or isinstance(lsj, LargeScaleJitter)):
        raise TypeError("lsj is None, True or a LargeScaleJitter, got {!r}".format(lsj))
    if is_train and lsj is True and cfg.INPUT.LSJ:
        lsj = LargeScaleJitter()
    if is_train and isinstance(lsj, LargeScaleJitter):
        augs = lsj.augmentations()
    else:
        augs = [ResizeShortestEdge.from_config(cfg, is_train)]
    if is_train and color_jitter is True and cfg.INPUT.COLOR_JITTER:
        color_jitter = ColorJitter()
    if is_train and isinstance(color_jitter, ColorJitter):
        augs.insert(0, color_jitter)
    if is_train:
        augs.append(RandomFlip())
        if cfg.INPUT.CROP.ENABLED:
            augs.insert(0, RandomCrop(cfg.INPUT.CROP.TYPE, cfg.INPUT.CROP.SIZE))
    return augs


def _xyxy(bbox, mode):
    """BoxMode.convert(bbox, mode, XYXY_ABS) of one annotation as the reference computes it (structures/boxes.py:43-129): a list is
    converted through `torch.tensor(list)` -- fp32 as soon as one entry is a float, int64 for ints -- added there, and turned back
    into a list.  The same roundings in numpy (a few microseconds per box; this runs for every annotation of every image)."""
    mode = BoxMode(int(mode))
    if mode == BoxMode.XYXY_ABS:
        return bbox
    if mode != BoxMode.XYWH_ABS:
        raise NotImplementedError("Conversion from BoxMode {} to XYXY_ABS is not supported".format(mode))
    if isinstance(bbox, (list, tuple)):
        assert len(bbox) == 4, "BoxMode.convert takes a 4-tuple/list or an Nx4 array"
        if all(isinstance(v, int) and not isinstance(v, bool) for v in bbox):
            return type(bbox)([bbox[0], bbox[1], bbox[2] + bbox[0], bbox[3] + bbox[1]])
        a = np.asarray(bbox, dtype=np.float32)
        a[2] += a[0]
        a[3] += a[1]
        return type(bbox)(a.tolist())
    arr = np.array(bbox).reshape(1, -1)
    arr[:, 2] += arr[:, 0]
    arr[:, 3] += arr[:, 1]
    return arr[0]


def _instances_ignore(boxes, annos, image_size):
    """lvc/data/detection_utils.py:16-49 annotations_to_instances_ignore: gt_boxes (the float64 boxes rounded to fp32 here),
    gt_classes, gt_ignores ("ignore_qe", default 0) and ids ("id", default -1) -- the last two are always set."""
    target = Instances(tuple(image_size))
    target.gt_boxes = Boxes(torch.from_numpy(np.asarray(boxes, dtype=np.float64).reshape(-1, 4).astype(np.float32)))
    target.gt_classes = torch.tensor([o["category_id"] for o in annos], dtype=torch.int64)
    target.gt_ignores = torch.tensor([o.get("ignore_qe", 0) for o in annos], dtype=torch.int64)
    target.ids = torch.tensor([o.get("id", -1) for o in annos], dtype=torch.int64)
    return target


def mapped_instances(annotations, transforms, image_size):
    """What the reference's mapper makes of an image's annotation list (dataset_mapper.py:181-208): crowd annotations dropped,
    transform_instance_annotations on each, annotations_to_instances_ignore, filter_empty_instances -- with the boxes of the image
    as ONE [N,4] float64 array: every step is elementwise per box, so the numbers are the per-annotation ones, and the caller's
    annotation dicts are not written to."""
    annos = [o for o in annotations if o.get("iscrowd", 0) == 0]
    boxes = np.array([_xyxy(o["bbox"], o["bbox_mode"]) for o in annos], dtype=np.float64).reshape(-1, 4)
    boxes = transforms.apply_box(boxes).clip(min=0)
    boxes = np.minimum(boxes, list(tuple(image_size) + tuple(image_size))[::-1])
    return filter_empty_instances(_instances_ignore(boxes, annos, image_size))


def filter_empty_instances(instances, box_threshold=1e-5):
    """detection_utils.filter_empty_instances (:452-479) by box."""
    return instances[instances.gt_boxes.nonempty(threshold=box_threshold)]


def _raw_of(dataset_dict):
    if "raw" not in dataset_dict:
        if "file_name" in dataset_dict:
            raise ValueError("this DatasetMapper does not decode files: the dict has \"file_name\" but no \"raw\"; decode the image "
                             "and pass it as \"raw\" (uint8 [H,W,3], INPUT.FORMAT channel order)")
        raise KeyError("dataset dict without \"raw\"")
    raw = dataset_dict["raw"]
    if isinstance(raw, np.ndarray):
        raw = torch.from_numpy(np.ascontiguousarray(raw))
    if raw.dtype != torch.uint8 or raw.dim() != 3 or raw.shape[2] != 3:
        raise ValueError("\"raw\" must be a uint8 [H,W,3] image, got {} {}".format(raw.dtype, tuple(raw.shape)))
    return raw


def plain_tiles(raw):
    """A plain image as the one tile that covers its canvas."""
    return [(raw, (0, 0, int(raw.shape[1]), int(raw.shape[0])), (0, 0))]


def jitter_item(tiles, window, params):
    """The job of kernels.color_jitter_tiles_u8 for an item whose params carry a jitter."""
    return (tiles, tuple(window), params.jitter[0], params.jitter[1])


class DatasetMapper:
    """See the module docstring.  `DatasetMapper.from_config(cfg, is_train=True)`; `mapper(dataset_dict)` -> the reference's dict."""

    def __init__(self, is_train, *, augmentations, image_format="BGR", pixel_mean=(0.0, 0.0, 0.0), pixel_std=(1.0, 1.0, 1.0),
                 device="cuda"):
        self.is_train = is_train
        self.augmentations = AugmentationList(augmentations)
        self.image_format = image_format
        self.pixel_mean, self.pixel_std = [float(v) for v in pixel_mean], [float(v) for v in pixel_std]
        self.device = torch.device(device)

    @classmethod
    def from_config(cls, cfg, is_train=True, *, color_jitter=None, lsj=None):
        return cls._from_config(cfg, is_train, color_jitter=color_jitter, lsj=lsj)

    @classmethod
    def _from_config(cls, cfg, is_train=True, allow=(), color_jitter=None, lsj=None):
        return cls(is_train, augmentations=build_augmentation(cfg, is_train, allow, color_jitter, lsj), image_format=cfg.INPUT.FORMAT,
                   pixel_mean=cfg.MODEL.PIXEL_MEAN, pixel_std=cfg.MODEL.PIXEL_STD, device=cfg.MODEL.DEVICE)

    def draw(self, dataset_dict):
        """The host half: (mapped dict without its image, raw image, TrainInputParams).  The dict carries "instances" when the input
        has "annotations"; every other key is kept."""
        raw = _raw_of(dataset_dict)
        d = {k: v for k, v in dataset_dict.items() if k != "raw"}      # nothing below writes into the caller's values
        if "sem_seg_file_name" in d:
            raise NotImplementedError("sem_seg_file_name: semantic segmentation is not implemented by the device training input")
        h, w = int(raw.shape[0]), int(raw.shape[1])
        if "width" in d and "height" in d and (d["width"], d["height"]) != (w, h):     # detection_utils.check_image_size
            raise ValueError("Mismatched image shape: got {}, expect {}".format((w, h), (d["width"], d["height"])))
        d.setdefault("width", w)
        d.setdefault("height", h)
        transforms, params = self.augmentations.draw(h, w)
        if "annotations" in d:
            d["instances"] = mapped_instances(d.pop("annotations"), transforms, params.new_size)
        return d, raw, params

    def __call__(self, dataset_dict):
        d, raw, params = self.draw(dataset_dict)
        raw = raw.to(self.device, non_blocking=True)
        nh, nw = params.new_size
        slot = torch.empty(1, nh, nw, 4, dtype=torch.float32, device=self.device)
        job = params.job()
        if params.jitter is not None:      # the jittered crop window is the image the resize reads
            raw, job = K.color_jitter_tiles_u8([jitter_item(plain_tiles(raw), params.crop, params)])[0], params.crop_job()
        if params.lsj is not None:
            item = params.lsj_item(plain_tiles(raw), job[0:4])
            u8 = K.train_input_lsj_u8([item], slot, self.pixel_mean, self.pixel_std, resample_coeffs, want_u8=True)[0]
        else:
            u8 = K.train_input_u8([raw], [job], slot, self.pixel_mean, self.pixel_std, resample_coeffs, want_u8=True)[0]
        d["image"] = u8.permute(2, 0, 1).contiguous()
        d["normalized"] = slot[0]       # [new_h,new_w,4] fp32: (image - mean) / std as the model's batch slot holds it
        return d


DatasetMapperIgnore = DatasetMapper
