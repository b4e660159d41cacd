"""Test-time augmentation: `DatasetMapperTTA` / `GeneralizedRCNNWithTTA` (reference detectron2/modeling/test_time_augmentation.py:
27-291) on the device path.

The reference, per input image: builds every ResizeShortestEdge(min_size, TEST.AUG.MAX_SIZE) of the uint8 image (Pillow) and, with
TEST.AUG.FLIP, its horizontal mirror -- order [s0, s0-flip, s1, s1-flip, ...] --; runs them through `model.inference(...,
do_postprocess=False)` in consecutive groups of `batch_size`, each group padded to its own largest size; maps every augmentation's
boxes back with `tfm.inverse().apply_box` in fp32 numpy; and merges the union with `fast_rcnn_inference_single_image` (one-hot scores,
finite filter, clip to (height, width), score > 1e-8, per-class NMS at ROI_HEADS.NMS_THRESH_TEST, the first
TEST.DETECTIONS_PER_IMAGE).  About 43 s per 240x320 image at the default TEST.AUG on CPU.

Here, with the default mapper: one upload per image; two launches build every augmentation straight into the normalised, padded
NHWC4 group buffers (csrc/tta.hip lvc_tta_resize_u8: Pillow-exact, mirrored slots written by the same pass); the groups -- the
reference's grouping, so the padding and hence the border features are the same -- run through the detector's device fast path
(GeneralizedRCNN.inference_nhwc); one launch sequence merges all images of the call (lvc_tta_merge: union, inverse transforms in the
reference's fp32 roundings, filters, batched NMS); one device->host read per call.  A custom `tta_mapper` goes through the general
path: its images through the model's own preprocessing, its `transforms` (TransformLists of resize / hflip / no-op) for the inverse,
the same merge.

Differences from the reference, on purpose: the reference's mapper draws its (single-valued) sizes from numpy's global RNG; this one
draws nothing.  Float images raise NotImplementedError (the reference resizes them with F.interpolate, not built here).
"""
import collections
import copy

import numpy as np
import torch
from torch import nn
from torch.nn.parallel import DistributedDataParallel

from .. import kernels as K
from ..data.transforms import HFlipTransform, NoOpTransform, ResizeShortestEdge, ResizeTransform, TransformList, resample_coeffs
from ..structures import ImageList
from .meta_arch import GeneralizedRCNN, GeneralizedRCNNRegOnly
from .proposal_generator import RPN
from .roi_heads import CascadeROIHeads, StandardROIHeads
from .roi_heads.roi_heads import instances_from_batched, run_with_fallbacks

__all__ = ["DatasetMapperTTA", "GeneralizedRCNNWithTTA"]


def _source(inp):
    """(device-agnostic tensor, H, W, element strides (sy, sx, sc)) of an input dict's uint8 image: CHW `image` or HWC `raw`."""
    if "image" in inp:
        img = inp["image"]
        if img.dtype != torch.uint8:
            raise NotImplementedError("test-time augmentation of float images: the reference resizes them with F.interpolate "
                                      "(ResizeTransform.apply_image), which is not built here; pass uint8 images")
        return img, int(img.shape[1]), int(img.shape[2]), (1, 2, 0)
    img = inp["raw"]
    if img.dtype != torch.uint8:
        raise NotImplementedError("test-time augmentation of float images is not built here; pass uint8 images")
    return img, int(img.shape[0]), int(img.shape[1]), (0, 1, 2)


class _Plan:
    """The augmentations of one H x W image (DatasetMapperTTA.__call__): sizes[j] = ResizeShortestEdge(min_sizes[j], max_size)
    output; augs = [(j, flipped)] in the reference's order."""

    def __init__(self, H, W, height, width, min_sizes, max_size, flip):
        self.H, self.W, self.height, self.width = H, W, int(height), int(width)
        self.sizes = []
        for s in min_sizes:
            if int(s) == 0:
                raise NotImplementedError("TEST.AUG.MIN_SIZES contains 0 (a no-op resize): not supported")
            self.sizes.append(ResizeShortestEdge(int(s), max_size).output_size(H, W, int(s)))
        self.augs = []
        for j in range(len(self.sizes)):
            self.augs.append((j, False))
            if flip:
                self.augs.append((j, True))

    def transforms(self, k):
        """The reference's `transforms` of augmentation k: TransformList([pre_tfm,] ResizeTransform[, HFlipTransform])."""
        j, flipped = self.augs[k]
        nh, nw = self.sizes[j]
        pre = NoOpTransform() if (self.H, self.W) == (self.height, self.width) else \
            ResizeTransform(self.height, self.width, self.H, self.W)
        tl = [pre, ResizeTransform(self.H, self.W, nh, nw)]
        if flipped:
            tl.append(HFlipTransform(nw))
        return TransformList(tl)

    def launch(self, img, strides, dev, slots=None, u8=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
        """Every augmentation in two launches: slots[k] / u8[k] the NHWC4 slot / uint8 [nh,nw,3] output of augmentation k (None:
        not written).  img: the device image; strides: its (sy, sx, sc)."""
        slots = slots or [None] * len(self.augs)
        u8 = u8 or [None] * len(self.augs)
        hjobs, hidx, keep = [], {}, []
        for nh, nw in self.sizes:
            if nw != self.W and nw not in hidx:
                xb, xk, ks = resample_coeffs(self.W, nw, dev)
                tmp = torch.empty(self.H * nw * 3, dtype=torch.uint8, device=dev)
                hidx[nw] = len(hjobs)
                hjobs.append((xb, xk, ks, nw, tmp))
        vjobs = []
        for j, (nh, nw) in enumerate(self.sizes):
            out = {}
            for k, (jj, fl) in enumerate(self.augs):
                if jj == j:
                    out[fl] = (slots[k], u8[k])
            if all(a is None and b is None for a, b in out.values()):
                continue
            yb = yk = None
            ks = 0
            if nh != self.H:
                yb, yk, ks = resample_coeffs(self.H, nh, dev)
                keep.append((yb, yk))
            plain, mirr = out.get(False, (None, None)), out.get(True, (None, None))
            vjobs.append((hidx.get(nw, -1), yb, yk, ks, nh, nw, plain[1], mirr[1], plain[0], mirr[0]))
        K.tta_resize_u8(img, self.H, self.W, strides, hjobs, vjobs, mean, std)
        return hjobs, keep     # scratch and tables: alive until the launches are queued (the allocator orders reuse on the stream)


class DatasetMapperTTA:
    """Reference test_time_augmentation.py:27-81: a dataset dict (uint8 CHW `image`, `height`, `width`) -> one dict per augmentation
    with `image` (the augmented uint8 image, CHW, on the device: csrc/tta.hip, Pillow-exact) and `transforms` (TransformList:
    [pre_tfm,] ResizeTransform[, HFlipTransform]).  Deterministic: the sizes are computed, not drawn from numpy's global RNG as the
    reference does (its draws are single-valued)."""

    def __init__(self, cfg):
        self.min_sizes = tuple(int(s) for s in cfg.TEST.AUG.MIN_SIZES)
        self.max_size = cfg.TEST.AUG.MAX_SIZE
        self.flip = bool(cfg.TEST.AUG.FLIP)
        self.image_format = cfg.INPUT.FORMAT
        self.device = torch.device(cfg.MODEL.DEVICE)

    def plan(self, dataset_dict):
        _, H, W, _ = _source(dataset_dict)
        return _Plan(H, W, dataset_dict.get("height", H), dataset_dict.get("width", W), self.min_sizes, self.max_size, self.flip)

    def __call__(self, dataset_dict):
        img, H, W, order = _source(dataset_dict)
        plan = self.plan(dataset_dict)
        dev = self.device
        img = img.to(dev, non_blocking=True)
        u8 = [torch.empty(plan.sizes[j][0], plan.sizes[j][1], 3, dtype=torch.uint8, device=dev) for j, _ in plan.augs]
        plan.launch(img, tuple(img.stride(d) for d in order), dev, u8=u8)
        ret = []
        for k, im in enumerate(u8):
            dic = copy.deepcopy({key: v for key, v in dataset_dict.items() if key not in ("image", "raw")})
            dic["transforms"] = plan.transforms(k)
            dic["image"] = im.permute(2, 0, 1)
            ret.append(dic)
        return ret


def _inverse_steps(tfm):
    """lvc_tta_merge's row for one augmentation: tfm.inverse() as (kind, a, b) steps -- 1: hflip (width), 2: resize (fp32 x / y
    factors, as numpy multiplies an fp32 array by the Python float new_w * 1.0 / w)."""
    inv = tfm.inverse()
    steps = []
    for t in (inv.transforms if hasattr(inv, "transforms") else [inv]):
        name = type(t).__name__
        if name == "NoOpTransform":
            continue
        if name == "HFlipTransform":
            steps.append((1.0, float(t.width), 0.0))
        elif name == "ResizeTransform":
            steps.append((2.0, float(np.float32(t.new_w * 1.0 / t.w)), float(np.float32(t.new_h * 1.0 / t.h))))
        else:
            raise NotImplementedError("test-time augmentation: the inverse of %s is not built on the device (resize, hflip and "
                                      "no-op transforms are)" % name)
    if len(steps) > K.TTA_MAX_STEPS:
        raise NotImplementedError("more than %d resize / flip steps in one augmentation's transforms" % K.TTA_MAX_STEPS)
    row = [float(len(steps))]
    for s in steps:
        row.extend(s)
    return row + [0.0] * (K.TTA_PARAM_STRIDE - len(row))


class GeneralizedRCNNWithTTA(nn.Module):
    """Reference test_time_augmentation.py:84-291 for lvc_amd's GeneralizedRCNN (RPN + StandardROIHeads, box-only).  `__call__`
    has GeneralizedRCNN.forward's format: list of dicts (`image` uint8 CHW or `raw` uint8 HWC, optional `height` / `width`) ->
    list of {"instances": Instances(image_size=(height, width))}."""

    def __init__(self, cfg, model, tta_mapper=None, batch_size=3):
        super().__init__()
        if isinstance(model, DistributedDataParallel):
            model = model.module
        assert isinstance(model, GeneralizedRCNN) and not isinstance(model, GeneralizedRCNNRegOnly), \
            "TTA is only supported on GeneralizedRCNN. Got a model of type {}".format(type(model))
        self.cfg = cfg.clone()
        assert not self.cfg.MODEL.KEYPOINT_ON, "TTA for keypoint is not supported yet"
        assert not self.cfg.MODEL.LOAD_PROPOSALS, "TTA for pre-computed proposals is not supported yet"
        if (not isinstance(model.proposal_generator, RPN) or not isinstance(model.roi_heads, StandardROIHeads)
                or isinstance(model.roi_heads, CascadeROIHeads) or getattr(model, "output_layer", None) == "BoxOnlyLayersCascade"):
            raise NotImplementedError("TTA runs on the RPN + StandardROIHeads detector (the reference's box branch)")
        assert int(batch_size) >= 1
        self.model = model
        self.default_mapper = tta_mapper is None
        self.tta_mapper = DatasetMapperTTA(cfg) if tta_mapper is None else tta_mapper
        self.batch_size = int(batch_size)
        self._tables = collections.OrderedDict()

    @property
    def device(self):
        return self.model.device

    @property
    def roi_heads(self):
        return self.model.roi_heads

    def forward(self, batched_inputs):
        return self.inference(batched_inputs)

    def inference(self, batched_inputs, do_postprocess=True):
        """The merged detections are in (height, width) coordinates whatever `do_postprocess` says (the reference's TTA output);
        the whole call is repeated if a limit the reference does not have is hit (roi_heads.run_with_fallbacks)."""
        assert not self.model.training
        if not batched_inputs:
            return []

        def once():
            ob, osc, ocl, cnt, status = self.inference_batched(batched_inputs, do_postprocess)
            insts = instances_from_batched(ob, osc, ocl, cnt, [self._out_size(x) for x in batched_inputs], status)   # the one read
            return [{"instances": r} for r in insts]

        return run_with_fallbacks(self.model, once)

    @staticmethod
    def _out_size(inp):
        _, H, W, _ = _source(inp)
        return int(inp.get("height", H)), int(inp.get("width", W))

    def _table(self, rows, dtype):
        """A small per-call table on the device, cached by value (bounded); a miss is one pinned, non-blocking upload."""
        key = (dtype, tuple(tuple(r) for r in rows))
        t = self._tables.get(key)
        if t is None:
            t = torch.tensor(rows, dtype=dtype).pin_memory().to(self.device, non_blocking=True)
            self._tables[key] = t
            while len(self._tables) > 256:
                self._tables.popitem(last=False)
        else:
            self._tables.move_to_end(key)
        return t

    def inference_batched(self, batched_inputs, do_postprocess=True):
        """Every input's augmentations, their groups through the detector, the merge: device-resident (boxes [B,topk,4], scores,
        classes int32, count [B] int32, status [1] int32), no host read -- what evaluation.PipelinedInference launches."""
        dev = self.device
        status = K.new_status(dev)
        outs, params, tab = [], [], []
        with torch.no_grad():
            for inp in batched_inputs:
                first = sum(o[0].shape[0] for o in outs)
                if self.default_mapper:
                    rows = self._fused(inp, status, outs)
                else:
                    rows = self._general(inp, status, outs)
                params.extend(rows)
                h, w = self._out_size(inp)
                tab.append([first, first + len(rows), h, w])
            T = outs[0][0].shape[1]
            ob = torch.cat([o[0] for o in outs]) if len(outs) > 1 else outs[0][0]
            osc = torch.cat([o[1] for o in outs]) if len(outs) > 1 else outs[0][1]
            ocl = torch.cat([o[2] for o in outs]) if len(outs) > 1 else outs[0][2]
            cnt = torch.cat([o[3] for o in outs]) if len(outs) > 1 else outs[0][3]
            nmax = max(t[1] - t[0] for t in tab) * T
            det = int(self.cfg.TEST.DETECTIONS_PER_IMAGE)
            topk = nmax if det < 0 else det
            mb, ms, mc, mn = K.tta_merge(ob, osc, ocl, cnt, self._table(params, torch.float32), self._table(tab, torch.int32),
                                         len(batched_inputs), nmax, 1e-8, float(self.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST), topk)
        return mb, ms, mc, mn, status

    def _fused(self, inp, status, outs):
        """Default mapper: the image once to the device, every augmentation written into its group's buffer by two launches, the
        groups through GeneralizedRCNN.inference_nhwc.  Returns the merge rows of the augmentations."""
        model, dev = self.model, self.device
        img, H, W, order = _source(inp)
        m = self.tta_mapper
        plan = _Plan(H, W, inp.get("height", H), inp.get("width", W), m.min_sizes, m.max_size, m.flip)
        img = img.to(dev, non_blocking=True)
        groups, slots = [], []
        n = len(plan.augs)
        for g0 in range(0, n, self.batch_size):
            sizes = [plan.sizes[j] for j, _ in plan.augs[g0:g0 + self.batch_size]]
            Hp, Wp = ImageList.padded_size(sizes, model.backbone.size_divisibility)
            buf = torch.empty(len(sizes), Hp, Wp, 4, device=dev, dtype=torch.float32)
            groups.append((buf, sizes))
            slots.extend(buf[i] for i in range(len(sizes)))
        plan.launch(img, tuple(img.stride(d) for d in order), dev, slots=slots, mean=model.pixel_mean, std=model.pixel_std)
        for buf, sizes in groups:
            ob, osc, ocl, cnt, _ = model.inference_nhwc(buf, sizes, None, status)
            outs.append((ob, osc, ocl, cnt))
        return [_inverse_steps(plan.transforms(k)) for k in range(n)]

    def _general(self, inp, status, outs):
        """Custom mapper: its augmented dicts through the model's own preprocessing in groups of batch_size, its transforms for the
        inverse."""
        aug_inputs = self.tta_mapper(inp)
        tfms = [x.pop("transforms") for x in aug_inputs]
        for g0 in range(0, len(aug_inputs), self.batch_size):
            ob, osc, ocl, cnt, _ = self.model.inference_batched(aug_inputs[g0:g0 + self.batch_size], do_postprocess=False, status=status)
            outs.append((ob, osc, ocl, cnt))
        return [_inverse_steps(t) for t in tfms]
