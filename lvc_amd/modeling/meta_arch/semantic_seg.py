"""SemSegFPNHead / SemanticSegmentor (reference detectron2/modeling/meta_arch/semantic_seg.py), inference only.

The head's state_dict is the reference's (`p2.0.weight`, `p2.0.norm.weight`, `p4.2.*`, `predictor.*`: the `Sequential` slots of the
upsamples stay empty of parameters, so a reference checkpoint loads with strict=True).  Each block is the project's Conv2d with a
GroupNorm norm (conv -> GN -> ReLU on the existing routes); the bilinear x2 upsamples, the head's x`COMMON_STRIDE` upsample +
`sem_seg_postprocess` + argmax are csrc/sem_seg.hip:

  * the LAST upsample of a level adds into the running level sum (`upsample2_bilinear_nhwc(y, acc=x, out=x)`), so the reference's
    order ((p2 + p3') + p4') + p5' holds and no add pass runs;
  * the 1x1 predictor is packed with zero output channels up to a multiple of 64 (54 % 4 != 0 would send it to the generic fp32
    entry), and its consumer reads rows of `ld` floats of which the first NUM_CLASSES count;
  * the full-resolution [K, H, W] map of the reference's `forward` is never formed: `postprocess` goes from the stride-`COMMON_STRIDE`
    logits to the output-size soft logits and / or label map in one launch per batch.

Training (`loss_sem_seg`) is not built and refuses before anything touches a device.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from ... import kernels as K
from ...layers import Conv2d
from ...layers.batch_norm import GroupNorm
from ...utils import weight_init
from ...utils.registry import Registry
from ..backbone import build_backbone
from .build import META_ARCH_REGISTRY
from .rcnn import _RCNNBase

SEM_SEG_HEADS_REGISTRY = Registry("SEM_SEG_HEADS")
TRAIN_REFUSAL = "training the semantic branch (loss_sem_seg) is not built"
_PREDICTOR_PAD = 64


def build_sem_seg_head(cfg, input_shape):
    return SEM_SEG_HEADS_REGISTRY.get(cfg.MODEL.SEM_SEG_HEAD.NAME)(cfg, input_shape)


class Upsample2(nn.Module):
    """The parameter-free slot of nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False) in a scale head."""

    def forward_nhwc(self, x, acc=None):
        return K.upsample2_bilinear_nhwc(x, acc=acc, out=acc)

    def extra_repr(self):
        return "scale_factor=2.0, mode=bilinear"


@SEM_SEG_HEADS_REGISTRY.register()
class SemSegFPNHead(nn.Module):
    def __init__(self, cfg, input_shape):
        super().__init__()
        H = cfg.MODEL.SEM_SEG_HEAD
        self.in_features = list(H.IN_FEATURES)
        strides = {k: v.stride for k, v in input_shape.items()}
        channels = {k: v.channels for k, v in input_shape.items()}
        self.ignore_value = H.IGNORE_VALUE
        self.num_classes = int(H.NUM_CLASSES)
        conv_dims = int(H.CONVS_DIM)
        self.common_stride = int(H.COMMON_STRIDE)
        norm = H.NORM
        self.loss_weight = H.LOSS_WEIGHT
        if norm not in ("GN", ""):
            raise NotImplementedError("MODEL.SEM_SEG_HEAD.NORM = {!r}: the semantic head is built for 'GN' and ''".format(norm))
        if conv_dims <= 0 or conv_dims % 64:
            raise NotImplementedError("MODEL.SEM_SEG_HEAD.CONVS_DIM = {}: the head's conv and GroupNorm routes take multiples of 64"
                                      .format(conv_dims))
        if self.num_classes < 1 or self.num_classes > K.SEG_MAX_LABELS:
            raise NotImplementedError("MODEL.SEM_SEG_HEAD.NUM_CLASSES = {}: the postprocess kernel takes 1 .. {}"
                                      .format(self.num_classes, K.SEG_MAX_LABELS))
        self.scale_heads = []
        for i, f in enumerate(self.in_features):
            if i > 0 and strides[f] == self.common_stride:
                raise NotImplementedError("MODEL.SEM_SEG_HEAD.IN_FEATURES = {}: a level at COMMON_STRIDE after the first has no "
                                          "upsample to add it into the level sum".format(self.in_features))
            head_length = max(1, int(np.log2(strides[f]) - np.log2(self.common_stride)))
            ops = []
            for k in range(head_length):
                conv = Conv2d(channels[f] if k == 0 else conv_dims, conv_dims, kernel_size=3, stride=1, padding=1, bias=not norm,
                              norm=GroupNorm(32, conv_dims) if norm == "GN" else None, activation=F.relu)
                weight_init.c2_msra_fill(conv)
                ops.append(conv)
                if strides[f] != self.common_stride:
                    ops.append(Upsample2())
            self.scale_heads.append(nn.Sequential(*ops))
            self.add_module(f, self.scale_heads[-1])
        self.predictor = Conv2d(conv_dims, self.num_classes, kernel_size=1, stride=1, padding=0)
        weight_init.c2_msra_fill(self.predictor)
        self.__dict__["_predictor_cache"] = type(self.predictor._cache)()

    @property
    def logits_ld(self):
        """Floats per pixel of `forward_nhwc`'s output: NUM_CLASSES rounded up to the predictor's packed width."""
        return (self.num_classes + _PREDICTOR_PAD - 1) // _PREDICTOR_PAD * _PREDICTOR_PAD

    def packed_predictor(self):
        """The 1x1 predictor with zero output channels up to `logits_ld`, so that it takes a pointwise MFMA route."""
        conv = self.predictor

        def build():
            w, b = conv.weight.detach(), conv.bias.detach()
            pad = self.logits_ld - w.shape[0]
            if pad:
                w = torch.cat([w, w.new_zeros((pad,) + tuple(w.shape[1:]))], 0)
                b = torch.cat([b, b.new_zeros(pad)], 0)
            return K.pack_conv(w, bias=b, stride=1, pad=0)

        pc = self._predictor_cache.get([conv.weight, conv.bias], build)
        pc.two_acc = True      # the logits feed an argmax
        pc.state = conv._range_state
        return pc

    def forward_nhwc(self, features):
        """features {name: [N,H_l,W_l,C]} -> the stride-COMMON_STRIDE logits [N,h,w,logits_ld] (channels past NUM_CLASSES: the packed
        operand's zero padding).  Gradient-free."""
        with torch.no_grad():
            x = None
            for f, head in zip(self.in_features, self.scale_heads):
                y, ops = features[f], list(head)
                for k, op in enumerate(ops):
                    if isinstance(op, Upsample2):
                        last = k == len(ops) - 1
                        if last and x is not None:
                            x = op.forward_nhwc(y, acc=x)
                            y = None
                        else:
                            y = op.forward_nhwc(y)
                    else:
                        y = op.forward_nhwc(y)
                if y is not None:
                    assert x is None
                    x = y
            return K.conv2d_nhwc(x, self.packed_predictor(), relu=False)

    def postprocess(self, logits, image_sizes, out_sizes, want_soft=True, want_labels=True):
        """F.interpolate(x COMMON_STRIDE) + sem_seg_postprocess (+ argmax) of a batch in one launch.  logits: `forward_nhwc`'s.
        -> per image (soft [K, out_h, out_w] fp32 or None, labels [out_h, out_w] uint8 / int32 or None), views of two batch buffers;
        and (labels buffer, label offsets) for the combine step."""
        N, h, w, ld = logits.shape
        Kc = self.num_classes
        jobs, soft_numel, labels_numel = K.sem_seg_jobs([(h, w)] * N, image_sizes, out_sizes, Kc, ld)
        soft, labels = K.sem_seg_postprocess(logits, jobs, Kc, self.common_stride, soft_numel, labels_numel, want_soft=want_soft,
                                             want_labels=want_labels)
        out = []
        for i, (oh, ow) in enumerate(out_sizes):
            s = soft[int(jobs[i, 7]): int(jobs[i, 7]) + Kc * oh * ow].view(Kc, oh, ow) if want_soft else None
            l = labels[int(jobs[i, 8]): int(jobs[i, 8]) + oh * ow].view(oh, ow) if want_labels else None
            out.append((s, l))
        return out, labels, [int(v) for v in jobs[:, 8]]

    def forward(self, features, targets=None):
        """The reference's interface on NCHW maps: eval -> ([N, K, H, W] logits at the input resolution, {}).  The models go through
        `forward_nhwc` + `postprocess` instead and never form this tensor."""
        if self.training:
            raise NotImplementedError(TRAIN_REFUSAL)
        from ...layers.layout import to_nhwc

        logits = self.forward_nhwc({f: to_nhwc(features[f]) for f in self.in_features})
        N, h, w, _ = logits.shape
        s = self.common_stride
        res, _, _ = self.postprocess(logits, [(h * s, w * s)] * N, [(h * s, w * s)] * N, want_labels=False)
        return torch.stack([r[0] for r in res]), {}


def semantic_outputs(head, feats, batched_inputs, sizes, out_sizes, keep_logits, need_labels):
    """Head + postprocess on the trunk's NHWC features -> (per image result dict, labels buffer, label offsets)."""
    logits = head.forward_nhwc(feats)
    res, labels, label_off = head.postprocess(logits, [tuple(s) for s in sizes], [tuple(s) for s in out_sizes], want_soft=keep_logits,
                                              want_labels=need_labels or not keep_logits)
    out = [{"sem_seg": s} if keep_logits else {"sem_seg_labels": l} for s, l in res]
    return out, labels, label_off


@META_ARCH_REGISTRY.register()
class SemanticSegmentor(_RCNNBase):
    """reference semantic_seg.py:33-96: backbone + semantic head; output key "sem_seg" ([K, H, W] soft logits at the output size), or
    with `keep_sem_seg_logits = False` "sem_seg_labels" ([H, W] label map) in its place."""

    keep_sem_seg_logits = True

    def __init__(self, cfg):
        super().__init__()
        self._init_common(cfg)
        self.backbone = build_backbone(cfg)
        self.sem_seg_head = build_sem_seg_head(cfg, self.backbone.output_shape())
        self.to(self.device)

    def forward(self, batched_inputs):
        if self.training:
            raise NotImplementedError(TRAIN_REFUSAL)
        from ..roi_heads.roi_heads import run_with_fallbacks

        return run_with_fallbacks(self, lambda: self._inference(batched_inputs))

    def _inference(self, batched_inputs):
        x4, sizes = self.preprocess_nhwc(batched_inputs)
        out_sizes = [(int(h), int(w)) for h, w in self.post_rows(batched_inputs, sizes)[1]]
        feats = self.backbone.forward_nhwc(x4)
        out, _, _ = semantic_outputs(self.sem_seg_head, feats, batched_inputs, sizes, out_sizes, self.keep_sem_seg_logits, False)
        K.check_conv_error_word(self.device)      # the pass's one read: the conv kernels' range words
        return out
