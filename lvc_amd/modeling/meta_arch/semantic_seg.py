"""SemSegFPNHead / SemanticSegmentor (reference detectron2/modeling/meta_arch/semantic_seg.py).

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

Training is opt-in (`enable_sem_seg_training()`; without it a model in training mode refuses before anything touches a device).  The
head then runs on the same NHWC features under autograd: the scale heads through `Conv2d.forward_nhwc` (conv -> GN -> ReLU), the x2
upsamples through `_Upsample2Fn` (backward: csrc/sem_seg_train.hip's gather kernel; the accumulator's gradient is dy itself), the
predictor in its packed, zero-padded form (`_PackedPredictorFn`: the training logits are `forward_nhwc`'s bits; the padded rows of
dW / db are dropped), and `loss_sem_seg` as ONE autograd.Function from the stride-`COMMON_STRIDE` logits and the label maps where
they lie -- forward `lvcst_sem_seg_loss_fwd`, backward `lvcst_sem_seg_loss_bwd` -- so the training path never forms the
full-resolution map either.
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


class _Upsample2Fn(torch.autograd.Function):
    """y = up2(x), or y = acc + up2(x) (a new tensor: the accumulator is another node's output).  Backward: dx by the gather kernel of
    csrc/sem_seg_train.hip, and d acc = dy itself, passed through."""

    @staticmethod
    def forward(ctx, x, acc):
        ctx.has_acc = acc is not None
        return K.upsample2_bilinear_nhwc(x, acc=acc)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = K.upsample2_bilinear_bwd_nhwc(dy) if ctx.needs_input_grad[0] else None
        return dx, dy if ctx.has_acc and ctx.needs_input_grad[1] else None


def upsample2_bilinear(x, acc=None):
    """`K.upsample2_bilinear_nhwc` under autograd: up2(x), or acc + up2(x) with the accumulator added last."""
    return _Upsample2Fn.apply(x, acc)


class _PackedPredictorFn(torch.autograd.Function):
    """The 1x1 predictor in its packed form (output channels zero-padded to `logits_ld`): the launch of `forward_nhwc`, so the training
    logits are its bits.  Backward from the [N,h,w,ld] gradient: dW and db of the ld rows, of which the first NUM_CLASSES are the
    parameters' (the padded rows are dropped), and dx on the predictor's own data-gradient operand, whose contraction is padded with
    zero rows to the same width."""

    @staticmethod
    def forward(ctx, x, weight, bias, head):
        ctx.save_for_backward(x)
        ctx.head = head
        return K.conv2d_nhwc(x, head.packed_predictor(), relu=False)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        head, dy = ctx.head, dy.contiguous()
        kc = head.num_classes
        dx = dw = db = None
        if ctx.needs_input_grad[1]:
            dw = K.conv_wgrad(x, dy, None, 1, 1, 1, 0)[:kc].permute(0, 3, 1, 2).contiguous()      # [ld,1,1,C] -> the parameter's OIHW
        if ctx.needs_input_grad[2]:
            db = K.colsum_rows(dy.view(-1, dy.shape[-1]))[:kc]
        if ctx.needs_input_grad[0]:
            dx = K.conv_dgrad(dy, head.predictor.packed_dgrad(), x.shape, 1)
        return dx, dw, db, None


class _SemSegLossFn(torch.autograd.Function):
    """mean cross entropy of the x`scale` bilinear interpolation of the logits against the label maps (ignore_index), from the
    stride-`scale` logits: forward lvcst_sem_seg_loss_fwd (keeps the per-pixel max and log-sum maps, the two parts of the log-sum-exp),
    backward lvcst_sem_seg_loss_bwd (reads the upstream scalar and the valid-pixel count on the device)."""

    @staticmethod
    def forward(ctx, logits, labels, jobs, num_classes, scale, ignore_value, status):
        loss, (mmax, lsum), _total, count, d_jobs = K.sem_seg_loss_fwd(logits, labels, jobs, num_classes, scale, ignore_value, status)
        ctx.save_for_backward(logits, labels, mmax, lsum, count, d_jobs)
        ctx.args = (jobs, num_classes, scale, ignore_value)
        return loss.view(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        logits, labels, mmax, lsum, count, d_jobs = ctx.saved_tensors
        jobs, num_classes, scale, ignore_value = ctx.args
        dlow = K.sem_seg_loss_bwd(logits, labels, jobs, d_jobs, num_classes, scale, ignore_value, (mmax, lsum), g.contiguous().view(1), count)
        return dlow, None, None, None, None, None, None


def sem_seg_loss(logits, labels, jobs, num_classes, scale, ignore_value, status):
    """-> the scalar mean loss (fp32, on the device) of logits [N,h,w,ld] against the label maps in `labels` (`K.sem_seg_loss_jobs`)."""
    return _SemSegLossFn.apply(logits, labels, jobs, int(num_classes), int(scale), int(ignore_value), status)


def check_sem_seg_items(batched_inputs, ignore_value, sizes=None):
    """The host's refusals, before anything touches a device: every item carries "sem_seg", an integer tensor of its image's size
    (sizes: per item (h, w); default the item's "image"), and IGNORE_VALUE is a value the maps' type holds.  -> the maps."""
    maps = []
    for i, inp in enumerate(batched_inputs):
        if "sem_seg" not in inp:
            raise ValueError('item {}: no "sem_seg" (the ground-truth label map [H, W] of the image) to train the semantic branch on'.format(i))
        m = inp["sem_seg"]
        if not torch.is_tensor(m) or m.is_floating_point() or m.dtype == torch.bool or m.is_complex():
            raise ValueError('item {}: "sem_seg" must be an integer tensor, got {}'.format(i, getattr(m, "dtype", type(m).__name__)))
        size = sizes[i] if sizes is not None else (tuple(inp["image"].shape[-2:]) if "image" in inp else None)
        if size is not None and tuple(m.shape) != (int(size[0]), int(size[1])):
            raise ValueError('item {}: "sem_seg" is {} but the image is {}'.format(i, tuple(m.shape), (int(size[0]), int(size[1]))))
        maps.append(m)
    if maps and all(m.dtype == torch.uint8 for m in maps) and not 0 <= int(ignore_value) <= 255:
        raise ValueError('MODEL.SEM_SEG_HEAD.IGNORE_VALUE = {}: outside what the uint8 "sem_seg" maps hold'.format(ignore_value))
    return maps


def sem_seg_targets(batched_inputs, sizes, device, ignore_value):
    """The items' "sem_seg" label maps as ONE device buffer and its job table.  Each map is an integer tensor of its item's image size
    (`sizes`: what the network saw); the padding to the batch size is the loss kernel's (a pixel outside a map counts as IGNORE_VALUE).
    -> (labels uint8 / int64 [sum h*w], jobs)."""
    maps = check_sem_seg_items(batched_inputs, ignore_value, sizes)
    dtype = torch.uint8 if all(m.dtype == torch.uint8 for m in maps) else torch.int64
    jobs, _ = K.sem_seg_loss_jobs([tuple(m.shape) for m in maps])
    on_dev = [m.to(device, non_blocking=True).to(dtype).reshape(-1) for m in maps]
    return (on_dev[0] if len(on_dev) == 1 else torch.cat(on_dev)).contiguous(), jobs


class Upsample2(nn.Module):
    """The parameter-free slot of nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False) in a scale head."""

    def forward_nhwc(self, x, acc=None):
        if torch.is_grad_enabled() and (x.requires_grad or (acc is not None and acc.requires_grad)):
            return upsample2_bilinear(x, acc)
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

    def _level_sum(self, features):
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
        return x

    def forward_nhwc(self, features):
        """features {name: [N,H_l,W_l,C]} -> the stride-COMMON_STRIDE logits [N,h,w,logits_ld] (channels past NUM_CLASSES: the packed
        operand's zero padding).  Gradient-free."""
        with torch.no_grad():
            return K.conv2d_nhwc(self._level_sum(features), self.packed_predictor(), relu=False)

    def forward_train_nhwc(self, features):
        """`forward_nhwc` under autograd: the same launches in the same order (an accumulating upsample writes a new tensor, not the
        running sum), so the logits are the same bits; every step has its backward on the device."""
        x = self._level_sum(features)
        p = self.predictor
        if torch.is_grad_enabled() and (x.requires_grad or p.weight.requires_grad or p.bias.requires_grad):
            return _PackedPredictorFn.apply(x, p.weight, p.bias, self)
        return K.conv2d_nhwc(x, self.packed_predictor(), relu=False)

    def losses(self, predictions, targets, status=None):
        """reference semantic_seg.py:179-187 with the stride-COMMON_STRIDE logits [N,h,w,logits_ld] in place of the full-size map, which
        is never formed.  targets: (labels buffer, job table) of `sem_seg_targets`.  status: the int32 word the loss kernel ORs an
        out-of-range label into (a new one when None; `check_loss_status` reads it).  -> {"loss_sem_seg": loss * LOSS_WEIGHT}."""
        labels, jobs = targets
        if status is None:
            status = torch.zeros(1, device=predictions.device, dtype=torch.int32)
        self.__dict__["_loss_status"] = status
        loss = sem_seg_loss(predictions, labels, jobs, self.num_classes, self.common_stride, self.ignore_value, status)
        return {"loss_sem_seg": loss * self.loss_weight}

    def check_loss_status(self, word):
        """Raise for the host copy of the loss's status word, as torch's CPU cross entropy raises for such a target."""
        if int(word) & K.SEGTRAIN_STATUS_LABEL_RANGE:
            raise IndexError('"sem_seg": a label is neither MODEL.SEM_SEG_HEAD.IGNORE_VALUE ({}) nor in [0, NUM_CLASSES = {}): target out of '
                             "bounds".format(self.ignore_value, self.num_classes))

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
        `forward_nhwc` + `postprocess` (training: `forward_train_nhwc` + `losses`) instead and never form this tensor."""
        if self.training:
            raise NotImplementedError(TRAIN_REFUSAL + " through SemSegFPNHead.forward: the models call forward_train_nhwc and losses "
                                      "(enable_sem_seg_training)")
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

    def enable_sem_seg_training(self, on=True):
        """Switch the training forward on (or off again); returns self.  Without the call the model in training mode refuses, as
        before.  Every item then carries "sem_seg": an integer label map of the image's size."""
        self.__dict__["_sem_seg_train_enabled"] = bool(on)
        return self

    def forward(self, batched_inputs):
        from ..roi_heads.roi_heads import run_with_fallbacks

        if self.training:
            if not self.__dict__.get("_sem_seg_train_enabled", False):
                raise NotImplementedError(TRAIN_REFUSAL)
            check_sem_seg_items(batched_inputs, self.sem_seg_head.ignore_value)
            return run_with_fallbacks(self, lambda: self._forward_train(batched_inputs))
        return run_with_fallbacks(self, lambda: self._inference(batched_inputs))

    def _losses_device(self, batched_inputs):
        """The step up to its one read: preprocess -> trunk (a graph only if something in it trains) -> head -> loss.
        -> (losses, the words that read brings back: the loss's status word, then the conv kernels' range summary)."""
        self._prepack_trainable()
        x4, sizes = self.preprocess_nhwc(batched_inputs)
        targets = sem_seg_targets(batched_inputs, sizes, self.device, self.sem_seg_head.ignore_value)
        with torch.set_grad_enabled(torch.is_grad_enabled() and any(p.requires_grad for p in self.backbone.parameters())):
            feats = self.backbone.forward_nhwc(x4)
        logits = self.sem_seg_head.forward_train_nhwc(feats)
        status = torch.zeros(1, device=self.device, dtype=torch.int32)
        losses = self.sem_seg_head.losses(logits, targets, status)
        return losses, torch.cat([status.long(), K.range_summary(self.device).long()])

    def _forward_train(self, batched_inputs):
        losses, words = self._losses_device(batched_inputs)
        word, flagged = words.tolist()      # the step's one read
        if flagged:
            K.check_conv_error_word(self.device)      # re-routes the layers concerned and raises: `run_with_fallbacks` repeats the pass
        self.sem_seg_head.check_loss_status(word)
        return losses

    def _inference(self, batched_inputs):
        x4, sizes = self.preprocess_nhwc(batched_inputs)
        out_sizes = [(int(h), int(w)) for h, w in self.post_rows(batched_inputs, sizes)[1]]
        feats = self.backbone.forward_nhwc(x4)
        out, _, _ = semantic_outputs(self.sem_seg_head, feats, batched_inputs, sizes, out_sizes, self.keep_sem_seg_logits, False)
        K.check_conv_error_word(self.device)      # the pass's one read: the conv kernels' range words
        return out
