"""MaskRCNNConvUpsampleHead (reference detectron2/modeling/roi_heads/mask_head.py:31-285): NUM_CONV 3x3 convs with
ReLU (`mask_fcn{k}`), a 2x2 stride-2 transposed convolution (`deconv`), ReLU, and the 1x1 `predictor`.  Parameter names and
initialisation are the reference's.

The convs run on the channels-last RoI maps [M, S, S, C] through `Conv2d.forward_nhwc`, as the conv box head's do.  The tail --
deconv + ReLU + predictor + pick the predicted class + sigmoid -- is ONE launch (csrc/mask_deconv.hip): the reference's
[M, C, 2S, 2S] and [M, K, 2S, 2S] tensors are never formed, only the selected-class probabilities [M, 2S, 2S] leave the kernel.

Training (opt-in: `GeneralizedRCNN.enable_mask_training()`): the same tail with the GROUND-TRUTH class and without the sigmoid
(lvc_mask_deconv_logits), the loss (lvc_mask_loss) and the tail's backward (lvc_mask_deconv_grad) are ONE autograd node,
`MaskTailLoss`; the convs before it are recorded by `Conv2d.forward_nhwc`.  `mask_rcnn_loss` keeps the reference's signature, but its
first argument is a `MaskTail` -- the tail's operands, not yet evaluated -- because the all-class logits are never formed.

Not built (each raises NotImplementedError): GroupNorm in the head (MODEL.ROI_MASK_HEAD.NORM), `layers()` with all-class logits,
VIS_PERIOD > 0, ground-truth masks that are not BitMasks (INPUT.MASK_FORMAT "bitmask")."""
import torch
import torch.nn.functional as F
from torch import nn

from ... import kernels as K
from ...layers import Conv2d, ConvTranspose2d, ShapeSpec
from ...layers.layout import to_nhwc
from ...utils import weight_init
from ...utils.events import get_event_storage
from ...utils.registry import Registry
from .tail import Tail, tail_loss_of_instances

ROI_MASK_HEAD_REGISTRY = Registry("ROI_MASK_HEAD")


def mask_rcnn_inference(prob, pred_instances):
    """The reference's contract (mask_head.py:113-151) on the kernel's output: `prob` [sum n_i, 2S, 2S] holds, row for row of the
    concatenated instances, the probabilities of each instance's predicted class (the kernel has already selected the class and
    applied the sigmoid); every Instances gets `pred_masks` [n_i, 1, 2S, 2S]."""
    counts = [len(i) for i in pred_instances]
    assert prob.shape[0] >= sum(counts), (prob.shape, counts)
    parts = prob[: sum(counts)][:, None].split(counts, dim=0)
    for p, inst in zip(parts, pred_instances):
        inst.pred_masks = p


class MaskTailLoss(torch.autograd.Function):
    """The head's tail and the mask loss as one node: forward = lvc_mask_deconv_logits + lvc_mask_loss, backward =
    lvc_mask_deconv_grad (+ the two GEMMs of `kernels.linear_backward`).  x [M, S, S, Cin] channels-last; classes int32 [M] (None:
    class-agnostic); targets uint8 / bool [M, 2S, 2S]; num_valid: device int32 [1] or None.  -> (loss scalar, fp64 sum [1], counts
    int64 [3]); gradients for x, deconv.weight, deconv.bias, predictor.weight, predictor.bias.  The upstream scalar stays on the
    device (a LossScaler makes it 1024)."""

    @staticmethod
    def forward(ctx, x, wd, bd, wp, bp, classes, targets, num_valid, status, packed):
        if packed is None:
            packed = K.pack_mask_deconv(wd)
        wp2 = wp.detach().reshape(wp.shape[0], -1)
        z = K.mask_deconv_logits(x, packed, bd.detach(), wp2, bp.detach(), classes=classes, num_valid=num_valid, status=status)
        loss, total, counts = K.mask_loss(z, targets, num_valid)
        ctx.save_for_backward(x, packed, bd, wp2, z, targets)
        ctx.misc = (classes, num_valid, status, wp.shape)
        ctx.mark_non_differentiable(total, counts)
        return loss.view(()), total, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_total, _g_counts):
        x, packed, bd, wp2, z, targets = ctx.saved_tensors
        classes, num_valid, status, wp_shape = ctx.misc
        need = ctx.needs_input_grad
        up = g.reshape(1).to(torch.float32).contiguous()
        dx, dwd, dbd, dwp, dbp = K.mask_deconv_grad(x, packed, bd, wp2, classes, z, targets, num_valid, up, status=status,
                                                    need_dx=need[0], need_dw=need[1])
        return dx, dwd, dbd, dwp.view(wp_shape), dbp, None, None, None, None, None


MaskTail = Tail      # (the all-class logits [M, K, 2S, 2S] as their operands)


def mask_scalars(counts, numel):
    """mask_rcnn/accuracy, false_positive, false_negative (reference mask_head.py:88-100) from the loss kernel's three counts --
    incorrect, positive and false-positive pixels -- and the number of target pixels."""
    incorrect, positive, false_pos = [float(c) for c in counts]
    return {"mask_rcnn/accuracy": 1 - incorrect / max(float(numel), 1.0),
            "mask_rcnn/false_positive": false_pos / max(float(numel) - positive, 1.0),
            "mask_rcnn/false_negative": (incorrect - false_pos) / max(positive, 1.0)}


def log_mask_scalars(counts, numel):
    storage = get_event_storage()
    for k, v in mask_scalars(counts, numel).items():
        storage.put_scalar(k, v)


def _require_bitmasks(masks):
    from ...structures import BitMasks

    if not isinstance(masks, BitMasks):
        raise NotImplementedError("gt_masks of type {}: the mask targets are built from BitMasks only; set INPUT.MASK_FORMAT to "
                                  "\"bitmask\" (polygon rasterisation is not built)".format(type(masks).__name__))
    return masks


def mask_rcnn_loss(pred_mask_logits, instances, vis_period=0):
    """Reference signature (mask_head.py:31-110).  `pred_mask_logits`: a `MaskTail` (see there) whose rows correspond 1:1 to the
    concatenated `instances`, each with `proposal_boxes`, `gt_classes` and `gt_masks` (BitMasks, one per row).  Logs the three
    mask_rcnn/* scalars (one device->host read) and returns the scalar loss."""
    if vis_period > 0:
        raise NotImplementedError("VIS_PERIOD > 0: visualising the mask predictions is not built")
    if not isinstance(pred_mask_logits, MaskTail):
        raise TypeError("mask_rcnn_loss takes the head's MaskTail: the all-class logits [M, K, 2S, 2S] are never formed")
    head = pred_mask_logits.head

    def per_image(inst, side):
        classes = inst.gt_classes.to(torch.int32)
        planes = _require_bitmasks(inst.gt_masks).crop_and_resize(inst.proposal_boxes.tensor, side)
        return (planes,) if head.cls_agnostic_mask else (classes, planes)

    def tail_loss(rows, status):
        loss, _total, counts = head.tail_loss(pred_mask_logits.x, rows[0] if len(rows) == 2 else None, rows[-1], status=status)
        return loss, counts

    loss, meta = tail_loss_of_instances("mask", pred_mask_logits, instances, per_image, tail_loss)
    if meta is None:
        return loss
    if meta[3] & K.MASK_BAD_CLASS:      # (meta: the reference reads its three scalars with .item())
        raise IndexError("mask head: a ground-truth class lies outside [0, {})".format(head.num_classes))
    side = pred_mask_logits.shape[2]
    log_mask_scalars(meta[:3], pred_mask_logits.x.shape[0] * side * side)
    return loss


@ROI_MASK_HEAD_REGISTRY.register()
class MaskRCNNConvUpsampleHead(nn.Module):
    map_scale = 2                   # the maps are map_scale x the pooled side
    loss_takes_classes = True       # `train_loss` takes the rows' classes before the targets

    def __init__(self, cfg, input_shape: ShapeSpec):
        super().__init__()
        H = cfg.MODEL.ROI_MASK_HEAD
        if H.NORM:
            raise NotImplementedError("MODEL.ROI_MASK_HEAD.NORM = {!r}: normalisation in the mask head is not built (a 14x14x256 sample "
                                      "does not fit the GroupNorm kernel's whole-sample regime)".format(H.NORM))
        conv_dims = [H.CONV_DIM] * (H.NUM_CONV + 1)
        self.num_classes = 1 if H.CLS_AGNOSTIC_MASK else cfg.MODEL.ROI_HEADS.NUM_CLASSES
        self.cls_agnostic_mask = bool(H.CLS_AGNOSTIC_MASK)
        self.vis_period = cfg.VIS_PERIOD
        self.conv_norm_relus = []
        cur = input_shape.channels
        for k, conv_dim in enumerate(conv_dims[:-1]):
            conv = Conv2d(cur, conv_dim, kernel_size=3, stride=1, padding=1, bias=True, norm=None, activation=F.relu)
            self.add_module("mask_fcn{}".format(k + 1), conv)
            self.conv_norm_relus.append(conv)
            cur = conv_dim
        K.mask_deconv_check(cur, conv_dims[-1])      # names MODEL.ROI_MASK_HEAD.CONV_DIM
        self.deconv = ConvTranspose2d(cur, conv_dims[-1], kernel_size=2, stride=2, padding=0)
        self.predictor = Conv2d(conv_dims[-1], self.num_classes, kernel_size=1, stride=1, padding=0)
        for layer in self.conv_norm_relus + [self.deconv]:
            weight_init.c2_msra_fill(layer)
        nn.init.normal_(self.predictor.weight, std=0.001)
        nn.init.constant_(self.predictor.bias, 0)

    @property
    def num_maps(self):
        return self.num_classes

    def _convs_nhwc(self, x):
        for layer in self.conv_norm_relus:
            x = layer.forward_nhwc(x)
        return x

    def forward_nhwc(self, pooled, classes=None, num_valid=None, status=None):
        """pooled [M, S, S, C] channels-last RoI maps; classes [M] int32 (ignored with CLS_AGNOSTIC_MASK); num_valid: device int32,
        rows past it are skipped by the tail kernel.  Returns prob [M, 2S, 2S]: the predicted class's mask probabilities."""
        x = pooled
        M, S = x.shape[0], x.shape[1]
        if M == 0:
            return x.new_zeros((0, 2 * S, 2 * S))
        x = self._convs_nhwc(x)
        if self.cls_agnostic_mask:
            classes = None
        elif classes is None:
            raise ValueError("MaskRCNNConvUpsampleHead.forward_nhwc: class-specific masks need the predicted classes")
        p = self.predictor
        return K.mask_deconv_predict(x.contiguous(), self.deconv.packed(), self.deconv.bias, p.weight.detach().view(p.out_channels, -1),
                                     p.bias, classes=classes, num_valid=num_valid, status=status)

    def forward(self, x, instances):
        """Reference signature (BaseMaskRCNNHead.forward, inference): x [M, C, S, S] pooled features of the concatenated instances,
        which get `pred_masks` [n, 1, 2S, 2S]."""
        if self.training:
            if not self.__dict__.get("_mask_train_enabled", False):
                raise NotImplementedError("training the mask branch (mask_rcnn_loss) is not built")
            h = self._convs_nhwc(to_nhwc(x).contiguous())
            return {"loss_mask": mask_rcnn_loss(MaskTail(h, self), instances, self.vis_period)}
        classes = None
        if not self.cls_agnostic_mask:
            classes = torch.cat([i.pred_classes for i in instances]).to(torch.int32).contiguous()
        status = K.new_status(x.device)
        prob = self.forward_nhwc(to_nhwc(x).contiguous(), classes, status=status)
        if int(status.item()) & K.MASK_BAD_CLASS:
            raise IndexError("mask head: a predicted class lies outside [0, {})".format(self.num_classes))
        mask_rcnn_inference(prob, instances)
        return instances

    def tail_loss(self, x, classes, targets, num_valid=None, status=None):
        """x [M, S, S, C] after the mask_fcn convs -> `MaskTailLoss` with this head's deconv and predictor."""
        if self.cls_agnostic_mask:
            classes = None
        packed = self.deconv.packed()      # (rebuilt when the parameter has changed)
        return MaskTailLoss.apply(x.contiguous(), self.deconv.weight, self.deconv.bias, self.predictor.weight, self.predictor.bias,
                                  classes, targets, num_valid, status, packed)

    def loss_nhwc(self, pooled, classes, targets, num_valid=None, status=None):
        """Training on padded rows, nothing read back: pooled [M, S, S, C]; classes int32 [M]: the ground-truth classes; targets uint8
        [M, 2S, 2S]; num_valid: device int32 [1] (the convs run on all rows, tail and loss on the rows below it).
        -> (loss scalar, fp64 sum [1], counts int64 [3])."""
        return self.tail_loss(self._convs_nhwc(pooled), classes, targets, num_valid=num_valid, status=status)

    def train_targets(self, boxes, matched, count, gt_masks, side):
        """The branch's targets on the padded tables (`StandardROIHeads._branch_loss_batched`): boxes [B, R, 4], matched int64 [B, R],
        count int32 [B], gt_masks: one BitMasks per image -> ((targets uint8 [B*R, side, side],), no counts of its own)."""
        planes = [_require_bitmasks(m).tensor.contiguous() for m in gt_masks]
        return (K.mask_targets(boxes, matched, count, planes, side),), {}

    def train_loss(self, pooled, rows, num_valid, status, num_images):
        """rows: (classes int32, targets) in the order of `pooled` -> (loss_mask, its counts by name)."""
        loss, _sum, counts = self.loss_nhwc(pooled, rows[0].contiguous(), rows[1], num_valid=num_valid, status=status)
        return loss, {"pixels": counts, "rows": num_valid}

    def layers(self, x):
        raise NotImplementedError("MaskRCNNConvUpsampleHead.layers (all-class mask logits) is not built: the kernel computes the "
                                  "predicted class's plane only")


def build_mask_head(cfg, input_shape):
    return ROI_MASK_HEAD_REGISTRY.get(cfg.MODEL.ROI_MASK_HEAD.NAME)(cfg, input_shape)
