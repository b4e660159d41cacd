"""KRCNNConvDeconvUpsampleHead (reference detectron2/modeling/roi_heads/keypoint_head.py:128-262): the 3x3 convs with ReLU
(`conv_fcn{k}`), the 4x4 stride-2 padding-1 transposed convolution `score_lowres`, the bilinear x2 upsampling and, at inference,
`heatmaps_to_keypoints` (detectron2/structures/keypoints.py:145-212).  Parameter names and initialisation are the reference's.

The convs run on the channels-last RoI maps [M, S, S, C] through `Conv2d.forward_nhwc`.  `score_lowres` is one launch
(csrc/keypoint.hip) that writes the low-resolution logit planes [M, K, 2S, 2S]; the decode is one launch (csrc/keypoint_decode.hip)
that forms the bilinear x2 map on chip, resizes it to every box with ATen's bicubic rule, and keeps maximum, position and score: the
reference's [M, K, 4S, 4S] tensor and its per-RoI [K, h, w] temporaries are never written.  `layers()` returns that tensor when asked
for (the decode kernel's `maps_out`).

Training (opt-in: `GeneralizedRCNN.enable_keypoint_training()`; without it the training forward refuses with `TRAIN_REFUSAL`): the
same `score_lowres` launch, the loss (lvc_keypoint_loss: the bilinear x2 map is formed on chip with the decode's expression, so
training and inference see the same logits) and the backward (lvc_keypoint_loss_grad, lvc_keypoint_deconv_dx,
lvc_keypoint_deconv_wgrad; csrc/keypoint_train.hip) are ONE autograd node, `KeypointTailLoss`; the convs before it are recorded by
`Conv2d.forward_nhwc`.  `keypoint_rcnn_loss` keeps the reference's signature, but its first argument is a `KeypointTail` -- the
operands of the logits, not yet evaluated -- because the [M, K, 4S, 4S] logits are never formed.

Not built (raises NotImplementedError): GroupNorm in the head."""
import torch
import torch.nn.functional as F
from torch import nn

from ... import kernels as K
from ...layers import Conv2d, ConvTranspose2d, ShapeSpec
from ...layers.layout import to_nhwc
from ...utils.events import get_event_storage
from ...utils.registry import Registry
from .tail import Tail, tail_loss_of_instances

ROI_KEYPOINT_HEAD_REGISTRY = Registry("ROI_KEYPOINT_HEAD")

TRAIN_REFUSAL = "training the keypoint branch (MODEL.KEYPOINT_ON: keypoint_rcnn_loss, gt_keypoints) is not built"


def keypoint_rcnn_inference(keypoints_xyls, pred_instances):
    """The reference's contract (keypoint_head.py:98-125) on the decode kernel's output: `keypoints_xyls` [sum n_i, K, 4] holds, row
    for row of the concatenated instances, (x, y, logit, score); every Instances gets `pred_keypoints` [n_i, K, 3] = (x, y, score)."""
    counts = [len(i) for i in pred_instances]
    assert keypoints_xyls.shape[0] >= sum(counts), (keypoints_xyls.shape, counts)
    real = keypoints_xyls[: sum(counts)]
    parts = torch.cat([real[:, :, :2], real[:, :, 3:4]], 2).split(counts, dim=0)
    for p, inst in zip(parts, pred_instances):
        inst.pred_keypoints = p


_TOTAL_SKIPPED = 0      # steps without a single valid keypoint (reference keypoint_head.py:19, logged as kpts_num_skipped_batches)


def log_skipped_batch():
    """The reference's bookkeeping of a step whose loss had no valid entry (keypoint_head.py:77-82)."""
    global _TOTAL_SKIPPED
    _TOTAL_SKIPPED += 1
    get_event_storage().put_scalar("kpts_num_skipped_batches", _TOTAL_SKIPPED, smoothing_hint=False)


class KeypointTailLoss(torch.autograd.Function):
    """`score_lowres` and the keypoint loss as one node: forward = lvc_keypoint_deconv (the inference launch: the same bits) +
    lvc_keypoint_loss, backward = lvc_keypoint_loss_grad, then lvc_keypoint_deconv_dx and lvc_keypoint_deconv_wgrad where
    `needs_input_grad` asks for them.  x [M, S, S, Cin] channels-last; weight [Cin, K, 4, 4]; bias [K]; target int32 / valid uint8
    [M, K]; num_valid: device int32 [1] or None; normalizer: None (the counted valid entries) or the number; packed / packed_dx: the
    layer's cached operands (None: packed here).  -> (loss scalar, fp64 sum [1], valid count int64 [1]); gradients for x, weight and
    bias.  The upstream scalar stays on the device (a LossScaler makes it 1024)."""

    @staticmethod
    def forward(ctx, x, weight, bias, target, valid, num_valid, status, normalizer, loss_weight, packed, packed_dx):
        k = weight.shape[1]
        if packed is None:
            packed = K.pack_keypoint_deconv(weight)
        low = K.keypoint_deconv(x, packed, None if bias is None else bias.detach(), k, num_valid=num_valid)
        loss, total, count, _term, pmax, plse = K.keypoint_loss(low, target, valid, num_valid=num_valid, normalizer=normalizer,
                                                                loss_weight=loss_weight, status=status)
        ctx.save_for_backward(x, weight, low, target, valid, pmax, plse, count)
        ctx.misc = (num_valid, normalizer, loss_weight, packed_dx, bias is not None)
        ctx.mark_non_differentiable(total, count)
        return loss.view(()), total, count

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_total, _g_count):
        x, weight, low, target, valid, pmax, plse, count = ctx.saved_tensors
        num_valid, normalizer, loss_weight, packed_dx, has_bias = ctx.misc
        need = ctx.needs_input_grad
        k = weight.shape[1]
        up = g.reshape(1).to(torch.float32).contiguous()
        dlow = K.keypoint_loss_grad(low, target, valid, pmax, plse, count, up, num_valid=num_valid, normalizer=normalizer,
                                    loss_weight=loss_weight)
        dx = dw = db = None
        if need[0]:
            if packed_dx is None:
                packed_dx = K.pack_keypoint_deconv_dx(weight)
            dx = K.keypoint_deconv_dx(dlow, packed_dx, k, num_valid=num_valid)
        if need[1] or (has_bias and need[2]):
            dw, db = K.keypoint_deconv_wgrad(x, dlow, k, num_valid=num_valid)
        return (dx, dw if need[1] else None, db if has_bias and need[2] else None) + (None,) * 8


KeypointTail = Tail      # (the logits [M, K, 4S, 4S] as their operands)


def keypoint_rcnn_loss(pred_keypoint_logits, instances, normalizer):
    """Reference signature (keypoint_head.py:40-96).  `pred_keypoint_logits`: a `KeypointTail` (see there) whose rows correspond 1:1 to
    the concatenated `instances`, each with `proposal_boxes` and `gt_keypoints` (one per row); normalizer: the number to divide by, or
    None for the visible keypoints of the batch.  One device->host read (the valid count and the status word); with no valid entry
    the loss is 0 and `kpts_num_skipped_batches` is logged.  Returns the scalar loss, not yet multiplied by LOSS_WEIGHT."""
    if not isinstance(pred_keypoint_logits, KeypointTail):
        raise TypeError("keypoint_rcnn_loss takes the head's KeypointTail: the logits [M, K, 4S, 4S] are never formed")
    tail = pred_keypoint_logits

    def per_image(inst, side):
        return inst.gt_keypoints.to_heatmap(inst.proposal_boxes.tensor.to(tail.x.device), side)

    def tail_loss(rows, status):
        loss, _total, count = tail.head.tail_loss(tail.x, rows[0].to(torch.int32), rows[1].to(torch.uint8), status=status, normalizer=normalizer,
                                                  loss_weight=1.0)
        return loss, count

    loss, meta = tail_loss_of_instances("keypoint", tail, instances, per_image, tail_loss)
    if meta is not None:      # (meta: the reference reads valid.numel() here)
        check_keypoint_status(meta[1], tail.shape[2])
    if meta is None or meta[0] == 0:
        log_skipped_batch()
    return loss


def check_keypoint_status(st, side=None):
    if st & K.KEYPOINT_BAD_TARGET:
        raise IndexError("keypoint head: a heatmap target lies outside the map{}".format("" if side is None else " [0, {})".format(side * side)))


@ROI_KEYPOINT_HEAD_REGISTRY.register()
class KRCNNConvDeconvUpsampleHead(nn.Module):
    loss_takes_classes = False      # `train_loss` takes the targets only

    def __init__(self, cfg, input_shape: ShapeSpec):
        super().__init__()
        H = cfg.MODEL.ROI_KEYPOINT_HEAD
        self.num_keypoints = int(H.NUM_KEYPOINTS)
        # reference BaseKeypointRCNNHead.from_config (keypoint_head.py:152-169)
        self.loss_weight = float(H.LOSS_WEIGHT)
        if H.NORMALIZE_LOSS_BY_VISIBLE_KEYPOINTS:
            self.loss_normalizer = "visible"
        else:
            self.loss_normalizer = float(self.num_keypoints * cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE * cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION)
        self.up_scale = 2
        self.map_scale = 2 * self.up_scale      # the maps are map_scale x the pooled side
        conv_dims = list(H.CONV_DIMS)
        self.blocks = []
        cur = input_shape.channels
        for k, dim in enumerate(conv_dims, 1):
            conv = Conv2d(cur, dim, kernel_size=3, stride=1, padding=1, bias=True, norm=None, activation=F.relu)
            self.add_module("conv_fcn{}".format(k), conv)
            self.blocks.append(conv)
            cur = dim
        K.keypoint_deconv_check(cur, self.num_keypoints)      # names MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS / NUM_KEYPOINTS
        self.score_lowres = ConvTranspose2d(cur, self.num_keypoints, kernel_size=4, stride=2, padding=1)
        for name, param in self.named_parameters():
            if "bias" in name:
                nn.init.constant_(param, 0)
            elif "weight" in name:
                # Caffe2's MSRAFill (reference keypoint_head.py:242-248)
                nn.init.kaiming_normal_(param, mode="fan_out", nonlinearity="relu")

    @property
    def num_maps(self):
        return self.num_keypoints

    def _convs_nhwc(self, x):
        for layer in self.blocks:
            x = layer.forward_nhwc(x)
        return x

    def lowres_nhwc(self, pooled, num_valid=None):
        """pooled [M, S, S, C] channels-last -> the low-resolution logit planes [M, K, 2S, 2S] (rows past num_valid are not written)."""
        x = self._convs_nhwc(pooled)
        return K.keypoint_deconv(x.contiguous(), self.score_lowres.packed(), self.score_lowres.bias, self.num_keypoints,
                                 num_valid=num_valid)

    def forward_nhwc(self, pooled, boxes, num_valid=None, status=None):
        """pooled [M, S, S, C] channels-last RoI maps; boxes [M, 4] (the coordinates the keypoints come out in); num_valid: device int32
        [1], rows past it are skipped by `score_lowres` and the decode (the convs run on all rows).  `status` is taken for symmetry
        with the mask head; neither kernel raises a condition.  Returns [M, K, 4] = (x, y, logit, score)."""
        M = pooled.shape[0]
        if M == 0:
            return pooled.new_zeros((0, self.num_keypoints, 4))
        low = self.lowres_nhwc(pooled, num_valid=num_valid)
        # rows past num_valid keep their bytes: zeros, so that nothing uninitialised is ever gathered
        out = torch.zeros(M, self.num_keypoints, 4, device=pooled.device, dtype=torch.float32)
        return K.heatmaps_to_keypoints(low, boxes.contiguous(), up=self.up_scale, num_valid=num_valid, out=out)

    def normalizer(self, num_images):
        """The number the summed loss is divided by (reference keypoint_head.py:187-190): None = the visible keypoints of the batch."""
        return None if self.loss_normalizer == "visible" else num_images * self.loss_normalizer

    def tail_loss(self, x, target, valid, num_valid=None, status=None, normalizer=None, loss_weight=None):
        """x [M, S, S, C] after the conv_fcn convs -> `KeypointTailLoss` with this head's `score_lowres`."""
        sl = self.score_lowres
        packed = sl.packed()      # (rebuilt when the parameter has changed)
        packed_dx = sl.packed_dx() if (x.requires_grad and torch.is_grad_enabled()) else None
        return KeypointTailLoss.apply(x.contiguous(), sl.weight, sl.bias, target, valid, num_valid, status, normalizer,
                                      self.loss_weight if loss_weight is None else loss_weight, packed, packed_dx)

    def loss_nhwc(self, pooled, target, valid, num_valid=None, status=None, num_images=1):
        """Training on padded rows, nothing read back: pooled [M, S, S, C]; target int32 / valid uint8 [M, K]
        (`kernels.keypoint_targets`); num_valid: device int32 [1] (the convs run on all rows, `score_lowres`, loss and backward on
        the rows below it); num_images: the images of the batch (the fixed normaliser's factor).
        -> (loss_keypoint scalar, LOSS_WEIGHT applied; fp64 sum [1]; valid count int64 [1])."""
        return self.tail_loss(self._convs_nhwc(pooled), target, valid, num_valid=num_valid, status=status, normalizer=self.normalizer(num_images))

    def train_targets(self, boxes, matched, count, gt_keypoints, side):
        """The branch's targets on the padded tables (`StandardROIHeads._branch_loss_batched`): boxes [B, R, 4], matched int64 [B, R],
        count int32 [B], gt_keypoints: one Keypoints per image; one launch makes targets, valid flags and the row selection
        -> ((target int32, valid uint8 [B*R, K]), its counts by name: the selected and the foreground rows of every image)."""
        with torch.no_grad():
            target, valid, _selected, sel_count = K.keypoint_targets(boxes, matched, count, [k.tensor.contiguous() for k in gt_keypoints], side)
        return (target, valid), {"selected": sel_count, "fg": count}

    def train_loss(self, pooled, rows, num_valid, status, num_images):
        """rows: (target, valid) in the order of `pooled` -> (loss_keypoint, its counts by name)."""
        loss, _sum, vcount = self.loss_nhwc(pooled, rows[0], rows[1], num_valid=num_valid, status=status, num_images=num_images)
        return loss, {"valid": vcount}

    def layers(self, x):
        """Reference signature: x [M, C, S, S] -> the logits [M, K, 4S, 4S] (the decode kernel's `maps_out`; the boxes are dummies)."""
        h = to_nhwc(x).contiguous()
        M = h.shape[0]
        side = 2 * self.up_scale * h.shape[1]
        maps = torch.zeros(M, self.num_keypoints, side, side, device=h.device, dtype=torch.float32)
        if M == 0:
            return maps
        low = self.lowres_nhwc(h)
        K.heatmaps_to_keypoints(low, torch.zeros(M, 4, device=h.device), up=self.up_scale, maps_out=maps)
        return maps

    def forward(self, x, instances):
        """Reference signature (BaseKeypointRCNNHead.forward, inference): x [M, C, S, S] pooled features of the concatenated instances,
        which get `pred_keypoints` [n, K, 3]."""
        if self.training:
            if not self.__dict__.get("_keypoint_train_enabled", False):
                raise NotImplementedError(TRAIN_REFUSAL)
            h = to_nhwc(x).contiguous()
            if h.shape[0] > 0:      # (no instance at all: the convs take no empty batch, and the loss below is x.sum() * 0)
                h = self._convs_nhwc(h)
            loss = keypoint_rcnn_loss(KeypointTail(h, self), instances, normalizer=self.normalizer(len(instances)))
            return {"loss_keypoint": loss * self.loss_weight}
        boxes = torch.cat([i.pred_boxes.tensor for i in instances]).to(torch.float32)
        keypoint_rcnn_inference(self.forward_nhwc(to_nhwc(x).contiguous(), boxes), instances)
        return instances


def build_keypoint_head(cfg, input_shape):
    return ROI_KEYPOINT_HEAD_REGISTRY.get(cfg.MODEL.ROI_KEYPOINT_HEAD.NAME)(cfg, input_shape)
