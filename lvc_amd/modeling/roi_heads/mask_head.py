"""MaskRCNNConvUpsampleHead, inference side (reference detectron2/modeling/roi_heads/mask_head.py:113-285): NUM_CONV 3x3 convs with
ReLU (`mask_fcn{k}`), a 2x2 stride-2 transposed convolution (`deconv`), ReLU, and the 1x1 `predictor`.  Parameter names and
initialisation are the reference's.

The convs run on the channels-last RoI maps [M, S, S, C] through `Conv2d.forward_nhwc`, as the conv box head's do.  The tail --
deconv + ReLU + predictor + pick the predicted class + sigmoid -- is ONE launch (csrc/mask_deconv.hip): the reference's
[M, C, 2S, 2S] and [M, K, 2S, 2S] tensors are never formed, only the selected-class probabilities [M, 2S, 2S] leave the kernel.

Not built (each raises NotImplementedError): GroupNorm in the head (MODEL.ROI_MASK_HEAD.NORM), `layers()` with all-class logits,
the training loss (`mask_rcnn_loss`)."""
import torch
import torch.nn.functional as F
from torch import nn

from ... import kernels as K
from ...layers import Conv2d, ConvTranspose2d, ShapeSpec
from ...layers.layout import to_nhwc
from ...utils import weight_init
from ...utils.registry import Registry

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


@ROI_MASK_HEAD_REGISTRY.register()
class MaskRCNNConvUpsampleHead(nn.Module):
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

    def forward_nhwc(self, pooled, classes=None, num_valid=None, status=None):
        """pooled [M, S, S, C] channels-last RoI maps; classes [M] int32 (ignored with CLS_AGNOSTIC_MASK); num_valid: device int32,
        rows past it are skipped by the tail kernel.  Returns prob [M, 2S, 2S]: the predicted class's mask probabilities."""
        x = pooled
        M, S = x.shape[0], x.shape[1]
        if M == 0:
            return x.new_zeros((0, 2 * S, 2 * S))
        for layer in self.conv_norm_relus:
            x = layer.forward_nhwc(x)
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
            raise NotImplementedError("training the mask branch (mask_rcnn_loss) is not built")
        classes = None
        if not self.cls_agnostic_mask:
            classes = torch.cat([i.pred_classes for i in instances]).to(torch.int32).contiguous()
        status = K.new_status(x.device)
        prob = self.forward_nhwc(to_nhwc(x).contiguous(), classes, status=status)
        if int(status.item()) & K.MASK_BAD_CLASS:
            raise IndexError("mask head: a predicted class lies outside [0, {})".format(self.num_classes))
        mask_rcnn_inference(prob, instances)
        return instances

    def layers(self, x):
        raise NotImplementedError("MaskRCNNConvUpsampleHead.layers (all-class mask logits) is not built: the kernel computes the "
                                  "predicted class's plane only")


def build_mask_head(cfg, input_shape):
    return ROI_MASK_HEAD_REGISTRY.get(cfg.MODEL.ROI_MASK_HEAD.NAME)(cfg, input_shape)
