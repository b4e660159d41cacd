"""KRCNNConvDeconvUpsampleHead (reference detectron2/modeling/roi_heads/keypoint_head.py:128-262): the 3x3 convs with ReLU
(`conv_fcn{k}`), the 4x4 stride-2 padding-1 transposed convolution `score_lowres`, the bilinear x2 upsampling and, at inference,
`heatmaps_to_keypoints` (detectron2/structures/keypoints.py:145-212).  Parameter names and initialisation are the reference's.

The convs run on the channels-last RoI maps [M, S, S, C] through `Conv2d.forward_nhwc`.  `score_lowres` is one launch
(csrc/keypoint.hip) that writes the low-resolution logit planes [M, K, 2S, 2S]; the decode is one launch (csrc/keypoint_decode.hip)
that forms the bilinear x2 map on chip, resizes it to every box with ATen's bicubic rule, and keeps maximum, position and score: the
reference's [M, K, 4S, 4S] tensor and its per-RoI [K, h, w] temporaries are never written.  `layers()` returns that tensor when asked
for (the decode kernel's `maps_out`).

Not built (raises NotImplementedError): training (`keypoint_rcnn_loss`, `Keypoints.to_heatmap`)."""
import torch
import torch.nn.functional as F
from torch import nn

from ... import kernels as K
from ...layers import Conv2d, ConvTranspose2d, ShapeSpec
from ...layers.layout import to_nhwc
from ...utils.registry import Registry

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


@ROI_KEYPOINT_HEAD_REGISTRY.register()
class KRCNNConvDeconvUpsampleHead(nn.Module):
    def __init__(self, cfg, input_shape: ShapeSpec):
        super().__init__()
        H = cfg.MODEL.ROI_KEYPOINT_HEAD
        self.num_keypoints = int(H.NUM_KEYPOINTS)
        self.up_scale = 2
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

    def lowres_nhwc(self, pooled, num_valid=None):
        """pooled [M, S, S, C] channels-last -> the low-resolution logit planes [M, K, 2S, 2S] (rows past num_valid are not written)."""
        x = pooled
        for layer in self.blocks:
            x = layer.forward_nhwc(x)
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
            raise NotImplementedError(TRAIN_REFUSAL)
        boxes = torch.cat([i.pred_boxes.tensor for i in instances]).to(torch.float32)
        keypoint_rcnn_inference(self.forward_nhwc(to_nhwc(x).contiguous(), boxes), instances)
        return instances


def build_keypoint_head(cfg, input_shape):
    return ROI_KEYPOINT_HEAD_REGISTRY.get(cfg.MODEL.ROI_KEYPOINT_HEAD.NAME)(cfg, input_shape)
