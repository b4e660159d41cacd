"""RetinaNet (reference detectron2/modeling/meta_arch/retinanet.py:37-449): `RetinaNetHead` + `RetinaNet`, inference and training.

`forward(batched_inputs: list[dict]) -> list[{"instances": Instances}]` in eval mode, `-> {"loss_cls", "loss_box_reg"}` in training
mode after `enable_training()`, with the reference's state_dict (names, order, shapes: `backbone.*`,
`head.{cls_subnet,bbox_subnet}.{0,2,4,6}.*`, `head.cls_score.*`, `head.bbox_pred.*`, `anchor_generator.cell_anchors.*`, `pixel_mean`,
`pixel_std`).

Inference launch plan, one stream, fixed shapes, ONE device->host read at the end (per-image counts + the status words):
  preprocess  ->  ResNet / FPN with P6, P7 from res5 (`LastLevelP6P7`)
  ->  the head: every layer of the two towers and the two predictors as ONE launch over the five levels (`kernels.conv3x3_levels`,
      the shared-layer form the RPN head runs on); outputs stay NHWC, so channel a*K + k of a pixel is already the reference's
      `permute_to_N_HWA_K` order
  ->  `kernels.retinanet_select` (csrc/retinanet.hip): threshold + per-level top-k + decode, one pass over the logits
  ->  `kernels.batched_nms_batch` over the L * topk candidate rows of an image  ->  `kernels.gather_detections` (keep order, at most
      DETECTIONS_PER_IMAGE, detector_postprocess).

Training (reference retinanet.py:128-282 `forward`, `losses`, `label_anchors`) is opt-in: a freshly built model in training mode keeps
refusing until `enable_training()` has been called.  One stream, ONE device->host read (the conv kernels' range summary + the number of
positive anchors, logged as `num_pos_anchors`):
  preprocess  ->  trunk and pyramid under autograd according to MODEL.BACKBONE.FREEZE_AT
  ->  the head level by level through `Conv2d.forward_nhwc` (the fused conv autograd function records it; the merged-levels launch and
      the padded 64-channel `bbox_pred` are inference-only)
  ->  `kernels.cat_ground_truth` + `kernels.match_boxes_batched` over the shared anchors (IOU_THRESHOLDS, IOU_LABELS, low-quality
      matches allowed): two launches
  ->  `kernels.retinanet_loss` (csrc/retinanet_loss.hip): focal loss + smooth-L1 in ONE streaming pass over the head's own NHWC outputs
      and a finish that counts the positives and advances the normaliser EMA on the device; its backward is ONE pass
      (`kernels.retinanet_loss_grad`) that writes the gradients of the predictors' outputs already scaled.
Config keys read for it: MODEL.RETINANET.{FOCAL_LOSS_ALPHA, FOCAL_LOSS_GAMMA, SMOOTH_L1_LOSS_BETA, IOU_THRESHOLDS, IOU_LABELS}.  The
box-transform weights stay MODEL.RETINANET.BBOX_REG_WEIGHTS, where the inference path reads them (the reference's training takes
MODEL.RPN.BBOX_REG_WEIGHTS; both default to (1, 1, 1, 1)).
"""
import math

import torch
from torch import nn

from ... import kernels as K
from ...layers import Conv2d
from ...layers.layout import to_nchw_view, to_nhwc
from ...layers.wrappers import _PackedCache
from ..anchor_generator import build_anchor_generator
from ..backbone import build_backbone
from ..box_regression import Box2BoxTransform
from ..roi_heads.roi_heads import instances_from_batched, run_with_fallbacks
from .build import META_ARCH_REGISTRY
from .rcnn import _RCNNBase

MERGE_LEVELS = True      # every head layer over all pyramid levels as one launch (RetinaNetHead.forward_nhwc)
_DELTA_PAD = 64          # bbox_pred's 4A = 36 outputs are packed with zero channels up to the direct 3x3 kernel's narrowest tile


class RetinaNetHead(nn.Module):
    """Two towers of NUM_CONVS x (3x3 conv + ReLU) and a 3x3 predictor each, shared by the levels (reference retinanet.py:377-448)."""

    def __init__(self, cfg, input_shape):
        super().__init__()
        in_channels = input_shape[0].channels
        num_classes = cfg.MODEL.RETINANET.NUM_CLASSES
        num_convs = cfg.MODEL.RETINANET.NUM_CONVS
        prior_prob = cfg.MODEL.RETINANET.PRIOR_PROB
        if cfg.MODEL.RETINANET.get("NORM", ""):
            raise NotImplementedError("MODEL.RETINANET.NORM: a normalised RetinaNet head is not built")
        num_anchors = build_anchor_generator(cfg, input_shape).num_cell_anchors
        if len(set(num_anchors)) != 1:
            raise NotImplementedError("MODEL.ANCHOR_GENERATOR: a different number of anchors per level is not built (nor in the reference)")
        num_anchors = num_anchors[0]
        self.num_anchors, self.num_classes = num_anchors, num_classes
        cls_subnet, bbox_subnet = [], []
        for _ in range(num_convs):
            cls_subnet += [Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1), nn.ReLU()]
            bbox_subnet += [Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1), nn.ReLU()]
        self.cls_subnet = nn.Sequential(*cls_subnet)
        self.bbox_subnet = nn.Sequential(*bbox_subnet)
        self.cls_score = Conv2d(in_channels, num_anchors * num_classes, kernel_size=3, stride=1, padding=1)
        self.bbox_pred = Conv2d(in_channels, num_anchors * 4, kernel_size=3, stride=1, padding=1)
        for modules in [self.cls_subnet, self.bbox_subnet, self.cls_score, self.bbox_pred]:
            for layer in modules.modules():
                if isinstance(layer, Conv2d):
                    # logits / deltas decide a top-k and an NMS: the two-accumulator form of the direct 3x3 kernel, as the RPN head
                    layer.two_acc = True
                    torch.nn.init.normal_(layer.weight, mean=0, std=0.01)
                    torch.nn.init.constant_(layer.bias, 0)
        torch.nn.init.constant_(self.cls_score.bias, -(math.log((1 - prior_prob) / prior_prob)))
        self._bbox_packed = _PackedCache()

    def towers(self):
        """[(Conv2d, relu)] of the classification and of the box branch, predictor last."""
        cls = [(m, True) for m in self.cls_subnet if isinstance(m, Conv2d)] + [(self.cls_score, False)]
        box = [(m, True) for m in self.bbox_subnet if isinstance(m, Conv2d)] + [(self.bbox_pred, False)]
        return cls, box

    def packed_bbox_pred(self):
        """bbox_pred with zero output channels up to `_DELTA_PAD`: 4A = 36 is below the 64 channels the direct 3x3 kernel's narrowest
        tile writes, and the generic fp32 kernel it would fall to is several times slower on the large levels."""
        conv = self.bbox_pred

        def build():
            w, b = conv.weight.detach(), conv.bias.detach()
            pad = max(0, _DELTA_PAD - w.shape[0])
            if pad:
                w = torch.cat([w, w.new_zeros((pad,) + tuple(w.shape[1:]))], 0)
                b = torch.cat([b, b.new_zeros(pad)], 0)
            pc = K.pack_conv(w, bias=b, stride=1, pad=1)
            return pc

        pc = self._bbox_packed.get([conv.weight, conv.bias], build)
        pc.two_acc = True
        pc.state = conv._range_state
        return pc

    def packed_layer(self, conv):
        return self.packed_bbox_pred() if conv is self.bbox_pred else conv.packed()

    def forward_nhwc(self, feats):
        """feats: list of [B,H_l,W_l,C] -> (logits: list of [B,H_l,W_l,A*K], deltas: list of [B,H_l,W_l,>=4A]; channels past 4A of the
        deltas are the packed operand's zero padding).  Gradient-free."""
        cls, box = self.towers()
        outs = []
        for tower in (cls, box):
            xs = list(feats)
            for conv, relu in tower:
                pc = self.packed_layer(conv)
                if MERGE_LEVELS and len(xs) > 1:
                    xs = K.conv3x3_levels(xs, pc, relu=relu)
                else:
                    xs = [K.conv2d_nhwc(x, pc, relu=relu) for x in xs]
            outs.append(xs)
        return outs[0], outs[1]

    def forward_train_nhwc(self, feats):
        """`forward_nhwc` under autograd: level by level through `Conv2d.forward_nhwc`, whose fused autograd function records every
        layer (the weights are shared by the levels: their gradients add up).  -> (logits: list of [B,H_l,W_l,A*K], deltas: list of
        [B,H_l,W_l,4A]), dense."""
        cls, box = self.towers()
        outs = []
        for tower in (cls, box):
            xs = list(feats)
            for conv, relu in tower:
                xs = [conv.forward_nhwc(x, relu=relu) for x in xs]
            outs.append(xs)
        return outs[0], outs[1]

    def forward(self, features):
        """Reference signature: list of NCHW maps -> (list of [N,A*K,H,W], list of [N,4A,H,W])."""
        with torch.no_grad():
            logits, deltas = self.forward_nhwc([to_nhwc(f) for f in features])
        A = self.num_anchors
        return [to_nchw_view(t) for t in logits], [to_nchw_view(t[..., :4 * A]) for t in deltas]


class _RetinaNetLossFn(torch.autograd.Function):
    """(loss_cls, loss_box_reg, num_pos) from the head's per-level outputs: `kernels.retinanet_loss` forward, `kernels.retinanet_loss_grad`
    backward (one launch; the upstream scalars and the normaliser are read on the device)."""

    @staticmethod
    def forward(ctx, pack, norm_in, norm_out, momentum, one_minus_momentum, *outs):
        losses, num_pos = K.retinanet_loss(pack, norm_in, norm_out, momentum, one_minus_momentum)
        ctx.pack, ctx.norm = pack, norm_out
        ctx.mark_non_differentiable(num_pos)
        return losses[0], losses[1], num_pos

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cls, g_box, _g_num):
        dlogits, ddeltas = K.retinanet_loss_grad(ctx.pack, ctx.norm, g_cls.float().contiguous(), g_box.float().contiguous())
        return (None, None, None, None, None) + tuple(dlogits) + tuple(ddeltas)


@META_ARCH_REGISTRY.register()
class RetinaNet(_RCNNBase):
    def __init__(self, cfg):
        super().__init__()
        self._init_common(cfg)
        R = cfg.MODEL.RETINANET
        self.num_classes = R.NUM_CLASSES
        self.in_features = R.IN_FEATURES
        self.score_threshold = R.SCORE_THRESH_TEST
        self.topk_candidates = R.TOPK_CANDIDATES_TEST
        self.nms_threshold = R.NMS_THRESH_TEST
        self.max_detections_per_image = cfg.TEST.DETECTIONS_PER_IMAGE
        self.focal_loss_alpha = float(R.FOCAL_LOSS_ALPHA)
        self.focal_loss_gamma = float(R.FOCAL_LOSS_GAMMA)
        self.smooth_l1_loss_beta = float(R.SMOOTH_L1_LOSS_BETA)
        self.iou_thresholds = [float(v) for v in R.IOU_THRESHOLDS]
        self.iou_labels = [int(v) for v in R.IOU_LABELS]
        self.vis_period = int(cfg.get("VIS_PERIOD", 0))
        self.loss_normalizer_momentum = 0.9
        # the EMA of the number of positive anchors (reference retinanet.py:80-87, a Python float there) as two device doubles: a pass
        # writes the slot that is not current, and the slot becomes current once the pass's range check has succeeded.  Plain tensors,
        # not buffers: the reference's state_dict has no such key
        self.__dict__["_train_enabled"] = False
        self.__dict__["_normalizer"] = {"slots": None, "cur": 0, "value": 100.0}
        self.backbone = build_backbone(cfg)
        backbone_shape = self.backbone.output_shape()
        feature_shapes = [backbone_shape[f] for f in self.in_features]
        self.head = RetinaNetHead(cfg, feature_shapes)
        self.anchor_generator = build_anchor_generator(cfg, feature_shapes)
        self.box2box_transform = Box2BoxTransform(weights=tuple(R.BBOX_REG_WEIGHTS))
        # the reference keeps the normalisation constants as buffers (part of its state_dict); the preprocess kernels take them as
        # host floats, kept next to the buffers and refreshed when a checkpoint brings its own (`_load_from_state_dict`)
        mean, std = self.pixel_mean, self.pixel_std
        del self.pixel_mean, self.pixel_std
        self.__dict__["_norm"] = (mean, std)
        self.register_buffer("pixel_mean", torch.Tensor(mean).view(-1, 1, 1))
        self.register_buffer("pixel_std", torch.Tensor(std).view(-1, 1, 1))
        self.max_survivors = K.RETINANET_MAX_SURVIVORS     # x 4 after every overflow, at last None = H*W*A*K (`widen_limits`)
        self.to(self.device)
        # (MODEL.BACKBONE.FREEZE_AT is the trunk's own)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        mean, std = state_dict.get(prefix + "pixel_mean"), state_dict.get(prefix + "pixel_std")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if mean is not None and std is not None and mean.numel() == 3 and std.numel() == 3:
            self.__dict__["_norm"] = ([float(v) for v in mean.flatten().tolist()], [float(v) for v in std.flatten().tolist()])

    def forward(self, batched_inputs):
        if self.training:
            if not self.__dict__["_train_enabled"]:
                raise NotImplementedError("RetinaNet training is opt-in and has not been enabled on this model: call "
                                          "`model.enable_training()` first")

            def once():
                self._prepack_trainable()
                return self._forward_train(batched_inputs)

            return run_with_fallbacks(self, once)
        return run_with_fallbacks(self, lambda: self._inference(batched_inputs))

    # ------------------------------------------------------------------ training
    def enable_training(self, on=True):
        """Switch the training forward on (or off again); returns self.  Settings the training path does not build raise here, on the
        host, naming their key."""
        if on:
            if self.vis_period > 0:
                raise NotImplementedError("VIS_PERIOD > 0: visualising training batches is not built")
            if 0.0 < self.focal_loss_gamma < 1.0 or self.focal_loss_gamma < 0.0:
                raise NotImplementedError("MODEL.RETINANET.FOCAL_LOSS_GAMMA = {}: an exponent in (0, 1) has an unbounded derivative at "
                                          "saturation; 0 or >= 1 are built".format(self.focal_loss_gamma))
            if len(self.iou_thresholds) not in (1, 2) or len(self.iou_labels) != len(self.iou_thresholds) + 1:
                raise NotImplementedError("MODEL.RETINANET.IOU_THRESHOLDS / IOU_LABELS: one or two thresholds with a label per interval")
        self.__dict__["_train_enabled"] = bool(on)
        return self

    def _normalizer_slots(self):
        st = self.__dict__["_normalizer"]
        if st["slots"] is None or st["slots"][0].device.type != torch.device(self.device).type:
            st["slots"] = [torch.full((1,), st["value"], dtype=torch.float64, device=self.device) for _ in range(2)]
            st["cur"] = 0
        return st

    @property
    def loss_normalizer(self):
        """The EMA the losses were last divided by, as the reference's Python float (reads the device: for logging and tests)."""
        st = self.__dict__["_normalizer"]
        if st["slots"] is None:
            return st["value"]
        return float(st["slots"][st["cur"]].item())

    @loss_normalizer.setter
    def loss_normalizer(self, value):
        st = self.__dict__["_normalizer"]
        st["value"] = float(value)
        if st["slots"] is not None:
            st["slots"][st["cur"]].fill_(float(value))

    def _cat_anchors(self, grid_sizes):
        """`Boxes.cat(anchors)` of the pyramid, [R,4] on the device; built once per set of map sizes."""
        cache = self.__dict__.setdefault("_anchor_cache", {})
        key = tuple((int(h), int(w)) for h, w in grid_sizes)
        t = cache.get(key)
        if t is None or t.device != next(iter(self.anchor_generator.cell_anchors)).device:
            if len(cache) > 64:
                cache.clear()
            t = cache[key] = torch.cat(self.anchor_generator._grid_anchors(key), 0).contiguous()
        return t

    def _loss_pack(self, logits, deltas, anchors, matches, labels, gt, gt_classes, gt_off):
        return K.RetinaNetLossArgs(logits, deltas, self.head.num_anchors, self.num_classes, anchors, matches, labels, gt, gt_classes, gt_off,
                                   alpha=self.focal_loss_alpha, gamma=self.focal_loss_gamma, beta=self.smooth_l1_loss_beta,
                                   box_weights=self.box2box_transform.weights)

    def _forward_train(self, batched_inputs):
        """Reference retinanet.py:146-171.  Everything up to the one read at the end is queued without a host sync."""
        from ...utils.events import get_event_storage
        from ..backbone.resnet import _as_nhwc4

        images = self.preprocess_image(batched_inputs)
        key = "instances" if "instances" in batched_inputs[0] else "targets"
        assert key in batched_inputs[0], "Instance annotations are missing in training!"
        gt_instances = [x[key].to(self.device) for x in batched_inputs]
        B = len(gt_instances)
        with torch.set_grad_enabled(torch.is_grad_enabled() and any(p.requires_grad for p in self.backbone.parameters())):
            feats = self.backbone.forward_nhwc(_as_nhwc4(images.tensor))
        feats = [feats[f] for f in self.in_features]
        logits, deltas = self.head.forward_train_nhwc(feats)
        anchors = self._cat_anchors([(f.shape[1], f.shape[2]) for f in feats])
        gt, gt_off, _lens = K.cat_ground_truth(gt_instances)
        gt_classes = torch.cat([g.gt_classes for g in gt_instances]).to(torch.int64).contiguous()
        matches, labels = K.match_boxes_batched(gt, gt_off, B, anchors, None, self.iou_thresholds, self.iou_labels, True)
        pack = self._loss_pack(logits, deltas, anchors, matches, labels, gt, gt_classes, gt_off)
        st = self._normalizer_slots()
        m = self.loss_normalizer_momentum
        loss_cls, loss_box, num_pos = _RetinaNetLossFn.apply(pack, st["slots"][st["cur"]], st["slots"][1 - st["cur"]], m, 1 - m, *logits, *deltas)
        n, flagged = torch.cat([num_pos, K.range_summary(self.device)]).tolist()      # the ONE read
        if flagged:
            K.check_conv_error_word(self.device)      # re-routes the layers concerned and raises: `run_with_fallbacks` repeats the pass
        st["cur"] = 1 - st["cur"]                     # the pass stands: its normaliser becomes the current one
        get_event_storage().put_scalar("num_pos_anchors", n / B)
        return {"loss_cls": loss_cls, "loss_box_reg": loss_box}

    @torch.no_grad()
    def label_anchors(self, anchors, gt_instances):
        """Reference retinanet.py:238-282: anchors list[Boxes] (per level), gt_instances list[Instances] -> (list of [R] int64 labels in
        {-1, 0..K}: -1 ignored, K background; list of [R,4] matched gt boxes, undefined where the anchor is not foreground).  The
        matching is `kernels.match_boxes_batched`, as in the training forward."""
        at = torch.cat([a.tensor for a in anchors], 0).float().contiguous().to(self.device)
        gt_instances = [g.to(self.device) for g in gt_instances]
        gt, gt_off, lens = K.cat_ground_truth(gt_instances)
        matches, labels = K.match_boxes_batched(gt, gt_off, len(gt_instances), at, None, self.iou_thresholds, self.iou_labels, True)
        out_labels, out_boxes = [], []
        for i, g in enumerate(gt_instances):
            if lens[i] > 0:
                idx = matches[i].long()
                boxes_i = g.gt_boxes.tensor[idx]
                labels_i = g.gt_classes.to(torch.int64)[idx]
                labels_i[labels[i] == 0] = self.num_classes
                labels_i[labels[i] == -1] = -1
            else:
                boxes_i = torch.zeros_like(at)
                labels_i = torch.full((at.shape[0],), self.num_classes, dtype=torch.int64, device=at.device)
            out_labels.append(labels_i)
            out_boxes.append(boxes_i)
        return out_labels, out_boxes

    def losses(self, anchors, pred_logits, gt_labels, pred_anchor_deltas, gt_boxes):
        """Reference retinanet.py:184-236: anchors list[Boxes]; pred_logits / pred_anchor_deltas lists of [N, H_l W_l A, K] / [N, H_l W_l A, 4]
        (`permute_to_N_HWA_K` order); gt_labels / gt_boxes as `label_anchors` returns them -> {"loss_cls", "loss_box_reg"}, differentiable in
        the predictions.  The same two kernels as the training forward (every anchor carries its own matched box); advances the normaliser
        and logs `num_pos_anchors` (one host read)."""
        from ...utils.events import get_event_storage

        A, Kc, N = self.head.num_anchors, self.num_classes, len(gt_labels)
        at = torch.cat([a.tensor for a in anchors], 0).float().contiguous().to(self.device)
        R = at.shape[0]
        gl = torch.stack([t.to(self.device) for t in gt_labels]).to(torch.int64)
        labels = torch.where(gl < 0, -1, torch.where(gl == Kc, 0, 1)).to(torch.int8).contiguous()
        gt = torch.stack([t.to(self.device) for t in gt_boxes]).float().reshape(N * R, 4).contiguous()
        gt_classes = gl.clamp(0, Kc).reshape(-1).contiguous()
        matches = torch.arange(R, dtype=torch.int32, device=at.device).repeat(N, 1).contiguous()
        gt_off = torch.arange(N + 1, dtype=torch.int32, device=at.device) * R
        logits = [t.float().contiguous().view(N, 1, t.shape[1] // A, A * Kc) for t in pred_logits]
        deltas = [t.float().contiguous().view(N, 1, t.shape[1] // A, A * 4) for t in pred_anchor_deltas]
        pack = self._loss_pack(logits, deltas, at, matches, labels, gt, gt_classes, gt_off)
        st = self._normalizer_slots()
        m = self.loss_normalizer_momentum
        loss_cls, loss_box, num_pos = _RetinaNetLossFn.apply(pack, st["slots"][st["cur"]], st["slots"][1 - st["cur"]], m, 1 - m, *logits, *deltas)
        st["cur"] = 1 - st["cur"]
        get_event_storage().put_scalar("num_pos_anchors", int(num_pos.item()) / N)
        return {"loss_cls": loss_cls, "loss_box_reg": loss_box}

    # ------------------------------------------------------------------ inference

    def inference(self, batched_inputs, detected_instances=None, do_postprocess=True):
        """The eval-mode forward under the R-CNN's name (what lvc_amd.evaluation's pipelines call to repeat a batch)."""
        assert not self.training
        if detected_instances is not None or not do_postprocess:
            raise NotImplementedError("RetinaNet.inference: detected_instances / do_postprocess=False are not built")
        return self.forward(batched_inputs)

    def head_outputs(self, feats):
        return self.head.forward_nhwc([feats[f] for f in self.in_features])

    def select_nms_post(self, logits, deltas, post, status=None, return_rows=False):
        """The head's per-level outputs -> (boxes [B,D,4], scores [B,D], classes [B,D] int32, count [B] int32, status): selection,
        class-wise NMS, the first D = DETECTIONS_PER_IMAGE kept rows through detector_postprocess (post [B,4] or None).  No sync.
        return_rows: two more values -- for every detection its row in the image's candidate list [B,D] int32, and the candidates' flat
        indices inside their level [B,L*topk] int32 (rows of a level follow those of the levels below it)."""
        A, Kc = self.head.num_anchors, self.num_classes
        ag = self.anchor_generator
        boxes, scores, classes, index, count, status = K.retinanet_select(
            [t[..., :A * Kc] for t in logits], [t[..., :4 * A] for t in deltas], list(ag.cell_anchors), ag.strides, ag.offset, Kc,
            self.topk_candidates, self.score_threshold, self.box2box_transform.weights, max_survivors=self.max_survivors, status=status)
        D = self.max_detections_per_image
        keep, num_keep = K.batched_nms_batch(boxes, scores, classes, count, self.nms_threshold, max_keep=D)
        if return_rows:
            pos = torch.arange(scores.shape[1], device=scores.device, dtype=torch.int32).repeat(scores.shape[0], 1)
            ob, osc, ocl, rows, cnt = K.gather_detections(boxes, scores, classes, pos, keep, num_keep, D, post=post)
            return ob, osc, ocl, cnt, status, rows, index
        ob, osc, ocl, _rows, cnt = K.gather_detections(boxes, scores, classes, index, keep, num_keep, D, post=post)
        return ob, osc, ocl, cnt, status

    def _out_sizes(self, batched_inputs, sizes, do_postprocess=True):
        out = []
        for inp, (h, w) in zip(batched_inputs, sizes):
            dh, dw = (int(inp["raw"].shape[0]), int(inp["raw"].shape[1])) if ("image" not in inp and "raw" in inp) else (h, w)
            out.append((inp.get("height", dh), inp.get("width", dw)) if do_postprocess else (h, w))
        return out

    def inference_batched(self, batched_inputs, do_postprocess=True, status=None):
        """Whole forward with device-resident, fixed-shape outputs and no host sync, in the form of GeneralizedRCNN.inference_batched:
        (boxes [B,D,4], scores [B,D], classes [B,D] int32, count [B] int32, status [1] int32), D = TEST.DETECTIONS_PER_IMAGE."""
        with torch.no_grad():
            x4, sizes = self.preprocess_nhwc(batched_inputs)
            post = None
            if do_postprocess:
                outs = self._out_sizes(batched_inputs, sizes)
                post = self._dev_const([[ow / w, oh / h, float(oh), float(ow)] for (oh, ow), (h, w) in zip(outs, sizes)], torch.float32)
            feats = self.backbone.forward_nhwc(x4)
            logits, deltas = self.head_outputs(feats)
            return self.select_nms_post(logits, deltas, post, status)

    def _inference(self, batched_inputs):
        ob, osc, ocl, cnt, status = self.inference_batched(batched_inputs)
        sizes = []
        for inp in batched_inputs:
            if "image" in inp:
                sizes.append((int(inp["image"].shape[-2]), int(inp["image"].shape[-1])))
            else:      # raw file pixels: the network saw the ResizeShortestEdge size
                t = self._test_resize.get_transform(inp["raw"])
                sizes.append((t.new_h, t.new_w) if t is not None else (int(inp["raw"].shape[0]), int(inp["raw"].shape[1])))
        insts = instances_from_batched(ob, osc, ocl, cnt, self._out_sizes(batched_inputs, sizes), status)      # the ONE read: counts, status, range words
        return [{"instances": r} for r in insts]
