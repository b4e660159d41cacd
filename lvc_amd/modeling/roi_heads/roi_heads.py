"""ROI heads: `ROIHeads` base + `StandardROIHeads` (reference lvc/modeling/roi_heads/roi_heads.py:
28, 90-306, 483-629).  Sub-module names `box_pooler`, `box_head`, `box_predictor` as in the reference.

Inference launch plan for B images x R proposals (all on device, fixed shapes, no host sync):
  assign levels + build rois (1 launch) -> ROIAlign over all levels (1 launch, output [B*R,7,7,C])
  -> fc1/fc2 MFMA GEMMs with fused bias+ReLU -> fused cls|bbox GEMM -> lvc_fast_rcnn_inference.
"""
import torch
from torch import nn

from ... import kernels as K
from ...layers import ShapeSpec
from ...layers.layout import require_device, to_nhwc
from ...structures import Boxes, Instances
from ...utils.events import get_event_storage
from ...utils.registry import Registry
from ..box_regression import Box2BoxTransform
from ..matcher import Matcher
from ..sampling import subsample_labels
from ..poolers import ROIPooler
from .box_head import build_box_head
from .fast_rcnn import ROI_HEADS_OUTPUT_REGISTRY
from .keypoint_head import TRAIN_REFUSAL as KEYPOINT_TRAIN_REFUSAL
from .keypoint_head import build_keypoint_head, keypoint_rcnn_inference
from .mask_head import build_mask_head, mask_rcnn_inference

ROI_HEADS_REGISTRY = Registry("ROI_HEADS")


def build_roi_heads(cfg, input_shape):
    if cfg.MODEL.KEYPOINT_ON and cfg.MODEL.ROI_HEADS.NAME != "StandardROIHeads":
        raise NotImplementedError("MODEL.KEYPOINT_ON with MODEL.ROI_HEADS.NAME = {!r}: the keypoint branch is built for StandardROIHeads"
                                  .format(cfg.MODEL.ROI_HEADS.NAME))
    return ROI_HEADS_REGISTRY.get(cfg.MODEL.ROI_HEADS.NAME)(cfg, input_shape)


def padded_boxes(instances, field, device):
    """The Boxes `field` of every Instances in one zero-padded table on `device` -> (boxes [B, R, 4] with R the largest count (at
    least 1), counts: the B lengths)."""
    counts = [len(p) for p in instances]
    boxes = torch.zeros(len(instances), max(max(counts), 1), 4, device=device)
    for i, p in enumerate(instances):
        boxes[i, : counts[i]] = p.get(field).tensor
    return boxes, counts


def front_rows(boxes, count, pooler, num_levels):
    """The rows of a padded [B, T] box table with the real ones (the first count[b] of image b) moved to the front, image after image,
    for a branch that runs on ONE number of valid rows -> (rois [B*T, 5], levels [B*T] int32 (None with one level), rows [B, T] int32:
    the row box i of image b owns, total [1] int32: the number of real rows, order [B*T] int64: the permutation, for whatever else the
    caller keeps per row).  pooler: the branch's pooler, whose level rule assigns the rows.  Nothing is read back."""
    B, T, _ = boxes.shape
    ar = torch.arange(T, device=boxes.device, dtype=torch.int32)
    cnt = count.clamp(min=0, max=T)
    valid = ar[None, :] < cnt[:, None]
    start = torch.cumsum(cnt, 0, dtype=torch.int32) - cnt
    rows = (start[:, None] + ar[None, :]).contiguous()
    total = cnt.sum(dtype=torch.int32).view(1)
    # stable: the real rows first, in (image, index) order -- row start_b + i is box i of image b
    order = torch.argsort((~valid).view(-1).to(torch.uint8), stable=True)
    # rows past an image's count hold whatever the box branch left there: zero boxes instead (empty sampling grids)
    boxes = torch.where(valid[:, :, None], boxes, torch.zeros_like(boxes))
    levels, rois = K.assign_levels_rois(boxes, pooler.min_level, pooler.max_level, pooler.canonical_box_size, pooler.canonical_level)
    rois = rois.index_select(0, order)
    levels = None if num_levels == 1 else levels.index_select(0, order)
    return rois, levels, rows, total, order


def _log_sample_counts(counts):
    """The two roi_head/num_*_samples scalars of label_and_sample_proposals from per-image (fg, bg) host counts."""
    storage = get_event_storage()
    n = max(1, len(counts))
    storage.put_scalar("roi_head/num_fg_samples", sum(c[0] for c in counts) / n)
    storage.put_scalar("roi_head/num_bg_samples", sum(c[1] for c in counts) / n)


def _log_box_accuracy(stats, nrows):
    """The three fast_rcnn/* scalars (reference fast_rcnn.py _log_accuracy) from the four host counts of `_box_stats`."""
    nfg, ncorrect, nfg_correct, nfg_bg = stats
    storage = get_event_storage()
    storage.put_scalar("fast_rcnn/cls_accuracy", float(ncorrect) / max(1, nrows))
    if nfg > 0:
        storage.put_scalar("fast_rcnn/fg_cls_accuracy", float(nfg_correct) / nfg)
        storage.put_scalar("fast_rcnn/false_negative", float(nfg_bg) / nfg)


class ROIHeads(nn.Module):
    def __init__(self, cfg, input_shape):
        super().__init__()
        RH, BH = cfg.MODEL.ROI_HEADS, cfg.MODEL.ROI_BOX_HEAD
        self.batch_size_per_image = RH.BATCH_SIZE_PER_IMAGE
        self.positive_sample_fraction = RH.POSITIVE_FRACTION
        self.test_score_thresh = RH.SCORE_THRESH_TEST
        self.test_nms_thresh = RH.NMS_THRESH_TEST
        self.test_detections_per_img = cfg.TEST.DETECTIONS_PER_IMAGE
        self.in_features = RH.IN_FEATURES
        self.num_classes = RH.NUM_CLASSES
        self.proposal_append_gt = RH.PROPOSAL_APPEND_GT
        self.feature_strides = {k: v.stride for k, v in input_shape.items()}
        self.feature_channels = {k: v.channels for k, v in input_shape.items()}
        self.cls_agnostic_bbox_reg = BH.CLS_AGNOSTIC_BBOX_REG
        self.smooth_l1_beta = BH.SMOOTH_L1_BETA
        self.box_reg_loss_type = BH.BBOX_REG_LOSS_TYPE
        self.loss_weight = {"loss_box_reg": BH.BBOX_REG_LOSS_WEIGHT}
        self.ignore_reg = RH.IGNORE_REG
        self.iou_thresholds, self.iou_labels = RH.IOU_THRESHOLDS, RH.IOU_LABELS
        self.box2box_transform = Box2BoxTransform(weights=BH.BBOX_REG_WEIGHTS)
        self.proposal_matcher = Matcher(RH.IOU_THRESHOLDS, RH.IOU_LABELS, allow_low_quality_matches=False)

    def _sample_proposals(self, matched_idxs, matched_labels, gt_classes, inference=False):
        """reference lvc roi_heads.py:129-171."""
        if gt_classes.numel() > 0:
            gt_classes = gt_classes[matched_idxs]
            gt_classes[matched_labels == 0] = self.num_classes
            gt_classes[matched_labels == -1] = -1
        else:
            gt_classes = torch.zeros_like(matched_idxs) + self.num_classes
        fg, bg = subsample_labels(gt_classes, self.batch_size_per_image, self.positive_sample_fraction, self.num_classes,
                                  inference)
        sampled = torch.cat([fg, bg], dim=0)
        return sampled, gt_classes[sampled]

    relabel_ignored_gt = True

    def _keeps_index(self, val):
        """A mask model's sampled rows do not carry gathered full-size ground-truth planes (the reference's gt_masks[matched_idxs]:
        512 x H x W bytes per image): the mask targets are cut from the image's planes through the matched INDEX of a row (the python
        attribute `_lvc_matched` / the sampler's table).  A box-only model keeps exactly the fields it had."""
        from ...structures import BitMasks

        return bool(getattr(self, "mask_on", False)) and isinstance(val, BitMasks)

    batched_sampling = True     # class switch for A/B runs and tests (False: the per-image loop in every case)

    batched_targets = True      # class switch for A/B runs and tests (False: the padded table built image by image with torch ops)

    @torch.no_grad()
    def label_and_sample_proposals(self, proposals, targets, inference=False, log=None):
        """reference lvc roi_heads.py:173-278: append GT, match (IoU kernel), gt_ignores toggle, subsample.
        `log` (default: not inference) controls only the EventStorage scalars: CascadeROIHeads inherits detectron2's
        label_and_sample_proposals, whose evaluation call still subsamples and merely skips the logging."""
        if (self.batched_sampling and not inference and self.proposal_append_gt and len(proposals) > 0
                and all(len(t) > 0 and not (self.relabel_ignored_gt and t.has("gt_ignores")) for t in targets)
                and all(p.proposal_boxes.tensor.is_cuda for p in proposals)):
            return self._label_and_sample_batched(proposals, targets, (not inference) if log is None else log)
        return self._label_and_sample_loop(proposals, targets, inference, log)

    def _label_and_sample_batched(self, proposals, targets, log):
        """The training case of the loop below for the whole batch with ONE device->host read (the per-image loop reads the device
        ~5 times per image: `nonzero`, the fg / bg counts): labels of all images in one padded [B, W] table, the fg / bg subsets
        drawn by ranking ONE random permutation of B*W keys within each row (any subset of a random permutation is in uniformly
        random order, so this is `positive[randperm(n)[:num_pos]]` in distribution; with `torch.randperm` patched to arange
        -- the parity tests -- it is the reference's selection exactly: the first num_pos positives, the first num_neg
        negatives, fg before bg).  Needs: training, PROPOSAL_APPEND_GT, every image with at least one gt box and (for lvc's own
        ROIHeads, which relabel proposals on ignored gt boxes) no gt_ignores field."""
        import math

        B, dev = len(proposals), proposals[0].proposal_boxes.tensor.device
        K_, bs = self.num_classes, self.batch_size_per_image
        gt_logit = math.log((1.0 - 1e-10) / (1 - (1.0 - 1e-10)))
        batch = getattr(proposals[0], "_lvc_batch", None)
        if (batch is not None and self.batched_targets and bs <= 1024 and all(len(t) <= 512 for t in targets)
                and len(self.proposal_matcher.user_thresholds) in (1, 2) and len(batch[3]) == B):
            # the proposals as RPN.forward made them -- one padded [B,P] table on the device -- and the concatenated ground truth: table
            # + Matcher + subsample_labels + gather for the whole batch in five launches (csrc/train_targets.hip), ONE device->host read
            pboxes, plogits, pcount, pcounts_host, gt, gt_off = batch
            s_boxes, s_logits, s_cls, s_m, s_gtb, cnt = self._sample_batched(pboxes, plogits, pcount, gt, gt_off, targets)
            counts = cnt.tolist()      # the one device->host read
            out = self._sampled_instances(proposals, targets, counts, s_boxes, s_logits, s_cls, s_m, s_gtb)
            # for _forward_train: the same rows as padded batch tensors (a python attribute, not a field); the matched gt index and the
            # device counts for the mask branch
            out[0]._lvc_sampled = (s_boxes, s_cls, s_gtb, [c[0] + c[1] for c in counts], s_m, cnt)
            if log:
                _log_sample_counts(counts)
            return out
        ns = [len(p) + len(t) for p, t in zip(proposals, targets)]
        W = max(max(ns), bs)
        boxes = torch.zeros(B, W, 4, device=dev)
        logits = torch.zeros(B, W, device=dev)
        labels = torch.full((B, W), -1, dtype=torch.int64, device=dev)     # -1: ignored / padding
        midx = torch.zeros(B, W, dtype=torch.int64, device=dev)
        for i, (prop, tgt) in enumerate(zip(proposals, targets)):
            gt, n, npr = tgt.gt_boxes.tensor, ns[i], len(prop)
            boxes[i, :npr] = prop.proposal_boxes.tensor
            boxes[i, npr:n] = gt
            logits[i, :npr] = prop.objectness_logits
            logits[i, npr:n] = gt_logit
            m, l = self.proposal_matcher.match(gt, boxes[i, :n])
            gc = tgt.gt_classes.to(torch.int64)[m]
            labels[i, :n] = torch.where(l == 0, torch.full_like(gc, K_), torch.where(l == -1, torch.full_like(gc, -1), gc))
            midx[i, :n] = m
        key = torch.randperm(B * W, device=dev).view(B, W)
        fg = (labels >= 0) & (labels != K_)
        bg = labels == K_
        big = B * W
        sf = torch.argsort(torch.where(fg, key, torch.full_like(key, big)), dim=1)
        sb = torch.argsort(torch.where(bg, key, torch.full_like(key, big)), dim=1)
        npos = fg.sum(1).clamp(max=int(bs * self.positive_sample_fraction))
        nneg = torch.minimum(bg.sum(1), bs - npos)
        j = torch.arange(bs, device=dev)[None, :]
        sampled = torch.where(j < npos[:, None], sf[:, :bs], torch.gather(sb, 1, (j - npos[:, None]).clamp(0, W - 1)))
        s_boxes = torch.gather(boxes, 1, sampled[:, :, None].expand(B, bs, 4))
        s_logits = torch.gather(logits, 1, sampled)
        s_cls = torch.gather(labels, 1, sampled)
        s_m = torch.gather(midx, 1, sampled)
        counts = torch.stack([npos, nneg], 1).tolist()      # the one device->host read
        if log:
            _log_sample_counts(counts)
        return self._sampled_instances(proposals, targets, counts, s_boxes, s_logits, s_cls, s_m)

    def _sampled_instances(self, proposals, targets, counts, s_boxes, s_logits, s_cls, s_m, s_gtb=None):
        """Per-image Instances from the sampled rows of the padded [B, bs] tables: the first fg + bg of image i (counts[i]), with the
        image's other gt_* fields gathered through the matched index s_m (gt_boxes too where the sampler did not hand them over)."""
        out = []
        for i, (prop, tgt) in enumerate(zip(proposals, targets)):
            c = counts[i][0] + counts[i][1]
            inst = Instances(prop.image_size)
            inst.proposal_boxes = Boxes(s_boxes[i, :c])
            inst.objectness_logits = s_logits[i, :c]
            inst.gt_classes = s_cls[i, :c]
            if s_gtb is not None:
                inst.gt_boxes = Boxes(s_gtb[i, :c])
            st = s_m[i, :c]
            for name, val in tgt.get_fields().items():
                if name.startswith("gt_") and not inst.has(name) and not self._keeps_index(val):
                    inst.set(name, val[st])
            inst._lvc_matched = st
            out.append(inst)
        return out

    def _sample_batched(self, pboxes, plogits, pcount, gt, gt_off, targets):
        """Table + Matcher + subsample_labels + gather for the whole batch (csrc/train_targets.hip), nothing read back:
        -> (boxes [B,bs,4], logits [B,bs], classes int64 [B,bs], matched gt index int64 [B,bs], matched gt boxes [B,bs,4], counts int32 [B,2])."""
        import math

        B, dev = pboxes.shape[0], pboxes.device
        K_, bs = self.num_classes, self.batch_size_per_image
        gt_logit = math.log((1.0 - 1e-10) / (1 - (1.0 - 1e-10)))
        Wt = pboxes.shape[1] + max(len(t) for t in targets)
        with torch.no_grad():
            tb, tl, nrow = K.roi_build_table(pboxes, plogits, pcount, gt, gt_off, gt_logit, Wt)
            m, lab = K.match_boxes_batched(gt, gt_off, B, tb, nrow, self.proposal_matcher.user_thresholds, self.proposal_matcher.labels,
                                           self.proposal_matcher.allow_low_quality_matches)
            key, seed = K.sampling_keys(B, Wt, dev)
            sel, cnt = K.subsample_batched(lab, key, int(bs * self.positive_sample_fraction), bs, seed=seed)
            gcls = torch.cat([t.gt_classes for t in targets]).to(torch.int64)
            s_boxes, s_logits, s_cls, s_m = K.roi_gather_sampled(tb, tl, m, sel, cnt, gcls, gt_off, K_)
            s_gtb = gt[(gt_off[:-1].long()[:, None] + s_m).clamp(max=max(gt.shape[0] - 1, 0)).view(-1)].view(B, bs, 4)
        return s_boxes, s_logits, s_cls, s_m, s_gtb, cnt

    def _label_and_sample_loop(self, proposals, targets, inference=False, log=None):
        out, num_fg, num_bg = [], [], []
        for prop, tgt in zip(proposals, targets):
            gt = tgt.gt_boxes.tensor
            pboxes, plogits = prop.proposal_boxes.tensor, prop.objectness_logits
            if self.proposal_append_gt:  # add_ground_truth_to_proposals: logit = log((1-1e-10)/(1-(1-1e-10)))
                import math

                gt_logit = math.log((1.0 - 1e-10) / (1 - (1.0 - 1e-10)))
                pboxes = torch.cat([pboxes, gt], 0)
                plogits = torch.cat([plogits, gt_logit * torch.ones(len(gt), device=gt.device)], 0)
            matched_idxs, matched_labels = self.proposal_matcher.match(gt, pboxes)
            # lvc's ROIHeads only (roi_heads.py:222-228); CascadeROIHeads derives from detectron2's StandardROIHeads,
            # whose label_and_sample_proposals (detectron2/modeling/roi_heads/roi_heads.py:220-306) has no such toggle
            if self.relabel_ignored_gt and tgt.has("gt_ignores") and bool(tgt.gt_ignores.bool().sum()):
                from ...structures import pairwise_iou

                ig = tgt.gt_ignores.bool()
                max_ig = pairwise_iou(Boxes(gt[ig]), Boxes(pboxes)).max(dim=0)[0]
                matched_labels[max_ig > self.proposal_matcher.thresholds[1]] = -1
            sampled, gt_classes = self._sample_proposals(matched_idxs, matched_labels, tgt.gt_classes, inference)
            if self.proposal_append_gt:
                inst = Instances(prop.image_size)
                inst.proposal_boxes = Boxes(pboxes[sampled])
                inst.objectness_logits = plogits[sampled]
            else:   # reference: proposals_per_image[sampled_idxs] -- every field the proposals carry is kept
                inst = prop[sampled]
            inst.gt_classes = gt_classes
            if len(gt) > 0:
                st = matched_idxs[sampled]
                for name, val in tgt.get_fields().items():
                    if name.startswith("gt_") and not inst.has(name) and not self._keeps_index(val):
                        inst.set(name, val[st])
                inst._lvc_matched = st
            else:
                inst.gt_boxes = Boxes(gt.new_zeros((len(sampled), 4)))
            num_bg.append(int((gt_classes == self.num_classes).sum()))
            num_fg.append(gt_classes.numel() - num_bg[-1])
            out.append(inst)
        if (not inference) if log is None else log:
            _log_sample_counts(list(zip(num_fg, num_bg)))
        return out


@ROI_HEADS_REGISTRY.register()
class StandardROIHeads(ROIHeads):
    # capacity of the per-image (roi, class) candidate list of fast_rcnn_inference; None = R*K.  16 384 keeps the
    # detection-stage NMS in its one-block form; `run_with_fallbacks` switches to None after the first overflow
    det_max_candidates = 16384
    keypoint_on = False         # (a subclass that builds its own heads has no keypoint branch)

    def __init__(self, cfg, input_shape):
        super().__init__(cfg, input_shape)
        self._init_branch(cfg, cfg.MODEL.ROI_BOX_HEAD, "box", build_box_head)
        self.box_predictor = ROI_HEADS_OUTPUT_REGISTRY.get(cfg.MODEL.ROI_HEADS.OUTPUT_LAYER)(cfg, self.box_head.output_size)
        self.mask_on = bool(cfg.MODEL.MASK_ON)
        if self.mask_on:
            self._init_branch(cfg, cfg.MODEL.ROI_MASK_HEAD, "mask", build_mask_head)
        self.keypoint_on = bool(cfg.MODEL.KEYPOINT_ON)
        if self.keypoint_on:
            if self.mask_on:
                raise NotImplementedError("MODEL.KEYPOINT_ON together with MODEL.MASK_ON: keypoints and masks in one model are not built")
            self._init_branch(cfg, cfg.MODEL.ROI_KEYPOINT_HEAD, "keypoint", build_keypoint_head)
        if cfg.DEBUG:
            raise NotImplementedError("cfg.DEBUG heads (FastRCNNOutputsDebug) are not part of the hot path")
        if cfg.MODEL.META_ARCHITECTURE == "GeneralizedRCNN_Context":
            raise NotImplementedError("GeneralizedRCNN_Context is unused by every shipped config")
        self.rbg = cfg.MODEL.PROPOSAL_GENERATOR.NAME == "RBG"
        self.reg_off = cfg.MODEL.ROI_HEADS.REG_OFF

    def _init_branch(self, cfg, node, name, build_head):
        """`<name>_pooler` + `<name>_head` over ROI_HEADS.IN_FEATURES (`<name>_in_features`) from the branch's config node, registered
        in that order: detectron2's StandardROIHeads._init_box_head / _init_mask_head / _init_keypoint_head (roi_heads.py:560-647)."""
        res = node.POOLER_RESOLUTION
        scales = tuple(1.0 / self.feature_strides[k] for k in self.in_features)
        in_channels = [self.feature_channels[f] for f in self.in_features]
        assert len(set(in_channels)) == 1, in_channels
        setattr(self, name + "_in_features", self.in_features)
        setattr(self, name + "_pooler", ROIPooler(output_size=res, scales=scales, sampling_ratio=node.POOLER_SAMPLING_RATIO,
                                                  pooler_type=node.POOLER_TYPE))
        setattr(self, name + "_head", build_head(cfg, ShapeSpec(channels=in_channels[0], height=res, width=res)))

    def _pool_branch(self, name, feats_nhwc, boxes, count, status=None):
        """The input of the mask or keypoint branch on padded batch tensors, nothing read back: the branch's feature maps, the real rows
        of the [B, topk] table moved to the front (`front_rows`), and all B*topk rows through ROIAlign over the pyramid with the
        branch's pooler (the vectorised NHWC kernel `roi_align_fwd_nhwc4_kernel`, which takes no row count: a zero box costs it a
        store of zeros).  -> (pooled [B*topk, S, S, C], rois [B*topk, 5], rows [B, topk] int32, total [1] int32, order [B*topk] int64)."""
        pl = getattr(self, name + "_pooler")
        feats = [feats_nhwc[f] for f in getattr(self, name + "_in_features")]
        rois, levels, rows, total, order = front_rows(boxes, count, pl, len(feats))
        pooled = K.roi_align_fpn_nhwc(feats, pl.scales, rois, levels, pl.output_size[0], pl.output_size[1], pl.sampling_ratio, pl.aligned,
                                      status=status)
        return pooled, rois, rows, total, order

    def pool_masks_batched(self, feats_nhwc, boxes, classes, count, status=None):
        """The mask branch's input (`_pool_branch`) and the classes in the order of its rows -> (pooled [B*topk, S, S, C], classes
        [B*topk] int32, rows [B, topk] int32: the row box i of image b owns, total [1] int32: the number of real rows)."""
        pooled, _rois, rows, total, order = self._pool_branch("mask", feats_nhwc, boxes, count, status=status)
        return pooled, classes.reshape(-1).index_select(0, order).contiguous(), rows, total

    def _branch_loss_batched(self, name, feats_nhwc, s_boxes, s_cls, s_m, fg_count, gt, status):
        """The training loss of the mask or keypoint branch `name` on the sampler's padded tables, with no device->host read (reference
        roi_heads.py `_forward_mask` / `_forward_keypoint` + `select_foreground_proposals` + the branch's loss).  s_boxes [B, R, 4], s_cls
        [B, R], s_m [B, R] int64 (the matched gt index of every sampled row), fg_count [B] int32 on the device: foreground comes before
        background in the sampled table, so the foreground rows of image b are its first fg_count[b], at most
        int(BATCH_SIZE_PER_IMAGE * POSITIVE_FRACTION); gt: one BitMasks / Keypoints per image.  One launch makes the targets (the head's
        `train_targets`; a foreground row the reference's keypoint selection would drop keeps its place and contributes nothing), the
        foreground rows move to the front (`front_rows`), the branch's pooler and convs run under autograd on ALL padded rows (zero
        boxes), and the total of foreground rows is the `num_valid` of tail, loss and backward (the head's `train_loss`).
        -> (loss scalar, the branch's counts: "<name>.<count>" -> device tensor, in the order they are packed; the last is the status word)."""
        if not getattr(self, name + "_on"):
            raise RuntimeError("{}_loss_batched: the model was built with MODEL.{}_ON = False".format(name, name.upper()))
        head, pooler = getattr(self, name + "_head"), getattr(self, name + "_pooler")
        cap = max(int(self.batch_size_per_image * self.positive_sample_fraction), 1)
        R = min(cap, s_boxes.shape[1])
        boxes = s_boxes[:, :R].detach().contiguous()
        matched = s_m[:, :R].to(torch.int64).contiguous()
        count = fg_count.to(torch.int32).clamp(min=0, max=R)
        rows, target_counts = head.train_targets(boxes, matched, count, gt, head.map_scale * pooler.output_size[0])
        feats = [feats_nhwc[f] for f in getattr(self, name + "_in_features")]
        rois, levels, _rows, total, order = front_rows(boxes, count, pooler, len(feats))
        if head.loss_takes_classes:
            rows = (s_cls[:, :R].to(torch.int32).reshape(-1),) + rows
        rows = [t.index_select(0, order) for t in rows]
        pooled = pooler.pool_rois_nhwc(feats, rois, levels, num_valid=total, status=status)
        loss, counts = head.train_loss(pooled, rows, total, status, s_boxes.shape[0])
        return loss, {name + "." + k: v for k, v in dict(counts, **target_counts, status=status).items()}

    def forward_masks_batched(self, feats_nhwc, boxes, classes, count, status=None):
        """The mask branch on padded batch tensors, nothing read back.  feats_nhwc: dict name -> [B,H,W,C]; boxes [B,topk,4] in network
        coordinates; classes [B,topk] int32; count [B] int32 (rows [0, count_b) of image b are real).
        Returns (prob [B*topk, 2S, 2S], rows [B,topk] int32): `pool_masks_batched` moves the real rows to the front, so that ONE
        number -- their total -- is the `num_valid` of the tail kernel; `rows[b, i]` is the row of `prob` that box i of image b owns.
        Rows of `prob` past the total are not written (ROIAlign and the convs run on all rows: zero boxes, zero maps)."""
        if not self.mask_on:
            raise RuntimeError("forward_masks_batched: the model was built with MODEL.MASK_ON = False")
        pooled, cls, rows, total = self.pool_masks_batched(feats_nhwc, boxes, classes, count, status=status)
        prob = self.mask_head.forward_nhwc(pooled, cls, num_valid=total, status=status)
        return prob, rows

    def forward_keypoints_batched(self, feats_nhwc, boxes, count, status=None):
        """The keypoint branch on padded batch tensors, nothing read back.  feats_nhwc: dict name -> [B,H,W,C]; boxes [B,topk,4] in
        network coordinates; count [B] int32 (rows [0, count_b) of image b are real).
        Returns (keypoints [B*topk, K, 4] = (x, y, logit, score) in network coordinates, rows [B,topk] int32): the real rows are moved
        to the front exactly as `pool_masks_batched` moves them (`front_rows`), so that ONE number -- their total -- is the `num_valid`
        of `score_lowres` and the decode; `rows[b, i]` is the row box i of image b owns.  Rows past the total are zero (ROIAlign and
        the convs run on all rows: zero boxes, zero maps)."""
        if not self.keypoint_on:
            raise RuntimeError("forward_keypoints_batched: the model was built with MODEL.KEYPOINT_ON = False")
        pooled, rois, rows, total, _order = self._pool_branch("keypoint", feats_nhwc, boxes, count, status=status)
        kp = self.keypoint_head.forward_nhwc(pooled, rois[:, 1:5].contiguous(), num_valid=total, status=status)
        return kp, rows

    def forward_with_given_boxes(self, features, instances):
        """Reference signature (detectron2 roi_heads.py:681-706): `instances` carry `pred_boxes` and `pred_classes` (network
        coordinates) and get `pred_masks` [n, 1, 2S, 2S], the predicted class's mask probabilities (a mask model), or
        `pred_keypoints` [n, K, 3] = (x, y, score) in network coordinates (a keypoint model)."""
        assert not self.training
        assert instances[0].has("pred_boxes") and instances[0].has("pred_classes")
        if not self._branches():
            return instances
        name = self._branches()[-1]
        in_features = getattr(self, name + "_in_features")
        feats = {f: to_nhwc(features[f]) for f in in_features}
        dev = feats[in_features[0]].device
        require_device(feats[in_features[0]], "StandardROIHeads")
        boxes, counts = padded_boxes(instances, "pred_boxes", dev)
        if name == "mask":
            classes = torch.zeros(boxes.shape[:2], dtype=torch.int32, device=dev)
            for i, p in enumerate(instances):
                classes[i, : counts[i]] = p.pred_classes.to(torch.int32)
        status = K.new_status(dev)
        count = torch.tensor(counts, dtype=torch.int32, device=dev)
        if name == "mask":
            out, _rows = self.forward_masks_batched(feats, boxes, classes, count, status=status)
        else:
            out, _rows = self.forward_keypoints_batched(feats, boxes, count, status=status)
        check_status(int(status.item()))
        (mask_rcnn_inference if name == "mask" else keypoint_rcnn_inference)(out, instances)
        return instances

    def forward_batched(self, feats_nhwc, prop_boxes, prop_count, image_sizes_dev, post=None, status=None):
        """feats_nhwc: dict name -> [B,H,W,C]; prop_boxes [B,R,4]; prop_count [B] int32 or None.
        Returns (boxes [B,topk,4], scores, classes int32, rows int32, count [B] int32), all on device."""
        if self.reg_off:
            raise NotImplementedError("ROI_HEADS.REG_OFF is not used by the shipped configs")
        feats = [feats_nhwc[f] for f in self.in_features]
        pooled = self.box_pooler.pool_nhwc(feats, prop_boxes, status=status)
        h = self.box_head.forward_nhwc(pooled)
        scores, deltas = self.box_predictor(h)
        return K.fast_rcnn_inference(scores, deltas, prop_boxes, prop_count, image_sizes_dev, self.num_classes,
                                     self.box2box_transform.weights, self.test_score_thresh, self.test_nms_thresh,
                                     self.test_detections_per_img, post=post, status=status,
                                     max_candidates=self.det_max_candidates)

    def forward(self, images, features, proposals, targets=None):
        """Reference signature (roi_heads.py:554-572): -> (list[Instances], losses)."""
        if self.training:
            if self.mask_on and not self.__dict__.get("_mask_train_enabled", False):
                raise NotImplementedError("training the mask branch (MODEL.MASK_ON: mask_rcnn_loss, gt_masks) is not built")
            if self.keypoint_on and not self.__dict__.get("_keypoint_train_enabled", False):
                raise NotImplementedError(KEYPOINT_TRAIN_REFUSAL)
            return self._forward_train(features, proposals, targets)
        if self.rbg:
            # reference roi_heads.py:561-562: with an RBG proposal generator the evaluation pass labels and subsamples the given
            # proposals against the ground truth first (inference=True: no EventStorage scalars), then runs the usual box branch
            proposals = self.label_and_sample_proposals(proposals, targets, inference=True)
        feats = {f: to_nhwc(features[f]) for f in self.in_features}
        dev = feats[self.in_features[0]].device
        require_device(feats[self.in_features[0]], "StandardROIHeads")
        boxes, counts = padded_boxes(proposals, "proposal_boxes", dev)
        sizes = torch.tensor([list(p.image_size) for p in proposals], dtype=torch.int32, device=dev)
        status = K.new_status(dev)
        ob, osc, ocl, orow, cnt = self.forward_batched(feats, boxes, torch.tensor(counts, dtype=torch.int32, device=dev),
                                                       sizes, status=status)
        prob = rows = kp = None
        if self.mask_on:
            prob, rows = self.forward_masks_batched(feats, ob, ocl, cnt, status=status)
        if self.keypoint_on:
            kp, rows = self.forward_keypoints_batched(feats, ob, cnt, status=status)
        insts = instances_from_batched(ob, osc, ocl, cnt, [p.image_size for p in proposals], status)
        if prob is not None:
            mask_rcnn_inference(prob, insts)      # the real rows lie image after image at the front of prob
        if kp is not None:
            keypoint_rcnn_inference(kp, insts)
        return insts, {}

    def can_batch_train(self, targets):
        return (self.batched_sampling and self.batched_targets and self.proposal_append_gt and not self.rbg and self.batch_size_per_image <= 1024
                and type(self)._forward_train is StandardROIHeads._forward_train and targets is not None and len(targets) > 0
                and all(0 < len(t) <= 512 and not (self.relabel_ignored_gt and t.has("gt_ignores")) for t in targets)
                and len(self.proposal_matcher.user_thresholds) in (1, 2))

    def _box_stats(self, pred, gc):
        """The four counts of FastRCNNOutputs._log_accuracy as one int64 [4] device tensor: foreground rows, correct rows, correct
        foreground rows, foreground rows predicted as background."""
        fg = (gc >= 0) & (gc < self.num_classes)
        hit = pred == gc
        return torch.stack([fg.sum(), hit.sum(), (hit & fg).sum(), ((pred == self.num_classes) & fg).sum()])

    def forward_train_batched(self, features, pboxes, plogits, pcount, gt, gt_off, targets):
        """StandardROIHeads' training branch on the proposal generator's batch tensors, without a device->host read: the sampled rows stay
        one padded [B, bs] table, ROIAlign / box head / losses run on all B * bs rows as if every image had filled its quota (the usual case;
        padding rows are zero boxes labelled background) and -> (losses, counts int32 [B,2], the step's counts as `pack_step_counts` made
        them: (int64 vector, layout)).  The CALLER reads the counts with the step's other scalars and, if some image did fall short of bs
        rows, discards these losses and runs the per-image path (`forward`) instead -- the reference's normalisation is by the true row count.
        Packed: `box`, the four accuracy counts; then for a mask model `mask.pixels` (the loss kernel's incorrect, positive and
        false-positive pixels), `mask.rows` and `mask.status`; for a keypoint model `keypoint.valid`, `keypoint.selected` and
        `keypoint.fg` (the selected and the foreground rows of every image) and `keypoint.status`."""
        from .fast_rcnn import fast_rcnn_losses

        s_boxes, _s_logits, s_cls, s_m, s_gtb, cnt = self._sample_batched(pboxes, plogits, pcount, gt, gt_off, targets)
        feats = [to_nhwc(features[f]) for f in self.in_features]
        below = any(f.requires_grad for f in feats) or any(p.requires_grad for p in self.box_head.parameters())
        with torch.set_grad_enabled(below and torch.is_grad_enabled()):
            h = self.box_head.forward_nhwc(self.box_pooler.pool_nhwc(feats, s_boxes))
        gc = s_cls.view(-1)
        losses, pred = fast_rcnn_losses(self.box_predictor, h, s_boxes.view(-1, 4), s_gtb.view(-1, 4), gc)
        with torch.no_grad():
            stats = self._box_stats(pred, gc)
        parts = {"box": stats}
        for name in self._branches():
            bfeats = {f: to_nhwc(features[f]) for f in getattr(self, name + "_in_features")}
            loss, counts = self._branch_loss_batched(name, bfeats, s_boxes, s_cls, s_m, cnt[:, 0], self._gt_of(name, targets),
                                                     K.new_status(s_boxes.device))
            losses = dict(losses)
            losses["loss_" + name] = loss
            parts.update(counts)
        with torch.no_grad():
            return losses, cnt, pack_step_counts(parts)

    def _branches(self):
        """The enabled branches behind the box branch, in the order they run."""
        return [name for name in ("mask", "keypoint") if getattr(self, name + "_on", False)]

    def _gt_of(self, name, targets):
        return _gt_masks_of(targets) if name == "mask" else _gt_keypoints_of(targets, self.keypoint_head.num_keypoints)

    def log_train_scalars(self, counts, values, layout, nrows):
        """EventStorage scalars of label_and_sample_proposals, FastRCNNOutputs._log_accuracy and the enabled branches from host values:
        the (fg, bg) rows of every image, and the step's counts as `forward_train_batched` packed them (values: the host list, layout: the
        pack's)."""
        named = unpack_step_counts(values, layout)
        _log_sample_counts(counts)
        for name in self._branches():
            getattr(self, "_log_{}_scalars".format(name))(named)
        _log_box_accuracy(named["box"], nrows)

    def _log_mask_scalars(self, c):
        """c: the host values of the step's counts by name -- `mask.pixels`: the loss kernel's three, `mask.rows`: the number of mask
        rows, `mask.status`: the mask kernels' status word."""
        from .mask_head import log_mask_scalars

        check_status(c["mask.status"][0])
        side = self.mask_head.map_scale * self.mask_pooler.output_size[0]
        log_mask_scalars(c["mask.pixels"], c["mask.rows"][0] * side * side)

    def _log_keypoint_scalars(self, c):
        """c: the host values of the step's counts by name -- `keypoint.valid`: the valid (row, keypoint) entries, `keypoint.selected` /
        `keypoint.fg`: the selected and the foreground rows of every image, `keypoint.status`: the keypoint kernels' status word.
        keypoint_head/num_fg_samples: the mean of the selected counts over the images that had foreground rows (reference roi_heads.py:95-119); kpts_num_skipped_batches whenever no entry was valid."""
        from .keypoint_head import check_keypoint_status, log_skipped_batch

        check_keypoint_status(c["keypoint.status"][0])
        kept = [s for s, f in zip(c["keypoint.selected"], c["keypoint.fg"]) if f > 0]
        if kept:
            get_event_storage().put_scalar("keypoint_head/num_fg_samples", sum(kept) / len(kept))
        if c["keypoint.valid"][0] == 0:
            log_skipped_batch()

    def _forward_train(self, features, proposals, targets):
        """StandardROIHeads training branch (reference roi_heads.py:554-629 + FastRCNNOutputs.losses)."""
        from .fast_rcnn import fast_rcnn_losses

        proposals = self.label_and_sample_proposals(proposals, targets)
        feats = [to_nhwc(features[f]) for f in self.in_features]
        dev = feats[0].device
        counts = [len(p) for p in proposals]
        R = max(max(counts), 1)
        sampled = getattr(proposals[0], "_lvc_sampled", None) if proposals else None
        if sampled is not None and sampled[3] == counts and sampled[0].shape[1] == R:
            boxes = sampled[0]          # the sampler's own padded [B,R,4] table: no per-image copies
        else:
            sampled = None
            boxes, _ = padded_boxes(proposals, "proposal_boxes", dev)
        full = all(c == R for c in counts)
        # no graph when everything below the predictor is frozen (ft_novel yaml); otherwise ROIAlign backward into the
        # pyramid and the fused Linear autograd of the box head (base / ft_all yamls)
        below = any(f.requires_grad for f in feats) or any(p.requires_grad for p in self.box_head.parameters())
        with torch.set_grad_enabled(below and torch.is_grad_enabled()):
            pooled = self.box_pooler.pool_nhwc(feats, boxes)
            if full:                    # every image filled its quota (the usual case): the pooled rows are the head's input as they lie
                h = self.box_head.forward_nhwc(pooled)
            else:
                keep = torch.cat([torch.arange(c, device=dev) + i * R for i, c in enumerate(counts)])
                h = self.box_head.forward_nhwc(pooled[keep].contiguous())
        if sampled is not None and full:
            pb, gc, gb = sampled[0].view(-1, 4), sampled[1].view(-1), sampled[2].view(-1, 4)
        else:
            pb = torch.cat([p.proposal_boxes.tensor for p in proposals], 0)
            gb = torch.cat([p.gt_boxes.tensor for p in proposals], 0)
            gc = torch.cat([p.gt_classes for p in proposals], 0)
        losses, pred = fast_rcnn_losses(self.box_predictor, h, pb, gb, gc)
        # accuracy scalars (reference fast_rcnn.py _log_accuracy): the four counts in ONE device->host read
        _log_box_accuracy(self._box_stats(pred, gc).tolist(), gc.numel())
        for name in self._branches():
            losses = dict(losses)
            losses["loss_" + name] = self._branch_loss_from_lists(name, features, proposals, targets, sampled if full else None)
        return proposals, losses

    def _sampled_tables(self, proposals, targets, sampled, branch):
        """(s_boxes [B,R,4], s_cls [B,R], s_m [B,R] int64, fg_count [B] int32) of the sampled Instances, for the per-image path's mask
        or keypoint loss: the sampler's own tables when they are at hand, else built from the lists."""
        dev = proposals[0].proposal_boxes.tensor.device
        if sampled is not None and len(sampled) >= 6:
            return sampled[0], sampled[1], sampled[4], sampled[5][:, 0]
        s_boxes, counts = padded_boxes(proposals, "proposal_boxes", dev)
        s_cls = torch.full(s_boxes.shape[:2], -1, dtype=torch.int64, device=dev)
        s_m = torch.zeros(s_boxes.shape[:2], dtype=torch.int64, device=dev)
        for i, p in enumerate(proposals):
            s_cls[i, : counts[i]] = p.gt_classes
            matched = getattr(p, "_lvc_matched", None)
            if matched is None and counts[i] and len(targets[i]) > 0:
                raise RuntimeError("the {} branch needs the matched gt index of every sampled row (label_and_sample_proposals)".format(branch))
            if counts[i] and matched is not None:      # (an image without ground truth has background rows only)
                s_m[i, : counts[i]] = matched
        # foreground precedes background in a sampled table: the foreground rows are the first fg_count[b]
        fg_count = ((s_cls >= 0) & (s_cls < self.num_classes)).sum(1).to(torch.int32)
        return s_boxes, s_cls, s_m, fg_count

    def _branch_loss_from_lists(self, name, features, proposals, targets, sampled):
        """The per-image path's mask or keypoint loss: the tables `_branch_loss_batched` takes, built from the sampled Instances (or the
        sampler's own tables when they are at hand), then one read for the logged counts."""
        dev = proposals[0].proposal_boxes.tensor.device
        s_boxes, s_cls, s_m, fg_count = self._sampled_tables(proposals, targets, sampled, name)
        bfeats = {f: to_nhwc(features[f]) for f in getattr(self, name + "_in_features")}
        loss, counts = self._branch_loss_batched(name, bfeats, s_boxes, s_cls, s_m, fg_count, self._gt_of(name, targets), K.new_status(dev))
        vec, layout = pack_step_counts(counts)
        getattr(self, "_log_{}_scalars".format(name))(unpack_step_counts(vec.tolist(), layout))
        return loss


def pack_step_counts(parts):
    """The counts a training step reads back, as ONE int64 device vector: parts: name -> integer device tensor, in the order packed.
    -> (vector, layout: ((name, length), ...)); a single part is handed over as it is (no copy)."""
    tensors = [v.reshape(-1).long() for v in parts.values()]
    return (tensors[0] if len(tensors) == 1 else torch.cat(tensors)), tuple((k, t.numel()) for k, t in zip(parts, tensors))


def unpack_step_counts(values, layout):
    """The host list read from `pack_step_counts`' vector, back under its names: -> {name: list of that part's values}."""
    if len(values) != sum(n for _name, n in layout):
        raise ValueError("unpack_step_counts: {} values for the layout {} ({} values)".format(len(values), layout, sum(n for _name, n in layout)))
    out, at = {}, 0
    for name, n in layout:
        out[name] = values[at:at + n]
        at += n
    return out


def _gt_field_of(targets, field, branch, check, empty):
    """The ground-truth `field` of every image (check(value) raises on one the branch does not take); an image without ground truth
    may come without the field: empty(instances)."""
    out = []
    for t in targets:
        if t.has(field):
            check(t.get(field))
            out.append(t.get(field))
        elif len(t) == 0:
            out.append(empty(t))
        else:
            raise ValueError("training the {} branch: an image's ground truth has no `{}` field".format(branch, field))
    return out


def _gt_masks_of(targets):
    """The ground-truth masks of every image; an image without ground truth may come without the field: no planes."""
    from ...structures import BitMasks

    return _gt_field_of(targets, "gt_masks", "mask", lambda m: None,
                        lambda t: BitMasks(torch.zeros(0, *t.image_size, dtype=torch.bool, device=t.gt_boxes.tensor.device)))


def _gt_keypoints_of(targets, num_keypoints):
    """The ground-truth keypoints of every image; an image without ground truth may come without the field: no instances."""
    from ...structures import Keypoints

    def check(kp):
        if not isinstance(kp, Keypoints):
            raise ValueError("training the keypoint branch: `gt_keypoints` must be a structures.Keypoints, got {}".format(type(kp).__name__))
        if kp.tensor.shape[1] != num_keypoints:
            raise ValueError("training the keypoint branch: gt_keypoints with {} keypoints, MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS = {}"
                             .format(kp.tensor.shape[1], num_keypoints))

    return _gt_field_of(targets, "gt_keypoints", "keypoint", check,
                        lambda t: Keypoints(torch.zeros(0, num_keypoints, 3, device=t.gt_boxes.tensor.device)))


def widen_limits(model, exc):
    """React to a capacity / range condition the reference does not have: candidate list sized for R*K, or the range-free
    bf16x3 split; logged once.  Returns False when the limit was already at its widest (the caller re-raises)."""
    import logging

    if isinstance(exc, CandidateOverflow):
        if hasattr(model, "max_survivors"):      # RetinaNet: the per-(image, level) list of entries above SCORE_THRESH_TEST
            if model.max_survivors is None:
                return False
            # four times the capacity per step (the workspace is 8 bytes per slot, image and level), H*W*A*K only as the last resort
            wider = None if model.max_survivors >= (1 << 28) else model.max_survivors * 4
            logging.getLogger("lvc_amd").warning(
                "more than %d entries above SCORE_THRESH_TEST on one (image, level): re-running with lists of %s and keeping that size",
                model.max_survivors, "H*W*A*K" if wider is None else wider)
            model.max_survivors = wider
            return True
        heads = getattr(model, "roi_heads", None)
        if heads is None or heads.det_max_candidates is None:
            return False
        logging.getLogger("lvc_amd").warning(
            "more than %d (roi, class) candidates above SCORE_THRESH_TEST in one image: re-running with the list sized "
            "for R*K and keeping that size", heads.det_max_candidates)
        heads.det_max_candidates = None
        return True
    if isinstance(exc, K.Fp16RangeError):
        if exc.rerouted:       # the layers that overflowed were moved to their next wider form (kernels.check_conv_error_word)
            return True
        if K.CONV_SPLIT == "bf16x3":
            return False
        K.use_range_free_split()
        return True
    return False


def run_with_fallbacks(model, fn):
    """Run fn() (one pass that ends by reading the status words); on CandidateOverflow / Fp16RangeError widen the limit
    (`widen_limits`) and run again -- the pass degrades (one repeated batch, slower kernels) instead of failing."""
    for _ in range(8):     # a pass may move layers up one tier at a time (one accumulator -> two -> bf16x3), a few layers per pass
        try:
            return fn()
        except (CandidateOverflow, K.Fp16RangeError) as e:
            if not widen_limits(model, e):
                raise
    return fn()


def instances_from_batched(boxes, scores, classes, count, image_sizes, status=None):
    """One device->host read (counts + status), then per-image `Instances` of device tensors."""
    classes64 = classes.to(torch.int64)     # one conversion for the batch (queued BEFORE the blocking read: it runs in the step's tail,
                                            # not in the gap behind it); the per-image fields below are views
    if status is not None:
        # ONE read: counts, the status word and whether any of the conv kernels' error / range words is set
        meta = torch.cat([count, status, K.range_summary(count.device)]).tolist()
        counts, st, flagged = meta[:-2], meta[-2], meta[-1]
        check_status(st)
        if flagged:
            K.check_conv_error_word(count.device)   # spin timeout / a layer beyond its fp16 split's range: re-routes and raises
    else:
        counts = count.tolist()
    out = []
    # The host builds these while the GPU idles (forward() returns the batch's results before the next batch can be enqueued): the
    # three fields of an image are rows [0, n) of device tensors of one shape -- the objects are filled directly instead of through
    # Boxes.__init__ (as_tensor, reshape of empties, asserts) and Instances.set (a length check per field); 90 -> 45 us per batch.
    # ... and the B x 3 row ranges come from three split calls over the flattened tensors (sizes n_0, T - n_0, n_1, T - n_1, ...: every
    # other piece) instead of 24 narrows.
    B, T = scores.shape[0], scores.shape[1]
    if boxes.is_contiguous() and scores.is_contiguous() and len(image_sizes) == B:
        pieces = []
        for n in counts[:B]:
            pieces.append(n)
            pieces.append(T - n)
        bx = boxes.view(B * T, boxes.shape[2]).split_with_sizes(pieces)[0::2]
        sc = scores.view(B * T).split_with_sizes(pieces)[0::2]
        cl = classes64.view(B * T).split_with_sizes(pieces)[0::2]
    else:
        bx = [boxes[i, :counts[i]] for i in range(len(image_sizes))]
        sc = [scores[i, :counts[i]] for i in range(len(image_sizes))]
        cl = [classes64[i, :counts[i]] for i in range(len(image_sizes))]
    for i, size in enumerate(image_sizes):
        b = Boxes.__new__(Boxes)
        b.tensor = bx[i]
        inst = Instances(tuple(size))
        inst._fields.update(pred_boxes=b, scores=sc[i], pred_classes=cl[i])
        out.append(inst)
    return out


class CandidateOverflow(RuntimeError):
    """More (roi, class) pairs above SCORE_THRESH_TEST in one image than the candidate list was sized for.  The model
    entry points catch it, size the list for R*K (`StandardROIHeads.det_max_candidates = None`) and run again."""


def check_status(st):
    """Device status word written by the kernels (no sync on the hot path; read with the results)."""
    if st & K.ROI_NEGATIVE_SIZE:
        raise RuntimeError("ROIs in ROIAlign cannot have non-negative size!")  # reference ROIAlign_cpu.cpp:149-152
    if st & K.DET_OVERFLOW:
        raise CandidateOverflow("lvc_fast_rcnn_inference: more (roi, class) candidates above SCORE_THRESH_TEST in one "
                                "image than the candidate list holds; re-run with max_candidates=None (= R*K)")
    if st & K.MASK_BAD_CLASS:
        raise IndexError("lvc_mask_deconv_predict / lvc_mask_deconv_logits / lvc_mask_deconv_grad: a class index lies outside the mask "
                         "predictor's [0, K)")
    if st & K.KEYPOINT_BAD_TARGET:
        raise IndexError("lvc_keypoint_loss: a heatmap target lies outside the keypoint map")
    if st & K.RETINA_OVERFLOW:
        raise CandidateOverflow("lvc_retinanet_select: more entries above SCORE_THRESH_TEST on one (image, level) than the survivor "
                                "list holds; re-run with max_survivors=None (= H*W*A*K)")
