"""PanopticFPN (reference detectron2/modeling/meta_arch/panoptic_fpn.py), inference only: the Mask R-CNN forward of
`GeneralizedRCNN` plus the semantic head on the same pyramid and `combine_semantic_and_instance_outputs` on the device.

The eval forward is one stream of launches around two device->host reads:
  trunk -> RPN -> box branch -> mask branch -> semantic head -> semantic postprocess (soft logits and / or label map, one launch)
  -> read 1 (the mask model's: counts, status, range words, the survivors' rows and boxes, from which the host builds the paste table)
  -> mask paste (one launch) -> combine (one launch: one workgroup per image) -> read 2 (the segment tables and their counts).
There is no host round trip per instance or per stuff label, where the reference has several `.item()` per instance.

Returns the reference's dicts: "instances", "sem_seg" ([K, H, W] soft logits; with `keep_sem_seg_logits = False` "sem_seg_labels"
in its place) and, with MODEL.PANOPTIC_FPN.COMBINE.ENABLED, "panoptic_seg" = (int32 [H, W], segments_info).
"""
import torch

from ... import kernels as K
from ..roi_heads import StandardROIHeads
from ..roi_heads.roi_heads import run_with_fallbacks
from ..proposal_generator import RPN
from .build import META_ARCH_REGISTRY
from .rcnn import GeneralizedRCNN
from .semantic_seg import TRAIN_REFUSAL, build_sem_seg_head, semantic_outputs


@META_ARCH_REGISTRY.register()
class PanopticFPN(GeneralizedRCNN):
    keep_sem_seg_logits = True

    def __init__(self, cfg):
        if not cfg.MODEL.MASK_ON:
            raise NotImplementedError("MODEL.MASK_ON = False: PanopticFPN combines the mask branch's planes with the semantic labels; "
                                      "build it with MODEL.MASK_ON: True")
        super().__init__(cfg)
        P = cfg.MODEL.PANOPTIC_FPN
        self.instance_loss_weight = P.INSTANCE_LOSS_WEIGHT
        self.combine_on = bool(P.COMBINE.ENABLED)
        self.combine_overlap_threshold = float(P.COMBINE.OVERLAP_THRESH)
        self.combine_stuff_area_limit = float(P.COMBINE.STUFF_AREA_LIMIT)
        self.combine_instances_confidence_threshold = float(P.COMBINE.INSTANCES_CONFIDENCE_THRESH)
        if not (isinstance(self.proposal_generator, RPN) and type(self.roi_heads) is StandardROIHeads and self._mask_on()):
            raise NotImplementedError("PanopticFPN is built on RPN + StandardROIHeads with the mask branch "
                                      "(MODEL.PROPOSAL_GENERATOR.NAME, MODEL.ROI_HEADS.NAME, MODEL.MASK_ON)")
        self.sem_seg_head = build_sem_seg_head(cfg, self.backbone.output_shape())
        self.sem_seg_head.to(self.device)

    def forward(self, batched_inputs):
        if self.training:
            raise NotImplementedError(TRAIN_REFUSAL)
        return run_with_fallbacks(self, lambda: self._inference_panoptic(batched_inputs))

    def inference(self, batched_inputs, detected_instances=None, do_postprocess=True):
        if detected_instances is None and do_postprocess:
            return self.forward(batched_inputs)
        raise NotImplementedError("PanopticFPN.inference: given boxes and do_postprocess=False are the mask model's (GeneralizedRCNN)")

    def _on_features(self, feats, batched_inputs, sizes, do_postprocess):
        # behind the mask branch, in front of the mask model's read: the semantic launches' range words travel with that read
        out_sizes = [(int(h), int(w)) for h, w in self.post_rows(batched_inputs, sizes)[1]]
        self.__dict__["_semantic"] = semantic_outputs(self.sem_seg_head, feats, batched_inputs, sizes, out_sizes,
                                                      self.keep_sem_seg_logits, self.combine_on)

    def _inference_panoptic(self, batched_inputs):
        self.__dict__.pop("_semantic", None)
        insts, planes = self._masks_and_planes(batched_inputs, True)
        sem, labels, label_off = self.__dict__.pop("_semantic")
        results = [dict(s, instances=r) for s, r in zip(sem, insts)]
        if not self.combine_on:
            return results
        B, T = planes["scores"].shape
        sizes = [tuple(s) for s in planes["out_sizes"]]
        pan, seg, cnt, pan_off, seg_off = K.panoptic_combine(
            planes["buffer"], planes["jobs"], planes["counts"], sizes, planes["scores"], planes["classes"], [i * T for i in range(B)],
            labels, label_off, self.sem_seg_head.num_classes, self.combine_overlap_threshold, self.combine_stuff_area_limit,
            self.combine_instances_confidence_threshold, use_boxes=self.mask_threshold > 0)
        table = torch.cat([cnt[:B], seg.view(-1)]).cpu().numpy()      # the second read: counts and segment rows
        counts, rows = table[:B], table[B:].reshape(-1, K.SEG_SEGMENT_FIELDS)
        for i, (h, w) in enumerate(sizes):
            info = K.segments_info(rows[seg_off[i]: seg_off[i] + int(counts[i])])
            results[i]["panoptic_seg"] = (pan[pan_off[i]: pan_off[i] + h * w].view(h, w), info)
        return results
