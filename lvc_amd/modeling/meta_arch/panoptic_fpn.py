"""PanopticFPN (reference detectron2/modeling/meta_arch/panoptic_fpn.py): the Mask R-CNN forward of `GeneralizedRCNN` plus the
semantic head on the same pyramid and `combine_semantic_and_instance_outputs` on the device.

The eval forward is one stream of launches around two device->host reads:
  trunk -> RPN -> box branch -> mask branch -> semantic head -> semantic postprocess (soft logits and / or label map, one launch)
  -> read 1 (the mask model's: counts, status, range words, the survivors' rows and boxes, from which the host builds the paste table)
  -> mask paste (one launch) -> combine (one launch: one workgroup per image) -> read 2 (the segment tables and their counts).
There is no host round trip per instance or per stuff label, where the reference has several `.item()` per instance.

Returns the reference's dicts: "instances", "sem_seg" ([K, H, W] soft logits; with `keep_sem_seg_logits = False` "sem_seg_labels"
in its place) and, with MODEL.PANOPTIC_FPN.COMBINE.ENABLED, "panoptic_seg" = (int32 [H, W], segments_info).

The training forward (opt-in: `enable_mask_training()` and `enable_sem_seg_training()`, both) is the mask model's step plus the semantic
loss on the same features (semantic_seg.py); the loss's status word rides on the read the step already makes.  Losses as the reference
(panoptic_fpn.py:84-108): `loss_sem_seg`, the RPN losses as they are, every detector loss times INSTANCE_LOSS_WEIGHT.
"""
import torch

from ... import kernels as K
from ..roi_heads import StandardROIHeads
from ..roi_heads.roi_heads import run_with_fallbacks
from ..proposal_generator import RPN
from .build import META_ARCH_REGISTRY
from .rcnn import GeneralizedRCNN
from .semantic_seg import TRAIN_REFUSAL, build_sem_seg_head, check_sem_seg_items, sem_seg_targets, semantic_outputs


def panoptic_losses(sem_seg_losses, proposal_losses, detector_losses, instance_loss_weight):
    """reference panoptic_fpn.py:103-107, its quirk included: the detector losses are scaled, the RPN losses are not."""
    losses = dict(sem_seg_losses)
    losses.update(proposal_losses)
    losses.update({k: v * instance_loss_weight for k, v in detector_losses.items()})
    return losses


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

    def enable_sem_seg_training(self, on=True):
        """Switch the semantic half of the training forward on (or off again); returns self.  The step needs `enable_mask_training()`
        too; without either call the model in training mode refuses, as before.  Every item then carries "sem_seg" (an integer label
        map of the image's size) beside its "instances"."""
        self.__dict__["_sem_seg_train_enabled"] = bool(on)
        return self

    def forward(self, batched_inputs):
        if not self.training:
            return run_with_fallbacks(self, lambda: self._inference_panoptic(batched_inputs))
        sem, mask = self.__dict__.get("_sem_seg_train_enabled", False), self.__dict__.get("_mask_train_enabled", False)
        if not sem and not mask:
            raise NotImplementedError(TRAIN_REFUSAL)
        if not sem:
            raise NotImplementedError(TRAIN_REFUSAL + " into this model's step: call enable_sem_seg_training() beside enable_mask_training()")
        if not mask:
            raise NotImplementedError("training PanopticFPN takes the mask model's step: call enable_mask_training() beside "
                                      "enable_sem_seg_training()")
        check_sem_seg_items(batched_inputs, self.sem_seg_head.ignore_value)
        return super().forward(batched_inputs)

    # ------------------------------------------------------------------ training: the mask model's step and its hooks
    def _forward_train(self, batched_inputs):
        self.__dict__.pop("_sem_train", None)
        losses = super()._forward_train(batched_inputs)
        sem = self.__dict__.pop("_sem_train")
        if sem["word"] is None:      # not the deferred-read step (per-image paths with reads of their own): one more read here
            sem["word"] = int(sem["status"].item())
        self.sem_seg_head.check_loss_status(sem["word"])
        return losses

    def _on_train_features(self, features, batched_inputs, images):
        from ...layers.layout import to_nhwc

        head = self.sem_seg_head
        targets = sem_seg_targets(batched_inputs, images.image_sizes, self.device, head.ignore_value)
        logits = head.forward_train_nhwc({f: to_nhwc(features[f]) for f in head.in_features})
        status = torch.zeros(1, device=self.device, dtype=torch.int32)
        self.__dict__["_sem_train"] = {"losses": head.losses(logits, targets, status), "status": status, "word": None}

    def _train_extra_words(self):
        return [self.__dict__["_sem_train"]["status"].long()]

    def _on_train_extra_words(self, words):
        self.__dict__["_sem_train"]["word"] = int(words[0])

    def _train_losses(self, detector_losses, proposal_losses):
        return panoptic_losses(self.__dict__["_sem_train"]["losses"], proposal_losses, detector_losses, self.instance_loss_weight)

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
