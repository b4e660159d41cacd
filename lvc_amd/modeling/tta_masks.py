"""`GeneralizedRCNNWithTTA` as `lvc_amd.modeling` hands it out: test_time_augmentation.py's class behind one refusal.

Test-time augmentation merges the box branch only (test_time_augmentation.py runs `inference_batched`, whose five return values carry
no masks), so a model built with MODEL.MASK_ON would come back box-only without a word.  The reference's TTA re-runs the mask head on
the merged boxes (`_reduce_pred_masks`); that is not built, and the wrapper says so under the key when it is constructed.
`lvc_amd.modeling.GeneralizedRCNNWithTTA` is this class; test_time_augmentation.py itself is left as it was."""
from torch.nn.parallel import DistributedDataParallel

from . import test_time_augmentation as _tta


class GeneralizedRCNNWithTTA(_tta.GeneralizedRCNNWithTTA):
    def __init__(self, cfg, model, tta_mapper=None, batch_size=3):
        inner = model.module if isinstance(model, DistributedDataParallel) else model
        if getattr(inner, "sem_seg_head", None) is not None:
            raise NotImplementedError("MODEL.META_ARCHITECTURE = {} (MODEL.SEM_SEG_HEAD): semantic and panoptic outputs under test-time "
                                      "augmentation are not built".format(type(inner).__name__))
        if cfg.MODEL.MASK_ON or getattr(getattr(inner, "roi_heads", None), "mask_on", False):
            raise NotImplementedError("MODEL.MASK_ON: masks under test-time augmentation are not built (the box branch only)")
        super().__init__(cfg, model, tta_mapper=tta_mapper, batch_size=batch_size)

