"""heatmaps_to_keypoints (reference detectron2/structures/keypoints.py:145-212) on device tensors: one launch of
csrc/keypoint_decode.hip for all RoIs and keypoints instead of the reference's Python loop over RoIs.  (`structures.Keypoints`, the
ground-truth container, and `Keypoints.to_heatmap` belong to training and are not built.)"""
import torch

from .. import kernels as K


@torch.no_grad()
def heatmaps_to_keypoints(maps, rois):
    """maps [#ROIs, #keypoints, POOL_H, POOL_W] logits (square, side <= 64), rois [#ROIs, 4] -> [#ROIs, #keypoints, 4] =
    (x, y, logit, score).  Among equal maxima of a resized map the lowest flat index y * w + x wins."""
    return K.heatmaps_to_keypoints(maps.detach().contiguous().float(), rois.detach().contiguous().float(), up=1)
