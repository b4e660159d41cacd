"""Keypoint structures (reference detectron2/structures/keypoints.py) on device tensors.

`heatmaps_to_keypoints` (:145-212): one launch of csrc/keypoint_decode.hip for all RoIs and keypoints instead of the reference's
Python loop over RoIs.

`Keypoints` (:9-141), the ground-truth container: tensor [N, K, 3] fp32 = (x, y, v) with v = 0 not labelled, 1 labelled but not
visible, 2 visible.  `to_heatmap` is one launch of csrc/keypoint_targets.hip (the training step calls the same kernel once for the
whole batch, with the row selection of `select_proposals_with_visible_keypoints` folded in: `kernels.keypoint_targets`)."""
import numpy as np
import torch

from .. import kernels as K


@torch.no_grad()
def heatmaps_to_keypoints(maps, rois):
    """maps [#ROIs, #keypoints, POOL_H, POOL_W] logits (square, side <= 64), rois [#ROIs, 4] -> [#ROIs, #keypoints, 4] =
    (x, y, logit, score).  Among equal maxima of a resized map the lowest flat index y * w + x wins."""
    return K.heatmaps_to_keypoints(maps.detach().contiguous().float(), rois.detach().contiguous().float(), up=1)


class Keypoints:
    """Keypoint annotations of N instances: `tensor` [N, K, 3] fp32 = (x, y, visibility)."""

    def __init__(self, keypoints):
        device = keypoints.device if isinstance(keypoints, torch.Tensor) else torch.device("cpu")
        if isinstance(keypoints, (list, tuple)) and len(keypoints) and isinstance(keypoints[0], torch.Tensor):
            keypoints = torch.stack(list(keypoints))
            device = keypoints.device
        keypoints = torch.as_tensor(keypoints if isinstance(keypoints, torch.Tensor) else np.asarray(keypoints, dtype=np.float32),
                                    dtype=torch.float32, device=device)
        assert keypoints.dim() == 3 and keypoints.shape[2] == 3, keypoints.shape
        self.tensor = keypoints

    def __len__(self):
        return self.tensor.size(0)

    def to(self, *args, **kwargs):
        return type(self)(self.tensor.to(*args, **kwargs))

    @property
    def device(self):
        return self.tensor.device

    @torch.no_grad()
    def to_heatmap(self, boxes, heatmap_size):
        """boxes [N, 4] (device) -> (heatmaps int64 [N, K]: the flat position y * size + x of every keypoint in its box's
        size x size map, 0 where not valid; valid int64 [N, K]: inside the map and v > 0).  The reference's plain rule, without the
        row selection.  A box of non-positive width or height is invalid (the reference floors an inf or a NaN there)."""
        n = len(self)
        assert boxes.shape == (n, 4), (boxes.shape, n)
        if n == 0:
            return boxes.new_zeros((0,), dtype=torch.int64), boxes.new_zeros((0,), dtype=torch.int64)
        dev = boxes.device
        kp = self.tensor.to(dev).contiguous()
        target, valid, _sel, _cnt = K.keypoint_targets(boxes.detach().float().contiguous().view(1, n, 4),
                                                       torch.arange(n, device=dev).view(1, n),
                                                       torch.full((1,), n, dtype=torch.int32, device=dev), [kp], heatmap_size,
                                                       apply_selection=False)
        return target.long(), valid.long()

    def __getitem__(self, item):
        """int: a Keypoints of one instance; slice, mask or index tensor: torch's indexing (may share storage)."""
        if isinstance(item, int):
            return Keypoints(self.tensor[item][None])
        return Keypoints(self.tensor[item])

    @staticmethod
    def cat(keypoints_list):
        assert len(keypoints_list) > 0 and all(isinstance(k, Keypoints) for k in keypoints_list)
        return Keypoints(torch.cat([k.tensor for k in keypoints_list], dim=0))

    def __repr__(self):
        return self.__class__.__name__ + "(num_instances={})".format(len(self.tensor))
