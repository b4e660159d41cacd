"""detector_postprocess (reference detectron2/modeling/postprocessing.py:10-79): boxes and masks.
On the hot path the same scale/clip/drop-empty is fused into the detection gather kernel
(csrc/boxes.hip det_gather_kernel) and the masks are pasted from one job table for the batch (GeneralizedRCNN); this host
version serves callers holding `Instances`."""
import torch

from .. import kernels as K
from ..structures import Instances


def paste_masks_in_image(masks, boxes, image_shape, threshold=0.5):
    """Reference detectron2/layers/mask_ops.py:67-135 through csrc/mask_paste.hip: masks [N, Sm, Sm] soft masks, boxes [N, 4] (Boxes or
    tensor) in image coordinates -> bool [N, H, W].  One device->host read (the boxes: the job table is built on the host).
    Boxes must be non-empty (detector_postprocess filters first); threshold >= 0."""
    assert masks.shape[-1] == masks.shape[-2], "Only square mask predictions are supported"
    if not isinstance(boxes, torch.Tensor):
        boxes = boxes.tensor
    N = len(masks)
    H, W = int(image_shape[0]), int(image_shape[1])
    assert len(boxes) == N, boxes.shape
    if N == 0:
        return torch.zeros((0, H, W), dtype=torch.bool, device=masks.device)
    jobs = K.paste_jobs(range(N), boxes.detach().float().cpu().numpy(), [(H, W)] * N, [i * H * W for i in range(N)])
    buf = K.paste_masks(masks.contiguous().float(), jobs, N * H * W, threshold=threshold)
    return buf[: N * H * W].view(N, H, W).view(torch.bool)


def detector_postprocess(results, output_height, output_width, mask_threshold=0.5):
    scale_x, scale_y = output_width / results.image_size[1], output_height / results.image_size[0]
    results = Instances((output_height, output_width), **results.get_fields())
    if results.has("pred_boxes"):
        output_boxes = results.pred_boxes
    elif results.has("proposal_boxes"):
        output_boxes = results.proposal_boxes
    else:
        return results
    output_boxes.scale(scale_x, scale_y)
    output_boxes.clip(results.image_size)
    results = results[output_boxes.nonempty()]
    if results.has("pred_masks"):
        results.pred_masks = paste_masks_in_image(results.pred_masks[:, 0, :, :], results.pred_boxes, results.image_size,
                                                  threshold=mask_threshold)
    if results.has("pred_keypoints"):
        # reference postprocessing.py:75-77: x and y scaled by two separate multiplies; keypoints are not clipped
        kp = results.pred_keypoints.clone()
        kp[:, :, 0] *= scale_x
        kp[:, :, 1] *= scale_y
        results.pred_keypoints = kp
    return results
