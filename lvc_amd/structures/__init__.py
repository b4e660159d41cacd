from .boxes import Boxes, BoxMode, pairwise_iou
from .image_list import ImageList
from .instances import Instances
from .keypoints import Keypoints, heatmaps_to_keypoints
from .masks import BitMasks

__all__ = ["Boxes", "BoxMode", "pairwise_iou", "ImageList", "Instances", "BitMasks", "Keypoints", "heatmaps_to_keypoints"]
