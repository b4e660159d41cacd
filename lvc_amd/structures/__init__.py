from .boxes import Boxes, BoxMode, pairwise_iou
from .image_list import ImageList
from .instances import Instances
from .keypoints import heatmaps_to_keypoints
from .masks import BitMasks

__all__ = ["Boxes", "BoxMode", "pairwise_iou", "ImageList", "Instances", "BitMasks", "heatmaps_to_keypoints"]
