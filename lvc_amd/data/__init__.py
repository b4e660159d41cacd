"""Input transforms of the detector (the part of detectron2/data that sits on the device here): the test-time resize, and the
training input -- crop, resize, flip, annotations, batching (dataset_mapper.py, build.py)."""
from .transforms import (AugmentationList, CropTransform, HFlipTransform, NoOpTransform, RandomCrop, RandomFlip, ResizeShortestEdge,
                         ResizeTransform, TrainInputParams, TransformList, resample_coeffs)
from .dataset_mapper import DatasetMapper, DatasetMapperIgnore, build_augmentation
from .build import AspectRatioGrouper, TrainingSampler, build_detection_train_loader

__all__ = ["AugmentationList", "CropTransform", "HFlipTransform", "NoOpTransform", "RandomCrop", "RandomFlip", "ResizeShortestEdge",
           "ResizeTransform", "TrainInputParams", "TransformList", "resample_coeffs", "DatasetMapper", "DatasetMapperIgnore",
           "build_augmentation", "AspectRatioGrouper", "TrainingSampler", "build_detection_train_loader"]
