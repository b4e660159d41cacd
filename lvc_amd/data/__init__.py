"""Input transforms of the detector (the part of detectron2/data that sits on the device here): the test-time resize, and the
training input -- crop, colour jitter, resize or large-scale jitter, flip, annotations, batching (dataset_mapper.py, build.py) and 4- / 9-tile mosaics (mosaic.py)."""
from .transforms import (AugmentationList, ColorJitter, ColorJitterTransform, CropTransform, HFlipTransform, NoOpTransform, RandomCrop, RandomFlip, ResizeShortestEdge,
                         FixedSizeCrop, LargeScaleJitter, PadTransform, ResizeScale, ResizeTransform, TrainInputParams, TransformList, resample_coeffs)
from .dataset_mapper import DatasetMapper, DatasetMapperIgnore, build_augmentation
from .build import AspectRatioGrouper, TrainingSampler, build_detection_train_loader, build_detection_train_mosaic_loader
from .mosaic import DatasetMapperMosaic, MapDatasetMosaic, mosaic4_layout, mosaic9_layout

__all__ = ["FixedSizeCrop", "LargeScaleJitter", "PadTransform", "ResizeScale", "AugmentationList", "ColorJitter", "ColorJitterTransform", "CropTransform", "HFlipTransform", "NoOpTransform", "RandomCrop", "RandomFlip", "ResizeShortestEdge",
           "ResizeTransform", "TrainInputParams", "TransformList", "resample_coeffs", "DatasetMapper", "DatasetMapperIgnore",
           "build_augmentation", "AspectRatioGrouper", "TrainingSampler", "build_detection_train_loader", "build_detection_train_mosaic_loader",
           "DatasetMapperMosaic", "MapDatasetMosaic", "mosaic4_layout", "mosaic9_layout"]
