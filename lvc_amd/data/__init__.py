"""Test-time input transform of the detector (the part of detectron2/data that sits on the device here)."""
from .transforms import HFlipTransform, NoOpTransform, ResizeShortestEdge, ResizeTransform, TransformList, resample_coeffs

__all__ = ["HFlipTransform", "NoOpTransform", "ResizeShortestEdge", "ResizeTransform", "TransformList", "resample_coeffs"]
