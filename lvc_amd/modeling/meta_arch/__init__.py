from .build import META_ARCH_REGISTRY, build_model
from .rcnn import GeneralizedRCNN, GeneralizedRCNNRegOnly, ProposalNetwork
from .retinanet import RetinaNet, RetinaNetHead
from .semantic_seg import SEM_SEG_HEADS_REGISTRY, SemanticSegmentor, SemSegFPNHead, build_sem_seg_head
from .panoptic_fpn import PanopticFPN

__all__ = [k for k in globals().keys() if not k.startswith("_")]
