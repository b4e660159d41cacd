"""Programmatic equivalents of the shipped yaml files, for environments where the reference's `configs/`
tree is not present (the GPU box, bench.py).  Values are the ones `configs/Base-RCNN-FPN.yaml:1-38` sets on
top of the defaults; loading the real yaml through `cfg.merge_from_file` gives the same node (asserted by
tests/test_config_dropin.py whenever /root/reference exists)."""
from . import get_cfg


def base_rcnn_fpn(depth=50, num_classes=80, device="cuda"):
    cfg = get_cfg()
    M = cfg.MODEL
    M.META_ARCHITECTURE = "GeneralizedRCNN"
    M.DEVICE = device
    M.MASK_ON = False
    M.BACKBONE.NAME = "build_resnet_fpn_backbone"
    M.RESNETS.OUT_FEATURES = ["res2", "res3", "res4", "res5"]
    M.RESNETS.DEPTH = depth
    M.FPN.IN_FEATURES = ["res2", "res3", "res4", "res5"]
    M.ANCHOR_GENERATOR.SIZES = [[32], [64], [128], [256], [512]]
    M.ANCHOR_GENERATOR.ASPECT_RATIOS = [[0.5, 1.0, 2.0]]
    M.RPN.IN_FEATURES = ["p2", "p3", "p4", "p5", "p6"]
    M.RPN.PRE_NMS_TOPK_TRAIN = 2000
    M.RPN.PRE_NMS_TOPK_TEST = 1000
    M.RPN.POST_NMS_TOPK_TRAIN = 1000
    M.RPN.POST_NMS_TOPK_TEST = 1000
    M.ROI_HEADS.NAME = "StandardROIHeads"
    M.ROI_HEADS.IN_FEATURES = ["p2", "p3", "p4", "p5"]
    M.ROI_HEADS.NUM_CLASSES = num_classes
    M.ROI_BOX_HEAD.NAME = "FastRCNNConvFCHead"
    M.ROI_BOX_HEAD.NUM_FC = 2
    M.ROI_BOX_HEAD.POOLER_RESOLUTION = 7
    return cfg


GN_OVERRIDES = ("MODEL.FPN.NORM", "GN", "MODEL.ROI_BOX_HEAD.NORM", "GN", "MODEL.ROI_BOX_HEAD.NUM_CONV", 4,
                "MODEL.ROI_BOX_HEAD.NUM_FC", 1)


def gn_rcnn_fpn(depth=50, num_classes=80, device="cuda"):
    """`base_rcnn_fpn` with GroupNorm in the pyramid and the 4conv1fc GroupNorm box head (detectron2's
    `Misc/scratch_mask_rcnn_R_50_FPN_*_gn.yaml` head and FPN settings; the trunk keeps FrozenBN)."""
    cfg = base_rcnn_fpn(depth=depth, num_classes=num_classes, device=device)
    cfg.merge_from_list(list(GN_OVERRIDES))
    return cfg


def mask_rcnn_fpn(depth=50, num_classes=80, device="cuda"):
    """Mask R-CNN on the ResNet-FPN trunk: what detectron2's `COCO-InstanceSegmentation/mask_rcnn_R_50_FPN_*.yaml` and the mask keys of
    `Base-RCNN-FPN.yaml` set on top of `base_rcnn_fpn` (four 3x3 convs, a 14x14 mask pooler).  Training is opt-in:
    `build_model(cfg).enable_mask_training()`."""
    cfg = base_rcnn_fpn(depth=depth, num_classes=num_classes, device=device)
    cfg.merge_from_list(["MODEL.MASK_ON", True, "MODEL.ROI_MASK_HEAD.NAME", "MaskRCNNConvUpsampleHead", "MODEL.ROI_MASK_HEAD.NUM_CONV", 4,
                         "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", 14])
    return cfg


def panoptic_fpn(depth=50, num_classes=80, num_stuff_classes=54, device="cuda"):
    """Panoptic FPN on the ResNet-FPN trunk: `mask_rcnn_fpn` with detectron2's `COCO-PanopticSegmentation/Base-Panoptic-FPN.yaml` on
    top (`META_ARCHITECTURE: PanopticFPN`, the semantic head's class count; the head keeps the defaults' GN, 128 channels, p2 .. p5
    and common stride 4; `MODEL.PANOPTIC_FPN.COMBINE.*` keep their defaults).  Training is opt-in:
    `build_model(cfg).enable_mask_training().enable_sem_seg_training()`; every item then carries "sem_seg" beside its "instances"."""
    cfg = mask_rcnn_fpn(depth=depth, num_classes=num_classes, device=device)
    cfg.merge_from_list(["MODEL.META_ARCHITECTURE", "PanopticFPN", "MODEL.SEM_SEG_HEAD.NUM_CLASSES", num_stuff_classes])
    return cfg


def keypoint_rcnn_fpn(depth=50, num_classes=1, device="cuda"):
    """Keypoint R-CNN on the ResNet-FPN trunk: the keys detectron2's `COCO-Keypoints/Base-Keypoint-RCNN-FPN.yaml` sets on top of
    `base_rcnn_fpn` that the model reads (one class -- person --, the keypoint branch with the defaults' eight 512-channel convs,
    17 keypoints and 14x14 pooler).  Training is opt-in: `build_model(cfg).enable_keypoint_training()`; it reads
    `MODEL.ROI_KEYPOINT_HEAD.LOSS_WEIGHT`, `MODEL.ROI_KEYPOINT_HEAD.NORMALIZE_LOSS_BY_VISIBLE_KEYPOINTS` (False: the summed loss is
    divided by images x NUM_KEYPOINTS x `MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE` x `MODEL.ROI_HEADS.POSITIVE_FRACTION`) and the
    sampler's keys; every image's ground truth carries `gt_keypoints` (structures.Keypoints).  `MIN_KEYPOINTS_PER_IMAGE` is a
    dataset filter and is not read."""
    cfg = base_rcnn_fpn(depth=depth, num_classes=num_classes, device=device)
    cfg.merge_from_list(["MODEL.KEYPOINT_ON", True, "MODEL.ROI_HEADS.NUM_CLASSES", num_classes])
    return cfg


def resnext_rcnn_fpn(depth=101, num_groups=32, width_per_group=8, num_classes=80, device="cuda"):
    """`base_rcnn_fpn` on a ResNeXt trunk: detectron2's `COCO-Detection/faster_rcnn_X_101_32x8d_FPN_3x.yaml` sets exactly these four
    keys (`STRIDE_IN_1X1: False` is the published X-101 setting; `True` builds too -- the grouped 3x3 is then always stride 1).
    32x4d, 32x8d and 64x4d are the widths the grouped kernel takes (kernels.grouped_conv_check)."""
    cfg = base_rcnn_fpn(depth=depth, num_classes=num_classes, device=device)
    cfg.merge_from_list(["MODEL.RESNETS.NUM_GROUPS", num_groups, "MODEL.RESNETS.WIDTH_PER_GROUP", width_per_group,
                         "MODEL.RESNETS.STRIDE_IN_1X1", False])
    return cfg


def resnet_d_rcnn_fpn(depth=50, num_classes=80, device="cuda"):
    """`base_rcnn_fpn` on the ResNet-D trunk (`MODEL.RESNETS.D: True`, the reference fork's CLIP-style RN50: DeepStem, and bottlenecks
    whose stride is a 2x2 average pool).  STRIDE_IN_1X1 has no effect on such a trunk.  Depths 50 / 101 / 152."""
    cfg = base_rcnn_fpn(depth=depth, num_classes=num_classes, device=device)
    cfg.merge_from_list(["MODEL.RESNETS.D", True])
    return cfg


def retinanet_r_fpn(depth=50, num_classes=80, device="cuda"):
    """RetinaNet on a ResNet-FPN trunk: what detectron2's `Base-RetinaNet.yaml` sets on top of the defaults (the pyramid over
    res3..res5 with P6 / P7 from res5, three anchor scales per octave and level).  Inference only."""
    cfg = get_cfg()
    M = cfg.MODEL
    M.META_ARCHITECTURE = "RetinaNet"
    M.DEVICE = device
    M.MASK_ON = False
    M.BACKBONE.NAME = "build_retinanet_resnet_fpn_backbone"
    M.RESNETS.OUT_FEATURES = ["res3", "res4", "res5"]
    M.RESNETS.DEPTH = depth
    M.FPN.IN_FEATURES = ["res3", "res4", "res5"]
    M.ANCHOR_GENERATOR.SIZES = [[x, x * 2 ** (1.0 / 3), x * 2 ** (2.0 / 3)] for x in [32, 64, 128, 256, 512]]
    M.ANCHOR_GENERATOR.ASPECT_RATIOS = [[0.5, 1.0, 2.0]]
    M.RETINANET.NUM_CLASSES = num_classes
    return cfg
