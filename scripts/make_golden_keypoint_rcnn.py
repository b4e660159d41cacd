"""Generate tests/golden/keypoint_rcnn_r50_fpn_keys.npz, keypoint_head_small.npz and keypoint_rcnn_small.npz: detectron2's Keypoint
R-CNN pieces (reference detectron2/modeling/roi_heads/keypoint_head.py `KRCNNConvDeconvUpsampleHead`, structures/keypoints.py
`heatmaps_to_keypoints`, roi_heads.py `StandardROIHeads`, meta_arch/rcnn.py `GeneralizedRCNN`) run on the CPU.  Runs only where the
reference tree exists (as oracle/make_golden.py, whose import shim it uses).  Only data is stored; inputs and weights are regenerated
from their seeds (lvc_amd.utils.synthetic).  TEST INFRASTRUCTURE ONLY.

  keypoint_rcnn_r50_fpn_keys.npz   names + shapes of the R50-FPN Keypoint R-CNN's state_dict, 1 class (format of
                                   mask_rcnn_r50_fpn_keys.npz; `pixel_mean` / `pixel_std` left out as there)
  keypoint_head_small.npz          the head's tail alone on `synthetic.keypoint_head_case` operands, cases (M, S, Cin, K) = (6, 14, 64, 17)
                                   and (3, 7, 32, 5): maps{32,64}_<i> = the reference head's layers() [M, K, 4S, 4S] (no conv_fcn; the small
                                   case only), kp{32,64}_<i> = heatmaps_to_keypoints(maps, boxes) [M, K, 4], boxes_<i>
  keypoint_rcnn_small.npz          R50-FPN Keypoint R-CNN, 1 class, TEST.DETECTIONS_PER_IMAGE 20, weights
                                   `conditioned_keypoint_rcnn_state_dict(seed 0)`, the two images of the other small fixtures:
      det{32,64}_{boxes,scores,classes}_{i}   the detections of the fp32 model and of the model as .double()
      raw32_boxes_{i}                         the fp32 model's boxes before detector_postprocess (network coordinates)
      kp{32,64}_{i}                           pred_keypoints [n, K, 3] after detector_postprocess
      logit{32,64}_{i}                        the keypoints' logits [n, K] (column 2 of heatmaps_to_keypoints)
      match_{i}                               for every fp32 detection the index of its fp64 twin (same class, IoU > 0.9), or -1
      band_logit                              max |logit32 - logit64| over the matched detections' keypoints
      moved_ref, matched_keypoints            matched keypoints whose fp32 and fp64 positions differ (by more than 0.5 px) / their number
      noise_keys / noise_vals                 oracle.noise.deviation(fp32 detections, fp64 detections), as mask_rcnn_small.npz
      logit_std                               standard deviation of the fp32 model's heatmap logits

    python scripts/make_golden_keypoint_rcnn.py
"""
import copy
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import make_golden as mg  # noqa: E402  (installs the import shim)

from lvc_amd.utils import synthetic as syn  # noqa: E402

SIZES = ((128, 160, 3), (120, 176, 4))
HEAD_CASES = ((6, 14, 64, 17), (3, 7, 32, 5))
YAML = "COCO-detection/faster_rcnn_R_50_FPN_base.yaml"
MOVED_TOL = 0.5      # px: the twins' boxes differ by ~0.01 px, neighbouring positions by ~1 px


def build(topk=100):
    from detectron2.modeling.meta_arch.rcnn import GeneralizedRCNN
    from lvc.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(mg.refshim.REF_ROOT, "configs", YAML))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.META_ARCHITECTURE", "GeneralizedRCNN", "MODEL.KEYPOINT_ON", True,
                         "MODEL.MASK_ON", False, "MODEL.ROI_HEADS.NUM_CLASSES", 1, "TEST.DETECTIONS_PER_IMAGE", topk])
    return GeneralizedRCNN(cfg).eval()


def gen_keys():
    sd = build().state_dict()
    keys = [k for k in sd.keys() if k not in ("pixel_mean", "pixel_std")]
    mg.save("keypoint_rcnn_r50_fpn_keys", keys=np.array(keys), shapes=np.array([str(tuple(sd[k].shape)) for k in keys]))


def gen_head():
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.roi_heads.keypoint_head import KRCNNConvDeconvUpsampleHead
    from detectron2.structures.keypoints import heatmaps_to_keypoints

    d = {}
    for i, (M, S, cin, K) in enumerate(HEAD_CASES):
        x, w, b, boxes = syn.keypoint_head_case(M, S, cin, K)
        head = KRCNNConvDeconvUpsampleHead(ShapeSpec(channels=cin, width=S, height=S), num_keypoints=K, conv_dims=[]).eval()
        head.load_state_dict({"score_lowres.weight": w, "score_lowres.bias": b}, strict=True)
        with torch.no_grad():
            for tag, h, xx in (("32", head, x), ("64", copy.deepcopy(head).double(), x.double())):
                maps = h.layers(xx)
                if maps.numel() <= 20000:      # (the 56 x 56 maps of the larger case would be 1.3 MB: its decoded keypoints only)
                    d["maps%s_%d" % (tag, i)] = maps
                d["kp%s_%d" % (tag, i)] = heatmaps_to_keypoints(maps, boxes.to(maps.dtype))
        d["boxes_%d" % i] = boxes
        print("  head %s: max |logit32 - logit64| %.3e, positions that differ %d" % (
            (M, S, cin, K), float((d["kp32_%d" % i][:, :, 2].double() - d["kp64_%d" % i][:, :, 2]).abs().max()),
            int(((d["kp32_%d" % i][:, :, :2].double() - d["kp64_%d" % i][:, :, :2]).abs().amax(2) > MOVED_TOL).sum())))
    d["cases"] = np.array(HEAD_CASES)
    mg.save("keypoint_head_small", **d)


def gen_model():
    import detectron2.structures.keypoints as kpmod
    from detectron2.layers.roi_align import ROIAlign
    from detectron2.modeling.postprocessing import detector_postprocess
    from detectron2.structures import pairwise_iou

    model = build(topk=20)
    model.load_state_dict(syn.conditioned_keypoint_rcnn_state_dict(model.state_dict(), seed=0), strict=True)
    model64 = copy.deepcopy(model).double()
    for m in model64.modules():      # the poolers hand ROIAlign fp32 rois whatever the maps' dtype: the native op wants one dtype
        if isinstance(m, ROIAlign):
            m.register_forward_pre_hook(lambda mod, args: (args[0], args[1].to(args[0].dtype)))
    inputs = [{"image": syn.synthetic_image(seed, h, w), "height": h, "width": w} for h, w, seed in SIZES]
    inputs64 = [dict(x, image=x["image"].double()) for x in inputs]
    # the logits are not part of pred_keypoints: record what heatmaps_to_keypoints returns
    import detectron2.modeling.roi_heads.keypoint_head as khmod

    rec = []
    inner = kpmod.heatmaps_to_keypoints

    def recording(maps, rois):
        out = inner(maps, rois.to(maps.dtype))
        rec.append((out, maps))
        return out

    khmod.heatmaps_to_keypoints = recording
    d = {}
    try:
        with torch.no_grad():
            raw32 = model.inference(inputs, do_postprocess=False)
            raw64 = model64.inference(inputs64, do_postprocess=False)
    finally:
        khmod.heatmaps_to_keypoints = inner
    (xyls32, maps32), (xyls64, _maps64) = rec
    d["logit_std"] = np.float64(maps32.std())
    print("  heatmap logits: std %.3f" % d["logit_std"])
    band, moved, matched = 0.0, 0, 0
    o32, o64 = 0, 0
    for i, (h, w, _) in enumerate(SIZES):
        n32, n64 = len(raw32[i]), len(raw64[i])
        l32, l64 = xyls32[o32: o32 + n32, :, 2], xyls64[o64: o64 + n64, :, 2]
        o32, o64 = o32 + n32, o64 + n64
        d["raw32_boxes_%d" % i] = raw32[i].pred_boxes.tensor.clone()
        raw32[i].logit, raw64[i].logit = l32, l64      # (per-instance fields survive detector_postprocess's non-empty filter)
        p32, p64 = detector_postprocess(raw32[i], h, w), detector_postprocess(raw64[i], h, w)
        for tag, out in (("32", p32), ("64", p64)):
            d["det%s_boxes_%d" % (tag, i)], d["det%s_scores_%d" % (tag, i)] = out.pred_boxes.tensor, out.scores
            d["det%s_classes_%d" % (tag, i)] = out.pred_classes
            d["kp%s_%d" % (tag, i)], d["logit%s_%d" % (tag, i)] = out.pred_keypoints, out.logit
        iou = pairwise_iou(p32.pred_boxes, type(p32.pred_boxes)(p64.pred_boxes.tensor.float()))
        iou[p32.pred_classes[:, None] != p64.pred_classes[None, :]] = 0
        if iou.numel():
            best, match = iou.max(1)
            match[best <= 0.9] = -1
        else:
            match = torch.full((len(p32),), -1, dtype=torch.int64)
        d["match_%d" % i] = match.to(torch.int32)
        for a in range(len(p32)):
            if match[a] >= 0:
                band = max(band, float((p32.logit[a].double() - p64.logit[match[a]]).abs().max()))
                diff = (p32.pred_keypoints[a][:, :2].double() - p64.pred_keypoints[match[a]][:, :2]).abs().amax(1)
                moved += int((diff > MOVED_TOL).sum())
                matched += diff.numel()
        print("  image %d: %d detections (fp64 %d), %d matched" % (i, len(p32), len(p64), int((match >= 0).sum())))
    d["band_logit"], d["moved_ref"], d["matched_keypoints"] = np.float64(band), np.int64(moved), np.int64(matched)
    print("  band_logit %.3e; %d of %d matched keypoints moved" % (band, moved, matched))
    assert matched > 0, "no matched detection"
    from oracle import noise as onoise

    dets = {t: [(d["det%s_boxes_%d" % (t, i)].float(), d["det%s_scores_%d" % (t, i)].float(), d["det%s_classes_%d" % (t, i)]) for i in range(2)]
            for t in ("32", "64")}
    wide = onoise.deviation(dets["32"], dets["64"], onoise.WIDE_BOX, onoise.WIDE_SCORE)
    box_tol = max(onoise.LOOSE_BOX, onoise.IDENT_K * wide["box_median"])
    score_tol = max(onoise.LOOSE_SCORE, onoise.IDENT_K * wide["score_median"])
    nz = onoise.deviation(dets["32"], dets["64"], box_tol, score_tol)
    nz["box_tol"], nz["score_tol"] = box_tol, score_tol
    d["noise_keys"] = np.array(list(nz.keys()))
    d["noise_vals"] = np.array([float(v) for v in nz.values()])
    print("  noise", nz)
    mg.save("keypoint_rcnn_small", **d)
    size = os.path.getsize(os.path.join(mg.GOLD, "keypoint_rcnn_small.npz"))
    assert size <= (1 << 20), "fixture of %d bytes: the repository's limit for a committed file is 1 MiB" % size


if __name__ == "__main__":
    torch.manual_seed(0)
    gen_keys()
    gen_head()
    gen_model()
