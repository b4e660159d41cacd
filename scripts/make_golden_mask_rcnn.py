"""Generate tests/golden/mask_rcnn_r50_fpn_keys.npz, mask_head_small.npz and mask_rcnn_small.npz: detectron2's Mask R-CNN pieces
(reference detectron2/modeling/roi_heads/mask_head.py `MaskRCNNConvUpsampleHead`, roi_heads.py `StandardROIHeads`, meta_arch/rcnn.py
`GeneralizedRCNN`, layers/mask_ops.py `paste_masks_in_image`) run on the CPU.  Runs only where the reference tree exists (as
oracle/make_golden.py, whose import shim it uses).  Only data is stored; inputs and weights are regenerated from their seeds
(lvc_amd.utils.synthetic).  TEST INFRASTRUCTURE ONLY.

  mask_rcnn_r50_fpn_keys.npz   names + shapes of the R50-FPN Mask R-CNN's state_dict, 80 classes (format of r50_fpn_state_dict_keys.npz;
                               detectron2's `pixel_mean` / `pixel_std` buffers are left out: the detector this project mirrors keeps them
                               as attributes, as r50_fpn_state_dict_keys.npz shows)
  mask_head_small.npz          the head's tail alone (deconv + ReLU + predictor + class pick + sigmoid) on `synthetic.mask_tail_case`
                               operands, cases (M, S, Cin, Cmid, K) = (37, 14, 256, 256, 20) and (3, 7, 64, 64, 3): prob32_<i>, classes_<i>,
                               err64_<i> = max |prob32 - prob64| given identical x
  mask_rcnn_small.npz          R50-FPN Mask R-CNN, 20 classes, TEST.DETECTIONS_PER_IMAGE 20, weights `conditioned_mask_rcnn_state_dict(seed 0)`,
                               the two images of the other small fixtures (128x160, 120x176):
      det{32,64}_{boxes,scores,classes}_{i}   the detections of the fp32 model and of the model as .double()
      raw32_{boxes}_{i}                       the fp32 model's boxes before detector_postprocess (network coordinates)
      prob32_{i}                              the fp32 model's soft masks [n, 28, 28] of the kept detections (what paste_masks_in_image gets)
      masks{32,64}_{i}                        pred_masks, np.packbits of [n, H, W]
      match_{i}                               for every fp32 detection the index of its fp64 twin (same class, IoU > 0.9), or -1
      band_soft                               max |soft32 - soft64| of the reference's own pasted soft values over the matched detections
      band_{i}                                packbits of [n, H, W]: pixels whose fp64 soft value lies within 3 * band_soft of 0.5 (rows
                                              of unmatched detections are zero and are not compared)
      share_compared, share_in_boxes          set-aside pixels / compared pixels of the matched masks; ... / pixels inside their boxes
      noise_keys / noise_vals                 oracle.noise.deviation(fp32 detections, fp64 detections) with the identity bars derived as
                                              oracle.noise.fp32_vs_fp64(derive_identity=True) derives them (box_tol, score_tol included)
      logit_std                               standard deviation of the selected-class mask logits (the conditioned head's spread)
  The script fails if share_compared exceeds CAP (0.1 %).

    python scripts/make_golden_mask_rcnn.py
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
NUM_CLASSES = 20
TAIL_CASES = ((37, 14, 256, 256, 20), (3, 7, 64, 64, 3))
CAP = 1e-3
YAML = "COCO-detection/faster_rcnn_R_50_FPN_base.yaml"


def build(num_classes, topk=100):
    from detectron2.modeling.meta_arch.rcnn import GeneralizedRCNN
    from lvc.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(mg.refshim.REF_ROOT, "configs", YAML))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.META_ARCHITECTURE", "GeneralizedRCNN", "MODEL.MASK_ON", True,
                         "MODEL.ROI_MASK_HEAD.NAME", "MaskRCNNConvUpsampleHead", "MODEL.ROI_MASK_HEAD.NUM_CONV", 4,
                         "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", 14, "MODEL.ROI_HEADS.NUM_CLASSES", num_classes,
                         "TEST.DETECTIONS_PER_IMAGE", topk])
    return GeneralizedRCNN(cfg).eval()


def gen_keys():
    sd = build(80).state_dict()
    keys = [k for k in sd.keys() if k not in ("pixel_mean", "pixel_std")]
    mg.save("mask_rcnn_r50_fpn_keys", keys=np.array(keys), shapes=np.array([str(tuple(sd[k].shape)) for k in keys]))


def gen_tail():
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.roi_heads.mask_head import MaskRCNNConvUpsampleHead, mask_rcnn_inference
    from detectron2.structures import Instances

    d = {}
    for i, (M, S, cin, cmid, K) in enumerate(TAIL_CASES):
        x, wd, bd, wp, bp, classes = syn.mask_tail_case(M, S, cin, cmid, K)
        head = MaskRCNNConvUpsampleHead(ShapeSpec(channels=cin, width=S, height=S), num_classes=K, conv_dims=[cmid]).eval()
        head.load_state_dict({"deconv.weight": wd, "deconv.bias": bd, "predictor.weight": wp, "predictor.bias": bp}, strict=True)
        out = []
        with torch.no_grad():
            for h, xx in ((head, x), (copy.deepcopy(head).double(), x.double())):
                inst = Instances((1, 1))
                inst.pred_classes = classes
                mask_rcnn_inference(h.layers(xx), [inst])
                out.append(inst.pred_masks[:, 0])
        err = float((out[0].double() - out[1]).abs().max())
        assert sorted(set(classes.tolist())) == list(range(K))
        print("  tail %s: max |prob32 - prob64| %.3e" % ((M, S, cin, cmid, K), err))
        d["prob32_%d" % i], d["classes_%d" % i], d["err64_%d" % i] = out[0], classes.to(torch.int32), np.float64(err)
    d["cases"] = np.array(TAIL_CASES)
    mg.save("mask_head_small", **d)


def soft_paste(mo, masks, boxes, H, W):
    return mo._do_paste_mask(masks, boxes, H, W, skip_empty=False)[0]


def gen_model():
    import detectron2.layers.mask_ops as mo
    from detectron2.modeling.postprocessing import detector_postprocess
    from detectron2.structures import pairwise_iou

    model = build(NUM_CLASSES, topk=20)
    model.load_state_dict(syn.conditioned_mask_rcnn_state_dict(model.state_dict(), seed=0), strict=True)
    model64 = copy.deepcopy(model).double()
    from detectron2.layers.roi_align import ROIAlign

    for m in model64.modules():      # the poolers hand ROIAlign fp32 rois whatever the maps' dtype: the native op wants one dtype
        if isinstance(m, ROIAlign):
            m.register_forward_pre_hook(lambda mod, args: (args[0], args[1].to(args[0].dtype)))
    inputs = [{"image": syn.synthetic_image(seed, h, w), "height": h, "width": w} for h, w, seed in SIZES]
    inputs64 = [dict(x, image=x["image"].double()) for x in inputs]
    grid_sample = mo.F.grid_sample
    d, logits = {}, []
    hook = model.roi_heads.mask_head.predictor.register_forward_hook(lambda m, i, o: logits.append(o))
    with torch.no_grad():
        raw32 = model.inference(inputs, do_postprocess=False)
        hook.remove()
        raw64 = model64.inference(inputs64, do_postprocess=False)
        cls = torch.cat([r.pred_classes for r in raw32])
        d["logit_std"] = np.float64(logits[0][torch.arange(len(cls)), cls].std())
        print("  selected-class mask logits: std %.3f" % d["logit_std"])
        softs, band_soft, n_compared, n_in_boxes = [], 0.0, 0, 0
        for i, (h, w, _) in enumerate(SIZES):
            d["raw32_boxes_%d" % i] = raw32[i].pred_boxes.tensor.clone()
            # the soft values first (detector_postprocess rescales the Instances' boxes in place)
            post = []
            for tag, r, dt in (("32", raw32[i], torch.float32), ("64", raw64[i], torch.float64)):
                if dt == torch.float64:
                    mo.F.grid_sample = lambda m, g, align_corners=False: grid_sample(m.double(), g.double(), align_corners=align_corners)
                try:
                    res = copy.deepcopy(r)
                    b = res.pred_boxes
                    b.scale(w / res.image_size[1], h / res.image_size[0])
                    b.clip((h, w))
                    keep = b.nonempty()
                    soft = soft_paste(mo, res.pred_masks[keep].to(dt), b.tensor[keep].to(dt), h, w)
                    if tag == "32":
                        d["prob32_%d" % i] = res.pred_masks[keep][:, 0].clone()
                    out = detector_postprocess(r, h, w)
                finally:
                    mo.F.grid_sample = grid_sample
                assert len(out) == len(soft) and (tag == "64" or torch.equal(out.pred_masks, soft >= 0.5))
                d["det%s_boxes_%d" % (tag, i)], d["det%s_scores_%d" % (tag, i)] = out.pred_boxes.tensor, out.scores
                d["det%s_classes_%d" % (tag, i)] = out.pred_classes
                d["masks%s_%d" % (tag, i)] = np.packbits(out.pred_masks.numpy().astype(np.uint8))
                post.append((out, soft))
            (o32, s32), (o64, s64) = post
            iou = pairwise_iou(o32.pred_boxes, type(o32.pred_boxes)(o64.pred_boxes.tensor.float()))
            iou[o32.pred_classes[:, None] != o64.pred_classes[None, :]] = 0
            best, match = iou.max(1)
            match[best <= 0.9] = -1
            d["match_%d" % i] = match.to(torch.int32)
            softs.append((s64, match, o32))
            for a in range(len(o32)):
                if match[a] >= 0:
                    band_soft = max(band_soft, float((s32[a].double() - s64[match[a]]).abs().max()))
        d["band_soft"] = np.float64(band_soft)
        aside = 0
        for i, (s64, match, o32) in enumerate(softs):
            n, (h, w) = len(o32), SIZES[i][:2]
            band = torch.zeros(n, h, w, dtype=torch.bool)
            ys, xs = torch.arange(h)[:, None] + 0.5, torch.arange(w)[None, :] + 0.5
            for a in range(n):
                if match[a] < 0:
                    continue
                band[a] = (s64[match[a]] - 0.5).abs() <= 3 * band_soft
                x0, y0, x1, y1 = o32.pred_boxes.tensor[a].tolist()
                n_in_boxes += int(((ys > y0) & (ys < y1) & (xs > x0) & (xs < x1)).sum())
                n_compared += h * w
            aside += int(band.sum())
            d["band_%d" % i] = np.packbits(band.numpy().astype(np.uint8))
            print("  image %d: %d detections (fp64 %d), %d matched" % (i, n, len(s64), int((match >= 0).sum())))
    # the reference against itself, as scripts/make_golden_retinanet.py records it: oracle.noise.deviation with derived identity bars
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
    d["share_compared"] = np.float64(aside / max(1, n_compared))
    d["share_in_boxes"] = np.float64(aside / max(1, n_in_boxes))
    print("  band_soft %.3e; set aside %d of %d compared pixels (%.5f %%), %.5f %% of the pixels inside the boxes"
          % (band_soft, aside, n_compared, 100 * d["share_compared"], 100 * d["share_in_boxes"]))
    assert n_compared > 0, "no matched detection"
    assert d["share_compared"] <= CAP, "set-aside share %.5f above the cap %.5f: change the conditioned weights' seed or scale" % (d["share_compared"], CAP)
    assert 2.0 <= d["logit_std"] <= 3.0, "the conditioned mask head's logits have std %.3f, want 2 .. 3 (synthetic.MASK_PREDICTOR_STD)" % d["logit_std"]
    mg.save("mask_rcnn_small", **d)
    size = os.path.getsize(os.path.join(mg.GOLD, "mask_rcnn_small.npz"))
    assert size <= (1 << 20), "fixture of %d bytes: the repository's limit for a committed file is 1 MiB" % size


if __name__ == "__main__":
    torch.manual_seed(0)
    gen_keys()
    gen_tail()
    gen_model()
