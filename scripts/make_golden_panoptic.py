"""Generate the fixtures of the semantic / panoptic tests from detectron2's own modules on the CPU (reference
detectron2/modeling/meta_arch/semantic_seg.py `SemSegFPNHead`, panoptic_fpn.py `PanopticFPN` and
`combine_semantic_and_instance_outputs`, postprocessing.py `sem_seg_postprocess`).  Runs only where the reference tree exists (as
oracle/make_golden.py, whose import shim it uses).  Only data is stored; inputs and weights are regenerated from their seeds
(lvc_amd.utils.synthetic).  TEST INFRASTRUCTURE ONLY.

  panoptic_fpn_keys.npz        names + shapes of the R50-FPN PanopticFPN's state_dict, 80 thing and 54 stuff classes (format of
                               r50_fpn_state_dict_keys.npz; `pixel_mean` / `pixel_std` left out as there)
  sem_seg_head_small.npz       `SemSegFPNHead` (GN, 128 channels) on `synthetic.sem_seg_pyramid` (p2 32x48 .. p5 4x6: a 32x44 p2 would not meet p5' in the level sum), weights
                               `synthetic.conditioned_sem_seg_head_state_dict`, in fp32 and as .double():
      low6, low6_err64                         the stride-4 logits [6, 32, 48] of the 6-class head, max |fp32 - fp64|
      err64_6_<j>                              max |fp32 - fp64| of sem_seg_postprocess(F.interpolate(x4), image_size (125, 173), OUTS[j])
      soft6_<j>                                its fp32 values [6, out_h, out_w], for the outputs SOFT_OUTS
      labels6_<j>, band6_<j>                   its argmax; packbits of the pixels whose fp64 top-two margin is below 2 * 3 * err64
      labels54_<j>, band54_<j>, err64_54_<j>   the same head with 54 classes (labels only), low54_err64 for its stride-4 logits
                               The script fails when a band exceeds CAP (0.1 %) of its pixels.
  panoptic_combine_cases.npz   hand-made masks, scores, classes and label maps on 61x83 and 40x57 canvases through
                               `combine_semantic_and_instance_outputs` (OVERLAP 0.5, STUFF_LIMIT 100, CONFIDENCE 0.5):
      names                                    the cases
      shape_<i>, masks_<i> (packbits [n,H,W]), scores_<i>, classes_<i>, labels_<i>       the inputs
      pan_<i>                                  panoptic_seg int32 [H, W]
      seg_<i>                                  int64 [segments, 5]: id, isthing, category_id, instance_id (-1: stuff), area (-1: thing)
      segscore_<i>                             float64 [segments]: score (0: stuff)

  panoptic_fpn_small.npz       the whole model on the two small fixture images: see `gen_model`

    python scripts/make_golden_panoptic.py [combine] [head] [keys] [model]
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

CAP = 1e-3
K_BAND = 3.0
OVERLAP, STUFF_LIMIT, CONFIDENCE = 0.5, 100, 0.5
BIG, SMALL = (61, 83), (40, 57)
IMAGE, OUTS = (125, 173), ((125, 173), (97, 131), (250, 346))
SOFT_OUTS = OUTS[:2]      # the soft values of the x2 output alone would be 2 MB: its labels and band are stored, as for 54 classes
YAML = "COCO-detection/faster_rcnn_R_50_FPN_base.yaml"


# ------------------------------------------------------------------------------------------------ combine
def _rect(shape, y0, x0, h, w):
    m = np.zeros(shape, dtype=bool)
    m[y0: y0 + h, x0: x0 + w] = True
    return m


def _stripes(shape, labels):
    """Vertical stripes of the given labels, left to right."""
    H, W = shape
    out = np.zeros(shape, dtype=np.int64)
    edges = np.linspace(0, W, len(labels) + 1).astype(int)
    for l, a, b in zip(labels, edges[:-1], edges[1:]):
        out[:, a:b] = l
    return out


def combine_cases():
    cases = []
    # overlap exactly at the threshold: 50 of 100 pixels taken -> 0.5 > 0.5 is false -> kept, on its free pixels
    cases.append(("overlap_at_threshold", BIG, [_rect(BIG, 10, 10, 10, 10), _rect(BIG, 10, 15, 10, 10)], [0.9, 0.8], [3, 7],
                  _stripes(BIG, [1, 2, 5])))
    # one free pixel fewer: 50 of 99 -> skipped
    m = _rect(BIG, 10, 15, 10, 10)
    m[19, 24] = False
    cases.append(("overlap_over_threshold", BIG, [_rect(BIG, 10, 10, 10, 10), m], [0.9, 0.8], [3, 7], _stripes(BIG, [1, 2, 5])))
    # a zero-area mask between two real ones; the list is not in score order
    cases.append(("zero_area", BIG, [_rect(BIG, 30, 40, 12, 9), np.zeros(BIG, dtype=bool), _rect(BIG, 5, 60, 20, 20)],
                  [0.7, 0.95, 0.99], [0, 1, 2], _stripes(BIG, [4, 0, 9])))
    # a score below the threshold in the middle of the list: the walk stops there, the 0.45 and 0.2 instances are never looked at
    cases.append(("low_score_in_the_middle", BIG, [_rect(BIG, 2, 2, 8, 8), _rect(BIG, 20, 20, 8, 8), _rect(BIG, 40, 40, 8, 8),
                                                   _rect(BIG, 50, 60, 8, 8)], [0.9, 0.45, 0.6, 0.2], [1, 2, 3, 4], _stripes(BIG, [7, 8])))
    # stuff areas: label 3 has exactly the limit (kept), label 4 one pixel less (skipped), label 6 has the limit but an instance
    # takes one of its pixels (skipped), label 0 is present and never a segment
    lab = np.zeros(BIG, dtype=np.int64)
    lab[0:10, 0:10] = 3
    lab[20:29, 0:11] = 4
    lab[40:50, 30:40] = 6
    lab[:, 60:] = 11
    cases.append(("stuff_area_limits", BIG, [_rect(BIG, 49, 39, 5, 5)], [0.8], [2], lab))
    cases.append(("no_instances", SMALL, [], [], [], _stripes(SMALL, [0, 2, 53])))
    # every instance rejected: below the threshold, empty, or covered
    cases.append(("all_rejected", SMALL, [_rect(SMALL, 3, 3, 6, 6), np.zeros(SMALL, dtype=bool)], [0.3, 0.4], [5, 6], _stripes(SMALL, [1, 3])))
    # a small canvas with instances, for a batch of two sizes in one call
    cases.append(("small_canvas", SMALL, [_rect(SMALL, 0, 0, 40, 30), _rect(SMALL, 10, 20, 20, 30), _rect(SMALL, 35, 50, 5, 7)],
                  [0.6, 0.97, 0.51], [19, 0, 4], _stripes(SMALL, [1, 1, 2, 0])))
    return cases


def gen_combine():
    from detectron2.modeling.meta_arch.panoptic_fpn import combine_semantic_and_instance_outputs
    from detectron2.structures import Instances

    d = {"names": np.array([c[0] for c in combine_cases()]), "params": np.array([OVERLAP, STUFF_LIMIT, CONFIDENCE], dtype=np.float64)}
    for i, (name, shape, masks, scores, classes, labels) in enumerate(combine_cases()):
        above = [s for s in scores if s >= CONFIDENCE]
        assert len(set(above)) == len(above), "%s: equal scores above the threshold" % name
        n = len(masks)
        inst = Instances(shape)
        inst.scores = torch.tensor(scores, dtype=torch.float32)
        inst.pred_classes = torch.tensor(classes, dtype=torch.int64)
        inst.pred_masks = torch.from_numpy(np.stack(masks)) if n else torch.zeros((0,) + shape, dtype=torch.bool)
        pan, info = combine_semantic_and_instance_outputs(inst, torch.from_numpy(labels), OVERLAP, STUFF_LIMIT, CONFIDENCE)
        d["shape_%d" % i] = np.array(shape)
        d["masks_%d" % i] = np.packbits(np.stack(masks).astype(np.uint8)) if n else np.zeros(0, dtype=np.uint8)
        d["scores_%d" % i], d["classes_%d" % i] = inst.scores, inst.pred_classes.to(torch.int32)
        d["labels_%d" % i] = labels.astype(np.uint8)
        d["pan_%d" % i] = pan.to(torch.int32)
        d["seg_%d" % i] = np.array([[s["id"], int(s["isthing"]), s["category_id"], s.get("instance_id", -1), s.get("area", -1)] for s in info],
                                   dtype=np.int64).reshape(-1, 5)
        d["segscore_%d" % i] = np.array([s.get("score", 0.0) for s in info], dtype=np.float64)
        print("  %-26s %s: %d instances -> %s" % (name, shape, n, [(s["id"], s["isthing"], s["category_id"]) for s in info]))
    mg.save("panoptic_combine_cases", **d)


# ------------------------------------------------------------------------------------------------ semantic head
def build_head(num_classes):
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.meta_arch.semantic_seg import SemSegFPNHead
    from lvc.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.SEM_SEG_HEAD.NUM_CLASSES", num_classes, "MODEL.SEM_SEG_HEAD.NORM", "GN",
                         "MODEL.SEM_SEG_HEAD.CONVS_DIM", 128, "MODEL.SEM_SEG_HEAD.COMMON_STRIDE", 4,
                         "MODEL.SEM_SEG_HEAD.IN_FEATURES", ["p2", "p3", "p4", "p5"]])
    shapes = {"p%d" % l: ShapeSpec(channels=256, stride=2 ** l) for l in (2, 3, 4, 5)}
    return SemSegFPNHead(cfg, shapes).eval()


def _post(mod, x, out):
    from detectron2.modeling.postprocessing import sem_seg_postprocess

    return sem_seg_postprocess(x, IMAGE, out[0], out[1])


def gen_head():
    d = {"image": np.array(IMAGE), "outs": np.array(OUTS)}
    feats = syn.sem_seg_pyramid(seed=0)
    for K in (6, 54):
        head = build_head(K)
        head.load_state_dict(syn.conditioned_sem_seg_head_state_dict(head.state_dict(), seed=0), strict=True)
        head64 = copy.deepcopy(head).double()
        with torch.no_grad():
            low32 = head.layers(feats)
            low64 = head64.layers({k: v.double() for k, v in feats.items()})
            up32, _ = head(feats)
            up64, _ = head64({k: v.double() for k, v in feats.items()})
        err = float((low32.double() - low64).abs().max())
        print("  %d classes: stride-4 logits std %.3f, max |fp32 - fp64| %.3e" % (K, float(low32.std()), err))
        d["low%d_err64" % K] = np.float64(err)
        if K == 6:
            d["low6"] = low32[0]
        for j, out in enumerate(OUTS):
            s32, s64 = _post(None, up32[0], out), _post(None, up64[0], out)
            e = float((s32.double() - s64).abs().max())
            top2 = s64.topk(2, dim=0).values
            band = (top2[0] - top2[1]) < 2 * K_BAND * e
            share = float(band.float().mean())
            differ = int((s32.argmax(0) != s64.argmax(0)).sum())
            print("    -> %s: err64 %.3e, band %d of %d pixels (%.4f %%), fp32 / fp64 argmaxes differing %d"
                  % (out, e, int(band.sum()), band.numel(), 100 * share, differ))
            assert share <= CAP, "band above the cap: change the conditioned predictor's spread (synthetic.SEM_SEG_PREDICTOR_STD)"
            assert torch.equal(s32.argmax(0)[~band], s64.argmax(0)[~band])
            d["err64_%d_%d" % (K, j)] = np.float64(e)
            if K == 6 and out in SOFT_OUTS:
                d["soft6_%d" % j] = s32
            d["labels%d_%d" % (K, j)] = s32.argmax(0).to(torch.uint8)
            d["band%d_%d" % (K, j)] = np.packbits(band.numpy().astype(np.uint8))
    mg.save("sem_seg_head_small", **d)
    size = os.path.getsize(os.path.join(mg.GOLD, "sem_seg_head_small.npz"))
    assert size <= (1 << 20), "fixture of %d bytes: the repository's limit for a committed file is 1 MiB" % size


# ------------------------------------------------------------------------------------------------ keys
def build_panoptic(num_things, num_stuff, topk=100):
    from detectron2.modeling.meta_arch.panoptic_fpn import PanopticFPN
    from lvc.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(mg.refshim.REF_ROOT, "configs", YAML))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.META_ARCHITECTURE", "PanopticFPN", "MODEL.MASK_ON", True,
                         "MODEL.ROI_MASK_HEAD.NAME", "MaskRCNNConvUpsampleHead", "MODEL.ROI_MASK_HEAD.NUM_CONV", 4,
                         "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", 14, "MODEL.ROI_HEADS.NUM_CLASSES", num_things,
                         "MODEL.SEM_SEG_HEAD.NUM_CLASSES", num_stuff, "TEST.DETECTIONS_PER_IMAGE", topk])
    return PanopticFPN(cfg).eval()


def gen_keys():
    sd = build_panoptic(80, 54).state_dict()
    keys = [k for k in sd.keys() if k not in ("pixel_mean", "pixel_std")]
    mg.save("panoptic_fpn_keys", keys=np.array(keys), shapes=np.array([str(tuple(sd[k].shape)) for k in keys]))
    print("  %d keys, %d of the semantic head" % (len(keys), sum(k.startswith("sem_seg_head.") for k in keys)))


# ------------------------------------------------------------------------------------------------ model
SIZES = ((128, 160, 3), (120, 176, 4))      # the two images of the other small fixtures
MODEL_STUFF_LIMIT = 400                     # (the default 4096 is a fifth of these images)
MODEL_CONFIDENCE = 0.8995                     # the walk stops inside both images' lists, in front of a mask smaller than its band
SOFT_CLASSES = (0, 17, 35, 53)              # the classes whose soft logits of image 0 are stored (all 54 would be 4.4 MB)


def _unpack(bits, n, h, w):
    return np.unpackbits(bits)[: n * h * w].reshape(n, h, w).astype(bool)


def gen_model():
    """panoptic_fpn_small.npz: PanopticFPN, 20 thing / 54 stuff classes, TEST.DETECTIONS_PER_IMAGE 20, STUFF_AREA_LIMIT 400, INSTANCES_CONFIDENCE_THRESH 0.8995, weights
    `conditioned_panoptic_state_dict(seed 0)`, in fp32 and as .double().  Its instance half is mask_rcnn_small.npz's (same modules, same
    seeded weights: asserted), whose detections, masks and mask bands the tests take from there.  Stored per image i:
      labels32_<i>, label_band_<i>    argmax of "sem_seg"; packbits of the pixels whose fp64 top-two margin is below 2 * 3 * sem_err64
      sem_err64, soft32_0             max |fp32 - fp64| of "sem_seg" over both images; the soft logits of image 0, classes SOFT_CLASSES
      pan32_<i>, seg32_<i>, segscore32_<i>    panoptic_seg and segments_info (format of panoptic_combine_cases.npz)
    Fails when a label band exceeds CAP, or when an accept / skip decision of the fp32 run could be flipped by the pixels in the bands."""
    from detectron2.layers.roi_align import ROIAlign

    model = build_panoptic(20, 54, topk=20)
    model.combine_stuff_area_limit = MODEL_STUFF_LIMIT
    model.combine_instances_confidence_threshold = MODEL_CONFIDENCE
    model.load_state_dict(syn.conditioned_panoptic_state_dict(model.state_dict(), seed=0), strict=True)
    model64 = copy.deepcopy(model).double()
    for m in model64.modules():
        if isinstance(m, ROIAlign):
            m.register_forward_pre_hook(lambda mod, args: (args[0], args[1].to(args[0].dtype)))
    inputs = [{"image": syn.synthetic_image(seed, h, w), "height": h, "width": w} for h, w, seed in SIZES]
    with torch.no_grad():
        out32 = model(inputs)
        out64 = model64([dict(x, image=x["image"].double()) for x in inputs])
    z = np.load(os.path.join(mg.GOLD, "mask_rcnn_small.npz"))
    nz = dict(zip(z["noise_keys"].tolist(), z["noise_vals"].tolist()))
    thr, conf = model.combine_overlap_threshold, model.combine_instances_confidence_threshold
    d = {"params": np.array([thr, MODEL_STUFF_LIMIT, conf], dtype=np.float64), "soft_classes": np.array(SOFT_CLASSES)}
    err = max(float((a["sem_seg"].double() - b["sem_seg"]).abs().max()) for a, b in zip(out32, out64))
    d["sem_err64"] = np.float64(err)
    d["soft32_0"] = out32[0]["sem_seg"][list(SOFT_CLASSES)]
    print("  sem_seg: std %.3f, max |fp32 - fp64| %.3e" % (float(out32[0]["sem_seg"].std()), err))
    for i, (h, w, _) in enumerate(SIZES):
        o, inst = out32[i], out32[i]["instances"]
        n = len(inst)
        assert torch.equal(inst.pred_boxes.tensor, torch.from_numpy(z["det32_boxes_%d" % i])), "the instance half is not mask_rcnn_small's"
        assert np.array_equal(inst.pred_masks.numpy(), _unpack(z["masks32_%d" % i], n, h, w))
        masks, mband = inst.pred_masks.numpy(), _unpack(z["band_%d" % i], n, h, w)
        s64 = out64[i]["sem_seg"]
        top2 = s64.topk(2, dim=0).values
        lband = ((top2[0] - top2[1]) < 2 * K_BAND * err).numpy()
        labels = o["sem_seg"].argmax(0).numpy()
        print("  image %d: label band %d of %d pixels (%.4f %%), %d labels present" % (i, int(lband.sum()), lband.size, 100 * lband.mean(), len(np.unique(labels))))
        assert lband.mean() <= CAP, "label band above the cap"
        assert np.array_equal(labels[~lband], s64.argmax(0).numpy()[~lband])
        pan, info = o["panoptic_seg"]
        pan = pan.numpy()
        # could the band pixels flip a decision?  replay the walk with the fp32 masks
        scores = inst.scores.numpy()
        order = np.argsort(-scores, kind="stable")
        taken = np.zeros((h, w), dtype=bool)
        taken_band = np.zeros((h, w), dtype=bool)
        for j in order:
            assert abs(float(scores[j]) - conf) > nz["score_tol"], "a score within the noise of the confidence threshold"
            if scores[j] < conf:
                break
            area, inter = int(masks[j].sum()), int((masks[j] & taken).sum())
            if z["match_%d" % i][j] < 0:
                # no fp64 twin at IoU 0.9, so mask_rcnn_small.npz has no band for it: decided only where the fp32 mask is empty and
                # so is the mask of the nearest fp64 detection of its class
                i64 = out64[i]["instances"]
                same = (i64.pred_classes == inst.pred_classes[j]).nonzero().flatten()
                assert area == 0 and len(same), "instance %d of image %d has no fp64 twin and a mask: its band is unknown" % (j, i)
                dist = (i64.pred_boxes.tensor[same].float() - inst.pred_boxes.tensor[j]).abs().max(1)[0]
                assert int(i64.pred_masks[same[int(dist.argmin())]].sum()) == 0, "instance %d of image %d: fp64 twin has a mask" % (j, i)
                continue
            unsure = int(mband[j].sum()) + int((taken_band & (masks[j] | mband[j])).sum())
            if area == 0:
                assert unsure == 0, "instance %d of image %d: an empty mask with band pixels" % (j, i)
                continue
            assert area > unsure, "instance %d of image %d: its area %d could be zero (%d band pixels)" % (j, i, area, unsure)
            margin = abs(inter - thr * area)
            assert margin > (1 + thr) * unsure, "instance %d of image %d: |intersect - thresh area| %.1f, %d band pixels" % (j, i, margin, unsure)
            if inter / area > thr:
                continue
            taken |= masks[j]
            taken_band |= mband[j]
        things = pan.copy()
        for s in info:
            if not s["isthing"]:
                things[pan == s["id"]] = 0
        free = things == 0
        for label in range(1, 54):
            area = int(((labels == label) & free).sum())
            unsure = int(lband.sum()) + int((taken_band & (labels == label)).sum())
            assert abs(area - MODEL_STUFF_LIMIT) > unsure, "label %d of image %d: area %d, %d band pixels" % (label, i, area, unsure)
        d["labels32_%d" % i] = labels.astype(np.uint8)
        d["label_band_%d" % i] = np.packbits(lband.astype(np.uint8))
        d["pan32_%d" % i] = pan.astype(np.int32)
        d["seg32_%d" % i] = np.array([[s["id"], int(s["isthing"]), s["category_id"], s.get("instance_id", -1), s.get("area", -1)] for s in info],
                                     dtype=np.int64).reshape(-1, 5)
        d["segscore32_%d" % i] = np.array([s.get("score", 0.0) for s in info], dtype=np.float64)
        info64 = out64[i]["panoptic_seg"][1]
        assert [(s["isthing"], s["category_id"]) for s in info] == [(s["isthing"], s["category_id"]) for s in info64], "fp32 / fp64 segments differ"
        print("  image %d: %d instances, label band %d pixels, segments %s" % (i, n, int(lband.sum()), [(s["id"], s["isthing"], s["category_id"]) for s in info]))
    mg.save("panoptic_fpn_small", **d)
    size = os.path.getsize(os.path.join(mg.GOLD, "panoptic_fpn_small.npz"))
    assert size <= (1 << 20), "fixture of %d bytes: the repository's limit for a committed file is 1 MiB" % size


if __name__ == "__main__":
    torch.manual_seed(0)
    what = sys.argv[1:] or ["combine", "head", "keys", "model"]
    if "model" in what:
        gen_model()
    if "combine" in what:
        gen_combine()
    if "head" in what:
        gen_head()
    if "keys" in what:
        gen_keys()
