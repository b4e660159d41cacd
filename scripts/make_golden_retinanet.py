"""Generate tests/golden/retinanet_r50_fpn_{keys,small}.npz and tests/golden/README_retinanet.md: detectron2's RetinaNet (reference
detectron2/modeling/meta_arch/retinanet.py, `LastLevelP6P7` in backbone/fpn.py) run on the CPU.  Runs only where the reference tree
exists (as oracle/make_golden.py, whose import shim it uses).  lvc's `build_model` keeps a registry of its own that does not hold
RetinaNet, so the class is instantiated directly from lvc's `get_cfg()`.  Only data is stored; inputs and weights are regenerated from
their seeds (lvc_amd.utils.synthetic).  TEST INFRASTRUCTURE ONLY.

  retinanet_r50_fpn_keys.npz    names + shapes of the R50 RetinaNet's state_dict, 80 classes (format of resnext_x50_fpn_keys.npz)
  retinanet_r50_fpn_small.npz   R50, 20 classes, the two images of make_golden_resnext.py (128x160, 120x176; batch padded to 128x192):
      logits_p3..p7, deltas_p3..p7   the head's outputs in fp32, whole, NHWC [2,H,W,A*K] / [2,H,W,4A] (channel a*K + k: the
                                     reference's permute_to_N_HWA_K order)
      err64_{logits,deltas}          per level max |fp32 - fp64| of those tensors, the model run as .double() (the whole fp64 tensors would put
                                     the file past the repository's 1 MiB limit; the tests need these maxima)
      cand_{index,score,class,box,level,image}   the candidates before NMS, image after image, level after level, in the reference's
                                     order: index = the flat index (p*A + a)*K + k inside the level
      det{32,64}_{boxes,scores,classes}_{0,1}    the final detections of the fp32 model and of the model as .double()
      noise_keys / noise_vals        oracle.noise.deviation(fp32 detections, fp64 detections) with the identity bars derived as
                                     oracle.noise.fp32_vs_fp64(derive_identity=True) derives them (box_tol, score_tol included),
                                     and the constants IDENT_K, WIDE_*, FLOOR_* they were derived with

    python scripts/make_golden_retinanet.py
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
from oracle import noise as onoise  # noqa: E402

from lvc_amd.utils import synthetic as syn  # noqa: E402

SIZES = ((128, 160, 3), (120, 176, 4))
NUM_CLASSES = 20


def ref_cfg(num_classes):
    from lvc.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_list([
        "MODEL.DEVICE", "cpu", "MODEL.META_ARCHITECTURE", "RetinaNet", "MODEL.BACKBONE.NAME", "build_retinanet_resnet_fpn_backbone",
        "MODEL.RESNETS.DEPTH", 50, "MODEL.RESNETS.OUT_FEATURES", ["res3", "res4", "res5"], "MODEL.FPN.IN_FEATURES", ["res3", "res4", "res5"],
        "MODEL.RETINANET.NUM_CLASSES", num_classes,
        "MODEL.ANCHOR_GENERATOR.SIZES", [[x, x * 2 ** (1.0 / 3), x * 2 ** (2.0 / 3)] for x in [32, 64, 128, 256, 512]],
        "MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS", [[0.5, 1.0, 2.0]]])
    return cfg


def build(num_classes):
    from detectron2.modeling.meta_arch.retinanet import RetinaNet

    return RetinaNet(ref_cfg(num_classes)).eval()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def head_outputs(model, inputs):
    images = model.preprocess_image(inputs)
    feats = model.backbone(images.tensor)
    feats = [feats[f] for f in model.in_features]
    logits, deltas = model.head(feats)
    return images, feats, logits, deltas


def level_candidates(model, anchors_l, logits_l, deltas_l, image_size):
    """The reference's own `inference_single_image` on ONE level with the NMS replaced by a recorder: what it hands to batched_nms.
    Run twice -- as it is, and with index-coded anchors (x1 = anchor index, width 1) and zero deltas, whose decoded x1 IS the anchor
    index -- so that the flat index of every candidate is known without restating the function."""
    import detectron2.modeling.meta_arch.retinanet as ref
    from detectron2.structures import Boxes

    rec = {}

    def recorder(boxes, scores, classes, thresh):
        rec["boxes"], rec["scores"], rec["classes"] = boxes.clone(), scores.clone(), classes.clone()
        return torch.arange(len(scores))

    real = ref.batched_nms
    ref.batched_nms = recorder
    try:
        model.inference_single_image([anchors_l], [logits_l.clone()], [deltas_l], image_size)      # (the function's sigmoid_ is in place)
        boxes, scores, classes = rec["boxes"], rec["scores"], rec["classes"]
        n = len(anchors_l)
        idx = torch.arange(n, dtype=torch.float32)
        coded = Boxes(torch.stack([idx, idx, idx + 1, idx + 1], 1))
        model.inference_single_image([coded], [logits_l.clone()], [torch.zeros_like(deltas_l)], image_size)
        anchor_idx = rec["boxes"][:, 0].round().long()
        assert torch.equal(rec["scores"], scores) and torch.equal(rec["classes"], classes) and n < (1 << 24)
    finally:
        ref.batched_nms = real
    return anchor_idx * model.num_classes + classes, scores, classes, boxes


def main():
    import detectron2.modeling.meta_arch.retinanet as ref

    sd = build(80).state_dict()
    mg.save("retinanet_r50_fpn_keys", keys=np.array(list(sd.keys())), shapes=np.array([str(tuple(v.shape)) for v in sd.values()]))

    model = build(NUM_CLASSES)
    model.load_state_dict(syn.conditioned_retinanet_state_dict(model.state_dict(), seed=0), strict=True)
    model64 = copy.deepcopy(model).double()
    inputs = [{"image": syn.synthetic_image(seed, h, w), "height": h, "width": w} for h, w, seed in SIZES]
    K, thresh, topk = model.num_classes, model.score_threshold, model.topk_candidates
    d, notes = {}, []
    with torch.no_grad():
        images, feats, logits, deltas = head_outputs(model, inputs)
        _, _, logits64, deltas64 = head_outputs(model64, inputs)
        anchors = model.anchor_generator(feats)
        err_l, err_d = [], []
        for name, a, b, a64, b64 in zip(model.in_features, logits, deltas, logits64, deltas64):
            d["logits_" + name], d["deltas_" + name] = nhwc(a), nhwc(b)
            err_l.append(float((a.double() - a64).abs().max()))
            err_d.append(float((b.double() - b64).abs().max()))
            notes.append("| %s | %dx%d | %.3e | %.3e | %.3e | %.3e |" % (name, a.shape[2], a.shape[3], err_l[-1], float(a64.abs().max()), err_d[-1], float(b64.abs().max())))
        d["err64_logits"], d["err64_deltas"] = np.array(err_l), np.array(err_d)

        cand = {k: [] for k in ("index", "score", "class", "box", "level", "image")}
        rows, over, under, worst_aside, n_cand = [], 0, 0, 0.0, [0, 0]
        for i, size in enumerate(images.image_sizes):
            for l, name in enumerate(model.in_features):
                lg = ref.permute_to_N_HWA_K(logits[l], K)[i]
                dl = ref.permute_to_N_HWA_K(deltas[l], 4)[i]
                index, scores, classes, boxes = level_candidates(model, anchors[l], lg, dl, tuple(size))
                num_topk = min(topk, dl.shape[0])
                prob = lg.flatten().sigmoid()
                survivors = int((prob > thresh).sum())
                over += survivors > num_topk
                under += 1 <= survivors < num_topk
                # candidates whose membership or order rounding can decide: equal to the first excluded probability, or within 1e-6 of
                # the threshold
                srt = prob.sort(descending=True)[0]
                aside = (scores.double() - thresh).abs() <= 1e-6
                if survivors > num_topk:
                    aside |= scores == srt[num_topk]
                frac = float(aside.sum()) / max(1, len(scores))
                worst_aside = max(worst_aside, frac)
                rows.append("| %d | %s | %d | %d | %d | %d | %d |" % (i, name, lg.numel(), num_topk, survivors, len(scores), int(aside.sum())))
                n_cand[i] += len(scores)
                for k, v in zip(("index", "score", "class", "box"), (index, scores, classes, boxes)):
                    cand[k].append(v)
                cand["level"].append(torch.full((len(scores),), l, dtype=torch.int64))
                cand["image"].append(torch.full((len(scores),), i, dtype=torch.int64))
        d["cand_index"] = torch.cat(cand["index"]).to(torch.int32)
        d["cand_score"] = torch.cat(cand["score"])
        d["cand_class"] = torch.cat(cand["class"]).to(torch.int32)
        d["cand_box"] = torch.cat(cand["box"])
        d["cand_level"] = torch.cat(cand["level"]).to(torch.int8)
        d["cand_image"] = torch.cat(cand["image"]).to(torch.int8)

        out32, out64 = model(inputs), model64(inputs)
    dets = {}
    for tag, out in (("32", out32), ("64", out64)):
        dets[tag] = []
        for i, o in enumerate(out):
            inst = o["instances"]
            d["det%s_boxes_%d" % (tag, i)], d["det%s_scores_%d" % (tag, i)] = inst.pred_boxes.tensor, inst.scores
            d["det%s_classes_%d" % (tag, i)] = inst.pred_classes
            dets[tag].append((inst.pred_boxes.tensor, inst.scores, inst.pred_classes))
    n_det = [len(t[1]) for t in dets["32"]]
    top_score = max(float(t[1].max()) for t in dets["32"])

    # the reference against itself, as oracle.noise.fp32_vs_fp64(derive_identity=True) derives the identity bars
    wide = onoise.deviation(dets["32"], dets["64"], onoise.WIDE_BOX, onoise.WIDE_SCORE)
    box_tol = max(onoise.LOOSE_BOX, onoise.IDENT_K * wide["box_median"])
    score_tol = max(onoise.LOOSE_SCORE, onoise.IDENT_K * wide["score_median"])
    nz = onoise.deviation(dets["32"], dets["64"], box_tol, score_tol)
    nz["box_tol"], nz["score_tol"] = box_tol, score_tol
    consts = {"IDENT_K": onoise.IDENT_K, "WIDE_BOX": onoise.WIDE_BOX, "WIDE_SCORE": onoise.WIDE_SCORE, "FLOOR_BOX": onoise.FLOOR_BOX,
              "FLOOR_SCORE": onoise.FLOOR_SCORE, "LOOSE_BOX": onoise.LOOSE_BOX, "LOOSE_SCORE": onoise.LOOSE_SCORE}
    d["noise_keys"] = np.array(list(nz.keys()) + list(consts.keys()))
    d["noise_vals"] = np.array([float(v) for v in nz.values()] + [float(v) for v in consts.values()])

    assert over >= 1, "(a) no (image, level) has more survivors than num_topk"
    assert under >= 1, "(b) no (image, level) has between 1 and num_topk - 1 survivors"
    assert all(nd < nc for nd, nc in zip(n_det, n_cand)) and all(nd < model.max_detections_per_image for nd in n_det), \
        "(c) NMS removes no candidate (or the detections are cut at DETECTIONS_PER_IMAGE)"
    assert top_score < 1 - 1e-6, "(d) a kept score saturates"
    assert worst_aside <= 0.01, "(e) more than 1 %% of a level's candidates tie at the cut or lie at the threshold (%.3f)" % worst_aside

    mg.save("retinanet_r50_fpn_small", **d)
    size = os.path.getsize(os.path.join(mg.GOLD, "retinanet_r50_fpn_small.npz"))
    assert size <= (1 << 20), "fixture of %d bytes: the repository's limit for a committed file is 1 MiB" % size
    with open(os.path.join(mg.GOLD, "README_retinanet.md"), "w") as f:
        f.write("# retinanet_r50_fpn_small.npz: what the generator found\n\n"
                "Written by `scripts/make_golden_retinanet.py` (R50 RetinaNet, %d classes, SCORE_THRESH_TEST %.2f, TOPK_CANDIDATES_TEST %d, "
                "weights `lvc_amd.utils.synthetic.conditioned_retinanet_state_dict(seed=0)`, images 128x160 and 120x176).\n\n"
                "| image | level | entries | num_topk | above the threshold | candidates | set aside (tie at the cut / within 1e-6 of the threshold) |\n"
                "|---|---|---|---|---|---|---|\n%s\n\n"
                "- (a) (image, level) pairs with more survivors than num_topk: %d\n"
                "- (b) pairs with 1 .. num_topk - 1 survivors: %d\n"
                "- (c) candidates per image %s, detections per image %s (DETECTIONS_PER_IMAGE %d): NMS removes the rest\n"
                "- (d) largest kept score: %.6f\n"
                "- (e) largest set-aside fraction of a level's candidates: %.4f (bar 0.01)\n\n"
                "Head outputs, the fp32 model against the model run as `.double()`:\n\n"
                "| level | map | max abs err logits | max abs logit | max abs err deltas | max abs delta |\n|---|---|---|---|---|---|\n%s\n\n"
                "The reference against itself (fp32 detections vs fp64 detections, `oracle.noise.deviation` with derived identity bars):\n\n%s\n"
                % (K, thresh, topk, "\n".join(rows), over, under, n_cand, n_det, model.max_detections_per_image, top_score, worst_aside,
                   "\n".join(notes), "\n".join("- %s: %s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in nz.items())))
    print("\n".join(rows))
    print("noise", nz)


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
