"""What the box, mask and keypoint branches compute, as 1-d arrays: tests/golden/heads_parent.npz is this script run on an MI355X from
the root of a checkout of the commit before the three branches were put on one path, and tests/test_gpu_heads_parent.py -- which runs the
functions below on the tree under test -- holds later commits to it.  Recorded, on the models and inputs of tests/test_gpu_mask_rcnn.py,
tests/test_gpu_keypoint_rcnn.py and tests/test_gpu_mask_train.py (conditioned weights, TEST.DETECTIONS_PER_IMAGE = 20, two synthetic
images of 128x160 and 120x176; the mask_train fixture's batch with 128 rows per image and identity randperm):
  `inference_case`: each of the three models with do_postprocess True and False, the mask and keypoint models also through
                    inference(detected_instances=...): counts, boxes, scores, classes and pred_masks / pred_keypoints;
  `state_dict_keys`: list(model.state_dict()) of the three models;
  `train_case`:     one step of the mask model on the deferred path and with GeneralizedRCNN.deferred_reads = False: every loss, the bias
                    gradients of the box predictor and the mask predictor, mask_head.deconv.weight.grad, the latest EventStorage scalars.
Every case runs twice, on freshly built models: `exact_names` lists the arrays the two runs gave bit for bit, `margin_names` those they
did not (held to 1e-6 of the array's largest entry by the test).  Boolean masks are packed with np.packbits; a reproduced array of more
than 64 KiB is stored as the SHA-256 of its bytes (`digest`), which holds every bit of it.
tests/golden/heads_train_parent.npz is `record_train` run the same way on the commit before the mask and keypoint TRAINING branches
were put on one path: `keypoint_train_case` (the keypoint_train fixture's batch: every loss, the box predictor's bias gradients,
score_lowres.weight.grad and .bias.grad, the scalars) at the full quota, and both `*train_case`s with POST_NMS_TOPK_TRAIN = SHORT_TOPK,
where no image fills its 128 rows and the deferred step falls back to the per-image heads.
Run from the root of the tree to record; argv: the mask_train fixture npz, output npz -- or `--train`, the mask_train and the
keypoint_train fixture npz, output npz (the training cases of heads_train_parent.npz only).  TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np
import torch

SIZES = ((128, 160, 3), (120, 176, 4))
MODELS = ("box", "mask", "keypoint")
BATCH_SIZE_PER_IMAGE = 128
SHORT_TOPK = 64     # proposals per image that leave every image short of BATCH_SIZE_PER_IMAGE sampled rows
DIGEST, DIGEST_BYTES = "sha256.", 1 << 16


def digest(a):
    """What the fixture stores under DIGEST + name for a large array held bit for bit (mask_head.deconv.weight.grad is 1 MiB)."""
    import hashlib

    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def build_model(name):
    """The eval-mode models of the inference cases, as the test modules' `model` fixtures build them."""
    from lvc_amd.config import presets
    from lvc_amd.modeling import build_model as build
    from lvc_amd.utils import synthetic as syn

    cfg = {"box": lambda: presets.base_rcnn_fpn(num_classes=20), "mask": lambda: presets.mask_rcnn_fpn(num_classes=20),
           "keypoint": presets.keypoint_rcnn_fpn}[name]()
    cfg.TEST.DETECTIONS_PER_IMAGE = 20
    load = {"box": syn.conditioned_r50_fpn_, "mask": syn.conditioned_mask_head_, "keypoint": syn.conditioned_keypoint_head_}[name]
    return load(build(cfg).eval())


def build_train_model(topk=None):
    from lvc_amd.config.presets import mask_rcnn_fpn
    from lvc_amd.modeling import build_model as build
    from lvc_amd.utils import synthetic as syn

    cfg = mask_rcnn_fpn(num_classes=20)
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = BATCH_SIZE_PER_IMAGE
    if topk is not None:
        cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN = topk
    return syn.conditioned_mask_head_(build(cfg)).train().enable_mask_training()


def build_keypoint_train_model(topk=None):
    """The training model of tests/test_gpu_keypoint_train.py."""
    from lvc_amd.config.presets import keypoint_rcnn_fpn
    from lvc_amd.modeling import build_model as build
    from lvc_amd.utils import synthetic as syn

    cfg = keypoint_rcnn_fpn(num_classes=1)
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = BATCH_SIZE_PER_IMAGE
    if topk is not None:
        cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN = topk
    return syn.conditioned_keypoint_head_(build(cfg)).train().enable_keypoint_training()


def inputs():
    from lvc_amd.utils import synthetic as syn

    return [{"image": syn.synthetic_image(seed, h, w), "height": h, "width": w} for h, w, seed in SIZES]


def _flat(t):
    a = t.detach().cpu().numpy()
    return np.packbits(a.reshape(-1)) if a.dtype == np.bool_ else np.ascontiguousarray(a.reshape(-1))


def _instances(tag, insts, extra):
    d = {tag + ".counts": np.array([len(r) for r in insts], dtype=np.int64)}
    for i, r in enumerate(insts):
        d["%s.boxes%d" % (tag, i)] = _flat(r.pred_boxes.tensor)
        d["%s.scores%d" % (tag, i)] = _flat(r.scores)
        d["%s.classes%d" % (tag, i)] = _flat(r.pred_classes)
        if extra is not None:
            d["%s.%s%d" % (tag, extra, i)] = _flat(r.get(extra))
    return d


def inference_case(name, model):
    """-> {"<name>.post1.*", "<name>.post0.*", and for the mask and keypoint models "<name>.given.*"}; the given boxes are the
    detections of the do_postprocess=False run (network coordinates)."""
    from lvc_amd.structures import Boxes, Instances

    extra = {"box": None, "mask": "pred_masks", "keypoint": "pred_keypoints"}[name]
    d = {}
    with torch.no_grad():
        out = model.inference(inputs(), do_postprocess=True)
        d.update(_instances(name + ".post1", [o["instances"] for o in out], extra))
        raw = model.inference(inputs(), do_postprocess=False)
        d.update(_instances(name + ".post0", raw, extra))
        if extra is not None:
            det = []
            for r in raw:
                inst = Instances(r.image_size)
                inst.pred_boxes = Boxes(r.pred_boxes.tensor.clone())
                inst.scores = r.scores.clone()
                inst.pred_classes = r.pred_classes.clone()
                det.append(inst)
            out = model.inference(inputs(), detected_instances=det)
            d.update(_instances(name + ".given", [o["instances"] for o in out], extra))
    return d


def state_dict_keys(name, model):
    return {"keys." + name: np.array(list(model.state_dict()))}


def train_batch(g):
    """The mask_train fixture's batch (g: the npz as numpy arrays or tensors)."""
    from lvc_amd.structures import BitMasks, Boxes, Instances
    from lvc_amd.utils import synthetic as syn

    batch = []
    for i, (h, w, seed) in enumerate(SIZES):
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(torch.as_tensor(np.asarray(g["gt_boxes%d" % i])))
        inst.gt_classes = torch.as_tensor(np.asarray(g["gt_classes%d" % i]))
        n = len(inst.gt_classes)
        planes = np.unpackbits(np.asarray(g["gt_masks%d" % i]))[: n * h * w].reshape(n, h, w)
        inst.gt_masks = BitMasks(torch.from_numpy(planes).bool())
        batch.append({"image": syn.synthetic_image(seed, h, w), "instances": inst, "height": h, "width": w})
    return batch


def keypoint_train_batch(g):
    """The keypoint_train fixture's batch (g: the npz as numpy arrays or tensors)."""
    from lvc_amd.structures import Boxes, Instances, Keypoints
    from lvc_amd.utils import synthetic as syn

    batch = []
    for i, (h, w, seed) in enumerate(SIZES):
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(torch.as_tensor(np.asarray(g["gt_boxes%d" % i])))
        inst.gt_classes = torch.as_tensor(np.asarray(g["gt_classes%d" % i]))
        inst.gt_keypoints = Keypoints(torch.as_tensor(np.asarray(g["gt_keypoints%d" % i])).clone())
        batch.append({"image": syn.synthetic_image(seed, h, w), "instances": inst, "height": h, "width": w})
    return batch


def train_case(model, g, deferred, tag="train"):
    """One step of the mask model -> {"<tag>.deferred<0|1>.*"}: losses, the bias gradients of the box and mask predictors,
    mask_head.deconv.weight.grad, scalars."""
    return _step_case(tag, model, train_batch(g), deferred, lambda n: n == "roi_heads.mask_head.deconv.weight"
                      or (n.endswith("bias") and ("box_predictor" in n or "mask_head.predictor" in n)))


def keypoint_train_case(model, g, deferred, tag="keypoint_train"):
    """One step of the keypoint model -> {"<tag>.deferred<0|1>.*"}: losses, the bias gradients of the box predictor,
    score_lowres.weight.grad and score_lowres.bias.grad, scalars."""
    return _step_case(tag, model, keypoint_train_batch(g), deferred,
                      lambda n: "keypoint_head.score_lowres." in n or (n.endswith("bias") and "box_predictor" in n))


def _step_case(tag, model, batch, deferred, recorded):
    """One step (forward + backward of the summed losses) with torch.randperm = arange; recorded(name): whether a parameter's
    gradient is recorded."""
    from lvc_amd.modeling.meta_arch.rcnn import GeneralizedRCNN
    from lvc_amd.utils.events import EventStorage

    tag = "%s.deferred%d" % (tag, int(deferred))
    randperm, was = torch.randperm, GeneralizedRCNN.deferred_reads
    torch.randperm = lambda n, **kw: torch.arange(n, **{k: v for k, v in kw.items() if k in ("device", "dtype")})
    GeneralizedRCNN.deferred_reads = bool(deferred)
    try:
        for p in model.parameters():
            p.grad = None
        with EventStorage(0) as storage:
            losses = model(batch)
            sum(losses.values()).backward()
            scalars = {k: (v[0] if isinstance(v, tuple) else v) for k, v in storage.latest().items()}
    finally:
        torch.randperm, GeneralizedRCNN.deferred_reads = randperm, was
    d = {"%s.loss.%s" % (tag, k): _flat(v).reshape(-1) for k, v in losses.items()}
    for n, p in model.named_parameters():
        if p.grad is not None and recorded(n):
            d["%s.grad.%s" % (tag, n)] = _flat(p.grad)
    for k, v in scalars.items():
        d["%s.scalar.%s" % (tag, k)] = np.array([float(v)], dtype=np.float64)
    return d


def record(g):
    d = {}
    for name in MODELS:
        model = build_model(name)
        d.update(state_dict_keys(name, model))
        d.update(inference_case(name, model))
    model = build_train_model()
    for deferred in (True, False):
        d.update(train_case(model, g, deferred))
    return d


TRAIN_CASES = (("keypoint_train", "keypoint", None), ("keypoint_short", "keypoint", SHORT_TOPK), ("mask_short", "mask", SHORT_TOPK))


def build_train_case_model(case):
    _tag, kind, topk = next(c for c in TRAIN_CASES if c[0] == case)
    return (build_keypoint_train_model if kind == "keypoint" else build_train_model)(topk)


def run_train_case(case, model, gm, gk, deferred):
    """gm / gk: the mask_train / keypoint_train fixture."""
    _tag, kind, _topk = next(c for c in TRAIN_CASES if c[0] == case)
    return keypoint_train_case(model, gk, deferred, tag=case) if kind == "keypoint" else train_case(model, gm, deferred, tag=case)


def record_train(gm, gk):
    d = {}
    for case, _kind, _topk in TRAIN_CASES:
        model = build_train_case_model(case)
        for deferred in (True, False):
            d.update(run_train_case(case, model, gm, gk, deferred))
    return d


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.getcwd())
    if sys.argv[1] == "--train":
        gm, gk = np.load(sys.argv[2]), np.load(sys.argv[3])
        del sys.argv[1:3]
        a, b = record_train(gm, gk), record_train(gm, gk)
    else:
        g = np.load(sys.argv[1])
        a, b = record(g), record(g)
    assert list(a) == list(b)
    exact = [k for k in a if a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()]
    margin = [k for k in a if k not in exact]
    for k in a:
        print("%-6s %-70s %-8s %6d %s" % ("exact" if k in exact else "MARGIN", k, a[k].dtype, a[k].size, a[k].tobytes()[:8].hex()))
    for k in margin:
        x, y = a[k].astype(np.float64), b[k].astype(np.float64)
        print("not reproduced:", k, "shapes", a[k].shape, b[k].shape,
              "max |a - b| / max |a| = %.3e" % (np.abs(x - y).max() / max(np.abs(x).max(), 1e-300)) if x.shape == y.shape else "")
    # an array of more than DIGEST_BYTES that the two runs gave bit for bit is stored as the SHA-256 of its bytes
    big = [k for k in exact if a[k].dtype.kind == "f" and a[k].nbytes > DIGEST_BYTES]
    stored = {(DIGEST + k if k in big else k): (digest(a[k]) if k in big else a[k]) for k in a}
    np.savez_compressed(sys.argv[2], exact_names=np.array(exact), margin_names=np.array(margin, dtype="U128"), **stored)
    print("arrays %d, not reproduced %d, file %d bytes" % (len(a), len(margin), os.path.getsize(sys.argv[2])))
