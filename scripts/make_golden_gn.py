"""Generate tests/golden/gn_*.npz and train_gn.npz: the reference R50-FPN with GroupNorm in the pyramid and the 4conv1fc GroupNorm box
head (MODEL.FPN.NORM / MODEL.ROI_BOX_HEAD.NORM "GN", NUM_CONV 4, NUM_FC 1) run on CPU.  Runs only where the reference tree exists (as
oracle/make_golden.py, whose import shim and `build_ref_model` it uses).  Only outputs are stored; the tests regenerate inputs and
weights from their seeds (lvc_amd.utils.synthetic: the conditioned weights of the e2e fixtures, then `seeded_group_norm_affine_`,
because the conditioned recipe leaves norm weights / biases at 1 / 0).  TEST INFRASTRUCTURE ONLY.

  gn_state_dict_keys.npz  names + shapes of the model's state_dict (format of r50_fpn_state_dict_keys.npz)
  gn_fpn_small.npz        p2..p6 of the two small images of gen_e2e / fpn_avg_small, sampled [:, ::16, ::2, ::2], featstat_* rows,
                          and noise_p*: max |fp32 - fp64| of the backbone run as .double() on the same input (whole maps)
  gn_box_head.npz         FastRCNNConvFCHead (4 conv GN + 1 fc) on a seeded [5,256,7,7] input, in fp32 and fp64
  train_gn.npz            one training step at the size of train_base.npz (its batch, randperm = identity): losses, scalars, and
                          sum / L2 norm / strided sample of the gradients of every GN weight and bias and of the conv weights of
                          fpn_lateral2, fpn_output2 and box_head.conv1

    python scripts/make_golden_gn.py            # under a minute on 8 cores
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

from lvc_amd.config.presets import GN_OVERRIDES  # noqa: E402
from lvc_amd.utils import synthetic as syn  # noqa: E402

YAML = "COCO-detection/faster_rcnn_R_50_FPN_base.yaml"
BOX_HEAD_SEED = 21
CONV_GRADS = ("backbone.fpn_lateral2.weight", "backbone.fpn_output2.weight", "roi_heads.box_head.conv1.weight")


def _model(opts=()):
    cfg, model = mg.build_ref_model(YAML, list(opts) + list(GN_OVERRIDES))
    calib = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(mg.GOLD, "r50_bn_calibration.npz")).items()}
    model.load_state_dict(syn.conditioned_state_dict(model.state_dict(), seed=0, bn_calibration=calib), strict=True)
    syn.seeded_group_norm_affine_(model, seed=0)
    gns = [n for n, m in model.named_modules() if isinstance(m, torch.nn.GroupNorm)]
    assert len(gns) == 12 and all(m.num_groups == 32 for m in model.modules() if isinstance(m, torch.nn.GroupNorm)), gns
    return cfg, model


def box_head_input():
    return torch.randn(5, 256, 7, 7, generator=torch.Generator().manual_seed(BOX_HEAD_SEED))


def gen_inference():
    cfg, model = _model(["MODEL.ROI_HEADS.NUM_CLASSES", 80])
    sd = model.state_dict()
    mg.save("gn_state_dict_keys", keys=np.array(list(sd.keys())), shapes=np.array([str(tuple(v.shape)) for v in sd.values()]))
    inputs = [{"image": syn.synthetic_image(3, 240, 320), "height": 480, "width": 640},
              {"image": syn.synthetic_image(4, 200, 352), "height": 200, "width": 352}]
    with torch.no_grad():
        x = model.preprocess_image(inputs).tensor
        feats = model.backbone(x)
        feats64 = copy.deepcopy(model.backbone).double()(x.double())
    d = {}
    for k, v in feats.items():
        d["feat_" + k] = v[:, ::16, ::2, ::2].contiguous()
        d["featstat_" + k] = torch.stack([v.mean(), v.std(), v.abs().max()])
        d["noise_" + k] = (v.double() - feats64[k]).abs().max()
        print("  %s max |fp32 - fp64| %.3e (largest value %.3e)" % (k, float(d["noise_" + k]), float(v.abs().max())))
    mg.save("gn_fpn_small", **d)

    head = model.roi_heads.box_head
    assert [type(m).__name__ for m in head.conv_norm_relus] == ["Conv2d"] * 4 and len(head.fcs) == 1
    xin = box_head_input()
    with torch.no_grad():
        out32 = head(xin)
        out64 = copy.deepcopy(head).double()(xin.double())
    print("  box head max |fp32 - fp64| %.3e (largest value %.3e)" % (float((out32.double() - out64).abs().max()), float(out64.abs().max())))
    mg.save("gn_box_head", out32=out32, out64=out64)


def gen_train(sizes=((240, 320, 3), (200, 352, 4))):
    from detectron2.structures import Boxes, Instances
    from detectron2.utils.events import EventStorage

    cfg, model = _model()
    model.train()
    t = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(mg.GOLD, "train_novel_ft.npz")).items()}
    batch, d = [], {}
    for i, (h, w, seed) in enumerate(sizes):
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(t["gt_boxes%d" % i])
        inst.gt_classes = t["gt_classes%d" % i]
        batch.append({"image": syn.synthetic_image(seed, h, w), "instances": inst, "height": h, "width": w})
        d["gt_boxes%d" % i], d["gt_classes%d" % i] = inst.gt_boxes.tensor, inst.gt_classes
    real = torch.randperm
    torch.randperm = lambda n, **kw: torch.arange(n, **{k: v for k, v in kw.items() if k in ("device", "dtype")})
    try:
        with EventStorage(0) as storage:
            losses = model(batch)
            sum(losses.values()).backward()
            scalars = {k: float(v[0]) if isinstance(v, tuple) else float(v) for k, v in storage.latest().items()}
    finally:
        torch.randperm = real
    gn_params = {n + "." + leaf for n, m in model.named_modules() if isinstance(m, torch.nn.GroupNorm) for leaf in ("weight", "bias")}
    kept = []
    for n_, p_ in model.named_parameters():
        if n_ in gn_params or n_ in CONV_GRADS:
            assert p_.requires_grad and p_.grad is not None, n_
            gflat = p_.grad.flatten()
            stride = max(1, gflat.numel() // 2048) | 1
            d["grad_sample." + n_] = gflat[::stride][:2048].clone()
            d["grad_stats." + n_] = torch.tensor([float(gflat.double().sum()), float(gflat.double().norm()), float(stride)], dtype=torch.float64)
            kept.append(n_)
    assert len(kept) == 24 + len(CONV_GRADS), kept
    print("  losses", {k: float(v.detach()) for k, v in losses.items()}, scalars)
    d["grad_names"] = np.array(kept)
    mg.save("train_gn", **d, **{"loss." + k: v.detach() for k, v in losses.items()},
            **{"scalar." + k.replace("/", "."): np.float64(v) for k, v in scalars.items()})


if __name__ == "__main__":
    torch.manual_seed(0)
    gen_inference()
    gen_train()
