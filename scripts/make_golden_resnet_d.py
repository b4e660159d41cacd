"""Generate tests/golden/resnet_d_*.npz: the reference's ResNet-D modules (RESNETS.D: `DeepStem`, `BottleneckBlockCLIP`) run on the CPU.
Runs only where the reference tree exists (as oracle/make_golden.py, whose import shim and `build_ref_model` it uses).  Only outputs
and key lists are stored; inputs and weights are regenerated from their seeds (lvc_amd.utils.synthetic).  TEST INFRASTRUCTURE ONLY.

  resnet_d_stem.npz             DeepStem(3, 64, "FrozenBN") on a seeded [2,3,37,53] image: out32, out64
  resnet_d_block_res2_0.npz     BottleneckBlockCLIP 64 -> 64 -> 256, stride 1 (projection shortcut, no pool)
  resnet_d_block_identity.npz   BottleneckBlockCLIP 256 -> 64 -> 256, stride 1 (no shortcut conv)
  resnet_d_block_proj.npz       BottleneckBlockCLIP 256 -> 128 -> 512, stride 2 (both pools); each block on a seeded [2,C,9,11] input
                                (9 -> 4 and 11 -> 5: the pools' floor): out32, out64
  resnet_d_r50_fpn_keys.npz     names + shapes of the R50-D-FPN GeneralizedRCNN's state_dict (format of r50_fpn_state_dict_keys.npz)
  resnet_d_r50_fpn_small.npz    p2..p6 of that model on two small images, in fp32 and from the backbone run as .double(), sampled
                                (p2 [:, ::16, ::2, ::2], the other levels [:, ::8])
  resnet_d_train.npz            one training step (60 classes, FREEZE_AT 2, randperm = identity) in the form of train_base.npz

    python scripts/make_golden_resnet_d.py
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

YAML = "COCO-detection/faster_rcnn_R_50_FPN_base.yaml"
R50D = ["MODEL.RESNETS.DEPTH", 50, "MODEL.RESNETS.D", True]
SIZES = ((128, 160, 3), (120, 176, 4))
STEM_SEED = 70
BLOCKS = (("resnet_d_block_res2_0", 64, 64, 256, 1, 71), ("resnet_d_block_identity", 256, 64, 256, 1, 72),
          ("resnet_d_block_proj", 256, 128, 512, 2, 73))
SAMPLE = {"p2": (16, 2), "p3": (8, 1), "p4": (8, 1), "p5": (8, 1), "p6": (8, 1)}


def stem_input(seed=STEM_SEED):
    return torch.randn(2, 3, 37, 53, generator=torch.Generator().manual_seed(seed))


def block_input(cin, seed):
    return torch.randn(2, cin, 9, 11, generator=torch.Generator().manual_seed(seed)).relu_()


def sample(k, v):
    c, s = SAMPLE[k]
    return v[:, ::c, ::s, ::s].contiguous()


def _run(name, mod, x, seed):
    mod.load_state_dict(syn.seeded_module_state_dict(mod.state_dict(), seed=seed), strict=True)
    with torch.no_grad():
        y32 = mod(x.clone())
        y64 = copy.deepcopy(mod).double()(x.double())
    print("  %s %s max |fp32 - fp64| %.3e (largest value %.3e)" % (name, tuple(y32.shape), float((y32.double() - y64).abs().max()),
                                                                  float(y64.abs().max())))
    mg.save(name, out32=y32, out64=y64)


def gen_stem_and_blocks():
    from detectron2.modeling.backbone.resnet import BottleneckBlockCLIP, DeepStem

    _run("resnet_d_stem", DeepStem(3, 64, "FrozenBN").eval(), stem_input(), STEM_SEED)
    for name, cin, width, cout, stride, seed in BLOCKS:
        blk = BottleneckBlockCLIP(cin, cout, bottleneck_channels=width, stride=stride, norm="FrozenBN").eval()
        assert (blk.shortcut is not None) == (cin != cout or stride > 1) and blk.conv2.stride == (1, 1)
        _run(name, blk, block_input(cin, seed), seed)


def gen_model():
    cfg, model = mg.build_ref_model(YAML, R50D + ["MODEL.ROI_HEADS.NUM_CLASSES", 80])
    sd = model.state_dict()
    mg.save("resnet_d_r50_fpn_keys", keys=np.array(list(sd.keys())), shapes=np.array([str(tuple(v.shape)) for v in sd.values()]))
    # (no FrozenBN calibration is stored for this trunk either: the ResNeXt recipe, conv3's norm scales its branch by 0.25)
    model.load_state_dict(syn.conditioned_resnext_state_dict(sd, seed=0), strict=True)
    inputs = [{"image": syn.synthetic_image(seed, h, w), "height": h, "width": w} for h, w, seed in SIZES]
    with torch.no_grad():
        x = model.preprocess_image(inputs).tensor
        assert x.shape[2] % 32 == 0 and x.shape[3] % 32 == 0, x.shape
        feats = model.backbone(x)
        feats64 = copy.deepcopy(model.backbone).double()(x.double())
    d = {}
    for k, v in feats.items():
        d["feat32_" + k], d["feat64_" + k] = sample(k, v), sample(k, feats64[k])
        print("  %s %s max |fp32 - fp64| %.3e on the sample (largest value %.3e)" % (k, tuple(v.shape), float((d["feat32_" + k].double() - d["feat64_" + k]).abs().max()), float(v.abs().max())))
    mg.save("resnet_d_r50_fpn_small", **d)


def gen_train():
    from detectron2.structures import Boxes, Instances
    from detectron2.utils.events import EventStorage

    cfg, model = mg.build_ref_model(YAML, R50D)
    model.load_state_dict(syn.conditioned_resnext_state_dict(model.state_dict(), seed=0), strict=True)
    model.train()
    batch, d = [], {}
    g = torch.Generator().manual_seed(9)
    for i, (h, w, seed) in enumerate(SIZES):
        n = 3 + i
        x0, y0 = torch.rand(n, generator=g) * (w - 60), torch.rand(n, generator=g) * (h - 60)
        bw, bh = 24 + torch.rand(n, generator=g) * 36, 24 + torch.rand(n, generator=g) * 36
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(torch.stack([x0, y0, x0 + bw, y0 + bh], 1))
        inst.gt_classes = torch.randint(0, 20, (n,), generator=g)
        batch.append({"image": syn.synthetic_image(seed, h, w), "instances": inst, "height": h, "width": w})
        d["gt_boxes%d" % i], d["gt_classes%d" % i] = inst.gt_boxes.tensor, inst.gt_classes
    real = torch.randperm
    torch.randperm = lambda n, **kw: torch.arange(n, **{k: v for k, v in kw.items() if k in ("device", "dtype")})
    try:
        with EventStorage(0):
            losses = model(batch)
            sum(losses.values()).backward()
    finally:
        torch.randperm = real
    frozen = []
    for n_, p_ in model.named_parameters():
        if p_.requires_grad:
            gflat = p_.grad.flatten()
            stride = max(1, gflat.numel() // 2048) | 1
            d["grad_sample." + n_] = gflat[::stride][:2048].clone()
            d["grad_stats." + n_] = torch.tensor([float(gflat.double().sum()), float(gflat.double().norm()), float(stride)], dtype=torch.float64)
        else:
            frozen.append(n_)
    print("  losses", {k: float(v.detach()) for k, v in losses.items()}, "frozen", len(frozen))
    d["frozen_names"] = np.array(frozen)
    mg.save("resnet_d_train", **d, **{"loss." + k: v.detach() for k, v in losses.items()})


if __name__ == "__main__":
    torch.manual_seed(0)
    gen_stem_and_blocks()
    gen_model()
    gen_train()
