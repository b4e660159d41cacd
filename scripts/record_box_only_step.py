"""One training step of the box-only detector on the mask_train fixture's batch (20 classes, 128 rows per image, identity randperm): the
four losses and the bias gradients of the box predictor and the RPN head, saved as an npz.  tests/golden/mask_train_parent_box.npz is
this script run on an MI355X from the root of a checkout of the commit before the mask branch's training (1-d arrays, compressed):
what tests/test_gpu_mask_train.py::test_box_only_step_gives_the_parent_commits_bits holds later commits to.  Run from the root of the
tree to record; argv: fixture npz, output npz.  TEST INFRASTRUCTURE ONLY."""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.getcwd()
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lvc_amd.config.presets import base_rcnn_fpn  # noqa: E402
from lvc_amd.modeling import build_model  # noqa: E402
from lvc_amd.structures import Boxes, Instances  # noqa: E402
from lvc_amd.utils import synthetic as syn  # noqa: E402
from lvc_amd.utils.events import EventStorage  # noqa: E402

torch.randperm = lambda n, **kw: torch.arange(n, **{k: v for k, v in kw.items() if k in ("device", "dtype")})
g = np.load(sys.argv[1])
cfg = base_rcnn_fpn(num_classes=20)
cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 128
model = syn.conditioned_r50_fpn_(build_model(cfg)).train()
batch = []
for i, (h, w, seed) in enumerate(((128, 160, 3), (120, 176, 4))):
    inst = Instances((h, w))
    inst.gt_boxes = Boxes(torch.from_numpy(g["gt_boxes%d" % i]))
    inst.gt_classes = torch.from_numpy(g["gt_classes%d" % i])
    batch.append({"image": syn.synthetic_image(seed, h, w), "instances": inst, "height": h, "width": w})
with EventStorage(0):
    losses = model(batch)
    sum(losses.values()).backward()
d = {"loss." + k: v.detach().cpu().numpy().reshape(-1) for k, v in losses.items()}
for n, p in model.named_parameters():
    if p.grad is not None and n.endswith("bias") and ("box_predictor" in n or "rpn_head" in n):
        d["bias_grad." + n] = p.grad.cpu().numpy()
np.savez_compressed(sys.argv[2], **d)
for k in sorted(d):
    print(k, d[k].astype(np.float64).sum().hex(), d[k].tobytes()[:8].hex())
