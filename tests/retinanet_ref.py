"""Torch-on-the-CPU restatement of RetinaNet's per-level candidate selection as csrc/retinanet.hip defines it: per (image, level) a
STABLE descending sort of the logits (equal logits: the lower flat index first), the cap num_topk = min(topk, anchors), the fp32 sigmoid
threshold, `apply_deltas` from lvc_amd's Box2BoxTransform against the grid anchors (shift + cell anchor).  The expected
value of tests/test_gpu_retinanet.py; pinned against the reference's own function in tests/test_host_retinanet.py (fixture
tests/golden/retinanet_r50_fpn_small.npz).  No test functions here."""
import torch


def stable_topk(flat, k):
    """Indices of the first k entries of a stable descending sort of `flat` (1-D), without sorting all of it: everything above the k-th
    largest value, then the lowest indices among the entries equal to it; that selection sorted (stable, descending)."""
    n = flat.numel()
    if k >= n:
        return torch.sort(flat, descending=True, stable=True)[1]
    t = torch.topk(flat, k, sorted=True)[0][-1]
    gt = (flat > t).nonzero().flatten()
    eq = (flat == t).nonzero().flatten()[: k - gt.numel()]
    sel = torch.sort(torch.cat([gt, eq]))[0]
    return sel[torch.sort(flat[sel], descending=True, stable=True)[1]]


def select_level(logits, deltas, anchors, num_classes, topk, thresh, weights=(1.0, 1.0, 1.0, 1.0)):
    """logits [HWA, K] (or flat), deltas [HWA, 4], anchors [HWA, 4], fp32 on the CPU -> (index, score, class, box) of the level's
    candidates in selection order."""
    from lvc_amd.modeling.box_regression import Box2BoxTransform

    flat = logits.reshape(-1)
    num_topk = min(int(topk), deltas.shape[0])
    order = stable_topk(flat, num_topk)
    prob = torch.sigmoid(flat)[order]      # (over the whole tensor, as the reference: ATen's vector and tail paths round apart)
    keep = prob > thresh
    index, score = order[keep], prob[keep]
    anchor, cls = torch.div(index, num_classes, rounding_mode="floor"), index % num_classes
    boxes = Box2BoxTransform(weights=tuple(weights)).apply_deltas(deltas[anchor], anchors[anchor])
    return index, score, cls, boxes


def grid_anchors(shapes, strides, cell_anchors, offset=0.0):
    """Grid anchors per level, [H*W*A, 4] (shift + cell anchor, pixel-major: reference anchor_generator.py:157-178)."""
    out = []
    for (gh, gw), stride, base in zip(shapes, strides, cell_anchors):
        base = base.float().cpu()
        sx = torch.arange(offset * stride, gw * stride, step=stride, dtype=torch.float32)
        sy = torch.arange(offset * stride, gh * stride, step=stride, dtype=torch.float32)
        yy, xx = torch.meshgrid(sy, sx, indexing="ij")
        xx, yy = xx.reshape(-1), yy.reshape(-1)
        shifts = torch.stack((xx, yy, xx, yy), dim=1)
        out.append((shifts.view(-1, 1, 4) + base.view(1, -1, 4)).reshape(-1, 4))
    return out


def select_pyramid(logits, deltas, cell_anchors, strides, offset, num_classes, topk, thresh, weights=(1.0, 1.0, 1.0, 1.0)):
    """logits[l] [B,H,W,A*K], deltas[l] [B,H,W,4A] (CPU, dense) -> per image, per level (index, score, class, box)."""
    A = cell_anchors[0].shape[0]
    anchors = grid_anchors([t.shape[1:3] for t in logits], strides, cell_anchors, offset)
    out = []
    for b in range(logits[0].shape[0]):
        out.append([select_level(lg[b].reshape(-1, num_classes), dl[b].reshape(-1, 4)[: lg[b].numel() // num_classes], an, num_classes, topk,
                                 thresh, weights) for lg, dl, an in zip(logits, deltas, anchors)])
        assert all(lg[b].numel() == an.shape[0] * num_classes and an.shape[0] % A == 0 for lg, an in zip(logits, anchors))
    return out


def flatten_image(per_level, rows):
    """One image's per-level candidates as the kernel lays them out: level after level, densely, zero rows up to `rows`.
    -> (index int32 [rows], score [rows], class int32 [rows], box [rows,4], count)."""
    index = torch.cat([p[0] for p in per_level]).to(torch.int32)
    n = index.numel()
    pad = rows - n
    z = lambda t, shape, dt: torch.cat([t.to(dt), torch.zeros((pad,) + shape, dtype=dt)])      # noqa: E731
    return (z(index, (), torch.int32), z(torch.cat([p[1] for p in per_level]), (), torch.float32),
            z(torch.cat([p[2] for p in per_level]), (), torch.int32), z(torch.cat([p[3] for p in per_level]), (4,), torch.float32), n)
