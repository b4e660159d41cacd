"""Plain torch-CPU mirror of RetinaNet's training loss (reference detectron2/modeling/meta_arch/retinanet.py:184-282 with
pairwise_iou, Matcher, Box2BoxTransform.get_deltas and fvcore's sigmoid_focal_loss / smooth_l1_loss), in float64 or float32: the
expected value of tests/test_gpu_retinanet_loss.py and tests/test_gpu_retinanet_train.py.  TEST INFRASTRUCTURE ONLY -- the product is
csrc/retinanet_loss.hip."""
import torch
import torch.nn.functional as F


def pairwise_iou(gt, anchors):
    """[G,4] x [R,4] -> [G,R], in the dtype of the inputs (detectron2/structures/boxes.py:315-347)."""
    a1 = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    a2 = (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
    wh = (torch.min(gt[:, None, 2:], anchors[:, 2:]) - torch.max(gt[:, None, :2], anchors[:, :2])).clamp(min=0)
    inter = wh.prod(dim=2)
    return torch.where(inter > 0, inter / (a1[:, None] + a2 - inter), torch.zeros(1, dtype=inter.dtype))


def matcher(q, thresholds=(0.4, 0.5), labels=(0, -1, 1), allow_low_quality_matches=True):
    """detectron2/modeling/matcher.py:61-126 -> (matches [R] int64, match labels [R] int8)."""
    R = q.shape[1]
    if q.shape[0] == 0:
        return torch.zeros(R, dtype=torch.int64), torch.full((R,), labels[0], dtype=torch.int8)
    vals, matches = q.max(dim=0)
    out = torch.full((R,), 1, dtype=torch.int8)
    th = [-float("inf")] + list(thresholds) + [float("inf")]
    for lab, lo, hi in zip(labels, th[:-1], th[1:]):
        out[(vals >= lo) & (vals < hi)] = lab
    if allow_low_quality_matches:
        best = q.max(dim=1)[0]
        out[(q == best[:, None]).any(0)] = 1
    return matches, out


def label_anchors(anchors, gt_boxes, gt_classes, num_classes, thresholds=(0.4, 0.5), labels=(0, -1, 1)):
    """anchors [R,4]; gt_boxes / gt_classes: per-image lists -> (gt_labels int64 [N,R] in {-1, 0..K}, matched gt index int64 [N,R],
    match labels int8 [N,R])."""
    gl, mi, ml = [], [], []
    for boxes, classes in zip(gt_boxes, gt_classes):
        m, lab = matcher(pairwise_iou(boxes.float(), anchors.float()), thresholds, labels)
        if len(boxes):
            g = classes.long()[m].clone()
            g[lab == 0] = num_classes
            g[lab == -1] = -1
        else:
            g = torch.full((anchors.shape[0],), num_classes, dtype=torch.int64)
        gl.append(g)
        mi.append(m)
        ml.append(lab)
    return torch.stack(gl), torch.stack(mi), torch.stack(ml)


def ema(normalizer, num_pos, momentum=0.9):
    """The reference's Python float recurrence, operation by operation."""
    return momentum * normalizer + (1 - momentum) * max(num_pos, 1)


def get_deltas(src, dst, weights):
    wx, wy, ww, wh = weights
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    scx, scy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = dst[:, 2] - dst[:, 0], dst[:, 3] - dst[:, 1]
    tcx, tcy = dst[:, 0] + 0.5 * tw, dst[:, 1] + 0.5 * th
    return torch.stack((wx * (tcx - scx) / sw, wy * (tcy - scy) / sh, ww * torch.log(tw / sw), wh * torch.log(th / sh)), dim=1)


def sigmoid_focal_loss_sum(x, t, alpha, gamma):
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    loss = ce * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss.sum()


def smooth_l1_sum(x, t, beta):
    n = (x - t).abs()
    if beta < 1e-5:
        return n.sum()
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta).sum()


def losses(logits, deltas, anchors, gt_labels, matched_boxes, num_classes, alpha, gamma, beta, weights, normalizer, dtype=torch.float64):
    """logits: list of [N, H_l W_l A, K]; deltas: list of [N, H_l W_l A, 4] (leaf tensors may require grad); anchors [R,4]; gt_labels
    [N,R] in {-1, 0..K}; matched_boxes [N,R,4]; normalizer: the value both sums are divided by.
    -> (loss_cls, loss_box_reg, sum_cls, sum_box) in `dtype`."""
    x = torch.cat([t.to(dtype) for t in logits], dim=1)
    d = torch.cat([t.to(dtype) for t in deltas], dim=1)
    valid = gt_labels >= 0
    pos = valid & (gt_labels != num_classes)
    target = F.one_hot(gt_labels[valid], num_classes=num_classes + 1)[:, :-1].to(dtype)
    s_cls = sigmoid_focal_loss_sum(x[valid], target, alpha, gamma)
    a = anchors.to(dtype)[None].expand(gt_labels.shape[0], -1, -1)
    tgt = get_deltas(a[pos], matched_boxes.to(dtype)[pos], weights)
    s_box = smooth_l1_sum(d[pos], tgt, beta)
    nz = torch.tensor(normalizer, dtype=dtype)
    return s_cls / nz, s_box / nz, s_cls, s_box
