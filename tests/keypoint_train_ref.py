"""The keypoint branch's training path restated with torch tensor arithmetic in any dtype, written from the formulas (reference
detectron2/structures/keypoints.py _keypoints_to_heatmap, modeling/roi_heads/roi_heads.py select_proposals_with_visible_keypoints,
modeling/roi_heads/keypoint_head.py keypoint_rcnn_loss and KRCNNConvDeconvUpsampleHead.layers): no convolution, no interpolate and no
autograd call.  tests/test_host_keypoint_train.py holds it to torch's own operators and to the reference's recorded step; the GPU
tests hold the kernels to it."""
import torch


# ------------------------------------------------------------------ targets and selection
def to_heatmap(kps, boxes, size):
    """Keypoints.to_heatmap in the reference's fp32 order: kps [N, K, 3], boxes [N, 4] -> (target int64 [N, K], valid bool [N, K]).
    A box of non-positive width or height has no valid entry (the project's rule; the reference floors an inf or a NaN there)."""
    kps, boxes = kps.to(torch.float32), boxes.to(torch.float32)
    if boxes.numel() == 0:
        return torch.zeros(0, kps.shape[1], dtype=torch.int64), torch.zeros(0, kps.shape[1], dtype=torch.bool)
    x1, y1, x2, y2 = [boxes[:, i][:, None] for i in range(4)]
    real = ((x2 - x1) > 0) & ((y2 - y1) > 0)
    w = torch.where(real, x2 - x1, torch.ones_like(x1))
    h = torch.where(real, y2 - y1, torch.ones_like(y1))
    scale_x = torch.tensor(float(size), dtype=torch.float32) / w
    scale_y = torch.tensor(float(size), dtype=torch.float32) / h
    x, y = kps[:, :, 0], kps[:, :, 1]
    fx = ((x - x1) * scale_x).floor()
    fy = ((y - y1) * scale_y).floor()
    fx = torch.where(x == x2, torch.full_like(fx, size - 1), fx)
    fy = torch.where(y == y2, torch.full_like(fy, size - 1), fy)
    valid = (fx >= 0) & (fy >= 0) & (fx < size) & (fy < size) & (kps[:, :, 2] > 0) & real
    fx = torch.where(valid, fx, torch.zeros_like(fx)).long()
    fy = torch.where(valid, fy, torch.zeros_like(fy)).long()
    return (fy * size + fx) * valid.long(), valid


def selection(kps, boxes):
    """select_proposals_with_visible_keypoints: any keypoint with v >= 1 inside the box, both ends inclusive -> bool [N]."""
    kps, boxes = kps.to(torch.float32), boxes.to(torch.float32)
    x1, y1, x2, y2 = [boxes[:, i][:, None] for i in range(4)]
    real = ((x2 - x1) > 0) & ((y2 - y1) > 0)
    x, y = kps[:, :, 0], kps[:, :, 1]
    inside = (x >= x1) & (x <= x2) & (y >= y1) & (y <= y2) & (kps[:, :, 2] >= 1)
    return (inside & real).any(1)


def table_targets(boxes, matched, count, keypoints, size):
    """The batched kernel's outputs for a padded table: boxes [B, R, 4], matched int64 [B, R], count [B], keypoints: B tensors [n_b, K, 3]
    -> (target int32 [B*R, K], valid uint8, selected uint8 [B*R], sel_count int32 [B]); rows past the count are zero."""
    B, R, _ = boxes.shape
    K = keypoints[0].shape[1]
    target = torch.zeros(B * R, K, dtype=torch.int32)
    valid = torch.zeros(B * R, K, dtype=torch.uint8)
    selected = torch.zeros(B * R, dtype=torch.uint8)
    sel_count = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        c = int(count[b])
        if c == 0:
            continue
        m = matched[b, :c]
        ok = (m >= 0) & (m < keypoints[b].shape[0])
        kp = torch.zeros(c, K, 3)
        if keypoints[b].shape[0]:
            kp[ok] = keypoints[b][m[ok]]
        t, v = to_heatmap(kp, boxes[b, :c], size)
        s = selection(kp, boxes[b, :c])
        v = v & s[:, None]
        target[b * R: b * R + c] = (t * v.long()).to(torch.int32)
        valid[b * R: b * R + c] = v.to(torch.uint8)
        selected[b * R: b * R + c] = s.to(torch.uint8)
        sel_count[b] = int(s.sum())
    return target, valid, selected, sel_count


# ------------------------------------------------------------------ the head's tail
def up2_matrix(P, dtype=torch.float64):
    """U [2P, P]: the bilinear x2 upsampling (align_corners=False, source index max(0, (dst + 0.5) / 2 - 0.5), taps clamped at the
    edge) along one axis; the x2 map of a plane is U plane U^T.  Every weight is 0, 0.25, 0.75 or 1."""
    U = torch.zeros(2 * P, P, dtype=dtype)
    for o in range(2 * P):
        s = max(0.0, (o + 0.5) * 0.5 - 0.5)
        i0 = int(s)
        i1 = i0 + (1 if i0 < P - 1 else 0)
        U[o, i0] += 1.0 - (s - i0)
        U[o, i1] += s - i0
    return U


def deconv(x, w, b):
    """ConvTranspose2d(Cin, K, 4, stride 2, padding 1): x [M, Cin, S, S], w [Cin, K, 4, 4], b [K] -> [M, K, 2S, 2S];
    out[m, k, 2 iy - 1 + ky, 2 ix - 1 + kx] += x[m, ci, iy, ix] w[ci, k, ky, kx]."""
    M, _, S, _ = x.shape
    K = w.shape[1]
    out = torch.zeros(M, K, 2 * S + 2, 2 * S + 2, dtype=x.dtype)      # row oy + 1
    for ky in range(4):
        for kx in range(4):
            out[:, :, ky: ky + 2 * S: 2, kx: kx + 2 * S: 2] += torch.einsum("mcyx,ck->mkyx", x, w[:, :, ky, kx])
    return out[:, :, 1: 2 * S + 1, 1: 2 * S + 1] + b[None, :, None, None]


def upsample(low):
    """[M, K, P, P] -> the logits [M, K, 2P, 2P]."""
    U = up2_matrix(low.shape[2], low.dtype)
    return torch.einsum("oy,mkyx,px->mkop", U, low, U)


def normaliser(valid, fixed=None):
    return float(valid.sum()) if fixed is None else float(fixed)


def loss_terms(low, target, valid):
    """-> (terms [M, K] (0 where not valid), softmax [M, K, (2P)^2]) of the x2 map of low [M, K, P, P]."""
    z = upsample(low).flatten(2)
    mx = z.max(2, keepdim=True)[0]
    e = (z - mx).exp()
    s = e.sum(2, keepdim=True)
    lse = (mx + s.log())[:, :, 0]
    picked = torch.gather(z, 2, target.long().clamp(0, z.shape[2] - 1)[:, :, None])[:, :, 0]
    return (lse - picked) * valid.to(z.dtype), e / s


def loss(low, target, valid, fixed=None, weight=1.0):
    """The scalar: sum of the valid terms / normaliser x weight; 0 when nothing is valid."""
    terms, _ = loss_terms(low, target, valid)
    n = float(valid.sum())
    if n == 0:
        return terms.sum() * 0
    return terms.sum() / normaliser(valid, fixed) * weight


def grads(x, w, b, target, valid, fixed=None, weight=1.0, upstream=1.0):
    """-> dict(low, terms, loss, dlow [M, K, P, P], dx [M, Cin, S, S], dW [Cin, K, 4, 4], db [K]) of loss x upstream."""
    M, _, S, _ = x.shape
    low = deconv(x, w, b)
    P = 2 * S
    terms, soft = loss_terms(low, target, valid)
    n = float(valid.sum())
    out = {"low": low, "terms": terms, "loss": terms.sum() * 0 if n == 0 else terms.sum() / normaliser(valid, fixed) * weight}
    scale = 0.0 if n == 0 else upstream / normaliser(valid, fixed) * weight
    onehot = torch.zeros_like(soft)
    onehot.scatter_(2, target.long().clamp(0, soft.shape[2] - 1)[:, :, None], 1.0)
    g = ((soft - onehot) * valid.to(soft.dtype)[:, :, None] * scale).view(M, -1, 2 * P, 2 * P)
    U = up2_matrix(P, x.dtype)
    dlow = torch.einsum("oy,mkop,px->mkyx", U, g, U)
    pad = torch.zeros(M, dlow.shape[1], P + 2, P + 2, dtype=x.dtype)
    pad[:, :, 1: P + 1, 1: P + 1] = dlow
    dx = torch.zeros_like(x)
    dW = torch.zeros_like(w)
    for ky in range(4):
        for kx in range(4):
            tap = pad[:, :, ky: ky + P: 2, kx: kx + P: 2]      # dlow[m, k, 2 iy - 1 + ky, 2 ix - 1 + kx]
            dx += torch.einsum("mkyx,ck->mcyx", tap, w[:, :, ky, kx])
            dW[:, :, ky, kx] = torch.einsum("mcyx,mkyx->ck", x, tap)
    out.update(dlow=dlow, dx=dx, dW=dW, db=dlow.sum((0, 2, 3)))
    return out
