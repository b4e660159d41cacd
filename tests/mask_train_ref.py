"""Plain torch restatement of Mask R-CNN's training kernels, in any dtype (the GPU tests use fp64, and fp32 for the deviation their
bands and bars are made of): the mask targets (BitMasks.crop_and_resize = ROIAlign((T, T), 1.0, 0, aligned=True) on a 0/1 plane, then
>= 0.5), the mask loss with its logged counts, and every gradient of the head's tail (ConvTranspose2d 2x2 stride 2 + ReLU + 1x1
predictor + pick the ground-truth class) under that loss.  Written from the formulas, with no convolution, ROIAlign or autograd call:
tests/test_host_mask_train.py checks it against torch's own operators and against the reference's recorded run."""
import math

import torch


def grid_of(box, T):
    """The adaptive sampling grid of one box, computed in fp32 as the reference's ROIAlign_cpu.cpp does (the grid is a count: both the
    fp32 and the fp64 evaluation use this one).  -> (gh, gw)."""
    b = box.to(torch.float32)
    half = torch.tensor(0.5, dtype=torch.float32)
    sw, sh, ew, eh = b[0] - half, b[1] - half, b[2] - half, b[3] - half
    rw, rh = ew - sw, eh - sh
    if not (float(rw) >= 0 and float(rh) >= 0):
        return 0, 0
    Tf = torch.tensor(float(T), dtype=torch.float32)
    return int(math.ceil(float(rh / Tf))), int(math.ceil(float(rw / Tf)))


def _axis(start, bin_size, g, T, size, dtype):
    """Sample coordinates of one axis: -> (valid [T, g] bool, low [T, g] long, high [T, g] long, l [T, g], h [T, g]) with the
    reference's forms l = y - y_low, h = 1 - l."""
    p = torch.arange(T, dtype=dtype)[:, None]
    i = torch.arange(g, dtype=dtype)[None, :]
    y = start + p * bin_size + (i + 0.5) * bin_size / g
    valid = ~((y < -1.0) | (y > size))
    y = torch.where(y <= 0, torch.zeros_like(y), y)
    low = y.to(torch.int64)
    top = low >= size - 1
    low = torch.where(top, torch.full_like(low, size - 1), low)
    high = torch.where(top, low, low + 1)
    y = torch.where(top, low.to(dtype), y)
    ly = y - low.to(dtype)
    hy = 1.0 - ly
    return valid, low.clamp(0, size - 1), high.clamp(0, size - 1), ly, hy


def target_average(plane, box, T, dtype=torch.float64):
    """plane [H, W] bool, box [4] (x0, y0, x1, y1, fp32 values) -> the ROIAlign averages [T, T] in `dtype`, every operation rounded in
    `dtype` and in the reference's order: per sample w1 v1 + w2 v2 + w3 v3 + w4 v4 (w1 = hy hx, w2 = hy lx, w3 = ly hx, w4 = ly lx),
    samples added iy-major, one division by max(gh gw, 1); a sample outside [-1, H] x [-1, W] adds nothing but counts."""
    H, W = plane.shape
    gh, gw = grid_of(box, T)
    out = torch.zeros(T, T, dtype=dtype)
    if gh == 0 or gw == 0:
        return out
    v = plane.to(dtype)
    b = box.to(torch.float32).to(dtype)
    sw, sh, ew, eh = b[0] - 0.5, b[1] - 0.5, b[2] - 0.5, b[3] - 0.5
    rw, rh = ew - sw, eh - sh
    vy, yl, yh, ly, hy = _axis(sh, rh / T, gh, T, H, dtype)
    vx, xl, xh, lx, hx = _axis(sw, rw / T, gw, T, W, dtype)
    for iy in range(gh):
        for ix in range(gw):
            a, c = (yl[:, iy][:, None], yh[:, iy][:, None]), (xl[:, ix][None, :], xh[:, ix][None, :])
            wly, why, wlx, whx = ly[:, iy][:, None], hy[:, iy][:, None], lx[:, ix][None, :], hx[:, ix][None, :]
            w1, w2, w3, w4 = why * whx, why * wlx, wly * whx, wly * wlx
            val = w1 * v[a[0], c[0]] + w2 * v[a[0], c[1]] + w3 * v[a[1], c[0]] + w4 * v[a[1], c[1]]
            ok = vy[:, iy][:, None] & vx[:, ix][None, :]
            out = out + torch.where(ok, val, torch.zeros_like(val))
    return out / max(gh * gw, 1)


def targets(planes, boxes, T):
    """planes: N planes [H, W] bool, boxes [N, 4] -> (bits bool [N, T, T] from the fp64 averages, band bool [N, T, T], deviation, the
    fp32 evaluation's bits): `band` marks the pixels whose fp64 average lies within 3 x `deviation` of 0.5, `deviation` being the
    expression's own max |fp32 - fp64| on these inputs -- there the fp32 result may fall on either side."""
    a64 = torch.stack([target_average(p, b, T, torch.float64) for p, b in zip(planes, boxes)]) if len(boxes) else torch.zeros(0, T, T, dtype=torch.float64)
    a32 = torch.stack([target_average(p, b, T, torch.float32) for p, b in zip(planes, boxes)]) if len(boxes) else torch.zeros(0, T, T)
    dev = float((a32.double() - a64).abs().max()) if len(boxes) else 0.0
    return a64 >= 0.5, (a64 - 0.5).abs() <= 3 * dev, dev, a32 >= 0.5


def loss(z, t, dtype=torch.float64):
    """z [M, P, P] logits, t [M, P, P] bool -> (sum, mean, (incorrect, positive, false positive) pixel counts): each term
    max(z, 0) - z t + log1p(exp(-|z|)); the mean of no pixel is 0."""
    zz, tt = z.to(dtype), t.to(dtype)
    terms = torch.clamp(zz, min=0) - zz * tt + torch.log1p(torch.exp(-zz.abs()))
    s = terms.sum()
    tb = t.bool()
    bad = (z > 0) != tb
    return s, (s / terms.numel() if terms.numel() else s * 0), (int(bad.sum()), int(tb.sum()), int((bad & ~tb).sum()))


def scalars(counts, numel):
    """The reference's logged scalars (mask_head.py:88-100) from the three counts."""
    bad, pos, fp = [float(c) for c in counts]
    return {"mask_rcnn/accuracy": 1 - bad / max(float(numel), 1.0), "mask_rcnn/false_positive": fp / max(float(numel) - pos, 1.0),
            "mask_rcnn/false_negative": (bad - fp) / max(pos, 1.0)}


def tail_logits(x, wd, bd, wp, bp, classes, dtype=torch.float64):
    """As mask_ref.tail without the sigmoid.  -> (z [M, 2S, 2S], pre-activation hidden [M, S, S, 2, 2, Cmid], class index [M])."""
    x, wd, bd, bp = x.to(dtype), wd.to(dtype), bd.to(dtype), bp.to(dtype)
    wp = wp.reshape(wp.shape[0], -1).to(dtype)
    M, _, S, _ = x.shape
    c = torch.zeros(M, dtype=torch.int64) if classes is None else classes.to(torch.int64)
    pre = torch.einsum("miyx,iodk->myxdko", x, wd) + bd
    z = torch.einsum("myxdko,mo->myxdk", torch.clamp(pre, min=0), wp[c]) + bp[c][:, None, None, None, None]
    return z.permute(0, 1, 3, 2, 4).reshape(M, 2 * S, 2 * S), pre, c


def grads(x, wd, bd, wp, bp, classes, t, upstream=1.0, dtype=torch.float64, z=None):
    """Every gradient of upstream * mean BCE(z[gt class], t) through predictor, ReLU and the transposed convolution, from the formulas:
    dz = (sigmoid(z) - t) upstream / N;  dbp[k] = sum of dz over the RoIs of class k;  dWp[k, o] = sum dz h;
    dh = dz Wp[c, o] [pre > 0];  dbd = sum dh;  dWd[i, o, dy, dx] = sum x dh;  dx = sum dh Wd.
    -> dict(dx [M, Cin, S, S], dWd, dbd, dWp [K, Cmid], dbp [K]).  `z`: logits to form dz from instead of the restatement's own."""
    zr, pre, c = tail_logits(x, wd, bd, wp, bp, classes, dtype)
    M, _, S, _ = x.shape
    K_ = wp.shape[0]
    z = zr if z is None else z.to(dtype)
    n = z.numel()
    dz = (1.0 / (1.0 + torch.exp(-z)) - t.to(dtype)) * upstream / max(n, 1)
    dz = dz.reshape(M, S, 2, S, 2).permute(0, 1, 3, 2, 4)          # [M, y, x, dy, dx]
    h = torch.clamp(pre, min=0)
    wp2 = wp.reshape(K_, -1).to(dtype)
    dbp = torch.zeros(K_, dtype=dtype).index_add_(0, c, dz.sum(dim=(1, 2, 3, 4)))
    dwp = torch.zeros(K_, wp2.shape[1], dtype=dtype).index_add_(0, c, torch.einsum("myxdk,myxdko->mo", dz, h))
    dh = dz[..., None] * wp2[c][:, None, None, None, None, :] * (pre > 0).to(dtype)
    return {"dx": torch.einsum("myxdko,iodk->miyx", dh, wd.to(dtype)), "dWd": torch.einsum("miyx,myxdko->iodk", x.to(dtype), dh),
            "dbd": dh.sum(dim=(0, 1, 2, 3, 4)), "dWp": dwp, "dbp": dbp}


def ellipse_masks(n, H, W, seed):
    """Seeded ground-truth planes [n, H, W] bool: each the union of one to three ellipses."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.arange(H, dtype=torch.float32)[:, None]
    xx = torch.arange(W, dtype=torch.float32)[None, :]
    out = torch.zeros(n, H, W, dtype=torch.bool)
    for i in range(n):
        for _ in range(1 + int(torch.randint(0, 3, (1,), generator=g))):
            r = torch.rand(4, generator=g)
            cy, cx = float(r[0]) * H, float(r[1]) * W
            ry, rx = 2.0 + float(r[2]) * H * 0.4, 2.0 + float(r[3]) * W * 0.4
            out[i] |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return out
