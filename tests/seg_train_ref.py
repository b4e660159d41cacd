"""Plain-torch restatements of what csrc/sem_seg_train.hip computes, without autograd: the adjoint of the bilinear x2 upsample, and the
mean cross entropy of the x`scale` bilinear interpolation of stride-`scale` logits with both of its by-products (the per-pixel
log-sum-exp map, the gradient with respect to the logits).  Everything runs in the dtype of its input (the tests use float64);
tests/test_host_panoptic_train.py holds it against torch's own autograd of F.interpolate + F.cross_entropy."""
import torch


def tap_matrix(scale, n_out, size, dtype=torch.float64):
    """[n_out, size]: row d holds the two bilinear weights of output d (align_corners=False, ATen's coordinates with the scale
    1 / scale_factor): s = max(scale (d + 0.5) - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, size - 1), w1 = s - i0, w0 = 1 - w1."""
    d = torch.arange(n_out, dtype=dtype)
    s = (torch.as_tensor(scale, dtype=dtype) * (d + 0.5) - 0.5).clamp(min=0)
    i0 = s.floor().long().clamp(max=size - 1)
    i1 = (i0 + 1).clamp(max=size - 1)
    w1 = s - i0.to(dtype)
    A = torch.zeros(n_out, size, dtype=dtype)
    A.scatter_add_(1, i0[:, None], (1 - w1)[:, None])
    A.scatter_add_(1, i1[:, None], w1[:, None])
    return A


def upsample2(x):
    """x [N,H,W,C] -> [N,2H,2W,C]."""
    N, H, W, C = x.shape
    Ay, Ax = tap_matrix(0.5, 2 * H, H, x.dtype), tap_matrix(0.5, 2 * W, W, x.dtype)
    return torch.einsum("yh,nhwc,xw->nyxc", Ay, x, Ax)


def upsample2_backward(dy):
    """The adjoint: dy [N,2H,2W,C] -> dx [N,H,W,C]."""
    N, H2, W2, C = dy.shape
    Ay, Ax = tap_matrix(0.5, H2, H2 // 2, dy.dtype), tap_matrix(0.5, W2, W2 // 2, dy.dtype)
    return torch.einsum("yh,nyxc,xw->nhwc", Ay, dy, Ax)


def padded_labels(labels, H, W, ignore_value):
    """ImageList.from_tensors(labels, pad_value=ignore_value): a list of [h_i, w_i] integer maps -> int64 [N, H, W]."""
    out = torch.full((len(labels), H, W), int(ignore_value), dtype=torch.int64)
    for i, m in enumerate(labels):
        out[i, : m.shape[0], : m.shape[1]] = m.long()
    return out


def interpolate(low, scale):
    """low [N,h,w,K] -> z [N, scale h, scale w, K]."""
    N, h, w, K = low.shape
    Ay, Ax = tap_matrix(1.0 / scale, scale * h, h, low.dtype), tap_matrix(1.0 / scale, scale * w, w, low.dtype)
    return torch.einsum("yh,nhwk,xw->nyxk", Ay, low, Ax)


def loss(low, labels, scale, ignore_value, upstream=1.0):
    """low [N,h,w,K] (only the classes), labels: a list of N integer maps, each at most [scale h, scale w] (the rest counts as
    ignore_value).  -> dict: z [N,H,W,K], lse [N,H,W], pixel [N,H,W] (lse - z_t, 0 where not valid), valid [N,H,W] bool, count, sum,
    mean (NaN without a valid pixel), dlow [N,h,w,K] = d (upstream * mean) / d low."""
    N, h, w, K = low.shape
    H, W = scale * h, scale * w
    t = padded_labels(labels, H, W, ignore_value)
    valid = t != ignore_value
    assert bool(((t[valid] >= 0) & (t[valid] < K)).all()), "a label out of range"
    z = interpolate(low, scale)
    m = z.max(dim=-1).values
    lse = m + (z - m[..., None]).exp().sum(-1).log()
    tt = torch.where(valid, t, torch.zeros_like(t))
    zt = z.gather(-1, tt[..., None])[..., 0]
    pixel = torch.where(valid, lse - zt, torch.zeros_like(lse))
    count = int(valid.sum())
    total = pixel.sum()
    mean = total / count if count else total * float("nan")
    dz = (z - lse[..., None]).exp()
    dz.scatter_add_(-1, tt[..., None], -torch.ones_like(lse)[..., None])
    dz = dz * valid[..., None].to(low.dtype) * (upstream / count if count else float("nan"))
    Ay, Ax = tap_matrix(1.0 / scale, H, h, low.dtype), tap_matrix(1.0 / scale, W, w, low.dtype)
    dlow = torch.einsum("yh,nyxk,xw->nhwk", Ay, dz, Ax)
    return {"z": z, "lse": lse, "pixel": pixel, "valid": valid, "count": count, "sum": total, "mean": mean, "dlow": dlow}
