"""Plain torch restatements of the small kernels around the descriptor network and the kNN preparation, in any dtype (the GPU tests
use fp64 for the reference and fp32 for the noise): crops, patch rows, tokens, LayerNorm, GELU, attention, row normalisation and its
backward, column mean.  Written from the formulas; tests/test_host_descriptor_ref.py checks them against torch's own modules and the
crop fixture."""
import math

import torch
import torch.nn.functional as F

from lvc_amd.wire import get_padding


# ------------------------------------------------------------------------------------------------------------------ crops
def crops(img, boxes, operation="pad", out_size=224):
    """img [C,H,W] (CPU); boxes: rows of integer (x1, y1, x2, y2), inclusive -> [K,C,out,out]: the box (operation 'context': widened
    by its own square pads and cut at the image) is sliced, zero-padded to a square and resized with nearest sampling."""
    C, H, W = img.shape
    out = []
    for x1, y1, x2, y2 in boxes:
        l, r, t, b = get_padding(y2 - y1 + 1, x2 - x1 + 1)
        if operation == "context":
            y1, x1 = max(0, y1 - t), max(0, x1 - l)
            y2, x2 = min(H, y2 + b), min(W, x2 + r)
            l, r, t, b = get_padding(y2 - y1 + 1, x2 - x1 + 1)
        elif operation != "pad":
            raise ValueError(operation)
        crop = F.pad(img[None, :, y1:y2 + 1, x1:x2 + 1], (l, r, t, b))      # a slice past the last pixel is cut by python
        out.append(F.interpolate(crop, (out_size, out_size), mode="nearest"))
    return torch.cat(out) if out else torch.empty(0, C, out_size, out_size, dtype=img.dtype)


def nearest_index(side, out):
    """The crop kernel's source index for every destination 0..out-1, in its own fp32 steps: min(floor(dst * (float(side) / float(out))),
    side - 1)."""
    s = torch.tensor(float(side), dtype=torch.float32) / torch.tensor(float(out), dtype=torch.float32)
    return torch.floor(torch.arange(out, dtype=torch.float32) * s).to(torch.int64).clamp(max=side - 1)


# --------------------------------------------------------------------------------------------------------- patches / tokens
def patchify(img, ps, kpad=None, mean=None, std=None):
    """img [B,C,H,W] -> [B * (H/ps) * (W/ps), kpad]: row (b, py, px), column c ps^2 + r ps + s, zero columns from C ps^2 to kpad.
    mean / std: the rows of (img - mean[c]) / std[c], evaluated in img's dtype."""
    B, C, H, W = img.shape
    if mean is not None:
        img = (img - torch.tensor(mean, dtype=img.dtype).view(1, C, 1, 1)) / torch.tensor(std, dtype=img.dtype).view(1, C, 1, 1)
    rows = F.unfold(img, kernel_size=ps, stride=ps).transpose(1, 2).reshape(-1, C * ps * ps)
    if kpad is not None and kpad > rows.shape[1]:
        rows = torch.cat([rows, torch.zeros(rows.shape[0], kpad - rows.shape[1], dtype=rows.dtype)], 1)
    return rows


def tokens(emb, cls, pos, B):
    """emb [B*P, D], cls [D], pos [P+1, D] -> [B*(P+1), D]: per image the class token then the patch rows, plus the positions."""
    D = emb.shape[1]
    P = emb.shape[0] // B
    return (torch.cat([cls.view(1, 1, D).expand(B, 1, D), emb.view(B, P, D)], 1) + pos.view(1, P + 1, D)).reshape(B * (P + 1), D)


# ------------------------------------------------------------------------------------------------------ LayerNorm / GELU
def layer_norm(x, w, b, eps, dtype=torch.float64):
    """Rows of x: (x - mean) / sqrt(var + eps) * w + b with the biased variance; w / b may be None."""
    x = x.to(dtype)
    mean = x.mean(1, keepdim=True)
    c = x - mean
    y = c / torch.sqrt((c * c).mean(1, keepdim=True) + eps)
    if w is not None:
        y = y * w.to(dtype)
    if b is not None:
        y = y + b.to(dtype)
    return y


def gelu(x, dtype=torch.float64):
    x = x.to(dtype)
    return x * 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


# ----------------------------------------------------------------------------------------------------------- attention
def _qkv(qkv, B, N, H, Dh, dtype):
    t = qkv.to(dtype).view(B, N, 3, H, Dh).permute(2, 0, 3, 1, 4)      # [3, B, H, N, Dh]
    return t[0], t[1], t[2]


def attention(qkv, B, N, H, Dh, scale, dtype=torch.float64):
    """qkv [B*N, 3*H*Dh] (column = which H Dh + h Dh + d) -> [B*N, H*Dh] = softmax(q k^T scale) v per image and head."""
    q, k, v = _qkv(qkv, B, N, H, Dh, dtype)
    s = (q @ k.transpose(-2, -1)) * scale
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = (p / p.sum(-1, keepdim=True)) @ v
    return o.transpose(1, 2).reshape(B * N, H * Dh)


def attention_cls(qkv, B, N, H, Dh, scale, dtype=torch.float64):
    """Row 0 (the class token) of `attention` for every image -> [B, H*Dh]."""
    q, k, v = _qkv(qkv, B, N, H, Dh, dtype)
    s = (q[:, :, :1] @ k.transpose(-2, -1)) * scale
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return ((p / p.sum(-1, keepdim=True)) @ v).reshape(B, H * Dh)


def split_logit_bound(qkv, B, N, H, Dh, scale):
    """(dS, max|v|) of the matrix-core attention's operand split, from the inputs in fp64: q scale and k enter as (fp16, fp16) pairs,
    about 2^-21 relative per product term after the three partial products, so a logit is off by at most
    dS = 2^-20 max over (query, key) of sum_d |q_d k_d| scale; a probability then by a factor within 1 +- dS and a row of
    softmax(s) v by at most 2 dS max|v|."""
    q, k, v = _qkv(qkv, B, N, H, Dh, torch.float64)
    ds = 2.0 ** -20 * float((q.abs() @ k.abs().transpose(-2, -1)).max()) * scale
    return ds, float(v.abs().max())


# ------------------------------------------------------------------------------------------------- row norm / column mean
def rownorm(x, mu=None, eps=1e-5, mode=0, dtype=torch.float64):
    """-> (y, den): y = (x - mu) / den row-wise, den = |x - mu| + eps (mode 0) or max(|x - mu|, eps) (mode 1)."""
    c = x.to(dtype)
    if mu is not None:
        c = c - mu.to(dtype)
    n = torch.sqrt((c * c).sum(1))
    den = n + eps if mode == 0 else n.clamp(min=eps)
    return c / den[:, None], den


def rownorm_backward(x, dy, eps, dtype=torch.float64):
    """Gradient w.r.t. x of sum(dy * x / (|x| + eps)) by autograd (a zero row's norm has gradient 0: the row gets dy / eps)."""
    xx = x.to(dtype).clone().requires_grad_(True)
    y = xx / (xx.norm(dim=1, keepdim=True) + eps)
    y.backward(dy.to(dtype))
    return xx.grad.detach()


def colmean(x, dtype=torch.float64):
    return x.to(dtype).sum(0) / x.shape[0]
