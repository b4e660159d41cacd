"""Plain torch restatement of the two Mask R-CNN inference kernels, in any dtype (the GPU tests use fp64): the mask head's tail
(ConvTranspose2d 2x2 stride 2 + ReLU + 1x1 predictor + pick the class + sigmoid) and paste_masks_in_image's soft values.  Written
from the formulas, with no convolution or grid_sample call: tests/test_host_mask_rcnn.py checks it against torch's own operators."""
import torch


def tail(x, wd, bd, wp, bp, classes, dtype=torch.float64):
    """x [M, Cin, S, S]; wd [Cin, Cmid, 2, 2]; bd [Cmid]; wp [K, Cmid] (or [K, Cmid, 1, 1]); bp [K]; classes [M] int or None (class 0).
    -> prob [M, 2S, 2S]: prob[m, 2y+dy, 2x+dx] = sigmoid(bp[c] + sum_co relu(bd[co] + sum_ci x[m,ci,y,x] wd[ci,co,dy,dx]) wp[c,co])."""
    x, wd, bd, bp = x.to(dtype), wd.to(dtype), bd.to(dtype), bp.to(dtype)
    wp = wp.reshape(wp.shape[0], -1).to(dtype)
    M, _, S, _ = x.shape
    c = torch.zeros(M, dtype=torch.int64) if classes is None else classes.to(torch.int64)
    h = torch.einsum("miyx,iodk->myxdko", x, wd) + bd          # [M, S, S, 2(dy), 2(dx), Cmid]
    h = torch.clamp(h, min=0)
    z = torch.einsum("myxdko,mo->myxdk", h, wp[c]) + bp[c][:, None, None, None, None]
    z = z.permute(0, 1, 3, 2, 4).reshape(M, 2 * S, 2 * S)      # [M, y, dy, x, dx]
    return 1.0 / (1.0 + torch.exp(-z))


def paste_soft(prob, boxes, H, W, dtype=torch.float64):
    """prob [N, Sm, Sm], boxes [N, 4] -> the soft pasted masks [N, H, W]: bilinear samples of prob (zeros outside it) at
    ix = ((gx + 1) Sm - 1) / 2, gx = (px + 0.5 - x0) / (x1 - x0) * 2 - 1 (likewise y)."""
    prob, boxes = prob.to(dtype), boxes.to(dtype)
    N, Sm, _ = prob.shape
    x0, y0, x1, y1 = [boxes[:, i:i + 1] for i in range(4)]
    px = torch.arange(W, dtype=dtype)[None, :] + 0.5
    py = torch.arange(H, dtype=dtype)[None, :] + 0.5
    gx = (px - x0) / (x1 - x0) * 2 - 1
    gy = (py - y0) / (y1 - y0) * 2 - 1
    ix = ((gx + 1) * Sm - 1) / 2         # [N, W]
    iy = ((gy + 1) * Sm - 1) / 2         # [N, H]
    fx, fy = torch.floor(ix), torch.floor(iy)
    w, n = ix - fx, iy - fy
    e, s = 1 - w, 1 - n
    fx, fy = fx.clamp(-2, Sm).long(), fy.clamp(-2, Sm).long()
    padded = torch.zeros(N, Sm + 4, Sm + 4, dtype=dtype)      # two cells of zeros all round: every tap index is valid
    padded[:, 2:-2, 2:-2] = prob
    ar = torch.arange(N)[:, None, None]

    def tap(dy, dx):
        return padded[ar, (fy + 2 + dy)[:, :, None], (fx + 2 + dx)[:, None, :]]

    ny, sy, wx, ex = s[:, :, None], n[:, :, None], e[:, None, :], w[:, None, :]
    # weights of the four taps: north (row fy) s, south n; west (column fx) e, east w
    return tap(0, 0) * (ny * wx) + tap(0, 1) * (ny * ex) + tap(1, 0) * (sy * wx) + tap(1, 1) * (sy * ex)


def paste(prob, boxes, H, W, threshold=0.5, dtype=torch.float64):
    return paste_soft(prob, boxes, H, W, dtype) >= threshold


def paste_inputs():
    """The paste tests' inputs: smooth probabilities (sigmoid of low-pass noise, like a head's output) and twelve boxes on a 61 x 83
    image: sub-pixel sized, whole-image, touching each border, 0.6 px high, 1 x 1, at half-integer corners."""
    torch.manual_seed(0)
    z = torch.randn(12, 1, 7, 7) * 3
    p = torch.sigmoid(torch.nn.functional.interpolate(z, size=28, mode="bicubic", align_corners=False))[:, 0].contiguous()
    b = torch.tensor([[3.2, 4.7, 40.9, 50.1], [0., 0., 83., 61.], [10.5, 10.5, 11.2, 30.], [70., 50., 83., 61.], [0., 20., 83., 20.6],
                      [5.25, 5.75, 33.25, 33.75], [40., 2., 41., 3.], [-0.0, 0., 2.5, 2.5], [20., 20., 76., 48.], [1., 1., 82., 60.],
                      [30.3, 0., 55.5, 61.], [12., 30., 19.9, 37.1]])
    return p, b, (61, 83)
