"""Plain torch / numpy restatements of the keypoint branch's operators, in the dtype of their inputs (fp32 or fp64), on the CPU:

  deconv4x4_s2_p1     ConvTranspose2d(Cin, K, 4, stride 2, padding 1) + bias on channels-last maps, as explicit sums
  bilinear_up2        F.interpolate(scale_factor=2, mode="bilinear", align_corners=False): ATen's clamped source index
  bicubic_resize      F.interpolate(size=(h, w), mode="bicubic", align_corners=False): A = -0.75, unclamped source index, clamped taps,
                      x first, then y
  heatmaps_to_keypoints   detectron2/structures/keypoints.py:145-212 with the tie rule written out: among equal maxima the LOWEST flat
                      index y * w + x wins (what torch.argmax does on the CPU)
  xy_from_position    the reference's fp32 expressions for (x, y) in numpy, one rounding per operation

tests/test_host_keypoint_rcnn.py holds them to F.conv_transpose2d, F.interpolate and the reference's stored outputs."""
import numpy as np
import torch


def deconv4x4_s2_p1(x_nhwc, weight, bias=None):
    """x [M, S, S, Cin]; weight [Cin, K, 4, 4]; -> [M, K, 2S, 2S].  out[oy, ox] += x[iy, ix] W[ky, kx], oy = 2 iy - 1 + ky."""
    M, S, _, _cin = x_nhwc.shape
    K = weight.shape[1]
    out = x_nhwc.new_zeros(M, K, 2 * S + 2, 2 * S + 2)      # one pixel of margin: position o + 1
    for ky in range(4):
        for kx in range(4):
            contrib = torch.einsum("myxc,ck->mkyx", x_nhwc, weight[:, :, ky, kx])
            out[:, :, ky: ky + 2 * S: 2, kx: kx + 2 * S: 2] += contrib      # o + 1 = 2 i + k
    out = out[:, :, 1: 2 * S + 1, 1: 2 * S + 1]
    if bias is not None:
        out = out + bias.view(1, K, 1, 1)
    return out.contiguous()


def _linear_taps(n_in, n_out, dtype):
    dst = torch.arange(n_out, dtype=dtype)
    src = ((dst + 0.5) * 0.5 - 0.5).clamp(min=0)
    i0 = src.floor().long()
    i1 = torch.where(i0 < n_in - 1, i0 + 1, i0)
    l1 = src - i0.to(dtype)
    return i0, i1, 1 - l1, l1


def bilinear_up2(maps):
    """[..., P, P] -> [..., 2P, 2P]"""
    P = maps.shape[-1]
    i0, i1, l0, l1 = _linear_taps(P, 2 * P, maps.dtype)
    rows = maps[..., :, i0] * l0 + maps[..., :, i1] * l1
    return (rows[..., i0, :] * l0[:, None] + rows[..., i1, :] * l1[:, None]).contiguous()


def _cubic_taps(n_in, n_out, dtype):
    A = -0.75
    scale = torch.tensor(n_in, dtype=dtype) / n_out
    dst = torch.arange(n_out, dtype=dtype)
    src = scale * (dst + 0.5) - 0.5
    fl = src.floor()
    t = src - fl

    def cc1(x):
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def cc2(x):
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A

    w = [cc2(t + 1), cc1(t), cc1(1 - t), cc2(2 - t)]
    idx = [(fl.long() + d).clamp(0, n_in - 1) for d in (-1, 0, 1, 2)]
    return idx, w


def bicubic_resize(maps, out_h, out_w):
    """[..., H, W] -> [..., out_h, out_w]"""
    H, W = maps.shape[-2:]
    ix, wx = _cubic_taps(W, out_w, maps.dtype)
    iy, wy = _cubic_taps(H, out_h, maps.dtype)
    rows = maps[..., :, ix[0]] * wx[0]
    for j in range(1, 4):
        rows = rows + maps[..., :, ix[j]] * wx[j]
    out = rows[..., iy[0], :] * wy[0][:, None]
    for j in range(1, 4):
        out = out + rows[..., iy[j], :] * wy[j][:, None]
    return out


def lowest_argmax(flat):
    """[K, n] -> the LOWEST index of each row's maximum."""
    mx = flat.max(1, keepdim=True)[0]
    n = flat.shape[1]
    idx = torch.arange(n)[None, :].expand_as(flat)
    return torch.where(flat == mx, idx, torch.full_like(idx, n)).min(1)[0]


def box_out_size(roi):
    """(out_h, out_w, h, w) of one box in fp32, as the reference computes them."""
    r = np.asarray(roi, dtype=np.float32)
    w = np.maximum(r[2] - r[0], np.float32(1))
    h = np.maximum(r[3] - r[1], np.float32(1))
    return int(np.ceil(h)), int(np.ceil(w)), h, w


def xy_from_position(roi, x_int, y_int):
    """The reference's fp32 expressions (keypoints.py:173-208), one rounding per operation, in numpy."""
    r = np.asarray(roi, dtype=np.float32)
    oh, ow, h, w = box_out_size(r)
    wc = np.float32(w / np.float32(ow))
    hc = np.float32(h / np.float32(oh))
    x = np.float32(np.float32(np.float32(x_int) + np.float32(0.5)) * wc)
    y = np.float32(np.float32(np.float32(y_int) + np.float32(0.5)) * hc)
    return np.float32(x + r[0]), np.float32(y + r[1])


def heatmaps_to_keypoints(maps, rois, resize=None, return_maps=False):
    """maps [M, K, P, P] (fp32 or fp64), rois [M, 4] fp32 -> [M, K, 4] = (x, y, logit, score) in maps' dtype, and the positions
    (x_int, y_int) int64 [M, K, 2].  The box sizes come from the fp32 rois in every case (as the kernel's do).
    resize: the resize function (default `bicubic_resize`; tests pass F.interpolate to hold this file to ATen)."""
    resize = resize or bicubic_resize
    M, K = maps.shape[:2]
    out = maps.new_zeros(M, K, 4)
    pos = torch.zeros(M, K, 2, dtype=torch.int64)
    full = []
    for i in range(M):
        oh, ow, h, w = box_out_size(rois[i].numpy())
        roi_map = resize(maps[i], oh, ow)
        flat = roi_map.reshape(K, -1)
        p = lowest_argmax(flat)
        mx = flat[torch.arange(K), p]
        x_int, y_int = p % ow, p // ow
        pool = (maps[i] - mx.view(K, 1, 1)).exp().sum((1, 2))
        wc_x = torch.tensor(float(w), dtype=maps.dtype) / ow
        wc_y = torch.tensor(float(h), dtype=maps.dtype) / oh
        out[i, :, 0] = (x_int.to(maps.dtype) + 0.5) * wc_x + rois[i, 0].to(maps.dtype)
        out[i, :, 1] = (y_int.to(maps.dtype) + 0.5) * wc_y + rois[i, 1].to(maps.dtype)
        out[i, :, 2] = mx
        out[i, :, 3] = (mx - mx).exp() / pool
        pos[i, :, 0], pos[i, :, 1] = x_int, y_int
        if return_maps:
            full.append(roi_map)
    return (out, pos, full) if return_maps else (out, pos)


def interpolate_bicubic(maps, out_h, out_w):
    """F.interpolate's bicubic resize of [K, H, W] (ATen itself)."""
    return torch.nn.functional.interpolate(maps[None], size=(out_h, out_w), mode="bicubic", align_corners=False)[0]


def smooth_maps(M, K, seed, P=14):
    """Seeded 3 * randn [M, K, P, P]: the low-resolution logits the decode tests upsample, so that neighbouring values correlate."""
    g = torch.Generator().manual_seed(seed)
    return 3 * torch.randn(M, K, P, P, generator=g)
