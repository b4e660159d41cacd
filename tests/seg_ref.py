"""numpy restatements of csrc/sem_seg.hip, bit for bit: every fp32 operation is one numpy float32 operation (no contraction), in the
kernels' order.  The x2 upsample, the two-stage postprocess (+ argmax) and the combine; the GPU tests compare bits against these, and
tests/test_host_panoptic.py holds these against torch on the CPU and against the reference's own outputs (tests/golden)."""
import numpy as np

F32 = np.float32


def tap(scale, n_out, size):
    """ATen's area_pixel_compute_source_index (align_corners=False) and the two taps, for outputs 0 .. n_out-1 of an axis of `size`
    inputs -> (i0, i1 int64, w0, w1 float32)."""
    d = np.arange(n_out, dtype=F32)
    s = F32(scale) * (d + F32(0.5)) - F32(0.5)
    s = np.where(s < 0, F32(0), s).astype(F32)
    i0 = np.minimum(s.astype(np.int64), size - 1)
    i1 = i0 + (i0 < size - 1)
    w1 = (s - i0.astype(F32)).astype(F32)
    w0 = (F32(1) - w1).astype(F32)
    return i0, i1, w0, w1


def identity_tap(n):
    i = np.arange(n, dtype=np.int64)
    return i, i, np.ones(n, F32), np.zeros(n, F32)


def bilerp(x, ty, tx):
    """x [..., h, w] float32 -> [..., len(ty), len(tx)]: l0 (m0 a + m1 b) + l1 (m0 c + m1 d), rows weigh l, columns m."""
    y0, y1, l0, l1 = ty
    x0, x1, m0, m1 = tx
    a, b = x[..., y0[:, None], x0[None, :]], x[..., y0[:, None], x1[None, :]]
    c, d = x[..., y1[:, None], x0[None, :]], x[..., y1[:, None], x1[None, :]]
    l0, l1, m0, m1 = l0[:, None], l1[:, None], m0[None, :], m1[None, :]
    assert a.dtype == F32
    return l0 * (m0 * a + m1 * b) + l1 * (m0 * c + m1 * d)


def upsample2(x, acc=None):
    """lvcseg_upsample2_bilinear_nhwc: x [N,H,W,C] float32 -> [N,2H,2W,C]; the accumulator is added last."""
    N, H, W, C = x.shape
    v = bilerp(np.ascontiguousarray(x.transpose(0, 3, 1, 2)), tap(0.5, 2 * H, H), tap(0.5, 2 * W, W)).transpose(0, 2, 3, 1)
    if acc is not None:
        v = acc + v
    return np.ascontiguousarray(v, dtype=F32)


def postprocess(low, num_classes, scale, image_size, out_size):
    """lvcseg_sem_seg_postprocess for one image: low [h, w, ld] float32 (channels >= num_classes are not read) ->
    (soft [K, out_h, out_w] float32, labels [out_h, out_w] int64: the lowest class among equal values)."""
    h, w, _ = low.shape
    (ih, iw), (oh, ow) = image_size, out_size
    x = np.ascontiguousarray(low[:, :, :num_classes].transpose(2, 0, 1), dtype=F32)
    rs = F32(1.0 / scale)
    ty, tx = tap(rs, scale * h, h), tap(rs, scale * w, w)
    v = bilerp(x, tuple(t[:ih] for t in ty), tuple(t[:iw] for t in tx))      # first stage, cropped to the image
    if (oh, ow) != (ih, iw):
        qy = identity_tap(oh) if oh == ih else tap(F32(ih) / F32(oh), oh, ih)
        qx = identity_tap(ow) if ow == iw else tap(F32(iw) / F32(ow), ow, iw)
        v = bilerp(v, qy, qx)
    return v, np.argmax(v, axis=0)


def combine(masks, scores, classes, labels, overlap_thresh, stuff_area_limit, instances_thresh):
    """lvcseg_panoptic_combine for one image: masks [n, H, W] bool / 0-1, scores [n] float32, classes [n], labels [H, W] ->
    (panoptic int32 [H, W], segments_info as the reference's list of dicts)."""
    labels = np.asarray(labels)
    pan = np.zeros(labels.shape, dtype=np.int32)
    scores = np.asarray(scores, dtype=F32)
    order = sorted(range(len(scores)), key=lambda j: (-float(scores[j]), j))      # descending, equal scores by the lower index
    cur, info = 0, []
    for j in order:
        score = float(scores[j])
        if score < instances_thresh:
            break
        m = np.asarray(masks[j]).astype(bool)
        area = int(m.sum())
        if area == 0:
            continue
        inter = int((m & (pan > 0)).sum())
        if inter / area > overlap_thresh:
            continue
        cur += 1
        pan[m & (pan == 0)] = cur
        info.append({"id": cur, "isthing": True, "score": score, "category_id": int(classes[j]), "instance_id": int(j)})
    for label in np.unique(labels).tolist():
        if label == 0:
            continue
        m = (labels == label) & (pan == 0)
        area = int(m.sum())
        if area < stuff_area_limit:
            continue
        cur += 1
        pan[m] = cur
        info.append({"id": cur, "isthing": False, "category_id": int(label), "area": area})
    return pan, info
