"""A plain fp64 reference of ROIAlign (forward and backward over a pyramid of NHWC maps), the error bound the kernels are held to, and
the case table tests/test_host_roi_align_ref.py and tests/test_gpu_roi_align_routes.py share.  numpy, torch and the input generator of tests/helpers.py only:
nothing here imports the package under test or the oracle.

The operation is separable: a sample is dropped when its row OR its column is out of range, and a tap's weight is a row factor times
a column factor.  Per RoI, with Wy [ph, H] and Wx [pw, W] the per-bin sums of the samples' weights onto the map's rows and columns,
    out[p, q, c]  = sum_y sum_x Wy[p, y] Wx[q, x] feat[y, x, c] / max(gh * gw, 1)
    dfeat[y, x, c] += sum_p sum_q Wy[p, y] G[p, q, c] Wx[q, x] / (gh * gw).

GEOMETRY is float32, in the operation order of the reference CPU kernel (the order at the top of csrc/roi_align.hip): roi start and
size, the `aligned` offset, the max(size, 1) clamp of aligned=False, bin, g = sr > 0 ? sr : ceil(size / pooled), every sample
coordinate, the < -1 / > L drop, the <= 0 clamp and the top-edge clamp.  That decides which samples exist and is discontinuous, so an
fp64 geometry would describe another operation.  WEIGHTS (l = v - lo, 1 - l), products and sums are fp64.

THE BOUND.  A sum of n fp32 terms taken in any order, each term a product of a few rounded factors, is off by at most
(n + c) * 2^-24 * A to first order, A the sum of the absolute terms.  n and A come from this reference:
  forward   n = 4 * (in-range sample rows of the bin) * (in-range sample columns): its taps.  The wave form sums window pixels instead
            (`wave_terms`): each term passes <= gh + gw roundings of the pre-summed weights, <= nrows fmas of the column sums and
            <= ncols fmas of the bin sums, and nrows + ncols <= nrows * ncols + 1; so n = max(taps, window pixels + gh + gw).
  backward  n = the taps the pixel receives over all RoIs.  The rows form pre-sums the weights of a bin (<= Ty - 1 and Tx - 1 adds,
            Ty, Tx the bin's taps onto this row / column), adds over the <= 7 bins of either axis that reach the pixel and one atomic
            per RoI; with SY, SX the taps of all bins onto the row / column, these are <= SY + SX - 2 <= SY * SX - 1 = n - 1.
  c         the roundings of one term outside its sums, longest chain in roi_align.hip = the scatter backward's
            `g * (hy * hx) / count`: hy = 1 - ly (1), hx = 1 - lx (1), hy * hx (1), g * w (1), / count (1) -- 5 (l = v - lo is exact:
            lo <= v < lo + 1).  The scalar forward has the same five (w * v for g * w); the wave forward 1 - l twice, 1 / count, * inv
            and the + 1 above (5); the rows backward 1 - l twice, g / count, g * wy, row * wx (5).  C_ROUND = 8 leaves three for the
            second-order terms (n * 2^-24 < 1e-3 at every n here).
The bound is clamped from below by one fp32 rounding of the result, 2^-24 |ref|.
"""
import collections
import functools
import math

import numpy as np
import torch

from helpers import full

F32 = np.float32
U = 2.0 ** -24
C_ROUND = 8
RB_MAXS, RB_MAXF = 448, 192      # csrc/roi_align.hip: samples per axis / footprint pixels the rows backward holds in its tables
WAVE_MAX = 64                    # window rows / columns the wave forward holds in a register


# ------------------------------------------------------------------------------------------------ geometry (float32)
def _axis(c0, c1, scale, L, pooled, sr, aligned):
    """One axis of one RoI.  Returns (g, v [pooled, g] float32 clamped sample coordinates, ok [pooled, g], lo, hi [pooled, g] int,
    start, size) -- every number float32 arithmetic in the kernel's order."""
    off = F32(0.5) if aligned else F32(0.0)
    start = F32(c0) * F32(scale) - off
    end = F32(c1) * F32(scale) - off
    size = F32(end - start)
    if aligned:
        if not size >= 0:
            raise ValueError("ROIs in ROIAlign cannot have negative size")
    else:
        size = size if size > F32(1.0) else F32(1.0)
    bin_ = F32(size / F32(pooled))
    g = int(sr) if sr > 0 else int(math.ceil(F32(size / F32(pooled))))
    p = np.arange(pooled, dtype=F32)[:, None]
    i = (np.arange(max(g, 0), dtype=F32) + F32(0.5))[None, :]
    with np.errstate(all="ignore"):
        v = (start + p * bin_) + (i * bin_) / F32(max(g, 1))
    assert v.dtype == F32
    ok = ~((v < F32(-1.0)) | (v > F32(L)))
    v = np.where(v <= 0, F32(0), v)
    lo = np.where(ok, v, 0).astype(np.int64)
    top = lo >= L - 1
    lo = np.where(top, L - 1, lo)
    hi = np.where(top, L - 1, lo + 1)
    v = np.where(top, lo.astype(F32), v)
    return g, v, ok, lo, hi, start, size, bin_


def _weights(ax, L):
    """W [pooled, L] fp64 weight sums, T [pooled, L] taps, nv [pooled] in-range samples."""
    g, v, ok, lo, hi = ax[:5]
    pooled = v.shape[0]
    W = np.zeros((pooled, L))
    T = np.zeros((pooled, L), dtype=np.int64)
    l = v.astype(np.float64) - lo
    for p in range(pooled):
        for i in range(max(g, 0)):
            if ok[p, i]:
                W[p, lo[p, i]] += 1.0 - l[p, i]
                W[p, hi[p, i]] += l[p, i]
                T[p, lo[p, i]] += 1
                T[p, hi[p, i]] += 1
    return W, T, ok.sum(axis=1)


def geometry(roi, scale, H, W, ph, pw, sr, aligned):
    """What the kernels' per-RoI branches depend on.  gh, gw; samples per axis (ph * gh, pw * gw); extent (y, x) = s_max - s_min of
    the rows backward (-1: no sample in range); win_rows [ph], win_cols: the window the wave forward reads for each output row."""
    ay = _axis(roi[2], roi[4], scale, H, ph, sr, aligned)
    ax = _axis(roi[1], roi[3], scale, W, pw, sr, aligned)
    ext = []
    for a in (ay, ax):
        ok = a[2]
        ext.append(int(a[4][ok].max() - a[3][ok].min()) if ok.any() else -1)
    (start_h, size_h, bin_h), (start_w, size_w) = ay[5:8], ax[5:7]
    rows = []
    for p in range(ph):
        yf, yl = start_h + F32(p) * bin_h, start_h + F32(p + 1) * bin_h
        y0 = min(int(math.floor(max(yf, F32(0)))), H - 1)
        y1 = min(int(math.floor(max(yl, F32(0)))) + 1, H - 1)
        rows.append(y1 - y0 + 1)
    x0 = min(int(math.floor(max(start_w, F32(0)))), W - 1)
    x1 = min(int(math.floor(max(F32(start_w + size_w), F32(0)))) + 1, W - 1)
    return {"gh": ay[0], "gw": ax[0], "samples": (ph * ay[0], pw * ax[0]), "extent": tuple(ext), "win_rows": rows, "win_cols": x1 - x0 + 1}


def wave_sep(geo):
    """True when the wave forward takes its separable form on every output row of this RoI (else the per-sample loop on some)."""
    return geo["gh"] > 0 and geo["gw"] > 0 and 1 <= geo["win_cols"] <= WAVE_MAX and all(1 <= r <= WAVE_MAX for r in geo["win_rows"])


def rows_tables(geo):
    """The rows backward's branch: 'tables', 'fallback-samples', 'fallback-footprint' or 'none' (no gradient)."""
    if geo["gh"] < 1 or geo["gw"] < 1:
        return "none"
    if max(geo["samples"]) > RB_MAXS:
        return "fallback-samples"
    if max(geo["extent"]) >= RB_MAXF:
        return "fallback-footprint"
    return "tables" if min(geo["extent"]) >= 0 else "none"


# ------------------------------------------------------------------------------------------------ forward / backward (float64)
def _roi_parts(roi, lvl, shapes, scales, ph, pw, sr, aligned):
    H, W = shapes[lvl]
    ay = _axis(roi[2], roi[4], scales[lvl], H, ph, sr, aligned)
    ax = _axis(roi[1], roi[3], scales[lvl], W, pw, sr, aligned)
    return ay, ax, _weights(ay, H), _weights(ax, W)


def _sandwich(Wy, f, Wx):
    """sum_y sum_x Wy[p, y] f[y, x, c] Wx[q, x] -> [p, q, c], the rows first."""
    return np.einsum("pxc,qx->pqc", np.tensordot(Wy, f, axes=(1, 0)), Wx)


def forward(feats, scales, rois, levels, ph, pw, sr, aligned, wave_terms=False):
    """feats: list of [B, H_l, W_l, C] (any float type); rois [K, 5]; levels [K] ints or None.  Returns (out, A, n), each
    [K, ph, pw, C] / n [K, ph, pw] : fp64 value, sum of |term|, number of terms (wave_terms: of the wave form)."""
    feats = [np.asarray(f, dtype=np.float64) for f in feats]
    rois = np.asarray(rois, dtype=np.float32)
    K, C = rois.shape[0], feats[0].shape[3]
    shapes = [f.shape[1:3] for f in feats]
    out, A, n = np.zeros((K, ph, pw, C)), np.zeros((K, ph, pw, C)), np.zeros((K, ph, pw), dtype=np.int64)
    for k in range(K):
        lvl = 0 if levels is None else int(levels[k])
        ay, ax, (Wy, Ty, nvy), (Wx, Tx, nvx) = _roi_parts(rois[k], lvl, shapes, scales, ph, pw, sr, aligned)
        cnt = max(ay[0] * ax[0], 1)
        f = feats[lvl][int(rois[k, 0])]
        out[k] = _sandwich(Wy, f, Wx) / cnt
        A[k] = _sandwich(Wy, np.abs(f), Wx) / cnt
        n[k] = 4 * nvy[:, None] * nvx[None, :]
        if wave_terms:
            geo = geometry(rois[k], scales[lvl], shapes[lvl][0], shapes[lvl][1], ph, pw, sr, aligned)
            win = np.asarray(geo["win_rows"], dtype=np.int64).clip(min=0) * max(geo["win_cols"], 0) + max(geo["gh"], 0) + max(geo["gw"], 0)
            n[k] = np.maximum(n[k], win[:, None])
    return out, A, n


def backward(grad, shapes, scales, rois, levels, sr, aligned, num_valid=None):
    """grad [K, ph, pw, C]; shapes: list of (B, H_l, W_l, C).  Returns a list over the levels of (dfeat, A [B, H, W, C], n [B, H, W]);
    num_valid: only the first num_valid RoIs scatter."""
    grad = np.asarray(grad, dtype=np.float64)
    rois = np.asarray(rois, dtype=np.float32)
    K, ph, pw, C = grad.shape
    hw = [sh[1:3] for sh in shapes]
    res = [(np.zeros(sh), np.zeros(sh), np.zeros(sh[:3], dtype=np.int64)) for sh in shapes]
    for k in range(K if num_valid is None else min(K, int(num_valid))):
        lvl = 0 if levels is None else int(levels[k])
        ay, ax, (Wy, Ty, _), (Wx, Tx, _) = _roi_parts(rois[k], lvl, hw, scales, ph, pw, sr, aligned)
        cnt = ay[0] * ax[0]
        if cnt <= 0:
            continue
        b = int(rois[k, 0])
        res[lvl][0][b] += _sandwich(Wy.T, grad[k], Wx.T) / cnt
        res[lvl][1][b] += _sandwich(Wy.T, np.abs(grad[k]), Wx.T) / cnt
        res[lvl][2][b] += np.einsum("py,qx->yx", Ty, Tx)
    return res


def bound(ref, A, n):
    """(n + C_ROUND) * 2^-24 * A, at least one fp32 rounding of the result; n broadcasts over the channels."""
    n = np.asarray(n, dtype=np.float64)
    if n.ndim == ref.ndim - 1:
        n = n[..., None]
    return np.maximum((n + C_ROUND) * U * A, U * np.abs(ref))


def ratio(got, ref, A, n):
    """Largest error / bound (0 where both are 0)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    b = bound(ref, A, n)
    r = np.where(err == 0, 0.0, err / np.where(b == 0, 1e-300, b))
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ inputs
B = 2
C_MAX = 260
PYRAMID = ((24, 32), (6, 8))
TALL = ((200, 8),)


def _edge_rois(H, W, scale, aligned, close):
    """The fixed edge list of one level, in image coordinates (level pixels / scale)."""
    o = 0.5 if aligned else 0.0      # a level coordinate c sits at image coordinate (c + o) / scale
    px = [
        (-0.9, -0.9, 5.0, 4.0),                          # over the left / top edge: samples in [-1, 0) (clamped) and below -1 (dropped)
        (W - 5.0, H - 4.0, W + 1.2, H + 1.3),            # samples in (L-1, L] (clamped to the last pixel) and beyond L (dropped)
        (-6.0, 1.0, 5.0, H - 2.0), (W - 6.0, 1.0, W + 8.0, H - 2.0), (2.0, -5.0, W - 3.0, 3.0), (2.0, H - 3.0, W - 3.0, H + 7.0),
        (-30.0, -30.0, -10.0, -12.0), (W + 5.0, H + 5.0, W + 20.0, H + 20.0),      # entirely outside: zeros, no gradient
        (3.0, 3.0, 3.0, 3.0), (4.0, 1.0, 4.0, H - 1.0),  # zero area; zero width only (gh * gw = 0, count 1, with sampling_ratio 0)
        (2.2, 1.1, 2.5, 1.4), (W - 3.3, 2.2, W - 2.6, 2.9),      # 0.3 px; below 1 px (aligned=False clamps the size to 1)
        (0.0, 0.0, float(W), float(H)), (-W / 2.0, -H / 2.0, 1.5 * W, 1.5 * H),      # the whole map, twice the whole map
        (W / 2.0 - 1.0, 0.0, W / 2.0 + 1.0, float(H)),   # 2 px wide by the full height
    ]
    if close:      # 1e-3 px wide (high), the start within 1e-5 of a pixel boundary above 20: sample positions round onto the boundary
        px += [(21.0 - 5e-6, 2.0, 21.0 - 5e-6 + 1e-3, 9.0), (3.0, 21.0 + 4e-6, 11.0, 21.0 + 4e-6 + 1e-3), (22.0 + 2e-6, 20.0 - 7e-6, 22.0 + 2e-6 + 1e-3, 20.0 - 7e-6 + 1e-3)]
    return [tuple((c + o) / scale for c in r) for r in px]


def _interior_rois(g, n, H, W, scale):
    x = torch.rand(n, 4, generator=g).double()
    w, h = 0.5 + x[:, 2] * (W - 2.0), 0.5 + x[:, 3] * (H - 2.0)
    x1, y1 = x[:, 0] * (W - w), x[:, 1] * (H - h)
    return [tuple(float(v) / scale for v in r) for r in torch.stack([x1, y1, x1 + w, y1 + h], 1)]


def _pack(per_level):
    rows, levels = [], []
    for lvl, boxes in enumerate(per_level):
        for i, bx in enumerate(boxes):
            rows.append((float(i % B),) + tuple(bx))
            levels.append(lvl)
    perm = torch.randperm(len(rows), generator=torch.Generator().manual_seed(len(rows)))      # levels and images interleaved
    return torch.tensor(rows, dtype=torch.float32)[perm].contiguous(), torch.tensor(levels, dtype=torch.int32)[perm].contiguous()


def _exact_rois(g, hw, ph, pw):
    per_level = []
    for (H, W), n in zip(hw, (16, 10) if len(hw) == 2 else (10,)):
        boxes = []
        for i in range(n):
            m = [(0.5, 1.0, 2.0, 4.0)[int(v)] for v in torch.randint(0, 4, (2,), generator=g)]
            x0 = int(torch.randint(-5, W + 2, (1,), generator=g))
            y0 = int(torch.randint(-5, min(H, 40) + 2, (1,), generator=g)) + (0 if H <= 40 or i % 2 else H - 30)
            if i == 0:
                x0, y0 = -3, -2                      # samples below -1 (dropped) and in [-1, 0) (clamped)
            if i == 1:
                x0, y0 = W - 2, H - 3                # samples in (L-1, L] and beyond L
            boxes.append((x0 + 0.5, y0 + 0.5, x0 + 0.5 + pw * m[0], y0 + 0.5 + ph * m[1]))
        per_level.append(boxes)
    return _pack(per_level)


# ------------------------------------------------------------------------------------------------ the case table
# maps: "pyramid" (24 x 32 and 6 x 8; scales 1/4 and 1/16 on the noise rows, 1 and 1 on the exact rows) or "tall" (200 x 8, scale 1).
# claim: what the name says about the per-RoI branch of every listed RoI -- (roi index, "wave-sep" | "wave-loop" | "tables" |
# "fallback-samples" | "fallback-footprint"); test_host_roi_align_ref.py asserts each from geometry().
Case = collections.namedtuple("Case", "name maps C pooled sr aligned kind fwd bwd claims")
POOLED = ((7, 7), (8, 7), (1, 7), (9, 7), (14, 14), (7, 14), (14, 7), (2, 3))
VEC_C, SCALAR_C = (4, 36, 260), (6, 258)


def fwd_route(C, pooled, has_num_valid=False):
    if C % 4 or has_num_valid:
        return "scalar"
    return "wave" if pooled[0] <= 8 and pooled[1] == 7 else "nhwc4"


def bwd_route(pooled):
    return "rows" if tuple(pooled) == (7, 7) else "scatter"


def case_shapes(case):
    return TALL if case.maps == "tall" else PYRAMID


def case_scales(case):
    if case.maps == "tall" or case.kind == "exact":
        return (1.0,) * len(case_shapes(case))
    return (0.25, 0.0625)


@functools.lru_cache(maxsize=None)
def _data(maps, pooled, sr, aligned, kind, extra):
    """(feats [B, H, W, C_MAX] per level, rois, levels, grad [K, ph, pw, C_MAX]) of every row with this key, whatever its C: a row
    takes the first C channels, so one reference serves them all."""
    hw = TALL if maps == "tall" else PYRAMID
    g = torch.Generator().manual_seed(1000 * pooled[0] + 10 * pooled[1] + sr + (500 if aligned else 0) + (7 if kind == "exact" else 0) + len(extra))
    ph, pw = pooled
    if extra:
        rois = torch.tensor([(float(i % B),) + tuple(bx) for i, bx in enumerate(extra)], dtype=torch.float32)
        levels = torch.zeros(len(extra), dtype=torch.int32)
    elif kind == "exact":
        rois, levels = _exact_rois(g, hw, ph, pw)
    else:
        scales = (1.0,) if maps == "tall" else (0.25, 0.0625)
        rois, levels = _pack([_interior_rois(g, n, H, W, s) + _edge_rois(H, W, s, aligned, close=H > 21 and W > 22)
                              for (H, W), s, n in zip(hw, scales, (12, 8))])
    K = rois.shape[0]
    if kind == "exact":
        feats = [torch.randint(-8, 9, (B, H, W, C_MAX), generator=g).float() for H, W in hw]
        grad = torch.randint(-8, 9, (K, ph, pw, C_MAX), generator=g).float()
    else:
        feats = [full(g, (B, H, W, C_MAX)) for H, W in hw]
        grad = full(g, (K, ph, pw, C_MAX))
    return feats, rois, levels, grad


def case_key(case):
    return (case.maps, case.pooled, case.sr, case.aligned, case.kind, _EXTRA.get(case.name, ()))


def case_data(case):
    """The row's tensors at its own channel count (contiguous copies of the shared ones)."""
    feats, rois, levels, grad = _data(*case_key(case))
    return [f[..., :case.C].contiguous() for f in feats], rois, levels, grad[..., :case.C].contiguous()


@functools.lru_cache(maxsize=None)
def _ref_forward(key, wave_terms):
    feats, rois, levels, _ = _data(*key)
    maps, pooled, sr, aligned, kind = key[:5]
    scales = (1.0,) * len(feats) if maps == "tall" or kind == "exact" else (0.25, 0.0625)
    return forward([f.numpy() for f in feats], scales, rois.numpy(), levels.numpy(), pooled[0], pooled[1], sr, aligned, wave_terms=wave_terms)


@functools.lru_cache(maxsize=None)
def _ref_backward(key, num_valid):
    feats, rois, levels, grad = _data(*key)
    maps, pooled, sr, aligned, kind = key[:5]
    scales = (1.0,) * len(feats) if maps == "tall" or kind == "exact" else (0.25, 0.0625)
    return backward(grad.numpy(), [tuple(f.shape) for f in feats], scales, rois.numpy(), levels.numpy(), sr, aligned, num_valid=num_valid)


def ref_forward(case, wave_terms=False):
    """(out, A, n) of the row, sliced to its channels (read-only views of the shared reference)."""
    out, A, n = _ref_forward(case_key(case), bool(wave_terms))
    return out[..., :case.C], A[..., :case.C], n


def ref_backward(case, num_valid=None):
    return [(d[..., :case.C], A[..., :case.C], n) for d, A, n in _ref_backward(case_key(case), num_valid)]


def _extent_box(target, aligned):
    """A RoI on the tall map whose rows backward footprint extent along y is exactly `target` with sampling_ratio 2 and 7 x 7 bins."""
    H, W = TALL[0]
    o = 0.5 if aligned else 0.0
    for i in range(4000):
        y2 = 150.0 + 0.05 * i
        roi = (0.0, 1.0 + o, -4.0 + o, 6.0 + o, y2 + o)
        if geometry(roi, 1.0, H, W, 7, 7, 2, aligned)["extent"][0] == target:
            return roi[1:]
    raise AssertionError("no box with extent %d" % target)


_EXTRA = {}      # case name -> the row's own RoIs (image coordinates), where the table names them


def _cases():
    rows = []

    def add(name, maps, C, pooled, sr, aligned, kind, claims=(), extra=None):
        if extra is not None:
            _EXTRA[name] = tuple(tuple(float(v) for v in bx) for bx in extra)
        rows.append(Case(name, maps, C, tuple(pooled), sr, aligned, kind, fwd_route(C, pooled), bwd_route(pooled), tuple(claims)))

    for pooled in POOLED:
        tag = "%dx%d" % pooled
        for C in VEC_C + SCALAR_C:
            combos = ((0, True), (0, False), (2, True), (2, False)) if C in (36, 258) else ((0, True), (2, False))
            for sr, aligned in combos:
                add("noise-%s-C%d-sr%d-a%d" % (tag, C, sr, aligned), "pyramid", C, pooled, sr, aligned, "noise")
            for sr in (0, 2):
                add("exact-%s-C%d-sr%d" % (tag, C, sr), "pyramid", C, pooled, sr, True, "exact")
    for sr in (1, 3):
        add("noise-14x14-C36-sr%d-a1" % sr, "pyramid", 36, (14, 14), sr, True, "noise")
    # ---- the tall map: the per-RoI branches of the wave forward and of the rows backward
    H, W = TALL[0]
    for aligned in (True, False):
        a = int(aligned)
        small = [(1.0, 10.0, 6.0, 150.0), (0.5, 120.0, 7.5, 199.0), (2.0, -3.0, 5.0, 40.0)]
        add("tall-7x7-tables-by-samples-a%d" % a, "tall", 4, (7, 7), 64, aligned, "noise", [(i, "tables") for i in range(3)] + [(i, "wave-sep") for i in range(3)], extra=small)
        add("tall-7x7-fallback-by-samples-a%d" % a, "tall", 4, (7, 7), 65, aligned, "noise", [(i, "fallback-samples") for i in range(3)], extra=small)
        add("tall-7x7-tables-footprint-191-a%d" % a, "tall", 36, (7, 7), 2, aligned, "noise", [(0, "tables"), (1, "tables")],
            extra=[_extent_box(191, aligned), (1.0, 20.0, 6.0, 120.0)])
        add("tall-7x7-fallback-footprint-192-a%d" % a, "tall", 36, (7, 7), 2, aligned, "noise", [(0, "fallback-footprint"), (1, "tables")],
            extra=[_extent_box(192, aligned), (1.0, 20.0, 6.0, 120.0)])
        # the wave forward's per-sample loop: an output row whose window has more than 64 map rows
        big = [(-2.0, -200.0, 9.0, 400.0), (0.0, 0.0, float(W), float(H)), (1.0, 30.0, 6.0, 90.0)]
        for sr in (0, 2):
            add("tall-7x7-wave-loop-sr%d-a%d" % (sr, a), "tall", 36, (7, 7), sr, aligned, "noise", [(0, "wave-loop"), (1, "wave-sep"), (2, "wave-sep")], extra=big)
            add("tall-1x7-wave-loop-sr%d-a%d" % (sr, a), "tall", 36, (1, 7), sr, aligned, "noise", [(0, "wave-loop"), (1, "wave-loop"), (2, "wave-sep")], extra=big)
    for sr in (0, 2):      # exact rows on the tall map: the rows backward's tables and the wave forward at 200 rows
        add("exact-tall-7x7-C36-sr%d" % sr, "tall", 36, (7, 7), sr, True, "exact")
        add("exact-tall-8x7-C4-sr%d" % sr, "tall", 4, (8, 7), sr, True, "exact")
    return tuple(rows)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def claim_holds(case, idx, claim):
    """Whether RoI `idx` of the row has the property `claim` names, from geometry() alone."""
    _, rois, levels, _ = _data(*case_key(case))
    lvl = int(levels[idx])
    H, W = case_shapes(case)[lvl]
    geo = geometry(rois[idx].numpy(), case_scales(case)[lvl], H, W, case.pooled[0], case.pooled[1], case.sr, case.aligned)
    if claim == "wave-sep":
        return wave_sep(geo)
    if claim == "wave-loop":
        return not wave_sep(geo) and geo["gh"] > 0 and geo["gw"] > 0
    return rows_tables(geo) == claim
