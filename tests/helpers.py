"""Shared test helpers: golden loading, the conditioned R50-FPN state_dict, detection matching."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def gold(name):
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind in "fiub" and z[k].ndim > 0 else z[k]) for k in z.files}


def r50_state_dict():
    """The conditioned synthetic R50-FPN weights every e2e fixture was generated with: shapes from the
    reference state_dict key fixture, values from lvc_amd.utils.synthetic, FrozenBN stats from the calibration
    fixture."""
    from lvc_amd.utils import synthetic as syn

    keys = gold("r50_fpn_state_dict_keys")
    template = {}
    for k, shp in zip(keys["keys"].tolist(), keys["shapes"].tolist()):
        template[k] = torch.zeros(eval(shp))
    from oracle import rcnn as orc

    for i, s in enumerate((32, 64, 128, 256, 512)):
        template["proposal_generator.anchor_generator.cell_anchors.%d" % i] = orc.generate_cell_anchors((s,), (0.5, 1.0, 2.0))
    calib = gold("r50_bn_calibration")
    return syn.conditioned_state_dict(template, seed=0, bn_calibration=calib)


def r101_state_dict():
    """Same for R101-FPN (tests/golden/r101_fpn_state_dict_keys.npz, r101_bn_calibration.npz: the weights of
    e2e_r101_fpn_small / e2e_r101_fpn_800x1333)."""
    from lvc_amd.utils import synthetic as syn
    from oracle import rcnn as orc

    keys = gold("r101_fpn_state_dict_keys")
    template = {k: torch.zeros(eval(shp)) for k, shp in zip(keys["keys"].tolist(), keys["shapes"].tolist())}
    for i, s in enumerate((32, 64, 128, 256, 512)):
        template["proposal_generator.anchor_generator.cell_anchors.%d" % i] = orc.generate_cell_anchors((s,), (0.5, 1.0, 2.0))
    return syn.conditioned_state_dict(template, seed=0, bn_calibration=gold("r101_bn_calibration"))


def found_bar(p0, n, margin=0.02):
    """Lower bar of a found fraction over n items when a valid fp32 evaluation of the same path (the oracle, fp32 vs fp64) finds the
    fraction p0 of its own exact answers: p0 - margin (oracle/noise.py IDENT_MARGIN) - two standard deviations of a count of n."""
    n = max(1, n)
    return p0 - margin - 2.0 * (max(p0 * (1.0 - p0), 1.0 / n) / n) ** 0.5


def match_detections(boxes, scores, classes, gboxes, gscores, gclasses, tol=1e-3):
    """Set-equality of detections within `tol` (order may differ where scores are closer than tol).
    Returns (ok, message)."""
    if len(boxes) != len(gboxes):
        return False, "count %d vs %d" % (len(boxes), len(gboxes))
    used = set()
    worst = 0.0
    for i in range(len(gboxes)):
        d = (boxes - gboxes[i]).abs().max(dim=1)[0] + (scores - gscores[i]).abs()
        d = d + (classes != gclasses[i]).float() * 1e6
        for u in used:
            d[u] = 1e9
        j = int(d.argmin())
        if float(d[j]) > 2 * tol:
            return False, "golden detection %d unmatched (best distance %g)" % (i, float(d[j]))
        worst = max(worst, float(d[j]))
        used.add(j)
    return True, "worst %g" % worst


def match_fraction(boxes, scores, classes, gboxes, gscores, gclasses, box_tol, score_tol):
    """Greedy one-to-one matching of golden detections to predictions; returns (fraction matched,
    worst box error among matched, worst score error among matched)."""
    used = set()
    matched, wb, ws = 0, 0.0, 0.0
    for i in range(len(gboxes)):
        db = (boxes - gboxes[i]).abs().max(dim=1)[0]
        ds = (scores - gscores[i]).abs()
        ok = (db <= box_tol) & (ds <= score_tol) & (classes == gclasses[i])
        for u in used:
            ok[u] = False
        idx = ok.nonzero().view(-1)
        if len(idx):
            j = int(idx[db[idx].argmin()])
            used.add(j)
            matched += 1
            wb, ws = max(wb, float(db[j])), max(ws, float(ds[j]))
    return matched / max(1, len(gboxes)), wb, ws


# ------------------------------------------------------------------------------------------------- conv backward: shapes and routes
# Weight gradient (N, H, W, C, K, R, stride, pad): the smallest shapes at which each mechanism of csrc/conv_wgrad.hip can fail.
WGRAD_SHAPES = (
    # pixel counts around the chunk sizes (16 pixels: bf16x3, 32: f32 and f16x2)
    (1, 1, 1, 64, 64, 1, 1, 0), (1, 1, 15, 64, 64, 1, 1, 0), (1, 1, 16, 64, 64, 1, 1, 0), (1, 1, 17, 64, 64, 1, 1, 0),
    (1, 1, 31, 64, 64, 1, 1, 0), (1, 1, 32, 64, 64, 1, 1, 0), (1, 1, 33, 64, 64, 1, 1, 0),
    (3, 5, 7, 32, 36, 3, 1, 1),          # 35 pixels per image: chunks straddle images and rows
    # maps narrower than the kernel: whole taps lie in the padding and must come out exactly 0
    (2, 1, 1, 8, 8, 3, 1, 1), (1, 4, 1, 16, 4, 3, 1, 1), (1, 2, 3, 4, 4, 3, 1, 1),
    # slices joined by atomics, a partial last chunk
    (1, 37, 29, 96, 36, 3, 1, 1),        # 1073 pixels: the last 16-pixel chunk holds one pixel, three slices per engine
    (1, 37, 29, 132, 260, 1, 1, 0),      # one full 128-tile and a tail of 4 on both channel axes
    # strides on odd and even maps
    (2, 51, 35, 64, 32, 1, 2, 0), (2, 50, 84, 32, 64, 1, 2, 0), (1, 13, 21, 32, 32, 3, 2, 1), (1, 12, 20, 32, 32, 3, 2, 1),
)

# Data gradient ((N, H, W, Cin, Kout, R, stride, pad) of the FORWARD layer, {DGRAD_SPLIT: the entry point `conv_dgrad` lands on}),
# the f16x2 column with kernels._HALO_H2_MIN_TILES = 0.
_H3, _H2 = "lvc_conv3x3_nhwc_bf16x3", "lvc_conv3x3_nhwc_f16x2"
_G3, _F32, _DMA = "lvc_conv2d_nhwc_bf16x3", "lvc_conv2d_nhwc_f32", "lvc_conv2d_nhwc_f16x2_dma"
DGRAD_CASES = (
    ((1, 1, 1, 128, 64, 3, 1, 1), {"bf16x3": _H3, "f16x2": _H2}),       # tiny 3x3 maps
    ((1, 2, 3, 128, 64, 3, 1, 1), {"bf16x3": _H3, "f16x2": _H2}),
    ((1, 13, 21, 128, 64, 3, 1, 1), {"bf16x3": _H3, "f16x2": _H2}),
    ((1, 37, 29, 128, 36, 3, 1, 1), {"bf16x3": _H3, "f16x2": _H2}),     # contraction padded 36 -> 64
    ((1, 13, 21, 256, 16, 1, 1, 0), {"bf16x3": _G3, "f16x2": _G3}),     # the padded RPN predictor, fewer than 2048 rows
    ((2, 33, 32, 64, 256, 1, 1, 0), {"bf16x3": _G3, "f16x2": _DMA}),    # 2112 rows, narrow output
    ((2, 33, 32, 256, 64, 1, 1, 0), {"bf16x3": _G3, "f16x2": _DMA}),    # 2112 rows
    ((2, 51, 35, 128, 64, 1, 2, 0), {"bf16x3": _G3, "f16x2": _G3}),     # strided 1x1 then scatter, odd maps
    ((1, 1, 9, 128, 64, 1, 2, 0), {"bf16x3": _G3, "f16x2": _G3}),
    ((1, 13, 21, 128, 64, 3, 2, 1), {"bf16x3": _H3, "f16x2": _H2}),     # dense 3x3 stride 2: zero-stuffed, then the stride-1 product
    ((1, 12, 20, 128, 64, 3, 2, 1), {"bf16x3": _H3, "f16x2": _H2}),
    ((1, 13, 21, 64, 96, 1, 1, 0), {"bf16x3": _F32, "f16x2": _F32}),    # fewer than 128 input channels on a small map: exact fp32 MFMA
    ((1, 13, 21, 32, 64, 3, 1, 1), {"bf16x3": _F32, "f16x2": _F32}),    # a 3x3 with fewer than 64 input channels: the same
)
DGRAD_ENTRIES_REQUIRED = (_H3, _G3, _F32, _H2, _DMA)


def dgrad_route(K, shape, split):
    """The entry point `kernels.conv_dgrad` runs the data gradient of forward layer `shape` on, from `kernels.conv_route` alone (no
    tensor, no library): the operand geometry of `kernels.pack_conv_dgrad` and the grid `conv_dgrad` multiplies on."""
    import types

    N, H, W, Cin, Kout, R, stride, pad = shape
    pcd = types.SimpleNamespace(R=R, S=R, C=(Kout + 31) // 32 * 32, K=Cin, stride=1, pad=R - 1 - pad, mode=0, two_acc=False, state={"tier": 0})
    if stride == 1 or R != 1:
        h, w = (H, W) if stride != 1 else ((H + 2 * pad - R) + 1, (W + 2 * pad - R) + 1)      # a strided 3x3: dy zero-stuffed onto the input grid
    else:
        h, w = (H - 1) // stride + 1, (W - 1) // stride + 1      # a strided 1x1: the product on the sub-sampled grid
    return K.conv_route(pcd, N, h, w, split=split).entry
