"""Shared test helpers: golden loading, the conditioned R50-FPN state_dict, detection matching."""
import collections
import os
import types

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
    N, H, W, Cin, Kout, R, stride, pad = shape
    pcd = types.SimpleNamespace(R=R, S=R, C=(Kout + 31) // 32 * 32, K=Cin, stride=1, pad=R - 1 - pad, mode=0, two_acc=False, state={"tier": 0})
    if stride == 1 or R != 1:
        h, w = (H, W) if stride != 1 else ((H + 2 * pad - R) + 1, (W + 2 * pad - R) + 1)      # a strided 3x3: dy zero-stuffed onto the input grid
    else:
        h, w = (H - 1) // stride + 1, (W - 1) // stride + 1      # a strided 1x1: the product on the sub-sampled grid
    return K.conv_route(pcd, N, h, w, split=split).entry


# ------------------------------------------------------------------- exact / fp64 conv tests: what the backward and the forward module share
K_NOISE = 3.0      # test C: ours <= K x the noise of torch's fp32 CPU evaluation of the same inputs (test_gpu_grouped_conv.py)
IMPULSE_BAR = {"f32": 0.0, "bf16x3": 2.0 ** -23, "f16x2": 2.0 ** -21}


def ids(shape):
    return "x".join(map(str, shape))


def gen(shape, salt):
    return torch.Generator().manual_seed(salt + sum((i + 1) * 7919 * v for i, v in enumerate(shape)))


def ints(g, shape, m):
    return torch.randint(-m, m + 1, shape, generator=g).float()


def pow2(g, n):
    return torch.tensor([0.5, 1.0, 2.0, 4.0])[torch.randint(0, 4, (n,), generator=g)]


def full(g, shape, mag=1.0):
    """Values with full fp32 mantissas and 2^-6 <= |v| / mag: inside fp16's normal range for mag = 1, second plane included."""
    r = torch.randn(shape, generator=g)
    return (r + torch.copysign(torch.full_like(r, 2.0 ** -6), r)) * mag


def out_hw(H, W, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


def assert_impulse(got, ref64, engine):
    """Every element is one operand value or exactly 0: the per-engine bar of B."""
    assert got.shape == ref64.shape
    if engine == "f32":
        assert torch.equal(got, ref64.float())
        return
    err = (got.double() - ref64).abs()
    bad = err > IMPULSE_BAR[engine] * ref64.abs()
    assert not bool(bad.any()), (int(bad.sum()), float((err / ref64.abs().clamp_min(1e-300))[bad].max()), int((ref64[bad] == 0).sum()))


def stats(got, ref64):
    d = got.double() - ref64
    return float(d.norm() / ref64.norm().clamp_min(1e-300)), float(d.abs().max())


def assert_noise(worst, key, engine, got, ref32, ref64):
    """Both statistics of C against the fp32-CPU noise (clamped from below by one fp32 rounding of the result); prints ours / noise,
    keeps the largest per engine in `worst` and returns the two ratios (the caller asserts them against its K)."""
    assert got.shape == ref64.shape
    zero = ref64 == 0
    assert float(got[zero].abs().max() if bool(zero.any()) else 0.0) == 0.0, key      # taps that lie in the padding
    o_rel, o_max = stats(got, ref64)
    n_rel, n_max = stats(ref32, ref64)
    n_rel, n_max = max(n_rel, 2.0 ** -25), max(n_max, 2.0 ** -24 * float(ref64.abs().max()))
    r_rel, r_max = o_rel / n_rel, o_max / n_max
    print("%-58s norm-rel ours %.3e noise %.3e ratio %5.2f | max-abs ours %.3e noise %.3e ratio %5.2f" % (key, o_rel, n_rel, r_rel, o_max, n_max, r_max))
    w = worst.setdefault(engine, [0.0, 0.0])
    w[0], w[1] = max(w[0], r_rel), max(w[1], r_max)
    return r_rel, r_max


# ------------------------------------------------------------------------------------------------ conv forward: shapes and routes
# tests/test_gpu_conv_forward_exact.py.  The switches of lvc_amd/kernels.py every row starts from (a row's own switches override them):
# the production configuration, with the size thresholds that keep small maps off a kernel taken away and Winograd off (its rows turn
# it on).
FWD_SWITCHES = {"CONV_ENGINE": "bf16x3", "CONV_SPLIT": "f16x2", "CONV_HALO": True, "_PW_NARROW": True, "HALO_S1": 2, "PW_S1": 2, "PW_W2": True,
                "CONV_WINO": False, "WINO_RPN": False, "PRESPLIT": False, "_HALO_H2_MIN_TILES": 0, "_WINO_MIN_TILES": 1, "_PW_W2_MIN_C": 256,
                "_PW_W2_MIN_ROWS": 1}
# shape: (N, H, W, C, K, R, stride, pad); switches: module switches of this row; entry: the entry point the launch must land on;
# opts: two_acc (pc.two_acc), res (the route needs a residual: only the epilogues with one run), streamk (WINO_STREAMK), patch / force
# (lvc_set_halo_test_hooks), pad_c (the tensor is launched with its channels zero-padded to pad_c: `pack_conv` takes multiples of 32),
# stem (`pack_conv(stem=True)` on NHWC4 rows), linear (`pack_linear` + `linear`).
FwdCase = collections.namedtuple("FwdCase", "shape switches entry opts")
_E = "lvc_conv2d_nhwc_f32 lvc_conv2d_nhwc_bf16x3 lvc_conv2d_nhwc_f16x2 lvc_conv2d_nhwc_f16x2_dma lvc_conv3x3_nhwc_bf16x3 lvc_conv3x3_nhwc_f16x2 " \
     "lvc_conv3x3_nhwc_f16x2_pipe lvc_conv3x3_nhwc_f16s1 lvc_conv3x3_nhwc_wino lvc_conv1x1_nhwc_f16x2_pipe lvc_conv1x1_nhwc_f16s1 lvc_conv1x1_nhwc_f16s1_w2".split()
_F32, _G3, _REG, _DMA, _H3, _H2, _H2P, _HS1, _WINO, _PWP, _PWS1, _PWW2 = _E


def _fwd_cases():
    rows = []

    def add(shape, entry, switches=None, **opts):
        rows.append(FwdCase(tuple(shape), dict(switches or {}), entry, dict(opts)))

    # ---- 3x3 / stride 1 / pad 1: every shape on every form
    s3 = ((1, 1, 1, 32, 64),        # single pixel: eight taps lie in the padding
          (1, 2, 3, 32, 64),        # tiny map
          (2, 7, 9, 32, 128),       # one partial patch, one channel chunk, image boundary inside a tile row
          (1, 13, 21, 64, 132),     # K tail of 4
          (1, 17, 33, 96, 128),     # odd width (Winograd's last pair has one pixel), W crosses the 32-column patch, H the 8- / 16-row ones, 3 chunks
          (3, 16, 32, 128, 256))    # exact patch multiples, two channel tiles
    for N, H, W, C, Kc in s3:
        sh = (N, H, W, C, Kc, 3, 1, 1)
        add(sh, _H3, {"CONV_SPLIT": "bf16x3"})              # (fewer than 128 tiles: the entry point hands over to the generic kernel)
        if H * W >= 63:
            add(sh, _H3, {"CONV_SPLIT": "bf16x3"}, force=1)     # ... and the halo kernel itself, as test_conv3x3_halo_matches_cpu forces it
        add(sh, _H2, {"HALO_S1": 0})
        add(sh, _H2P, {"HALO_S1": 1})
        add(sh, _HS1)
        if Kc >= 128:
            for mode in (0, 1, 2):
                add(sh, _WINO, {"CONV_WINO": True}, streamk=mode)
    add((1, 13, 21, 64, 132, 3, 1, 1), _H2P, two_acc=True)       # the layer flag keeps two accumulators under HALO_S1 = 2
    for patch in ((3, 70), (10, 24)):
        add((1, 17, 33, 96, 128, 3, 1, 1), _H3, {"CONV_SPLIT": "bf16x3"}, force=1, patch=patch)
    # ---- 1x1 with at least 2048 rows
    add((2, 33, 32, 64, 256, 1, 1, 0), _PWP)                     # 2112 rows (a 64-row tail); C < 256 keeps two accumulators
    add((2, 33, 32, 64, 256, 1, 1, 0), _DMA, {"PW_S1": 0})
    add((2, 33, 32, 64, 256, 1, 1, 0), _G3, {"CONV_SPLIT": "bf16x3"})
    add((2, 33, 32, 256, 64, 1, 1, 0), _PWS1)                    # 64-channel narrow tile
    add((2, 33, 32, 256, 64, 1, 1, 0), _PWP, two_acc=True)
    add((2, 33, 32, 256, 64, 1, 1, 0), _DMA, {"PW_S1": 0})
    add((2, 33, 32, 256, 64, 1, 1, 0), _G3, {"CONV_SPLIT": "bf16x3"})
    add((2, 33, 32, 256, 16, 1, 1, 0), _DMA)                     # 32-channel narrow tile (fewer than 64 outputs: never the pipelined kernel)
    add((2, 33, 32, 256, 16, 1, 1, 0), _G3, {"CONV_SPLIT": "bf16x3"})
    add((2, 33, 32, 288, 132, 1, 1, 0), _PWS1)                   # nine chunks, K tail
    add((2, 33, 32, 288, 132, 1, 1, 0), _PWP, two_acc=True)
    add((2, 33, 32, 288, 132, 1, 1, 0), _DMA, {"PW_S1": 0})
    add((2, 33, 32, 288, 132, 1, 1, 0), _REG, {"PW_S1": 0}, res=1)      # a residual with K % 32 != 0: the register-staged kernel
    add((2, 33, 32, 288, 132, 1, 1, 0), _G3, {"CONV_SPLIT": "bf16x3"})
    add((2, 33, 32, 256, 256, 1, 1, 0), _PWW2)                   # the 256 x 256 tile ...
    add((2, 33, 32, 256, 256, 1, 1, 0), _PWS1, {"PW_W2": False})      # ... against the 256 x 128 tile
    add((2, 33, 32, 256, 256, 1, 1, 0), _PWP, two_acc=True)
    add((2, 33, 32, 256, 256, 1, 1, 0), _DMA, {"PW_S1": 0})
    add((2, 65, 65, 256, 128, 1, 2, 0), _PWS1)                   # stride 2 on an odd map: 2178 rows
    add((2, 65, 65, 256, 128, 1, 2, 0), _PWP, two_acc=True)
    add((2, 65, 65, 256, 128, 1, 2, 0), _DMA, {"PW_S1": 0})
    add((2, 65, 65, 256, 128, 1, 2, 0), _G3, {"CONV_SPLIT": "bf16x3"})
    add((2, 34, 32, 256, 256, 1, 1, 0), _PWW2, res=2)            # upsample-add: residual [2, 17, 16, 256]
    add((2, 34, 32, 256, 256, 1, 1, 0), _PWS1, {"PW_W2": False}, res=2)
    add((2, 34, 32, 256, 256, 1, 1, 0), _PWP, two_acc=True, res=2)
    add((2, 34, 32, 256, 256, 1, 1, 0), _DMA, {"PW_S1": 0}, res=2)
    add((2, 34, 32, 256, 256, 1, 1, 0), _G3, {"CONV_SPLIT": "bf16x3"}, res=2)
    # ---- small and generic
    add((1, 13, 21, 128, 132, 1, 1, 0), _G3)                     # fewer than 2048 rows
    add((1, 13, 21, 256, 15, 1, 1, 0), _F32)                     # K % 4 != 0
    add((1, 13, 21, 16, 64, 3, 1, 1), _F32, {"CONV_HALO": False}, pad_c=32)      # C % 32 != 0: launched zero-padded to 32 channels
    add((1, 13, 21, 32, 32, 3, 1, 1), _F32)                      # a 3x3 with fewer than 64 output channels
    add((1, 13, 21, 32, 128, 3, 2, 1), _G3)                      # strided 3x3, odd and even maps
    add((1, 12, 20, 32, 128, 3, 2, 1), _G3)
    add((1, 1, 9, 128, 128, 1, 2, 0), _G3)                       # strided 1x1 on a one-row map
    add((1, 37, 41, 3, 64, 7, 2, 3), _F32, stem=True)            # BasicStem's 7x7 / 2 on NHWC4 rows
    add((2, 14, 18, 3, 64, 7, 2, 3), _F32, stem=True)
    add((300, 1, 1, 1024, 81, 1, 1, 0), _F32, linear=True)       # the box predictor's class scores
    return tuple(rows)


FWD_CASES = _fwd_cases()
# the fused and multi-map launches the forward module drives next to `conv2d_nhwc`: its tests take the entry point they assert from here,
# so the host test's union over this table cannot stay whole when one of them goes
FWD_FUSED = {"levels": "lvc_conv3x3_nhwc_f16_levels", "layers": "lvc_conv3x3_nhwc_f16_layers", "levels_pred": "lvc_conv3x3_nhwc_f16_levels_pred",
             "wino_pred": "lvc_conv3x3_nhwc_wino_pred", "presplit_3x3": "lvc_conv3x3_nhwc_f16s1_presplit",
             "presplit_1x1": "lvc_conv1x1_nhwc_f16s1_presplit", "chain": "lvc_conv1x1_chain_nhwc_f16s1", "bottleneck": "lvc_bottleneck_nhwc_f16s1"}
FWD_FUSED_ENTRIES = tuple(FWD_FUSED.values())


def fwd_case_id(case):
    opts = "".join("-%s%s" % (k, "" if v is True else "x".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in sorted(case.opts.items()))
    return "%s-%s%s" % (ids(case.shape), case.entry[4:].replace("_nhwc", ""), opts)


def fwd_set_switches(monkeypatch, K, case):
    for name, value in dict(FWD_SWITCHES, **case.switches).items():
        monkeypatch.setattr(K, name, value)


def fwd_route(K, case, res_mode=0, ldo=None):
    """The entry point `kernels.conv2d_nhwc` runs `case` on under the switches as they are (`fwd_set_switches`), from `kernels.conv_route`
    on plain numbers: res_mode 0 / 1 / 2 the residual operand, ldo the last dimension of the output buffer (None: K)."""
    N, H, W, C, Kc, R, stride, pad = case.shape
    o = case.opts
    C = 4 if o.get("stem") else o.get("pad_c", C)
    pc = types.SimpleNamespace(R=R, S=R, C=C, K=Kc, stride=stride, pad=pad, mode=1 if o.get("stem") else 0, two_acc=bool(o.get("two_acc")), state={"tier": 0})
    Ho, Wo = out_hw(H, W, R, stride, pad)
    res_numel = 0 if not res_mode else N * Ho * Wo * Kc if res_mode == 1 else N * (Ho // 2) * (Wo // 2) * Kc
    return K.conv_route(pc, N, H, W, ldo=ldo, out_numel=None if ldo is None else N * Ho * Wo * ldo, ldr=Kc if res_mode else None, res_numel=res_numel).entry


class Recorded:
    """`kernels._launch` wrapped (the bracket around every conv / GEMM launch): `ran` lists the entry points that ran, in order.
    monkeypatch undoes the wrap when the test ends; `ran.clear()` starts a new list."""

    def __init__(self, K, monkeypatch):
        self.ran = []
        launch = K._launch
        monkeypatch.setattr(K, "_launch", lambda tag, flops, nbytes, slot, what, call: (self.ran.append(what), launch(tag, flops, nbytes, slot, what, call))[1])
