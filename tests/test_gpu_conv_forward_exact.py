"""Exact and fp64 tests of the forward convolution kernels, every route: the thirteen entry points `kernels.conv_route` chooses among
(helpers.FWD_CASES: shape, module switches, the entry point the launch must land on -- tests/test_host_conv_dispatch.py holds the table
against `conv_route` without a GPU) and the launches beside it: `conv3x3_levels` (shared layer / a layer per map), `conv3x3_levels_pred`
(direct and Winograd), the presplit pair, `conv1x1_chain`, `bottleneck_fused`, `stem_conv_pool`, `linear`.  Every case wraps
`kernels._launch` and asserts the list of entry points that ran; the conv error word is cleared before and must be 0 after.
Three kinds of test, as in tests/test_gpu_conv_backward_exact.py, none with a tolerance that was chosen:

A. integer-exact (every entry point, every epilogue it takes: none, affine + ReLU, res_mode 1, res_mode 2 on even maps, an output
   buffer whose rows are 12 floats wider than K -- an epilogue under which `conv_route` leaves the row's entry point is not run on
   that row).  x holds integers in [-7, 7], the weights integers in [-3, 3], the per-channel scale is one of {0.5, 1, 2, 4}, shift and
   residual are small integers: every operand is exact in bf16 and in fp16 (after the power-of-two operand scalings of the
   one-accumulator forms too), every product and partial sum a multiple of 0.5 far below 2^24, so every engine, in any summation order
   -- stream-K hand-offs, the atomics of the fused predictor -- must return the fp64 reference BIT FOR BIT.  Winograd F(2,3)
   qualifies: V = d0 - d2, d1 + d2, d2 - d1, d1 - d3 are integers of at most 14, U = g0, (g0 +- g1 + g2) / 2, g2 half-integers, both
   exact in fp16.  One output channel of every case has an all-zero weight row (RetinaNet's zero-padded bbox_pred; the degenerate row
   exponent of lvc_split_weights_rowscaled): its result is exactly shift (+ residual).  The chained launches draw sparser, smaller
   integers: every intermediate activation of the fp64 reference is a multiple of 0.5 with |v| <= 4094, the result below 2^22
   (asserted on the CPU before anything is launched).  Catches indexing: a tail channel read from its neighbour, a residual row off by
   one, a partial sum added twice, the missing second pixel of Winograd's last pair.
B. impulse with full mantissas (the `conv2d_nhwc` entry points).  (1) weights 0 / 1.0 with a single 1.0 per output row, x with full fp32
   mantissas (|v| >= 2^-6); (2) x one-hot per image, weights with full mantissas, a power-of-two scale.  Every output is ONE operand
   value (times a power of two) or exactly 0.  f32: bit-equal.  bf16x3: |err| <= 2^-23 |v| (hi + mid + lo == v exactly; the kept
   products with 1.0 are summed in fp32 with zeros: at most one rounding).  f16x2 with two accumulators: 2^-21 |v| (two fp16 planes
   carry 22 bits).  f16x2 with one accumulator (f16s1, f16s1_w2): 2^-21 |v| as well -- csrc/conv3x3_halo_s1.hip's header: the
   unscaled residual plane is normal for |a| >= 2^-7 (activations x 2^4) and for row entries >= 2^-17 of the row's largest (rows x 2^e),
   which the values drawn here are, so the two planes again carry 22 bits.  Zeros (taps in the padding, channels beyond the impulse)
   must come out exactly 0.  Catches a lost or misplaced operand plane: a lost `lo` plane is an error of up to 2^-11.
   Winograd, sub-case (2): a one-hot x makes V = +-1 at up to three positions of a pair's window, so an output is a sum / difference of
   up to three transformed weights of ONE filter row (g0, g1, g2): one-hot d1 -> Y0 = U1 - U2 = g1, Y1 = U1 + U2 - U3 = g0; d2 -> Y0 =
   U1 + U2 - U0 = g2, Y1 = U1 - U2 = g1; d0 -> Y0 = U0; d3 -> Y1 = U3; everything else exact zeros.  Each U is formed in fp64, rounded
   to fp32 (2^-24 |U|) and split into two fp16 planes of the row-scaled value (22 bits: 2^-22 |U|): <= 1.25 * 2^-22 |U| each.  With
   |U1|, |U2| <= S / 2, |U0|, |U3| <= S, S = |g0| + |g1| + |g2|, the three of a sum hold <= 1.25 * 2^-22 * 2 S = 0.625 * 2^-20 S.  The
   products with V = +-1 are exact (hi and lo plane of each U: up to six terms), their fp32 sum rounds at most six times at a partial
   sum of at most S: 6 * 2^-24 S = 0.375 * 2^-20 S.  All other channels and chunks add exact zeros, the epilogue's scale is a power
   of two.  Bar: |err| <= 2^-20 * scale * S of the filter row read; outputs whose reference is 0 must be exactly 0.
   Sub-case (1) is left out for Winograd: with impulse WEIGHTS an output is x at one pixel, but it is computed as V0 + (V1 + V2) / 2
   and the like -- the error is bounded by the planes of the NEIGHBOURING pixels' values, not by the value that comes out, so there is
   no "one operand value" bar; A and C cover that path.
C. random values against fp64 (the `conv2d_nhwc` entry points).  x = randn.relu() * 3, He-scaled weights whose centre taps are
   multiplied by logspace(-3, 1, K) (the row-scaling case), a FrozenBN-like affine, a residual on the rows whose route takes one.
   Arithmetic cap, per element: |y - ref64| <= (2^-21 + n 2^-24) * sum|x||w| * |scale| with n the contraction length (2^-23 in place
   of 2^-21 for bf16x3 and f32): a bound, not a measurement.  It bounds the sum and its scaling, not the roundings of "+ shift +
   residual" (2^-24 |y| each, far above the cap where a logspace row makes sum |x||w| 1e-3 of the residual), so it is held on a second
   launch of the layer with the scale alone (the register-staged row, whose route needs a residual, gets one of exact zeros), where
   torch's fp32 evaluation is asserted to meet it as well.  Noise bar (full epilogue): norm-relative and max-abs error against fp64,
   each at most K_NOISE = 3 times the same statistic of torch's fp32 CPU conv2d on the same inputs (clamped from below by one fp32
   rounding of the result, as `helpers.assert_noise` does).  The GELU epilogue gets one C case per kernel of kernels._GELU_EPILOGUE against fp64
   gelu (noise bar only: the cap above is a statement about the convolution sum, which the same kernels' plain cases hold).

Shapes the issue lists that are run differently: (1, 13, 21, 16, 64) 3x3 -- `pack_conv` and the fp32 kernel take multiples of 32 input
channels only, so the row is launched zero-padded to 32 channels (CONV_HALO off keeps it on lvc_conv2d_nhwc_f32); (1, 13, 21, 32, 32)
3x3 is added as the fp32 route a layer really reaches (fewer than 64 output channels).  lvc_set_halo_test_hooks is read by
lvc_conv3x3_nhwc_bf16x3 alone: the "3,70" / "10,24" patches run there.

Largest measured ours / noise of C on an MI355X, per entry point over all its rows (norm-relative, max-abs; K = 3):
   lvc_conv2d_nhwc_f32           1.00, 0.79      lvc_conv3x3_nhwc_bf16x3       1.34, 1.70
   lvc_conv2d_nhwc_bf16x3        1.29, 1.29      lvc_conv3x3_nhwc_f16x2        2.00, 1.99
   lvc_conv2d_nhwc_f16x2         0.48, 0.38      lvc_conv3x3_nhwc_f16x2_pipe   2.00, 1.99
   lvc_conv2d_nhwc_f16x2_dma     0.87, 0.77      lvc_conv3x3_nhwc_f16s1        1.24, 1.09
   lvc_conv1x1_nhwc_f16x2_pipe   0.86, 0.77      lvc_conv3x3_nhwc_wino         1.08, 0.99
   lvc_conv1x1_nhwc_f16s1        0.71, 0.54      GELU epilogue: f16x2_pipe 0.82, 0.71; f16s1 0.63, 0.49; f16s1_w2 0.72, 0.58;
   lvc_conv1x1_nhwc_f16s1_w2     0.73, 0.54                     f16x2_dma 0.82, 0.71
No shape is dropped from C.  A, B and the arithmetic cap hold on every row.  Reproduced by A (ADVICE.md had named it): the presplit
producer compared the SCALED value (x 2^4) with the consumer's limit of 4094 and raised conv3's range word for any conv2 output
above 255.9 (fixed in csrc/conv3x3_halo_s1.hip; the presplit case below asserts that its hand-over tensor exceeds 255.9).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import (FWD_CASES, FWD_FUSED, FWD_SWITCHES, K_NOISE, assert_impulse, assert_noise, full, fwd_case_id, fwd_route, fwd_set_switches, gen, ids,
                     ints, out_hw, pow2)

pytestmark = pytest.mark.gpu

_WORST = {}      # entry point -> largest ours / noise of this run (norm-relative, max-abs): printed when the module is done
PITCH = 12       # floats an output row is wider than K in the pitched epilogue
CASE_IDS = [fwd_case_id(c) for c in FWD_CASES]


def _dev():
    return torch.device("cuda:0")


def _engine(entry):
    """The row of B's bars an entry point belongs to."""
    return "f32" if entry.endswith("_f32") else "bf16x3" if "bf16x3" in entry else "f16x2"


def _conv_ref(x, w, stride, pad, dtype=torch.float64):
    """conv2d of x [N,H,W,C] with w [K,C,R,R] on the CPU -> [N,Ho,Wo,K]."""
    return F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()


def _epilogue(conv, scale, shift, res, res_mode, relu, act=None):
    y = conv
    if scale is not None:
        y = y * scale.to(conv.dtype)
    if shift is not None:
        y = y + shift.to(conv.dtype)
    if res_mode == 1:
        y = y + res.to(conv.dtype)
    elif res_mode == 2:
        y = y + res.to(conv.dtype).repeat_interleave(2, 1).repeat_interleave(2, 2)
    if relu:
        y = y.relu()
    return F.gelu(y) if act == "gelu" else y


class _Recorded:
    """`kernels._launch` wrapped: the entry points that ran, in order."""

    def __init__(self, Kn, monkeypatch):
        self.ran = []
        launch = Kn._launch
        monkeypatch.setattr(Kn, "_launch", lambda tag, flops, nbytes, slot, what, call: (self.ran.append(what), launch(tag, flops, nbytes, slot, what, call))[1])


def _conv(Kn, monkeypatch, case, x, w, scale=None, shift=None, relu=False, res=None, res_mode=0, pitch=0, act=None):
    """`conv2d_nhwc` (`linear` for the linear row) of `case` under its switches: asserts the route first (the pure `conv_route`), that
    the launch that ran is that entry point, and the error word.  x [N,H,W,C], w [K,C,R,R] on the CPU -> y [N,Ho,Wo,K] on the CPU."""
    from lvc_amd import _lib

    N, H, W, C, Kc, R, stride, pad = case.shape
    o, dev = case.opts, _dev()
    Ho, Wo = out_hw(H, W, R, stride, pad)
    fwd_set_switches(monkeypatch, Kn, case)
    assert fwd_route(Kn, case, res_mode, Kc + pitch if pitch else None) == case.entry
    dv = lambda t: t.to(dev) if t is not None else None
    if o.get("stem"):
        xl = torch.zeros(N, H, W, 4)
        xl[..., :3] = x
        pc = Kn.pack_conv(w.to(dev), stride=stride, pad=pad, stem=True, affine=(dv(scale), dv(shift)))
    elif o.get("linear"):
        xl = x
        pc = Kn.pack_linear(w.view(Kc, C).to(dev), dv(shift))
        pc.scale = dv(scale)
    else:
        cp = o.get("pad_c", C)
        xl = F.pad(x, (0, cp - C))
        pc = Kn.pack_conv(F.pad(w, (0, 0, 0, 0, 0, cp - C)).to(dev), stride=stride, pad=pad, affine=(dv(scale), dv(shift)))
        pc.two_acc = bool(o.get("two_acc"))
    out = torch.full((N, Ho, Wo, Kc + pitch), 1000.0, device=dev) if pitch else None
    streamk = Kn.WINO_STREAMK
    rec = _Recorded(Kn, monkeypatch)
    Kn.clear_conv_error_word(dev)
    try:
        if "streamk" in o:
            Kn.set_wino_streamk(o["streamk"])
        if "force" in o:
            _lib.lib().lvc_set_halo_test_hooks(*(o.get("patch", (0, 0)) + (1,)))
        if o.get("linear") and not (pitch or res_mode or act):
            y = Kn.linear(xl.view(N, C).to(dev), pc, relu=relu).view(N, 1, 1, Kc)
        else:
            y = Kn.conv2d_nhwc(xl.to(dev), pc, relu=relu, residual=dv(res), res_mode=res_mode, out=out, act=act)
        y = y.cpu()
    finally:
        if "streamk" in o:
            Kn.set_wino_streamk(streamk)
        if "force" in o:
            _lib.lib().lvc_set_halo_test_hooks(0, 0, 0)
    assert rec.ran == [case.entry], rec.ran
    assert Kn.conv_error_word(dev) == 0
    if pitch:
        assert bool((y[..., Kc:] == 1000.0).all()), "the launch wrote past K in a wider row"
        y = y[..., :Kc].contiguous()
    return y


def _assert_bit_equal(got, ref, what):
    """A's assertion: the count of wrong elements and the first few (n, y, x, k) with got / want."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if torch.equal(got, ref):
        return
    bad = (got != ref).nonzero()
    first = ["%s got %r want %r" % (tuple(i.tolist()), float(got[tuple(i)]), float(ref[tuple(i)])) for i in bad[:6]]
    raise AssertionError("%s: %d of %d elements differ, max |d| %g; first: %s" % (what, len(bad), ref.numel(), float((got - ref).abs().max()), "; ".join(first)))


def _assert_exact_ref(ref, *intermediates):
    """What makes A exact, checked on the CPU: multiples of 0.5 below 2^22, intermediates within the one-accumulator range."""
    assert torch.equal(ref, (ref * 2).round() / 2) and float(ref.abs().max()) < 2 ** 22
    for t in intermediates:
        assert torch.equal(t, (t * 2).round() / 2) and float(t.abs().max()) <= 4094


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    for entry in sorted(_WORST):
        print("largest ours / noise, %-30s norm-rel %.2f  max-abs %.2f  (K = %g)" % (entry, _WORST[entry][0], _WORST[entry][1], K_NOISE))


# ===================================================================================================== A. conv2d_nhwc, integer-exact
EPILOGUES = (      # name, affine, relu, res_mode, pitch
    ("none", False, False, 0, 0), ("affine_relu", True, True, 0, 0), ("res1_relu", True, True, 1, 0), ("res2", True, False, 2, 0),
    ("pitched", True, False, 0, PITCH), ("pitched_res1", True, True, 1, PITCH))


@functools.lru_cache(maxsize=None)
def _int_case(shape):
    N, H, W, C, Kc, R, stride, pad = shape
    Ho, Wo = out_hw(H, W, R, stride, pad)
    g = gen(shape, 31)
    x, w, scale, shift = ints(g, (N, H, W, C), 7), ints(g, (Kc, C, R, R), 3), pow2(g, Kc), ints(g, (Kc,), 5)
    zero_row = Kc // 2 + 1
    w[zero_row] = 0.0
    res1 = ints(g, (N, Ho, Wo, Kc), 9)
    res2 = ints(g, (N, Ho // 2, Wo // 2, Kc), 9) if Ho % 2 == 0 and Wo % 2 == 0 else None
    return x, w, scale, shift, res1, res2, zero_row, _conv_ref(x, w, stride, pad)


@pytest.mark.parametrize("case", FWD_CASES, ids=CASE_IDS)
def test_forward_integer_exact(case, monkeypatch):
    from lvc_amd import kernels as Kn

    x, w, scale, shift, res1, res2, zero_row, conv = _int_case(case.shape)
    Kc = case.shape[4]
    assert float(x.abs().max()) <= 4094
    fwd_set_switches(monkeypatch, Kn, case)
    ran = []
    for name, affine, relu, res_mode, pitch in EPILOGUES:
        res = res1 if res_mode == 1 else res2 if res_mode == 2 else None
        if (res_mode and res is None) or fwd_route(Kn, case, res_mode, Kc + pitch if pitch else None) != case.entry:
            continue      # an odd map has no upsample-add; under this epilogue the layer is another entry point's
        sc, sh = (scale, shift) if affine else (None, None)
        ref = _epilogue(conv, sc, sh, res, res_mode, relu)
        _assert_exact_ref(ref)
        want0 = _epilogue(torch.zeros_like(conv[..., zero_row]), None, sh[zero_row] if affine else None, res[..., zero_row] if res_mode else None,
                          res_mode, relu)
        assert torch.equal(ref[..., zero_row], want0)      # the all-zero weight row: shift (+ residual)
        got = _conv(Kn, monkeypatch, case, x, w, sc, sh, relu, res, res_mode, pitch)
        _assert_bit_equal(got, ref.float(), "%s, epilogue %s" % (fwd_case_id(case), name))
        ran.append(name)
    assert ran and ("res" not in case.opts or any(n.startswith("res%d" % case.opts["res"]) for n in ran)), ran


# ============================================================================================ B. conv2d_nhwc, impulse, full mantissas
@pytest.mark.parametrize("case", [c for c in FWD_CASES if "wino" not in c.entry], ids=[i for i in CASE_IDS if "wino" not in i])
def test_forward_impulse_weights_copy_x(case, monkeypatch):
    """B (1): w[k] is a single 1.0 at (channel, tap) = f(k); every output is one x value or, where the tap lies in the padding, 0."""
    from lvc_amd import kernels as Kn

    N, H, W, C, Kc, R, stride, pad = case.shape
    g = gen(case.shape, 32)
    x = full(g, (N, H, W, C))
    w = torch.zeros(Kc, C, R, R)
    k = torch.arange(Kc)
    w[k, (k * 5 + 1) % C, (k % (R * R)) // R, k % R] = 1.0
    ref = _conv_ref(x, w, stride, pad)
    assert int((ref != 0).sum()) > 0 and bool(torch.isin(ref, torch.cat([x.double().flatten(), torch.zeros(1, dtype=torch.float64)])).all())
    res_mode = case.opts.get("res", 0)      # a route that needs its residual operand gets zeros
    Ho, Wo = out_hw(H, W, R, stride, pad)
    res = torch.zeros(N, Ho // 2, Wo // 2, Kc) if res_mode == 2 else torch.zeros(N, Ho, Wo, Kc) if res_mode else None
    got = _conv(Kn, monkeypatch, case, x, w, res=res, res_mode=res_mode)
    assert_impulse(got, ref, _engine(case.entry))


def _one_hot_positions(H, W, C):
    return ((0, 0, 0), (H - 1, W - 1, C - 1), (H // 2, W - 1, C // 2))


@pytest.mark.parametrize("case", FWD_CASES, ids=CASE_IDS)
def test_forward_one_hot_x_copies_the_scaled_weights(case, monkeypatch):
    """B (2): one 1.0 per image in x (first pixel / first channel, last pixel / last channel, right border / a middle channel, rotating
    over the images and three launches); every output is scale[k] * w[k, c, tap] or exactly 0.  Winograd: the bar of the docstring."""
    from lvc_amd import kernels as Kn

    N, H, W, C, Kc, R, stride, pad = case.shape
    g = gen(case.shape, 33)
    w, scale = full(g, (Kc, C, R, R), 0.0625), pow2(g, Kc)
    res_mode = case.opts.get("res", 0)
    Ho, Wo = out_hw(H, W, R, stride, pad)
    res = torch.zeros(N, Ho // 2, Wo // 2, Kc) if res_mode == 2 else torch.zeros(N, Ho, Wo, Kc) if res_mode else None
    pos = _one_hot_positions(H, W, C)
    for j in range(3):
        x = torch.zeros(N, H, W, C)
        for n in range(N):
            y0, x0, c0 = pos[(j + n) % 3]
            x[n, y0, x0, c0] = 1.0
        ref = _conv_ref(x, w, stride, pad) * scale.double()
        assert int((ref != 0).sum()) > 0
        got = _conv(Kn, monkeypatch, case, x, w, scale, res=res, res_mode=res_mode)
        if "wino" in case.entry:
            rows = w.double().abs().sum(3, keepdim=True).expand(-1, -1, -1, 3)      # S = |g0| + |g1| + |g2| of the filter row read
            bar = 2.0 ** -20 * _conv_ref(x, rows, stride, pad) * scale.double()
            err = (got.double() - ref).abs()
            bad = (err > bar) | ((ref == 0) & (got != 0))
            assert not bool(bad.any()), (j, int(bad.sum()), float((err / bar.clamp_min(1e-300))[bad].max()), int(((ref == 0) & (got != 0)).sum()))
        else:
            assert_impulse(got, ref, _engine(case.entry))


# ======================================================================================================= C. conv2d_nhwc against fp64
@functools.lru_cache(maxsize=None)
def _rand_case(shape):
    N, H, W, C, Kc, R, stride, pad = shape
    Ho, Wo = out_hw(H, W, R, stride, pad)
    g = gen(shape, 34)
    x = torch.randn(N, H, W, C, generator=g).relu_() * 3.0
    w = torch.randn(Kc, C, R, R, generator=g) * (2.0 / (C * R * R)) ** 0.5
    w[:, :, R // 2, R // 2] *= torch.logspace(-3, 1, Kc)[:, None]          # rows of very different magnitude: the row scaling's case
    scale = (torch.rand(Kc, generator=g) + 0.5) * (torch.rand(Kc, generator=g) + 0.5 + 1e-5).rsqrt()
    shift = torch.randn(Kc, generator=g) * 0.1 - torch.randn(Kc, generator=g) * 0.1 * scale
    res1 = torch.randn(N, Ho, Wo, Kc, generator=g)
    res2 = torch.randn(N, Ho // 2, Wo // 2, Kc, generator=g) if Ho % 2 == 0 and Wo % 2 == 0 else None
    mass = _conv_ref(x.abs(), w.abs(), stride, pad) * scale.double().abs()      # sum |x||w| |scale| per output element
    return x, w, scale, shift, res1, res2, _conv_ref(x, w, stride, pad), _conv_ref(x, w, stride, pad, torch.float32), mass


def _cap(case, mass):
    N, H, W, C, Kc, R, stride, pad = case.shape
    return ((2.0 ** -21 if _engine(case.entry) == "f16x2" else 2.0 ** -23) + C * R * R * 2.0 ** -24) * mass


@pytest.mark.parametrize("case", FWD_CASES, ids=CASE_IDS)
def test_forward_random_within_the_cap_and_the_fp32_noise(case, monkeypatch):
    from lvc_amd import kernels as Kn

    x, w, scale, shift, res1, res2, conv64, conv32, mass = _rand_case(case.shape)
    fwd_set_switches(monkeypatch, Kn, case)
    res_mode = case.opts.get("res", 1)
    if fwd_route(Kn, case, res_mode) != case.entry or (res_mode == 2 and res2 is None):
        res_mode = 0      # a route that takes no residual (Winograd)
    res = res1 if res_mode == 1 else res2 if res_mode == 2 else None
    ref64, ref32 = _epilogue(conv64, scale, shift, res, res_mode, False), _epilogue(conv32, scale, shift, res, res_mode, False)
    got = _conv(Kn, monkeypatch, case, x, w, scale, shift, False, res, res_mode)
    r_rel, r_max = assert_noise(_WORST, fwd_case_id(case), case.entry, got, ref32, ref64)
    assert max(r_rel, r_max) <= K_NOISE, (r_rel, r_max)
    # the arithmetic cap is a bound on the convolution sum times the scale: it has no term for the roundings of "+ shift + residual"
    # (2^-24 |y| each, with |y| up to the residual's size where sum |x||w| is 1e-3 of it: the logspace rows), so it is held on a launch
    # of the same layer with the scale alone -- where torch's own fp32 evaluation has to meet it too
    zero = None
    if res_mode and fwd_route(Kn, case, 0) != case.entry:
        zero = torch.zeros_like(res)      # the register-staged row keeps its route with a residual only: exact zeros do not round
    cap = _cap(case, mass)
    assert bool(((conv32.double() * scale.double() - conv64 * scale.double()).abs() <= cap).all())
    plain = _conv(Kn, monkeypatch, case, x, w, scale, res=zero, res_mode=res_mode if zero is not None else 0)
    over = (plain.double() - conv64 * scale.double()).abs() / cap.clamp_min(1e-300)
    assert float(over.max()) <= 1.0, ("arithmetic cap", float(over.max()), int((over > 1).sum()))


def _gelu_cases():
    from_entry = {}
    for c in FWD_CASES:
        if "res" not in c.opts:
            from_entry.setdefault(c.entry, c)
    return from_entry


@pytest.mark.parametrize("entry", ("lvc_conv1x1_nhwc_f16x2_pipe", "lvc_conv1x1_nhwc_f16s1", "lvc_conv1x1_nhwc_f16s1_w2", "lvc_conv2d_nhwc_f16x2_dma"))
def test_forward_gelu_epilogue_within_the_fp32_noise(entry, monkeypatch):
    """torch.nn.GELU() in the epilogue of the kernels that have it (kernels._GELU_EPILOGUE), against fp64 gelu of the fp64 layer."""
    from lvc_amd import kernels as Kn

    assert set(Kn._GELU_EPILOGUE) == {"lvc_conv1x1_nhwc_f16x2_pipe", "lvc_conv1x1_nhwc_f16s1", "lvc_conv1x1_nhwc_f16s1_w2", "lvc_conv2d_nhwc_f16x2_dma"}
    case = _gelu_cases()[entry]
    x, w, scale, shift, _, _, conv64, conv32, _ = _rand_case(case.shape)
    ref64, ref32 = _epilogue(conv64, scale, shift, None, 0, False, "gelu"), _epilogue(conv32, scale, shift, None, 0, False, "gelu")
    got = _conv(Kn, monkeypatch, case, x, w, scale, shift, act="gelu")
    r_rel, r_max = assert_noise(_WORST, "gelu " + fwd_case_id(case), "gelu " + entry, got, ref32, ref64)
    assert max(r_rel, r_max) <= K_NOISE, (r_rel, r_max)


# ================================================================================ A. the fused and multi-map launches, integer-exact
def _switches(monkeypatch, Kn, **over):
    for name, value in dict(FWD_SWITCHES, **over).items():
        monkeypatch.setattr(Kn, name, value)


def _sparse(g, shape, m, keep):
    """Integers in [-m, m], a fraction `keep` of them kept: the operands of the chained launches."""
    return ints(g, shape, m) * (torch.rand(shape, generator=g) < keep).float()


def _affine(g, n, scales=(0.5, 1.0, 2.0, 4.0), m=5):
    return torch.tensor(scales)[torch.randint(0, len(scales), (n,), generator=g)], ints(g, (n,), m)


def _dv(ts):
    return tuple(t.to(_dev()) if t is not None else None for t in ts)


LEVEL_MAPS = ((13, 21), (7, 11), (4, 6))


@pytest.mark.parametrize("two_acc", (False, True), ids=("one_acc", "two_acc"))
@pytest.mark.parametrize("shared", (True, False), ids=("levels", "layers"))
def test_conv3x3_levels_integer_exact(shared, two_acc, monkeypatch):
    """`conv3x3_levels` over three small maps, N = 2, C = K = 128: the shared layer (lvc_conv3x3_nhwc_f16_levels) and a layer per map
    (lvc_conv3x3_nhwc_f16_layers), in the one- and the two-accumulator form; stream-K splits the few tiles by chunk."""
    from lvc_amd import kernels as Kn

    _switches(monkeypatch, Kn)
    dev, N, C = _dev(), 2, 128
    g = gen((N, C, int(shared), int(two_acc)), 41)
    xs = [ints(g, (N, h, w, C), 7) for h, w in LEVEL_MAPS]
    layers = [(ints(g, (C, C, 3, 3), 3),) + _affine(g, C) for _ in range(1 if shared else len(xs))]
    refs = []
    for i, x in enumerate(xs):
        w, sc, sh = layers[0 if shared else i]
        refs.append(_epilogue(_conv_ref(x, w, 1, 1), sc, sh, None, 0, shared))
        _assert_exact_ref(refs[-1])
    pcs = []
    for w, sc, sh in layers:
        pcs.append(Kn.pack_conv(w.to(dev), stride=1, pad=1, affine=_dv((sc, sh))))
        pcs[-1].two_acc = two_acc
    rec = _Recorded(Kn, monkeypatch)
    Kn.clear_conv_error_word(dev)
    outs = Kn.conv3x3_levels([x.to(dev) for x in xs], pcs[0] if shared else pcs, relu=shared)
    assert rec.ran == [FWD_FUSED["levels" if shared else "layers"]], rec.ran
    assert all(pc.last_one == (not two_acc) for pc in pcs)
    for i, (o, ref) in enumerate(zip(outs, refs)):
        _assert_bit_equal(o.cpu(), ref.float(), "map %d" % i)
    assert Kn.conv_error_word(dev) == 0


@pytest.mark.parametrize("wino", (False, True), ids=("direct", "wino"))
@pytest.mark.parametrize("pred_k", (3, 15))
def test_conv3x3_levels_pred_integer_exact(pred_k, wino, monkeypatch):
    """relu(conv3x3) -> 1x1 predictor in one launch (lvc_conv3x3_nhwc_f16_levels_pred; under WINO_RPN one lvc_conv3x3_nhwc_wino_pred
    launch per map): the two 128-channel slices of the 256-channel hidden map meet in atomics on the zeroed output, exact on integers."""
    from lvc_amd import kernels as Kn

    _switches(monkeypatch, Kn, CONV_WINO=wino, WINO_RPN=wino)
    dev, N, C, Kh = _dev(), 2, 128, 256      # 256 hidden channels: two 128-channel slices per output element
    g = gen((N, C, pred_k), 42)
    xs = [_sparse(g, (N, h, w, C), 3, 0.5) for h, w in LEVEL_MAPS]
    wc, (sc, tc) = _sparse(g, (Kh, C, 3, 3), 1, 0.5), _affine(g, Kh, (1.0, 2.0), 3)
    wp, (sp, tp) = ints(g, (pred_k, Kh, 1, 1), 3), _affine(g, pred_k)
    refs = []
    for x in xs:
        hidden = _epilogue(_conv_ref(x, wc, 1, 1), sc, tc, None, 0, True)
        refs.append(_epilogue(_conv_ref(hidden, wp, 1, 0), sp, tp, None, 0, False))
        _assert_exact_ref(refs[-1], hidden)
    pc = Kn.pack_conv(wc.to(dev), stride=1, pad=1, affine=_dv((sc, tc)))
    pc.two_acc = True
    pred = Kn.pack_conv(wp.to(dev), affine=_dv((sp, tp)))
    rec = _Recorded(Kn, monkeypatch)
    Kn.clear_conv_error_word(dev)
    outs = Kn.conv3x3_levels_pred([x.to(dev) for x in xs], pc, pred, relu=True)
    assert outs is not None
    assert rec.ran == ([FWD_FUSED["wino_pred"]] * len(xs) if wino else [FWD_FUSED["levels_pred"]]), rec.ran
    for i, (o, ref) in enumerate(zip(outs, refs)):
        _assert_bit_equal(o.cpu(), ref.float(), "map %d" % i)
    assert Kn.conv_error_word(dev) == 0


@pytest.mark.parametrize("with_res", (False, True), ids=("plain", "residual"))
def test_presplit_pair_integer_exact(with_res, monkeypatch):
    """`conv3x3_conv1x1_presplit` at (2, 33, 32, 64, 64 -> 256): conv2 hands conv3 its operand planes; 2112 rows (a 64-row tail)."""
    from lvc_amd import kernels as Kn

    _switches(monkeypatch, Kn, PRESPLIT=True)
    dev, N, H, W, C, Kc = _dev(), 2, 33, 32, 64, 256
    g = gen((N, H, W, C, Kc), 43)
    x = _sparse(g, (N, H, W, C), 3, 0.5)
    w2, (s2, t2) = _sparse(g, (C, C, 3, 3), 2, 0.5), _affine(g, C, (1.0, 2.0), 3)
    w3, (s3, t3) = ints(g, (Kc, C, 1, 1), 3), _affine(g, Kc)
    res = ints(g, (N, H, W, Kc), 9) if with_res else None
    mid = _epilogue(_conv_ref(x, w2, 1, 1), s2, t2, None, 0, True)
    ref = _epilogue(_conv_ref(mid, w3, 1, 0), s3, t3, res, 1 if with_res else 0, True)
    _assert_exact_ref(ref, mid)
    assert float(mid.max()) > 4094 / 16      # inside the consumer's range, beyond a sixteenth of it: the range word must stay 0
    p2 = Kn.pack_conv(w2.to(dev), stride=1, pad=1, affine=_dv((s2, t2)))
    p3 = Kn.pack_conv(w3.to(dev), affine=_dv((s3, t3)))
    rec = _Recorded(Kn, monkeypatch)
    Kn.clear_conv_error_word(dev)
    y = Kn.conv3x3_conv1x1_presplit(x.to(dev), p2, p3, residual=res.to(dev) if with_res else None, relu=True)
    assert rec.ran == [FWD_FUSED["presplit_3x3"], FWD_FUSED["presplit_1x1"]], rec.ran
    _assert_bit_equal(y.cpu(), ref.float(), "presplit pair")
    assert Kn.conv_error_word(dev) == 0


@pytest.mark.parametrize("shape", ((64, 256, 64), (128, 256, 64), (128, 512, 128)), ids=ids)
def test_conv1x1_chain_integer_exact(shape, monkeypatch):
    """`conv1x1_chain` on every kernels.CHAIN_SHAPES: M = 2 * 128 + 45 rows (a ragged last workgroup), x rows 32 floats wider than the
    contraction (the other columns hold a large integer), the shortcut add on the first layer."""
    from lvc_amd import kernels as Kn

    assert shape in Kn.CHAIN_SHAPES and len(Kn.CHAIN_SHAPES) == 3
    _switches(monkeypatch, Kn)
    K1, N1, N2 = shape
    dev, M, ldx = _dev(), 128 * 2 + 45, K1 + 32
    g = gen(shape, 44)
    x = torch.full((M, 1, 1, ldx), 1000.0)
    x[..., :K1] = _sparse(g, (M, 1, 1, K1), 3, 0.5).abs()
    r = ints(g, (M, 1, 1, N1), 9)
    wa, (sa, ta) = ints(g, (N1, K1, 1, 1), 2), _affine(g, N1, (1.0, 2.0), 3)
    wb, (sb, tb) = _sparse(g, (N2, N1, 1, 1), 2, 0.5), _affine(g, N2)
    r1 = _epilogue(_conv_ref(x[..., :K1], wa, 1, 0), sa, ta, r, 1, True)
    r2 = _epilogue(_conv_ref(r1, wb, 1, 0), sb, tb, None, 0, True)
    _assert_exact_ref(r2, r1)
    ch = Kn.pack_chain(Kn.pack_conv(wa.to(dev), affine=_dv((sa, ta))), Kn.pack_conv(wb.to(dev), affine=_dv((sb, tb))))
    rec = _Recorded(Kn, monkeypatch)
    Kn.clear_conv_error_word(dev)
    y1, y2 = Kn.conv1x1_chain(x.to(dev), ch, residual=r.to(dev))
    assert rec.ran == [FWD_FUSED["chain"]], rec.ran
    _assert_bit_equal(y1.cpu(), r1.float(), "first layer")
    _assert_bit_equal(y2.cpu(), r2.float(), "second layer")
    assert Kn.conv_error_word(dev) == 0


@pytest.mark.parametrize("proj", (False, True), ids=("identity", "projection"))
@pytest.mark.parametrize("shape", ((1, 1, 1), (2, 13, 70), (3, 9, 31)), ids=ids)
def test_bottleneck_fused_integer_exact(shape, proj, monkeypatch):
    """`bottleneck_fused` on both kernels.BNECK_SHAPES: a single pixel, ragged tiles in both directions, more than one image."""
    from lvc_amd import kernels as Kn

    _switches(monkeypatch, Kn)
    N, H, W = shape
    cin = 64 if proj else 256
    assert (cin, 64, 256, proj) in Kn.BNECK_SHAPES and len(Kn.BNECK_SHAPES) == 2
    dev = _dev()
    g = gen(shape + (cin,), 45)
    x = _sparse(g, (N, H, W, cin), 3, 0.25).abs()
    w1, (s1, t1) = _sparse(g, (64, cin, 1, 1), 1, 0.5), _affine(g, 64, (1.0, 2.0), 2)
    w2, (s2, t2) = _sparse(g, (64, 64, 3, 3), 1, 0.25), _affine(g, 64, (1.0, 2.0), 2)
    w3, (s3, t3) = ints(g, (256, 64, 1, 1), 2), _affine(g, 256, (1.0, 2.0), 5)
    ws, (ss, ts) = ints(g, (256, cin, 1, 1), 3), _affine(g, 256, (1.0, 2.0), 5)
    a1 = _epilogue(_conv_ref(x, w1, 1, 0), s1, t1, None, 0, True)
    a2 = _epilogue(_conv_ref(a1, w2, 1, 1), s2, t2, None, 0, True)
    short = _epilogue(_conv_ref(x, ws, 1, 0), ss, ts, None, 0, False) if proj else x.double()
    ref = (_epilogue(_conv_ref(a2, w3, 1, 0), s3, t3, None, 0, False) + short).relu()
    _assert_exact_ref(ref, a1, a2)
    p1, p2 = Kn.pack_conv(w1.to(dev), affine=_dv((s1, t1))), Kn.pack_conv(w2.to(dev), pad=1, affine=_dv((s2, t2)))
    if proj:      # BottleneckBlock._fused_projection: [conv3 | shortcut] over [conv2 output | block input], scales folded into the weights
        wf = torch.cat([w3 * s3.view(-1, 1, 1, 1), ws * ss.view(-1, 1, 1, 1)], 1).contiguous()
        p3 = Kn.pack_conv(wf.to(dev), affine=(None, (t3 + ts).to(dev)))
    else:
        p3 = Kn.pack_conv(w3.to(dev), affine=_dv((s3, t3)))
    bk = Kn.pack_bottleneck(p1, p2, p3, proj)
    rec = _Recorded(Kn, monkeypatch)
    Kn.clear_conv_error_word(dev)
    y = Kn.bottleneck_fused(x.to(dev), bk)
    assert rec.ran == [FWD_FUSED["bottleneck"]], rec.ran
    _assert_bit_equal(y.cpu(), ref.float(), "fused bottleneck")
    assert Kn.conv_error_word(dev) == 0


@pytest.mark.parametrize("shape", ((1, 37, 41), (2, 14, 18)), ids=ids)
def test_stem_conv_pool_integer_exact(shape, monkeypatch):
    """`stem_conv_pool`: conv 7x7 / 2 + affine + ReLU + max-pool 3x3 / 2 in one launch, odd and even maps whose patches straddle the borders."""
    from lvc_amd import kernels as Kn

    _switches(monkeypatch, Kn)
    N, H, W = shape
    dev = _dev()
    g = gen(shape, 46)
    x, w, (sc, sh) = ints(g, (N, H, W, 3), 7), ints(g, (64, 3, 7, 7), 3), _affine(g, 64)
    act = _epilogue(_conv_ref(x, w, 2, 3), sc, sh, None, 0, True)
    ref = F.max_pool2d(act.permute(0, 3, 1, 2), kernel_size=3, stride=2, padding=1).permute(0, 2, 3, 1).contiguous()
    _assert_exact_ref(ref)
    x4 = torch.zeros(N, H, W, 4)
    x4[..., :3] = x
    pc = Kn.pack_conv(w.to(dev), stride=2, pad=3, stem=True, affine=_dv((sc, sh)))
    Kn.clear_conv_error_word(dev)
    y = Kn.stem_conv_pool(x4.to(dev), pc)
    _assert_bit_equal(y.cpu(), ref.float(), "fused stem")
    assert Kn.conv_error_word(dev) == 0
