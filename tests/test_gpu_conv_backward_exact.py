"""Exact and fp64 tests of the kernels that carry the gradient: the weight gradient (csrc/conv_wgrad.hip: `kernels.conv_wgrad` on the
bf16x3 / f32 / f16x2 engines, the grouped launch + its finalize pass, the pitched dy of the C ABI), the data gradient
(`kernels.pack_conv_dgrad` + `kernels.conv_dgrad` on the forward kernels), the grouped 3x3 kernels (csrc/conv_grouped.hip) and
`kernels.relu_backward`.  Three kinds of test, each aimed at another way of being wrong, none with a tolerance that was chosen:

A. integer-exact.  x holds integers in [-7, 7], dy and the weights integers in [-3, 3], the per-channel scale is one of {0.5, 1, 2, 4}:
   every operand is exact in bf16 and fp16, every product and partial sum an integer (or a multiple of 0.5) far below 2^24, so every
   engine, in any summation order, atomics included, must return the fp64 reference bit for bit.  Catches indexing: a dropped chunk, a
   slice edge counted twice, a wrong tap offset, a tail channel read from its neighbour.
B. impulse with full mantissas.  One operand is 0 / 1.0 with a single 1.0 per channel, the other has full fp32 mantissas: every
   result is ONE operand value (or exactly 0).  f32 routes: bit-equal; bf16x3: |err| <= 2^-23 |v| (hi + mid + lo == v exactly, the kept
   products with 1.0 are summed in fp32: at most one rounding); f16x2: |err| <= 2^-21 |v| (two fp16 planes carry 22 bits; values are
   drawn inside fp16's normal range and the conv error word must stay 0).  Catches a lost or misplaced operand plane: a lost `lo`
   plane is an error of up to 2^-17.
C. random gradient-sized values against fp64.  dy = randn * 10^-e, e in {2, 5, 8} (the wide-range log-normal dy of
   test_gpu_backward.py for f16x2); the norm-relative and the max-abs error of the kernel, both against the fp64 reference, must stay
   within K x the same two statistics of torch's fp32 CPU evaluation of the same inputs (the noise).  The noise is clamped from below
   by what storing the fp64 result as fp32 costs: 2^-25 (norm-relative, the r.m.s. of a rounding) and 2^-24 max|ref| (max-abs).
   K = 3 (K_NOISE of test_gpu_grouped_conv.py); 4 for the bf16x3 weight gradient (below).

Largest measured ours / noise of C on an MI355X, per engine over all its shapes (norm-relative, max-abs):
   weight gradient   bf16x3 1.92, 3.05 (K = 4: 3.05 at 3x5x7x32x36 3x3, dy 1e-8, against measured noise; the f32 engine has 2.60 there)
                     f32    2.29, 2.60 (K = 3)
                     f16x2  1.78, 1.66 (K = 3) over the seventeen shapes; at 16 / 17 / 31 pixels, the shortest sums the fp16 kernel
                            itself runs, 1.20, 1.07 / 1.78, 1.41 / 0.91, 0.64.  The shapes with fewer than 16 pixels run the exact fp32
                            form (lvc_conv_wgrad_nhwc_f16x2) and measure 0.75 .. 1.22.  Four runs: the one-slice shapes repeat bit for
                            bit, the shapes whose slices meet in atomics move in the third digit (1.453e-07 .. 1.457e-07 norm-relative)
   data gradient     bf16x3 0.97, 1.41;  f32 1.32, 1.85;  f16x2 1.09, 1.79 (K = 3)
A, B and every f32 route hold bit for bit / at their arithmetic bars on all shapes.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import DGRAD_CASES, WGRAD_SHAPES, assert_noise, dgrad_route
from helpers import assert_impulse as _assert_impulse, full as _full, gen as _gen, ids as _ids, ints as _ints, out_hw as _out_hw, pow2 as _pow2

pytestmark = pytest.mark.gpu

# K of test C per engine ("<kernel family> <engine the launch ran on>")
K_NOISE = {"wgrad bf16x3": 4.0, "wgrad f32": 3.0, "wgrad f16x2": 3.0, "dgrad bf16x3": 3.0, "dgrad f32": 3.0, "dgrad f16x2": 3.0}
_WORST = {}      # engine -> largest ours / noise of this run (norm-relative, max-abs): printed when the module is done

ENGINES = ("bf16x3", "f32", "f16x2")
SPLITS = ("bf16x3", "f16x2")


def _dev():
    return torch.device("cuda:0")


def _assert_noise(key, engine, got, ref32, ref64):
    return assert_noise(_WORST, key, engine, got, ref32, ref64)


def _wgrad_ref(x, dy, scale, R, stride, pad, dtype=torch.float64):
    """dW [K,R,R,C] of y = conv(x, W) * scale from torch's own conv2d backward on the CPU.  x [N,H,W,C], dy [N,Ho,Wo,K]."""
    g = dy.to(dtype).permute(0, 3, 1, 2)
    if scale is not None:
        g = g * scale.to(dtype).view(1, -1, 1, 1)
    w = torch.zeros(dy.shape[3], x.shape[3], R, R, dtype=dtype, requires_grad=True)
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w, stride=stride, padding=pad)
    (y * g).sum().backward()
    return w.grad.permute(0, 2, 3, 1).contiguous()


def _dgrad_ref(dy, w, scale, x_shape, stride, pad, dtype=torch.float64):
    """dx [N,H,W,C] of y = conv(x, w) * scale from torch's own conv2d backward on the CPU.  dy [N,Ho,Wo,K], w [K,C,R,R]."""
    N, H, W, C = x_shape
    g = dy.to(dtype).permute(0, 3, 1, 2)
    if scale is not None:
        g = g * scale.to(dtype).view(1, -1, 1, 1)
    x = torch.zeros(N, C, H, W, dtype=dtype, requires_grad=True)
    y = F.conv2d(x, w.to(dtype), stride=stride, padding=pad)
    (y * g).sum().backward()
    return x.grad.permute(0, 2, 3, 1).contiguous()


def _wgrad(Kn, monkeypatch, engine, x, dy, scale, R, stride, pad):
    dev = _dev()
    if engine == "f16x2":
        Kn.clear_conv_error_word(dev)
    else:
        monkeypatch.setattr(Kn, "WGRAD_ENGINE", engine)
    dw = Kn.conv_wgrad(x.to(dev), dy.to(dev), scale.to(dev) if scale is not None else None, R, R, stride, pad,
                       split="f16x2" if engine == "f16x2" else "bf16x3").cpu()
    if engine == "f16x2":
        assert Kn.conv_error_word(dev) == 0
    return dw


def _dgrad(Kn, monkeypatch, shape, want, split, dy, w, scale):
    """`pack_conv_dgrad` + `conv_dgrad` of forward layer `shape` under DGRAD_SPLIT = split; asserts the route first (the pure
    `conv_route`), and that the launch that ran is that entry point."""
    N, H, W, Cin, Kout, R, stride, pad = shape
    dev = _dev()
    monkeypatch.setattr(Kn, "DGRAD_SPLIT", split)
    if split == "f16x2":
        monkeypatch.setattr(Kn, "_HALO_H2_MIN_TILES", 0)
    assert dgrad_route(Kn, shape, split) == want[split]
    ran = []
    launch = Kn._launch
    monkeypatch.setattr(Kn, "_launch", lambda tag, flops, nbytes, slot, what, call: (ran.append(what), launch(tag, flops, nbytes, slot, what, call))[1])
    Kn.clear_conv_error_word(dev)
    pcd = Kn.pack_conv_dgrad(w.to(dev), scale.to(dev) if scale is not None else None, pad)
    dx = Kn.conv_dgrad(dy.to(dev), pcd, (N, H, W, Cin), stride).cpu()
    monkeypatch.setattr(Kn, "_launch", launch)
    assert ran == [want[split]], ran
    assert Kn.conv_error_word(dev) == 0
    return dx


def _dgrad_engine(want, split):
    e = want[split]
    return "f32" if e.endswith("_f32") else "f16x2" if "f16x2" in e else "bf16x3"


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    for engine in sorted(_WORST):
        print("largest ours / noise, %-13s norm-rel %.2f  max-abs %.2f  (K = %g)" % (engine, _WORST[engine][0], _WORST[engine][1], K_NOISE[engine]))


# ============================================================================================================ 1. kernels.conv_wgrad
@functools.lru_cache(maxsize=None)
def _wgrad_int_case(shape):
    N, H, W, C, Kc, R, stride, pad = shape
    Ho, Wo = _out_hw(H, W, R, stride, pad)
    g = _gen(shape, 1)
    x, dy, scale = _ints(g, (N, H, W, C), 7), _ints(g, (N, Ho, Wo, Kc), 3), _pow2(g, Kc)
    ref = _wgrad_ref(x, dy, scale, R, stride, pad)
    assert float(ref.abs().max()) < 2 ** 22 and torch.equal(ref, (ref * 2).round() / 2)
    return x, dy, scale, ref.float()


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=_ids)
def test_wgrad_integer_exact(shape, engine, monkeypatch):
    from lvc_amd import kernels as Kn

    x, dy, scale, ref = _wgrad_int_case(shape)
    dw = _wgrad(Kn, monkeypatch, engine, x, dy, scale, shape[5], shape[6], shape[7])
    assert dw.shape == ref.shape and torch.equal(dw, ref), (int((dw != ref).sum()), float((dw - ref).abs().max()))


def _impulse_pixels(M, W, chunk=16):
    """Pixels (flat index into the N*Ho*Wo rows) every channel cycles through: first, last, one on each map border, and the edges of the
    16- and 32-pixel chunks -- the last pixel of a partial chunk is M - 1."""
    cand = [0, M - 1, W // 2, W - 1, M - W, M - W + W // 2, (M // W // 2) * W, (M // W // 2) * W + W - 1,
            chunk - 1, chunk, 2 * chunk - 1, 2 * chunk, M - 2, (M - 1) // chunk * chunk, (M - 1) // (2 * chunk) * (2 * chunk)]
    out = []
    for p in cand:
        if 0 <= p < M and p not in out:
            out.append(p)
    return out


def _impulses(rows, channels, W):
    """[rows, channels] of zeros with one 1.0 per channel: the border / chunk-edge pixels first, then spread over the rows."""
    t = torch.zeros(rows, channels)
    px = _impulse_pixels(rows, W)
    for c in range(channels):
        t[px[c] if c < len(px) else (c * 7919 + 13) % rows, c] = 1.0
    return t


@functools.lru_cache(maxsize=None)
def _wgrad_impulse_case(shape, mirror):
    N, H, W, C, Kc, R, stride, pad = shape
    Ho, Wo = _out_hw(H, W, R, stride, pad)
    g = _gen(shape, 2 + mirror)
    if mirror:      # an impulse per input channel in x, full mantissas in dy
        x = _impulses(N * H * W, C, W).view(N, H, W, C)
        dy = _full(g, (N, Ho, Wo, Kc))
    else:           # an impulse per output channel in dy, full mantissas in x
        x = _full(g, (N, H, W, C))
        dy = _impulses(N * Ho * Wo, Kc, Wo).view(N, Ho, Wo, Kc)
    ref = _wgrad_ref(x, dy, None, R, stride, pad)
    src = (dy if mirror else x).double()
    assert bool(torch.isin(ref, torch.cat([src.flatten(), torch.zeros(1, dtype=torch.float64)])).all())      # single terms, exact in fp64
    return x, dy, ref


@pytest.mark.parametrize("mirror", (0, 1), ids=("impulse_dy", "impulse_x"))
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=_ids)
def test_wgrad_impulse_keeps_every_operand_plane(shape, engine, mirror, monkeypatch):
    from lvc_amd import kernels as Kn

    x, dy, ref = _wgrad_impulse_case(shape, mirror)
    dw = _wgrad(Kn, monkeypatch, engine, x, dy, None, shape[5], shape[6], shape[7])
    short = dy.numel() // dy.shape[3] < 16      # fewer pixels than one k-step of the fp16 MFMA: lvc_conv_wgrad_nhwc_f16x2 runs the exact form
    _assert_impulse(dw, ref, "f32" if engine == "f16x2" and short else engine)


@functools.lru_cache(maxsize=None)
def _wgrad_random_case(shape, flavour):
    """flavour: the exponent e of dy = randn * 10^-e, or "wide" -- the log-normal dy of test_conv_wgrad_f16x2_matches_torch."""
    N, H, W, C, Kc, R, stride, pad = shape
    Ho, Wo = _out_hw(H, W, R, stride, pad)
    g = _gen(shape, 5)
    x = torch.randn(N, H, W, C, generator=g)
    dy = torch.randn(N, Ho, Wo, Kc, generator=g)
    dy = dy * 0.05 * torch.exp(2.0 * torch.randn(N, Ho, Wo, Kc, generator=g)) if flavour == "wide" else dy * 10.0 ** -flavour
    scale = torch.rand(Kc, generator=g) + 0.5 if (H + C) % 2 else None
    return x, dy, scale, _wgrad_ref(x, dy, scale, R, stride, pad, torch.float32), _wgrad_ref(x, dy, scale, R, stride, pad)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=_ids)
def test_wgrad_random_within_the_fp32_noise(shape, engine, monkeypatch):
    """C for the three weight-gradient engines.  A layer with fewer than 16 output pixels (less than one k-step of the fp16 MFMA) runs
    the exact fp32 form under split="f16x2" too: two fp16 planes carry 22 bits per operand and the a2 b2 product is left out, up to
    2^-21 per product, which an fp32 sum of a few terms -- exact to a rounding -- cannot hide.  The f16x2 cases with 1, 2, 4, 6 and 15
    pixels therefore measure that route (`test_wgrad_impulse_keeps_every_operand_plane` holds it bit-equal)."""
    from lvc_amd import kernels as Kn

    worst = []
    for flavour in (("wide",) if engine == "f16x2" else (2, 5, 8)):
        x, dy, scale, ref32, ref64 = _wgrad_random_case(shape, flavour)
        dw = _wgrad(Kn, monkeypatch, engine, x, dy, scale, shape[5], shape[6], shape[7])
        worst.append(max(_assert_noise("wgrad %s %s dy %s" % (engine, _ids(shape), flavour), "wgrad " + engine, dw, ref32, ref64)))
    assert max(worst) <= K_NOISE["wgrad " + engine], worst


# ======================================================================= 2. lvc_conv_wgrad_group_bf16x3 + lvc_wgrad_finalize_group
def test_grouped_wgrad_launch_integer_exact():
    """Eight jobs in one launch; jobs 4 and 5 are two uses of ONE parameter (one accumulation buffer takes both jobs' atomics); the
    finalize pass adds into an integer-valued prior gradient (beta = 1) or writes over NaN-filled memory (beta = 0): bit-equal."""
    from lvc_amd import _lib

    dev = _dev()
    picks = [WGRAD_SHAPES[i] for i in (7, 11, 12, 13, 15, 16, 3, 9)]
    assert picks[4][3:6] == picks[5][3:6] and picks[4][:3] != picks[5][:3]
    owner = [0, 1, 2, 3, 4, 4, 5, 6]                  # job -> parameter
    cases = [_wgrad_int_case(s) for s in picks]
    n, nf = len(picks), max(owner) + 1
    dims = {owner[j]: (s[4], s[3], s[5]) for j, s in enumerate(picks)}       # parameter -> (K, C, R)
    sizes = [dims[f][0] * dims[f][1] * dims[f][2] ** 2 for f in range(nf)]
    offs = [0]
    for sz in sizes:
        offs.append(offs[-1] + (sz + 3) // 4 * 4)
    flat = torch.zeros(offs[-1], device=dev)
    g = torch.Generator().manual_seed(17)
    prior = [_ints(g, (dims[f][0], dims[f][1], dims[f][2], dims[f][2]), 100) if f % 2 == 0 else None for f in range(nf)]
    outs = [p.to(dev) if p is not None else torch.full((dims[f][0], dims[f][1], dims[f][2], dims[f][2]), float("nan"), device=dev)
            for f, p in enumerate(prior)]
    PA, PF = ctypes.c_void_p * n, ctypes.c_void_p * nf
    xs, dys, scs, dws, srcs, dsts = PA(), PA(), PA(), PA(), PF(), PF()
    sh, fsh = (ctypes.c_int * (10 * n))(), (ctypes.c_int * (4 * nf))()
    keep = []
    shared_scale = cases[4][2]
    for j, (s, (x, dy, scale, _)) in enumerate(zip(picks, cases)):
        N, H, W, C, Kc, R, stride, pad = s
        scale = shared_scale if owner[j] == 4 else scale if j % 3 else None      # (one parameter: one FrozenBN scale)
        t = (x.to(dev), dy.to(dev), scale.to(dev) if scale is not None else None)
        keep.append(t + (scale,))
        xs[j], dys[j], scs[j] = t[0].data_ptr(), t[1].data_ptr(), (t[2].data_ptr() if scale is not None else None)
        dws[j] = flat.data_ptr() + 4 * offs[owner[j]]
        sh[10 * j: 10 * j + 10] = [N, H, W, C, Kc, R, R, stride, pad, Kc]
    for f in range(nf):
        srcs[f], dsts[f] = flat.data_ptr() + 4 * offs[f], outs[f].data_ptr()
        fsh[4 * f: 4 * f + 4] = [dims[f][0], dims[f][1], dims[f][2] ** 2, 1 if prior[f] is not None else 0]
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.lib().lvc_conv_wgrad_group_bf16x3(ctypes.c_int(n), xs, dys, scs, dws, sh, st), "lvc_conv_wgrad_group_bf16x3")
    _lib.check(_lib.lib().lvc_wgrad_finalize_group(ctypes.c_int(nf), srcs, dsts, fsh, st), "lvc_wgrad_finalize_group")
    for f in range(nf):
        ref = prior[f].double() if prior[f] is not None else torch.zeros(outs[f].shape, dtype=torch.float64)
        for j, s in enumerate(picks):
            if owner[j] == f:
                ref = ref + _wgrad_ref(cases[j][0], cases[j][1], keep[j][3], s[5], s[6], s[7]).permute(0, 3, 1, 2)
        assert float(ref.abs().max()) < 2 ** 22
        got = outs[f].cpu()
        assert torch.equal(got, ref.float()), (f, int((got != ref.float()).sum()))


# ============================================================================================ 3. the pitched dy of the C ABI
@pytest.mark.parametrize("entry", ("lvc_conv_wgrad_nhwc_bf16x3", "lvc_conv_wgrad_nhwc", "lvc_conv_wgrad_nhwc_f16x2"))
@pytest.mark.parametrize("shape", [WGRAD_SHAPES[i] for i in (3, 7, 9, 11, 12, 15)], ids=_ids)
def test_wgrad_pitched_dy_integer_exact(shape, entry):
    """dy as the first K columns of a [M, K + 12] buffer (lddy = K + 12) whose other columns hold a large integer: the contiguous
    launch's result, which is the reference's."""
    from lvc_amd import _lib, kernels as Kn

    dev = _dev()
    N, H, W, C, Kc, R, stride, pad = shape
    x, dy, scale, ref = _wgrad_int_case(shape)
    M = dy.numel() // Kc
    wide = torch.full((M, Kc + 12), 1000.0)
    wide[:, :Kc] = dy.view(M, Kc)
    xd, sd = x.to(dev), scale.to(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    Kn.clear_conv_error_word(dev)
    got = []
    for buf, ld in ((dy.view(M, Kc).to(dev), Kc), (wide.to(dev), Kc + 12)):
        assert buf.is_contiguous() and buf.shape[1] == ld and buf.data_ptr() % 16 == 0
        dw = torch.full((Kc, R, R, C), float("nan"), device=dev)
        args = [_lib.ptr(xd), _lib.ptr(buf), _lib.ptr(sd), _lib.ptr(dw)] + [ctypes.c_int(v) for v in (N, H, W, C, Kc, R, R, stride, pad, ld)]
        if entry.endswith("f16x2"):
            args.append(_lib.ptr(Kn._conv_error_view(dev)))
        _lib.check(getattr(_lib.lib(), entry)(*args, st), entry)
        got.append(dw.cpu())
    assert Kn.conv_error_word(dev) == 0
    assert torch.equal(got[0], ref) and torch.equal(got[1], got[0]), (int((got[1] != ref).sum()), float((got[1] - ref).abs().max()))


# ================================================================================ 4. kernels.pack_conv_dgrad + kernels.conv_dgrad
def _dgrad_params():
    return [pytest.param(shape, want, split, id="%s-%s" % (_ids(shape), split)) for shape, want in DGRAD_CASES for split in SPLITS]


@functools.lru_cache(maxsize=None)
def _dgrad_int_case(shape):
    N, H, W, Cin, Kout, R, stride, pad = shape
    Ho, Wo = _out_hw(H, W, R, stride, pad)
    g = _gen(shape, 11)
    dy, w, scale = _ints(g, (N, Ho, Wo, Kout), 3), _ints(g, (Kout, Cin, R, R), 3), _pow2(g, Kout)
    ref = _dgrad_ref(dy, w, scale, (N, H, W, Cin), stride, pad)
    assert float(ref.abs().max()) < 2 ** 22 and torch.equal(ref, (ref * 2).round() / 2)
    return dy, w, scale, ref.float()


@pytest.mark.parametrize("shape,want,split", _dgrad_params())
def test_dgrad_integer_exact(shape, want, split, monkeypatch):
    from lvc_amd import kernels as Kn

    dy, w, scale, ref = _dgrad_int_case(shape)
    dx = _dgrad(Kn, monkeypatch, shape, want, split, dy, w, scale)
    assert dx.shape == ref.shape and torch.equal(dx, ref), (int((dx != ref).sum()), float((dx - ref).abs().max()))


@pytest.mark.parametrize("shape,want,split", _dgrad_params())
def test_dgrad_impulse_copies_the_flipped_scaled_weights(shape, want, split, monkeypatch):
    """One 1.0 in dy: dx is scale[k] * w[k] (a power of two times a full-mantissa weight: exact) around that pixel, flipped, and
    exactly 0 elsewhere.  First pixel / first channel, last pixel / last channel (inside the zero-padded 32-channel chunk when Kout
    is no multiple of 32), a pixel on the right border / a middle channel."""
    from lvc_amd import kernels as Kn

    N, H, W, Cin, Kout, R, stride, pad = shape
    Ho, Wo = _out_hw(H, W, R, stride, pad)
    g = _gen(shape, 12)
    w, scale = _full(g, (Kout, Cin, R, R), 0.0625), _pow2(g, Kout)
    for n, oy, ox, k in {(0, 0, 0, 0), (N - 1, Ho - 1, Wo - 1, Kout - 1), (0, Ho // 2, Wo - 1, Kout // 2)}:
        dy = torch.zeros(N, Ho, Wo, Kout)
        dy[n, oy, ox, k] = 1.0
        ref = _dgrad_ref(dy, w, scale, (N, H, W, Cin), stride, pad)
        assert int((ref != 0).sum()) > 0 and bool(torch.isin(ref, torch.cat([(w[k].double() * scale[k].double()).flatten(), torch.zeros(1, dtype=torch.float64)])).all())
        dx = _dgrad(Kn, monkeypatch, shape, want, split, dy, w, scale)
        _assert_impulse(dx, ref, _dgrad_engine(want, split))


@functools.lru_cache(maxsize=None)
def _dgrad_random_case(shape, flavour):
    N, H, W, Cin, Kout, R, stride, pad = shape
    Ho, Wo = _out_hw(H, W, R, stride, pad)
    g = _gen(shape, 13)
    w = torch.randn(Kout, Cin, R, R, generator=g) * (2.0 / (Cin * R * R)) ** 0.5
    dy = torch.randn(N, Ho, Wo, Kout, generator=g)
    dy = dy * 0.05 * torch.exp(2.0 * torch.randn(N, Ho, Wo, Kout, generator=g)) if flavour == "wide" else dy * 10.0 ** -flavour
    scale = torch.rand(Kout, generator=g) + 0.5 if (H + Kout) % 2 else None
    xs = (N, H, W, Cin)
    return dy, w, scale, _dgrad_ref(dy, w, scale, xs, stride, pad, torch.float32), _dgrad_ref(dy, w, scale, xs, stride, pad)


@pytest.mark.parametrize("shape,want,split", _dgrad_params())
def test_dgrad_random_within_the_fp32_noise(shape, want, split, monkeypatch):
    from lvc_amd import kernels as Kn

    engine = "dgrad " + _dgrad_engine(want, split)
    worst = []
    for flavour in (("wide",) if split == "f16x2" else (2, 5, 8)):
        dy, w, scale, ref32, ref64 = _dgrad_random_case(shape, flavour)
        dx = _dgrad(Kn, monkeypatch, shape, want, split, dy, w, scale)
        worst.append(max(_assert_noise("dgrad %s %s dy %s -> %s" % (split, _ids(shape), flavour, want[split][4:]), engine, dx, ref32, ref64)))
    assert max(worst) <= K_NOISE[engine], worst


def test_prepack_packs_the_strided_3x3_data_gradient_operand_as_packed_dgrad():
    """`Conv2d.prepack`'s dgrad job of a dense 3x3 / stride 2 layer (its operand does not depend on the stride) against `packed_dgrad()`."""
    from lvc_amd.layers import Conv2d, FrozenBatchNorm2d

    dev = _dev()
    g = torch.Generator().manual_seed(3)
    conv = Conv2d(128, 96, 3, stride=2, padding=1, bias=False, norm=FrozenBatchNorm2d(96))
    with torch.no_grad():
        conv.weight.copy_(torch.randn(96, 128, 3, 3, generator=g) * 0.05)
        conv.norm.weight.copy_(torch.rand(96, generator=g) + 0.5)
        conv.norm.running_var.copy_(torch.rand(96, generator=g) + 0.5)
    conv = conv.to(dev)
    Conv2d.prepack([conv])
    pd = conv._cache_dgrad.value
    conv._cache_dgrad.key = None
    rd = conv.packed_dgrad()
    assert rd is not pd and torch.equal(pd.w, rd.w) and (pd.K, pd.C, pd.R, pd.S, pd.stride, pd.pad, pd.Kg) == (rd.K, rd.C, rd.R, rd.S, rd.stride, rd.pad, rd.Kg)
    assert (rd.K, rd.C, rd.stride, rd.pad) == (128, 96, 1, 1)
    assert pd._w3 is not None and torch.equal(pd._w3.view(torch.int16), rd.split3().view(torch.int16))


# ================================================================================================ 5. csrc/conv_grouped.hip
@pytest.mark.parametrize("H,W", ((5, 7), (6, 8)))
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("G,cg", ((32, 4), (32, 8)))
def test_grouped_conv_gradients_integer_exact(G, cg, stride, H, W):
    from lvc_amd import kernels as Kn

    dev = _dev()
    N, C = 2, G * cg
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = _gen((G, cg, stride, H, W), 21)
    x, dy, w, scale = _ints(g, (N, H, W, C), 7), _ints(g, (N, Ho, Wo, C), 3), _ints(g, (C, cg, 3, 3), 3), _pow2(g, C)
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    y = F.conv2d(x64, w64, None, stride, 1, 1, G) * scale.double().view(1, -1, 1, 1)
    (y * dy.double().permute(0, 3, 1, 2)).sum().backward()
    assert float(max(w64.grad.abs().max(), x64.grad.abs().max())) < 2 ** 22
    dw = Kn.conv_wgrad_grouped(x.to(dev), dy.to(dev), scale.to(dev), G, stride).cpu()
    assert dw.shape == w.shape and torch.equal(dw, w64.grad.float()), int((dw != w64.grad.float()).sum())
    pcd = Kn.pack_conv_dgrad(w.to(dev), scale.to(dev), 1, groups=G)
    assert Kn.conv_route(pcd, N, H, W).entry == "lvc_conv3x3_grouped_nhwc"
    dx = Kn.conv_dgrad(dy.to(dev), pcd, (N, H, W, C), stride).cpu()
    ref = x64.grad.permute(0, 2, 3, 1).float()
    assert dx.shape == ref.shape and torch.equal(dx, ref), int((dx != ref).sum())


# ==================================================================================================== 6. kernels.relu_backward
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n", (1, 3, 4, 5, 1023, 1024, 1025, 262147))
def test_relu_backward_bit_equal(n):
    """out = y > 0 ? dy : 0, bit for bit: +0.0, -0.0, the smallest denormals and negative values in y; the float4 form (n % 4 == 0,
    16-byte aligned) and the scalar form (any other n, or a pointer 4 bytes past a 16-byte boundary)."""
    from lvc_amd import kernels as Kn

    dev = _dev()
    g = torch.Generator().manual_seed(n)
    special = torch.tensor([0.0, -0.0, 2.0 ** -149, -(2.0 ** -149), -1.0, 1.0, 2.0 ** -126, -3.5])
    y = torch.randn(n, generator=g)
    idx = torch.randperm(n, generator=g)[: max(1, n // 2)]
    y[idx] = special[torch.arange(len(idx)) % len(special)]
    dy = torch.randn(n, generator=g)
    dy[::3] = torch.tensor([-0.0, 2.0 ** -149, -7.25])[torch.arange(len(dy[::3])) % 3]
    want = torch.where(y > 0, dy, torch.zeros(()))
    got = Kn.relu_backward(dy.to(dev), y.to(dev)).cpu()
    assert torch.equal(_bits(got), _bits(want))
    if n % 4 == 0:
        # the same elements through views whose pointer is 4 bytes past a 16-byte boundary: the scalar form at n % 4 == 0
        bd, by = torch.zeros(n + 1, device=dev), torch.zeros(n + 1, device=dev)
        bd[1:], by[1:] = dy.to(dev), y.to(dev)
        vd, vy = bd[1:], by[1:]
        assert vd.data_ptr() % 16 == 4 and vy.data_ptr() % 16 == 4 and vd.is_contiguous()
        assert torch.equal(_bits(Kn.relu_backward(vd, vy).cpu()), _bits(want))
        assert torch.equal(_bits(Kn.relu_backward(vd, y.to(dev)).cpu()), _bits(want))
