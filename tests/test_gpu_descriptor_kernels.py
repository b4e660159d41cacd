"""The small kernels of the label-verification side, one by one: crops, patch rows, tokens, LayerNorm, GELU, class-token attention, the
online softmax of both attention kernels under large jumps of the row maximum, row normalisation (both entry points) and its backward,
column mean and the scalar maximum.  Each is compared with tests/descriptor_ref.py at the smallest shapes at which it can go wrong.

Three bars and no other: bit-equality (gathers, single roundings); the noise rule of `helpers.assert_noise` (error vs fp64 at most
K_NOISE = 3 x the error of torch's fp32 CPU evaluation of the same inputs, that noise clamped from below by one fp32 rounding); for
attention `2 * err32 + 1e-6` as in test_gpu_vit.py, and -- the matrix-core kernel at large logits only -- the operand-split bound
derived from the inputs (`descriptor_ref.split_logit_bound`).

Worst figures on the MI355X (the module prints them at its end).  Noise rule, ours / noise, bar 3:

    kernel               norm-rel  max-abs
    layernorm              2.77     2.91
    gelu                   0.45     0.51
    rownorm                1.66     1.57
    rownorm_h (y)          1.66     1.57
    rownorm_h (den)        1.00     0.98
    rownorm_h (resid)      2.66     1.33
    rownorm_backward       2.90     2.06
    colmean                1.00     0.79

Attention, error / bar, bar 1:

    mha_cls                               0.49   attention rule
    mha scalar, row 0 (the mha_cls cases) 0.63   attention rule
    mha scalar, row-maximum jumps         0.81   attention rule
    mha matrix-core, row-maximum jumps    0.88   attention rule in five cases of six; N = 130 (b) -- the maximum in the last tile of
                                                 two keys -- needed the operand-split bound: error 2.25e-05, attention rule 2.08e-05,
                                                 derived bound 2.13e-03

Every noise-rule figure is asserted per sub-case (one M, one path); everything else in the module is bit-equality.
"""
import math
from ctypes import c_float, c_int, c_longlong

import pytest
import torch

import descriptor_ref as R
from helpers import K_NOISE, assert_noise, gen, stats

pytestmark = pytest.mark.gpu

WORST = {}      # kernel -> [worst norm-rel ratio, worst max-abs ratio] under the noise rule
ATT = {}        # kernel -> [worst err / (2 err32 + 1e-6), rule that the worst case needed]
F32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst ours / noise per kernel (norm-rel, max-abs):")
    for k in sorted(WORST):
        print("  %-28s %5.2f %5.2f" % (k, WORST[k][0], WORST[k][1]))
    print("worst error / bar per attention kernel:")
    for k in sorted(ATT):
        print("  %-28s %5.2f  (%s)" % (k, ATT[k][0], ATT[k][1]))


def _K():
    from lvc_amd import kernels as K

    return K


def _noise(kernel, key, got, ref32, ref64):
    if not bool(ref64.any()):      # nothing to take a ratio of (one row of +-1 has no fp16 residual): zero is the only right answer
        assert got.shape == ref64.shape and not bool(got.any()), key
        return
    r = assert_noise(WORST, key, kernel, got, ref32, ref64)
    assert max(r) <= K_NOISE, (key, r)


def _attention_rule(kernel, key, got, ref32, ref64, split=None):
    """err <= 2 err32 + 1e-6; split = (dS, max|v|): where that fails, err <= 2 dS max|v| + the same term.  Returns the rule used."""
    err, err32 = stats(got, ref64)[1], stats(ref32, ref64)[1]
    bar = 2 * err32 + 1e-6
    rule = "attention rule"
    if err > bar and split is not None:
        rule, bar = "operand-split bound", 2 * split[0] * split[1] + bar
    print("%-58s max-abs ours %.3e torch fp32 %.3e bar %.3e ratio %5.2f  %s%s" % (
        key, err, err32, bar, err / bar, rule, "" if split is None else "  (split bound alone %.3e)" % (2 * split[0] * split[1])))
    w = ATT.setdefault(kernel, [0.0, rule])
    if err / bar > w[0]:
        w[0], w[1] = err / bar, rule
    assert err <= bar, (key, err, bar)
    return rule


def _pitch(D, vec):
    """The smallest row pitch above D that is (vec) / is not a multiple of 4."""
    ld = D + 1
    while (ld % 4 == 0) != vec:
        ld += 1
    return ld


# ------------------------------------------------------------------------------------------------------------------ crops
def _boxes(H, W):
    return [(5, 7, 5, 7),                                                                        # one pixel
            (0, 0, 9, 6), (W - 8, 0, W - 1, 10), (0, H - 6, 11, H - 1), (W - 7, H - 9, W - 1, H - 1),      # the four corners
            (0, 10, 6, 20), (W - 5, 8, W - 1, 19), (12, 0, 25, 8), (10, H - 4, 30, H - 1),       # each border
            (W - 10, H - 12, W, H),                                                              # one past the last pixel: the slice clamps
            (7, 0, 7, H - 1), (0, 9, W - 1, 9),                                                  # one pixel wide / high, full length
            (0, 0, W - 1, H - 1),                                                                # the whole image
            (3, 4, 12, 8), (3, 4, 12, 9), (4, 3, 8, 12)]                                         # side differences 5, 4, 5: both pad splits, both axes


@pytest.mark.parametrize("op", ["pad", "context"])
@pytest.mark.parametrize("out_size", [224, 7, 1])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", [(37, 53), (64, 40)])
def test_crop_resize_nearest(H, W, C, out_size, op):
    """A gather: bit-equal to slice + pad + F.interpolate(nearest).  16 boxes x 3 x 224 x 224 elements are more than the launch's
    8192 x 256 threads: the grid-stride loop wraps."""
    from lvc_amd.wire import crop_windows

    K = _K()
    img = torch.randn(C, H, W, generator=gen((H, W, C), 1)) + 3.0
    boxes = _boxes(H, W)
    win = torch.tensor(crop_windows(boxes, H, W, op), dtype=torch.int32).reshape(-1, 8)
    got = K.crop_resize_nearest(img.cuda(), win.cuda(), out_size).cpu()
    ref = R.crops(img, boxes, op, out_size)
    assert got.shape == ref.shape == (len(boxes), C, out_size, out_size)
    for k, box in enumerate(boxes):
        assert torch.equal(got[k], ref[k]), (op, box)


def test_crop_resize_nearest_no_boxes():
    K = _K()
    out = K.crop_resize_nearest(torch.randn(3, 8, 8).cuda(), torch.empty(0, 8, dtype=torch.int32).cuda(), 7)
    assert out.shape == (0, 3, 7, 7)


# --------------------------------------------------------------------------------------------------------- patches / tokens
_PATCH_SHAPES = {1: ((16, 24), (8, 40)), 8: ((16, 24), (8, 40)), 16: ((16, 48), (32, 16))}      # 16 divides neither 16x24 nor 8x40: see the refusals


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("ps", [1, 8, 16])
def test_vit_patchify(ps, C, B):
    """Rows against F.unfold, bit for bit; the padded form (zero columns, the left part untouched); the fused normalisation against
    torch's fp32 (img - mean[c]) / std[c] on the CPU, bit for bit as csrc/vit.hip claims."""
    K = _K()
    for H, W in _PATCH_SHAPES[ps]:
        img = torch.randn(B, C, H, W, generator=gen((B, C, H, W, ps), 2))
        kc = C * ps * ps
        ref = R.patchify(img, ps)
        assert torch.equal(K.vit_patchify(img.cuda(), ps).cpu(), ref)
        kpad = (kc + 32) // 32 * 32
        padded = K.vit_patchify(img.cuda(), ps, kpad=kpad).cpu()
        assert padded.shape == (ref.shape[0], kpad) and torch.equal(padded, R.patchify(img, ps, kpad=kpad))
        mean, std = [0.485 - 0.07 * c for c in range(C)], [0.229 + 0.013 * c for c in range(C)]
        assert torch.equal(K.vit_patchify(img.cuda(), ps, mean=mean, std=std).cpu(), R.patchify(img, ps, mean=mean, std=std))
        padded = K.vit_patchify(img.cuda(), ps, kpad=kpad, mean=mean, std=std).cpu()
        assert torch.equal(padded, R.patchify(img, ps, kpad=kpad, mean=mean, std=std))


def test_vit_patchify_grid_wraps():
    """112 x 3 x 224 x 224 elements are more than 65535 x 256 threads."""
    K = _K()
    img = torch.randn(112, 3, 224, 224, generator=gen((112,), 3))
    assert img.numel() > 65535 * 256
    assert torch.equal(K.vit_patchify(img.cuda(), 8).cpu(), R.patchify(img, 8))


def test_vit_patchify_refusals():
    K = _K()
    from lvc_amd._lib import check, lib, ptr

    for H, W, ps in ((16, 24, 16), (8, 40, 16), (12, 16, 8), (16, 12, 8)):
        with pytest.raises(RuntimeError):
            K.vit_patchify(torch.zeros(1, 3, H, W).cuda(), ps)
    with pytest.raises(RuntimeError):
        K.vit_patchify(torch.zeros(1, 9, 8, 8).cuda(), 8, mean=[0.0] * 9, std=[1.0] * 9)
    img, out = torch.zeros(1, 3, 8, 8).cuda(), torch.zeros(1, 192).cuda()
    three = (c_float * 3)(0.5, 0.5, 0.5)
    for mean, std in ((three, None), (None, three)):
        with pytest.raises(RuntimeError):
            check(lib().lvc_vit_patchify_norm(ptr(img), mean, std, ptr(out), c_int(1), c_int(3), c_int(8), c_int(8), c_int(8), K._stream(img)),
                  "lvc_vit_patchify_norm")
    torch.cuda.synchronize()
    assert not bool(out.any())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("P", [1, 49])
@pytest.mark.parametrize("D", [4, 384])
def test_vit_tokens(D, P, B):
    """One fp32 addition per element: bit-equal."""
    K = _K()
    g = gen((D, P, B), 4)
    emb, cls, pos = torch.randn(B * P, D, generator=g), torch.randn(D, generator=g), torch.randn(P + 1, D, generator=g)
    assert torch.equal(K.vit_tokens(emb.cuda(), cls.cuda(), pos.cuda(), B).cpu(), R.tokens(emb, cls, pos, B))


def test_vit_tokens_refuses_width():
    K = _K()
    with pytest.raises(RuntimeError):
        K.vit_tokens(torch.zeros(2, 6).cuda(), torch.zeros(6).cuda(), torch.zeros(3, 6).cuda(), 1)


# ------------------------------------------------------------------------------------------------------------ LayerNorm
def _layernorm_raw(x, w, b, eps, ldy=None):
    """The C entry: w / b may be None (null), the output may have a pitch; the columns past D hold a sentinel."""
    from lvc_amd._lib import check, lib, ptr

    K = _K()
    M, D = x.shape
    ldy = ldy or D
    y = torch.full((M, ldy), -77.0, device=x.device)
    check(lib().lvc_layernorm(ptr(x), c_int(x.stride(0)), ptr(w), ptr(b), ptr(y), c_int(ldy), c_int(M), c_int(D), c_float(eps), K._stream(x)),
          "lvc_layernorm")
    return y


@pytest.mark.parametrize("D", [1, 63, 64, 65, 384, 2047, 2048])
def test_layernorm(D):
    """Every register count of the 2048-wide row, lane tails (d < D), one to two workgroups of four rows, a row pitch (a multiple of 4 and
    not), rows whose mean dwarfs their spread; torch's F.layer_norm in fp32 on the CPU is the noise."""
    import torch.nn.functional as F

    K = _K()
    eps = 1e-6
    for M in (1, 4, 5, 7):
        for kind in ("dense", "pitch", "pitch4", "offset1000"):
            g = gen((D, M, len(kind)), 5)
            w, b = torch.randn(D, generator=g), torch.randn(D, generator=g)
            x = torch.randn(M, D, generator=g) + (1000.0 if kind == "offset1000" else 0.0)
            if kind.startswith("pitch"):
                wide = torch.full((M, _pitch(D, kind == "pitch4")), 5.0)
                wide[:, :D] = x
                xd = wide.cuda()[:, :D]
                assert xd.stride(0) == wide.shape[1]
            else:
                xd = x.cuda()
            got = K.layernorm(xd, w.cuda(), b.cuda(), eps).cpu()
            _noise("layernorm", "layernorm D=%d M=%d %s" % (D, M, kind), got, F.layer_norm(x, (D,), w, b, eps), R.layer_norm(x, w, b, eps))
    # a column slice that starts one element in: neither the pointer nor the pitch is 16-byte aligned
    g = gen((D,), 6)
    wide, w, b = torch.randn(5, D + 3, generator=g), torch.randn(D, generator=g), torch.randn(D, generator=g)
    x = wide[:, 1:1 + D]
    got = K.layernorm(wide.cuda()[:, 1:1 + D], w.cuda(), b.cuda(), eps).cpu()
    _noise("layernorm", "layernorm D=%d M=5 slice 1:" % D, got, F.layer_norm(x.contiguous(), (D,), w, b, eps), R.layer_norm(x, w, b, eps))
    # no weight, no bias, both, and an output pitch, through the C entry
    x = torch.randn(5, D, generator=g)
    for ww, bb in ((None, None), (w, None), (None, b)):
        got = _layernorm_raw(x.cuda(), None if ww is None else ww.cuda(), None if bb is None else bb.cuda(), eps, ldy=D + 3).cpu()
        assert bool((got[:, D:] == -77.0).all())
        _noise("layernorm", "layernorm D=%d M=5 w=%s b=%s ldy=D+3" % (D, ww is not None, bb is not None), got[:, :D].contiguous(),
               F.layer_norm(x, (D,), ww, bb, eps), R.layer_norm(x, ww, bb, eps))


@pytest.mark.parametrize("D", [1, 63, 64, 65, 384, 2047, 2048])
def test_layernorm_constant_row_is_bias(D):
    """-2.75 has three mantissa bits: every partial sum of up to 2048 copies is exact in fp32, so the mean is the value, the centred
    row is 0 and the output is the bias, bit for bit."""
    K = _K()
    g = gen((D,), 7)
    x, w, b = torch.randn(6, D, generator=g), torch.randn(D, generator=g), torch.randn(D, generator=g)
    x[1], x[4] = -2.75, 1536.0
    got = K.layernorm(x.cuda(), w.cuda(), b.cuda(), 1e-6).cpu()
    assert torch.equal(got[1], b) and torch.equal(got[4], b)


def test_layernorm_empty_and_too_wide():
    K = _K()
    w = torch.ones(64).cuda()
    assert K.layernorm(torch.empty(0, 64).cuda(), w, w, 1e-6).shape == (0, 64)
    w = torch.ones(2049).cuda()
    with pytest.raises(RuntimeError):
        K.layernorm(torch.zeros(2, 2049).cuda(), w, w, 1e-6)


# ----------------------------------------------------------------------------------------------------------------- GELU
def _gelu_points():
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 6.0, -6.0, 12.0, -12.0, 5.999999, -5.999999, float("nan"), float("nan")])
    x = torch.cat([torch.linspace(-12, 12, 4801), special, torch.randn(2000, generator=gen((1,), 8)) * 3])
    return x[:x.numel() // 4 * 4].clone()


def test_gelu():
    import torch.nn.functional as F

    K = _K()
    from lvc_amd._lib import check, lib, ptr

    x = _gelu_points()
    got = K.gelu(x.cuda()).cpu()
    nan = torch.isnan(x)
    assert int(nan.sum()) == 2 and bool(torch.isnan(got[nan]).all()) and not bool(torch.isnan(got[~nan]).any())
    _noise("gelu", "gelu on [-12, 12], zeros, subnormals", got[~nan], F.gelu(x[~nan]), R.gelu(x[~nan]))
    # where erf is +-1 to fp32 rounding -- fp64's erf, rounded, says where -- the result is x or a zero, bit for bit
    sat = (x.abs() >= 6) & ~nan
    e = torch.erf(x[sat].double() / math.sqrt(2.0)).float()
    assert bool((e.abs() == 1).all())
    want = x[sat] * 0.5 * (1.0 + e)
    assert torch.equal(got[sat], want)
    assert bool((got[sat][x[sat] >= 6] == x[sat][x[sat] >= 6]).all()) and not bool(got[sat][x[sat] <= -6].any())
    # in place
    xd = x.cuda()
    check(lib().lvc_gelu(ptr(xd), ptr(xd), c_longlong(xd.numel()), K._stream(xd)), "lvc_gelu")
    inplace = xd.cpu()
    assert torch.equal(inplace[~nan], got[~nan]) and bool(torch.isnan(inplace[nan]).all())


def test_gelu_empty_and_refused():
    K = _K()
    assert K.gelu(torch.empty(0).cuda()).numel() == 0
    with pytest.raises(RuntimeError):
        K.gelu(torch.zeros(6).cuda())


def test_gelu_grid_wraps():
    """n / 4 beyond 65535 x 256: every element, the wrapped ones included, equals the small launch's value of the same input."""
    K = _K()
    p = (torch.randn(4096, generator=gen((2,), 8)) * 3).cuda()
    small = K.gelu(p)
    reps = 65535 * 256 * 4 // 4096 + 2
    x = p.repeat(reps)
    assert x.numel() // 4 > 65535 * 256
    y = K.gelu(x)
    y = y.view(reps, 4096)
    for r in range(0, reps, 1024):
        assert bool((y[r:r + 1024] == small).all()), r


# ------------------------------------------------------------------------------------------------------ class-token attention
def _qkv_random(B, N, H, salt):
    return torch.randn(B * N, 3 * H * 64, generator=gen((B, N, H), salt)) * 1.5


@pytest.mark.parametrize("H", [1, 6])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 197, 1024])
def test_mha_cls(N, H):
    K = _K()
    scale = 64 ** -0.5
    for B in (1, 3):
        qkv = _qkv_random(B, N, H, 9)
        ref, ref32 = R.attention_cls(qkv, B, N, H, 64, scale), R.attention_cls(qkv, B, N, H, 64, scale, F32)
        got = K.mha_cls(qkv.cuda(), B, N, H, 64, scale).cpu()
        _attention_rule("mha_cls", "mha_cls B=%d N=%d H=%d" % (B, N, H), got, ref32, ref)
        row0 = K.mha(qkv.cuda(), B, N, H, 64, scale, mfma=False).cpu().view(B, N, H * 64)[:, 0]
        _attention_rule("mha (scalar), row 0", "mha scalar row 0 B=%d N=%d H=%d" % (B, N, H), row0, ref32, ref)


@pytest.mark.parametrize("N", [1, 63, 65, 197, 1024])
def test_mha_cls_equal_keys_give_mean_of_v(N):
    K = _K()
    B, H = 2, 3
    qkv = _qkv_random(B, N, H, 10).view(B, N, 3, H * 64)
    qkv[:, :, 1] = qkv[:, :1, 1].clone()
    qkv = qkv.reshape(B * N, 3 * H * 64)
    v = qkv.view(B, N, 3, H * 64)[:, :, 2]
    got = K.mha_cls(qkv.cuda(), B, N, H, 64, 0.125).cpu()
    _attention_rule("mha_cls", "mha_cls equal keys N=%d" % N, got, v.mean(1), v.double().mean(1))


@pytest.mark.parametrize("N,star", [(1, 0), (63, 62), (65, 64), (197, 0), (197, 100), (1024, 1023)])
def test_mha_cls_dominant_key_gives_its_v_row(N, star):
    """One logit 60 above the largest other: the other probabilities are below e^-60, far under half an ulp of 1 -- the output is that
    key's row of V, bit for bit."""
    K = _K()
    B, H, scale = 2, 3, 0.125
    g = gen((N, star), 11)
    qkv = torch.randn(B, N, 3, H, 64, generator=g)
    qkv[:, :, 2] += torch.copysign(torch.full_like(qkv[:, :, 2], 0.25), qkv[:, :, 2])      # no V entry near 0
    q0 = qkv[:, 0, 0].double()                                                             # [B, H, 64]
    if N > 1:
        others = torch.einsum("bhd,bnhd->bhn", q0, qkv[:, :, 1].double()) * scale
        others[:, :, star] = -1e30
        need = others.amax(-1) + 60.0                                                      # the logit the star key gets
        qkv[:, star, 1] = (q0 * (need / ((q0 * q0).sum(-1) * scale))[..., None]).float()
        logits = torch.einsum("bhd,bnhd->bhn", q0, qkv[:, :, 1].double()) * scale
        top2 = logits.topk(2, dim=-1).values
        assert bool((logits.argmax(-1) == star).all()) and float((top2[..., 0] - top2[..., 1]).min()) > 59.0
    got = K.mha_cls(qkv.view(B * N, -1).cuda(), B, N, H, 64, scale).cpu()
    assert torch.equal(got, qkv[:, star, 2].reshape(B, H * 64))


def test_mha_cls_refuses_more_than_1024_keys():
    K = _K()
    from lvc_amd._lib import check, lib, ptr

    qkv, out = torch.zeros(1025, 192).cuda(), torch.zeros(1, 64).cuda()
    with pytest.raises(RuntimeError):
        K.mha_cls(qkv, 1, 1025, 1, 64, 0.125)
    with pytest.raises(RuntimeError):
        check(lib().lvc_mha_cls(ptr(qkv), ptr(out), c_int(1), c_int(1025), c_int(1), c_float(0.125), K._stream(qkv)), "lvc_mha_cls")


# ------------------------------------------------------------------------------- online softmax under jumps of the row maximum
def _stress_qkv(N, H, where):
    """Logits spread over about +-40 (q ~ 10 N(0,1), k ~ N(0,1), scale 1/8), plus 90 on chosen keys through dimension 63 (q = 8 there,
    k = the offset): (a) keys of the first 64-key tile; (b) keys of the last, partial tile -- everything accumulated before is rescaled
    by about e^-90; (c) one key per tile, 90 more each tile."""
    g = gen((N, H, ord(where)), 12)
    qkv = torch.randn(N, 3, H, 64, generator=g)
    qkv[:, 0] *= 10.0
    qkv[:, 2] *= 1.5
    off = torch.zeros(N)
    if where == "a":
        off[[3, 17, 40]] = 90.0
    elif where == "b":
        off[[N - 1, N - 2]] = 90.0
    else:
        for t in range((N + 63) // 64):
            off[min(N - 1, 64 * t + 21)] = 90.0 * (t + 1)
    qkv[:, 0, :, 63] = 8.0
    qkv[:, 1, :, 63] = off[:, None]
    return qkv.reshape(N, 3 * H * 64), off


@pytest.mark.parametrize("mfma", [True, False])
@pytest.mark.parametrize("where", ["a", "b", "c"])
@pytest.mark.parametrize("N", [130, 197])
def test_attention_row_maximum_jumps(N, where, mfma):
    """The scalar kernel under the attention rule.  The matrix-core kernel under the attention rule or, where that fails, the bound
    its two-way fp16 operand split implies for these inputs (about 2^-21 relative per product term, which fp32 CPU arithmetic does not
    have): 2 dS max|v| on top, dS = 2^-20 max sum_d |q_d k_d| scale.  The printed line says which."""
    K = _K()
    H, scale = 2, 0.125
    qkv, off = _stress_qkv(N, H, where)
    ref, ref32 = R.attention(qkv, 1, N, H, 64, scale), R.attention(qkv, 1, N, H, 64, scale, F32)
    s = torch.einsum("nhd,mhd->hnm", qkv.view(N, 3, H, 64)[:, 0].double(), qkv.view(N, 3, H, 64)[:, 1].double()) * scale
    base = s - off.double()[None, None, :]
    assert 30 < float(base.max()) < 60 and -60 < float(base.min()) < -30
    arg = s.argmax(-1)
    want = {"a": arg < 64, "b": arg >= N - 2, "c": arg == min(N - 1, 64 * ((N - 1) // 64) + 21)}[where]
    assert bool(want.all())                                                   # the row maximum sits where the case says, for every query
    K.clear_conv_error_word(torch.device("cuda:0"))
    got = K.mha(qkv.cuda(), 1, N, H, 64, scale, mfma=mfma).cpu()
    assert K.conv_error_word(torch.device("cuda:0")) == 0                    # operands inside fp16's range
    name = "mha (matrix-core), stress" if mfma else "mha (scalar), stress"
    _attention_rule(name, "%s N=%d (%s)" % (name, N, where), got, ref32, ref, split=R.split_logit_bound(qkv, 1, N, H, 64, scale) if mfma else None)


# ------------------------------------------------------------------------------------------------------ row normalisation
_RN_EPS = {0: 1e-5, 1: 1e-3}


def _rownorm_inputs(M, D, use_mu, path, mode):
    """x on the host as the kernel sees it, the device views, and whether the launchers must take the scalar path.  Five rows carry
    a zero row (1) and, in mode 1, a row with 0 < norm < eps (3)."""
    g = gen((M, D, int(use_mu), len(path), mode), 13)
    x = torch.randn(M, D, generator=g)
    mu = torch.randn(D, generator=g) * 0.3 if use_mu else None
    if M == 5:
        x[1] = mu if use_mu else 0.0
        if mode == 1:
            tiny = torch.randn(D, generator=g) * (1e-5 / math.sqrt(D))
            x[3] = mu + tiny if use_mu else tiny
    if path == "mu+1":
        buf = torch.zeros(D + 1)
        buf[1:] = mu
        mud = buf.cuda()[1:]                      # 4-byte, not 16-byte aligned
    else:
        mud = mu.cuda() if use_mu else None
    if path in ("pitch", "pitch4"):
        ld = _pitch(D, path == "pitch4")
        wide = torch.full((M, ld), 9.0)
        wide[:, :D] = x
        xd = wide.cuda()[:, :D]
        assert xd.stride(0) == ld
    else:
        xd = x.cuda()
    scalar = D % 4 != 0 or path in ("mu+1", "pitch")
    return x, mu, xd, mud, scalar


def _rownorm_cases(D):
    for M in (1, 4, 5):
        for use_mu in (False, True):
            for path in ("dense", "pitch", "pitch4", "mu+1"):
                if (path == "mu+1" and not use_mu) or (path == "pitch4" and D % 4 != 0):
                    continue
                yield M, use_mu, path


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("D", [1, 3, 4, 255, 256, 260, 512, 516, 1024, 1028, 2048, 2052])
def test_rownorm_and_rownorm_h(D, mode):
    """Values of both entry points vs fp64 under the noise rule on the vector and the scalar path (forced by D % 4, by an unaligned mu,
    by a row pitch), every register instance of rownorm_h (D <= 512 / 1024 / 2048) and its wide fallback; then the statements of
    csrc/elementwise.hip: y of the two entry points bit-equal when both take the same path (aligned D <= 2048, and whenever the rows
    are unaligned), yh = fp16(y), y = (x - mu) / den bit for bit, resid = |y - yh|."""
    K = _K()
    eps = _RN_EPS[mode]
    for M, use_mu, path in _rownorm_cases(D):
        x, mu, xd, mud, scalar = _rownorm_inputs(M, D, use_mu, path, mode)
        key = "D=%d M=%d mode=%d mu=%d %s" % (D, M, mode, use_mu, path)
        ref, den64 = R.rownorm(x, mu, eps, mode)
        ref32, den32 = R.rownorm(x, mu, eps, mode, F32)
        y = K.rownorm(xd, mud, eps, mode).cpu()
        _noise("rownorm", "rownorm " + key, y, ref32, ref)
        yh_y, yh, den, resid = [t.cpu() for t in K.rownorm_h(xd, mud, eps, mode, want_resid=True)]
        _noise("rownorm_h", "rownorm_h " + key, yh_y, ref32, ref)
        _noise("rownorm_h den", "rownorm_h den " + key, den, den32, den64)
        same_path = scalar or D <= 2048
        if same_path:
            assert torch.equal(yh_y, y), key
        else:      # wide aligned rows, summed in another order than rownorm's: apart by no more than K_NOISE x the fp32 noise of these inputs
            (d_rel, d_max), (n_rel, n_max) = stats(yh_y, y.double()), stats(ref32, ref)
            n_rel, n_max = max(n_rel, 2.0 ** -25), max(n_max, 2.0 ** -24 * float(ref.abs().max()))
            print("rownorm_h vs rownorm %s: %d of %d elements differ, norm-rel %.3e (noise %.3e) max-abs %.3e (noise %.3e)" % (
                key, int((yh_y != y).sum()), y.numel(), d_rel, n_rel, d_max, n_max))
            assert d_rel <= K_NOISE * n_rel and d_max <= K_NOISE * n_max, key
        assert torch.equal(yh, yh_y.half()), key
        c = x - mu if use_mu else x
        assert torch.equal(c / den[:, None], yh_y), key
        r64 = (yh_y.double() - yh.double()).norm(dim=1)
        _noise("rownorm_h resid", "rownorm_h resid " + key, resid, (yh_y - yh.float()).norm(dim=1), r64)
        if M == 5:
            assert not bool(y[1].any()) and not bool(yh_y[1].any()) and not bool(yh[1].any()) and float(resid[1]) == 0.0
            assert float(den[1]) == float(torch.tensor(eps, dtype=F32))
            if mode == 1:
                assert float(den[3]) == float(torch.tensor(eps, dtype=F32)) and bool(yh_y[3].any()), key      # 0 < norm < eps: the eps branch
        # without the fp32 rows: the other three outputs do not change
        none, yh2, den2, resid2 = K.rownorm_h(xd, mud, eps, mode, want_rows=False, want_resid=True)
        assert none is None and torch.equal(yh2.cpu(), yh) and torch.equal(den2.cpu(), den) and torch.equal(resid2.cpu(), resid), key
        y3, yh3, den3 = K.rownorm_h(xd, mud, eps, mode)
        assert torch.equal(y3.cpu(), yh_y) and torch.equal(yh3.cpu(), yh) and torch.equal(den3.cpu(), den), key


@pytest.mark.parametrize("D", [3, 4, 255, 256, 260, 512, 516, 1024, 1028, 2048, 2052])
def test_rownorm_exact_rows(D):
    """Rows (3k, 0, ..., 0, 4k) and the like: the squares, their sum and its root are exact, so y is ONE rounding -- x / 5k (mode 1,
    eps = 0) or x / fl(5k + eps) (mode 0) -- bit-equal to torch's fp32 division.  The non-zeros sit in the first and the last lane."""
    K = _K()
    x = torch.zeros(5, D)
    for r, (a, b) in enumerate(((3, 4), (5, 12), (8, 15), (21, 20), (6, 8))):
        x[r, 0], x[r, D - 1] = a * (r + 1), -b * (r + 1)
    n = x.double().norm(dim=1).float()
    assert torch.equal(n.double(), x.double().norm(dim=1))
    for mode, eps in ((1, 0.0), (0, 1e-5), (1, 1e-5)):
        den = n + torch.tensor(eps, dtype=F32) if mode == 0 else n.clamp(min=eps)
        want = x / den[:, None]
        for xd in (x.cuda(), torch.cat([x, x[:, :1]], 1).cuda()[:, :D]):      # dense; a pitch of D + 1 (the scalar path for every D)
            assert torch.equal(K.rownorm(xd, None, eps, mode).cpu(), want), (mode, eps)
            y, yh, dn = K.rownorm_h(xd, None, eps, mode)
            assert torch.equal(y.cpu(), want) and torch.equal(dn.cpu(), den) and torch.equal(yh.cpu(), want.half()), (mode, eps)


def test_rownorm_out_pitch_and_one_column():
    """`out` with a row pitch (the columns past D stay), D = 1 exact: x / (|x| + eps) in fp32 steps."""
    K = _K()
    x = torch.tensor([[3.0], [-0.5], [0.0], [7.0], [1e-3]])
    want = x / (x.abs() + torch.tensor(1e-5, dtype=F32))
    assert torch.equal(K.rownorm(x.cuda(), None, 1e-5, 0).cpu(), want)
    for D in (8, 6):
        x = torch.randn(5, D, generator=gen((D,), 14))
        wide = torch.full((5, D + 4), -77.0).cuda()
        out = K.rownorm(x.cuda(), None, 1e-5, 0, out=wide[:, :D])
        assert out.data_ptr() == wide.data_ptr() and bool((wide[:, D:] == -77.0).all())
        assert torch.equal(wide[:, :D].cpu(), K.rownorm(x.cuda(), None, 1e-5, 0).cpu())


# ------------------------------------------------------------------------------------------------------ row-norm backward
@pytest.mark.parametrize("eps", [1e-5, 1e-2])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 1024])
def test_rownorm_backward(D, eps):
    """fp64 autograd of x / (|x| + eps) is the reference, the same autograd in fp32 on the CPU the noise; a zero row gets dy / eps in one
    rounding; accumulate_into adds onto what the tensor holds and returns it."""
    K = _K()
    for M in (1, 4, 5):
        g = gen((D, M), 15)
        x, dy = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
        if M == 5:
            x[2] = 0.0
        got = K.rownorm_backward(x.cuda(), dy.cuda(), eps).cpu()
        live = [r for r in range(M) if not (M == 5 and r == 2)]      # the zero row is 1 / eps times the others: checked exactly, kept out of the noise rule
        _noise("rownorm_backward", "rownorm_backward D=%d M=%d eps=%g" % (D, M, eps), got[live], R.rownorm_backward(x, dy, eps, F32)[live], R.rownorm_backward(x, dy, eps)[live])
        if M == 5:
            assert torch.equal(got[2], dy[2] / torch.tensor(eps, dtype=F32))
        prior = torch.randn(M, D, generator=g)
        acc = prior.cuda()
        back = K.rownorm_backward(x.cuda(), dy.cuda(), eps, accumulate_into=acc)
        assert back is acc and torch.equal(acc.cpu(), prior + got)


# ----------------------------------------------------------------------------------------------------------- column mean
@pytest.mark.parametrize("M", [1, 31, 32, 33, 128, 129, 160, 161, 289])
def test_colmean(M):
    """Rows around the 32 row groups, the five-deep unrolled loop (it runs while m + 128 < M) and its tail; columns around the blocks
    of 32; a row pitch.  Integer values and M a power of two: every sum and the product with 1 / M are exact.  Two runs: the same bits."""
    K = _K()
    for D in (1, 31, 32, 33, 100):
        for ld in (D, D + 3):
            g = gen((M, D, ld), 16)
            wide = torch.randn(M, ld, generator=g)
            x = wide[:, :D]
            xd = wide.cuda()[:, :D]
            got = K.colmean(xd)
            _noise("colmean", "colmean M=%d D=%d ld=%d" % (M, D, ld), got.cpu(), x.mean(0), R.colmean(x))
            assert torch.equal(K.colmean(xd), got)
        if M & (M - 1) == 0:
            xi = torch.randint(-1000, 1001, (M, D), generator=g).float()
            assert torch.equal(K.colmean(xi.cuda()).cpu(), xi.mean(0)) and torch.equal(xi.mean(0).double(), xi.double().mean(0))


# ---------------------------------------------------------------------------------------------------------- scalar maximum
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100003])
def test_max_f32(n):
    K = _K()
    ninf = float("-inf")
    x = torch.randn(n, generator=gen((n,), 17))
    if n == 0:
        assert float(K.max_f32(x.cuda())) == ninf
        return
    x[-1] = 9.5                                                  # the maximum in the last element
    assert float(K.max_f32(x.cuda())) == 9.5
    x[-1] = -9.5
    assert float(K.max_f32(x.cuda())) == float(x.max())
    x[::3] = float("nan")                                        # NaN entries are ignored
    live = x[~torch.isnan(x)]
    assert float(K.max_f32(x.cuda())) == (float(live.max()) if live.numel() else ninf)
    assert float(K.max_f32(torch.full((n,), ninf).cuda())) == ninf


# ------------------------------------------------------------------------------------------------- empty and refused inputs
def test_row_kernels_empty_and_refused():
    K = _K()
    e = torch.empty(0, 8).cuda()
    assert K.rownorm(e).shape == (0, 8) and K.rownorm_backward(e, e).shape == (0, 8)
    y, yh, den, resid = K.rownorm_h(e, want_resid=True)
    assert y.shape == yh.shape == (0, 8) and den.shape == resid.shape == (0,)
    assert K.mha_cls(torch.empty(0, 192).cuda(), 0, 5, 1, 64, 0.125).shape == (0, 64)
    with pytest.raises(RuntimeError):
        K.colmean(e)                                             # the mean of no rows
    with pytest.raises(RuntimeError):
        K.rownorm(torch.empty(3, 0).cuda())
    with pytest.raises(RuntimeError):
        K.rownorm_h(torch.empty(3, 0).cuda())
