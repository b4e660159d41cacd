"""The references of tests/descriptor_ref.py against what they restate, on the CPU: the crop fixture, torch's own modules, and the
crop kernel's fp32 index rule against torch's nearest resize."""
import pytest
import torch
import torch.nn.functional as F

import descriptor_ref as R
from helpers import K_NOISE, assert_noise, gold, stats


def _same_function(mine64, torch64):
    """Both in fp64: apart by far less than one fp32 rounding of the result (the clamp of `helpers.assert_noise`)."""
    rel, mx = stats(mine64, torch64)
    assert rel <= 2.0 ** -25 and mx <= 2.0 ** -24 * float(torch64.abs().max()), (rel, mx)


@pytest.mark.parametrize("op", ["pad", "context"])
def test_crop_reference_reproduces_fixture(op):
    from lvc_amd.utils import synthetic as syn

    g = gold("crops")
    img = syn.synthetic_image(7, 300, 420)
    ref = R.crops(img, g["boxes"].long().tolist(), op, 224)
    assert ref.shape == (len(g["boxes"]), 3, 224, 224)
    assert torch.equal(ref[:, :, ::7, ::7], g["crops_" + op])
    assert torch.allclose(ref.double().sum(dim=(1, 2, 3)), g["sum_" + op], rtol=1e-12, atol=0)


def test_crop_reference_windows_agree_with_wire():
    """The reference derives its slices and pads on its own; `wire.crop_windows` (what the kernel is fed) describes the same squares."""
    from lvc_amd.wire import crop_windows

    img = torch.arange(3 * 37 * 53, dtype=torch.float32).view(3, 37, 53) + 1.0       # no zero pixel: zeros are padding
    boxes = [(5, 7, 5, 7), (0, 0, 9, 6), (43, 25, 53, 37), (7, 0, 7, 36), (0, 9, 52, 9), (3, 4, 12, 8), (3, 4, 12, 9)]
    for op in ("pad", "context"):
        for box, (xa, ya, xb, yb, l, t, sw, sh) in zip(boxes, crop_windows(boxes, 37, 53, op)):
            full = torch.zeros(3, sh, sw)
            full[:, t:t + yb - ya + 1, l:l + xb - xa + 1] = img[:, ya:yb + 1, xa:xb + 1]
            want = F.interpolate(full[None], (7, 7), mode="nearest")
            assert torch.equal(R.crops(img, [box], op, 7), want), (op, box)


def test_index_rule_matches_torch_nearest():
    """min(floor(dst * (float)side / (float)out), side - 1) is torch's CPU nearest index for every side 1..699 and out in {1, 7, 224, 225}:
    bit-equality is the right bar for the crop kernel."""
    for out in (1, 7, 224, 225):
        for side in range(1, 700):
            want = F.interpolate(torch.arange(side, dtype=torch.float32).view(1, 1, 1, side), (1, out), mode="nearest").view(-1).long()
            assert torch.equal(R.nearest_index(side, out), want), (side, out)


def test_patch_and_token_references():
    g = torch.Generator().manual_seed(3)
    img = torch.randn(2, 3, 16, 24, generator=g)
    w = torch.randn(5, 3, 8, 8, generator=g)
    rows = R.patchify(img.double(), 8)
    conv = F.conv2d(img.double(), w.double(), stride=8).flatten(2).transpose(1, 2).reshape(-1, 5)       # the GEMM the rows exist for
    _same_function(rows @ w.double().reshape(5, -1).t(), conv)
    padded = R.patchify(img, 8, kpad=224)
    assert torch.equal(padded[:, :192], R.patchify(img, 8)) and not bool(padded[:, 192:].any())
    emb, cls, pos = torch.randn(2 * 6, 4, generator=g), torch.randn(4, generator=g), torch.randn(7, 4, generator=g)
    t = R.tokens(emb, cls, pos, 2).view(2, 7, 4)
    assert torch.equal(t[:, 0], (cls + pos[0]).expand(2, 4)) and torch.equal(t[1, 3], emb[6 + 2] + pos[3])


def test_layer_norm_reference():
    g = torch.Generator().manual_seed(4)
    worst = {}
    for D in (1, 65, 384):
        x, w, b = torch.randn(5, D, generator=g), torch.randn(D, generator=g), torch.randn(D, generator=g)
        ref = R.layer_norm(x, w, b, 1e-6)
        _same_function(ref, F.layer_norm(x.double(), (D,), w.double(), b.double(), 1e-6))
        r = assert_noise(worst, "layer_norm D=%d: F.layer_norm fp32 against the fp32 reference" % D, "cpu", F.layer_norm(x, (D,), w, b, 1e-6),
                         R.layer_norm(x, w, b, 1e-6, torch.float32), ref)
        assert max(r) <= K_NOISE
    _same_function(R.layer_norm(x, None, None, 1e-6), F.layer_norm(x.double(), (D,), None, None, 1e-6))


def test_gelu_reference():
    x = torch.linspace(-12, 12, 4001)
    ref = R.gelu(x)
    _same_function(ref, F.gelu(x.double()))
    r = assert_noise({}, "gelu: F.gelu fp32 against the fp32 reference", "cpu", F.gelu(x), R.gelu(x, torch.float32), ref)
    assert max(r) <= K_NOISE


def test_attention_reference():
    g = torch.Generator().manual_seed(5)
    B, N, H, Dh = 2, 65, 3, 64
    qkv = torch.randn(B * N, 3 * H * Dh, generator=g) * 1.5
    ref = R.attention(qkv, B, N, H, Dh, Dh ** -0.5)
    q, k, v = [t.transpose(1, 2).double() for t in qkv.view(B, N, 3, H, Dh).unbind(2)]      # [B, H, N, Dh]
    sdpa = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * N, H * Dh)
    _same_function(ref, sdpa)
    q, k, v = [t.transpose(1, 2) for t in qkv.view(B, N, 3, H, Dh).unbind(2)]
    sdpa32 = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * N, H * Dh)
    err, err32 = stats(sdpa32, ref)[1], stats(R.attention(qkv, B, N, H, Dh, Dh ** -0.5, torch.float32), ref)[1]
    print("attention: torch fp32 %.2e, the fp32 reference %.2e" % (err, err32))
    assert err <= 2 * err32 + 1e-6                                                            # the attention rule of the GPU tests
    _same_function(R.attention_cls(qkv, B, N, H, Dh, Dh ** -0.5), ref.view(B, N, -1)[:, 0])
    ds, vmax = R.split_logit_bound(qkv, B, N, H, Dh, Dh ** -0.5)
    assert 0 < ds < 1e-3 and vmax == float(qkv.view(B, N, 3, H * Dh)[:, :, 2].abs().max())


def test_rownorm_and_colmean_references():
    g = torch.Generator().manual_seed(6)
    x, mu, dy = torch.randn(5, 65, generator=g), torch.randn(65, generator=g), torch.randn(5, 65, generator=g)
    x[2] = 0
    y, den = R.rownorm(x, None, 1e-8, 1)
    _same_function(y, F.normalize(x.double(), dim=1, eps=1e-8))                               # max(|x|, eps)
    assert float(den[2]) == 1e-8 and not bool(y[2].any())
    y, den = R.rownorm(x, mu, 1e-5, 0)
    c = x.double() - mu.double()
    _same_function(y, c / (c.norm(dim=1, keepdim=True) + 1e-5))
    gx = R.rownorm_backward(x, dy, 1e-2)
    assert torch.equal(gx[2], dy[2].double() / 1e-2)                                          # the zero row
    n = x.double().norm(dim=1, keepdim=True)
    live = [0, 1, 3, 4]
    closed = dy.double() / (n + 1e-2) - x.double() * (dy.double() * x.double()).sum(1, keepdim=True) / ((n + 1e-2) ** 2 * n)
    _same_function(gx[live], closed[live])
    _same_function(R.colmean(x), x.double().mean(0))
