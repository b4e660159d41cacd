"""The 2x2 average pool of the ResNet-D trunk on the device (csrc/avgpool.hip, `kernels.avgpool2_into` / `avgpool2_backward` /
`avgpool2_nhwc`).

The arithmetic is pinned -- (((x00 + x01) + x10) + x11) * 0.25f -- so the first oracle is that expression in numpy float32, bit for bit.
The second is F.avg_pool2d on the CPU in float64, at the project's measured bar: 3 x max |torch CPU fp32 - fp64| on the same input.
Every (ours, noise, bar, ratio) row is written to profiles/avgpool_parity.json (LVC_AVGPOOL_PARITY_OUT: another path)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from avgpool_rows import dev as _dev, record as _record, write_parity  # noqa: F401  (the fixture writes this module's rows)

pytestmark = pytest.mark.gpu

# the smallest map; odd sizes (a dropped row AND column); several channel vectors with a ragged last workgroup; more than one workgroup
SHAPES = ((1, 2, 2, 4), (2, 5, 3, 32), (2, 13, 17, 64), (1, 8, 70, 256))
SENTINEL = -12345.678


def _pinned(x):
    """The pinned order in numpy float32 (every operation rounds to float32; no contraction in numpy)."""
    x = x.numpy()
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    v = x[:, : 2 * Ho, : 2 * Wo]
    x00, x01, x10, x11 = v[:, 0::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 0::2], v[:, 1::2, 1::2]
    y = (((x00 + x01) + x10) + x11) * np.float32(0.25)
    assert y.dtype == np.float32 and y.shape == (N, Ho, Wo, C)
    return torch.from_numpy(np.ascontiguousarray(y))


def _pool_cpu(x):
    return F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded input, the pinned-order result, torch's CPU pool in float32 and float64, an upstream gradient and the closed-form and
    autograd input gradients (computed once, never modified)."""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(1000 * H + 10 * W + C)
    x = torch.randn(N, H, W, C, generator=g) * 3.0
    dy = torch.randn(N, H // 2, W // 2, C, generator=g)
    dx = torch.zeros(N, H, W, C)
    q = dy * 0.25
    for a in (0, 1):
        for b in (0, 1):
            dx[:, a: 2 * (H // 2): 2, b: 2 * (W // 2): 2] = q
    xa = x.clone().requires_grad_(True)
    (_pool_cpu(xa) * dy).sum().backward()
    return {"x": x, "pinned": _pinned(x), "y32": _pool_cpu(x), "y64": _pool_cpu(x.double()), "dy": dy, "dx": dx, "dx_autograd": xa.grad}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_is_the_pinned_expression_and_meets_the_fp64_bar(shape):
    from lvc_amd import kernels as K

    c = _case(shape)
    y = K.avgpool2_into(c["x"].to(_dev())).cpu()
    assert y.shape == c["pinned"].shape and y.dtype == torch.float32
    assert torch.equal(y.view(torch.int32), c["pinned"].view(torch.int32))      # bit for bit
    noise = float((c["y32"].double() - c["y64"]).abs().max())
    ours = float((y.double() - c["y64"]).abs().max())
    bar = _record("fwd %s" % "x".join(map(str, shape)), ours, noise)
    assert ours <= bar, (ours, bar)
    again = K.avgpool2_into(c["x"].to(_dev())).cpu()
    assert torch.equal(y.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("offset", (0, 32))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_into_a_channel_slice_leaves_the_other_channels(shape, offset):
    from lvc_amd import kernels as K

    c = _case(shape)
    N, H, W, C = shape
    ldo = C + 32
    buf = torch.full((N, H // 2, W // 2, ldo), SENTINEL, device=_dev())
    out = K.avgpool2_into(c["x"].to(_dev()), buf[..., offset:offset + C])
    assert out.data_ptr() == buf.data_ptr() + 4 * offset
    got = buf.cpu()
    assert torch.equal(got[..., offset:offset + C].contiguous().view(torch.int32), c["pinned"].view(torch.int32))
    rest = torch.cat([got[..., :offset], got[..., offset + C:]], -1)
    assert rest.shape[-1] == 32 and torch.equal(rest.view(torch.int32), torch.full_like(rest, SENTINEL).view(torch.int32))
    noise = float((c["y32"].double() - c["y64"]).abs().max())
    ours = float((got[..., offset:offset + C].double() - c["y64"]).abs().max())
    assert ours <= _record("fwd %s into [%d:%d) of %d" % ("x".join(map(str, shape)), offset, offset + C, ldo), ours, noise)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_is_the_closed_form(shape):
    from lvc_amd import kernels as K

    c = _case(shape)
    N, H, W, C = shape
    dev = _dev()
    dx = K.avgpool2_backward(c["dy"].to(dev), H, W).cpu()
    assert dx.shape == (N, H, W, C)
    assert torch.equal(dx.view(torch.int32), c["dx"].view(torch.int32))      # zeros in a dropped row / column are +0.0 bits too
    assert torch.equal(dx, c["dx_autograd"])                                # 0.25 * dy is exact: autograd of F.avg_pool2d gives the same values
    if H % 2:
        assert float(dx[:, H - 1].abs().max()) == 0.0
    if W % 2:
        assert float(dx[:, :, W - 1].abs().max()) == 0.0
    # dy as a channel slice with leading dimension C + 32
    wide = torch.full((N, H // 2, W // 2, C + 32), SENTINEL, device=dev)
    wide[..., 32:] = c["dy"].to(dev)
    dx2 = K.avgpool2_backward(wide[..., 32:], H, W).cpu()
    assert torch.equal(dx2.view(torch.int32), c["dx"].view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES[1:3], ids=lambda s: "x".join(map(str, s)))
def test_autograd_function(shape):
    from lvc_amd import kernels as K

    c = _case(shape)
    dev = _dev()
    x = c["x"].to(dev).requires_grad_(True)
    y = K.avgpool2_nhwc(x)
    assert y.requires_grad
    (y * c["dy"].to(dev)).sum().backward()
    assert torch.equal(y.detach().cpu().view(torch.int32), c["pinned"].view(torch.int32))
    assert torch.equal(x.grad.cpu().view(torch.int32), c["dx"].view(torch.int32))
    with torch.no_grad():
        assert not K.avgpool2_nhwc(x).requires_grad


def test_the_library_refuses_what_the_kernel_does_not_take():
    """The C entry itself (the Python wrapper raises ValueError first): no launch for a bad shape, pitch or alignment."""
    from lvc_amd import _lib
    from lvc_amd._lib import c_int, ptr

    dev = _dev()
    x, y = torch.zeros(1, 4, 4, 8, device=dev), torch.zeros(1, 2, 2, 8, device=dev)
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream

    def call(xp, yp, N, H, W, C, ld):
        return L.lvc_avgpool2_nhwc(xp, yp, c_int(N), c_int(H), c_int(W), c_int(C), c_int(ld), _lib.c_void_p(st))

    assert call(ptr(x), ptr(y), 1, 4, 4, 8, 8) == 0
    for args in ((1, 1, 4, 8, 8), (1, 4, 1, 8, 8), (1, 4, 4, 6, 8), (1, 4, 4, 8, 10), (1, 4, 4, 8, 4), (0, 4, 4, 8, 8)):
        assert call(ptr(x), ptr(y), *args) == 1, args
        assert b"lvc_avgpool2_nhwc" in L.lvc_last_error()
    assert call(ptr(x), _lib.c_void_p(y.data_ptr() + 4), 1, 4, 4, 8, 8) == 1      # a pointer off the 16-byte grid
    assert L.lvc_avgpool2_bwd_nhwc(ptr(y), ptr(x), c_int(1), c_int(4), c_int(4), c_int(6), c_int(8), _lib.c_void_p(st)) == 1
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0
