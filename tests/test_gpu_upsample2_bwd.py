"""lvcst_upsample2_bilinear_bwd_nhwc on the device: the adjoint of the scale heads' bilinear x2 upsample.  Exact on integer gradients
(every weight is a multiple of 1/16), to a measured bar against float64 on random ones, adjoint to the forward kernel, and the
autograd.Function around both forms of the forward."""
import math

import pytest
import torch
import torch.nn.functional as F

import seg_train_ref

pytestmark = pytest.mark.gpu

K_BAR = 3.0          # bars are K_BAR x the deviation of torch's own fp32 CPU evaluation from float64 on the same input
SHAPES = [(1, 1, 1, 4), (2, 3, 5, 128), (1, 7, 2, 64), (1, 1, 6, 8), (1, 2, 1, 4)]
GUARD = 64


def _kernels():
    from lvc_amd import kernels as K

    return K


def _torch_bwd(dy, dtype):
    """torch's own autograd of F.interpolate on the CPU: dy [N,2H,2W,C] -> dx [N,H,W,C]."""
    N, H2, W2, C = dy.shape
    x = torch.zeros(N, C, H2 // 2, W2 // 2, dtype=dtype, requires_grad=True)
    y = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    y.backward(dy.to(dtype).permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1).contiguous()


def _bar(dev32, magnitude):
    """3 x torch's fp32 deviation from float64, with a floor of one fp32 ulp of the quantity's magnitude: where torch's fp32 result
    happens to round to the float64 one, an fp32 result cannot be asked to."""
    return max(K_BAR * dev32, math.ldexp(1.0, math.frexp(magnitude)[1] - 24) if magnitude > 0 else 0.0)


def _run_guarded(dy):
    """The kernel into a buffer with guard elements in front of and behind dx -> (dx on the host, the guards are checked)."""
    K = _kernels()
    N, H2, W2, C = dy.shape
    n = N * (H2 // 2) * (W2 // 2) * C
    buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    out = buf[GUARD: GUARD + n].view(N, H2 // 2, W2 // 2, C)
    got = K.upsample2_bilinear_bwd_nhwc(dy.cuda(), out=out)
    assert got is out
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool(torch.isnan(host[:GUARD]).all()) and bool(torch.isnan(host[GUARD + n:]).all()), "elements outside dx were written"
    return host[GUARD: GUARD + n].view(N, H2 // 2, W2 // 2, C).clone()


@pytest.mark.parametrize("shape", SHAPES)
def test_integer_gradients_are_exact_whatever_the_order(shape):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    dy = torch.randint(-8, 9, (N, 2 * H, 2 * W, C), generator=g).float()
    want = _torch_bwd(dy, torch.float64)
    assert torch.equal(_torch_bwd(dy, torch.float32).double(), want), "torch's own fp32 is exact here"      # the premise, on the CPU
    assert torch.equal(seg_train_ref.upsample2_backward(dy.double()), want)
    got = _run_guarded(dy)
    assert torch.equal(got.double(), want)
    assert torch.equal(_run_guarded(dy), got), "two runs differ"


@pytest.mark.parametrize("shape", SHAPES)
def test_random_gradients_against_float64_and_adjointness(shape):
    K = _kernels()
    N, H, W, C = shape
    g = torch.Generator().manual_seed(100 + sum(shape))
    dy = torch.randn(N, 2 * H, 2 * W, C, generator=g) * 3
    x = torch.randn(N, H, W, C, generator=g) * 3
    want = _torch_bwd(dy, torch.float64)
    dev32 = float((_torch_bwd(dy, torch.float32).double() - want).abs().max())
    got = _run_guarded(dy)
    err = float((got.double() - want).abs().max())
    print("upsample2 bwd %s: |hip - fp64| %.3e, torch fp32 deviation %.3e, ratio %.2f" % (shape, err, dev32, err / dev32 if dev32 else 0.0))
    assert err <= _bar(dev32, float(want.abs().max()))
    assert torch.equal(_run_guarded(dy), got), "two runs differ"
    # <up2(x), dy> = <x, up2^T(dy)> with both kernels, the inner products in float64
    y = K.upsample2_bilinear_nhwc(x.cuda()).cpu()
    lhs, rhs = float((y.double() * dy.double()).sum()), float((x.double() * got.double()).sum())
    y64 = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    y32 = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    # the bar of an inner product: the deviations of both factors, each against the other's magnitude
    bar = _bar(float(((y32.double() - y64).abs() * dy.double().abs()).sum()) + float((x.double().abs()).sum()) * dev32,
               abs(float((y64 * dy.double()).sum())))
    print("  adjointness: <up2 x, dy> %.9e, <x, up2^T dy> %.9e, |difference| %.3e, bar %.3e" % (lhs, rhs, abs(lhs - rhs), bar))
    assert abs(lhs - rhs) <= bar


def test_both_forms_under_autograd():
    from lvc_amd.modeling.meta_arch.semantic_seg import Upsample2, upsample2_bilinear

    g = torch.Generator().manual_seed(7)
    x = (torch.randint(-8, 9, (2, 3, 5, 8), generator=g).float()).cuda().requires_grad_()
    acc = (torch.randint(-8, 9, (2, 6, 10, 8), generator=g).float()).cuda().requires_grad_()
    dy = torch.randint(-8, 9, (2, 6, 10, 8), generator=g).float().cuda()
    want = _torch_bwd(dy.cpu(), torch.float64)
    # y = up2(x)
    y = upsample2_bilinear(x)
    assert torch.equal(y, _kernels().upsample2_bilinear_nhwc(x.detach()))
    y.backward(dy)
    assert torch.equal(x.grad.cpu().double(), want)
    # y = acc + up2(x): d acc is dy, the accumulator itself stays as it was (the module's in-place form is the gradient-free one)
    x.grad = None
    before = acc.detach().clone()
    y = Upsample2().forward_nhwc(x, acc=acc)
    assert y.data_ptr() != acc.data_ptr() and torch.equal(acc.detach(), before)
    assert torch.equal(y, _kernels().upsample2_bilinear_nhwc(x.detach(), acc.detach()))
    y.backward(dy)
    assert torch.equal(acc.grad, dy) and torch.equal(x.grad.cpu().double(), want)
    # only the accumulator asks for a gradient: no gather launch is needed, dy is handed through
    acc2 = acc.detach().clone().requires_grad_()
    Upsample2().forward_nhwc(x.detach(), acc=acc2).backward(dy)
    assert torch.equal(acc2.grad, dy)
    # gradient-free: in place on the accumulator, as the inference head runs it
    with torch.no_grad():
        a = before.clone()
        out = Upsample2().forward_nhwc(x, acc=a)
        assert out.data_ptr() == a.data_ptr()
