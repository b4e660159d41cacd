"""Two small kernels without a direct test so far: `lvc_decode_boxes` (csrc/boxes.hip) against apply_deltas + clip in float64, and
`lvc_maxpool2d_nhwc` (csrc/elementwise.hip) against F.max_pool2d (bit-exact: a maximum rounds nothing)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _k():
    from lvc_amd import kernels

    return kernels


# --------------------------------------------------------------------------------------------------------------- 6. decode + clip
# The project's own decode comparisons are not bit-exact (expf): tests/test_gpu_boxes.py allows 1e-4 px for the RPN decode against the
# fp32 oracle and 1e-3 px for fast_rcnn_inference, the path with this kernel's weights and clamp, at coordinates up to ~1333 px.
# This test keeps every decoded coordinate below ~1500 px (half an ulp there: 6e-5; a coordinate is four rounded operations from the
# inputs) and takes the 1e-3 px of fast_rcnn_inference against float64.
DECODE_TOL = 1e-3
_SIZES = [(200, 300), (480, 640), (97, 131)]


def _decode_reference(deltas, boxes, weights, sizes, R):
    """Box2BoxTransform.apply_deltas (box_regression.py:73-110) + Boxes.clip in float64 -> (unclipped, clipped) [M,4]."""
    k = _k()
    b, d = boxes.double().view(-1, 4), deltas.double()
    wx, wy, ww, wh = weights
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    cx, cy = b[:, 0] + 0.5 * w, b[:, 1] + 0.5 * h
    dx, dy = d[:, 0] / wx, d[:, 1] / wy
    dw, dh = (d[:, 2] / ww).clamp(max=k.SCALE_CLAMP), (d[:, 3] / wh).clamp(max=k.SCALE_CLAMP)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    raw = torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], 1)
    if sizes is None:
        return raw, raw, None
    hw = torch.tensor(sizes, dtype=torch.float64).repeat_interleave(R, 0)            # row i belongs to image i // R
    hi = torch.stack([hw[:, 1], hw[:, 0], hw[:, 1], hw[:, 0]], 1)
    return raw, torch.min(raw.clamp(min=0), hi), hi


def _decode_inputs(R, ld, weights, B=3):
    k = _k()
    M = B * R
    g = torch.Generator().manual_seed(100 * R + ld)
    xy = torch.rand(M, 2, generator=g) * 600 - 40
    boxes = torch.cat([xy, xy + 4 + torch.rand(M, 2, generator=g) * 200], 1)
    unit = torch.cat([torch.randn(M, 2, generator=g) * 0.4, torch.randn(M, 2, generator=g) * 0.25], 1)
    i = torch.arange(M)
    # dw / dh just below, just above and far above the clamp, on narrow boxes (the clamp multiplies the size by 62.5)
    for res, f in ((0, 1.0 - 1e-3), (1, 1.0 + 1e-3), (2, 3.0)):
        rows = i % 7 == res
        boxes[rows, 2:] = boxes[rows, :2] + 2 + torch.rand(int(rows.sum()), 2, generator=g) * 10
        unit[rows, 2] = k.SCALE_CLAMP * f
        unit[rows, 3] = k.SCALE_CLAMP * (2.0 - f if f < 2 else f)
    zero = i % 7 == 3
    boxes[zero, 2:] = boxes[zero, :2]                    # zero-size boxes
    if R > 5:
        boxes[5] = torch.tensor([-30.0, -20.0, 50.0, 60.0])          # past the left and the top edge
        unit[5] = 0.0
    # the last row of image 0 and the first of image 1: the same box, past the right and bottom edge of both images
    boxes[R - 1] = boxes[R] = torch.tensor([10.0, 10.0, 1000.0, 1000.0])
    unit[R - 1] = unit[R] = 0.0
    wide = torch.full((M, ld), 1e30)                     # deltas are the first four columns of a wider row
    wide[:, :4] = unit * torch.tensor(weights)
    return wide, boxes


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("weights", [(10.0, 10.0, 5.0, 5.0), (30.0, 30.0, 15.0, 15.0)], ids=["w10", "w30"])
@pytest.mark.parametrize("ld", [4, 8, 324])
@pytest.mark.parametrize("R", [1, 100])
def test_decode_boxes_equals_fp64_apply_deltas_and_clip(R, ld, weights, clip):
    k = _k()
    B = 3
    M = B * R
    wide, boxes = _decode_inputs(R, ld, weights)
    raw, want, hi = _decode_reference(wide[:, :4], boxes, weights, _SIZES if clip else None, R)
    sz = torch.tensor(_SIZES, dtype=torch.int32, device=DEV) if clip else None
    junk = torch.full((B, R, 4), float("nan"), device=DEV)
    del junk
    out = k.decode_boxes(wide.to(DEV)[:, :4], boxes.view(B, R, 4).to(DEV), weights, sz).cpu().view(M, 4)
    err = float((out.double() - want).abs().max())
    print("decode_boxes R=%d ld=%d w=%g clip=%d: max |err| %.2e px (bound %.0e), max |coordinate| %.0f"
          % (R, ld, weights[0], clip, err, DECODE_TOL, float(want.abs().max())))
    assert float(want.abs().max()) < 1600.0, "the tolerance above is argued for coordinates of this size"
    assert err <= DECODE_TOL
    if clip:
        over, under = raw > hi + DECODE_TOL, raw < -DECODE_TOL
        if R > 5:
            assert bool(over[:, 2].any()) and bool(over[:, 3].any()) and bool(under[:, 0].any()) and bool(under[:, 1].any())
        assert torch.equal(out[over].double(), hi[over]), "a clipped coordinate equals the bound exactly"
        assert not bool(out[under].ne(0).any())
        assert out[R - 1].tolist() == [10.0, 10.0, 300.0, 200.0] and out[R].tolist() == [10.0, 10.0, 640.0, 480.0]
    else:
        assert out[R - 1].tolist() == [10.0, 10.0, 1000.0, 1000.0] and out[R].tolist() == [10.0, 10.0, 1000.0, 1000.0]


# --------------------------------------------------------------------------------------------------------------- 7. max pool
def _pool_reference(x, k, s, p):
    return F.max_pool2d(x.permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1).contiguous()


_WINDOWS = [(3, 2, 1), (1, 2, 0), (2, 2, 0), (3, 1, 1)]


# a 1x1 map: under (3,2,1) every tap but one is padding, under (1,2,0) it is a copy ((2,2,0) has no output there)
_POOL_CASES = [(w, (1, 1)) for w in ((3, 2, 1), (1, 2, 0))] + [(w, hw) for hw in ((7, 9), (8, 8), (33, 50)) for w in _WINDOWS]


@pytest.mark.parametrize("win,hw", _POOL_CASES, ids=["k%ds%dp%d-%dx%d" % (w + hw) for w, hw in _POOL_CASES])
def test_maxpool2d_nhwc_equals_torch(win, hw):
    k = _k()
    H, W = hw
    g = torch.Generator().manual_seed(H * 100 + W)
    for C in (4, 64, 100):
        for N in (1, 3):
            x = torch.randn(N, H, W, C, generator=g)
            for inp in (x, -1.0 - x.abs()):     # all negative: a border window must not see its padding as 0
                want = _pool_reference(inp, *win)
                junk = torch.full(want.shape, float("nan"), device=DEV)
                del junk
                got = k.maxpool2d_nhwc(inp.to(DEV), *win).cpu()
                assert got.shape == want.shape and torch.equal(got, want), (win, hw, C, N)


def test_maxpool2d_nhwc_windows_of_minus_infinity():
    k = _k()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 7, 9, 8, generator=g)
    x[0, :3, :3, :] = float("-inf")             # the whole first window (and the padded corner window) of image 0
    x[1, 4, 5, 3] = float("-inf")
    for win in _WINDOWS:
        got = k.maxpool2d_nhwc(x.to(DEV), *win).cpu()
        assert torch.equal(got, _pool_reference(x, *win)), win
    assert bool(torch.isinf(k.maxpool2d_nhwc(x.to(DEV), 3, 2, 1)[0, 0, 0]).all())


def test_maxpool2d_nhwc_rejects_channels_not_a_multiple_of_four():
    k = _k()
    from lvc_amd._lib import LvcNativeError

    with pytest.raises(LvcNativeError, match="multiple of 4"):
        k.maxpool2d_nhwc(torch.zeros(1, 8, 8, 6, device=DEV), 3, 2, 1)
    torch.cuda.synchronize()


def test_maxpool2d_nhwc_more_outputs_than_the_grid_has_threads():
    """2 x 256 x 256 x 64 under (3,1,1): 2 097 152 float4 outputs against a grid capped at 256*16 workgroups of 256 threads, so each
    thread walks its grid-stride loop twice."""
    k = _k()
    g = torch.Generator().manual_seed(10)
    x = torch.randn(2, 256, 256, 64, generator=g)
    assert x.numel() // 4 > 256 * 16 * 256
    got = k.maxpool2d_nhwc(x.to(DEV), 3, 1, 1).cpu()
    assert torch.equal(got, _pool_reference(x, 3, 1, 1))
