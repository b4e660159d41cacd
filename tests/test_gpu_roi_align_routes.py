"""Every route of csrc/roi_align.hip, forward and back, against the fp64 reference of tests/roi_align_ref.py on the rows of its case
table: bit for bit where the arithmetic is exact (integer operands, dyadic weights, power-of-two counts), inside the derived bound
(n + c) 2^-24 A element by element elsewhere.  Every row asserts the route it names (lvc_roi_align_route, the dispatch the launches
use) before it launches.  With them: num_valid in both directions, nothing written outside the output, the forward's determinism, the
status word, lvc_assign_levels_rois at the level boundaries and the two autograd nodes of modeling/poolers.py."""
import numpy as np
import pytest
import torch

import roi_align_ref as R

pytestmark = pytest.mark.gpu

WORST = {}      # route -> largest error / bound over the noise rows
SENTINEL = -12345.678


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for route in sorted(WORST):
        print("ROIAlign worst error / bound  %-16s %.3f" % (route, WORST[route]))


def _dev():
    return torch.device("cuda")


def _note(route, r):
    WORST[route] = max(WORST.get(route, 0.0), r)


def _largest(case):
    return max(H * W * case.C for H, W in R.case_shapes(case))


def _assert_routes(case, has_num_valid=False):
    from lvc_amd import kernels as k

    ph, pw = case.pooled
    fwd = k.roi_align_route(False, True, case.C, ph, pw, has_num_valid, _largest(case))
    bwd = k.roi_align_route(True, True, case.C, ph, pw, has_num_valid, _largest(case))
    assert fwd == ("scalar" if has_num_valid else case.fwd) and bwd == case.bwd, (case.name, fwd, bwd)
    assert fwd == R.fwd_route(case.C, case.pooled, has_num_valid)
    return fwd, bwd


def _run_forward(case, num_valid=None, status=None, out=None, rois=None, order=None):
    from lvc_amd import kernels as k

    feats, rois0, levels, _ = R.case_data(case)
    d = _dev()
    rois = rois0 if rois is None else rois
    nv = None if num_valid is None else torch.tensor([num_valid], dtype=torch.int32, device=d)
    return k.roi_align_fpn_nhwc([f.to(d) for f in feats], R.case_scales(case), rois.to(d), levels.to(d) if len(feats) > 1 else None,
                                case.pooled[0], case.pooled[1], case.sr, case.aligned, num_valid=nv, status=status, out=out, order=order)


def _run_backward(case, num_valid=None, status=None, outs=None, rois=None, K=None):
    from lvc_amd import kernels as k

    feats, rois0, levels, grad = R.case_data(case)
    d = _dev()
    rois = rois0 if rois is None else rois
    if K is not None:
        rois, levels, grad = rois[:K], levels[:K], grad[:K]
    nv = None if num_valid is None else torch.tensor([num_valid], dtype=torch.int32, device=d)
    return k.roi_align_fpn_backward_nhwc(grad.to(d), [tuple(f.shape) for f in feats], R.case_scales(case), rois.to(d),
                                         levels.to(d) if len(feats) > 1 else None, case.sr, case.aligned, num_valid=nv, status=status, outs=outs)


def _check(case, route, what, got, ref, A, n):
    got = got.cpu()
    assert tuple(got.shape) == ref.shape
    if case.kind == "exact":
        assert torch.equal(got.double(), torch.from_numpy(np.ascontiguousarray(ref))), (case.name, what)
        return 0.0
    assert bool(torch.isfinite(got).all())
    r = R.ratio(got.numpy(), ref, A, n)
    print("%-44s %-18s %-8s error / bound %.3f" % (case.name, what, route, r))
    _note(what.split()[0] + " " + route, r)
    assert r <= 1.0, (case.name, what, r)
    return r


# ------------------------------------------------------------------------------------------------ every row, both directions
@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_forward_row(case):
    fwd, _ = _assert_routes(case)
    out, A, n = R.ref_forward(case, wave_terms=fwd == "wave")
    _check(case, fwd, "forward", _run_forward(case), out, A, n)


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_backward_row(case):
    _, bwd = _assert_routes(case)
    outs = _run_backward(case)
    for l, (d, A, n) in enumerate(R.ref_backward(case)):
        _check(case, bwd, "backward level %d" % l, outs[l], d, A, n)


# ------------------------------------------------------------------------------------------------ num_valid
_NV_FWD = ("noise-7x7-C36-sr2-a1", "noise-14x14-C260-sr0-a1", "noise-8x7-C258-sr2-a0", "exact-14x14-C258-sr2", "exact-8x7-C4-sr0", "exact-7x7-C260-sr2")


@pytest.mark.parametrize("which", ["0", "1", "K-1", "K"])
@pytest.mark.parametrize("name", _NV_FWD)
def test_forward_num_valid(name, which):
    """Rows below num_valid equal the reference, rows from it on are exactly 0: the scalar kernel, whatever the channel count."""
    case = R.BY_NAME[name]
    fwd, _ = _assert_routes(case, has_num_valid=True)
    assert fwd == "scalar"
    out, A, n = R.ref_forward(case)
    K = out.shape[0]
    nv = {"0": 0, "1": 1, "K-1": K - 1, "K": K}[which]
    got = _run_forward(case, num_valid=nv)
    assert got.shape[0] == K
    assert not bool(got[nv:].any()), "rows from num_valid on must be exactly 0"
    _check(case, "scalar", "forward num_valid", got[:nv], out[:nv], A[:nv], n[:nv])


_NV_BWD = ("noise-7x7-C260-sr0-a1", "noise-7x7-C258-sr2-a0", "exact-7x7-C36-sr2", "noise-14x14-C258-sr2-a0", "noise-14x14-C36-sr0-a1", "exact-14x14-C260-sr0")


@pytest.mark.parametrize("which", ["0", "mid", "K"])
@pytest.mark.parametrize("name", _NV_BWD)
def test_backward_num_valid(name, which):
    """The maps equal the reference run on the first num_valid rows; with 0 every map is exactly 0."""
    case = R.BY_NAME[name]
    _, bwd = _assert_routes(case, has_num_valid=True)
    K = R.case_data(case)[1].shape[0]
    nv = {"0": 0, "mid": K // 2 + 1, "K": K}[which]
    outs = _run_backward(case, num_valid=nv)
    for l, (d, A, n) in enumerate(R.ref_backward(case, num_valid=nv)):
        if nv == 0:
            assert not bool(outs[l].any())
        _check(case, bwd, "backward num_valid level %d" % l, outs[l], d, A, n)


@pytest.mark.parametrize("name", ("noise-7x7-C36-sr2-a1", "noise-14x14-C258-sr2-a0"))
def test_backward_of_no_rois_zeroes_every_map(name):
    case = R.BY_NAME[name]
    feats = R.case_data(case)[0]
    outs = [torch.full(tuple(f.shape), SENTINEL, device=_dev()) for f in feats]
    res = _run_backward(case, outs=outs, K=0)
    assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, outs))
    assert all(not bool(o.any()) for o in outs)


# ------------------------------------------------------------------------------------------------ nothing written outside the output
_GUARD = ("noise-7x7-C260-sr2-a0", "noise-8x7-C260-sr0-a1", "noise-14x14-C260-sr0-a1", "noise-14x14-C258-sr2-a1", "noise-7x7-C258-sr0-a0",
          "noise-2x3-C4-sr0-a1", "noise-1x7-C6-sr2-a0", "exact-9x7-C260-sr2")


@pytest.mark.parametrize("name", _GUARD)
def test_forward_writes_its_rows_and_nothing_else(name):
    case = R.BY_NAME[name]
    fwd, _ = _assert_routes(case)
    K = R.case_data(case)[1].shape[0]
    ph, pw = case.pooled
    buf = torch.full((K + 4, ph, pw, case.C), SENTINEL, device=_dev())
    got = _run_forward(case, out=buf[2:K + 2])
    assert got.data_ptr() == buf[2].data_ptr()
    assert not bool((buf[2:K + 2] == SENTINEL).any()), "an output element was never written"
    assert bool((buf[:2] == SENTINEL).all()) and bool((buf[K + 2:] == SENTINEL).all()), "written outside the output"
    assert torch.equal(got, _run_forward(case))
    out, A, n = R.ref_forward(case, wave_terms=fwd == "wave")
    _check(case, fwd, "forward out=", got, out, A, n)


@pytest.mark.parametrize("name", _GUARD)
def test_backward_writes_its_maps_and_nothing_else(name):
    case = R.BY_NAME[name]
    _, bwd = _assert_routes(case)
    feats = R.case_data(case)[0]
    bufs = [torch.full((R.B + 2,) + tuple(f.shape[1:]), SENTINEL, device=_dev()) for f in feats]
    outs = _run_backward(case, outs=[b[1:R.B + 1] for b in bufs])
    for l, (b, (d, A, n)) in enumerate(zip(bufs, R.ref_backward(case))):
        assert bool((b[0] == SENTINEL).all()) and bool((b[R.B + 1] == SENTINEL).all()), "written outside level %d" % l
        assert not bool((b[1:R.B + 1] == SENTINEL).any())
        _check(case, bwd, "backward outs= level %d" % l, outs[l], d, A, n)


# ------------------------------------------------------------------------------------------------ determinism, status word
@pytest.mark.parametrize("name", ("noise-7x7-C260-sr0-a1", "noise-14x14-C260-sr2-a0", "noise-14x14-C258-sr0-a1", "tall-7x7-wave-loop-sr0-a1"))
def test_forward_is_deterministic(name):
    case = R.BY_NAME[name]
    _assert_routes(case)
    assert torch.equal(_run_forward(case), _run_forward(case))
    if case.C % 4 == 0:      # ... and the scalar kernel on the same row
        assert torch.equal(_run_forward(case, num_valid=5), _run_forward(case, num_valid=5))


@pytest.mark.parametrize("name", ("noise-7x7-C260-sr0-a1", "exact-8x7-C36-sr2", "tall-1x7-wave-loop-sr2-a0"))
def test_a_work_order_changes_no_value(name):
    """The wave forward lets workgroup i pool RoI order[i]: row k of the output is RoI k whatever the permutation."""
    case = R.BY_NAME[name]
    fwd, _ = _assert_routes(case)
    assert fwd == "wave"
    K = R.case_data(case)[1].shape[0]
    order = torch.arange(K - 1, -1, -1, dtype=torch.int32, device=_dev())
    assert torch.equal(_run_forward(case, order=order), _run_forward(case))


@pytest.mark.parametrize("name", ("noise-7x7-C36-sr2-a1", "noise-7x7-C36-sr0-a1", "noise-8x7-C260-sr0-a1", "noise-14x14-C36-sr2-a1", "noise-14x14-C36-sr0-a1",
                                  "noise-7x7-C258-sr2-a1", "noise-14x14-C6-sr0-a1"))
def test_status_word_reports_a_negative_size(name):
    """A RoI with x2 < x1 under aligned=True sets bit 0 on every NHWC route and leaves the output finite; the same call without one
    leaves the word 0.  (No values are compared: the reference refuses such input.)"""
    case = R.BY_NAME[name]
    assert case.aligned
    _assert_routes(case)
    rois = R.case_data(case)[1].clone()
    bad = rois.clone()
    k0 = int((R.case_data(case)[2] == 0).nonzero()[0])
    bad[k0] = torch.tensor([0.0, 60.0, 20.0, 31.0, 50.0])
    for run in (_run_forward, _run_backward):
        for r, want in ((rois, 0), (bad, 1)):
            status = torch.zeros(1, dtype=torch.int32, device=_dev())
            got = run(case, status=status, rois=r)
            assert int(status.item()) == want, (case.name, run.__name__, want)
            for t in (got if isinstance(got, list) else [got]):
                assert bool(torch.isfinite(t).all())


# ------------------------------------------------------------------------------------------------ lvc_assign_levels_rois
def _assign_ref(boxes, min_level, max_level, canonical_box_size, canonical_level):
    """assign_boxes_to_levels + convert_boxes_to_pooler_format, restated in fp32 torch on the CPU."""
    Bn, Rn, _ = boxes.shape
    b = boxes.reshape(-1, 4)
    sizes = torch.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    lv = torch.floor(canonical_level + torch.log2(sizes / canonical_box_size + 1e-8))
    lv = torch.clamp(lv, min=min_level, max=max_level).to(torch.int64) - min_level
    idx = (torch.arange(Bn * Rn) // Rn).float()[:, None]
    return lv.int(), torch.cat([idx, b], 1)


def _well_posed(boxes, canonical_box_size, canonical_level):
    """Whether every row's level is the same for both fp32 neighbours of the true log2: a faithful log2f (the accuracy the device's
    and the host's libraries document, below one ulp) may return either, so only such rows have ONE fp32 answer.  The reference's
    defaults (224, 4) are well posed at 56 .. 896 and one ulp either side; 160 / 3 or 300 / 5 are not (one ulp below 40 or 75 the sum
    lands within half an ulp of an integer), which is why the other settings here are 448 / 5, 200 / 4 and 384 / 5."""
    b = boxes.reshape(-1, 4)
    q = torch.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) / canonical_box_size + 1e-8
    t = torch.log2(q.double())
    near = t.float()
    lo = torch.where(near.double() > t, torch.nextafter(near, torch.full_like(near, -1e30)), near)
    hi = torch.where(near.double() < t, torch.nextafter(near, torch.full_like(near, 1e30)), near)
    return bool((torch.floor(canonical_level + lo) == torch.floor(canonical_level + hi)).all())


@pytest.mark.parametrize("levels", [(2, 5, 224, 4), (2, 6, 448, 5), (3, 4, 224, 4), (2, 5, 200, 4), (3, 6, 384, 5)])
@pytest.mark.parametrize("B_, R_", [(1, 1), (3, 85), (2, 128), (1, 257)])
def test_assign_levels_at_the_boundaries(B_, R_, levels):
    from lvc_amd import kernels as k

    min_level, max_level, size0, lvl0 = levels
    sizes = []
    for m in (0.25, 0.5, 1.0, 2.0, 4.0):      # 56 .. 896 for the defaults: where the level steps, and one ulp either side
        s = torch.tensor(size0 * m, dtype=torch.float32)
        sizes += [float(torch.nextafter(s, torch.tensor(0.0))), float(s), float(torch.nextafter(s, torch.tensor(1e9)))]
    g = torch.Generator().manual_seed(B_ * 1000 + R_)
    rows = []
    for i in range(B_ * R_):
        kind = (i + B_) % 19
        if kind < 15:
            rows.append((0.0, 0.0, sizes[kind], sizes[kind]))      # w = h = s: sqrt(fl(s * s)) == s
        elif kind < 17:
            rows.append((0.0, 0.0, 0.0, 0.0))                      # padding rows: the lowest level
        else:
            x = torch.rand(4, generator=g) * 600
            rows.append((float(x[0]), float(x[1]), float(x[0] + x[2] + 1.0), float(x[1] + x[3] + 1.0)))
    boxes = torch.tensor(rows, dtype=torch.float32).view(B_, R_, 4)
    assert _well_posed(boxes, size0, lvl0)
    want_lv, want_rois = _assign_ref(boxes, min_level, max_level, size0, lvl0)
    lv, rois = k.assign_levels_rois(boxes.to(_dev()), min_level, max_level, size0, lvl0)
    bad = (lv.cpu() != want_lv).nonzero().view(-1)
    assert lv.dtype == torch.int32 and len(bad) == 0, [(boxes.view(-1, 4)[i].tolist(), int(lv[i]), int(want_lv[i])) for i in bad[:8]]
    assert torch.equal(rois.cpu().view(torch.int32), want_rois.view(torch.int32))      # bit-equal rows, the image index column i / R
    pad = (boxes.view(-1, 4) == 0).all(1)
    assert not bool(want_lv[pad].any())
    if B_ * R_ >= 255:
        assert set(want_lv.tolist()) == set(range(max_level - min_level + 1))


# ------------------------------------------------------------------------------------------------ the autograd nodes of the pooler
def _pooler_inputs(sr):
    g = torch.Generator().manual_seed(77 + sr)
    hw, scales, C = ((24, 32), (12, 16)), (0.25, 0.125), 36
    feats = [R.full(g, (R.B, H, W, C)) for H, W in hw]
    per_level = [R._interior_rois(g, 10, H, W, s) + R._edge_rois(H, W, s, True, close=False)[:8] for (H, W), s in zip(hw, scales)]
    rois, levels = R._pack(per_level)
    grad = R.full(g, (rois.shape[0], 14, 14, C))
    return hw, scales, C, feats, rois, levels, grad


@pytest.mark.parametrize("sr", [0, 2])
def test_pool_rois_autograd_carries_num_valid(sr):
    """ROIPooler.pool_rois_nhwc under autograd (_PoolRois): the forward pools every row, the level-map gradients are the reference's
    backward on the first num_valid rows."""
    from lvc_amd.modeling.poolers import ROIPooler

    hw, scales, C, feats, rois, levels, grad = _pooler_inputs(sr)
    K = rois.shape[0]
    d = _dev()
    pooler = ROIPooler((14, 14), scales, sr, "ROIAlignV2")
    fd = [f.to(d).requires_grad_(True) for f in feats]
    nv = torch.tensor([K - 3], dtype=torch.int32, device=d)
    out = pooler.pool_rois_nhwc(fd, rois.to(d), levels.to(d), num_valid=nv)
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith("_PoolRois")
    ref, A, n = R.forward([f.numpy() for f in feats], scales, rois.numpy(), levels.numpy(), 14, 14, sr, True)
    r = R.ratio(out.detach().cpu().numpy(), ref, A, n)
    assert r <= 1.0, r
    out.backward(grad.to(d))
    want = R.backward(grad.numpy(), [tuple(f.shape) for f in feats], scales, rois.numpy(), levels.numpy(), sr, True, num_valid=K - 3)
    every = R.backward(grad.numpy(), [tuple(f.shape) for f in feats], scales, rois.numpy(), levels.numpy(), sr, True)
    assert any(not np.array_equal(w[0], e[0]) for w, e in zip(want, every)), "the last three rows must carry gradient for this to test anything"
    for l, (dref, A, n) in enumerate(want):
        r = R.ratio(fd[l].grad.cpu().numpy(), dref, A, n)
        print("_PoolRois sr %d level %d error / bound %.3f" % (sr, l, r))
        _note("backward scatter", r)
        assert r <= 1.0, (l, r)


@pytest.mark.parametrize("sr", [0, 2])
def test_pool_all_levels_autograd(sr):
    """ROIPooler.pool_nhwc under autograd (_PoolAllLevels): levels from lvc_assign_levels_rois, every row scatters."""
    from lvc_amd.modeling.poolers import ROIPooler

    hw, scales, C, feats, rois, _, grad = _pooler_inputs(sr)
    K = rois.shape[0] // R.B * R.B
    boxes = rois[:K, 1:].clone().view(R.B, K // R.B, 4)
    boxes[1, -2:] = 0.0                          # padding rows
    # the 128 x 96 image holds no box of size 112, the step between the two levels: these hang over it
    boxes[0, :2] = torch.tensor([[-20.0, -10.0, 140.0, 110.0], [-64.0, -48.0, 192.0, 144.0]])
    boxes[1, :1] = torch.tensor([[-30.0, 5.0, 150.0, 92.0]])
    grad = grad[:K]
    d = _dev()
    pooler = ROIPooler((14, 14), scales, sr, "ROIAlignV2")
    lv, rr = _assign_ref(boxes, pooler.min_level, pooler.max_level, pooler.canonical_box_size, pooler.canonical_level)
    assert set(lv.tolist()) == {0, 1}
    fd = [f.to(d).requires_grad_(True) for f in feats]
    out = pooler.pool_nhwc(fd, boxes.to(d))
    assert type(out.grad_fn).__name__.startswith("_PoolAllLevels")
    ref, A, n = R.forward([f.numpy() for f in feats], scales, rr.numpy(), lv.numpy(), 14, 14, sr, True)
    assert R.ratio(out.detach().cpu().numpy(), ref, A, n) <= 1.0
    out.backward(grad.to(d))
    for l, (dref, A, n) in enumerate(R.backward(grad.numpy(), [tuple(f.shape) for f in feats], scales, rr.numpy(), lv.numpy(), sr, True)):
        r = R.ratio(fd[l].grad.cpu().numpy(), dref, A, n)
        print("_PoolAllLevels sr %d level %d error / bound %.3f" % (sr, l, r))
        _note("backward scatter", r)
        assert r <= 1.0, (l, r)
