"""tests/roi_align_ref.py, the fp64 reference the ROIAlign kernels are held to, pinned on the CPU: against the reference project's own
outputs (tests/golden/roi_align.npz), against the oracle on every row of the shared case table -- inside the same bound the GPU gets,
bit for bit on the exact rows -- and the table against itself: a row that names an in-kernel sub-route has RoIs with that property."""
import numpy as np
import pytest
import torch

import roi_align_ref as R
from helpers import gold
from oracle import ops as oops

_KEYS = sorted({R.case_key(c): c for c in R.CASES}.items(), key=lambda kv: kv[1].name)      # one row per shared reference
_KEY_IDS = [c.name for _, c in _KEYS]


def _full(case):
    return case._replace(C=R.C_MAX)


# ------------------------------------------------------------------------------------------------ the golden file
def test_forward_matches_the_reference_projects_outputs():
    gd = gold("roi_align")
    keys = [k for k in gd if k.startswith("out_")]
    assert len(keys) == 16
    feat = gd["feat"].permute(0, 2, 3, 1).numpy()
    worst = 0.0
    for key in keys:
        _, s, a, sr = key.split("_")
        out, A, n = R.forward([feat], [float(s[1:])], gd["rois"].numpy(), None, 7, 7, int(sr[2:]), bool(int(a[1:])))
        r = R.ratio(gd[key].permute(0, 2, 3, 1).numpy(), out, A, n)
        worst = max(worst, r)
        assert r <= 1.0, (key, r)
    print("golden forward: worst error / bound %.3f" % worst)


def test_backward_matches_the_reference_projects_outputs():
    gd = gold("roi_align")
    keys = [k for k in gd if k.startswith("bwd_")]
    assert len(keys) == 3
    grad = gd["grad"].permute(0, 2, 3, 1).numpy()
    for key in keys:
        _, s, a, sr = key.split("_")
        (d, A, n), = R.backward(grad, [(2, 50, 84, 8)], [float(s[1:])], gd["rois"].numpy(), None, int(sr[2:]), bool(int(a[1:])))
        r = R.ratio(gd[key].permute(0, 2, 3, 1).numpy(), d, A, n)
        print("golden %s: error / bound %.3f" % (key, r))
        assert r <= 1.0, (key, r)


# ------------------------------------------------------------------------------------------------ the oracle, every row
def _oracle_forward(case):
    feats, rois, levels, _ = R.case_data(case)
    ph, pw = case.pooled
    out = torch.zeros(rois.shape[0], ph, pw, case.C)
    for l, s in enumerate(R.case_scales(case)):
        sel = (levels == l).nonzero().view(-1)
        if len(sel):
            out[sel] = oops.roi_align_forward(feats[l].permute(0, 3, 1, 2), rois[sel], s, ph, pw, case.sr, case.aligned).permute(0, 2, 3, 1)
    return out.numpy()


def _oracle_backward(case):
    feats, rois, levels, grad = R.case_data(case)
    ph, pw = case.pooled
    outs = []
    for l, s in enumerate(R.case_scales(case)):
        sel = (levels == l).nonzero().view(-1)
        Bn, H, W, C = feats[l].shape
        outs.append(oops.roi_align_backward(grad[sel].permute(0, 3, 1, 2), rois[sel], s, ph, pw, Bn, C, H, W, case.sr, case.aligned)
                    .permute(0, 2, 3, 1).numpy())
    return outs


@pytest.mark.parametrize("key_case", _KEYS, ids=_KEY_IDS)
def test_oracle_forward_within_the_bound(key_case):
    case = _full(key_case[1])
    got = _oracle_forward(case)
    out, A, n = R.ref_forward(case)
    if case.kind == "exact":
        assert np.array_equal(got.astype(np.float64), out), case.name
        assert np.abs(out).max() > 0
    else:
        r = R.ratio(got, out, A, n)
        print("%-44s oracle forward error / bound %.3f" % (case.name, r))
        assert r <= 1.0, (case.name, r)


@pytest.mark.parametrize("key_case", _KEYS, ids=_KEY_IDS)
def test_oracle_backward_within_the_bound(key_case):
    case = _full(key_case[1])
    got = _oracle_backward(case)
    for l, (d, A, n) in enumerate(R.ref_backward(case)):
        if case.kind == "exact":
            assert np.array_equal(got[l].astype(np.float64), d), (case.name, l)
        else:
            r = R.ratio(got[l], d, A, n)
            print("%-44s level %d oracle backward error / bound %.3f" % (case.name, l, r))
            assert r <= 1.0, (case.name, l, r)


def test_num_valid_bounds_the_reference_backward():
    case = R.BY_NAME["noise-14x14-C36-sr2-a1"]
    _, rois, levels, grad = R.case_data(case)
    K = rois.shape[0]
    cut = R.ref_backward(case, num_valid=K - 3)
    head = R.backward(grad[:K - 3].numpy(), [(R.B, H, W, case.C) for H, W in R.PYRAMID], R.case_scales(case), rois[:K - 3].numpy(),
                      levels[:K - 3].numpy(), case.sr, case.aligned)
    for (d, A, n), (d2, A2, n2) in zip(cut, head):
        assert np.array_equal(d, d2) and np.array_equal(n, n2)
    assert all(not d.any() for d, _, _ in R.ref_backward(case, num_valid=0))


# ------------------------------------------------------------------------------------------------ the table tells the truth about itself
def test_every_route_and_channel_count_has_its_rows():
    seen = {(c.fwd, c.kind, c.aligned, c.sr) for c in R.CASES} | {(c.bwd, c.kind, c.aligned, c.sr) for c in R.CASES}
    for route in ("scalar", "nhwc4", "wave", "scatter", "rows"):
        for sr in (0, 2):
            assert (route, "exact", True, sr) in seen, (route, sr)
            for aligned in (True, False):
                assert (route, "noise", aligned, sr) in seen, (route, aligned, sr)
    for pooled in R.POOLED:
        cs = {c.C for c in R.CASES if c.pooled == pooled and c.maps == "pyramid"}
        assert cs >= set(R.VEC_C + R.SCALAR_C), pooled
    assert {c.sr for c in R.CASES if c.pooled == (14, 14)} >= {0, 1, 2, 3}
    want = {(7, 7): ("wave", "rows"), (8, 7): ("wave", "scatter"), (1, 7): ("wave", "scatter"), (9, 7): ("nhwc4", "scatter"),
            (14, 14): ("nhwc4", "scatter"), (7, 14): ("nhwc4", "scatter"), (14, 7): ("nhwc4", "scatter"), (2, 3): ("nhwc4", "scatter")}
    for c in R.CASES:
        assert (c.fwd, c.bwd) == (want[c.pooled] if c.C % 4 == 0 else ("scalar", want[c.pooled][1])), c.name


def test_the_limit_rows_straddle_their_limits():
    names = {"tables": 0, "fallback-samples": 0, "fallback-footprint": 0, "wave-sep": 0, "wave-loop": 0}
    for case in R.CASES:
        for idx, claim in case.claims:
            assert R.claim_holds(case, idx, claim), (case.name, idx, claim)
            names[claim] += 1
    assert all(v > 0 for v in names.values()), names
    H, W = R.TALL[0]
    for a in (0, 1):
        for name, samples in (("tall-7x7-tables-by-samples-a%d" % a, 448), ("tall-7x7-fallback-by-samples-a%d" % a, 455)):
            case = R.BY_NAME[name]
            _, rois, _, _ = R.case_data(case)
            for roi in rois:
                assert R.geometry(roi.numpy(), 1.0, H, W, 7, 7, case.sr, case.aligned)["samples"] == (samples, samples)
        for name, extent in (("tall-7x7-tables-footprint-191-a%d" % a, 191), ("tall-7x7-fallback-footprint-192-a%d" % a, 192)):
            case = R.BY_NAME[name]
            _, rois, _, _ = R.case_data(case)
            geo = R.geometry(rois[0].numpy(), 1.0, H, W, 7, 7, 2, case.aligned)
            assert max(geo["extent"]) == geo["extent"][0] == extent and max(geo["samples"]) <= R.RB_MAXS, (name, geo)
    assert (R.RB_MAXS, R.RB_MAXF, R.WAVE_MAX) == (448, 192, 64)


def test_the_pyramid_rows_take_the_separable_forms():
    """Every interior RoI of a pyramid row sits inside the wave forward's registers and the rows backward's tables, and the edge
    list holds what its comments say: clamped and dropped samples on either side, empty grids, boxes outside the map."""
    case = R.BY_NAME["noise-7x7-C36-sr2-a1"]
    _, rois, levels, _ = R.case_data(case)
    kinds = set()
    for roi, lvl in zip(rois, levels):
        H, W = R.PYRAMID[int(lvl)]
        s = R.case_scales(case)[int(lvl)]
        geo = R.geometry(roi.numpy(), s, H, W, 7, 7, 2, True)
        assert R.wave_sep(geo) and R.rows_tables(geo) in ("tables", "none")
        for c0, c1, L in ((roi[2], roi[4], H), (roi[1], roi[3], W)):
            g, v, ok, lo, hi, start, size, bin_ = R._axis(float(c0), float(c1), s, L, 7, 2, True)
            raw = (start + np.arange(7, dtype=np.float32)[:, None] * bin_) + ((np.arange(2, dtype=np.float32) + np.float32(0.5))[None, :] * bin_) / np.float32(2)
            kinds |= {"below" for x in raw.ravel() if x < -1} | {"clamp0" for x in raw.ravel() if -1 <= x < 0}
            kinds |= {"clampL" for x in raw.ravel() if L - 1 < x <= L} | {"beyond" for x in raw.ravel() if x > L}
            kinds |= {"none"} if not ok.any() else set()
            kinds |= {"on-boundary" for x in raw.ravel() if x > 20 and x == np.floor(x)}
    assert kinds == {"below", "clamp0", "clampL", "beyond", "none", "on-boundary"}, kinds
    geo0 = [R.geometry(roi.numpy(), R.case_scales(case)[int(l)], *R.PYRAMID[int(l)], 7, 7, 0, True) for roi, l in zip(rois, levels)]
    assert any(g["gh"] == 0 and g["gw"] == 0 for g in geo0) and any(g["gh"] > 0 and g["gw"] == 0 for g in geo0)


def test_negative_size_is_refused():
    with pytest.raises(ValueError):
        R.forward([np.zeros((1, 8, 8, 4))], [1.0], np.array([[0, 5, 5, 2, 7.0]]), None, 7, 7, 0, True)
