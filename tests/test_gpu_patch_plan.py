"""The 3x3 kernels under the two-region patch plan (csrc/patch_plan.h) against the single-shape plan (`lvc_set_patch_plan(0)`): the
switch is set through `_lib.lib()` directly, `kernels.py` is not involved.  `lvc_set_patch_plan(1)`, the default, plans the Winograd
kernel, whose outputs do not depend on the patches; `lvc_set_patch_plan(2)` the direct kernel as well, whose stream-K boundaries move
with the tile count ("the plan" below: 1 for Winograd, 2 for the direct kernel).  Under 1 the direct kernel's outputs are asserted
bit-equal to 0.  Which of the maps below the planner really cuts in two is held without a GPU by tests/test_patch_plan_host.py
(GPU_TEST_PLANS).

Winograd (lvc_conv3x3_nhwc_wino, C = 32, K = 128, N = 2): 20 x 24, 8 x 40, 9 x 17, 16 x 32 (ties: the plan is the old one), 17 x 33,
24 x 48, 24 x 40 (cut after the first 8 rows: 8 x 32-pixel patches there, 16 x 16 below).  Random operands (helpers' fp64 comparison,
K_NOISE x the fp32 CPU evaluation's noise): plan 1 is `torch.equal` to plan 0 -- an output's sum runs over (chunk, filter row) in the
same order whatever the patch -- and within the bar; integer operands: bit-equal to the fp64 reference.  One
lvc_conv3x3_nhwc_wino_pred case (128 hidden channels, 15 outputs), integer operands: exact under both plans.

Direct kernel (C = 32, K = 64 and 128): single maps 40 x 9, 20 x 24 (one region), 20 x 37 (cut after 12 columns), 37 x 20 (after 25 rows),
N = 2, in the one-accumulator form and, the two that are cut, in the two-accumulator form; three levels 20 x 24, 10 x 12, 5 x 6 (every
level its own shape under the plan, the largest map's under plan 0) and 37 x 20, 22 x 34, 10 x 12 (two levels cut) through
lvc_conv3x3_nhwc_f16_levels (shared weights), _f16_layers (a layer per map) and _f16_levels_pred (K = 128).  Integer operands: the
fp64 reference bit for bit under both plans (stream-K hand-offs move with the tile count; every association is exact).  Random
operands: within the same bar under both plans.  Ten repeated launches: bit-identical to the first.
"""
import functools

import pytest
import torch

from helpers import FWD_FUSED, K_NOISE, FwdCase, assert_noise, fwd_case_id, gen, ints
from test_gpu_conv_forward_exact import (_affine, _assert_bit_equal, _assert_exact_ref, _conv, _conv_ref, _dev, _dv, _epilogue, _int_case, _rand_case,
                                         _Recorded, _sparse, _switches)

pytestmark = pytest.mark.gpu

_WORST = {}
_WINO, _HS1, _H2P = "lvc_conv3x3_nhwc_wino", "lvc_conv3x3_nhwc_f16s1", "lvc_conv3x3_nhwc_f16x2_pipe"
WINO_MAPS = ((20, 24), (8, 40), (17, 33), (9, 17), (16, 32), (24, 48), (24, 40))
DIRECT_MAPS = ((40, 9), (20, 24), (20, 37), (37, 20))
LEVEL_SETS = (((20, 24), (10, 12), (5, 6)), ((37, 20), (22, 34), (10, 12)))
hw_id = lambda m: "x".join(map(str, m)) if isinstance(m[0], int) else "_".join("x".join(map(str, h)) for h in m)


@pytest.fixture
def set_plan():
    from lvc_amd import _lib

    L = _lib.lib()
    L.lvc_set_patch_plan.restype = None
    assert L.lvc_patch_plan() in (0, 1, 2)
    yield lambda mode: (L.lvc_set_patch_plan(int(mode)), L.lvc_patch_plan())[1]
    L.lvc_set_patch_plan(1)


def _noise(key, entry, got, ref32, ref64):
    r_rel, r_max = assert_noise(_WORST, key, entry, got, ref32, ref64)
    assert max(r_rel, r_max) <= K_NOISE, (key, r_rel, r_max)


# ============================================================================================================================ Winograd
@pytest.mark.parametrize("hw", WINO_MAPS, ids=hw_id)
def test_wino_plan_is_bit_identical_and_within_the_bar(hw, set_plan, monkeypatch):
    from lvc_amd import kernels as Kn

    case = FwdCase((2, hw[0], hw[1], 32, 128, 3, 1, 1), {"CONV_WINO": True}, _WINO, {"streamk": 0})
    x, w, scale, shift, _, _, conv64, conv32, _ = _rand_case(case.shape)
    got = {}
    for plan in (0, 1):
        set_plan(plan)
        got[plan] = _conv(Kn, monkeypatch, case, x, w, scale, shift)
    assert torch.equal(got[1], got[0]), "plan 1 differs from plan 0 in %d elements" % int((got[1] != got[0]).sum())
    _noise(fwd_case_id(case), case.entry, got[1], _epilogue(conv32, scale, shift, None, 0, False), _epilogue(conv64, scale, shift, None, 0, False))
    xi, wi, sci, shi, _, _, _, convi = _int_case(case.shape)
    ref = _epilogue(convi, sci, shi, None, 0, True)
    _assert_exact_ref(ref)
    _assert_bit_equal(_conv(Kn, monkeypatch, case, xi, wi, sci, shi, relu=True), ref.float(), fwd_case_id(case))


def test_wino_pred_plan_integer_exact(set_plan, monkeypatch):
    from lvc_amd import kernels as Kn

    _switches(monkeypatch, Kn, CONV_WINO=True, WINO_RPN=True)
    dev, N, C, Kh, pred_k = _dev(), 2, 32, 128, 15
    g = gen((N, C, Kh, pred_k), 61)
    x = _sparse(g, (N, 17, 33, C), 3, 0.5)
    wc, (sc, tc) = _sparse(g, (Kh, C, 3, 3), 1, 0.5), _affine(g, Kh, (1.0, 2.0), 3)
    wp, (sp, tp) = ints(g, (pred_k, Kh, 1, 1), 3), _affine(g, pred_k)
    hidden = _epilogue(_conv_ref(x, wc, 1, 1), sc, tc, None, 0, True)
    ref = _epilogue(_conv_ref(hidden, wp, 1, 0), sp, tp, None, 0, False)
    _assert_exact_ref(ref, hidden)
    pc = Kn.pack_conv(wc.to(dev), stride=1, pad=1, affine=_dv((sc, tc)))
    pc.two_acc = True
    pred = Kn.pack_conv(wp.to(dev), affine=_dv((sp, tp)))
    rec = _Recorded(Kn, monkeypatch)
    Kn.clear_conv_error_word(dev)
    for plan in (0, 1):
        set_plan(plan)
        outs = Kn.conv3x3_levels_pred([x.to(dev)], pc, pred, relu=True)
        assert outs is not None
        _assert_bit_equal(outs[0].cpu(), ref.float(), "plan %d" % plan)
    assert rec.ran == [FWD_FUSED["wino_pred"]] * 2, rec.ran
    assert Kn.conv_error_word(dev) == 0


# ======================================================================================================================= direct kernel
def _direct_cases():
    rows = []
    for hw in DIRECT_MAPS:
        for K in (64, 128):
            rows.append(FwdCase((2, hw[0], hw[1], 32, K, 3, 1, 1), {}, _HS1, {}))
            if hw in ((20, 37), (37, 20)):
                rows.append(FwdCase((2, hw[0], hw[1], 32, K, 3, 1, 1), {}, _H2P, {"two_acc": True}))
    return rows


@pytest.mark.parametrize("case", _direct_cases(), ids=fwd_case_id)
def test_direct_single_map_under_both_plans(case, set_plan, monkeypatch):
    from lvc_amd import kernels as Kn

    xi, wi, sci, shi, _, _, _, convi = _int_case(case.shape)
    refi = _epilogue(convi, sci, shi, None, 0, True)
    _assert_exact_ref(refi)
    x, w, scale, shift, _, _, conv64, conv32, _ = _rand_case(case.shape)
    ref64, ref32 = _epilogue(conv64, scale, shift, None, 0, False), _epilogue(conv32, scale, shift, None, 0, False)
    got = {}
    for plan in (0, 1, 2):
        assert set_plan(plan) == plan
        _assert_bit_equal(_conv(Kn, monkeypatch, case, xi, wi, sci, shi, relu=True), refi.float(), "%s plan %d" % (fwd_case_id(case), plan))
        first = got[plan] = _conv(Kn, monkeypatch, case, x, w, scale, shift)
        _noise("%s plan %d" % (fwd_case_id(case), plan), case.entry, first, ref32, ref64)
    assert torch.equal(got[1], got[0]), "the default leaves the direct kernel's decomposition, and every bit, where it was"
    for i in range(10):      # plan 2
        assert torch.equal(_conv(Kn, monkeypatch, case, x, w, scale, shift), first), "launch %d differs from the first" % (i + 2)


@functools.lru_cache(maxsize=None)
def _level_operands(maps, K, integer):
    """Per map x; three layers (w, scale, shift); the layers' fp64 and fp32 convolutions of every map.  Integer operands: exact."""
    N, C = 2, 32
    g = gen((N, C, K, int(integer)) + tuple(v for m in maps for v in m), 62)
    if integer:
        xs = [ints(g, (N, h, w, C), 7) for h, w in maps]
        layers = [(ints(g, (K, C, 3, 3), 3),) + _affine(g, K) for _ in maps]
    else:
        xs = [torch.randn(N, h, w, C, generator=g).relu_() * 3.0 for h, w in maps]
        layers = []
        for _ in maps:
            w = torch.randn(K, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5
            w[:, :, 1, 1] *= torch.logspace(-3, 1, K)[:, None]
            layers.append((w, torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.1))
    return xs, layers


@pytest.mark.parametrize("K", (64, 128))
@pytest.mark.parametrize("shared", (True, False), ids=("levels", "layers"))
@pytest.mark.parametrize("maps", LEVEL_SETS, ids=hw_id)
def test_direct_levels_under_both_plans(maps, shared, K, set_plan, monkeypatch):
    from lvc_amd import kernels as Kn

    _switches(monkeypatch, Kn)
    dev = _dev()
    rec = _Recorded(Kn, monkeypatch)
    Kn.clear_conv_error_word(dev)
    launches = 0
    for integer in (True, False):
        xs, layers = _level_operands(maps, K, integer)
        pcs = [Kn.pack_conv(w.to(dev), stride=1, pad=1, affine=_dv((sc, sh))) for w, sc, sh in (layers[:1] if shared else layers)]
        xd = [x.to(dev) for x in xs]
        run = lambda: [o.cpu() for o in Kn.conv3x3_levels(xd, pcs[0] if shared else pcs, relu=integer)]
        for plan in (0, 2):
            set_plan(plan)
            outs = run()
            launches += 1
            for i, (x, o) in enumerate(zip(xs, outs)):
                w, sc, sh = layers[0 if shared else i]
                ref64 = _epilogue(_conv_ref(x, w, 1, 1), sc, sh, None, 0, integer)
                what = "%s %s K%d map %d plan %d" % (hw_id(maps), "levels" if shared else "layers", K, i, plan)
                if integer:
                    _assert_exact_ref(ref64)
                    _assert_bit_equal(o, ref64.float(), what)
                else:
                    _noise(what, "levels", o, _epilogue(_conv_ref(x, w, 1, 1, torch.float32), sc, sh, None, 0, False), ref64)
        if not integer:      # plan 2
            for i in range(10):
                again = run()
                launches += 1
                assert all(torch.equal(a, o) for a, o in zip(again, outs)), "launch %d differs from the first" % (i + 2)
    assert rec.ran == [FWD_FUSED["levels" if shared else "layers"]] * launches, rec.ran
    assert Kn.conv_error_word(dev) == 0


@pytest.mark.parametrize("maps", LEVEL_SETS, ids=hw_id)
def test_direct_levels_pred_under_both_plans(maps, set_plan, monkeypatch):
    from lvc_amd import kernels as Kn

    _switches(monkeypatch, Kn)
    dev, N, C, Kh, pred_k = _dev(), 2, 32, 128, 15
    rec = _Recorded(Kn, monkeypatch)
    Kn.clear_conv_error_word(dev)
    launches = 0
    for integer in (True, False):
        g = gen((N, C, Kh, pred_k, int(integer)) + tuple(v for m in maps for v in m), 63)
        if integer:
            xs = [_sparse(g, (N, h, w, C), 3, 0.5) for h, w in maps]
            wc, (sc, tc) = _sparse(g, (Kh, C, 3, 3), 1, 0.5), _affine(g, Kh, (1.0, 2.0), 3)
            wp, (sp, tp) = ints(g, (pred_k, Kh, 1, 1), 3), _affine(g, pred_k)
        else:
            xs = [torch.randn(N, h, w, C, generator=g).relu_() * 3.0 for h, w in maps]
            wc, sc, tc = torch.randn(Kh, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5, torch.rand(Kh, generator=g) + 0.5, torch.randn(Kh, generator=g) * 0.1
            wp, sp, tp = torch.randn(pred_k, Kh, 1, 1, generator=g) * (2.0 / Kh) ** 0.5, torch.rand(pred_k, generator=g) + 0.5, torch.randn(pred_k, generator=g) * 0.1
        refs = []
        for x in xs:
            chain = []
            for dt in (torch.float64, torch.float32):
                hidden = _epilogue(_conv_ref(x, wc, 1, 1, dt), sc, tc, None, 0, True)
                chain.append((_epilogue(_conv_ref(hidden, wp, 1, 0, dt), sp, tp, None, 0, False), hidden))
            if integer:
                _assert_exact_ref(chain[0][0], chain[0][1])
            refs.append((chain[0][0], chain[1][0]))
        pc = Kn.pack_conv(wc.to(dev), stride=1, pad=1, affine=_dv((sc, tc)))
        pc.two_acc = True
        pred = Kn.pack_conv(wp.to(dev), affine=_dv((sp, tp)))
        xd = [x.to(dev) for x in xs]

        def run():
            outs = Kn.conv3x3_levels_pred(xd, pc, pred, relu=True)
            assert outs is not None
            return [o.cpu() for o in outs]

        for plan in (0, 2):
            set_plan(plan)
            outs = run()
            launches += 1
            for i, (o, (ref64, ref32)) in enumerate(zip(outs, refs)):
                what = "%s levels_pred map %d plan %d" % (hw_id(maps), i, plan)
                if integer:
                    _assert_bit_equal(o, ref64.float(), what)
                else:
                    _noise(what, "levels_pred", o, ref32, ref64)
        if not integer:      # plan 2
            for i in range(10):
                again = run()
                launches += 1
                assert all(torch.equal(a, o) for a, o in zip(again, outs)), "launch %d differs from the first" % (i + 2)
    assert rec.ran == [FWD_FUSED["levels_pred"]] * launches, rec.ran
    assert Kn.conv_error_word(dev) == 0
