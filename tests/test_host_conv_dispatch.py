"""The host dispatch of the conv/GEMM layers (lvc_amd/kernels.py: conv_route, the launch bracket, the grouped entry points) without a
GPU: scripts/conv_dispatch_trace.py replaces the native library by a recorder and walks a grid of layers, forms and switches;
tests/golden/conv_dispatch_trace.json is that script's output on the commit before the dispatch was given one routing function."""
import importlib.util
import itertools
import json
import os
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_dispatch_trace.json")

ENTRY_POINTS = [
    "lvc_conv2d_nhwc_f32", "lvc_conv2d_nhwc_bf16x3", "lvc_conv2d_nhwc_f16x2", "lvc_conv2d_nhwc_f16x2_dma",
    "lvc_conv3x3_nhwc_bf16x3", "lvc_conv3x3_nhwc_f16x2", "lvc_conv3x3_nhwc_f16x2_pipe", "lvc_conv3x3_nhwc_f16s1",
    "lvc_conv3x3_nhwc_f16s1_presplit", "lvc_conv3x3_nhwc_wino", "lvc_conv3x3_nhwc_wino_pred",
    "lvc_conv3x3_nhwc_f16_levels", "lvc_conv3x3_nhwc_f16_layers", "lvc_conv3x3_nhwc_f16_levels_pred",
    "lvc_conv1x1_nhwc_f16x2_pipe", "lvc_conv1x1_nhwc_f16s1", "lvc_conv1x1_nhwc_f16s1_w2", "lvc_conv1x1_nhwc_f16s1_presplit",
    "lvc_conv1x1_chain_nhwc_f16s1", "lvc_bottleneck_nhwc_f16s1", "lvc_gelu",
]


@pytest.fixture(scope="module")
def T():
    spec = importlib.util.spec_from_file_location("conv_dispatch_trace", os.path.join(ROOT, "scripts", "conv_dispatch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


CASE_AXES = ("tier", "two_acc", "split", "residual", "relu_act")


def _signatures(T, tr, cell):
    return [tr["signatures"][T.ALPHABET.index(r) if isinstance(r, str) else r] for r in tr["cells"][cell]["routes"]]


def test_dispatch_trace_equals_the_recorded_one(T, golden):
    """What ran (signatures) is compared case by case, the complete records (integer arguments, NULL flags, flops, bytes) through the
    cells' digests; `scripts/conv_dispatch_trace.py --full` on both commits shows the records of a cell whose digest differs."""
    got = json.loads(T.dumps(T.compact(T.trace())))
    assert got["axes"] == golden["axes"] and got["layers"] == golden["layers"] and got["settings"] == golden["settings"]
    for setting in golden["settings"]:
        for layer in golden["layers"]:
            a, b = got["conv2d"][setting][layer], golden["conv2d"][setting][layer]
            for combo, x, y in zip(itertools.product(*(golden["axes"][k] for k in CASE_AXES)), _signatures(T, got, a), _signatures(T, golden, b)):
                assert x == y, "conv2d_nhwc, {}, {}, {} = {}".format(setting, layer, CASE_AXES, combo)
            assert got["cells"][a]["sha256"] == golden["cells"][b]["sha256"], "arguments or timer records of conv2d_nhwc, {}, {}".format(setting, layer)
        a, b = got["extras"][setting], golden["extras"][setting]
        for label, x, y in zip(golden["axes"]["extras"], _signatures(T, got, a), _signatures(T, golden, b)):
            assert x == y, "{}, {}".format(setting, label)
        assert got["cells"][a]["sha256"] == golden["cells"][b]["sha256"], "arguments or timer records of the extras, {}".format(setting)
        assert got["presplit_pair_ok"][setting] == golden["presplit_pair_ok"][setting], setting
    with open(FIXTURE) as f:
        assert T.dumps(got) == f.read()      # the script's output is byte for byte the committed file


def test_every_entry_point_is_in_the_recorded_trace(golden):
    reached = {launch[0] for s in golden["signatures"] for launch in s["launches"]}
    assert sorted(set(ENTRY_POINTS) - reached) == []
    assert all(s["end_slot"] == 0 for s in golden["signatures"])


def test_conv_route_alone_gives_the_recorded_routes(T, golden, monkeypatch):
    """conv_route on plain numbers -- no tensor, no stand-in library, no stub -- for every conv2d_nhwc row of the grid."""
    from lvc_amd import _lib
    from lvc_amd import kernels as K

    def no_library():
        raise AssertionError("conv_route touched the native library")

    monkeypatch.setattr(_lib, "lib", no_library)
    axes = [golden["axes"][k] for k in CASE_AXES]
    rows = 0
    for setting, change in T.SETTINGS:
        for k, v in T.DEFAULTS.items():
            monkeypatch.setattr(K, k, change.get(k, v))
        for name, (R, S, C, Kc, stride, pad, mode, (N, H, W)) in T.LAYERS.items():
            Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
            for (tier, two_acc, split, res, _), want in zip(itertools.product(*axes), _signatures(T, golden, golden["conv2d"][setting][name])):
                pc = types.SimpleNamespace(R=R, S=S, C=C, K=Kc, stride=stride, pad=pad, mode=mode, two_acc=two_acc, state={"tier": tier})
                res_numel = 0 if res == 0 else N * Ho * Wo * Kc if res == 1 else N * ((Ho + 1) // 2) * ((Wo + 1) // 2) * Kc
                route = K.conv_route(pc, N, H, W, ldr=Kc if res else None, res_numel=res_numel, split=split)
                entry, slot = want["launches"][0]
                assert isinstance(route, tuple) and route.entry == entry and route.engine == want["timer"][0], (setting, name, route)
                assert route.slotted == (slot != 0) and want["last_one"] == [route.one if route.slotted else "unset"], (setting, name, route)
                rows += 1
    assert rows == len(T.SETTINGS) * len(T.LAYERS) * 216


def _failing_cases(T, K):
    L, meta = T.Layer, T.meta
    x = meta(8, 50, 84, 256)
    yield "lvc_conv3x3_nhwc_f16s1", lambda: K.conv2d_nhwc(x, L(3, 3, 256, 256, 1, 1, slot=5))
    yield "lvc_conv2d_nhwc_f16x2_dma", lambda: K.conv2d_nhwc(x, L(1, 1, 256, 1024, slot=5), split="f16x2")      # not slotted
    yield "lvc_conv1x1_nhwc_f16s1_w2", lambda: K.conv2d_nhwc(meta(8000, 1, 1, 12544), L(1, 1, 12544, 1024, slot=5))
    yield "lvc_conv3x3_nhwc_f16_layers", lambda: K.conv3x3_levels([x, meta(8, 25, 42, 256)], [L(3, 3, 256, 256, 1, 1, slot=5), L(3, 3, 256, 256, 1, 1, slot=6)])
    yield "lvc_conv3x3_nhwc_f16_levels_pred", lambda: K.conv3x3_levels_pred([x], L(3, 3, 256, 256, 1, 1, two_acc=True, slot=5), L(1, 1, 256, 15, slot=6))
    yield "lvc_conv3x3_nhwc_f16s1_presplit", lambda: K.conv3x3_conv1x1_presplit(x, L(3, 3, 256, 256, 1, 1, slot=5), L(1, 1, 256, 1024, slot=6))


def test_failed_status_names_the_called_entry_point_and_resets_the_slot(T):
    from lvc_amd._lib import LvcNativeError

    rec = T.Recorder()
    with T.install_stubs(rec) as K:
        cases = list(_failing_cases(T, K))
        for entry, call in cases:
            rec.reset()
            rec.status = 0
            call()
            assert rec.calls[0][0] == entry and rec.slot == 0      # the case's first launch is the entry point it is meant for
            rec.reset()
            rec.status = 3
            with pytest.raises(LvcNativeError) as e:
                call()
            assert rec.calls[-1][0] == entry and len(rec.calls) == 1
            assert str(e.value).startswith(entry + " failed (status 3)")
            assert rec.raw[-1] == ("lvc_set_range_slot", [0]) and rec.slot == 0


def test_data_gradient_cases_reach_their_entry_points(monkeypatch):
    """The data-gradient cases of tests/test_gpu_conv_backward_exact.py (helpers.DGRAD_CASES) land on the entry points they are
    there for -- `conv_route` on plain numbers, under the switches those tests run with -- and between them reach every forward
    kernel the data gradient is built on: a change of the routing thresholds cannot quietly empty a GPU case."""
    from helpers import DGRAD_CASES, DGRAD_ENTRIES_REQUIRED, dgrad_route
    from lvc_amd import _lib
    from lvc_amd import kernels as K

    def no_library():
        raise AssertionError("conv_route touched the native library")

    monkeypatch.setattr(_lib, "lib", no_library)
    for name, value in (("CONV_ENGINE", "bf16x3"), ("CONV_SPLIT", "f16x2"), ("CONV_HALO", True), ("_PW_NARROW", True)):
        monkeypatch.setattr(K, name, value)
    reached = set()
    for split in ("bf16x3", "f16x2"):
        monkeypatch.setattr(K, "DGRAD_SPLIT", split)
        if split == "f16x2":
            monkeypatch.setattr(K, "_HALO_H2_MIN_TILES", 0)
        for shape, want in DGRAD_CASES:
            got = dgrad_route(K, shape, split)
            assert got == want[split], (shape, split, got)
            reached.add(got)
    assert set(DGRAD_ENTRIES_REQUIRED) <= reached
    assert len({shape for shape, _ in DGRAD_CASES}) == len(DGRAD_CASES)


def test_forward_exact_cases_reach_their_entry_points(monkeypatch):
    """The rows of helpers.FWD_CASES (tests/test_gpu_conv_forward_exact.py) land on the entry points they name -- `conv_route` on plain
    numbers under each row's switches, with the residual a row needs for its route -- and, with the fused launches that module drives,
    name every forward entry point there is: a change of the routing cannot quietly move a GPU case onto another kernel."""
    from helpers import FWD_CASES, FWD_FUSED_ENTRIES, fwd_case_id, fwd_route, fwd_set_switches
    from lvc_amd import _lib
    from lvc_amd import kernels as K

    def no_library():
        raise AssertionError("conv_route touched the native library")

    monkeypatch.setattr(_lib, "lib", no_library)
    for case in FWD_CASES:
        fwd_set_switches(monkeypatch, K, case)
        got = fwd_route(K, case, res_mode=case.opts.get("res", 0))
        assert got == case.entry, (fwd_case_id(case), got)
        if case.opts.get("pad_c"):      # the row as written (its own channel count) is the fp32 kernel's as well
            assert fwd_route(K, case._replace(opts={}), 0) == case.entry
    assert len({fwd_case_id(c) for c in FWD_CASES}) == len(FWD_CASES)
    six = {"lvc_conv2d_nhwc_f32", "lvc_conv2d_nhwc_bf16x3", "lvc_conv2d_nhwc_f16x2", "lvc_conv2d_nhwc_f16x2_dma", "lvc_conv3x3_nhwc_bf16x3",
           "lvc_conv3x3_nhwc_f16x2"}
    assert {c.entry for c in FWD_CASES} | set(FWD_FUSED_ENTRIES) == (set(ENTRY_POINTS) - {"lvc_gelu"}) | six


def test_data_gradient_of_an_unbuilt_strided_layer_says_so():
    """Strided layers have a data gradient for 1x1 / padding 0 and 3x3 / padding 1 at stride 2; anything else raises a
    NotImplementedError that names the layer before anything is launched (no bare assert in the middle of a backward pass)."""
    from lvc_amd import kernels as K

    for R, pad, stride in ((3, 0, 2), (3, 1, 3), (1, 0, 3), (5, 2, 2), (1, 1, 2)):
        pcd = types.SimpleNamespace(groups=1, R=R, S=R, pad=R - 1 - pad, C=32, K=32)
        with pytest.raises(NotImplementedError, match="{0}x{0} convolution with stride {1} and padding {2}".format(R, stride, pad)):
            K.conv_dgrad(None, pcd, (1, 8, 8, 32), stride)
