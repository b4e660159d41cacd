"""Integer-exact gradient-flow tests of the wiring ABOVE the conv kernels: the Python that decides which launch a layer takes, whether
autograd sees it, when a weight gradient is final and where it is delivered.  The kernels themselves are held by
tests/test_gpu_conv_forward_exact.py and tests/test_gpu_conv_backward_exact.py; here whole modules -- bottleneck blocks, stages walked
with look-ahead, a small ResNet, the FPN top-down path with both top blocks, the shared RPN head -- and `GradientBuckets` over a small
net are compared with the fp64 reference of tests/module_ref.py BIT FOR BIT: the data follows that module's exact recipe, its condition
is asserted on the CPU before anything is launched (`Tape.check_caps`), and then every engine, route and switch setting must return the
reference rounded to fp32 (`torch.equal`; there is no tolerance in this file).  The conv error word is cleared before each run and must
be 0 after.

Module matrix.  States: T all parameters trainable; F0 all frozen, inputs without grad, autograd enabled; Fx all frozen, inputs require
grad; M mixed (per case).  Every case asserts the outputs, the gradient of every differentiable input and of every trainable
parameter (present, and equal to the reference -- so a gradient that is missing or zero where the reference's is not fails), `grad is
None` on every frozen parameter, and in F0 that the recorded entry points are those of the same pass under `torch.no_grad()` and hold
the fused launch the case is there for (lvc_bottleneck_nhwc_f16s1, the chain kernel, the fused projection GEMM, the merged-levels
launches): the input guards must not buy correctness by turning those routes off.  T and M are repeated under DGRAD_SPLIT in {bf16x3,
f16x2} x WGRAD_ENGINE in {bf16x3, f32, f16x2} x DEFER_WGRAD in {on, off}: one reference serves all twelve.

Delivery matrix.  A small net of `Conv2d` layers (32 / 64 channels, 6 x 8 maps, one layer used three times) under `GradientBuckets` with
four buckets, for the switch sets default / DEFER_WGRAD off / WGRAD_ENGINE f32 / DGRAD_SPLIT f16x2: a step after an abandoned
grad-enabled forward, after a forward that raised half-way, three steps in a row, `torch.autograd.grad` after an abandoned forward,
and a step in which one branch ran forward but is left out of the loss.  Every `.grad` is the bucket view and equals the reference;
`pending == 0` BEFORE `finish()` in every bucket whose parameters were all used (`finish` must not be what supplies a used parameter's
gradient); no positive use count and an empty queue after.

Reproduced by these tests on an MI355X at the parent commit's library code, 37 of 97 failing (each cause named in ADVICE.md or in the
issue that asked for this file):
  * stale use counts (`GradientBuckets._hook` read `kernels._WGRAD_USES`): test_delivery "abandoned", "failed", "grad_then_step" and
    "unused_branch" under the three non-default switch sets (12 cases) -- "before finish(): pending 1 in the bucket of ..." for the
    first bucket with a conv weight (after the forward that raised half-way: the bucket of shared.weight, one of the two layers that
    had run): every conv weight that the abandoned forward had counted stayed unseen and `finish()` would have zero-filled it.  The
    default set passed (the final flush of the deferred queue clears the counts), and so did "three_steps" everywhere;
  * parameter-only `_grad_free` of `BottleneckBlock`: test_block[identity-Fx], [projection-Fx], [stride2_1x1-Fx] ("output 0:
    requires_grad False, the reference's True": the fused block / the fused projection GEMM returned a detached tensor);
    test_stage[*-Fx] of all five stages; [*-M_last_frozen] of res2x2, res2x3, res2x3_chain and res3 (the frozen last block cut the
    gradient to the trainable first one); [*-M_first_frozen] and [*-M_conv3_only] of res2x2, res2x3 and res3 ("input 0 received no
    gradient", or a detached output).  The stride-in-3x3, ResNeXt and ResNet-D blocks already took the autograd path.
    (test_block[projection_concat-*] cannot run there: it passes x to `can_fuse_projection`, which took no argument);
  * parameter-only `grad_free` of `FPN.forward_nhwc`: test_fpn[*-Fx], all four -- the merged output convs returned detached maps, no
    trunk map received a gradient.
All 97 pass with the guards on the inputs (`BottleneckBlock._grad_free(x, t)`, `FPN.forward_nhwc`), the queue-only hook and the counts
dropped in `finish()`; every T, F0 and mixed FPN / RPN / ResNet case passed before and after.  The guards run on the host once per
block (and once per pyramid) per forward: a few attribute reads each, whose cost was not measured.
"""
import types

import pytest
import torch
import torch.nn.functional as F

from helpers import FWD_FUSED, FWD_SWITCHES, Recorded, gen
from module_ref import Tape, exact_module_, nchw, nhwc, ref_block, ref_fpn, ref_resnet, ref_rpn_head, ref_stage, sparse_ints

pytestmark = pytest.mark.gpu

SWITCH_SETS = tuple({"DGRAD_SPLIT": d, "WGRAD_ENGINE": w, "DEFER_WGRAD": f}
                    for d in ("bf16x3", "f16x2") for w in ("bf16x3", "f32", "f16x2") for f in (True, False))
DEFAULT_SET = ({"DGRAD_SPLIT": "bf16x3", "WGRAD_ENGINE": "bf16x3", "DEFER_WGRAD": True},)


def _dev():
    return torch.device("cuda:0")


def _equal(got, ref64, what):
    """got (device, fp32) against the fp64 reference: the reference is an fp32 number, and got is that number."""
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64), what + ": the reference is not exact in fp32"
    got = got.detach().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if torch.equal(got, ref):
        return
    bad = (got != ref).nonzero()
    first = ["%s got %r want %r" % (tuple(i.tolist()), float(got[tuple(i)]), float(ref[tuple(i)])) for i in bad[:4]]
    raise AssertionError("%s: %d of %d elements differ (%d non-zero in the result, %d in the reference); first: %s" % (
        what, len(bad), ref.numel(), int((got != 0).sum()), int((ref != 0).sum()), "; ".join(first)))


def _case(module, xs, dev_fwd, ref_fwd, switches=None, f0_entries=(), f0_launches=None, out_channels=None):
    """module: the parameters' owner; xs: CPU NHWC inputs; dev_fwd(xs on the device) -> list of NHWC outputs; ref_fwd(tape, NCHW fp64
    inputs) -> list of NCHW outputs; f0_entries / f0_launches: the entry points the F0 pass must hold / its number of launches;
    out_channels: the leading channels of a device output the reference has (the fused predictor's rows are padded)."""
    return types.SimpleNamespace(module=module, xs=xs, dev_fwd=dev_fwd, ref_fwd=ref_fwd, switches=dict(switches or {}), f0_entries=tuple(f0_entries),
                                 f0_launches=f0_launches, out_channels=out_channels)


def _set_state(case, state):
    """Apply a state to the case's parameters -> whether the inputs require grad.  state: "T" / "F0" / "Fx" or (name, fn) with
    fn(module) -> the trainable parameters of a mixed state (inputs require grad, unless a third entry says otherwise)."""
    params = list(case.module.parameters())
    if isinstance(state, str):
        for p in params:
            p.requires_grad_(state == "T")
        return state != "F0"
    keep = {id(p) for p in state[1](case.module)}
    assert keep and len(keep) < len(params)
    for p in params:
        p.requires_grad_(id(p) in keep)
    return state[2] if len(state) > 2 else True


def _state_id(state):
    return state if isinstance(state, str) else state[0]


def reference(case, state):
    """The reference half, on the CPU: the state applied, the fp64 pass and its backward, the condition of module_ref asserted.
    tests/test_host_gradient_flow.py runs it alone for every case on a machine without a GPU."""
    in_grad = _set_state(case, state)
    params = [p for p in case.module.parameters()]
    tape = Tape()
    xr = [nchw(x).double().requires_grad_(in_grad) for x in case.xs]
    yr = case.ref_fwd(tape, xr)
    g = gen(tuple(case.xs[0].shape), 71)
    dys = []
    for y in yr:
        n, c, h, w = y.shape
        dys.append(sparse_ints(g, (n, h, w, case.out_channels or c), 3, 0.25))      # NHWC, as wide as the device's output
    diff = [i for i, y in enumerate(yr) if y.requires_grad]
    if diff:
        torch.autograd.backward([yr[i] for i in diff], [nchw(dys[i])[:, :yr[i].shape[1]].double() for i in diff])
    figures = tape.check_caps()
    print("caps %s: max |activation| %g, max|v|/quantum %g, sum|a||b| %g quanta, smallest quantum %g" % (
        _state_id(state), figures["act"], figures["ratio"], figures["sum"], figures["quantum"]))
    if state == "F0":
        assert not diff
    else:
        assert diff and (not in_grad or all(x.grad is not None and bool((x.grad != 0).any()) for x in xr)), "the reference itself has no gradient to lose"
        assert all(tape.grad(p) is not None and bool((tape.grad(p) != 0).any()) for p in params if p.requires_grad)
    return tape, in_grad, xr, yr, dys, diff


def _run(case, state, monkeypatch):
    from lvc_amd import kernels as Kn

    dev = _dev()
    for name, value in dict(FWD_SWITCHES, **case.switches).items():
        monkeypatch.setattr(Kn, name, value)
    case.module.to(dev)
    # ---- the reference, once, and its condition: nothing of ours has been launched yet
    tape, in_grad, xr, yr, dys, diff = reference(case, state)
    params = [p for p in case.module.parameters()]
    # ---- the device
    rec = Recorded(Kn, monkeypatch)
    for sw in (SWITCH_SETS if not isinstance(state, str) or state == "T" else DEFAULT_SET):
        what = "%s %s" % (_state_id(state), "/".join("%s" % v for v in sw.values()))
        for name, value in sw.items():
            monkeypatch.setattr(Kn, name, value)
        for p in params:
            p.grad = None
        xd = [x.to(dev).requires_grad_(in_grad) for x in case.xs]
        Kn.clear_conv_error_word(dev)
        del rec.ran[:]
        yd = case.dev_fwd(xd)
        ran = list(rec.ran)
        assert len(yd) == len(yr)
        for i, (a, b) in enumerate(zip(yd, yr)):
            c = b.shape[1]
            _equal(a[..., :c], nhwc(b.detach()), "%s output %d" % (what, i))
            assert bool((a[..., c:] == 0).all()), "%s output %d: pad channels" % (what, i)
            assert a.requires_grad == b.requires_grad, "%s output %d: requires_grad %s, the reference's %s" % (what, i, a.requires_grad, b.requires_grad)
        if diff:
            torch.autograd.backward([yd[i] for i in diff], [dys[i].to(dev) for i in diff])
        assert Kn.conv_error_word(dev) == 0, what
        assert not Kn._WGRAD_Q and not any(n > 0 for n in Kn._WGRAD_USES.values()), what
        for i, (a, b) in enumerate(zip(xd, xr)):
            if in_grad:
                assert a.grad is not None, "%s input %d received no gradient" % (what, i)
                _equal(a.grad, nhwc(b.grad), "%s gradient of input %d" % (what, i))
        for name, p in case.module.named_parameters():
            if p.requires_grad:
                assert p.grad is not None, "%s %s received no gradient" % (what, name)
                _equal(p.grad, tape.grad(p), "%s gradient of %s" % (what, name))
            else:
                assert p.grad is None, "%s frozen %s has a gradient" % (what, name)
        if state == "F0":
            del rec.ran[:]
            with torch.no_grad():
                yn = case.dev_fwd([x.to(dev) for x in case.xs])
            assert ran == rec.ran, "F0 ran %s, no_grad %s" % (ran, rec.ran)
            for a, b in zip(yd, yn):
                assert torch.equal(a, b)
            for entry in case.f0_entries:
                assert entry in ran, (entry, ran)
            if case.f0_launches is not None:
                assert len(ran) == case.f0_launches, ran


@pytest.fixture(autouse=True)
def _clean_state():
    """Nothing leaks into the next test: the process-wide queue and use counts are reset whatever happened."""
    from lvc_amd import kernels as Kn

    Kn.reset_wgrad_queue()
    try:
        yield
    finally:
        Kn.reset_wgrad_queue()
        Kn.clear_conv_error_word(_dev())


# ============================================================================================================ single blocks
N, H, W = 2, 9, 11      # odd extents, ragged tiles; the fused routes have no lower size limit under helpers.FWD_SWITCHES


def _block(kind):
    from lvc_amd.modeling.backbone.resnet import BottleneckBlock, BottleneckBlockCLIP

    g = gen((N, H, W, len(kind)) + tuple(map(ord, kind[:6])), 72)
    sw, entries, launches = {}, (), None
    B = FWD_FUSED["bottleneck"]
    if kind == "identity":              # a kernels.BNECK_SHAPES row
        blk, entries, launches = BottleneckBlock(256, 256, bottleneck_channels=64, stride_in_1x1=True, norm="FrozenBN"), (B,), 1
    elif kind == "projection":          # a kernels.BNECK_SHAPES row
        blk, entries, launches = BottleneckBlock(64, 256, bottleneck_channels=64, stride_in_1x1=True, norm="FrozenBN"), (B,), 1
    elif kind == "projection_concat":   # K.BNECK off: conv1, conv2 into the concat buffer, conv3 + shortcut as one GEMM
        blk, sw, launches = BottleneckBlock(64, 256, bottleneck_channels=64, stride_in_1x1=True, norm="FrozenBN"), {"BNECK": False}, 3
    elif kind == "stride2_1x1":         # the strided fused projection with subsample2_into: three launches, not four
        blk, launches = BottleneckBlock(256, 512, bottleneck_channels=128, stride=2, stride_in_1x1=True, norm="FrozenBN"), 3
    elif kind == "stride2_3x3":
        blk, launches = BottleneckBlock(256, 512, bottleneck_channels=128, stride=2, stride_in_1x1=False, norm="FrozenBN"), None
    elif kind == "resnext":             # grouped conv2: declines the dense routes
        blk, launches = BottleneckBlock(256, 256, bottleneck_channels=128, num_groups=32, stride_in_1x1=True, norm="FrozenBN"), None
    elif kind == "clip_s1":
        blk, launches = BottleneckBlockCLIP(64, 256, bottleneck_channels=64, stride=1, norm="FrozenBN"), None
    else:
        assert kind == "clip_s2"        # pooled fused projection in gradient-free passes: three launches, not four
        blk, launches = BottleneckBlockCLIP(256, 512, bottleneck_channels=128, stride=2, norm="FrozenBN"), 3
    exact_module_(blk, g)
    x = sparse_ints(g, (N, H, W, blk.in_channels), 3, 0.5)

    def dev_fwd(xs):
        (xd,) = xs
        if kind == "projection_concat" and blk.can_fuse_projection(xd) and not blk.fused_eligible(xd):
            # what ResNet.forward_nhwc does for res2.0: the producer of x (there: the stem) leaves a second copy in the buffer's tail
            cb = blk.conv2.out_channels
            concat = torch.empty(N, H, W, cb + blk.in_channels, device=xd.device)
            concat[..., cb:] = xd.detach()
            return [blk.forward_nhwc(xd, concat=concat)]
        return [blk.forward_nhwc(xd)]

    return _case(blk, [x], dev_fwd, lambda tape, xr: [ref_block(tape, blk, xr[0])], switches=sw, f0_entries=entries, f0_launches=launches)


BLOCKS = ("identity", "projection", "projection_concat", "stride2_1x1", "stride2_3x3", "resnext", "clip_s1", "clip_s2")


@pytest.mark.parametrize("state", ("T", "F0", "Fx"))
@pytest.mark.parametrize("kind", BLOCKS)
def test_block(kind, state, monkeypatch):
    _run(_block(kind), state, monkeypatch)


# ==================================================================================================================== stages
def _walk(blocks, x):
    """The walk of `ResNet.forward_nhwc` over one stage: `forward_chained` with look-ahead."""
    from lvc_amd.modeling.backbone.resnet import BottleneckBlock

    t = None
    for i, blk in enumerate(blocks):
        nxt = blocks[i + 1] if i + 1 < len(blocks) else None
        if isinstance(blk, BottleneckBlock):
            x, t = blk.forward_chained(x, t, nxt if isinstance(nxt, BottleneckBlock) else None)
        else:
            x, t = blk.forward_nhwc(x), None
    return x


def _stage(kind):
    from lvc_amd import kernels as Kn
    from lvc_amd.modeling.backbone.resnet import BottleneckBlock, ResNet

    g = gen((N, H, W) + tuple(map(ord, kind[:8])), 73)
    B, C = FWD_FUSED["bottleneck"], FWD_FUSED["chain"]
    if kind.startswith("res2"):
        n = int(kind[5])
        blocks = ResNet.make_stage(BottleneckBlock, n, 1, in_channels=256, out_channels=256, bottleneck_channels=64, stride_in_1x1=True, norm="FrozenBN")
        if kind.endswith("chain"):      # K.BNECK off: conv3 -> next conv1 on the chain kernel, row (64, 256, 64)
            assert (64, 256, 64) in Kn.CHAIN_SHAPES
            sw, entries, launches = {"BNECK": False}, (C,), 3 * n - (n - 1)
        else:
            sw, entries, launches = {}, (B,), n
    else:
        assert kind == "res3" and (128, 512, 128) in Kn.CHAIN_SHAPES
        blocks = ResNet.make_stage(BottleneckBlock, 3, 2, in_channels=256, out_channels=512, bottleneck_channels=128, stride_in_1x1=True, norm="FrozenBN")
        sw, entries, launches = {}, (C,), 4 + 3 + 3 - 2      # the head keeps its shortcut launch: its conv3 chains into res3.1.conv1
    stage = torch.nn.Sequential(*blocks)
    exact_module_(stage, g)
    x = sparse_ints(g, (N, H, W, 256), 3, 0.5)
    return _case(stage, [x], lambda xs: [_walk(list(stage), xs[0])], lambda tape, xr: [ref_stage(tape, list(stage), xr[0])],
                 switches=sw, f0_entries=entries, f0_launches=launches)


STAGES = ("res2x2", "res2x3", "res2x2_chain", "res2x3_chain", "res3")
STAGE_STATES = ("T", "F0", "Fx",
                ("M_first_frozen", lambda st: [p for b in list(st)[1:] for p in b.parameters()]),
                ("M_last_frozen", lambda st: list(st[0].parameters())),      # the frozen block's input requires grad through the block before it
                ("M_conv3_only", lambda st: [st[1].conv3.weight]))


@pytest.mark.parametrize("state", STAGE_STATES, ids=_state_id)
@pytest.mark.parametrize("kind", STAGES)
def test_stage(kind, state, monkeypatch):
    _run(_stage(kind), state, monkeypatch)


# ============================================================================================================== a small ResNet
def _resnet(bneck):
    from lvc_amd.modeling.backbone.resnet import BasicStem, BottleneckBlock, ResNet

    g = gen((2, 40, 56, int(bneck)), 74)
    stages, cin = [], 64
    for i, (mid, cout) in enumerate(((64, 256), (128, 512), (256, 1024), (512, 2048))):
        stages.append(ResNet.make_stage(BottleneckBlock, 1, 1 if i == 0 else 2, in_channels=cin, out_channels=cout, bottleneck_channels=mid,
                                        stride_in_1x1=True, norm="FrozenBN"))
        cin = cout
    net = ResNet(BasicStem(3, 64, norm="FrozenBN"), stages, out_features=["res2", "res3", "res4", "res5"])
    exact_module_(net, g)
    names = ["res2", "res3", "res4", "res5"]
    image = sparse_ints(g, (2, 40, 56, 3), 3, 0.5)

    def dev_fwd(xs):
        x4 = F.pad(xs[0], (0, 1)).contiguous()
        out = net.forward_nhwc(x4)
        return [out[k] for k in names]

    def ref_fwd(tape, xr):
        out = ref_resnet(tape, net, xr[0])
        return [out[k] for k in names]

    return _case(net, [image], dev_fwd, ref_fwd, switches={"BNECK": bneck, "STEM_FUSED": True}), net, image, dev_fwd


def _freeze_at_2(net):
    frozen = {id(p) for p in list(net.stem.parameters()) + list(net.res2.parameters())}
    return [p for p in net.parameters() if id(p) not in frozen]


_resnet_state = ("freeze_at_2", _freeze_at_2, False)      # (the image never requires grad: the stem's convolution is not trainable by design)


@pytest.mark.parametrize("bneck", (True, False), ids=("bneck", "concat_chain"))
def test_resnet_freeze_at_2(bneck, monkeypatch):
    """BasicStem + one block per stage, `freeze(2)`: the stem runs as the fused stem + pool launch (with K.BNECK off it writes the second
    copy into res2.0's concat buffer, and res2.0 ends in its fused projection GEMM); res2 stays on its fused routes under enabled
    autograd with res3..res5 training, whose gradients are exact.  Asserted on the recorded launches of the training pass itself."""
    from lvc_amd import kernels as Kn

    case, net, image, dev_fwd = _resnet(bneck)
    _run(case, _resnet_state, monkeypatch)
    # the launches of one TRAINING forward (autograd enabled, res3..res5 trainable), the stem's among them
    rec = Recorded(Kn, monkeypatch)
    stem = Kn.stem_conv_pool
    monkeypatch.setattr(Kn, "stem_conv_pool", lambda x4, pc, relu=True, second=None: (rec.ran.append("stem+pool" + ("+copy" if second is not None else "")),
                                                                                     stem(x4, pc, relu=relu, second=second))[1])
    assert any(p.requires_grad for p in net.res3.parameters()) and torch.is_grad_enabled()
    out = dev_fwd([image.to(_dev())])
    assert not out[0].requires_grad and all(o.requires_grad for o in out[1:])
    # res2 (one block) keeps its fused route: one launch with K.BNECK; else the stem leaves the second copy in res2.0's concat buffer and
    # the block is conv1, conv2 into the buffer, conv3 + shortcut as one GEMM.  res3.0 .. res5.0 train: four launches each, none fused
    res2 = 1 if bneck else 3
    assert rec.ran[0] == ("stem+pool" if bneck else "stem+pool+copy"), rec.ran
    assert len(rec.ran) == 1 + res2 + 12, rec.ran
    assert (rec.ran[1] == FWD_FUSED["bottleneck"]) == bneck and all(e not in FWD_FUSED.values() for e in rec.ran[2:]), rec.ran


# ======================================================================================================================= FPN
FPN_MAPS = (("res3", 64, 8, 12, 16), ("res4", 128, 16, 6, 8), ("res5", 256, 32, 3, 4))      # name, channels, stride, H, W: even extents where res_mode 2 reads


def _fpn(fuse, top):
    from lvc_amd.layers import ShapeSpec
    from lvc_amd.modeling.backbone.backbone import Backbone
    from lvc_amd.modeling.backbone.fpn import FPN, LastLevelMaxPool, LastLevelP6P7

    class Trunk(Backbone):
        """A stub trunk: hands out the maps it was given, as leaves."""

        def __init__(self):
            super().__init__()
            self.maps = None

        def output_shape(self):
            return {n: ShapeSpec(channels=c, stride=s) for n, c, s, _, _ in FPN_MAPS}

        def forward_nhwc(self, x4):
            return dict(self.maps)

    g = gen((N, len(fuse), len(top)), 75)
    trunk = Trunk()
    tb = LastLevelMaxPool() if top == "maxpool" else LastLevelP6P7(256, 64, in_feature="res5")
    fpn = FPN(trunk, [n for n, *_ in FPN_MAPS], 64, norm="", top_block=tb, fuse_type=fuse)
    exact_module_(fpn, g)
    xs = [sparse_ints(g, (N, h, w, c), 3, 0.5) for _, c, _, h, w in FPN_MAPS]
    names = [n for n, *_ in FPN_MAPS]

    def dev_fwd(xd):
        trunk.maps = dict(zip(names, xd))
        out = fpn.forward_nhwc(None)
        return [out[k] for k in fpn._out_features]

    def ref_fwd(tape, xr):
        return ref_fpn(tape, fpn, dict(zip(names, xr)))

    # gradient-free: three laterals, ONE launch for the three output convs (a layer per map), the top block's convs
    return _case(fpn, xs, dev_fwd, ref_fwd, f0_entries=(FWD_FUSED["layers"],), f0_launches=3 + 1 + (0 if top == "maxpool" else 2))


FPN_STATES = ("T", "F0", "Fx", ("M_laterals", lambda m: [p for c in m.lateral_convs for p in c.parameters()]))


@pytest.mark.parametrize("state", FPN_STATES, ids=_state_id)
@pytest.mark.parametrize("top", ("maxpool", "p6p7"))
@pytest.mark.parametrize("fuse", ("sum", "avg"))
def test_fpn(fuse, top, state, monkeypatch):
    """The gradient reaching each trunk map is the sum of its lateral path and of everything upsampled below it (and, for res5 under
    LastLevelP6P7, of p6 and p7 through `_Relu`; under LastLevelMaxPool p6 scatters into p5 through `_Subsample2`)."""
    _run(_fpn(fuse, top), state, monkeypatch)


# ================================================================================================================== RPN head
RPN_MAPS = ((12, 16), (6, 8), (3, 5))


def _rpn():
    from lvc_amd.modeling.proposal_generator.rpn import StandardRPNHead

    g = gen((N, 128, 3), 76)
    head = StandardRPNHead(in_channels=128, num_anchors=3, box_dim=4)      # 3 + 12 = 15 predictor rows, padded to 16
    exact_module_(head, g)
    xs = [sparse_ints(g, (N, h, w, 128), 3, 0.5) for h, w in RPN_MAPS]
    # the upstream gradient is 16 channels wide: what reaches the zero pad channel must not leak into either parameter
    return _case(head, xs, lambda xd: list(head.forward_nhwc(xd)), lambda tape, xr: ref_rpn_head(tape, head, xr),
                 f0_entries=(FWD_FUSED["levels_pred"],), f0_launches=1, out_channels=16)


RPN_STATES = ("T", "F0", "Fx",
              ("M_objectness", lambda m: list(m.objectness_logits.parameters())),
              ("M_conv", lambda m: list(m.conv.parameters())))


@pytest.mark.parametrize("state", RPN_STATES, ids=_state_id)
def test_rpn_head(state, monkeypatch):
    """One head shared by three levels of different sizes: in T the shared conv and both predictors receive the exact sum over the levels."""
    _run(_rpn(), state, monkeypatch)


def module_cases():
    """(id, builder of the case, state) of the whole module matrix."""
    rows = [("block-%s-%s" % (k, st), (lambda k=k: _block(k)), st) for k in BLOCKS for st in ("T", "F0", "Fx")]
    rows += [("stage-%s-%s" % (k, _state_id(st)), (lambda k=k: _stage(k)), st) for k in STAGES for st in STAGE_STATES]
    rows += [("fpn-%s-%s-%s" % (f, t, _state_id(st)), (lambda f=f, t=t: _fpn(f, t)), st) for f in ("sum", "avg") for t in ("maxpool", "p6p7") for st in FPN_STATES]
    rows += [("rpn-%s" % _state_id(st), _rpn, st) for st in RPN_STATES]
    rows += [("resnet-%s" % ("bneck" if b else "concat_chain"), (lambda b=b: _resnet(b)[0]), _resnet_state) for b in (True, False)]
    return rows


# ============================================================================================================ delivery matrix
DELIVERY_SETS = {"default": {}, "defer_off": {"DEFER_WGRAD": False}, "wgrad_f32": {"WGRAD_ENGINE": "f32"}, "dgrad_f16x2": {"DGRAD_SPLIT": "f16x2"}}


class _Net(torch.nn.Module):
    """a (3x3, 32 -> 64) -> shared (1x1, 64 -> 64) three times -> b (3x3, 64 -> 32) and side (1x1, 64 -> 32)."""

    def __init__(self):
        from lvc_amd.layers import Conv2d

        super().__init__()
        self.a = Conv2d(32, 64, 3, padding=1, activation=F.relu_)
        self.shared = Conv2d(64, 64, 1, bias=False, activation=F.relu_)
        self.b = Conv2d(64, 32, 3, padding=1)
        self.side = Conv2d(64, 32, 1)
        self.fail = False

    def forward(self, x):
        h = self.shared.forward_nhwc(self.a.forward_nhwc(x))
        if self.fail:
            raise RuntimeError("half-way")      # two layers ran
        h = self.shared.forward_nhwc(self.shared.forward_nhwc(h))
        return self.b.forward_nhwc(h), self.side.forward_nhwc(h)


def _net_ref(tape, net, x):
    h = tape.conv(net.a, x)
    for _ in range(3):
        h = tape.conv(net.shared, h)
    return tape.conv(net.b, h), tape.conv(net.side, h)


@pytest.mark.parametrize("scenario", ("abandoned", "failed", "three_steps", "grad_then_step", "unused_branch"))
@pytest.mark.parametrize("switches", list(DELIVERY_SETS), ids=list(DELIVERY_SETS))
def test_delivery(switches, scenario, monkeypatch):
    from lvc_amd import distributed as D, kernels as Kn

    dev = _dev()
    for name, value in dict(FWD_SWITCHES, **dict(DEFAULT_SET[0], **DELIVERY_SETS[switches])).items():
        monkeypatch.setattr(Kn, name, value)
    g = gen((2, 6, 8, 32), 77)
    net = exact_module_(_Net(), g).to(dev)
    x = sparse_ints(g, (2, 6, 8, 32), 3, 0.5)
    dy = [sparse_ints(g, (2, 6, 8, 32), 3, 0.25) for _ in range(2)]
    params = list(net.parameters())
    names = {id(p): n for n, p in net.named_parameters()}
    # the reference, with and without the side branch in the loss
    refs = {}
    for use_side in (True, False):
        tape = Tape()
        ym, ys = _net_ref(tape, net, nchw(x).double())
        outs, gs = ([ym, ys], dy) if use_side else ([ym], dy[:1])
        torch.autograd.backward(outs, [nchw(d).double() for d in gs])
        tape.check_caps()
        refs[use_side] = {id(p): tape.grad(p) for p in params}
        ref_out = (ym.detach(), ys.detach())
    side = {id(p) for p in net.side.parameters()}
    assert all(refs[True][id(p)] is not None and bool((refs[True][id(p)] != 0).any()) for p in params)
    assert all((refs[False][id(p)] is None) == (id(p) in side) for p in params)
    buckets = D.GradientBuckets(params, bucket_bytes=80 << 10)
    assert len(buckets.buckets) >= 3
    xd, dyd = x.to(dev), [d.to(dev) for d in dy]
    Kn.clear_conv_error_word(dev)

    def step(use_side=True):
        for p in params:
            p.grad = None
        ym, ys = net(xd)      # (the side branch always runs forward: left out of the loss, its backward never runs)
        _equal(ym, nhwc(ref_out[0]), "output")
        _equal(ys, nhwc(ref_out[1]), "side output")
        torch.autograd.backward([ym, ys] if use_side else [ym], dyd if use_side else dyd[:1])
        for b in buckets.buckets:
            if use_side or not any(id(p) in side for p in b["params"]):
                assert b["pending"] == 0, "before finish(): pending %d in the bucket of %s" % (b["pending"], [names[id(p)] for p in b["params"]])
        buckets.finish()
        for p in params:
            flat = buckets.buckets[buckets._where[id(p)][0]]["flat"]
            assert p.grad is not None and flat.data_ptr() <= p.grad.data_ptr() < flat.data_ptr() + flat.numel() * 4, names[id(p)]
            ref = refs[use_side][id(p)]
            _equal(p.grad, ref if ref is not None else torch.zeros_like(p, device="cpu").double(), "gradient of " + names[id(p)])
        assert not Kn._WGRAD_Q and not any(n > 0 for n in Kn._WGRAD_USES.values()), dict(Kn._WGRAD_USES)
        assert Kn.conv_error_word(dev) == 0

    try:
        if scenario == "abandoned":
            net(xd)      # grad-enabled, result dropped
            step()
        elif scenario == "failed":
            net.fail = True
            with pytest.raises(RuntimeError, match="half-way"):
                net(xd)
            net.fail = False
            step()
        elif scenario == "three_steps":
            for _ in range(3):
                step()
        elif scenario == "grad_then_step":
            net(xd)
            ym, ys = net(xd)
            got = torch.autograd.grad([ym, ys], params, dyd)
            for p, gp in zip(params, got):
                _equal(gp, refs[True][id(p)], "autograd.grad of " + names[id(p)])
            assert not Kn._WGRAD_Q
            step()
        else:
            net(xd)
            step(use_side=False)      # the side layer alone may be zero-filled
            step()
    finally:
        buckets.remove()
        Kn.reset_wgrad_queue()
