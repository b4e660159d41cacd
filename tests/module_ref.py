"""A plain fp64 reference of the conv modules, on the CPU in torch, and the exact-data recipe that makes it a BIT-FOR-BIT reference
(tests/test_gpu_gradient_flow.py; the "kind A" recipe of tests/test_gpu_conv_forward_exact.py / test_gpu_conv_backward_exact.py carried
from single launches to whole modules).

Reference: `Tape.conv` is conv + affine + residual (res_mode 1; res_mode 2 = nearest x2 upsample-add) + ReLU of one `lvc_amd.layers.Conv2d`
with torch's own conv2d and autograd in fp64; `ref_bottleneck`, `ref_bottleneck_d`, `ref_stage`, `ref_resnet`, `ref_fpn` (both top
blocks) and `ref_rpn_head` compose it the way the reference implementation's modules do.  Parameters are copied from the module as it
stands (one fp64 leaf per parameter: a shared weight gets the sum over its uses), the affine is what `Conv2d._affine()` returns.

Exact data (`exact_conv_`, `exact_module_`, `sparse_ints`): weights 0 / +-1 with an expected two non-zeros per filter (about one filter
in eight is all zero: the degenerate row exponent of the row-scaled split), FrozenBN with eps 0, running_var 1, running_mean 0, weight in
{0.5, 1, 1, 1} and an integer bias in [-1, 1] -- so that `_affine()` is an exact power-of-two scale and an integer shift, which
`Tape.conv` asserts --, conv biases integers in [-1, 1], inputs and upstream gradients sparse integers in [-3, 3].

Condition (`Tape.check_caps`, on the CPU, before anything is launched).  The reference is evaluated a second way: every conv on the
absolute values of its operands, and every tensor with its quantum q(t), the largest power of two that divides all its elements.
  * every forward activation (conv input and result) has |v| <= 4094, the limit of the one-accumulator kernels;
  * every operand tensor (activation, folded weight, masked upstream gradient) has max|v| / q < 2^21 and q >= 2^-14: it is the sum of
    two fp16 planes exactly (22 bits; both planes normal or zero), and of three bf16 planes a fortiori;
  * for every conv result (with shift and residual -- the fused projection contracts conv3 and the shortcut in one sum), every data
    gradient and every weight gradient, sum |a||b| < 2^23 in units of the product of the operands' quanta: every partial sum, in any
    order and through any split of the operands into planes, is an integer below 2^24 in that unit, hence exact in fp32.
Under these every engine, route and switch setting must return the fp64 result bit for bit, the ReLU mask (relu'(0) = 0, torch's and
lvc_relu_backward's convention alike) included.
"""
import torch
import torch.nn.functional as F

CAP_ACT = 4094.0
CAP_RATIO = 2.0 ** 21
CAP_SUM = 2.0 ** 23
MIN_QUANTUM = 2.0 ** -14


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def quantum(*ts):
    """The largest power of two that divides every element of the tensors (1.0 when all are zero)."""
    v = torch.cat([t.detach().double().reshape(-1) for t in ts])
    v = v[v != 0]
    if not v.numel():
        return 1.0
    assert bool(torch.isfinite(v).all())
    m, e = torch.frexp(v)                                    # v = m 2^e, 0.5 <= |m| < 1: m 2^53 is an integer
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()                                # its lowest set bit
    tz = torch.log2(low).round().to(torch.int64)             # (exact: a power of two)
    return 2.0 ** int((e.to(torch.int64) + tz - 53).min())


def sparse_ints(g, shape, m=3, keep=0.5):
    """Integers in [-m, m], a fraction `keep` of them kept."""
    return torch.randint(-m, m + 1, shape, generator=g).float() * (torch.rand(shape, generator=g) < keep).float()


def exact_conv_(conv, g, nonzeros=2.0):
    """The exact-data recipe on one `Conv2d` (on the CPU or the device; the values are drawn on the CPU from generator g)."""
    from lvc_amd.layers import FrozenBatchNorm2d

    Kc, C, R, S = conv.weight.shape
    keep = torch.rand(Kc, C, R, S, generator=g) < nonzeros / (C * R * S)
    sign = torch.randint(0, 2, (Kc, C, R, S), generator=g) * 2 - 1
    with torch.no_grad():
        conv.weight.copy_((keep * sign).float())
        if conv.bias is not None:
            conv.bias.copy_(torch.randint(-1, 2, (Kc,), generator=g).float())
        if conv.norm is not None:
            assert isinstance(conv.norm, FrozenBatchNorm2d), "GroupNorm is not exact (rsqrt): out of this recipe's scope"
            conv.norm.eps = 0.0
            conv.norm.running_var.fill_(1.0)
            conv.norm.running_mean.zero_()
            conv.norm.weight.copy_(torch.tensor([0.5, 1.0, 1.0, 1.0])[torch.randint(0, 4, (Kc,), generator=g)])
            conv.norm.bias.copy_(torch.randint(-1, 2, (Kc,), generator=g).float())


def exact_module_(module, g):
    """`exact_conv_` on every Conv2d of `module`, in registration order."""
    from lvc_amd.layers import Conv2d

    for m in module.modules():
        if isinstance(m, Conv2d):
            exact_conv_(m, g)
    return module


def exact_affine(conv):
    """(scale, shift) of `Conv2d._affine()` as fp64 CPU tensors (None where absent), asserted to be what the recipe set: the scale the
    FrozenBN weight itself, a power of two; the shift an integer."""
    scale, shift = conv._affine()
    if scale is not None:
        scale = scale.detach().cpu().double()
        assert torch.equal(scale, conv.norm.weight.detach().cpu().double()), "FrozenBN scale is not weight * rsqrt(1 + 0) exactly"
        assert bool((torch.frexp(scale)[0] == 0.5).all()), "FrozenBN scale is no power of two"
    if shift is not None:
        shift = shift.detach().cpu().double()
        assert torch.equal(shift, shift.round()), "shift is no integer"
    return scale, shift


class Tape:
    """The fp64 leaves of the parameters and one record per conv evaluated (operands, result, upstream gradient once backward ran)."""

    def __init__(self):
        self.leaves = {}
        self.records = []

    def leaf(self, p):
        if id(p) not in self.leaves:
            self.leaves[id(p)] = (p, p.detach().cpu().double().requires_grad_(p.requires_grad))
        return self.leaves[id(p)][1]

    def grad(self, p):
        """fp64 gradient of parameter p (None: not used, or frozen)."""
        ent = self.leaves.get(id(p))
        return None if ent is None else ent[1].grad

    def conv(self, layer, x, residual=None, res_mode=0, relu=None):
        """x, residual: NCHW fp64.  relu None: the layer's own activation."""
        if relu is None:
            relu = layer.activation is not None
        w = self.leaf(layer.weight)
        scale, shift = exact_affine(layer)
        z = F.conv2d(x, w, None, layer.stride, layer.padding, 1, layer.groups)
        w_eff = w.detach()
        if scale is not None:
            z = z * scale.view(1, -1, 1, 1)
            w_eff = w_eff * scale.view(-1, 1, 1, 1)
        bias = None
        if layer.bias is not None and layer.norm is None:
            bias = self.leaf(layer.bias)
            z = z + bias.view(1, -1, 1, 1)
        elif shift is not None:
            z = z + shift.view(1, -1, 1, 1)
        # the second evaluation: absolute values and quanta
        xa, wa = x.detach().abs(), w_eff.abs()
        absb = F.conv2d(xa, wa, None, layer.stride, layer.padding, 1, layer.groups)
        q = quantum(x) * quantum(w_eff)
        if shift is not None:
            absb = absb + shift.abs().view(1, -1, 1, 1)
            q = min(q, quantum(shift))
        if residual is not None:
            r = residual if res_mode == 1 else residual.repeat_interleave(2, 2).repeat_interleave(2, 3)
            z = z + r
            rb = getattr(residual, "_absb", None)
            rb = residual.detach().abs() if rb is None else rb
            absb = absb + (rb if res_mode == 1 else rb.repeat_interleave(2, 2).repeat_interleave(2, 3))
            q = min(q, getattr(residual, "_q", None) or quantum(residual))
        rec = {"layer": layer, "x": x.detach(), "w_eff": w_eff, "absb": absb, "q": q, "x_grad": x.requires_grad, "w_grad": w.requires_grad}
        if z.requires_grad:
            z.register_hook(lambda g, rec=rec: rec.__setitem__("g", g.detach().clone()))      # masked by the ReLU below: what the kernels multiply
        y = F.relu(z) if relu else z
        rec["y"] = y.detach()
        y._absb, y._q = absb, q
        self.records.append(rec)
        return y

    def check_caps(self):
        """The condition of the module docstring, for every conv recorded.  Returns the figures (for the curious)."""
        worst = {"act": 0.0, "ratio": 0.0, "sum": 0.0, "quantum": 1.0}

        def operand(t, what, layer):
            qt = quantum(t)
            ratio = float(t.abs().max()) / qt
            assert ratio < CAP_RATIO and qt >= MIN_QUANTUM, (what, layer, ratio, qt)
            worst["ratio"], worst["quantum"] = max(worst["ratio"], ratio), min(worst["quantum"], qt)
            return qt

        def total(t, unit, what, layer):
            s = float(t.max()) / unit
            assert s < CAP_SUM, (what, layer, s)
            worst["sum"] = max(worst["sum"], s)

        for r in self.records:
            layer, x, w = r["layer"], r["x"], r["w_eff"]
            act = max(float(x.abs().max()), float(r["y"].abs().max()))
            assert act <= CAP_ACT, ("activation", layer, act)
            worst["act"] = max(worst["act"], act)
            qx, qw = operand(x, "input", layer), operand(w, "weight", layer)
            total(r["absb"], r["q"], "forward sum", layer)
            g = r.get("g")
            if g is None:
                continue
            qg = operand(g, "upstream gradient", layer)
            xa, wa = x.abs().requires_grad_(True), w.abs().requires_grad_(True)
            za = F.conv2d(xa, wa, None, layer.stride, layer.padding, 1, layer.groups)
            dxa, dwa = torch.autograd.grad(za, [xa, wa], g.abs())
            if r["x_grad"]:
                total(dxa, qg * qw, "data gradient", layer)
            if r["w_grad"]:
                total(dwa, qg * qx, "weight gradient", layer)
        return worst


# ------------------------------------------------------------------------------------------------------------------ the modules
def ref_bottleneck(tape, blk, x):
    """BottleneckBlock (reference resnet.py:195-211): conv1 -> conv2 -> conv3 + shortcut -> ReLU."""
    t = tape.conv(blk.conv2, tape.conv(blk.conv1, x))
    shortcut = tape.conv(blk.shortcut, x) if blk.shortcut is not None else x
    return tape.conv(blk.conv3, t, residual=shortcut, res_mode=1, relu=True)


def ref_bottleneck_d(tape, blk, x):
    """BottleneckBlockCLIP (reference resnet.py:434-444): AvgPool2d(stride) in front of conv3 and of the shortcut conv."""
    pool = (lambda v: F.avg_pool2d(v, 2)) if blk.stride == 2 else (lambda v: v)
    t = tape.conv(blk.conv2, tape.conv(blk.conv1, x))
    shortcut = tape.conv(blk.shortcut, pool(x)) if blk.shortcut is not None else x
    return tape.conv(blk.conv3, pool(t), residual=shortcut, res_mode=1, relu=True)


def ref_block(tape, blk, x):
    from lvc_amd.modeling.backbone.resnet import BottleneckBlockCLIP

    return (ref_bottleneck_d if isinstance(blk, BottleneckBlockCLIP) else ref_bottleneck)(tape, blk, x)


def ref_stage(tape, blocks, x):
    for blk in blocks:
        x = ref_block(tape, blk, x)
    return x


def ref_resnet(tape, net, image):
    """ResNet with a BasicStem over an NCHW 3-channel image -> {name: map}."""
    y = tape.conv(net.stem.conv1, image)
    x = F.max_pool2d(y, kernel_size=3, stride=2, padding=1)
    out = {}
    if "stem" in net._out_features:
        out["stem"] = x
    for stage, name in net.stages_and_names:
        x = ref_stage(tape, list(stage), x)
        if name in net._out_features:
            out[name] = x
    return out


def ref_fpn(tape, fpn, feats):
    """FPN.forward over given trunk maps {name: NCHW} (reference fpn.py:109-144) -> the list of outputs, fine to coarse."""
    from lvc_amd.modeling.backbone.fpn import LastLevelMaxPool, LastLevelP6P7

    x = [feats[f] for f in fpn.in_features[::-1]]
    prev = tape.conv(fpn.lateral_convs[0], x[0])
    results = [tape.conv(fpn.output_convs[0], prev)]
    for feat, lateral, output in zip(x[1:], fpn.lateral_convs[1:], fpn.output_convs[1:]):
        prev = tape.conv(lateral, feat, residual=prev, res_mode=2)
        if fpn._fuse_type == "avg":
            prev = prev * 0.5
        results.insert(0, tape.conv(output, prev))
    tb = fpn.top_block
    if tb is not None:
        src = feats.get(tb.in_feature)
        if src is None:
            src = results[fpn._out_features.index(tb.in_feature)]
        if isinstance(tb, LastLevelMaxPool):
            results.append(src[:, :, ::2, ::2])
        else:
            assert isinstance(tb, LastLevelP6P7)
            p6 = tape.conv(tb.p6, src)
            results.extend([p6, tape.conv(tb.p7, F.relu(p6))])
    return results


def ref_rpn_head(tape, head, feats):
    """StandardRPNHead over a list of NCHW maps -> per level [N, A + A * box_dim, H, W]: objectness | anchor deltas."""
    out = []
    for x in feats:
        h = tape.conv(head.conv, x)
        out.append(torch.cat([tape.conv(head.objectness_logits, h), tape.conv(head.anchor_deltas, h)], 1))
    return out
