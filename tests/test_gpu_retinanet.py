"""RetinaNet on the device: the selection kernel (csrc/retinanet.hip) against tests/retinanet_ref.py, and the head, the chain
select -> NMS -> postprocess and the whole model against the reference's own RetinaNet run on the CPU (tests/golden/
retinanet_r50_fpn_small.npz, scripts/make_golden_retinanet.py, whose seeds these tests repeat).

Bars are measured or derived, not set: scores may deviate from the fp64 sigmoid by 3 x what torch's CPU fp32 sigmoid deviates on the same
logits; head outputs by 3 x the fixture's own max |fp32 - fp64| per tensor; detections are gated by oracle.noise with the reference
RetinaNet's fp32-vs-fp64 run as the yardstick.  Indices, classes and counts are compared exactly.  Rows go to
profiles/retinanet_parity.json (LVC_RETINANET_PARITY_OUT: another path)."""
import json
import os

import pytest
import torch

import retinanet_ref as ref
from helpers import ROOT, found_bar, gold, match_fraction

pytestmark = pytest.mark.gpu

LEVELS = ("p3", "p4", "p5", "p6", "p7")
STRIDES = (8, 16, 32, 64, 128)
SHAPES = ((25, 42), (13, 21), (7, 11), (4, 6), (2, 3))
B, A, K = 3, 9, 20
PAD_L, PAD_D = 12, 4
SETTINGS = ((1000, 0.05), (100, 0.5), (1000, 0.0))
_SIZES = ((128, 160, 3), (120, 176, 4))
_PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def write_parity():
    yield
    if not _PARITY:
        return
    path = os.environ.get("LVC_RETINANET_PARITY_OUT") or os.path.join(ROOT, "profiles", "retinanet_parity.json")
    try:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.update(_PARITY)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def _dev():
    return torch.device("cuda:0")


def _record(key, ours, noise):
    bar = 3.0 * noise
    _PARITY[key] = {"ours": ours, "noise": noise, "bar": bar}
    print("%-44s ours %.3e  reference's own %.3e  bar %.3e" % (key, ours, noise, bar))
    return bar


def _cells(base=(32, 64, 128, 256, 512)):
    from lvc_amd.modeling.anchor_generator import DefaultAnchorGenerator

    return [DefaultAnchorGenerator.generate_cell_anchors([x, x * 2 ** (1.0 / 3), x * 2 ** (2.0 / 3)], (0.5, 1.0, 2.0)).float() for x in base]


# Test 1's cell anchors are the RetinaNet set scaled by 1/16 (2 .. 51 px): decoded coordinates stay below 1024 px, where one fp32 ulp
# is 6e-5 px and a 1-ulp expf difference moves a side by < 4e-5 px -- the 1e-4 px bar of tests/test_gpu_boxes.py then means what it
# means there.  (With 813 px anchors a correctly rounded coordinate near 4000 px has an ulp of 2.4e-4.)
_SMALL_CELLS = (2, 4, 8, 16, 32)


@pytest.fixture(scope="module")
def small():
    """The small pyramid: padded rows (1e9 planted in the logits' padding), every 5th entry of a level equal (1.5 on the two large
    levels: the cut of every setting falls inside that group; -4 on the small ones: below both thresholds), any logit whose fp64
    sigmoid is within 1e-6 of a threshold replaced by -10."""
    g = torch.Generator().manual_seed(11)
    logits, deltas = [], []
    for l, (h, w) in enumerate(SHAPES):
        x = 1.5 * torch.randn(B, h, w, A * K, generator=g) - 3.0
        flat = x.view(B, -1)
        flat[:, ::5] = 1.5 if l < 2 else -4.0
        p = torch.sigmoid(x.double())
        for _, th in SETTINGS:
            x[(p - th).abs() <= 1e-6] = -10.0
        full = torch.full((B, h, w, A * K + PAD_L), 1e9)
        full[..., : A * K] = x
        d = torch.zeros(B, h, w, 4 * A + PAD_D)
        d[..., : 4 * A] = 0.5 * torch.randn(B, h, w, 4 * A, generator=g)
        logits.append(full)
        deltas.append(d)
    return {"logits": logits, "deltas": deltas, "cells": _cells(_SMALL_CELLS), "expected": {}}


def _select(case, topk, thresh, max_survivors=None, checked=False, cells=None, strides=STRIDES, k=K):
    from lvc_amd import kernels as Kn

    dev = _dev()
    a = case["cells"][0].shape[0]
    lg = [t.to(dev)[..., : a * k] for t in case["logits"]]
    dl = [t.to(dev)[..., : 4 * a] for t in case["deltas"]]
    fn = Kn.retinanet_select_checked if checked else Kn.retinanet_select
    out = fn(lg, dl, [c.to(dev) for c in case["cells"]], strides[: len(lg)], 0.0, k, topk, thresh, (1.0, 1.0, 1.0, 1.0), max_survivors=max_survivors)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def _expected(case, topk, thresh, strides=STRIDES, k=K):
    key = (topk, thresh)
    if key not in case["expected"]:
        a = case["cells"][0].shape[0]
        lg = [t[..., : a * k].contiguous() for t in case["logits"]]
        dl = [t[..., : 4 * a].contiguous() for t in case["deltas"]]
        case["expected"][key] = ref.select_pyramid(lg, dl, case["cells"], strides[: len(lg)], 0.0, k, topk, thresh)
    return case["expected"][key]


def _kept_logits(case, per_level, b, k=K):
    a = case["cells"][0].shape[0]
    return torch.cat([lg[b][..., : a * k].reshape(-1)[p[0]] for lg, p in zip(case["logits"], per_level)])


def _sigmoid_bar(logits32):
    """(torch's CPU fp32 sigmoid against fp64 on these logits, 3 x that): the rule of the GN and grouped-conv parity tests."""
    exact = torch.sigmoid(logits32.double())
    noise = float((torch.sigmoid(logits32).double() - exact).abs().max()) if logits32.numel() else 0.0
    return exact, noise


@pytest.mark.parametrize("topk,thresh", SETTINGS)
def test_select_small_pyramid_vs_ref(small, topk, thresh):
    boxes, scores, classes, index, count, status = _select(small, topk, thresh)
    want = _expected(small, topk, thresh)
    rows = len(SHAPES) * topk
    assert boxes.shape == (B, rows, 4) and int(status) == 0
    worst_box = worst_score = worst_noise = 0.0
    for b in range(B):
        wi, ws, wc, wb, n = ref.flatten_image(want[b], rows)
        assert int(count[b]) == n, (b, int(count[b]), n)
        assert torch.equal(index[b], wi) and torch.equal(classes[b], wc)          # exact, in order, zero past the count
        assert not boxes[b, n:].any() and not scores[b, n:].any()
        assert (index[b, :n].long() % K == classes[b, :n]).all() and int(index[b, :n].max()) < SHAPES[0][0] * SHAPES[0][1] * A * K
        worst_box = max(worst_box, float((boxes[b, :n] - wb[:n]).abs().max()))
        exact, noise = _sigmoid_bar(_kept_logits(small, want[b], b))
        worst_score = max(worst_score, float((scores[b, :n].double() - exact).abs().max()))
        worst_noise = max(worst_noise, noise)
        assert float(boxes[b, :n].abs().max()) < 1024.0
    print("topk %d thresh %.2f: counts %s, box %.3e px, score vs fp64 %.3e (torch %.3e)" % (topk, thresh, count.tolist(), worst_box, worst_score, worst_noise))
    assert worst_box <= 1e-4, worst_box
    bar = _record("sigmoid/small_topk%d_thresh%.2f" % (topk, thresh), worst_score, worst_noise)
    assert worst_score <= bar, (worst_score, bar)
    if thresh == 0.05:
        assert any(len(p[0]) == min(topk, h * w * A) for p, (h, w) in zip(want[0], SHAPES))          # the cap is the number of ANCHORS
        assert len(want[0][4][0]) == 54


def test_select_unaligned_rows():
    """A*K = 15 and rows of 17 floats: no float4 path; A = 3, K = 5, one level larger than a compaction block."""
    g = torch.Generator().manual_seed(12)
    shapes, a, k = ((23, 31), (5, 7)), 3, 5
    case = {"logits": [], "deltas": [], "cells": [c[:a] for c in _cells(_SMALL_CELLS)[:2]], "expected": {}}
    for h, w in shapes:
        x = torch.full((2, h, w, a * k + 2), 1e9)
        x[..., : a * k] = (1.5 * torch.randn(2, h, w, a * k, generator=g) - 3.0).clamp(max=-3.1) + (torch.rand(2, h, w, a * k, generator=g) < 0.1) * 4.0
        case["logits"].append(x)
        case["deltas"].append(0.5 * torch.randn(2, h, w, 4 * a + 1, generator=g))
    for t in case["logits"]:
        v = t[..., : a * k]
        v[(torch.sigmoid(v.double()) - 0.05).abs() <= 1e-6] = -10.0
    boxes, scores, classes, index, count, status = _select(case, 300, 0.05, k=k)
    want = _expected(case, 300, 0.05, k=k)
    for b in range(2):
        wi, ws, wc, wb, n = ref.flatten_image(want[b], 600)
        assert int(count[b]) == n and n > 100
        assert torch.equal(index[b], wi) and torch.equal(classes[b], wc)
        assert float((boxes[b] - wb).abs().max()) <= 1e-4


# ------------------------------------------------------------------ one large level: the multi-workgroup compaction, the radix select
@pytest.fixture(scope="module")
def large():
    g = torch.Generator().manual_seed(13)
    h, w, k = 100, 168, 80
    base = 1.5 * torch.randn(2, h, w, A * k, generator=g) - 3.0
    base[(torch.sigmoid(base.double()) - 0.05).abs() <= 1e-6] = -10.0
    deltas = 0.5 * torch.randn(2, h, w, 4 * A, generator=g)
    return {"base": base, "deltas": deltas, "cells": _cells()[:1], "few": None}


def _large_case(large, mode):
    x = large["base"].clone()
    flat = x.view(2, -1)
    if mode == "few":
        g = torch.Generator().manual_seed(14)
        for b in range(2):
            v = torch.topk(flat[b], 1000)[0][-1]
            flat[b, torch.randint(0, flat.shape[1], (40,), generator=g)] = v
    elif mode == "many":
        flat[:, ::7] = 9.0
    else:
        x.fill_(0.5)
    return {"logits": [x], "deltas": [large["deltas"]], "cells": large["cells"], "expected": {}}


@pytest.mark.parametrize("mode", ("few", "many", "constant"))
def test_select_one_large_level(large, mode):
    case = _large_case(large, mode)
    boxes, scores, classes, index, count, status = _select(case, 1000, 0.05, max_survivors=1 << 16, checked=True, k=80)
    want = _expected(case, 1000, 0.05, k=80)
    for b in range(2):
        wi = want[b][0][0].to(torch.int32)
        assert int(count[b]) == 1000 == len(wi)
        assert torch.equal(index[b, :1000], wi), (mode, b, int((index[b, :1000] != wi).sum()))
        assert torch.equal(classes[b, :1000].long(), want[b][0][2])
    if mode == "constant":
        assert index[0, :1000].tolist() == list(range(1000))
    if mode == "many":
        assert index[1, :1000].tolist() == list(range(0, 7000, 7))


def test_select_is_deterministic(large):
    case = _large_case(large, "few")
    a = _select(case, 1000, 0.05, max_survivors=None, k=80)          # (5.8 M of the 12.1 M entries lie above the threshold)
    b = _select(case, 1000, 0.05, max_survivors=None, k=80)
    assert int(a[5]) == 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ empty and overflow
def test_overflow_sets_the_status_bit_and_the_checked_entry_recovers(small):
    from lvc_amd import kernels as Kn

    raw = _select(small, 1000, 0.05, max_survivors=64)
    assert int(raw[5]) & Kn.RETINANET_OVERFLOW
    full = _select(small, 1000, 0.05, max_survivors=None)
    got = _select(small, 1000, 0.05, max_survivors=64, checked=True)
    assert int(full[5]) == 0 and int(got[5]) == 0
    for x, y in zip(got[:5], full[:5]):
        assert torch.equal(x, y)


@pytest.fixture(scope="module")
def model():
    from lvc_amd.config.presets import retinanet_r_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    m = build_model(retinanet_r_fpn(num_classes=20)).eval()
    return syn.conditioned_retinanet_(m, seed=0)


def _inputs(dev=None):
    from lvc_amd.utils import synthetic as syn

    return [{"image": syn.synthetic_image(seed, h, w).to(dev) if dev is not None else syn.synthetic_image(seed, h, w), "height": h, "width": w}
            for h, w, seed in _SIZES]


def test_nothing_above_the_threshold(small, model):
    from lvc_amd.modeling.roi_heads.roi_heads import instances_from_batched

    case = dict(small, logits=[torch.full_like(t, -10.0) for t in small["logits"]], expected={})
    boxes, scores, classes, index, count, status = _select(case, 1000, 0.05)
    assert count.tolist() == [0] * B and int(status) == 0
    assert not boxes.any() and not scores.any() and not classes.any() and not index.any()
    g = gold("retinanet_r50_fpn_small")
    dev = _dev()
    logits = [torch.full_like(g["logits_" + k], -10.0).to(dev) for k in LEVELS]
    deltas = [g["deltas_" + k].to(dev) for k in LEVELS]
    post = torch.tensor([[1.0, 1.0, h, w] for h, w, _ in _SIZES], device=dev)
    with torch.no_grad():
        ob, osc, ocl, cnt, st = model.select_nms_post(logits, deltas, post)
    insts = instances_from_batched(ob, osc, ocl, cnt, [(h, w) for h, w, _ in _SIZES], st)
    assert [len(i) for i in insts] == [0, 0]
    assert insts[0].pred_boxes.tensor.shape == (0, 4) and insts[0].scores.shape == (0,) and insts[0].pred_classes.dtype == torch.int64


# ------------------------------------------------------------------ head, chain, end to end against the reference's RetinaNet
def test_head_parity(model):
    g = gold("retinanet_r50_fpn_small")
    dev = _dev()
    with torch.no_grad():
        images = model.preprocess_image(_inputs())
        n, _, hp, wp = images.tensor.shape
        x4 = images.tensor.as_strided((n, hp, wp, 4), (hp * wp * 4, wp * 4, 4, 1), images.tensor.storage_offset())
        logits, deltas = model.head_outputs(model.backbone.forward_nhwc(x4))
    torch.cuda.synchronize()
    bad = []
    for l, name in enumerate(LEVELS):
        for kind, ours, width, noise in (("logits", logits[l], A * 20, float(g["err64_logits"][l])), ("deltas", deltas[l], 4 * A, float(g["err64_deltas"][l]))):
            want = g["%s_%s" % (kind, name)]
            got = ours[..., :width].cpu()
            assert got.shape == want.shape, (name, kind, got.shape, want.shape)
            if ours.shape[-1] > width:
                assert not ours[..., width:].any()          # the packed operand's zero channels
            err = float((got - want).abs().max())
            bar = _record("head/%s_%s" % (kind, name), err, noise)
            if err > bar:
                bad.append((name, kind, err, bar))
    assert not bad, bad


def _groups_sorted(scores_ref, classes, boxes):
    """Row order with the rows inside every run of equal reference scores sorted by (class, x1, y1)."""
    order, i, n = [], 0, len(scores_ref)
    while i < n:
        j = i
        while j < n and float(scores_ref[j]) == float(scores_ref[i]):
            j += 1
        order += sorted(range(i, j), key=lambda r: (int(classes[r]), float(boxes[r, 0]), float(boxes[r, 1])))
        i = j
    return torch.tensor(order, dtype=torch.long)


def test_chain_select_nms_postprocess(model):
    g = gold("retinanet_r50_fpn_small")
    dev = _dev()
    logits = [g["logits_" + k].to(dev) for k in LEVELS]
    deltas = [g["deltas_" + k].to(dev) for k in LEVELS]
    post = torch.tensor([[1.0, 1.0, h, w] for h, w, _ in _SIZES], device=dev)
    with torch.no_grad():
        ob, osc, ocl, cnt, st, rows, cand_index = model.select_nms_post(logits, deltas, post, return_rows=True)
    torch.cuda.synchronize()
    assert int(st) == 0
    rows, cand_index = rows.cpu().long(), cand_index.cpu().long()
    for i in range(2):
        wb, ws, wc = g["det32_boxes_%d" % i], g["det32_scores_%d" % i], g["det32_classes_%d" % i]
        n = int(cnt[i])
        assert n == len(ws), (i, n, len(ws))
        gb, gs, gc = ob[i, :n].cpu(), osc[i, :n].cpu(), ocl[i, :n].cpu().long()
        ow, og = _groups_sorted(ws, wc, wb), _groups_sorted(ws, gc, gb)
        aside = int((gc[og] != wc[ow]).sum())
        assert aside <= 0.01 * n, (i, aside, n)          # (the fixture records no tie at a cut or at the threshold: 0 expected)
        same = gc[og] == wc[ow]
        # scores against the fp64 sigmoid of exactly the kept detections' logits: a detection's row in the image's candidate list gives
        # its level (the fixture's candidates per level, which test 1 and the host test pin) and its flat index inside it
        per_level = [int(((g["cand_image"] == i) & (g["cand_level"] == l)).sum()) for l in range(5)]
        ends = torch.tensor(per_level).cumsum(0)
        level = torch.bucketize(rows[i, :n], ends, right=True)
        assert int(level.max()) < 5
        flat = cand_index[i][rows[i, :n]]
        kept = torch.stack([g["logits_" + LEVELS[int(l)]][i].reshape(-1)[int(f)] for l, f in zip(level, flat)])
        assert torch.equal(flat % 20, gc)
        exact, noise = _sigmoid_bar(kept)
        serr = float((gs.double() - exact).abs().max())
        bar = _record("chain/scores_image%d" % i, serr, noise)
        assert serr <= bar, (i, serr, bar)
        tol = 1e-4 * max(1.0, float(wb.abs().max()) / 1000.0)
        berr = float((gb[og][same] - wb[ow][same]).abs().max())
        print("image %d: %d detections, box err %.3e (bar %.3e), score vs fp64 %.3e (torch %.3e)" % (i, n, berr, tol, serr, noise))
        assert berr <= tol, (i, berr, tol)


def test_head_layers_on_the_levels_launch():
    """The route the head takes at full size: `kernels.conv3x3_levels` -- ONE lvc_conv3x3_nhwc_f16_levels launch over five maps, in the
    two-accumulator form -- with cls_score's K = 720 (a partial sixth 128-channel tile) and bbox_pred's operand packed to K = 64, on maps
    large enough for that launch (the fixture images are not).  Against an fp64 evaluation at 256 pixels per level and every channel;
    the bar is 3 x what the per-level generic fp32 kernel (lvc_conv2d_nhwc_f32) deviates from it at the same places."""
    from lvc_amd import kernels as Kn
    from lvc_amd.config.presets import retinanet_r_fpn
    from lvc_amd.layers import ShapeSpec
    from lvc_amd.modeling.meta_arch.retinanet import RetinaNetHead

    dev = _dev()
    g = torch.Generator().manual_seed(21)
    head = RetinaNetHead(retinanet_r_fpn(), [ShapeSpec(channels=256, stride=s) for s in STRIDES])
    with torch.no_grad():
        for conv, std in ((head.cls_score, (2.0 / 2304) ** 0.5), (head.bbox_pred, 0.01)):
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * std)
            conv.bias.copy_(torch.randn(conv.bias.shape, generator=g) * 0.1)
    head = head.to(dev)
    shapes = ((64, 128), (32, 64), (16, 32), (8, 16), (4, 8))
    xs_cpu = [torch.randn(2, h, w, 256, generator=g).relu_() for h, w in shapes]
    xs = [x.to(dev) for x in xs_cpu]
    launched = []
    real = Kn._launch

    def traced(tag, flops, nbytes, slot, what, call):
        launched.append(what)
        return real(tag, flops, nbytes, slot, what, call)

    for conv, name, width in ((head.cls_score, "cls_score", 720), (head.bbox_pred, "bbox_pred", 36)):
        pc = head.packed_layer(conv)
        assert pc.K == (720 if name == "cls_score" else 64) and pc.two_acc
        del launched[:]
        Kn._launch = traced
        try:
            with torch.no_grad():
                outs = Kn.conv3x3_levels(xs, pc, relu=False)
        finally:
            Kn._launch = real
        assert launched == ["lvc_conv3x3_nhwc_f16_levels"], launched
        engine = Kn.CONV_ENGINE
        Kn.CONV_ENGINE = "f32"
        try:
            plain = Kn.pack_conv(conv.weight.detach(), bias=conv.bias.detach(), stride=1, pad=1)
            assert Kn.conv_route(plain, 2, 64, 128).entry == "lvc_conv2d_nhwc_f32"
            refs = [Kn.conv2d_nhwc(x, plain) for x in xs]
        finally:
            Kn.CONV_ENGINE = engine
        torch.cuda.synchronize()
        assert Kn.conv_error_word(dev) == 0
        w64, b64 = conv.weight.detach().cpu().double(), conv.bias.detach().cpu().double()
        ours = noise = 0.0
        for x, o, r, (h, w) in zip(xs_cpu, outs, refs, shapes):
            if o.shape[-1] > width:
                assert not o[..., width:].any()          # the packed operand's zero channels
            n = min(256, 2 * h * w)
            pix = torch.randperm(2 * h * w, generator=g)[:n]
            pix = torch.cat([pix, torch.tensor([0, w - 1, h * w - 1, 2 * h * w - 1])])          # corners: the zero padding
            bi, yi, xi = pix // (h * w), (pix % (h * w)) // w, pix % w
            xp = torch.nn.functional.pad(x.double(), (0, 0, 1, 1, 1, 1))
            patch = torch.stack([xp[bi, yi + r_, xi + s_] for r_ in range(3) for s_ in range(3)], 1).view(-1, 3, 3, 256)
            exact = torch.einsum("prsc,kcrs->pk", patch, w64) + b64
            ours = max(ours, float((o.cpu()[bi, yi, xi][:, :width].double() - exact).abs().max()))
            noise = max(noise, float((r.cpu()[bi, yi, xi].double() - exact).abs().max()))
        bar = _record("levels/%s_K%d" % (name, pc.K), ours, noise)
        assert ours <= bar, (name, ours, bar)


def test_graphed_and_pipelined_inference_take_the_model_unchanged(model):
    """lvc_amd.evaluation's GraphedInference and inference_on_dataset (PipelinedInference, two streams) over a RetinaNet, as they are:
    the same detections as the eager forward."""
    from lvc_amd.evaluation import GraphedInference, inference_on_dataset

    inputs = _inputs(_dev())
    with torch.no_grad():
        eager = model(inputs)
    torch.cuda.synchronize()

    def same(out):
        for a, b in zip(out, eager):
            a, b = a["instances"], b["instances"]
            assert a.image_size == b.image_size and torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor)
            assert torch.equal(a.scores, b.scores) and torch.equal(a.pred_classes, b.pred_classes)

    graphed = GraphedInference(model, inputs)
    graphed.replay(inputs)
    same(graphed.instances())
    batches = [inputs, inputs, inputs]
    got = list(inference_on_dataset(model, batches, depth=2))
    assert len(got) == 3
    for _, out in got:
        same(out)


def test_end_to_end_vs_reference(model):
    from oracle import noise as onoise

    g = gold("retinanet_r50_fpn_small")
    nz = dict(zip(g["noise_keys"].tolist(), [float(v) for v in g["noise_vals"].tolist()]))
    nz["counts_equal"] = bool(nz["counts_equal"])
    with torch.no_grad():
        out = model(_inputs())
    torch.cuda.synchronize()
    ours = [(o["instances"].pred_boxes.tensor.cpu(), o["instances"].scores.cpu(), o["instances"].pred_classes.cpu()) for o in out]
    want = [(g["det32_boxes_%d" % i], g["det32_scores_%d" % i], g["det32_classes_%d" % i].long()) for i in range(2)]
    dev = onoise.deviation(ours, want, nz["box_tol"], nz["score_tol"])
    ok, bars, msg = onoise.gate(dev, nz)
    print("deviation", dev, "bars", bars)
    _PARITY["e2e/deviation"] = {k: (float(v) if not isinstance(v, bool) else v) for k, v in dev.items()}
    _PARITY["e2e/bars"] = {k: float(v) for k, v in bars.items()}
    assert ok, msg
    for (b, s, c), (gb, gs, gc) in zip(ours, want):
        frac, _, _ = match_fraction(b, s, c, gb, gs, gc, nz["box_tol"], nz["score_tol"])
        assert frac >= found_bar(nz["matched_fraction"], len(gs)), (frac, len(gs))
    assert out[0]["instances"].image_size == (128, 160) and out[1]["instances"].image_size == (120, 176)


def test_forward_reads_the_device_once(model):
    """Everything before the final read of counts and status runs under torch's sync-debug mode "error": a host read inside
    (an .item(), a nonzero, a blocking copy) raises."""
    from lvc_amd.modeling.roi_heads.roi_heads import instances_from_batched

    inputs = _inputs(_dev())
    with torch.no_grad():
        model(inputs)                                   # packs the weights, fills the constant caches
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            ob, osc, ocl, cnt, status = model.inference_batched(inputs)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    insts = instances_from_batched(ob, osc, ocl, cnt, [(h, w) for h, w, _ in _SIZES], status)          # the one read
    assert [len(i) for i in insts] == [len(gold("retinanet_r50_fpn_small")["det32_scores_%d" % i]) for i in range(2)]
