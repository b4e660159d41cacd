"""The kernels that build training targets and losses (csrc/train.hip, csrc/train_targets.hip), each against a plain restatement
written here in torch on the CPU: the Matcher in fp32 (bit equality: integer boxes make every area exact and the one division is
correctly rounded on both sides), the two loss kernels against float64 autograd, the gathers against torch indexing (bit equality:
they copy).  The whole-step tests of test_gpu_train.py use one class count, full sampling quotas and tame logits; these do not."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RPN_MATCHER = ([0.3, 0.7], [0, -1, 1], True)
ROI_MATCHER = ([0.5], [0, 1], False)


def _k():
    from lvc_amd import kernels

    return kernels


def _poison(*shapes):
    """Fill blocks of the caching allocator with NaN so that an output element the kernel does not write shows in a dense compare."""
    for s in shapes:
        t = torch.full(s, float("nan"), device=DEV)
        del t


# --------------------------------------------------------------------------------------------------------------- 1. Matcher
def _pairwise_iou(gt, boxes):
    """boxes.py:315-347 in fp32, [G,N]; union = (area1 + area2) - inter."""
    a1 = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    a2 = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    wh = (torch.min(gt[:, None, 2:], boxes[None, :, 2:]) - torch.max(gt[:, None, :2], boxes[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = (a1[:, None] + a2[None, :]) - inter
    return torch.where(inter > 0, inter / union, torch.zeros_like(inter))


def _matcher(gt, boxes, thresholds, labels, low_quality):
    """Matcher.__call__ + set_low_quality_matches_ (matcher.py:61-126) -> (matches int64 [N], labels int8 [N], matched_vals fp32 [N])."""
    N, G = boxes.shape[0], gt.shape[0]
    if G == 0:
        return torch.zeros(N, dtype=torch.int64), torch.full((N,), labels[0], dtype=torch.int8), torch.zeros(N)
    iou = _pairwise_iou(gt, boxes)
    vals = iou.max(dim=0).values
    first = torch.where(iou == vals[None, :], torch.arange(G)[:, None], G).min(dim=0).values       # first arg-max on ties
    thr = [-math.inf] + [float(torch.tensor(t, dtype=torch.float32)) for t in thresholds] + [math.inf]
    lab = torch.full((N,), 127, dtype=torch.int8)
    for l, lo, hi in zip(labels, thr[:-1], thr[1:]):
        lab[(vals >= lo) & (vals < hi)] = l
    if low_quality:
        best_per_gt = iou.max(dim=1).values
        lab[(iou == best_per_gt[:, None]).any(dim=0)] = 1
    return first, lab, vals


def _int_boxes(g, n, zero_area_every=0):
    xy = torch.randint(0, 900, (n, 2), generator=g)
    wh = torch.randint(1, 125, (n, 2), generator=g)
    b = torch.cat([xy, xy + wh], 1).float()
    if zero_area_every:
        b[::zero_area_every, 2] = b[::zero_area_every, 0]
    return b


def _match_inputs(N, G, seed):
    g = torch.Generator().manual_seed(seed)
    gt = _int_boxes(g, G)
    boxes = _int_boxes(g, N, zero_area_every=11 if N > 11 else 0)
    # boxes near ground truth (jittered copies, and exact copies: IoU 1 and ties between boxes), otherwise most IoUs are 0
    pick = torch.randint(0, G, (N,), generator=g)
    near = gt[pick] + torch.randint(-12, 13, (N, 4), generator=g).float()
    near[:, 2:] = torch.max(near[:, 2:], near[:, :2] + 1)
    use = torch.rand(N, generator=g) < 0.6
    boxes[use] = near[use].clamp(0, 1024)
    boxes[torch.rand(N, generator=g) < 0.05] = gt[0]
    # while there are boxes left, every gt box overlaps one: a gt box disjoint from all boxes turns EVERY label into 1 under low-quality
    # matching (pinned in the edge test below), which would leave the thresholds untested.  Even rows: a copy; odd rows: its upper half.
    n = min(N, G)
    boxes[:n] = gt[:n]
    boxes[1:n:2, 3] = gt[1:n:2, 1] + torch.ceil((gt[1:n:2, 3] - gt[1:n:2, 1]) / 2)
    if G >= 2:
        gt[G - 1] = gt[0]                   # two identical ground-truth boxes: the first one wins
    return gt, boxes


@pytest.mark.parametrize("cfg", [RPN_MATCHER, ROI_MATCHER], ids=["rpn", "roi"])
@pytest.mark.parametrize("G", [1, 2, 37, 512])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_match_boxes_equals_the_restated_matcher(N, G, cfg):
    k = _k()
    gt, boxes = _match_inputs(N, G, 1000 * N + G)
    want = _matcher(gt, boxes, *cfg)
    _poison((N,), (N,))
    m, l, v = k.match_boxes(gt.to(DEV), boxes.to(DEV), *cfg)
    assert torch.equal(v.cpu(), want[2])
    assert torch.equal(m.cpu(), want[0])
    assert torch.equal(l.cpu(), want[1])
    if G >= 2:
        assert not bool((m.cpu() == G - 1).any()), "a duplicate of gt 0 may never win the arg-max"


_EDGE_GT = [[0, 0, 10, 10], [0, 0, 10, 10], [100, 100, 120, 130]]
_EDGE_BOXES = [[0, 0, 10, 5],        # IoU 50/100 = the ROI threshold
               [0, 0, 10, 7],        # 70/100: equals fp32(0.7), so it is NOT below the upper RPN threshold
               [0, 0, 10, 3],        # 30/100 = fp32(0.3): not below the lower one
               [0, 0, 10, 10],       # IoU 1 with two identical gt boxes
               [0, 0, 9, 7],         # 63/100, between the thresholds
               [0, 0, 7, 4],         # 28/100, below both
               [5, 5, 5, 9],         # zero area inside a gt box
               [50, 50, 50, 50],     # zero area, a point
               [200, 200, 300, 300],     # disjoint from every gt box
               [100, 100, 110, 130],     # half of gt 2: its best box -> low-quality match
               [10, 10, 20, 20]]         # touches gt 0 in a corner: intersection 0


@pytest.mark.parametrize("with_disjoint_gt", [False, True])
@pytest.mark.parametrize("cfg", [RPN_MATCHER, ROI_MATCHER], ids=["rpn", "roi"])
def test_match_boxes_threshold_ties_zero_area_and_disjoint_ground_truth(cfg, with_disjoint_gt):
    k = _k()
    gt = torch.tensor(_EDGE_GT + ([[500, 500, 600, 600]] if with_disjoint_gt else []), dtype=torch.float32)
    boxes = torch.tensor(_EDGE_BOXES, dtype=torch.float32)
    want = _matcher(gt, boxes, *cfg)
    # the restatement itself, on the rows the case is about
    assert want[2][:6].tolist() == [0.5, float(torch.tensor(0.7, dtype=torch.float32)), float(torch.tensor(0.3, dtype=torch.float32)),
                                    1.0, float(torch.tensor(0.63, dtype=torch.float32)), float(torch.tensor(0.28, dtype=torch.float32))]
    assert want[0][:6].tolist() == [0] * 6 and want[2][6:9].tolist() == [0.0, 0.0, 0.0]
    if cfg is ROI_MATCHER:
        assert want[1].tolist() == [1, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0]
    elif not with_disjoint_gt:
        assert want[1].tolist() == [-1, 1, -1, 1, -1, 0, 0, 0, 0, 1, 0]
    else:
        # the best IoU of the disjoint gt box is 0, so every box with IoU 0 to it -- all of them -- is a low-quality match
        assert want[1].tolist() == [1] * len(_EDGE_BOXES)
    m, l, v = k.match_boxes(gt.to(DEV), boxes.to(DEV), *cfg)
    assert torch.equal(v.cpu(), want[2]) and torch.equal(m.cpu(), want[0]) and torch.equal(l.cpu(), want[1])
    # the batched form on the same rows (one image)
    off = torch.tensor([0, len(gt)], dtype=torch.int32, device=DEV)
    mb, lb, vb = k.match_boxes_batched(gt.to(DEV), off, 1, boxes.to(DEV), None, *cfg, return_vals=True)
    assert torch.equal(vb[0].cpu(), want[2]) and torch.equal(mb[0].cpu().long(), want[0]) and torch.equal(lb[0].cpu(), want[1])


def test_match_boxes_rejects_more_than_512_ground_truth_boxes():
    k = _k()
    from lvc_amd._lib import LvcNativeError

    g = torch.Generator().manual_seed(513)
    with pytest.raises(LvcNativeError, match="512"):
        k.match_boxes(_int_boxes(g, 513).to(DEV), _int_boxes(g, 8).to(DEV), *RPN_MATCHER)
    torch.cuda.synchronize()


@pytest.mark.parametrize("cfg", [RPN_MATCHER, ROI_MATCHER], ids=["rpn", "roi"])
@pytest.mark.parametrize("N", [257, 1000])
def test_match_boxes_batched_equals_the_restated_matcher(N, cfg):
    """B = 3 with ragged ground truth (one image has none): shared boxes, and per-image boxes with fewer rows in use than N.
    Rows at or past an image's count: label -1, match 0.  The image without ground truth: label labels[0], match 0, value 0."""
    k = _k()
    B, counts = 3, (4, 0, 37)
    g = torch.Generator().manual_seed(N)
    gts, per = [], []
    for b, G in enumerate(counts):
        gt, boxes = _match_inputs(N, max(G, 1), 77 * N + b)
        gts.append(gt[:G])
        per.append(boxes)
    gt_all = torch.cat(gts, 0)
    off = [0]
    for G in counts:
        off.append(off[-1] + G)
    gt_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    shared = per[2]
    _poison((B, N), (B, N))
    m, l, v = k.match_boxes_batched(gt_all.to(DEV), gt_off, B, shared.to(DEV), None, *cfg, return_vals=True)
    for b in range(B):
        want = _matcher(gts[b], shared, *cfg)
        assert torch.equal(v[b].cpu(), want[2]) and torch.equal(m[b].cpu().long(), want[0]) and torch.equal(l[b].cpu(), want[1]), b
    nbox = [N, 200, 256]
    stack = torch.stack(per)
    _poison((B, N), (B, N))
    m, l, v = k.match_boxes_batched(gt_all.to(DEV), gt_off, B, stack.to(DEV), torch.tensor(nbox, dtype=torch.int32, device=DEV), *cfg,
                                    return_vals=True)
    for b in range(B):
        nb = nbox[b]
        want = _matcher(gts[b], per[b][:nb], *cfg)
        assert torch.equal(v[b, :nb].cpu(), want[2]) and torch.equal(m[b, :nb].cpu().long(), want[0]), b
        assert torch.equal(l[b, :nb].cpu(), want[1]), b
        assert bool((l[b, nb:] == -1).all()) and bool((m[b, nb:] == 0).all()), b
    assert bool((l[1, :nbox[1]] == cfg[1][0]).all()) and bool((m[1] == 0).all()) and bool((v[1, :nbox[1]] == 0).all())


# --------------------------------------------------------------------------------------------------------------- 2. Fast R-CNN losses
def _get_deltas(src, tgt, weights):
    """box_regression.py:40-71 in the dtype of its inputs."""
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    scx, scy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tcx, tcy = tgt[:, 0] + 0.5 * tw, tgt[:, 1] + 0.5 * th
    wx, wy, ww, wh = weights
    return torch.stack([wx * (tcx - scx) / sw, wy * (tcy - scy) / sh, ww * torch.log(tw / sw), wh * torch.log(th / sh)], 1)


def _smooth_l1_sum(x, t, beta):
    """fvcore smooth_l1_loss, reduction "sum"."""
    n = (x - t).abs()
    if beta < 1e-5:
        return n.sum()
    return torch.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta).sum()


def _f32(v):
    """The double that equals fp32(v): the kernels take beta and the weights as floats."""
    return float(torch.tensor(v, dtype=torch.float32))


def _frcnn_reference(logits, deltas, proposals, gt_boxes, cls, K, weights, beta):
    lg = logits.double().requires_grad_(True)
    dl = deltas.double().requires_grad_(True)
    R = lg.shape[0]
    loss_cls = F.cross_entropy(lg, cls, reduction="mean")
    fg = ((cls >= 0) & (cls < K)).nonzero().view(-1)
    t = _get_deltas(proposals[fg].double(), gt_boxes[fg].double(), weights)
    cols = torch.arange(4)[None, :] + (0 if dl.shape[1] == 4 else 4 * cls[fg][:, None])
    loss_box = _smooth_l1_sum(dl[fg[:, None], cols], t, _f32(beta)) / R
    (loss_cls + loss_box).backward()
    return float(loss_cls), float(loss_box), lg.grad, dl.grad


def _frcnn_inputs(R, K, agnostic, fg_mode, beta, seed):
    """Random rows plus, where R allows, the rows the issue names: |x - t| == beta exactly, x == t exactly (both with targets that
    are exact in fp32 AND fp64: power-of-two proposal sizes, integer shifts, equal sizes -> t = (w * shift / size, ..., 0, 0)), a row
    whose logits span +-80 with the target at the bottom, and a row of equal logits."""
    g = torch.Generator().manual_seed(seed)
    weights = (10.0, 10.0, 5.0, 5.0)
    nreg = 4 if agnostic else 4 * K
    logits = torch.randn(R, K + 1, generator=g) * 3
    if fg_mode == "none":
        cls = torch.full((R,), K, dtype=torch.int64)
    elif fg_mode == "all":
        cls = torch.randint(0, K, (R,), generator=g)
    else:
        cls = torch.randint(0, K + 1, (R,), generator=g)
    xy = torch.rand(R, 2, generator=g) * 500
    proposals = torch.cat([xy, xy + 8 + torch.rand(R, 2, generator=g) * 200], 1)
    pw = (proposals[:, 2:] - proposals[:, :2])
    gxy = proposals[:, :2] + (torch.rand(R, 2, generator=g) - 0.5) * 0.3 * pw
    gt_boxes = torch.cat([gxy, gxy + pw * torch.exp((torch.rand(R, 2, generator=g) - 0.5) * 0.8)], 1)
    deltas = torch.randn(R, nreg, generator=g) * 0.5
    special = {}
    if fg_mode != "none" and R >= 5:
        for r, (size, shift) in zip((1, 2), ((64.0, 0.0), (32.0, 4.0))):
            proposals[r] = torch.tensor([16.0, 32.0, 16.0 + size, 32.0 + size])
            gt_boxes[r] = proposals[r] + shift
            cls[r] = (r * 7) % K
            special[r] = torch.tensor([10.0 * shift / size, 10.0 * shift / size, 0.0, 0.0])
    if R >= 5:
        row = torch.linspace(-80.0, 80.0, K + 1)[torch.randperm(K + 1, generator=g)]
        j, c = int(row.argmin()), int(cls[3])
        row[j], row[c] = float(row[c]), -80.0           # the target at the bottom: its exp(-160) must not cost the loss its lse - x_c
        logits[3] = row
        logits[4] = 1.25
    t32 = _get_deltas(proposals, gt_boxes, weights)            # fp32, the kernel's operation order
    fgrows = ((cls >= 0) & (cls < K)).nonzero().view(-1)
    # near targets on the foreground rows so that both smooth-L1 branches are taken
    for r in fgrows.tolist():
        c0 = 0 if agnostic else 4 * int(cls[r])
        deltas[r, c0:c0 + 4] = t32[r] + torch.randn(4, generator=g) * max(2.0 * beta, 0.05)
    b32 = torch.tensor(beta, dtype=torch.float32)
    for r, t in special.items():
        assert torch.equal(t32[r], t), "the special rows' targets must be exact in fp32"
        c0 = 0 if agnostic else 4 * int(cls[r])
        if r == 1:      # t == 0: x = +-beta exactly, and one x == t
            deltas[r, c0:c0 + 4] = torch.stack([b32, -b32, torch.tensor(0.0), b32])
        else:           # x == t on a non-zero target, and |x - t| about beta
            deltas[r, c0:c0 + 4] = torch.stack([t[0], t[1] + b32, t[2], t[3] - b32])
    return logits, deltas, proposals, gt_boxes, cls, weights


def _check_frcnn(R, K, agnostic, fg_mode, beta, seed):
    k = _k()
    logits, deltas, proposals, gt_boxes, cls, weights = _frcnn_inputs(R, K, agnostic, fg_mode, beta, seed)
    assert int(cls.min()) >= 0 and int(cls.max()) <= K          # the wrapper's contract
    lc, lb, gl, gd = _frcnn_reference(logits, deltas, proposals, gt_boxes, cls, K, weights, beta)
    nreg = deltas.shape[1]
    # the layout of the fused predictor GEMM: logits | deltas side by side in one wider row, with columns to spare
    wide = torch.full((R, (K + 1) + 3 + nreg + 5), 1e30)
    wide[:, :K + 1] = logits
    wide[:, K + 4:K + 4 + nreg] = deltas
    wide = wide.to(DEV)
    args = (proposals.to(DEV), gt_boxes.to(DEV), cls.to(DEV), K, weights, beta)
    res = []
    for lg_d, dl_d in ((logits.to(DEV), deltas.to(DEV)), (wide[:, :K + 1], wide[:, K + 4:K + 4 + nreg])):
        _poison((R, K + 1), (R, nreg))
        out, dlg, ddl = k.fast_rcnn_losses(lg_d, dl_d, *args)
        res.append((out.cpu(), dlg.cpu(), ddl.cpu()))
    (out, dlg, ddl), sliced = res
    assert all(torch.equal(a, b) for a, b in zip(res[0], sliced)), "row pitch changes the result"
    assert dlg.shape == (R, K + 1) and ddl.shape == (R, nreg)
    e_cls, e_box = abs(float(out[0]) - lc), abs(float(out[1]) - lb)
    e_gl = float((dlg.double() - gl).abs().max()) / float(gl.abs().max())
    gmax = float(gd.abs().max())
    e_gd = float((ddl.double() - gd).abs().max()) / gmax if gmax > 0 else float(ddl.abs().max())
    print("fast_rcnn_losses R=%d K=%d agnostic=%d fg=%s beta=%g: loss_cls %.3e/%.1e loss_box %.3e/%.1e dlogits %.2e ddeltas %.2e (of 1e-5)"
          % (R, K, agnostic, fg_mode, beta, e_cls, 1e-5 * max(1.0, abs(lc)), e_box, 1e-5 * max(1.0, abs(lb)), e_gl, e_gd))
    assert torch.isfinite(out).all() and torch.isfinite(dlg).all() and torch.isfinite(ddl).all()
    assert e_cls <= 1e-5 * max(1.0, abs(lc))
    assert e_box <= 1e-5 * max(1.0, abs(lb))
    assert e_gl <= 1e-5
    if gmax > 0:
        assert e_gd <= 1e-5
    else:
        assert float(out[1]) == 0.0 and not bool(ddl.ne(0).any()), "no foreground row: loss_box_reg 0, ddeltas all zero"


_KS = [1, 20, 62, 63, 64, 80, 200]
_RS = [1, 3, 4, 5, 1023, 1025, 2049]
_BETAS = [0.0, 1e-6, 1.0 / 9, 1.0]


@pytest.mark.parametrize("K", _KS)
@pytest.mark.parametrize("R", _RS)
def test_fast_rcnn_losses_equal_fp64_autograd(R, K):
    """Every class count against every row count; regression layout and beta rotate so that each value meets each R and each K."""
    i = _RS.index(R) + _KS.index(K)
    _check_frcnn(R, K, agnostic=bool(i % 2), fg_mode="mixed", beta=_BETAS[(i // 2) % 4], seed=31 * R + K)


@pytest.mark.parametrize("agnostic", [False, True], ids=["per_class", "agnostic"])
@pytest.mark.parametrize("beta", _BETAS)
@pytest.mark.parametrize("fg_mode", ["mixed", "none", "all"])
def test_fast_rcnn_losses_betas_and_foreground_extremes(fg_mode, beta, agnostic):
    _check_frcnn(1025, 63, agnostic, fg_mode, beta, seed=7)
    _check_frcnn(5, 20, agnostic, fg_mode, beta, seed=8)


# --------------------------------------------------------------------------------------------------------------- 3. RPN losses
def _rpn_reference(logits, deltas, anchors, gt_boxes, labels, beta, normalizer):
    lg = logits.double().requires_grad_(True)
    dl = deltas.double().requires_grad_(True)
    valid = (labels >= 0).nonzero().view(-1)
    pos = (labels == 1).nonzero().view(-1)
    loss_cls = F.binary_cross_entropy_with_logits(lg[valid], (labels[valid] == 1).double(), reduction="sum") / normalizer
    t = _get_deltas(anchors[pos].double(), gt_boxes[pos].double(), (1.0, 1.0, 1.0, 1.0))
    loss_loc = _smooth_l1_sum(dl[pos], t, _f32(beta)) / normalizer
    (loss_cls + loss_loc).backward()
    return float(loss_cls), float(loss_loc), lg.grad, dl.grad


def _rpn_inputs(S, layout, beta, seed, bs=256):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(S, generator=g) * 30).clamp(-90, 90)
    logits[::17] = 90.0
    logits[5::17] = -90.0
    labels = (torch.rand(S, generator=g) < 0.4).to(torch.int8)
    if layout == "tail":            # as lvc_rpn_gather_sampled writes them: behind the sampled anchors of each image's block
        for s0 in range(0, S, bs):
            n = min(bs, S - s0)
            cut = s0 + int(torch.randint(n // 2, n + 1, (1,), generator=g)) if s0 else s0 + n // 2
            labels[cut:s0 + n] = -1
    elif layout == "mixed":
        labels[torch.rand(S, generator=g) < 0.3] = -1
    xy = torch.rand(S, 2, generator=g) * 400
    anchors = torch.cat([xy, xy + 16 + torch.rand(S, 2, generator=g) * 200], 1)
    aw = anchors[:, 2:] - anchors[:, :2]
    gxy = anchors[:, :2] + (torch.rand(S, 2, generator=g) - 0.5) * 0.5 * aw
    gt_boxes = torch.cat([gxy, gxy + aw * torch.exp((torch.rand(S, 2, generator=g) - 0.5))], 1)
    deltas = _get_deltas(anchors, gt_boxes, (1.0, 1.0, 1.0, 1.0)) + torch.randn(S, 4, generator=g) * max(2.0 * beta, 0.05)
    pad = labels < 0
    if layout == "tail":            # the gather's padding rows
        logits[pad] = 0.0
        deltas[pad] = 0.0
        anchors[pad] = torch.tensor([0.0, 0.0, 1.0, 1.0])
        gt_boxes[pad] = torch.tensor([0.0, 0.0, 1.0, 1.0])
    return logits, deltas, anchors, gt_boxes, labels


@pytest.mark.parametrize("beta", [0.0, 1.0 / 9])
@pytest.mark.parametrize("layout", ["no_padding", "tail", "mixed"])
@pytest.mark.parametrize("S", [1, 63, 1024, 1025, 2560])
def test_rpn_losses_equal_fp64_autograd(S, layout, beta):
    """Rows with label -1 (the padding of an image that sampled fewer anchors than its quota) add nothing to either loss and have
    a zero gradient.  rpn_losses_kernel used to take them as y = -1: a padding row of logit 0 then adds log 2 / normalizer to
    loss_rpn_cls (by that formula, S = 2560 "tail": 783 rows, +0.21 on a loss of 11.1 against a bound of 1.1e-4) and has the gradient
    (sigmoid(0) + 1) / normalizer, 1.5 x the largest true one.  The "no_padding" layout is the same before and after."""
    k = _k()
    normalizer = 256.0 * max(1, -(-S // 256))
    ins = _rpn_inputs(S, layout, beta, 13 * S + 1)
    assert layout == "no_padding" or S == 1 or bool((ins[4] < 0).any())
    lc, ll, gl, gd = _rpn_reference(*ins, beta, normalizer)
    dev = [t.to(DEV) for t in ins]
    out = k.rpn_losses(*dev, beta, normalizer).cpu()
    _poison((S,), (S, 4))
    out_g, dlg, ddl = [t.cpu() for t in k.rpn_losses(*dev, beta, normalizer, with_grad=True)]
    assert torch.equal(out, out_g), "lvc_rpn_losses and lvc_rpn_losses_grad must give the same losses bit for bit"
    e_cls, e_loc = abs(float(out[0]) - lc), abs(float(out[1]) - ll)
    glmax, gdmax = float(gl.abs().max()), float(gd.abs().max())
    e_gl = float((dlg.double() - gl).abs().max()) / glmax if glmax > 0 else float(dlg.abs().max())
    e_gd = float((ddl.double() - gd).abs().max()) / gdmax if gdmax > 0 else float(ddl.abs().max())
    print("rpn_losses S=%d %s beta=%g: loss_cls %.3e/%.1e loss_loc %.3e/%.1e dlogits %.2e ddeltas %.2e (of 1e-5)"
          % (S, layout, beta, e_cls, 1e-5 * max(1.0, abs(lc)), e_loc, 1e-5 * max(1.0, abs(ll)), e_gl, e_gd))
    assert torch.isfinite(out).all() and torch.isfinite(dlg).all() and torch.isfinite(ddl).all()
    assert e_cls <= 1e-5 * max(1.0, abs(lc))
    assert e_loc <= 1e-5 * max(1.0, abs(ll))
    assert e_gl <= (1e-5 if glmax > 0 else 0.0)
    assert e_gd <= (1e-5 if gdmax > 0 else 0.0)
    ignored = ins[4] < 0
    assert not bool(dlg[ignored].ne(0).any()) and not bool(ddl[ignored].ne(0).any()), "ignored rows have a zero gradient"


def test_rpn_losses_of_no_rows_are_zero():
    k = _k()
    e = torch.zeros(0, device=DEV)
    out = k.rpn_losses(e, e.view(0, 4), e.view(0, 4), e.view(0, 4), torch.zeros(0, dtype=torch.int8, device=DEV), 1.0 / 9, 512.0)
    assert out.cpu().tolist() == [0.0, 0.0]


# --------------------------------------------------------------------------------------------------------------- 4. RPN gather
def test_rpn_gather_sampled_equals_torch_indexing():
    """Reference built as the trainable branch of RPN._losses_batched builds its rows: flat logits / deltas by cat over the levels,
    anchors from the anchor generator, gt rows by gt_off[b] + matches[b, r].  Every output is a copy or one fp32 add: bit equality."""
    k = _k()
    from lvc_amd.modeling.anchor_generator import DefaultAnchorGenerator

    g = torch.Generator().manual_seed(4)
    A, B, bs = 3, 3, 16
    shapes, pitches, strides = [(5, 7), (3, 4), (1, 2)], [15, 16, 32], [4, 8, 16]
    ag = DefaultAnchorGenerator(sizes=[[32], [64], [128]], aspect_ratios=[[0.5, 1.0, 2.0]], strides=strides, offset=0.0)
    fused = [torch.randn(B, h, w, ld, generator=g) for (h, w), ld in zip(shapes, pitches)]
    flat_logits = torch.cat([f[..., :A].reshape(B, -1) for f in fused], 1)
    flat_deltas = torch.cat([f[..., A:5 * A].reshape(B, -1, 4) for f in fused], 1)
    anchors = torch.cat(ag._grid_anchors(shapes), 0)
    R = anchors.shape[0]
    first = [0, 105, 141]
    last = [104, 140, 146]
    assert R == 147 and flat_logits.shape == (B, R)
    gcount = [3, 2, 0]
    gt = torch.rand(5, 4, generator=g) * 100
    gt_off = torch.tensor([0, 3, 5, 5], dtype=torch.int32)
    matches = torch.stack([torch.randint(0, max(n, 1), (R,), generator=g) for n in gcount]).to(torch.int32)
    sel = torch.full((B, bs), -1, dtype=torch.int32)
    sel[0] = torch.tensor(first + last + [7, 50, 99, 106, 120, 139, 142, 143, 144, 145])          # a full image
    sel[1, :8] = torch.tensor([146, 0, 104, 33, 105, 141, 2, 140])                                # fewer than bs: -1 in the tail
    sel[2, :7] = torch.tensor([141, 3, 104, 0, 146, 105, 60])                                     # no ground truth, no positives
    counts = torch.tensor([[6, 10], [3, 5], [0, 7]], dtype=torch.int32)
    want_lg = torch.zeros(B, bs)
    want_dl = torch.zeros(B, bs, 4)
    want_an = torch.tensor([0.0, 0.0, 1.0, 1.0]).repeat(B, bs, 1)
    want_gt = want_an.clone()
    want_lab = torch.full((B, bs), -1, dtype=torch.int8)
    for b in range(B):
        n = int(counts[b].sum())
        idx = sel[b, :n].long()
        want_lg[b, :n] = flat_logits[b, idx]
        want_dl[b, :n] = flat_deltas[b, idx]
        want_an[b, :n] = anchors[idx]
        npos = int(counts[b, 0])
        want_gt[b, :npos] = gt[int(gt_off[b]) + matches[b, idx[:npos]].long()]
        want_lab[b, :npos] = 1
        want_lab[b, npos:n] = 0
    S = B * bs
    _poison((S,), (S, 4), (S, 4), (S, 4))
    lg, dl, an, gtb, lab = k.rpn_gather_sampled([f.to(DEV) for f in fused], A, [c.to(DEV) for c in ag.cell_anchors], strides, sel.to(DEV),
                                                counts.to(DEV), matches.to(DEV), gt.to(DEV), gt_off.to(DEV))
    assert torch.equal(lab.cpu(), want_lab.view(-1))
    assert torch.equal(lg.cpu(), want_lg.view(-1))
    assert torch.equal(dl.cpu(), want_dl.view(-1, 4))
    assert torch.equal(an.cpu(), want_an.view(-1, 4))
    assert torch.equal(gtb.cpu(), want_gt.view(-1, 4))


# --------------------------------------------------------------------------------------------------------------- 5. ROI table / gather
def _roi_table_case(g):
    B, P, Wt = 3, 10, 16
    pcount = [0, 7, 13]                 # 13 > P: clamps to P
    gcount = [1, 4, 2]
    pboxes = torch.rand(B, P, 4, generator=g) * 300
    plogits = torch.randn(B, P, generator=g)
    gt = torch.rand(sum(gcount), 4, generator=g) * 300
    off = [0, 1, 5, 7]
    gt_logit = math.log((1.0 - 1e-10) / 1e-10)
    boxes = torch.zeros(B, Wt, 4)
    logits = torch.zeros(B, Wt)
    nrow = []
    for b in range(B):
        n = min(pcount[b], P)
        boxes[b, :n] = pboxes[b, :n]
        logits[b, :n] = plogits[b, :n]
        boxes[b, n:n + gcount[b]] = gt[off[b]:off[b + 1]]
        logits[b, n:n + gcount[b]] = gt_logit               # the fp32 value of it
        nrow.append(n + gcount[b])
    return (pboxes, plogits, torch.tensor(pcount, dtype=torch.int32), gt, torch.tensor(off, dtype=torch.int32), gt_logit, Wt), \
        (boxes, logits, torch.tensor(nrow, dtype=torch.int32)), gcount


def test_roi_build_table_equals_the_restatement():
    k = _k()
    (pb, pl, pc, gt, off, gl, Wt), want, _ = _roi_table_case(torch.Generator().manual_seed(51))
    _poison((3, Wt, 4), (3, Wt))
    boxes, logits, nrow = k.roi_build_table(pb.to(DEV), pl.to(DEV), pc.to(DEV), gt.to(DEV), off.to(DEV), gl, Wt)
    assert nrow.cpu().tolist() == want[2].tolist() == [1, 11, 12]
    assert torch.equal(boxes.cpu(), want[0])
    assert torch.equal(logits.cpu(), want[1])


@pytest.mark.parametrize("K", [1, 60])
def test_roi_gather_sampled_equals_the_restatement(K):
    k = _k()
    g = torch.Generator().manual_seed(52 + K)
    _, (boxes, logits, nrow), gcount = _roi_table_case(g)
    B, Wt, bs = 3, boxes.shape[1], 8
    off = [0, 1, 5, 7]
    gt_classes = torch.randint(0, K, (7,), generator=g)
    matches = torch.stack([torch.randint(0, n, (Wt,), generator=g) for n in gcount]).to(torch.int32)
    sel = torch.full((B, bs), -1, dtype=torch.int32)
    sel[0, :1] = torch.tensor([0])                                  # one row in the table: one sample
    sel[1] = torch.tensor([10, 7, 0, 3, 9, 1, 8, 2])                # full: 3 foreground, 5 background
    sel[2, :5] = torch.tensor([11, 10, 4, 0, 9])                    # short: 2 + 3
    counts = torch.tensor([[1, 0], [3, 5], [2, 3]], dtype=torch.int32)
    w_box = torch.zeros(B, bs, 4)
    w_lg = torch.zeros(B, bs)
    w_cls = torch.full((B, bs), K, dtype=torch.int64)
    w_m = torch.zeros(B, bs, dtype=torch.int64)
    for b in range(B):
        n, npos = int(counts[b].sum()), int(counts[b, 0])
        idx = sel[b, :n].long()
        assert int(idx.max()) < int(nrow[b])
        w_box[b, :n] = boxes[b, idx]
        w_lg[b, :n] = logits[b, idx]
        w_m[b, :n] = matches[b, idx].long()
        w_cls[b, :npos] = gt_classes[off[b] + w_m[b, :npos]]
    _poison((B, bs, 4), (B, bs), (B, bs), (B, bs))
    sb, sl, sc, sm = k.roi_gather_sampled(boxes.to(DEV), logits.to(DEV), matches.to(DEV), sel.to(DEV), counts.to(DEV), gt_classes.to(DEV),
                                          torch.tensor(off, dtype=torch.int32, device=DEV), K)
    assert torch.equal(sb.cpu(), w_box) and torch.equal(sl.cpu(), w_lg)
    assert torch.equal(sc.cpu(), w_cls), "foreground rows: the matched gt's class; background and padding rows: K"
    assert torch.equal(sm.cpu(), w_m)
