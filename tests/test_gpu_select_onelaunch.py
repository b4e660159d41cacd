"""lvc_rpn_proposals with the per-level top-k in its short forms (csrc/boxes.hip) against the multi-launch selection they replace
(kernels.set_select_onelaunch(0): five radix phases + two finishing kernels) and against the oracle.  Mode 3 (the default): one wide
launch writes the keys and their top-digit histogram, one workgroup per (image, level) does the rest (rpn_topk_one_kernel); mode 7:
that workgroup does everything, ONE launch.  All paths define the selected set and its order by (key, index) alone, so boxes, logits
and counts must be EQUAL, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu
D = "cuda:0"
A = 3
SMALL = [(7, 9), (13, 5), (1, 1)]          # 189, 195 and 3 anchors per image: the last is smaller than one radix bucket
SMALL_SIZES = [(30, 38), (26, 33)]
LARGE = [(64, 96), (7, 9)]                 # 18 432 anchors: more than one trip of eight loads per thread, and the old path's slices
LARGE_SIZES = [(256, 380), (250, 384)]


def _logits(mode, shapes, pre, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in shapes:
        n = h * w * A
        lg = torch.randn(2, n, generator=g) * 2
        if mode == "constant":
            lg[:] = 0.75
        elif mode == "cut":        # exactly pre + 3 equal values on top of everything else: the cut falls inside the tie
            if n >= pre + 3:
                for b in range(2):
                    pos = torch.randperm(n, generator=g)[: pre + 3]
                    lg[b, pos] = float(lg[b].max()) + 1.0
        elif mode == "special":    # +-inf, -0.0 / +0.0 (equal keys), ties among them
            lg[:, ::5] = 0.0
            lg[:, 1::7] = -0.0
            lg[:, 2::11] = float("inf")
            lg[:, 3::13] = float("-inf")
        elif mode == "ties":
            lg[:, ::5] = lg[:, :1]
        out.append(lg)
    return out


def _run(shapes, sizes, logits, pre, post, seed):
    from lvc_amd import kernels as k
    from oracle import rcnn as orc

    g = torch.Generator().manual_seed(1000 + seed)
    deltas = [torch.randn(2, h * w * A, 4, generator=g) * 0.5 for h, w in shapes]
    strides = [4, 8, 16][: len(shapes)]
    cell = [orc.generate_cell_anchors((s,), (0.5, 1.0, 2.0)) for s in (32, 64, 128)[: len(shapes)]]
    fused = [torch.cat([lg.view(2, h, w, A), dl.view(2, h, w, A * 4)], dim=3).contiguous().to(D)
             for lg, dl, (h, w) in zip(logits, deltas, shapes)]
    isz = torch.tensor(sizes, dtype=torch.int32, device=D)
    res = {}
    for mode in (0, 3, 7):
        k.set_select_onelaunch(mode)
        try:
            b, l, c = k.rpn_proposals([f[..., :A] for f in fused], [f[..., A:] for f in fused], [c.to(D) for c in cell], strides, isz,
                                      pre, post, 0.7)
            res[mode] = (b.cpu(), l.cpu(), c.cpu())
        finally:
            k.set_select_onelaunch(3)
    old = res[0]
    for mode in (3, 7):
        new = res[mode]
        assert torch.equal(new[2], old[2]), mode
        assert torch.equal(new[1], old[1]), mode
        assert torch.equal(new[0], old[0]), mode
    return res[3], (cell, strides, deltas)


@pytest.mark.parametrize("pre", [50, 189, 195, 1000])
@pytest.mark.parametrize("mode", ["random", "ties", "constant", "cut", "special"])
def test_one_launch_topk_equals_the_multi_launch_form_small_levels(mode, pre):
    """B = 2, levels of 7x9, 13x5 and 1x1 cells: pre_nms_topk below, equal to and above the levels' anchor counts; constant logits (the
    tie-break alone), pre + 3 values tied across the cut, +-inf and -0.0 keys."""
    from oracle import rcnn as orc

    logits = _logits(mode, SMALL, pre, 7 * pre)
    (boxes, olog, count), (cell, strides, deltas) = _run(SMALL, SMALL_SIZES, logits, pre, 300, pre)
    if mode == "special":
        return      # the oracle's sort is not defined on the non-finite rows the device drops; old == new is the check here
    ref = orc.find_top_rpn_proposals(orc.grid_anchors(cell, SMALL, strides), logits, deltas, SMALL_SIZES, 0.7, pre, 300)
    for n in range(2):
        rb, rl = ref[n]
        assert int(count[n]) == len(rb)
        assert torch.equal(olog[n, : len(rl)], rl)
        assert (boxes[n, : len(rb)] - rb).abs().max() <= 1e-4


@pytest.mark.parametrize("mode", ["random", "constant", "cut", "special"])
def test_one_launch_topk_equals_the_multi_launch_form_64x96(mode):
    from oracle import rcnn as orc

    pre = 1000
    logits = _logits(mode, LARGE, pre, 5)
    (boxes, olog, count), (cell, strides, deltas) = _run(LARGE, LARGE_SIZES, logits, pre, 1000, 5)
    if mode == "special":
        return
    ref = orc.find_top_rpn_proposals(orc.grid_anchors(cell, LARGE, strides), logits, deltas, LARGE_SIZES, 0.7, pre, 1000)
    for n in range(2):
        rb, rl = ref[n]
        assert int(count[n]) == len(rb)
        assert torch.equal(olog[n, : len(rl)], rl)
        assert (boxes[n, : len(rb)] - rb).abs().max() <= 1e-4
