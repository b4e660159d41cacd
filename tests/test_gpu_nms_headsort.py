"""lvc_batched_nms, head-block form (Nmax > 2048, max_keep << Nmax): the default path orders only the head rows (radix select + sort of
the head, csrc/nms.hip: nms_prep_head_kernel) and sorts rows [head, n) on the device only for an image whose head block did not yield
max_keep boxes (nms_tail_sort_kernel).  kernels.set_select_onelaunch(0) keeps the full sort it replaces.  Keep lists and counts must
be EQUAL between the two, and equal to the oracle's.  (`keep` rows past num_keep are not written by either path and are not compared.)

With max_keep = 8 the head is the form's minimum of 1024 rows (csrc/nms.hip: head = max(1024, 8 * max_keep rounded up to 64))."""
import pytest
import torch

pytestmark = pytest.mark.gpu
D = "cuda:0"
HEAD = 1024


def _boxes(g, n, jitter, nbase):
    base = torch.rand(nbase, 2, generator=g) * torch.tensor([1200.0, 700.0])
    wh = 8 + torch.rand(nbase, 2, generator=g) * 250
    base = torch.cat([base, base + wh], dim=1)
    b = base[torch.randint(0, nbase, (n,), generator=g)] + torch.randn(n, 4, generator=g) * jitter
    b[:, 2:] = torch.max(b[:, 2:], b[:, :2] + 0.5)
    return b


def _tie_across(scores, n, row, width):
    """the scores of sorted rows [row - width, row + width) made equal: a tie that straddles `row`"""
    if n >= row + width:
        order = torch.argsort(scores[:n], descending=True, stable=True)
        scores[order[row - width: row + width]] = float(scores[order[row - width]])


def _case(Nmax, with_idxs, seed):
    g = torch.Generator().manual_seed(seed)
    counts = torch.tensor([Nmax, Nmax, 0, 1, HEAD + 1 if Nmax > HEAD else 5], dtype=torch.int32)
    B = len(counts)
    boxes = torch.zeros(B, Nmax, 4)
    scores = torch.zeros(B, Nmax)
    idxs = torch.zeros(B, Nmax, dtype=torch.int32)
    for b in range(B):
        n = int(counts[b])
        if b == 1:
            # (b) five clusters of near-identical boxes take every high score: fewer than 8 survive among the first 1024 rows, and the
            # scattered boxes with the lowest scores (the unsorted tail) have to complete the list
            bb = _boxes(g, Nmax, 0.01, 5)
            ss = torch.rand(Nmax, generator=g) + 1.0
            lone = torch.randperm(Nmax, generator=g)[:600]
            bb[lone] = _boxes(g, 600, 4.0, 200)
            ss[lone] = torch.rand(600, generator=g)
            ii = torch.zeros(Nmax, dtype=torch.int32)
        else:
            # (a) scattered boxes: the list is complete inside the head
            bb = _boxes(g, Nmax, 4.0, max(4, Nmax // 6))
            ss = torch.randn(Nmax, generator=g)
            ii = torch.randint(0, 4, (Nmax,), generator=g).int()
        ss[::9] = ss[4]
        _tie_across(ss, n, HEAD, 20)
        if b == 1:
            _tie_across(ss, n, 3000, 20)       # and a tie inside the tail
        boxes[b], scores[b], idxs[b] = bb, ss, ii
    return boxes, scores, (idxs if with_idxs else None), counts


def _check(Nmax, with_idxs, max_keep, thr, seed):
    from lvc_amd import kernels as k
    from oracle import ops as oops

    boxes, scores, idxs, counts = _case(Nmax, with_idxs, seed)
    res = {}
    for mode in (0, 3):
        k.set_select_onelaunch(mode)
        try:
            keep, nk = k.batched_nms_batch(boxes.to(D), scores.to(D), idxs.to(D) if with_idxs else None, counts.to(D), thr,
                                           max_keep=max_keep)
            res[mode] = (keep.cpu(), nk.cpu())
        finally:
            k.set_select_onelaunch(3)
    assert torch.equal(res[3][1], res[0][1])
    kept = []
    for b in range(len(counts)):
        n, m = int(counts[b]), int(res[3][1][b])
        assert torch.equal(res[3][0][b, :m], res[0][0][b, :m]), b
        ref = oops.batched_nms(boxes[b, :n], scores[b, :n], idxs[b, :n].long() if with_idxs else torch.zeros(n, dtype=torch.int64), thr)
        ref = ref[:max_keep]
        assert m == len(ref), (b, m, len(ref))
        assert res[3][0][b, :m].tolist() == ref.tolist(), b
        order = torch.argsort(scores[b, :n], descending=True, stable=True)
        rank = {int(i): r for r, i in enumerate(order.tolist())}
        kept.append([rank[int(i)] for i in ref.tolist()])
    return kept


@pytest.mark.parametrize("with_idxs", [True, False])
def test_head_only_sort_equals_the_full_sort(with_idxs):
    """Nmax = 4096, max_keep = 8: image 0 finishes inside the head, image 1 needs the tail, counts of 0, 1 and head + 1 (a tail of one
    row); score ties straddle row `head` in every full image."""
    kept = _check(4096, with_idxs, 8, 0.5, 11)
    assert max(kept[0]) < HEAD                    # (a) really ends in the head
    assert max(kept[1]) >= HEAD and sum(r < HEAD for r in kept[1]) < 8      # (b) really needs the tail


def test_one_block_form_is_untouched():
    """Nmax <= NMS_HEAD_MIN: no head block, one sort, either setting."""
    _check(2048, True, 8, 0.5, 12)
