"""lvc_keypoint_targets (csrc/keypoint_targets.hip) against tests/keypoint_train_ref.py and the reference's recorded targets: the integer
outputs are compared exactly."""
import pytest
import torch

import keypoint_train_ref as R
from helpers import gold

pytestmark = pytest.mark.gpu

SIDE = 56


def _dev():
    return torch.device("cuda:0")


def _table(seed, R_, K):
    """B = 3 images (the second without foreground rows), R_ rows each, counts below R_: seeded boxes at fractional corners and
    `synthetic_gt_keypoints` on the ground-truth boxes (edge points, points just outside, v in {0, 1, 2}, bare instances); rows are
    the ground-truth boxes themselves (on-edge keypoints meet the clamp), jittered copies, and one box of zero width."""
    from lvc_amd.utils import synthetic as syn

    g = torch.Generator().manual_seed(seed)
    B, n = 3, (5, 3, 4)
    counts = torch.tensor([R_ - 3, 0, min(R_, 7)], dtype=torch.int32)
    boxes = torch.zeros(B, R_, 4)
    matched = torch.zeros(B, R_, dtype=torch.int64)
    kps = []
    for b in range(B):
        xy = torch.rand(n[b], 2, generator=g) * 100
        wh = 8 + torch.rand(n[b], 2, generator=g) * 90
        gt = torch.cat([xy, xy + wh], 1)
        kps.append(syn.synthetic_gt_keypoints(gt, K, seed=seed + b))
        m = torch.randint(0, n[b], (R_,), generator=g)
        jit = (torch.rand(R_, 4, generator=g) - 0.5) * 6
        jit[:: 3] = 0          # every third row is its ground-truth box, bit for bit
        boxes[b] = gt[m] + jit
        matched[b] = m
    boxes[0, 1, 2] = boxes[0, 1, 0]          # a real row of zero width
    boxes[2, 2, 3] = boxes[2, 2, 1] - 1.0    # ... and one of negative height
    boxes[:, -2:] = float("nan")             # rows past every count hold NaN boxes and an index out of range
    matched[:, -2:] = 1 << 40
    return boxes, matched, counts, kps


def _check(boxes, matched, counts, kps, apply_selection=True):
    from lvc_amd import kernels as K

    dev = _dev()
    got = K.keypoint_targets(boxes.to(dev), matched.to(dev), counts.to(dev), [k.to(dev) for k in kps], SIDE, apply_selection=apply_selection)
    want = R.table_targets(boxes, matched, counts, kps, SIDE)
    names = ("target", "valid", "selected", "sel_count")
    for name, a, b in zip(names, got, want):
        if not apply_selection and name in ("target", "valid"):
            continue
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b), name
    return [t.cpu() for t in got], want


@pytest.mark.parametrize("R_,K", [(300, 17), (9, 8)])
def test_targets_are_the_restatements(R_, K):
    """R_ = 300 crosses the workgroup's 256-row stride; every case of the docstring of `_table` is present."""
    boxes, matched, counts, kps = _table(11 + R_, R_, K)
    got, want = _check(boxes, matched, counts, kps)
    target, valid, selected, sel = got
    B = 3
    assert int(sel[1]) == 0 and not bool(valid[R_: 2 * R_].any())
    for b in range(B):      # rows past the count: untouched zeros
        c = int(counts[b])
        assert not bool(target[b * R_ + c: (b + 1) * R_].any()) and not bool(selected[b * R_ + c: (b + 1) * R_].any())
    c0 = int(counts[0])
    kp0 = kps[0][matched[0, :c0]]
    own = (boxes[0, :c0, None, :] == torch.cat([kps[0][:, 0, 0:1], kps[0][:, 1, 1:2], kps[0][:, 2, 0:1], kps[0][:, 3, 1:2]], 1)[None]).all(2).any(1)
    assert bool(own.any())
    v = valid[:c0].bool()
    # on a row that is its ground-truth box: the points on the four edges are valid, x == x2 and y == y2 through the clamp ...
    lab = own & (kp0[:, 0, 2] > 0)
    assert bool(lab.any())
    assert bool(v[lab][:, :4].all())
    assert bool((target[:c0][lab][:, 2] % SIDE == SIDE - 1).all()) and bool((target[:c0][lab][:, 3] // SIDE == SIDE - 1).all())
    assert bool((target[:c0][lab][:, 0] % SIDE == 0).all()) and bool((target[:c0][lab][:, 1] // SIDE == 0).all())
    # ... the two just outside are not, and v = 0 never is
    assert not bool(v[lab][:, 4:6].any())
    assert not bool(v[kp0[:, :, 2] == 0].any()) and bool((kp0[:, :, 2] == 0).any()) and bool((kp0[:, :, 2] == 1).any())
    assert int(selected[1]) == 0 and not bool(valid[1].any()), "a box of zero width is real"
    assert 0 < int(sel[0]) < c0, "some rows are dropped by the selection (bare instances), some are kept"


def test_selection_can_be_left_out():
    """apply_selection = False is Keypoints.to_heatmap's plain rule: `selected` is still reported."""
    boxes, matched, counts, kps = _table(5, 40, 17)
    got, _want = _check(boxes, matched, counts, kps, apply_selection=False)
    c0 = int(counts[0])
    t, v = R.to_heatmap(kps[0][matched[0, :c0]], boxes[0, :c0], SIDE)
    assert torch.equal(got[0][:c0].long(), t) and torch.equal(got[1][:c0].bool(), v)


def _fixture_tables(g):
    n = [len(g["fg_matched%d" % i]) for i in range(2)]
    R_ = max(n)
    boxes = torch.zeros(2, R_, 4)
    matched = torch.zeros(2, R_, dtype=torch.int64)
    for i in range(2):
        boxes[i, : n[i]] = g["fg_boxes%d" % i]
        matched[i, : n[i]] = g["fg_matched%d" % i].long()
    return boxes, matched, torch.tensor(n, dtype=torch.int32), [g["gt_keypoints%d" % i] for i in range(2)], n, R_


def test_targets_are_the_references_on_the_fixture():
    g = gold("keypoint_train")
    boxes, matched, counts, kps, n, R_ = _fixture_tables(g)
    (target, valid, selected, sel), _ = _check(boxes, matched, counts, kps)
    for i in range(2):
        keep = g["selected%d" % i].bool()
        rows = slice(i * R_, i * R_ + n[i])
        assert torch.equal(selected[rows].bool(), keep)
        assert int(sel[i]) == int(keep.sum())
        want_v = g["valid%d" % i].bool() & keep[:, None]
        assert torch.equal(valid[rows].bool(), want_v)
        assert torch.equal(target[rows].long(), g["targets%d" % i].long() * want_v.long())


def test_keypoints_to_heatmap_agrees_with_both():
    from lvc_amd.structures import Keypoints

    g = gold("keypoint_train")
    dev = _dev()
    for i in range(2):
        kp = Keypoints(g["gt_keypoints%d" % i])[g["fg_matched%d" % i].long()]
        h, v = kp.to(dev).to_heatmap(g["fg_boxes%d" % i].to(dev), SIDE)
        assert h.dtype == torch.int64 and v.dtype == torch.int64 and h.shape == (len(kp), 17)
        assert torch.equal(h.cpu(), g["targets%d" % i].long()) and torch.equal(v.cpu(), g["valid%d" % i].long())
        t, vv = R.to_heatmap(kp.tensor, g["fg_boxes%d" % i], SIDE)
        assert torch.equal(h.cpu(), t) and torch.equal(v.cpu().bool(), vv)
    boxes, matched, counts, kps = _table(3, 20, 8)
    c0 = int(counts[0])
    h, v = Keypoints(kps[0][matched[0, :c0]]).to(dev).to_heatmap(boxes[0, :c0].to(dev), 24)
    t, vv = R.to_heatmap(kps[0][matched[0, :c0]], boxes[0, :c0], 24)
    assert torch.equal(h.cpu(), t) and torch.equal(v.cpu().bool(), vv)
    e = Keypoints(torch.zeros(0, 17, 3)).to(dev).to_heatmap(torch.zeros(0, 4, device=dev), SIDE)
    assert e[0].numel() == 0 and e[1].numel() == 0
