"""lvc_mask_targets (csrc/mask_targets.hip) against tests/mask_train_ref.py: two images of different sizes in one call, T = 28 and 2,
boxes from sub-pixel to whole-image, counts, the untouched rows, the invalid-sample rule and an exact tie.  Pixels whose fp64 average
lies within 3 x the reference expression's own max |fp32 - fp64| of 0.5 are set aside (their share is capped); every other byte must
be equal."""
import pytest
import torch

import mask_train_ref as R

pytestmark = pytest.mark.gpu

SIZES = ((61, 83), (40, 57))
SENTINEL = 0xAB
CAP_INSIDE = 1e-3       # boxes inside their image (training proposals are clipped)
CAP_BORDER = 1e-2       # boxes reaching over the border: a half-outside bin inside the mask averages k +- ulp over 2k

# image 0 (61 x 83): sub-pixel (grid 1x1), whole image (grid 3x3), touching each border, 0.6 px high
BOXES_0 = [[10.5, 10.5, 11.2, 11.4], [0., 0., 83., 61.], [0., 12.3, 30.7, 40.2], [3.2, 0., 40.9, 50.1], [50.3, 20.1, 83., 44.],
           [12., 30.5, 60.4, 61.], [0., 20., 83., 20.6], [5.25, 5.75, 33.25, 33.75]]
MATCH_0 = [0, 1, 2, 3, 0, 1, 5, 4]          # plane 4 is empty, plane 5 is full
BOXES_1 = [[0., 0., 57., 40.], [7.7, 3.1, 30.2, 38.9], [20., 10., 20.4, 10.3], [40.1, 0., 57., 21.5], [2., 2., 55., 39.]]
MATCH_1 = [1, 0, 2, 3, 0]
ROWS = 10


def _planes():
    p0 = R.ellipse_masks(6, *SIZES[0], seed=1)
    p0[4], p0[5] = False, True
    p1 = R.ellipse_masks(4, *SIZES[1], seed=2)
    return [p0, p1]


def _table(boxes_lists, match_lists):
    boxes = torch.zeros(2, ROWS, 4)
    matched = torch.zeros(2, ROWS, dtype=torch.int64)
    for b, (bl, ml) in enumerate(zip(boxes_lists, match_lists)):
        boxes[b, : len(bl)] = torch.tensor(bl, dtype=torch.float32).reshape(-1, 4)
        matched[b, : len(ml)] = torch.tensor(ml, dtype=torch.int64)
    return boxes, matched


def _run(planes, boxes, matched, counts, T):
    from lvc_amd import kernels as K

    dev = torch.device("cuda:0")
    out = torch.full((boxes.shape[0] * boxes.shape[1], T, T), SENTINEL, dtype=torch.uint8, device=dev)
    K.mask_targets(boxes.to(dev), matched.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev), [p.to(dev) for p in planes], T, out=out)
    return out.cpu()


def _compare(planes, boxes, matched, counts, T, cap, tag):
    got = _run(planes, boxes, matched, counts, T)
    rows, ps, bs = [], [], []
    for b in range(boxes.shape[0]):
        for r in range(boxes.shape[1]):
            if r < counts[b]:
                rows.append(b * boxes.shape[1] + r)
                ps.append(planes[b][int(matched[b, r])])
                bs.append(boxes[b, r])
            else:
                assert bool((got[b * boxes.shape[1] + r] == SENTINEL).all()), "row %d of image %d lies past the count and was written" % (r, b)
    if not rows:
        return 0, 0
    bits, band, dev, bits32 = R.targets(ps, torch.stack(bs), T)
    g = got[rows]
    assert bool(((g == 0) | (g == 1)).all())
    bad = ((g != 0) != bits) & ~band
    aside, n = int(band.sum()), band.numel()
    print("%s T=%d: reference deviation %.2e, %d of %d pixels set aside (%.3f %%), %d bytes differ from the reference's fp32 bits"
          % (tag, T, dev, aside, n, 100.0 * aside / n, int(((g != 0) != bits32).sum())))
    assert not bool(bad.any()), "%d target pixels outside the band differ" % int(bad.sum())
    assert aside <= cap * n, "set-aside share %.4f above the cap %.4f" % (aside / n, cap)
    return aside, n


@pytest.mark.parametrize("T", [28, 2])
def test_targets_two_images_one_call(T):
    planes = _planes()
    boxes, matched = _table([BOXES_0, BOXES_1], [MATCH_0, MATCH_1])
    _, n = _compare(planes, boxes, matched, [len(BOXES_0), len(BOXES_1)], T, CAP_INSIDE, "inside")
    assert n == (len(BOXES_0) + len(BOXES_1)) * T * T


@pytest.mark.parametrize("T", [28, 2])
def test_targets_count_zero_and_short_counts(T):
    planes = _planes()
    boxes, matched = _table([BOXES_0, BOXES_1], [MATCH_0, MATCH_1])
    _compare(planes, boxes, matched, [0, 3], T, CAP_INSIDE, "count 0 / 3")
    _compare(planes, boxes, matched, [2, 0], T, CAP_INSIDE, "count 2 / 0")


def test_targets_empty_and_full_planes():
    planes = _planes()
    boxes, matched = _table([BOXES_0, BOXES_1], [[4] * len(BOXES_0), MATCH_1])
    got = _run(planes, boxes, matched, [len(BOXES_0), 0], 28)
    assert not bool(got[: len(BOXES_0)].any())
    boxes, matched = _table([BOXES_0, BOXES_1], [[5] * len(BOXES_0), MATCH_1])
    got = _run(planes, boxes, matched, [len(BOXES_0), 0], 28)
    assert bool((got[: len(BOXES_0)] == 1).all())      # boxes inside the image on a full plane: every average is 1


@pytest.mark.parametrize("T", [28, 2])
def test_targets_invalid_sample_rule(T):
    """Boxes reaching over the border: a sample outside [-1, H] x [-1, W] adds nothing and still counts in the divisor."""
    planes = _planes()
    over0 = [[-9.3, -7.2, 30.4, 33.1], [60.2, 40.7, 95.5, 70.3], [-20., 10., 100., 50.], [30., -15., 50., 75.]]
    over1 = [[-6.1, -3.3, 20.2, 18.8], [35.5, 22.2, 70.7, 52.1]]
    boxes, matched = _table([over0, over1], [[0, 1, 5, 5], [0, 1]])
    _compare(planes, boxes, matched, [4, 2], T, CAP_BORDER, "over the border")
    # ... and on its own where every sum is exact: a full plane, an integer-aligned box whose bins hold 4 x 4 samples one pixel apart;
    # 12 of the 28 bin rows lie outside [-1, H]: their averages are 0, the bins inside average 1, the bin rows across the edge in between
    full = [torch.ones(1, 56, 56, dtype=torch.bool), planes[1]]
    boxes, matched = _table([[[-28., -28., 84., 84.]], []], [[0], []])
    got = _run(full, boxes, matched, [1, 0], 28)[0]
    bits, band, dev, _ = R.targets([full[0][0]], boxes[0, :1], 28)
    assert dev == 0.0 and not bool(band.any()) and torch.equal(got != 0, bits[0])
    assert not bool(got[:6].any()) and bool((got[8:20, 8:20] == 1).all())


def test_targets_exact_tie():
    """Plane true for x < 31, box [4, 4, 60, 60], bins of 2 px: all arithmetic is exact, one column of bins averages exactly 0.5 and
    must come out set (>= 0.5), with nothing set aside."""
    plane = torch.zeros(1, 64, 64, dtype=torch.bool)
    plane[:, :, :31] = True
    box = torch.tensor([[4., 4., 60., 60.]])
    avg = R.target_average(plane[0], box[0], 28)
    assert float((R.target_average(plane[0], box[0], 28, torch.float32).double() - avg).abs().max()) == 0.0
    assert int((avg == 0.5).sum()) == 28
    from lvc_amd import kernels as K

    dev = torch.device("cuda:0")
    got = K.mask_targets(box.view(1, 1, 4).to(dev), torch.zeros(1, 1, dtype=torch.int64, device=dev), torch.ones(1, dtype=torch.int32, device=dev),
                         [plane.to(dev)], 28).cpu()
    assert torch.equal(got[0] != 0, avg >= 0.5)


def test_bitmasks_crop_and_resize_is_the_batched_entry():
    from lvc_amd.structures import BitMasks

    planes = _planes()
    dev = torch.device("cuda:0")
    boxes, matched = _table([BOXES_0, BOXES_1], [MATCH_0, MATCH_1])
    want = _run(planes, boxes, matched, [len(BOXES_0), len(BOXES_1)], 28)
    for b, (bl, ml) in enumerate(((BOXES_0, MATCH_0), (BOXES_1, MATCH_1))):
        masks = BitMasks(planes[b].to(dev))[torch.tensor(ml, device=dev)]
        got = masks.crop_and_resize(torch.tensor(bl, device=dev), 28)
        assert got.dtype == torch.bool and got.shape == (len(bl), 28, 28)
        assert torch.equal(got.cpu(), want[b * ROWS: b * ROWS + len(bl)] != 0)
