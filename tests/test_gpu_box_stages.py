"""The box selection stages around the top-k and the NMS (lvc_amd/csrc/boxes.hip), called directly through `lvc_amd.kernels`.

Routes each group reaches (every routed case asserts its precondition from sizes the C ABI reports, `_row_stats_route`):

  1. candidate stage of `fast_rcnn_inference`
     test_candidates_row_stats_route_K       det_row_stats_kernel (K + 1 < 97, statistics fit the NMS scratch): K = 1, one mask word
                                             (63, 64), two words (65, 95), LDS pitch ncol | 1 for even and odd ncol, B*R = 260 rows
                                             (four full 64-row tiles and one of 4)
     test_candidates_in_kernel_route_K       det_candidates_kernel's own per-thread loops: K + 1 >= 97 (K = 96, 130)
     test_candidates_same_input_both_routes  K = 95 on row-stats (default capacity) and on the in-kernel loops (capacity 64): bit-equal
     test_candidates_rows_across_1024        the 1024-row trip and the carried `base`: R = 1024, 1025, 2050, prop_count clipped to R,
                                             rows past the count that would pass the threshold, prop_count = None
     test_candidates_cls_agnostic / _padded  deltas [B*R, 4]; ld_cls = K + 8 and ld_delta = 4K + 12 with 1e30 in the padding, on both
                                             routes
     test_candidates_threshold_is_strict     p == score_thresh is no candidate, p == nextafter(score_thresh, 0) ... is, on both routes
     test_candidates_non_finite_rows         a NaN row, -inf rows with one finite entry, on both routes
     test_candidates_truncated               a candidate list of 37: status bit, and WHICH candidates survive
  2. det_gather_kernel
     test_gather_detections_direct           `lvc_gather_detections`: chunks of 256 (topk = 1 .. 600), the carry between chunks, boxes
                                             dropped by `post` at wave and chunk borders and in the middle
     test_gather_through_fast_rcnn_inference the same kernel behind the NMS with more than 256 kept per image and a non-unit `post`
  3. RPN after the top-k
     test_rpn_min_box_size                   rpn_decode_seg_kernel's `> min_box_size` (exact: zero deltas) and a random case
     test_rpn_non_finite_selected            non-finite deltas / logits on selected candidates: clamp keeps NaN, isfinite + nonempty
     test_rpn_merge_routes                   rpn_merge_levels_kernel: kept scores in global memory (total > 8192) and in LDS
     test_rpn_ties_across_levels             the merge's `sm == s && m < l` with the cut inside a tie between two levels
     test_rpn_shapes                         L = 1 (A = 1, A = 15), L = 8 = MAXL, two image sizes, pre above the small levels' sizes

How results are judged.  Discrete outputs (counts, classes, rows, order, status) equal the oracle's (oracle/rcnn.py, fp32) exactly.
The only fp-sensitive decision these stages add is `p > score_thresh`: every case asserts on the CPU that no float64 probability lies
within 1e-6 of the threshold, and that the oracle evaluated in float64 makes the same discrete choices as in fp32 (so the case is
settled before the device is asked).  Values (scores, boxes) are compared with the float64 evaluation of the oracle on the same input;
the bar is K_BAR = 3 x the deviation of the oracle's own fp32 evaluation from that float64 evaluation, measured in the test and printed
next to the device's error (the convention of tests/test_gpu_sem_seg.py).  Where that deviation is 0 the device must be equal.  Rows
past the count are zero.  One exception, measured and explained at `_det_check`: the class scores of long rows are held to 3 x the
deviation of the fp32 softmax summed serially, as the kernels document their sum, where that is larger than torch's.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
D = "cuda:0"
K_BAR = 3.0
BOX_W = (10.0, 10.0, 5.0, 5.0)
EPS_P = 1e-6         # no float64 probability may lie this close to the score threshold


def _k():
    from lvc_amd import kernels
    return kernels


def _orc():
    from oracle import rcnn
    return rcnn


# ===================================================================================================== 1. fast_rcnn_inference
def _row_stats_route(B, R, K, max_candidates):
    """True: `lvc_fast_rcnn_inference` takes the softmax statistics from det_row_stats_kernel; False: det_candidates_kernel computes
    them in its own loops.  From the sizes alone, as the entry point decides it."""
    from lvc_amd import _lib
    nmax = max(1, R * K) if max_candidates is None else min(max_candidates, max(1, R * K))
    nms = _lib.size_query("lvc_batched_nms_workspace_bytes", B, nmax)
    return K + 1 < 97 and B * R * 28 + 64 <= (nms + 15) // 16 * 16


def _det_case(seed, B, R, K, thresh=0.05, nms=0.5, topk=100, counts=None, sizes=None, agnostic=False, logit_std=2.5, delta_std=1.2):
    g = torch.Generator().manual_seed(seed)
    props = torch.rand(B, R, 4, generator=g) * 400
    props[..., 2:] = props[..., :2] + 4 + torch.rand(B, R, 2, generator=g) * 300
    cls = torch.randn(B * R, K + 1, generator=g) * logit_std
    dl = torch.randn(B * R, 4 if agnostic else 4 * K, generator=g) * delta_std
    sizes = sizes or [(480, 640), (500, 700), (300, 300)][:B]
    return dict(B=B, R=R, K=K, cls=cls, dl=dl, props=props, counts=counts, sizes=sizes, thresh=thresh, nms=nms, topk=topk, post=None)


def _det_oracle(c, dtype, limit=None):
    """The oracle on every image of case `c`, evaluated in `dtype` -> per image (boxes, scores, classes, rows).  limit: only the first
    `limit` candidates of an image in (row, class) order exist (the truncated candidate list).  Asserts that the case is settled."""
    orc = _orc()
    out = []
    R, K = c["R"], c["K"]
    for i in range(c["B"]):
        n = R if c["counts"] is None else min(c["counts"][i], R)
        cls = c["cls"][i * R: i * R + n].to(dtype)
        dl = c["dl"][i * R: i * R + n].to(dtype)
        pb = orc.apply_deltas(dl, c["props"][i, :n], BOX_W)
        pr = torch.softmax(cls, -1)
        if dtype == torch.float64:
            assert not bool(((pr[:, :K] - c["thresh"]).abs() < EPS_P).any()), "a float64 probability lies within 1e-6 of the threshold"
        if limit is not None:
            hit = (pr[:, :K] > c["thresh"]).reshape(-1)
            late = hit & (hit.cumsum(0) > limit)
            pr = pr.clone()
            pr[:, :K].masked_fill_(late.view(-1, K), 0)
        rb, rs, rc, rr = orc.fast_rcnn_inference_single_image(pb, pr, c["sizes"][i], c["thresh"], c["nms"], c["topk"])
        if c["post"] is not None:
            oh, ow = c["post"][i]
            rb, rs, rc, keep = orc.detector_postprocess(rb, rs, rc, c["sizes"][i], oh, ow, return_keep=True)
            rr = rr[keep]
        out.append((rb, rs, rc, rr))
    return out


def _det_refs(c, limit=None):
    """(fp32 oracle, float64 oracle) of the case, with the discrete outputs asserted equal between the two."""
    r32, r64 = _det_oracle(c, torch.float32, limit), _det_oracle(c, torch.float64, limit)
    for a, b in zip(r32, r64):
        assert a[2].tolist() == b[2].tolist() and a[3].tolist() == b[3].tolist(), "fp32 and float64 oracle choose differently: not settled"
    return r32, r64


def _post_tensor(c):
    if c["post"] is None:
        return None
    return torch.tensor([[ow / w, oh / h, oh, ow] for (oh, ow), (h, w) in zip(c["post"], c["sizes"])], dtype=torch.float32, device=D)


def _det_run(c, cls=None, dl=None, max_candidates=16384, status=None):
    K = _k()
    cls = c["cls"].to(D) if cls is None else cls
    dl = c["dl"].to(D) if dl is None else dl
    cnt = None if c["counts"] is None else torch.tensor(c["counts"], dtype=torch.int32, device=D)
    return K.fast_rcnn_inference(cls, dl, c["props"].to(D), cnt, torch.tensor(c["sizes"], dtype=torch.int32, device=D), c["K"], BOX_W,
                                 c["thresh"], c["nms"], c["topk"], post=_post_tensor(c), status=status, max_candidates=max_candidates)


def _judge(what, got, ref32, ref64, serial32=None):
    """One value comparison: |device - float64| <= K_BAR x |fp32 oracle - float64|, both printed; equal where the latter is 0.
    serial32: a second fp32 evaluation of the oracle's formula (`_serial_softmax32`); the bar takes the larger deviation of the two."""
    if ref64.numel() == 0:
        assert got.numel() == 0
        return
    dev32 = float((ref32.double() - ref64).abs().max())
    err = float((got.double() - ref64).abs().max())
    if serial32 is None:
        print("%s: |hip - fp64| %.3e, oracle fp32 deviation %.3e" % (what, err, dev32))
    else:
        ser = float((serial32.double() - ref64).abs().max())
        print("%s: |hip - fp64| %.3e, oracle fp32 deviation %.3e, summed serially %.3e" % (what, err, dev32, ser))
        dev32 = max(dev32, ser)
    assert err <= K_BAR * dev32, (what, err, dev32)


def _serial_softmax32(cls):
    """The oracle's softmax in fp32 with the sum taken serially in class order and the quotient as a product with the reciprocal: the
    order of operations det_row_stats_kernel documents (one thread walks its row).  torch sums a row in vector lanes, which rounds
    fewer times: on rows of 64 and more classes its deviation from float64 is a third of this evaluation's."""
    with np.errstate(all="ignore"):
        x = cls.numpy()
        e = np.exp(x - x.max(1, keepdims=True)).astype(np.float32)
        acc = np.zeros(len(x), np.float32)
        for k in range(x.shape[1]):
            acc = acc + e[:, k]
        return torch.from_numpy(e * (np.float32(1) / acc)[:, None])


def _det_check(what, c, got, refs):
    """Scores: measured on the K >= 63 cases, the device's error is 3.3 to 3.6 x the deviation of torch's fp32 softmax from float64
    (e.g. K = 96: 4.30e-07 against 1.21e-07), and equal to the deviation of the same fp32 formula summed serially (4.30e-07): the excess
    is the summation order, not the kernel.  So the scores are held to K_BAR x the larger of the two fp32 evaluations' deviations, both
    measured here on the case's input and printed; K_BAR itself stays.  Boxes are held to the oracle's deviation alone."""
    b, s, cl, rows, cnt = [t.cpu() for t in got]
    r32, r64 = refs
    ns = [len(r[1]) for r in r32]
    assert cnt.tolist() == ns
    R = c["R"]
    for i, n in enumerate(ns):
        assert cl[i, :n].tolist() == r32[i][2].tolist() and rows[i, :n].tolist() == r32[i][3].tolist()
        assert not b[i, n:].any() and not s[i, n:].any() and not cl[i, n:].any() and not rows[i, n:].any()      # rows past the count
    cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
    serial = cat([_serial_softmax32(c["cls"][i * R: (i + 1) * R])[r[3], r[2]] for i, r in enumerate(r32)])
    _judge(what + " scores", cat([s[i, :n] for i, n in enumerate(ns)]), cat([r[1] for r in r32]), cat([r[1] for r in r64]), serial)
    _judge(what + " boxes", cat([b[i, :n] for i, n in enumerate(ns)]), cat([r[0] for r in r32]), cat([r[0] for r in r64]))


@pytest.mark.parametrize("K", [1, 63, 64, 65, 95])
def test_candidates_row_stats_route_K(K):
    c = _det_case(100 + K, 2, 130, K)
    refs = _det_refs(c)
    assert _row_stats_route(2, 130, K, 16384), "precondition: det_row_stats_kernel"
    _det_check("row-stats K=%d" % K, c, _det_run(c), refs)


@pytest.mark.parametrize("K", [96, 130])
def test_candidates_in_kernel_route_K(K):
    c = _det_case(201 + K, 2, 130, K)
    refs = _det_refs(c)
    assert not _row_stats_route(2, 130, K, 16384), "precondition: det_candidates_kernel's own loops"
    _det_check("in-kernel K=%d" % K, c, _det_run(c), refs)


def _peaked_case():
    """K = 95, every third row peaked on one foreground class, threshold 0.5: a few dozen candidates per image."""
    c = _det_case(31, 2, 130, 95, thresh=0.5, logit_std=1.0)
    g = torch.Generator().manual_seed(32)
    rows = torch.arange(0, 260, 3)
    c["cls"][rows, torch.randint(0, 95, (len(rows),), generator=g)] += 12.0
    return c


def test_candidates_same_input_both_routes():
    """The header comment of det_row_stats_kernel promises bit-identical scores: the same input on both routes is torch.equal."""
    K = _k()
    c = _peaked_case()
    refs = _det_refs(c)
    ncand = [int((torch.softmax(c["cls"][i * 130: (i + 1) * 130], -1)[:, :95] > 0.5).sum()) for i in range(2)]
    assert all(24 <= n <= 64 for n in ncand), ncand
    assert _row_stats_route(2, 130, 95, 16384) and not _row_stats_route(2, 130, 95, 64), "precondition: the two runs take different routes"
    st_a, st_b = K.new_status(D), K.new_status(D)
    a = _det_run(c, status=st_a)
    b = _det_run(c, max_candidates=64, status=st_b)
    assert int(st_a) == 0 and int(st_b) == 0            # no overflow
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    _det_check("both routes K=95", c, a, refs)


@pytest.mark.parametrize("R,use_counts", [(1024, True), (1025, True), (2050, True), (1025, False)])
def test_candidates_rows_across_1024(R, use_counts):
    """The second image's rows past its count (R = 2050: rows 1030 ..) are peaked on a foreground class: read, they are detections."""
    counts = [R, 1030] if use_counts else None
    c = _det_case(300 + R + use_counts, 2, R, 5, thresh=0.3, counts=counts)
    if use_counts and R > 1030:
        c["cls"][R + 1030:, 2] += 20.0
    refs = _det_refs(c)
    assert _row_stats_route(2, R, 5, 16384), "precondition: det_row_stats_kernel"
    _det_check("R=%d counts=%s" % (R, counts), c, _det_run(c), refs)


def test_candidates_cls_agnostic():
    c = _det_case(41, 2, 130, 20, agnostic=True)
    assert c["dl"].shape == (260, 4)
    refs = _det_refs(c)
    _det_check("cls_agnostic", c, _det_run(c), refs)


@pytest.mark.parametrize("K", [20, 96])
def test_candidates_padded_rows(K):
    """cls_logits and deltas as column slices of wider tensors, as the box head emits them; the padding would win every softmax."""
    c = _det_case(50 + K, 2, 130, K)
    refs = _det_refs(c)
    assert _row_stats_route(2, 130, K, 16384) == (K == 20)
    wide_c = torch.full((260, K + 8), 1e30)
    wide_c[:, : K + 1] = c["cls"]
    wide_d = torch.full((260, 4 * K + 12), 1e30)
    wide_d[:, : 4 * K] = c["dl"]
    wide_c, wide_d = wide_c.to(D), wide_d.to(D)
    got = _det_run(c, cls=wide_c[:, : K + 1], dl=wide_d[:, : 4 * K])
    _det_check("padded K=%d" % K, c, got, refs)


@pytest.mark.parametrize("ncol,R", [(2, 70), (4, 70), (8, 70), (128, 40)])
def test_candidates_threshold_is_strict(ncol, R):
    """K + 1 equal logits: every probability is exactly 1 / (K + 1) on both sides (exp(0) = 1, a sum of ones, a power of two).  At
    score_thresh = 1 / (K + 1) nothing is a candidate; at the next float below, every class of every row is.  K + 1 = 2, 4, 8 run on
    the row-stats route; 128 equal logits are the same exact case on det_candidates_kernel's own loops."""
    K = ncol - 1
    c = _det_case(60 + ncol, 1, R, K, sizes=[(480, 640)])
    c["cls"][:] = torch.randn(R, 1, generator=torch.Generator().manual_seed(ncol)).expand(R, ncol)
    p = 1.0 / ncol
    assert torch.equal(torch.softmax(c["cls"], -1), torch.full((R, ncol), p))
    assert _row_stats_route(1, R, K, 16384) == (ncol < 97)
    c["thresh"] = p
    got = _det_run(c)
    assert int(got[4][0]) == 0 and not any(bool(t.any()) for t in got[:4])
    assert len(_det_oracle(c, torch.float32)[0][1]) == 0
    below = float(torch.nextafter(torch.tensor(p), torch.tensor(0.0)))
    c["thresh"] = below
    r32 = _det_oracle(c, torch.float32)
    assert int((torch.softmax(c["cls"], -1)[:, :K] > below).sum()) == R * K            # every class of every row is a candidate
    got = _det_run(c)
    b, s, cl, rows, cnt = [t.cpu() for t in got]
    rb, rs, rc, rr = r32[0]
    n = len(rs)
    assert n > 0 and int(cnt[0]) == n
    assert cl[0, :n].tolist() == rc.tolist() and rows[0, :n].tolist() == rr.tolist()
    assert torch.equal(s[0, :n], rs) and torch.equal(rs, torch.full((n,), p))          # exact on both sides
    # the float64 softmax is 1 / (K + 1) too, so only the boxes carry rounding: judged against the float64 decode of the same rows
    orc = _orc()
    pb64 = orc.clip_boxes_(orc.apply_deltas(c["dl"].double(), c["props"][0], BOX_W).reshape(-1, 4), c["sizes"][0]).view(R, K, 4)
    _judge("strict threshold 1/%d R=%d boxes" % (ncol, R), b[0, :n], rb, pb64[rr, rc])


@pytest.mark.parametrize("K", [7, 96])
def test_candidates_non_finite_rows(K):
    c = _det_case(70 + K, 2, 70, K)
    c["cls"][3] = float("nan")
    c["cls"][5] = float("-inf"); c["cls"][5, 2] = 0.25          # one finite foreground entry: probability 1
    c["cls"][6] = float("-inf"); c["cls"][6, K] = -3.0          # only the background is finite: nothing
    c["cls"][70 + 69] = float("nan")                            # the last row of the second image
    c["cls"][70 + 11] = float("-inf"); c["cls"][70 + 11, K - 1] = 1e4
    refs = _det_refs(c)
    assert (5, 2) in list(zip(refs[0][0][3].tolist(), refs[0][0][2].tolist())) and 3 not in refs[0][0][3].tolist() and 6 not in refs[0][0][3].tolist()
    assert _row_stats_route(2, 70, K, 16384) == (K == 7)
    _det_check("non-finite rows K=%d" % K, c, _det_run(c), refs)


def test_candidates_truncated():
    """A candidate list of 37 on about 100 candidates per image: the status word has the overflow bit, and the detections are the
    oracle's on the first 37 candidates of each image in (row, class) order, as det_candidates_kernel documents it."""
    K = _k()
    c = _det_case(81, 2, 130, 20, thresh=0.35)
    ncand = [int((torch.softmax(c["cls"][i * 130: (i + 1) * 130], -1)[:, :20] > 0.35).sum()) for i in range(2)]
    assert all(70 <= n <= 140 for n in ncand), ncand
    full, cut = _det_refs(c), _det_refs(c, limit=37)
    assert [r[3].tolist() for r in full[0]] != [r[3].tolist() for r in cut[0]]
    st = K.new_status(D)
    got = _det_run(c, max_candidates=37, status=st)
    assert int(st) & K.DET_OVERFLOW
    _det_check("truncated to 37", c, got, cut)
    st = K.new_status(D)
    got = _det_run(c, max_candidates=None, status=st)
    assert int(st) == 0
    _det_check("full capacity", c, got, full)


# ===================================================================================================== 2. gather
def _gather_ref(boxes, scores, classes, rows, keep, num_keep, topk, post):
    """det_gather_kernel in numpy: rows keep[b][:min(num_keep[b], topk)] in that order, through scale / clip / drop-empty."""
    B = len(num_keep)
    ob, osc = np.zeros((B, topk, 4), np.float32), np.zeros((B, topk), np.float32)
    ocl, orow, cnt = np.zeros((B, topk), np.int32), np.zeros((B, topk), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        idx = keep[b, : min(int(num_keep[b]), topk)]
        bx = boxes[b, idx].copy()
        ok = np.ones(len(idx), bool)
        if post is not None:
            sx, sy, oh, ow = post[b]
            bx[:, 0::2] = np.clip(bx[:, 0::2] * sx, np.float32(0), ow)
            bx[:, 1::2] = np.clip(bx[:, 1::2] * sy, np.float32(0), oh)
            ok = (bx[:, 2] - bx[:, 0] > 0) & (bx[:, 3] - bx[:, 1] > 0)
        n = int(ok.sum())
        ob[b, :n], osc[b, :n], ocl[b, :n], orow[b, :n], cnt[b] = bx[ok], scores[b, idx][ok], classes[b, idx][ok], rows[b, idx][ok], n
    return ob, osc, ocl, orow, cnt


@pytest.mark.parametrize("with_post", [False, True])
@pytest.mark.parametrize("topk", [1, 255, 256, 257, 600])
def test_gather_detections_direct(topk, with_post):
    K = _k()
    rng = np.random.RandomState(topk)
    B, Nmax = 3, 700
    num_keep = np.array([0, 300, 700], np.int32)
    keep = np.stack([rng.permutation(Nmax) for _ in range(B)]).astype(np.int32)
    post = np.array([[0.75, 1.5, 450, 300], [1.25, 0.5, 200, 500], [0.625, 0.875, 350, 250]], np.float32)
    xy = (rng.rand(B, Nmax, 2) * 300).astype(np.float32)
    boxes = np.concatenate([xy, xy + 1 + (rng.rand(B, Nmax, 2) * 200).astype(np.float32)], 2)
    out_w = (post[:, 3] / post[:, 0])[:, None]
    far = rng.rand(B, Nmax) < 0.1                      # past out_w before the scale: dropped by `post`, anywhere in a chunk
    boxes[..., 0] = np.where(far, out_w + 5, boxes[..., 0]); boxes[..., 2] = np.where(far, out_w + 50, boxes[..., 2])
    planted = 0
    for b in range(B):
        nk = min(int(num_keep[b]), topk)
        for j, pos in enumerate(sorted({p for p in (0, 63, 64, 255, 256, nk - 1) if 0 <= p < nk})):
            i = keep[b, pos]
            if j % 3 == 0:      # zero width after clamping to out_w
                boxes[b, i] = [out_w[b, 0] + 1, 10, out_w[b, 0] + 90, 60]
            elif j % 3 == 1:    # fully outside the image
                boxes[b, i] = [-80, -70, -10, -5]
            else:               # exactly zero area
                boxes[b, i] = [40, 30, 40, 90]
            planted += 1
    assert planted == {1: 2, 255: 8, 256: 8, 257: 10, 600: 12}[topk]
    scores = rng.rand(B, Nmax).astype(np.float32)
    classes = rng.randint(0, 80, (B, Nmax)).astype(np.int32)
    rows = rng.randint(0, 1000, (B, Nmax)).astype(np.int32)
    ref = _gather_ref(boxes, scores, classes, rows, keep, num_keep, topk, post if with_post else None)
    if with_post:
        full = np.minimum(num_keep, topk)
        assert all(0 < ref[4][b] < full[b] for b in (1, 2)) or topk == 1, "post must drop some and keep some"
    dv = lambda a: torch.from_numpy(a).to(D)
    got = K.gather_detections(dv(boxes), dv(scores), dv(classes), dv(rows), dv(keep), dv(num_keep), topk, post=dv(post) if with_post else None)
    for g, r in zip(got, ref):
        assert torch.equal(g.cpu(), torch.from_numpy(r))      # a multiply and a clamp: exact; includes the zero tail and the counts


def test_gather_through_fast_rcnn_inference():
    """topk = 300 behind an NMS that keeps more than 256 per image: the second chunk of det_gather_kernel with a non-unit `post`."""
    c = _det_case(91, 2, 400, 5, thresh=0.1, nms=0.95, topk=300, sizes=[(410, 392), (420, 388)])
    kept = [len(r[1]) for r in _det_oracle(c, torch.float32)]
    assert all(n > 256 for n in kept), kept              # the oracle's NMS keeps more than 256 per image (before `post`)
    c["post"] = [(225, 330), (450, 490)]                 # (out_h, out_w): scales 0.842 x 0.549 and 1.263 x 1.071; proposals right of
                                                         # the image are clipped to zero width, pass the NMS and are dropped here
    refs = _det_refs(c)
    after = [len(r[1]) for r in refs[0]]
    assert all(256 < a for a in after) and any(a < n for a, n in zip(after, kept)), (kept, after)
    _det_check("gather behind the NMS, topk 300", c, _det_run(c), refs)


# ===================================================================================================== 3. RPN after the top-k
SIZES5, STRIDES5, RATIOS = (32, 64, 128, 256, 512), (4, 8, 16, 32, 64), (0.5, 1.0, 2.0)


def _rpn_case(seed, shapes, sizes, pre, post, nms=0.7, min_box_size=0.0, N=2, cell=None, strides=None, logit_std=2.0, delta_std=0.5):
    orc = _orc()
    g = torch.Generator().manual_seed(seed)
    L = len(shapes)
    cell = cell or [orc.generate_cell_anchors((s,), RATIOS) for s in SIZES5[:L]]
    strides = list(strides or STRIDES5[:L])
    A = cell[0].shape[0]
    logits = [torch.randn(N, h * w * A, generator=g) * logit_std for h, w in shapes]
    deltas = [torch.randn(N, h * w * A, 4, generator=g) * delta_std for h, w in shapes]
    return dict(shapes=list(shapes), sizes=list(sizes), pre=pre, post=post, nms=nms, mbs=min_box_size, N=N, cell=cell, strides=strides, A=A,
                logits=logits, deltas=deltas)


def _rpn_oracle(c, dtype, post=None):
    orc = _orc()
    anchors = orc.grid_anchors(c["cell"], c["shapes"], c["strides"])
    return orc.find_top_rpn_proposals(anchors, c["logits"], [d.to(dtype) for d in c["deltas"]], c["sizes"], c["nms"], c["pre"],
                                      c["post"] if post is None else post, min_box_size=c["mbs"])


def _rpn_refs(c):
    r32, r64 = _rpn_oracle(c, torch.float32), _rpn_oracle(c, torch.float64)
    for (b32, l32), (b64, l64) in zip(r32, r64):
        assert torch.equal(l32, l64), "fp32 and float64 oracle choose differently: not settled"
    return r32, r64


def _rpn_run(c):
    K = _k()
    A = c["A"]
    fused = []
    for lg, dl, (h, w) in zip(c["logits"], c["deltas"], c["shapes"]):       # one NHWC tensor per level, as the predictor conv emits it
        N = lg.shape[0]
        fused.append(torch.cat([lg.view(N, h, w, A), dl.reshape(N, h, w, A * 4)], dim=3).contiguous().to(D))
    return K.rpn_proposals([f[..., :A] for f in fused], [f[..., A:] for f in fused], [t.to(D) for t in c["cell"]], c["strides"],
                           torch.tensor(c["sizes"], dtype=torch.int32, device=D), c["pre"], c["post"], c["nms"], min_box_size=c["mbs"])


def _rpn_check(what, c, got, refs, exact=False):
    boxes, olog, count = [t.cpu() for t in got]
    r32, r64 = refs
    ns = [len(r[1]) for r in r32]
    assert count.tolist() == ns
    for n, k in enumerate(ns):
        assert torch.equal(olog[n, :k], r32[n][1])                      # the same candidates in the same order
        assert not boxes[n, k:].any() and not olog[n, k:].any()         # rows past the count
    cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
    b32, b64 = cat([r[0] for r in r32]), cat([r[0] for r in r64])
    if exact:
        assert torch.equal(b32.double(), b64), "the case is meant to be exact on both sides"
    _judge(what + " boxes", cat([boxes[n, :k] for n, k in enumerate(ns)]), b32, b64)


SHAPES_SMALL = [(12, 16), (6, 8), (3, 4), (2, 2), (1, 1)]


@pytest.mark.parametrize("mbs", [32.0, float(np.nextafter(np.float32(32.0), np.float32(0.0))), 8.0])
def test_rpn_min_box_size(mbs):
    """Zero deltas: every proposal is its anchor clipped to the image.  The cell anchors have integer corners here (size s: 1.5 s x
    0.75 s, s x s, 0.75 s x 1.5 s; sqrt(2) is not a float), so the decode is exact on both sides and the boxes must be equal.  At
    min_box_size = 32 the 32 x 32 anchors (size 32, ratio 1: [-16, 16] around integer centres) are dropped (the comparison is strict),
    at the next float below they stay.  min_box_size = 8 runs with random deltas on the usual anchors."""
    zero = mbs != 8.0
    cell = [torch.tensor([[-0.75, -0.375, 0.75, 0.375], [-0.5, -0.5, 0.5, 0.5], [-0.375, -0.75, 0.375, 0.75]]) * s for s in SIZES5] if zero else None
    c = _rpn_case(7, SHAPES_SMALL, [(48, 64), (44, 60)], 100, 400, min_box_size=mbs, delta_std=0.0 if zero else 0.5, cell=cell)
    refs = _rpn_refs(c)
    if zero:
        wh = [(r[0][:, 2] - r[0][:, 0], r[0][:, 3] - r[0][:, 1]) for r in refs[0]]
        n32 = sum(int(((w == 32) & (h == 32)).sum()) for w, h in wh)
        assert (n32 == 0) if mbs == 32.0 else (n32 > 0), n32
    else:
        loose = dict(c, mbs=0.0)
        assert sum(len(r[1]) for r in refs[0]) < sum(len(r[1]) for r in _rpn_oracle(loose, torch.float32)), "min_box_size must drop some"
    _rpn_check("min_box_size %r" % mbs, c, _rpn_run(c), refs, exact=zero)


def test_rpn_non_finite_selected():
    """Non-finite deltas and a non-finite logit on candidates the top-k is certain to select (the highest logits of their level).
    The oracle filters by isfinite and then by nonempty; torch.clamp(max=) keeps a NaN, as select_common.h states for the device."""
    inf, nan = float("inf"), float("nan")
    c = _rpn_case(11, SHAPES_SMALL, [(48, 64), (44, 60)], 50, 300, nms=0.9)
    plant = [(0, 17, 100.0, 0, inf),      # dx = +inf: the box is not finite, dropped
             (0, 40, 99.0, 2, inf),       # dw = +inf: clamped to log(1000 / 16), kept
             (0, 77, 98.0, 2, nan),       # dw = NaN: stays NaN, dropped
             (0, 101, 97.0, 2, -inf),     # dw = -inf: width 0, dropped as empty
             (1, 9, 100.0, 3, inf),       # dh = +inf on the next level: kept
             (1, 30, 99.0, 1, -inf),      # dy = -inf: dropped
             (2, 5, 100.0, 3, nan)]       # dh = NaN on a level smaller than pre
    for n in range(2):
        for l, i, lg, comp, val in plant:
            c["logits"][l][n, i + n] = lg
            c["deltas"][l][n, i + n, comp] = val
        c["logits"][0][n, 200 + n] = inf  # selected first, then dropped
    refs = _rpn_refs(c)
    for n in range(2):
        kept = refs[0][n][1].tolist()
        assert inf not in kept and 98.0 not in kept and 97.0 not in kept and kept.count(99.0) == 1 and kept.count(100.0) == 1
    _rpn_check("non-finite on selected candidates", c, _rpn_run(c), refs)


def test_rpn_merge_routes():
    """Five levels of 26 x 26 x 3 anchors, pre = 2000, NMS threshold 1.0 (nothing is suppressed), image larger than every anchor's
    reach: post = 2000 leaves more than 8192 kept scores over the levels (rpn_merge_levels_kernel reads them from global memory),
    post = 1000 at most 5000 (the LDS route).  Both match the oracle; the first 1000 rows of the first equal the second bit for bit."""
    c = _rpn_case(13, [(26, 26)] * 5, [(1800, 1900), (1750, 1850)], 2000, 2000, nms=1.0, delta_std=0.3)
    totals = [len(r[1]) for r in _rpn_oracle(c, torch.float32, post=10 ** 6)]
    assert all(t > 8192 for t in totals), totals
    assert 5 * 1000 <= 8192
    refs = _rpn_refs(c)
    assert all(len(r[1]) == 2000 for r in refs[0])
    big = _rpn_run(c)
    _rpn_check("merge from global memory (kept %s)" % totals, c, big, refs)
    c2 = dict(c, post=1000)
    small = _rpn_run(c2)
    _rpn_check("merge from LDS", c2, small, _rpn_refs(c2))
    assert torch.equal(big[0][:, :1000], small[0]) and torch.equal(big[1][:, :1000], small[1])
    assert small[2].tolist() == [1000, 1000]


def _levels_of(c, n, post):
    """Level of every row of image n's merged list: the oracle run level by level (batched_nms never lets levels interact) and merged
    by (score descending, level ascending, the level's own order)."""
    orc = _orc()
    anchors = orc.grid_anchors(c["cell"], c["shapes"], c["strides"])
    rows = []
    for l in range(len(c["shapes"])):
        b, s = orc.find_top_rpn_proposals([anchors[l]], [c["logits"][l][n: n + 1]], [c["deltas"][l][n: n + 1]], [c["sizes"][n]], c["nms"],
                                          c["pre"], 10 ** 6, min_box_size=c["mbs"])[0]
        rows += [(-float(v), l, t) for t, v in enumerate(s)]
    rows.sort()
    return [r[1] for r in rows[:post]], [-r[0] for r in rows[:post]]


def test_rpn_ties_across_levels():
    """Logits in multiples of 1/8: equal scores are common within and across levels.  Order: score descending, then level ascending,
    then the level's own order.  `post` cuts image 0's list between two equal scores of different levels."""
    c = _rpn_case(17, [(20, 24), (10, 12), (5, 6), (3, 3), (2, 2)], [(80, 96), (76, 90)], 300, 10 ** 6)
    for l in range(5):
        c["logits"][l] = torch.round(c["logits"][l] * 8) / 8
    full = _rpn_oracle(c, torch.float32)
    lv, sc = _levels_of(c, 0, 10 ** 6)
    assert sc == full[0][1].tolist()                       # the merged order is the stated one
    post = next(p for p in range(60, len(sc)) if sc[p - 1] == sc[p] and lv[p - 1] != lv[p])
    assert full[0][1][post - 1] == full[0][1][post] and lv[post - 1] < lv[post]     # last kept and first dropped: equal, two levels
    cross = sum(1 for p in range(1, post) if sc[p - 1] == sc[p] and lv[p - 1] != lv[p])
    assert cross >= 5, cross
    c["post"] = post
    _rpn_check("ties across levels, post %d" % post, c, _rpn_run(c), _rpn_refs(c))


def _shape_cases():
    orc = _orc()
    one = [orc.generate_cell_anchors((32,), (1.0,))]
    fifteen = [orc.generate_cell_anchors(SIZES5, RATIOS)]
    maps8 = [(16, 16), (12, 12), (8, 8), (6, 6), (4, 4), (3, 3), (2, 2), (1, 1)]
    cell8 = [orc.generate_cell_anchors((s,), RATIOS) for s in (16, 24, 32, 48, 64, 96, 128, 256)]
    return {"L1-A1": lambda: _rpn_case(21, [(5, 7)], [(40, 56), (33, 50)], 20, 50, cell=one, strides=[8]),
            "L1-A15": lambda: _rpn_case(22, [(5, 7)], [(80, 112), (70, 100)], 200, 100, cell=fifteen, strides=[16]),
            "L8": lambda: _rpn_case(23, maps8, [(64, 64), (50, 61)], 100, 300, cell=cell8, strides=[4, 5, 8, 10, 16, 21, 32, 64])}


@pytest.mark.parametrize("name", ["L1-A1", "L1-A15", "L8"])
def test_rpn_shapes(name):
    """One level with one and with fifteen anchors per pixel, eight levels (the maximum) from 16 x 16 down to 1 x 1, two images of
    different sizes, pre above the size of the small levels (L8: 100 against 3, 12, 27 and 48 anchors)."""
    c = _shape_cases()[name]()
    assert c["A"] == {"L1-A1": 1, "L1-A15": 15, "L8": 3}[name] and c["sizes"][0] != c["sizes"][1]
    refs = _rpn_refs(c)
    assert all(len(r[1]) > 0 for r in refs[0])
    _rpn_check("shape " + name, c, _rpn_run(c), refs)
