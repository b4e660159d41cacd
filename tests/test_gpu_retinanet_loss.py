"""csrc/retinanet_loss.hip (`kernels.retinanet_loss`, `kernels.retinanet_loss_grad`) against tests/retinanet_loss_ref.py in float64
(autograd for the gradients).

Bars: 3 x the deviation of the SAME mirror run in torch-CPU float32 from its float64 run on the same inputs -- relative for the two loss
sums (the entry's fp64 sums; the fp32 losses are checked to be those sums over the normaliser, rounded once), max-abs for dlogits and
ddeltas.  Every measured ours / bar pair is written to profiles/retinanet_loss_parity.json.
`num_pos`, the zero gradients (ignored anchors, padding channels, non-positive anchors of ddeltas), run-to-run identity and the normaliser
recurrence are exact checks."""
import json
import os

import pytest
import torch

import retinanet_loss_ref as lref
from helpers import ROOT

pytestmark = pytest.mark.gpu

A = 9
PYRAMID = ((16, 24), (8, 12), (4, 6), (2, 3), (1, 2))
STRIDES = (8, 16, 32, 64, 128)
PLANTED = (0.0, 30.0, -30.0, 90.0, -90.0)
_PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def write_parity():
    yield
    if not _PARITY:
        return
    path = os.environ.get("LVC_RETINANET_LOSS_PARITY_OUT") or os.path.join(ROOT, "profiles", "retinanet_loss_parity.json")
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


def _anchors(shapes, strides):
    from lvc_amd.modeling.anchor_generator import DefaultAnchorGenerator

    out = []
    for (h, w), s in zip(shapes, strides):
        x = 4.0 * s
        cell = DefaultAnchorGenerator.generate_cell_anchors([x, x * 2 ** (1.0 / 3), x * 2 ** (2.0 / 3)], (0.5, 1.0, 2.0)).float()
        sx = torch.arange(0, w * s, step=s, dtype=torch.float32)
        sy = torch.arange(0, h * s, step=s, dtype=torch.float32)
        yy, xx = torch.meshgrid(sy, sx, indexing="ij")
        shifts = torch.stack((xx.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1)), 1)
        out.append((shifts.view(-1, 1, 4) + cell.view(1, -1, 4)).reshape(-1, 4))
    return torch.cat(out).contiguous()


class Case:
    """Inputs on the CPU (the mirror's) and on the device (the kernels'), made once."""

    def __init__(self, shapes, K, gts, seed=0, strides=None, pad_logit=0, ld_delta=None, misalign=False):
        from lvc_amd import kernels as Kn

        g = torch.Generator().manual_seed(seed)
        self.shapes, self.K, self.B = shapes, K, len(gts)
        strides = strides or STRIDES[:len(shapes)]
        self.anchors = _anchors(shapes, strides)
        R = self.R = self.anchors.shape[0]
        W, H = shapes[0][1] * strides[0], shapes[0][0] * strides[0]
        self.gt_boxes, self.gt_classes = [], []
        for n in gts:
            x0, y0 = torch.rand(n, generator=g) * W * 0.6, torch.rand(n, generator=g) * H * 0.6
            bw, bh = 12 + torch.rand(n, generator=g) * W * 0.4, 12 + torch.rand(n, generator=g) * H * 0.4
            self.gt_boxes.append(torch.stack([x0, y0, x0 + bw, y0 + bh], 1))
            self.gt_classes.append(torch.randint(0, K, (n,), generator=g))
        dev = _dev()
        self.gt = torch.cat(self.gt_boxes).to(dev) if sum(gts) else torch.zeros(0, 4, device=dev)
        self.gtc = torch.cat(self.gt_classes).to(dev)
        off = [0]
        for n in gts:
            off.append(off[-1] + n)
        self.gt_off = torch.tensor(off, dtype=torch.int32, device=dev)
        self.anchors_d = self.anchors.to(dev)
        # the matcher is the training forward's own; a few anchors of every image are then set to "ignored" by hand, so that every case
        # has some whatever its boxes are
        self.matches, self.labels = Kn.match_boxes_batched(self.gt, self.gt_off, self.B, self.anchors_d, None, [0.4, 0.5], [0, -1, 1], True)
        self.labels[:, 1::7] = torch.where(self.labels[:, 1::7] == 0, -1, self.labels[:, 1::7].int()).to(torch.int8)
        lab, mat = self.labels.cpu().long(), self.matches.cpu().long()
        gl = torch.full((self.B, R), K, dtype=torch.int64)
        self.matched_boxes = torch.zeros(self.B, R, 4)
        for b, n in enumerate(gts):
            gl[b][lab[b] < 0] = -1
            if n:
                pos = lab[b] == 1
                gl[b][pos] = self.gt_classes[b][mat[b][pos]]
                self.matched_boxes[b][pos] = self.gt_boxes[b][mat[b][pos]]
        self.gt_labels = gl
        self.num_pos = int(((gl >= 0) & (gl != K)).sum())
        # predictions: logits ~ N(0, 3), deltas ~ N(0, 0.5); planted logits on positive, background and ignored anchors of image 0
        self.logits_rk, self.deltas_r4 = [], []         # the mirror's [B, HWA, K] / [B, HWA, 4]
        r0 = 0
        for h, w in shapes:
            n = h * w * A
            x = torch.randn(self.B, n, K, generator=g) * 3.0
            for kind in (gl[0, r0:r0 + n] == K, (gl[0, r0:r0 + n] >= 0) & (gl[0, r0:r0 + n] != K), gl[0, r0:r0 + n] < 0):
                for j, r in enumerate(torch.nonzero(kind).flatten()[:len(PLANTED)].tolist()):
                    x[0, r, :] = PLANTED[j]
            self.logits_rk.append(x)
            self.deltas_r4.append(torch.randn(self.B, n, 4, generator=g) * 0.5)
            r0 += n
        # the head's layout: [B,H,W,ld] rows with NaN in the padding channels (read as an entry, a NaN would reach the sums)
        self.ldl = A * K + pad_logit
        self.ldd = ld_delta or 4 * A
        self.logits_d, self.deltas_d = [], []
        for (h, w), x, d in zip(shapes, self.logits_rk, self.deltas_r4):
            extra = 1 if misalign else 0
            buf = torch.full((self.B, h, w, self.ldl + extra), float("nan"))
            buf[..., extra:extra + A * K] = x.reshape(self.B, h, w, A * K)
            full = buf.to(dev)
            self.logits_d.append(full[..., extra:] if misalign else (full[..., :A * K] if pad_logit else full))
            bd = torch.full((self.B, h, w, self.ldd), float("nan"))
            bd[..., :4 * A] = d.reshape(self.B, h, w, 4 * A)
            fd = bd.to(dev)
            self.deltas_d.append(fd[..., :4 * A] if self.ldd != 4 * A else fd)
        self.misalign = misalign

    def pack(self, alpha, gamma, beta, weights=(1.0, 1.0, 1.0, 1.0)):
        from lvc_amd import kernels as Kn

        return Kn.RetinaNetLossArgs(self.logits_d, self.deltas_d, A, self.K, self.anchors_d, self.matches, self.labels, self.gt, self.gtc,
                                    self.gt_off, alpha=alpha, gamma=gamma, beta=beta, box_weights=weights)

    def mirror(self, dtype, alpha, gamma, beta, normalizer, g_cls, g_box, weights=(1.0, 1.0, 1.0, 1.0)):
        xs = [t.detach().clone().to(dtype).requires_grad_(True) for t in self.logits_rk]       # fresh leaves: a case serves several tests
        ds = [t.detach().clone().to(dtype).requires_grad_(True) for t in self.deltas_r4]
        lc, lb, sc, sb = lref.losses(xs, ds, self.anchors, self.gt_labels, self.matched_boxes, self.K, alpha, gamma, beta, weights, normalizer, dtype)
        (g_cls * lc + g_box * lb).backward()
        zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
        return float(sc.detach()), float(sb.detach()), [zero(t).double() for t in xs], [zero(t).double() for t in ds]


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300) if b != 0 else abs(a)


def run_and_check(name, case, alpha=0.25, gamma=2.0, beta=0.1, up=(1.0, 1.0), normalizer_in=100.0):
    from lvc_amd import kernels as Kn

    dev = _dev()
    pack = case.pack(alpha, gamma, beta)
    n_in = torch.tensor([normalizer_in], dtype=torch.float64, device=dev)
    n_out = torch.zeros(1, dtype=torch.float64, device=dev)
    losses, num_pos, sums = Kn.retinanet_loss(pack, n_in, n_out, return_sums=True)
    g_cls, g_box = torch.tensor(up[0], device=dev), torch.tensor(up[1], device=dev)
    # gradient tensors in the padded layout where the case has one, filled with NaN: the padding must come back zero
    dl = [torch.full(t.shape[:3] + (case.ldl,), float("nan"), device=dev) for t in case.logits_d]
    dd = [torch.full(t.shape[:3] + (case.ldd,), float("nan"), device=dev) for t in case.deltas_d]
    Kn.retinanet_loss_grad(pack, n_out, g_cls, g_box, dl, dd)
    torch.cuda.synchronize()
    assert int(num_pos) == case.num_pos
    nz = float(n_out)
    assert nz == lref.ema(normalizer_in, case.num_pos) and float(n_in) == normalizer_in
    AK = A * case.K
    ours_cls, ours_box = float(sums[0]), float(sums[1])
    # the fp32 losses are the fp64 sums over the normaliser, rounded once
    assert float(losses[0]) == float(torch.tensor(ours_cls / nz, dtype=torch.float64).float()) and float(losses[1]) == float(torch.tensor(ours_box / nz, dtype=torch.float64).float())
    for t in dl + dd:
        assert bool(torch.isfinite(t).all())
    for t in dl:
        assert float(t[..., AK:].abs().sum()) == 0.0
    for t in dd:
        assert float(t[..., 4 * A:].abs().sum()) == 0.0
    ours_dl = [t[..., :AK].reshape(case.B, -1, case.K).double().cpu() for t in dl]
    ours_dd = [t[..., :4 * A].reshape(case.B, -1, 4).double().cpu() for t in dd]
    # exact zeros: ignored anchors in dlogits, every anchor that is not positive in ddeltas
    gl = case.gt_labels
    ign, pos = gl < 0, (gl >= 0) & (gl != case.K)
    assert bool(ign.any())
    assert float(torch.cat(ours_dl, 1)[ign].abs().sum()) == 0.0
    assert float(torch.cat(ours_dd, 1)[~pos].abs().sum()) == 0.0
    if case.num_pos == 0:
        assert ours_box == 0.0
    s64 = case.mirror(torch.float64, alpha, gamma, beta, nz, *up)
    s32 = case.mirror(torch.float32, alpha, gamma, beta, nz, *up)
    rows = {
        "sum_cls": (_rel(ours_cls, s64[0]), _rel(s32[0], s64[0])),
        "sum_box": (_rel(ours_box, s64[1]), _rel(s32[1], s64[1])),
        "dlogits": (max(float((a - b).abs().max()) for a, b in zip(ours_dl, s64[2])), max(float((a - b).abs().max()) for a, b in zip(s32[2], s64[2]))),
        "ddeltas": (max(float((a - b).abs().max()) for a, b in zip(ours_dd, s64[3])), max(float((a - b).abs().max()) for a, b in zip(s32[3], s64[3]))),
    }
    bad = []
    for k, (ours, noise) in rows.items():
        bar = 3.0 * noise
        _PARITY["%s/%s" % (name, k)] = {"ours": ours, "fp32_mirror": noise, "bar": bar, "ratio": (ours / bar) if bar > 0 else (0.0 if ours == 0 else float("inf"))}
        print("%-40s %-8s ours %.3e  fp32 mirror %.3e  bar %.3e" % (name, k, ours, noise, bar))
        if not ours <= bar:
            bad.append((k, ours, bar))
    assert not bad, bad
    return losses, dl, dd


@pytest.fixture(scope="module")
def pyramid20():
    return Case(PYRAMID, 20, (3, 0, 5), seed=1)


@pytest.mark.parametrize("K", [1, 3, 20, 80])
def test_pyramid_classes(K, pyramid20):
    """A*K = 9 and 27 take the scalar path, 180 and 720 the 16-byte path; three images, the second without ground truth."""
    case = pyramid20 if K == 20 else Case(PYRAMID, K, (3, 0, 5), seed=1)
    run_and_check("pyramid_K%d" % K, case)


@pytest.mark.parametrize("shape,K", [((1, 2), 3), ((2, 3), 20)])
def test_one_tiny_level(shape, K):
    run_and_check("level_%dx%d_K%d" % (shape + (K,)), Case((shape,), K, (2,), seed=2, strides=(8,)))


@pytest.fixture(scope="module")
def large():
    return Case(((33, 37),), 20, (6,), seed=3, strides=(8,))


def test_one_level_many_workgroups(large):
    """33 x 37 x 9 x 20 = 219 780 entries: several workgroups and a tail."""
    run_and_check("level_33x37_K20", large)


@pytest.mark.parametrize("K", [20, 3])
def test_padded_rows(K):
    """ld_logit = A*K + 4, ld_delta = 64, NaN in the padding: never read; the gradient's padding comes back zero."""
    run_and_check("padded_K%d" % K, Case(PYRAMID[1:], K, (4, 2), seed=4, pad_logit=4, ld_delta=64))


def test_misaligned_base_takes_the_scalar_path():
    """A channel slice that starts one float into a wider row: A*K = 180 but neither the stride nor the base allow 16-byte loads."""
    run_and_check("misaligned_K20", Case(PYRAMID[2:], 20, (3,), seed=5, misalign=True))


def test_no_ground_truth_in_the_batch():
    case = Case(PYRAMID[1:], 20, (0, 0, 0), seed=6)
    losses, _dl, dd = run_and_check("no_gt", case)
    assert case.num_pos == 0 and float(losses[1]) == 0.0 and all(float(t.abs().sum()) == 0.0 for t in dd)


@pytest.mark.parametrize("alpha,gamma", [(0.25, 2.0), (-1.0, 2.0), (0.25, 0.0), (0.25, 1.5)])
@pytest.mark.parametrize("beta,up", [(0.1, (1.0, 1.0)), (0.0, (1024.0, 0.5))])
def test_loss_parameters(alpha, gamma, beta, up, pyramid20):
    run_and_check("params_a%g_g%g_b%g_up%g" % (alpha, gamma, beta, up[0]), pyramid20, alpha, gamma, beta, up)


def test_single_image_batch():
    run_and_check("B1", Case(PYRAMID, 20, (4,), seed=7), beta=0.0, up=(1024.0, 0.5))


def test_gamma_between_0_and_1_is_refused(pyramid20):
    with pytest.raises(NotImplementedError, match="MODEL.RETINANET.FOCAL_LOSS_GAMMA"):
        pyramid20.pack(0.25, 0.5, 0.1)


def test_runs_are_bit_identical(large, pyramid20):
    from lvc_amd import kernels as Kn

    dev = _dev()
    for case in (large, pyramid20):
        outs = []
        for _ in range(2):
            pack = case.pack(0.25, 2.0, 0.1)
            n_in = torch.tensor([100.0], dtype=torch.float64, device=dev)
            n_out = torch.zeros(1, dtype=torch.float64, device=dev)
            losses, _n = Kn.retinanet_loss(pack, n_in, n_out)
            dl, dd = Kn.retinanet_loss_grad(pack, n_out, torch.tensor(1024.0, device=dev), torch.tensor(0.5, device=dev))
            outs.append([losses, n_out] + dl + dd)
        for a, b in zip(*outs):
            assert torch.equal(a, b)


def test_normaliser_recurrence_and_uncommitted_call(pyramid20):
    """Three consecutive calls, each reading the slot the previous one wrote, leave the Python recurrence on the counted positives;
    a call whose normalizer_out is not made current leaves the current value as it was."""
    from lvc_amd import kernels as Kn

    dev = _dev()
    slots = [torch.tensor([100.0], dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)]
    cur, want = 0, 100.0
    pack = pyramid20.pack(0.25, 2.0, 0.1)
    for _ in range(3):
        _l, n = Kn.retinanet_loss(pack, slots[cur], slots[1 - cur])
        cur = 1 - cur
        want = lref.ema(want, int(n))
        assert float(slots[cur]) == want
    before = float(slots[cur])
    Kn.retinanet_loss(pack, slots[cur], slots[1 - cur])          # not committed: `cur` stays
    assert float(slots[cur]) == before == want
    with pytest.raises(ValueError):
        Kn.retinanet_loss(pack, slots[cur], slots[cur])
