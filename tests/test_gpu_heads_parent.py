"""The box, mask and keypoint branches against what the commit before they were put on one path computed on an MI355X
(tests/golden/heads_parent.npz, recorded there by scripts/record_heads_parent.py): the functions of that script run on this tree, and
every array they return is held to the fixture -- bit for bit where that commit reproduced the array between its own two runs
(`exact_names`), to 1e-6 of the array's largest entry where it did not (`margin_names`).  Which array is of which kind is read from the
fixture.  The same for the mask and keypoint TRAINING branches against tests/golden/heads_train_parent.npz, recorded by the same script
(`--train`) on the commit before those two were put on one path."""
import importlib.util
import os

import numpy as np
import pytest

from helpers import ROOT, gold

pytestmark = pytest.mark.gpu


def _script():
    spec = importlib.util.spec_from_file_location("record_heads_parent", os.path.join(ROOT, "scripts", "record_heads_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rec = _script()


@pytest.fixture(scope="module")
def want():
    return np.load(os.path.join(ROOT, "tests", "golden", "heads_parent.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def want_train():
    return np.load(os.path.join(ROOT, "tests", "golden", "heads_train_parent.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def models():
    built = {}

    def get(name):
        if name not in built:
            if name in [c[0] for c in rec.TRAIN_CASES]:
                built[name] = rec.build_train_case_model(name)
            else:
                built[name] = rec.build_train_model() if name == "train" else rec.build_model(name)
        return built[name]

    return get


def _hold(got, want, prefix):
    """Every array of `got` against the fixture, and no array of the fixture under `prefix` left out."""
    exact, margin = set(want["exact_names"].tolist()), set(want["margin_names"].tolist())
    recorded = {k for k in exact | margin if k.startswith(prefix)}
    assert set(got) == recorded, (sorted(set(got) - recorded), sorted(recorded - set(got)))
    bad = []
    for k, a in got.items():
        if k in margin:
            ref = want[k]
            assert a.shape == ref.shape, k
            dev, top = float(np.abs(a.astype(np.float64) - ref.astype(np.float64)).max()), float(np.abs(ref).max())
            print("%-70s held to the margin: max deviation %.3e of %.3e" % (k, dev, top))
            if not dev <= 1e-6 * top:
                bad.append(k)
        elif rec.DIGEST + k in want.files:
            if rec.digest(a).tobytes() != want[rec.DIGEST + k].tobytes():
                bad.append(k)
        else:
            ref = want[k]
            if not (a.dtype == ref.dtype and a.shape == ref.shape and a.tobytes() == ref.tobytes()):
                bad.append(k)
    assert not bad, bad


def _only_conv_bias_gradients_on_the_margin(want):
    for k in want["margin_names"].tolist():
        assert ".grad." in k and k.endswith(".bias") and "box_predictor" not in k, k
    assert len(want["exact_names"]) + len(want["margin_names"]) == len([k for k in want.files if not k.endswith("_names")])


def test_only_conv_bias_gradients_are_held_to_the_margin(want):
    """The list of arrays the recording commit did not reproduce is a condition of the fixture: nothing but bias gradients of
    convolutions (a conv's bias gradient joins slabs with float atomics) may be on it."""
    _only_conv_bias_gradients_on_the_margin(want)


def test_training_fixture_holds_the_bit_stable_gradients_exactly(want_train):
    """The same condition on heads_train_parent.npz; score_lowres' gradients come from kernels documented as bit-stable and are
    held bit for bit.  Its short cases must be short: fewer sampled rows per image than the quota, or the deferred step would not
    fall back to the per-image heads."""
    _only_conv_bias_gradients_on_the_margin(want_train)
    exact = set(want_train["exact_names"].tolist())
    for case, kind, topk in rec.TRAIN_CASES:
        for deferred in (0, 1):
            tag = "%s.deferred%d." % (case, deferred)
            if kind == "keypoint":
                for leaf in ("weight", "bias"):
                    assert tag + "grad.roi_heads.keypoint_head.score_lowres." + leaf in exact
            rows = float(want_train[tag + "scalar.roi_head/num_fg_samples"][0]) + float(want_train[tag + "scalar.roi_head/num_bg_samples"][0])
            assert (rows < rec.BATCH_SIZE_PER_IMAGE) if topk is not None else (rows == rec.BATCH_SIZE_PER_IMAGE), (tag, rows)


@pytest.mark.parametrize("name", rec.MODELS)
def test_inference_gives_the_parent_commits_bits(name, models, want):
    """do_postprocess True and False and, for the mask and keypoint models, inference(detected_instances=...): counts, boxes, scores,
    classes and pred_masks / pred_keypoints."""
    _hold(rec.inference_case(name, models(name)), want, name + ".")


@pytest.mark.parametrize("name", rec.MODELS)
def test_state_dict_keys_keep_their_order(name, models, want):
    assert list(models(name).state_dict()) == want["keys." + name].tolist()


@pytest.mark.parametrize("deferred", [True, False])
def test_mask_training_step_gives_the_parent_commits_bits(deferred, models, want):
    """One step of the mask model (the mask_train fixture's batch, 128 rows per image, identity randperm) on the deferred path and with
    GeneralizedRCNN.deferred_reads = False: every loss, the bias gradients of the box and mask predictors, mask_head.deconv.weight.grad
    and the latest value of every scalar the step logged."""
    g = {k: v.numpy() if hasattr(v, "numpy") else v for k, v in gold("mask_train").items()}
    tag = "train.deferred%d." % int(deferred)
    _hold(rec.train_case(models("train"), g, deferred), want, tag)


@pytest.mark.parametrize("deferred", [True, False])
@pytest.mark.parametrize("case", [c[0] for c in rec.TRAIN_CASES])
def test_training_step_gives_the_parent_commits_bits(case, deferred, models, want_train):
    """One step of the keypoint model at the full quota (`keypoint_train`), and of the keypoint and the mask model with
    MODEL.RPN.POST_NMS_TOPK_TRAIN = 64 (`keypoint_short`, `mask_short`: no image fills its 128 rows, so the deferred step discards its
    padded losses and runs the heads per image), each on the deferred path and with GeneralizedRCNN.deferred_reads = False: every loss,
    the recorded gradients and the latest value of every scalar the step logged."""
    gm = {k: v.numpy() if hasattr(v, "numpy") else v for k, v in gold("mask_train").items()}
    gk = {k: v.numpy() if hasattr(v, "numpy") else v for k, v in gold("keypoint_train").items()}
    _hold(rec.run_train_case(case, models(case), gm, gk, deferred), want_train, "%s.deferred%d." % (case, int(deferred)))
