"""What tests/test_gpu_avgpool.py and tests/test_gpu_resnet_d.py share: the device, the measured bar (K_NOISE x the reference's own
fp32-vs-fp64 deviation) and the (ours, noise, bar, ratio) rows that both merge into profiles/avgpool_parity.json
(LVC_AVGPOOL_PARITY_OUT: another path).  A test module imports `write_parity` to have its rows written when it ends."""
import json
import os

import pytest
import torch

from helpers import ROOT

K_NOISE = 3.0
_PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def write_parity():
    yield
    if not _PARITY:
        return
    path = os.environ.get("LVC_AVGPOOL_PARITY_OUT") or os.path.join(ROOT, "profiles", "avgpool_parity.json")
    try:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.update(_PARITY)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def dev():
    return torch.device("cuda:0")


def record(key, ours, noise):
    bar = K_NOISE * noise
    _PARITY[key] = {"ours": ours, "noise": noise, "bar": bar, "ratio": ours / bar if bar > 0 else (0.0 if ours == 0 else float("inf"))}
    print("%-48s ours %.3e  noise %.3e  bar %.3e" % (key, ours, noise, bar))
    return bar
