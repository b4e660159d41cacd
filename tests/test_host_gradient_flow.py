"""The reference half of tests/test_gpu_gradient_flow.py on a machine without a GPU: every case of the module matrix is built on the
CPU with the exact-data recipe, evaluated by the fp64 reference (tests/module_ref.py) and held to the condition under which the
device must return that reference bit for bit -- activations within 4094, operands within two fp16 planes, every sum below 2^23
operand quanta (`Tape.check_caps`) -- and to having a gradient to lose: a non-zero reference gradient for every differentiable input
and every trainable parameter.  The quantum helper is checked on numbers whose answer is known."""
import pytest
import torch

import module_ref
from test_gpu_gradient_flow import module_cases, reference

CASES = module_cases()


def test_quantum():
    q = module_ref.quantum
    assert q(torch.tensor([0.0, 0.0])) == 1.0
    assert q(torch.tensor([6.0, -10.0])) == 2.0
    assert q(torch.tensor([3.0, 0.5, 0.0])) == 0.5
    assert q(torch.tensor([1.0 + 2.0 ** -20]), torch.tensor([4.0])) == 2.0 ** -20
    assert q(torch.tensor([2.0 ** 30], dtype=torch.float64)) == 2.0 ** 30


@pytest.mark.parametrize("build,state", [(b, s) for _, b, s in CASES], ids=[i for i, _, _ in CASES])
def test_reference_meets_the_exactness_condition(build, state):
    case = build()
    tape, in_grad, xr, yr, dys, diff = reference(case, state)      # asserts the condition and that there is a gradient to lose
    assert len(tape.records) > 0
    for y in yr:
        assert torch.equal(y.detach().float().double(), y.detach())


def test_zero_filters_occur():
    """About one filter in eight of the recipe is all zero: the degenerate row exponent of the row-scaled split stays in the test."""
    from lvc_amd.layers import Conv2d

    g = torch.Generator().manual_seed(3)
    conv = Conv2d(64, 256, 1, bias=False)
    module_ref.exact_conv_(conv, g)
    zero = int((conv.weight.abs().sum((1, 2, 3)) == 0).sum())
    assert 256 // 16 <= zero <= 256 // 4, zero
    assert set(conv.weight.unique().tolist()) <= {-1.0, 0.0, 1.0}
