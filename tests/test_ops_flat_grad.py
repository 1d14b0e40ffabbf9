"""The one test "is this parameter's .grad still the optimiser's flat view?" (ops._flat_grad) and the three routes built on it:
_grad_into (weights), _affine_grad_targets (BatchNorm gamma / beta), _zero_bias_grad (conv biases under train-mode BatchNorm).
Plain Python over tensors: CPU tensors and a counting stand-in for the optimiser's marker, no library."""
import pytest
import torch

from arco_amd import ops


def _param(state, n=4):
    """A parameter with a zero-filled flat view installed as optim.SGDNesterov installs it, then: 'flat' - untouched; 'replaced' -
    somebody assigned a new .grad; 'none' - .grad was reset to None.  Returns (parameter, view, list of marks)."""
    p = torch.nn.Parameter(torch.arange(float(n)))
    flat, marks = torch.zeros(n), []
    p.grad = flat[0:n].view(p.shape)
    p._arco_grad_view = p.grad
    p._arco_mark = lambda: marks.append(1)
    view = p._arco_grad_view
    if state == "replaced":
        p.grad = torch.zeros_like(p)
    elif state == "none":
        p.grad = None
    return p, view, marks


def test_flat_grad_is_the_view_only_while_grad_is_the_view():
    p, view, marks = _param("flat")
    assert ops._flat_grad(p) is view and marks == []              # the test itself marks nothing: the writer does
    for state in ("replaced", "none"):
        p, view, marks = _param(state)
        assert ops._flat_grad(p) is None and marks == []
    assert ops._flat_grad(torch.nn.Parameter(torch.zeros(3))) is None      # no view installed at all


@pytest.mark.parametrize("state", ["flat", "replaced", "none"])
def test_grad_into(state):
    p, view, marks = _param(state)
    calls = []

    def compute(out, accumulate):
        calls.append((out, accumulate))
        out.add_(1.0) if accumulate else out.fill_(1.0)

    got = ops._grad_into(p, compute)
    assert len(calls) == 1
    if state == "flat":
        assert got is None and calls[0][0] is view and calls[0][1] == 1 and marks == [1]
        assert torch.equal(view, torch.ones(4))
    else:
        assert got is calls[0][0] and calls[0][1] == 0 and marks == []
        assert got.shape == p.shape and torch.equal(got, torch.ones(4)) and torch.equal(view, torch.zeros(4))


@pytest.mark.parametrize("state", ["flat", "replaced", "none"])
def test_affine_grad_targets(state):
    gamma, gview, gmarks = _param(state)
    beta, bview, bmarks = _param(state)
    dg_t, db_t, acc, dgamma, dbeta = ops._affine_grad_targets(gamma, beta)
    if state == "flat":
        assert dg_t is gview and db_t is bview and acc == 1 and dgamma is None and dbeta is None
        assert gmarks == [1] and bmarks == [1]
    else:
        assert acc == 0 and dg_t is dgamma and db_t is dbeta and gmarks == [] and bmarks == []
        assert dgamma.shape == gamma.shape and dbeta.shape == beta.shape
        assert dgamma.data_ptr() not in (gview.data_ptr(), bview.data_ptr()) and dbeta.data_ptr() != dgamma.data_ptr()


def test_affine_grad_targets_need_both_parameters_on_the_flat_route():
    gamma, gview, gmarks = _param("flat")
    beta, bview, bmarks = _param("replaced")
    dg_t, db_t, acc, dgamma, dbeta = ops._affine_grad_targets(gamma, beta)
    assert acc == 0 and dg_t is dgamma and db_t is dbeta and dg_t is not gview and gmarks == [] and bmarks == []


@pytest.mark.parametrize("state", ["flat", "replaced", "none"])
def test_zero_bias_grad(state):
    b, view, marks = _param(state)
    got = ops._zero_bias_grad(b, 4, torch.device("cpu"))
    if state == "flat":
        assert got is None and marks == [1] and torch.equal(view, torch.zeros(4))
    else:
        assert marks == [] and got.shape == (4,) and got.dtype == torch.float32 and torch.equal(got, torch.zeros(4))
