"""The shared helpers of the train-mode stage operators in arco_amd/ops.py (-m gpu): the one bn_groups batch check
(_bn_group_count) in front of every operator that splits a batch into BatchNorm groups, and the flat-gradient route
(_flat_grad: gradients written straight into the optimiser's flat buffer) against the returned-gradient route."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rand(shape, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32)).cuda()


def _bn_buffers(c):
    return torch.zeros(c, device="cuda"), torch.ones(c, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")


def _group_check_cases():
    """name -> (callable under bn_groups(2) on a batch of 3, the BatchNorm buffers it would have updated)."""
    from arco_amd import ops
    cases = {}
    rm, rv, nbt = _bn_buffers(16)
    x2 = ops.to_channels_last(_rand((3, 16, 8, 8), 1))
    w2, b2, g, be = _rand((16, 16, 3, 3), 2, 0.1), _rand((16,), 3), _rand((16,), 4), _rand((16,), 5)
    cases["conv_bn_act"] = (lambda: ops.conv_bn_act(x2, w2, b2, g, be, rm, rv, num_batches_tracked=nbt), (rm, rv, nbt))

    convs = [torch.nn.Conv2d(16, 16, 3, padding=1).cuda() for _ in range(2)]
    bns = [torch.nn.BatchNorm2d(16).cuda() for _ in range(2)]
    act = torch.nn.LeakyReLU()
    xb = ops.to_channels_last(_rand((3, 16, 16, 16), 6))
    cases["conv_block"] = (lambda: ops.conv_block(xb, convs[0], bns[0], act, 0.0, convs[1], bns[1], act),
                           tuple(t for bn in bns for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)))

    rm3, rv3, nbt3 = _bn_buffers(16)
    z3 = ops.to_channels_last(_rand((3, 16, 4, 4, 4), 7))
    cases["bn_act"] = (lambda: ops.bn_act(z3, g, be, rm3, rv3, num_batches_tracked=nbt3), (rm3, rv3, nbt3))

    rm4, rv4, nbt4 = _bn_buffers(4)
    y4 = ops.to_channels_last(_rand((3, 32, 2, 2, 2), 8))
    g4, be4 = _rand((4,), 9), _rand((4,), 10)
    cases["bn_act_d2s"] = (lambda: ops.bn_act_d2s(y4, g4, be4, rm4, rv4, num_batches_tracked=nbt4), (rm4, rv4, nbt4))

    convs3 = [torch.nn.Conv3d(16, 16, 3, padding=1).cuda() for _ in range(2)]
    bns3 = [torch.nn.BatchNorm3d(16).cuda() for _ in range(2)]

    def nograd():
        with torch.no_grad():
            return ops.conv_block3d_nograd(z3, list(zip(convs3, bns3)))
    cases["conv_block3d_nograd"] = (nograd, tuple(t for bn in bns3 for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)))
    return cases


@pytest.mark.parametrize("name", ["conv_bn_act", "conv_block", "bn_act", "bn_act_d2s", "conv_block3d_nograd"])
def test_a_batch_that_is_no_multiple_of_the_groups_is_refused_before_anything_changes(name):
    from arco_amd import ops
    call, buffers = _group_check_cases()[name]
    before = [t.clone() for t in buffers]
    stats = dict(ops.block_fuse_stats)
    prev, ops.BLOCK_FUSE = ops.BLOCK_FUSE, 1
    try:
        with ops.bn_groups(2):
            with pytest.raises(RuntimeError, match=r"bn_groups\(2\) needs a batch that is a multiple of 2, got 3"):
                call()
    finally:
        ops.BLOCK_FUSE = prev
    torch.cuda.synchronize()
    assert dict(ops.block_fuse_stats) == stats
    for t, b in zip(buffers, before):
        assert torch.equal(t, b)


def _install_flat(params):
    """Zero-filled flat gradient views, installed the way optim.SGDNesterov.__init__ installs them; returns the per-parameter mark
    counts."""
    flat_g = torch.zeros(sum(p.numel() for p in params), device="cuda")
    marks = [0] * len(params)

    def marker(i):
        def mark():
            marks[i] += 1
        return mark

    off = 0
    for i, p in enumerate(params):
        k = p.numel()
        p.grad = flat_g[off:off + k].view(p.shape)
        p._arco_grad_view = p.grad
        p._arco_mark = marker(i)
        off += k
    return marks


def _run_stage(flat):
    from arco_amd import ops
    prm = [torch.nn.Parameter(t) for t in (_rand((16, 3, 3, 3), 11, 0.2), _rand((16,), 12), _rand((16,), 13), _rand((16,), 14, 0.2))]
    marks = _install_flat(prm) if flat else None
    weight, bias, gamma, beta = prm
    rm, rv, nbt = _bn_buffers(16)
    x = ops.to_channels_last(_rand((4, 3, 16, 16), 15))
    ops.reseed_dropout(99)
    with ops.bn_groups(2):
        a = ops.conv_bn_act(x, weight, bias, gamma, beta, rm, rv, slope=0.01, p=0.2, num_batches_tracked=nbt)
    (a * _rand(tuple(a.shape), 16)).sum().backward()
    torch.cuda.synchronize()
    return [p.grad.clone() for p in prm], marks


def _run_d2s(flat):
    from arco_amd import ops
    prm = [torch.nn.Parameter(t) for t in (_rand((4,), 21), _rand((4,), 22, 0.2))]
    marks = _install_flat(prm) if flat else None
    rm, rv, nbt = _bn_buffers(4)
    y = ops.to_channels_last(_rand((2, 32, 4, 4, 4), 23)).requires_grad_(True)
    a = ops.bn_act_d2s(y, prm[0], prm[1], rm, rv, num_batches_tracked=nbt)
    (a * _rand(tuple(a.shape), 24)).sum().backward()
    torch.cuda.synchronize()
    return [p.grad.clone() for p in prm], marks


def test_flat_route_equals_returned_route_conv_bn_act():
    (w0, b0, g0, be0), none = _run_stage(False)
    (w1, b1, g1, be1), marks = _run_stage(True)
    assert none is None and marks == [1, 1, 1, 1]                   # weight, bias, gamma, beta: each marked exactly once
    assert torch.equal(w0, w1) and torch.equal(g0, g1) and torch.equal(be0, be1)
    assert float(w0.abs().max()) > 0 and float(g0.abs().max()) > 0 and float(be0.abs().max()) > 0
    assert torch.equal(b0, torch.zeros_like(b0)) and torch.equal(b1, torch.zeros_like(b1))      # exact zeros on both routes


def test_flat_route_equals_returned_route_bn_act_d2s():
    (g0, be0), none = _run_d2s(False)
    (g1, be1), marks = _run_d2s(True)
    assert none is None and marks == [1, 1]
    assert torch.equal(g0, g1) and torch.equal(be0, be1)
    assert float(g0.abs().max()) > 0 and float(be0.abs().max()) > 0
