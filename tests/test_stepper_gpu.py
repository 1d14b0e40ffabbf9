"""arco_amd/stepper.py on the device: the one writer of the process-wide mode switches (every stepper sets all five, whatever a
stepper of the other rank left behind) and the order in which the two constructors consume the torch CPU generator."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = ["--batch_size", "2", "--queue_size", "64", "--K", "4", "--graphs", "0", "--synthetic", "1"]
SWITCHES = ("CONV_MMA", "ACT_HALF", "HEAD_MMA", "LOSS_SCALE", "WGRAD_SIDE")


def _make2d(extra=()):
    from arco_amd import train_arco_2d as T
    args = T.build_parser().parse_args(SMALL + list(extra))
    args.patch_size = [32, 32]
    return T.ArcoStep2D(args, "cuda:0")


def _make3d(extra=()):
    from arco_amd import train_arco_3d as T3
    args = T3.build_parser().parse_args(SMALL + ["--num_classes", "2"] + list(extra))
    args.patch_size = [16, 16, 16]
    return T3.ArcoStep3D(args, "cuda:0")


def test_every_constructor_writes_the_full_table_of_switches():
    from arco_amd import ops
    saved = {n: getattr(ops, n) for n in SWITCHES}
    env = ops._WGRAD_SIDE_ENV                # ARCO_WGRAD_SIDE, as the package read it
    wg = (lambda default: default) if env is None else (lambda default: int(env))
    table = lambda: tuple(getattr(ops, n) for n in SWITCHES)
    try:
        _make3d(["--act_dtype", "f16"])
        assert table() == (3, True, 1, 16384.0, wg(3))
        _make2d()
        assert table() == (3, False, 0, 16384.0, wg(0))
        _make3d()
        assert table() == (3, False, 0, 16384.0, wg(3))
    finally:
        for n, v in saved.items():
            setattr(ops, n, v)
        torch.cuda.empty_cache()


def test_constructors_consume_the_cpu_generator_in_the_reference_order():
    """3-D: the banks come first (train_arco_3d.py:144-151: one randn(1, 16) per class) - bit for bit the first C draws of the seeded
    generator.  2-D: the banks are zeros (train_arco_2d.py:147-154) and draw nothing."""
    from arco_amd import ops
    saved = {n: getattr(ops, n) for n in SWITCHES}
    try:
        random.seed(5); np.random.seed(5); torch.manual_seed(5)
        draws = [torch.randn(1, 16) for _ in range(2)]
        random.seed(5); np.random.seed(5); torch.manual_seed(5)
        st = _make3d()
        assert len(st.memobank) == 2 and st.queue_size == [64, 64]
        for c in range(2):
            assert torch.equal(st.memobank[c][0].cpu(), draws[c]), c
            assert int(st.queue_ptrlis[c]) == 0
        st = _make2d()
        assert len(st.memobank) == 4
        for c in range(4):
            assert st.memobank[c][0].shape == (1, 496) and not bool(st.memobank[c][0].any()), c
    finally:
        for n, v in saved.items():
            setattr(ops, n, v)
        torch.cuda.empty_cache()
