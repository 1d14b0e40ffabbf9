"""--act_dtype f16 of the 2-D trainer: the command line and the refused combinations (no GPU needed: the stepper's constructor
checks its arguments before it touches the device)."""
import pytest


def test_parser_accepts_act_dtype_and_loss_scale():
    from arco_amd import train_arco_2d as T
    a = T.build_parser().parse_args(["--act_dtype", "f16", "--loss_scale", "1024"])
    assert a.act_dtype == "f16" and a.loss_scale == 1024.0
    d = T.build_parser().parse_args([])
    assert d.act_dtype == "f32" and d.loss_scale == 16384.0          # opt-in: the default is unchanged
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--act_dtype", "bf16"])


def test_3d_parser_keeps_its_flags_and_defaults():
    from arco_amd import train_arco_3d as T3
    a = T3.build_parser().parse_args(["--act_dtype", "f16"])
    assert (a.act_dtype, a.loss_scale, a.head_mma) == ("f16", 16384.0, "auto")
    assert T3.build_parser().parse_args([]).act_dtype == "f32"
    assert "V-Net" in next(x for x in T3.build_parser()._actions if x.dest == "act_dtype").help


@pytest.mark.parametrize("extra,names", [(["--dense_head", "1"], ("--act_dtype f16", "--dense_head 1")),
                                          (["--revisit", "1"], ("--act_dtype f16", "--revisit 1"))])
def test_refused_combinations_name_their_flags(extra, names):
    from arco_amd import ops, train_arco_2d as T
    args = T.build_parser().parse_args(["--synthetic", "1", "--act_dtype", "f16"] + extra)
    try:
        with pytest.raises(ValueError) as e:
            T.ArcoStep2D(args, "cpu")
        assert all(n in str(e.value) for n in names), str(e.value)
        assert not ops.ACT_HALF                 # a refused constructor leaves no f16 switch behind
    finally:
        ops.ACT_HALF = False


def test_both_steppers_share_one_loss_scale_guard():
    from arco_amd import train_arco_2d as T, train_arco_3d as T3
    from arco_amd.loss_scale import LossScaleGuard
    for name in ("_unscale_and_guard", "_guard_heads_and_publish", "_loss_scale_update", "_recapture_train_graphs"):
        assert getattr(T.ArcoStep2D, name) is getattr(LossScaleGuard, name) is getattr(T3.ArcoStep3D, name)


def test_both_steppers_share_one_base():
    """What arco_amd/stepper.py owns is ONE function object for both ranks (the same identity check as the loss-scale one): the
    writer of the mode switches, banks, heads / optimizer / plans, the graphed passes both have, head and tail of a step, q_rep, the
    side-stream accessor.  The per-rank points of the tail are overridden where - and only where - a rank waits for something."""
    from arco_amd import train_arco_2d as T, train_arco_3d as T3
    from arco_amd.stepper import ArcoStepBase
    assert issubclass(T.ArcoStep2D, ArcoStepBase) and issubclass(T3.ArcoStep3D, ArcoStepBase)
    for name in ("_set_modes", "_build_banks", "_build_heads", "_build_graphs", "_step_head", "_step_tail", "q_rep", "_stream"):
        assert getattr(T.ArcoStep2D, name) is getattr(ArcoStepBase, name) is getattr(T3.ArcoStep3D, name), name
    assert T.ArcoStep2D._before_backward is not ArcoStepBase._before_backward           # the optional SIDE_SYNC wait
    assert T.ArcoStep2D._after_backward is not ArcoStepBase._after_backward             # side-stream wait, merge_second
    assert T3.ArcoStep3D._before_backward is ArcoStepBase._before_backward
    assert T3.ArcoStep3D._after_backward is not ArcoStepBase._after_backward            # the _tps_pending wait
    assert T.ArcoStep2D._make_tps is not T3.ArcoStep3D._make_tps


def test_train_and_main_are_bindings_of_the_shared_drivers(monkeypatch):
    """train_arco_2d.train / .main and train_arco_3d.train / .main (importable without a GPU) hand their own stepper class, synthetic
    batch function, build_loaders and parser to stepper.train / stepper.main and add nothing."""
    from arco_amd import stepper, train_arco_2d as T, train_arco_3d as T3
    calls = []
    monkeypatch.setattr(stepper, "train", lambda *a: calls.append(("train",) + a) or "t")
    monkeypatch.setattr(stepper, "main", lambda *a: calls.append(("main",) + a) or "m")
    args = object()
    assert T.train(args, "snap") == "t" and T3.train(args, "snap3") == "t"
    assert T.main(["--synthetic", "1"]) == "m" and T3.main() == "m"
    assert calls == [("train", args, "snap", T.ArcoStep2D, T.synthetic_batch, T.build_loaders),
                     ("train", args, "snap3", T3.ArcoStep3D, T3.synthetic_volume_batch, T3.build_loaders),
                     ("main", ["--synthetic", "1"], T.build_parser, T.train),
                     ("main", None, T3.build_parser, T3.train)]


@pytest.mark.parametrize("case", ["fm_rows_without_act_dtype", "conv_mma_bf16"])
def test_refused_2d_constructor_changes_no_switch(case):
    """The 2-D constructor writes the five process-wide switches of arco_amd.ops once, after its flag validation: refused, it leaves
    every one of them as it found it (set to values no 2-D stepper would write, so an early write could not hide)."""
    from arco_amd import ops, train_arco_2d as T
    names = ("CONV_MMA", "ACT_HALF", "HEAD_MMA", "LOSS_SCALE", "WGRAD_SIDE")
    saved = {n: getattr(ops, n) for n in names}
    if case == "fm_rows_without_act_dtype":
        args = T.build_parser().parse_args(["--synthetic", "1", "--fm_rows", "f16", "--loss_scale", "1024"])
    else:
        args = T.build_parser().parse_args(["--synthetic", "1", "--loss_scale", "1024"])
        args.conv_mma = "bf16"               # (the 2-D parser rejects it: a hand-made namespace, as the benchmark builds them)
    before = dict(CONV_MMA=1, ACT_HALF=True, HEAD_MMA=2, LOSS_SCALE=4.0, WGRAD_SIDE=2)
    try:
        for n, v in before.items():
            setattr(ops, n, v)
        with pytest.raises(ValueError):
            T.ArcoStep2D(args, "cpu")
        assert {n: getattr(ops, n) for n in names} == before
    finally:
        for n, v in saved.items():
            setattr(ops, n, v)
