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
