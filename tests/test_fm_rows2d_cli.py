"""--fm_rows f16 of the 2-D trainer: the command line, the refused combinations (no GPU needed: the stepper's constructor checks its
arguments before it touches the device) and the C ABI of the two f16-`hi` row kernels."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("arco_gather_upcat_rows_h", "arco_lerp4_cat_rows_h")


def test_parser_accepts_fm_rows():
    from arco_amd import train_arco_2d as T
    a = T.build_parser().parse_args(["--act_dtype", "f16", "--fm_rows", "f16"])
    assert a.fm_rows == "f16" and a.act_dtype == "f16"
    assert T.build_parser().parse_args([]).fm_rows == "f32"                       # opt-in: the default is unchanged
    assert T.build_parser().parse_args(["--act_dtype", "f16"]).fm_rows == "f32"   # ... also with f16 storage
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--fm_rows", "bf16"])


@pytest.mark.parametrize("extra,names", [([], ("--fm_rows f16", "--act_dtype f16")),
                                          (["--act_dtype", "f16", "--dense_head", "1"], ("--fm_rows f16", "--dense_head 1")),
                                          (["--act_dtype", "f16", "--revisit", "1"], ("--fm_rows f16", "--revisit 1")),
                                          (["--act_dtype", "f16", "--dense_teacher", "1"], ("--fm_rows f16", "--dense_teacher 1"))])
def test_refused_combinations_name_their_flags(extra, names):
    from arco_amd import ops, train_arco_2d as T
    args = T.build_parser().parse_args(["--synthetic", "1", "--fm_rows", "f16"] + extra)
    try:
        with pytest.raises(ValueError) as e:
            T.ArcoStep2D(args, "cpu")
        assert all(n in str(e.value) for n in names), str(e.value)
        assert not ops.ACT_HALF                 # a refused constructor leaves no f16 switch behind
        assert ops.FM_CAST is True
    finally:
        ops.ACT_HALF = False


def test_fm_rows_half_count_form():
    """ops.fm_rows_half(k): the U-Net's count form sets ('keep', k) - distinct from True in a graph's capture key although 1 == True -
    and restores the previous value; without an argument it is the V-Net's 'lowres', as before."""
    from arco_amd import ops
    assert ops.FM_CAST is True
    with ops.fm_rows_half(3):
        assert ops.FM_CAST == ("keep", 3) and ops.FM_CAST != True and ops.FM_CAST      # noqa: E712
        with ops.logits_only():
            assert ops.FM_CAST is False
        assert ops.FM_CAST == ("keep", 3)
    assert ops.FM_CAST is True
    with ops.fm_rows_half(1):
        assert hash(ops.FM_CAST) != hash(True) or ops.FM_CAST != True                  # noqa: E712
    with ops.fm_rows_half():
        assert ops.FM_CAST == "lowres"
    assert ops.FM_CAST is True
    for bad in (0, 5):
        with pytest.raises(ValueError):
            ops.fm_rows_half(bad)


def test_new_entry_points_declared_and_registered():
    from arco_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "arco_hip.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        base = name[:-2]
        assert name in L._SIGS and L._SIGS[name] == L._SIGS[base], name      # same argument list as the fp32 entry point (hi: a pointer)


def test_new_entry_points_exported():
    """The built library exports both (tests/test_cabi_exports.py checks the whole table against the header)."""
    import ctypes
    from arco_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(L.LIB_PATH + " is not built")
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
