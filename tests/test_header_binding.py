"""arco_amd/_lib.py derives its ctypes tables from include/arco_hip.h: the parser is held to rows written out by hand from the
declarations, to its refusals on text it cannot read, and the ctypes mirror of ArcoActPro to the header's struct."""
import ctypes
import os
import re

import pytest

from arco_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "arco_hip.h")
P, I, L, F, D, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_uint64

# one row per construct of the header, each typed from its declaration; the last letter of a call is the stream
CALLS = {
    "arco_bn_act_bwd": [P, L, P, L, L, I, P, P, P, P, F, I, F, U64, L, P, P, P, I, P, L, P, I, P],
    "arco_surface_sp_dist": [P, P, I, I, I, I, I, D, D, D, I, I, P, L, P, P, L, P, P],
    "arco_conv3d_fwd_pro": [P, L, I, P, I, P, L, P, P, L, P, P, I, I, I, I, I, I, I, P, P],      # const ArcoActPro* pro, then the stream
    "arco_conv1x1_upres_fwd": [P, L, I, P, I, P, L, P, L, I, I, I, I, I, I, I, P],
}
QUERIES = {
    "arco_proto_ws_floats": ([L, I, I], L),
    "arco_grid_sample_many_finish": ([], None),
    "arco_wgrad_config": ([I, I, I, I, I, I, I, I, L, L, I, I, I, P, P, P], I),      # ends in a pointer that is no stream
    "arco_conv_last_route": ([], I),
}


@pytest.fixture(scope="module")
def tables():
    with open(HEADER) as f:
        return _lib.parse_header(f.read())


@pytest.mark.parametrize("name", sorted(CALLS))
def test_call_rows(tables, name):
    sigs, queries = tables
    assert name not in queries
    assert sigs[name] == CALLS[name], name


@pytest.mark.parametrize("name", sorted(QUERIES))
def test_query_rows(tables, name):
    sigs, queries = tables
    assert name not in sigs
    assert tuple(queries[name]) == QUERIES[name], name


def test_module_tables_are_the_parsed_header(tables):
    sigs, queries = tables
    assert _lib._SIGS == sigs and _lib._QUERIES == queries
    assert _lib.EXPORTS == sorted(list(sigs) + list(queries)) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    assert not set(sigs) & set(queries)
    assert all(a[-1] is P for a in sigs.values())          # the stream that `call` appends


def test_small_header():
    sigs, queries = _lib.parse_header("""
        /* int arco_in_a_comment(int n); */
        #include <stdint.h>
        typedef struct S { const float* a; int n; } S;   // int arco_in_a_line_comment(void);
        int arco_a(const float* x, long n, const S* s,
                   uint64_t seed /* a comment, with a comma */, double q, void * stream);
        long arco_b();
        void arco_c(void);
        int arco_d(float alpha, int* out);
    """)
    assert sigs == {"arco_a": [P, L, P, U64, D, P]}
    assert queries == {"arco_b": ([], L), "arco_c": ([], None), "arco_d": ([F, P], I)}


def test_unmapped_parameter_type_names_the_function():
    with pytest.raises(RuntimeError, match="arco_narrow"):
        _lib.parse_header("int arco_ok(int n, void* stream);\nint arco_narrow(const float* x, short n, void* stream);")
    with pytest.raises(RuntimeError, match="arco_wide"):
        _lib.parse_header("int arco_wide(unsigned long long n);")
    with pytest.raises(RuntimeError, match="arco_ret"):
        _lib.parse_header("short arco_ret(int n);")
    with pytest.raises(RuntimeError, match="arco_status"):          # `call` reads an int status from whatever takes a stream
        _lib.parse_header("long arco_status(int n, void* stream);")


@pytest.mark.parametrize("text", [
    "int arco_ok(int n, void* stream);\nint arco_cb(int (*fn)(int), void* stream);",      # parentheses inside the parameter list
    "int arco_ok(int n, void* stream);\nint arco_open(int n\nlong arco_next(void);",          # a declaration that never closes
    "int arco_ok(int n);\nint arco_ok(long n);",                                             # declared twice
])
def test_unreadable_declaration_trips_the_count(text):
    with pytest.raises(RuntimeError, match="declarations read"):
        _lib.parse_header(text)


@pytest.mark.parametrize("text", ["", "/* int arco_gone(int n); */\n#define ARCO_X 1\ntypedef struct T { int n; } T;\n"])
def test_header_without_declarations(text):
    with pytest.raises(RuntimeError, match="declarations read"):
        _lib.parse_header(text)


def test_missing_header_names_the_path(tmp_path):
    path = str(tmp_path / "include" / "arco_hip.h")
    with pytest.raises(RuntimeError, match=re.escape(path)):
        _lib.read_header(path)


def test_act_pro_mirrors_the_header_struct():
    """ArcoActPro: four pointers, four 4-byte scalars, a uint64, a pointer - the layout csrc/igemm_args.h asserts for the kernels."""
    assert ctypes.sizeof(_lib.ActPro) == 64 and _lib.ActPro.seed.offset == 48
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+ArcoActPro\s*\{(.*?)\}\s*ArcoActPro\s*;", text, flags=re.S).group(1)
    fields = [(re.search(r"(\w+)\s*$", d).group(1), "*" in d) for d in body.split(";") if d.strip()]
    assert [n for n, _ in fields] == ["mean", "istd", "gamma", "beta", "slope", "groups", "drop_mode", "p", "seed", "seed_dev"]
    assert [n for n, _ in fields] == [f[0] for f in _lib.ActPro._fields_]
    assert [ptr for _, ptr in fields] == [f[1] is P for f in _lib.ActPro._fields_]
