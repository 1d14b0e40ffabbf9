"""The C-ABI library loads on a CPU-only host and exports every symbol include/arco_hip.h declares."""
import ctypes
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_header_symbols():
    from arco_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "arco_hip.h")).read()
    declared = set(re.findall(r"\b(arco_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert "arco_conv_last_route" in declared          # the test-facing record of the kernel a forward launch took
    assert isinstance(_lib.query("arco_conv_last_route"), int)
    assert {"arco_wgrad_config", "arco_wgrad_last_route"} <= declared      # ... and of the weight-gradient route, with its query
    assert isinstance(_lib.query("arco_wgrad_last_route"), int)
    assert _lib.query("arco_wgrad_config", 0, 9, 1, 1, 16, 16, 16, 16, 16, 16, 0, 0, 1, None, None, None) == 9201616


def test_library_defines_only_declared_symbols():
    """The other direction: every dynamic function symbol arco_* that the built library defines is declared in the header."""
    from arco_amd import _lib
    nm = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "neither nm nor llvm-nm found: cannot read the library's symbols"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {f[2] for f in (ln.split() for ln in out.splitlines()) if len(f) == 3 and f[1] in "TW" and f[2].startswith("arco_")}
    assert len(defined) > 100, len(defined)
    assert defined == set(_lib.EXPORTS), defined ^ set(_lib.EXPORTS)      # EXPORTS: the header's declarations (the test above)


def test_missing_library_fails_loudly(monkeypatch):
    from arco_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libarco_hip.so")
    import pytest
    with pytest.raises(RuntimeError):
        _lib.load()
