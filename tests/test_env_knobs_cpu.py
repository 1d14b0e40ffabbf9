"""The environment variables that the C-ABI library reads: every getenv("ARCO_...") of arco_amd/csrc is documented in INTEGRATION.md,
and none of the retired A/B knobs of the convolution dispatch is read (or named) there any more.  RETIRED is the only place where the
old names live on: each experiment is decided, the dispatchers do what the default did."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arco_amd", "csrc")

# name: what the dispatcher does now
RETIRED = {
    "ARCO_IGEMM_WANT": "512 workgroups wanted per launch", "ARCO_IGEMM_WANT3": "512 in split-bf16 mode too",
    "ARCO_IGEMM_256": "no 256-position flat tile", "ARCO_CONV_HALO": "halo kernels on", "ARCO_CONV1X1_STREAM": "narrow 1x1 streams on",
    "ARCO_GEMM224": "64 x 224 tile", "ARCO_WGRAD_REDUCE4": "wgrad_reduce4_kernel on", "ARCO_CONV_RW16": "16 -> 16 on the resident-weights kernel",
    "ARCO_HWGRAD_TARGET": "512", "ARCO_HWGRAD1_TARGET": "512", "ARCO_WGRAD1_TARGET": "512", "ARCO_WGRAD_TARGET": "the 512 / 768 rule",
    "ARCO_WGRAD_FLAT_SPLIT": "split kernel on narrow planes", "ARCO_WGRAD_Q": "wgrad_q_kernel on", "ARCO_WGRAD_Q_TP": "64-pixel tiles",
    "ARCO_CONV3D_RW": "conv3d_rw16_kernel on", "ARCO_CONV_SP_TILES": "192 work items", "ARCO_CONV_SP_MINN": "16", "ARCO_CONV_RW": "on",
    "ARCO_CONV_RW_NARROW": "on", "ARCO_CONV_RW8": "eight MFMA waves everywhere", "ARCO_CONV3D_FC": "per-chunk form on",
    "ARCO_CONV3D_FL_NO5": "320-position tiles stay", "ARCO_CONV3D_DW": "depth-walking form deleted", "ARCO_CONV3D_DW_S": "deleted with it",
    "ARCO_HCONV_WANT": "256", "ARCO_HCONV2_WANT": "256", "ARCO_HCONV_256": "256-pixel tiles on", "ARCO_HCONV_FC": "on",
    "ARCO_HCONV_FC_BIG": "320 / 384-position tiles on", "ARCO_HCONV_RW": "16 channels on 8 x 16 tiles only",
    # process flags that keep their setter (arco_conv_sp_set, arco_conv3d_fl_set, arco_gemm_sp_set) and lose the environment read
    "ARCO_CONV_SP": "arco_conv_sp_set", "ARCO_CONV3D_FL": "arco_conv3d_fl_set", "ARCO_GEMM_SP": "arco_gemm_sp_set",
    "ARCO_GEMM_SP_TILES": "arco_gemm_sp_set",
    # compile-time switches (-D...) of decided experiments; the findings stand in the comments of split_bf16.h, interp.h, wgrad.hip, conv_h.hip
    "ARCO_AC_FAST": "contraction off in ac_src", "ARCO_SPLIT_TRUNC0": "first term rounded to nearest", "ARCO_SPLIT_RNE": "truncated second term",
    "ARCO_SPLIT_PACKED": "element-wise form gone with the all-RNE split", "ARCO_HCONV_ROWS_48_80": "rows of 8 / 24 dwords",
    "ARCO_WG_SWZ": "swizzled rows (constexpr WG_SWZ)", "ARCO_WG_CSZ": "72 (constexpr WG_CSZ)", "ARCO_WG_CSX": "136 (constexpr WG_CSX)",
}


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) >= 10
    return {f: open(f, encoding="utf-8").read() for f in files}


def test_every_variable_the_library_reads_is_documented():
    read = set()
    for text in _sources().values():
        read |= set(re.findall(r'getenv\(\s*"(ARCO_[A-Z0-9_]+)"', text))
    assert {"ARCO_CONV3D_FL_CFG", "ARCO_HCONV_FC_CFG"} <= read          # the two forcing variables of the tile-shape tests stay
    doc = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    documented = set(re.findall(r"ARCO_[A-Z0-9_]+", doc))
    assert read <= documented, sorted(read - documented)
    assert not read & set(RETIRED), sorted(read & set(RETIRED))


def test_no_retired_knob_is_named_in_the_library_sources():
    for path, text in _sources().items():
        names = set(re.findall(r"ARCO_[A-Z0-9_]+", text))           # whole identifiers: ARCO_CONV3D_FL_CFG is not ARCO_CONV3D_FL
        assert not names & set(RETIRED), (os.path.basename(path), sorted(names & set(RETIRED)))
