"""Do two builds of the C-ABI library choose the same kernels?  python tools/route_sweep.py <libA.so> <libB.so>

For each library one child interpreter (ARCO_LIB selects it) calls the host-side route queries over a grid of shapes and the parent
prints the points where the two disagree.  Forward: arco_conv_config_mma, arco_conv_mblocks_mma (1 and 2 BatchNorm groups),
arco_conv_mblocks_pro and arco_conv_split_ok under each combination of arco_conv3d_fl_set(0|1) x arco_conv_sp_set(0|1); weight
gradient: arco_wgrad_config (route, slabs, slab_floats, reduce) for entries 0 and 1.  The queries are pure host functions; without a
device the CU count falls back to 256, the MI355X's figure, so the table is the one the GPU machine would produce.  The launch-only
routes (gemm_sp_kernel, the 1x1 streams) have no query: the route assertions of tests/test_conv_kernels_gpu.py cover them."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBS = (1, 2, 8, 48, 96)
PLANES = ((7, 5), (14, 10), (28, 20), (56, 40), (10, 6), (20, 12), (40, 24), (80, 48), (33, 45), (16, 16), (32, 32), (64, 64),
          (128, 128), (256, 256))
CHANS = ((1, 16), (3, 16), (4, 16), (16, 4), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128),
         (256, 256), (20, 48), (240, 240), (448, 448), (496, 496))
TAPS = (1, 9, 27)


def _ld(c, pad, mma):
    ld = c + pad
    return (ld + 7) // 8 * 8 if mma == 4 else ld


def sweep():
    sys.path.insert(0, ROOT)
    from arco_amd import _lib as L
    lib = L.load()
    table = {}
    for fl, sp in itertools.product((0, 1), (0, 1)):
        lib.arco_conv3d_fl_set(fl); lib.arco_conv_sp_set(sp)
        for taps, mma, nb, (h, w), (ci, co), pad in itertools.product(TAPS, (0, 3, 4), NBS, PLANES, CHANS, (0, 4)):
            ld = _ld(ci, pad, mma)
            table["f %d %d | %d %d %d %d %d %d %d %d" % (fl, sp, taps, mma, nb, h, w, ci, co, ld)] = (
                lib.arco_conv_config_mma(taps, nb, h, w, ci, co, ld, mma),
                lib.arco_conv_mblocks_mma(taps, nb, h, w, ci, co, ld, 1, mma),
                lib.arco_conv_mblocks_mma(taps, nb, h, w, ci, co, ld, 2, mma),
                lib.arco_conv_mblocks_pro(taps, nb, h, w, ci, co, ld, 1, mma, 1),
                lib.arco_conv_mblocks_pro(taps, nb, h, w, ci, co, ld, 2, mma, 2),
                lib.arco_conv_split_ok(taps, nb, h, w, ci, co, ld))
    lib.arco_conv3d_fl_set(1); lib.arco_conv_sp_set(1)
    slabs, sf, red = ctypes.c_long(), ctypes.c_long(), ctypes.c_int()
    for taps, mma, nb, (h, w), (ci, co), pad, pro, al in itertools.product(TAPS, (0, 2, 3, 4), NBS, PLANES, CHANS, (0, 4), (0, 2), (0, 1)):
        d3 = 2 if taps == 27 and nb % 2 == 0 else 1
        nv = nb // d3
        ld_in, ld_dz = _ld(ci, pad, mma), _ld(co, pad, mma)
        for entry in (0, 1):
            if entry == 1 and not (ci <= 4 and d3 == 1 and taps == 9):
                continue
            slabs.value = sf.value = -1; red.value = -1
            r = lib.arco_wgrad_config(entry, taps, nv, d3, h, w, ci, co, ld_dz, ld_in, mma, pro, al, ctypes.byref(slabs), ctypes.byref(sf),
                                      ctypes.byref(red))
            table["w %d | %d %d %d %d %d %d %d %d %d %d %d %d" % (entry, taps, mma, nv, d3, h, w, ci, co, ld_dz, ld_in, pro, al)] = (
                r, slabs.value, sf.value, red.value)
    return table


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        json.dump(sweep(), open(sys.argv[2], "w"))
        return 0
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    import tempfile
    tables = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(sys.argv[1:3]):
            out = os.path.join(tmp, "t%d.json" % i)
            env = {k: v for k, v in os.environ.items() if not k.startswith("ARCO_")}
            env["ARCO_LIB"] = os.path.abspath(lib)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, check=True)
            tables.append(json.load(open(out)))
    a, b = tables
    diff = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    for k in diff[:50]:
        print("DIFF", k, a.get(k), b.get(k))
    nf = sum(k.startswith("f") for k in a); nw = sum(k.startswith("w") for k in a)
    routes = len({v[0] for k, v in a.items() if v[0] > 0})
    print("forward points %d, weight-gradient points %d, distinct routes %d, differences %d" % (nf, nw, routes, len(diff)))
    return 1 if diff or set(a) != set(b) else 0


if __name__ == "__main__":
    sys.exit(main())
