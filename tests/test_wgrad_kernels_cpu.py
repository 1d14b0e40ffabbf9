"""The CPU half of the weight-gradient kernel tests (tests/wgrad_kernel_refs.py, tests/test_wgrad_kernels_gpu.py): no GPU is touched.

  routes        every case's kernel id, slab size and reduction kernel through arco_wgrad_config - the function the launch itself calls
  slab sweep    slabs * floats_per_slab <= arco_wgrad_ws_floats and slabs >= 1 over the whole grid taps {1, 9, 27} x mma 0..4 x Cout, Cin
                {1, 4, 16, 20, 32, 64, 192} x NB {1, 7, 64, 200, 512, 2000} x H, W {1, 2, 4, 7, 16, 17, 40, 64, 250} x aligned | odd strides
                (714 420 shapes), each compared with the dispatcher's earlier formulas restated below (one slab per tile up to the
                target, wgrad_q_kernel's own check included): slabs == min(earlier, reserved); and over the six shapes of many small
                planes for which the earlier formulas exceed the reservation
  unchanged     for every convolution that the U-Net and the V-Net declare (read from the modules) at every level's size of a 256 x 256
                image and of the LA (112 x 112 x 80) and LiTS (160 x 160 x 96) patches, in mma 0, 3, 4 and with the consumer-side
                activation, the slab count equals the earlier formulas': the clamp changes no launch of the trainers
  inputs        the exactness budget of the fixed kind, the placing of the impulses, f16 operands generated as f16
  emulation     the wide kind summed in fp32 (chains of P pixels, a balanced tree; arco_colsum: its rstep chains per block, float64 across
                blocks) stays inside the bounds the GPU file uses
  planted       a dropped last tile, a plane from the neighbouring volume, a transposed tap, an omitted slab, accumulate ignored and a
                leaking pad channel are each caught by the helpers the GPU file uses
  rejections    null pointers, taps, mma, sizes and strides (ARCO_ERR_ARG) and the listed ARCO_ERR_UNSUPPORTED cases of every entry point

Worst err / bound of the fp32 emulation per route (the bound's constant is min(gamma(n), 9 sqrt(n) u), wgrad_kernel_refs.py):
  wgrad_kernel 0.047; wgrad_halo2_kernel fp32 0.047 (rectangular), 0.038 (flat), bf16 operands 0.61 / 0.64; wgrad_split_kernel 0.057, with
  the activation 0.033; wgrad_image3d_kernel<1> 0.020, <3> 0.033; hwgrad_kernel<.,.,9> 0.077 (taps 9), 0.113 (taps 27), <.,.,1> 0.055;
  himage_wgrad_kernel 0.031; colsum_partial_kernel in its own per-block order 0.20 (C = 1024, one row), otherwise <= 0.03.
  (The MI355X figures are in the header of tests/test_wgrad_kernels_gpu.py.)"""
import ctypes
import itertools

import pytest
import torch

import wgrad_kernel_refs as R
from conv_kernel_refs import ERR_ARG, ERR_UNSUPPORTED, equal_bits, im2col
from loss_kernel_refs import worst


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


def config(L, entry, taps, nv, d3, h, w, cin, cout, ldz, ldi, mma, pro=0, aligned=1):
    s, f, r = ctypes.c_long(), ctypes.c_long(), ctypes.c_int()
    route = L.query("arco_wgrad_config", entry, taps, nv, d3, h, w, cin, cout, ldz, ldi, mma, pro, aligned, ctypes.byref(s), ctypes.byref(f), ctypes.byref(r))
    return route, s.value, f.value, r.value


def case_config(L, c, aligned=1):
    return config(L, c["entry"], c["taps"], c["nv"], c["d3"], c["h"], c["w"], c["k"], c["n"], c["ld_dz"], c["ld_in"], c["mma"], c["pro"], aligned)


# ---- the dispatcher's earlier formulas: one slab per workgroup, min(target / (ydim zdim), n_tiles) workgroups ------------------------------
def earlier_slabs(taps, NB, H, W, cin, cout, ldz, ldi, mma, need):
    """slabs the launch wrote before the clamp (conv3d_wgrad_impl / hwgrad_dispatch as they were; entry 0, aligned operands, no
    environment knobs); need = arco_wgrad_ws_floats of the shape, which only the wgrad_q branch consulted"""
    M = NB * H * W
    up = lambda v, m: -(-v // m) * m
    if mma == 4 and not (taps >= 9 and cin == 1):
        if taps >= 9:
            hco, hci = (32 if cout > 16 else 16), (32 if cin > 16 else 16)
            y = (up(cout, hco) // hco) * (up(cin, hci) // hci)
            return max(1, min(512 // ((taps // 9) * y), NB * -(-H // 8) * -(-W // 16)))
        cb = lambda v: 64 if v >= 64 else (32 if v > 16 else 16)
        y = (up(cout, cb(cout)) // cb(cout)) * (up(cin, cb(cin)) // cb(cin))
        return min(max(1, 512 // y), -(-M // 128))
    if taps >= 9 and cin == 1 and cout <= 16 and cout % 4 == 0 and ldz % 4 == 0:
        return min(512, NB * -(-H // 16) * -(-W // 16))
    if taps >= 9:
        hco, hci = (32 if cout > 16 else 16), (32 if cin > 16 else 16)
        split_ok = mma == 3 and cout % 4 == 0 and cin % 4 == 0 and ldz % 4 == 0 and ldi % 4 == 0
        flat = W % 16 != 0 and W + 2 <= 64 and not (split_ok and W >= 10)
        tiles = NB * -(-(H * (W + 2)) // 128) if flat else NB * -(-H // 8) * -(-W // 16)
        y = (up(cout, hco) // hco) * (up(cin, hci) // hci)
        target = 512 if (hci == 32 and (hco == 32 or mma == 3)) else 768
        return max(1, min(target // ((taps // 9) * y), tiles))
    cb = lambda v: 64 if v >= 64 else (32 if v > 16 else 16)
    tiles = -(-M // 128)
    if cout >= 192 and cin >= 192 and M >= 32768 and cout % 4 == 0 and cin % 4 == 0 and ldz % 4 == 0 and ldi % 4 == 0:
        cop, cip = up(cout, 128), up(cin, 128)            # wgrad_q_kernel<64>: it checked its slabs against the reservation itself
        yzq = (cop // 128) * (cip // 128)
        chq = min(max(1, 256 // yzq), tiles)
        if chq * cop * cip <= need:
            ch2 = min(max(1, 512 // yzq), -(-M // 64))
            return ch2 if ch2 * cop * cip <= need else chq
    yz = (up(cout, cb(cout)) // cb(cout)) * (up(cin, cb(cin)) // cb(cin)) * taps
    return min(max(1, 512 // yz), tiles)


# ======================================================================================================================================
@pytest.mark.parametrize("c", R.CASES, ids=R.NAMES)
def test_route_of_every_case(L, c):
    route, slabs, sf, red = case_config(L, c)
    assert route == c["route"], (c["name"], route)
    assert sf == R.slab_floats(c)
    need = L.query("arco_wgrad_ws_floats", c["n"], c["k"], c["taps"], c["M"])
    assert 1 <= slabs <= R.target_slabs(c) and slabs * sf <= need
    assert slabs <= R.n_tiles(c)
    assert not c["red"] or red == c["red"], (c["name"], red)
    assert red == (1 if slabs <= 16 else (3 if c["k"] % 4 == 0 and c["n"] * c["k"] * c["taps"] >= 4096 else 2))
    if c["fam"] == R.F_Q:                              # the operands' 16-byte alignment is part of the decision
        assert case_config(L, c, aligned=0)[0] == R.rid(1, R.F_GEMM, 0, 64, 64)
    if c["entry"] == 1:
        assert case_config(L, c, aligned=0)[0] == ERR_UNSUPPORTED


def test_every_family_and_tile_has_a_case():
    have = {c["route"] for c in R.CASES}
    want = {R.rid(1, R.F_GEMM, 0, a, b) for a in (16, 32, 64) for b in (16, 32, 64)} | {R.rid(1, R.F_Q, 0, 0, 64)}
    want |= {R.rid(9, R.F_HALO, v, a, b) for v in range(4) for a in (16, 32) for b in (16, 32)}
    want |= {R.rid(9, R.F_SPLIT, v, a, b) for v in range(2) for a in (16, 32) for b in (16, 32)}
    want |= {R.rid(9, R.F_IMAGE, 1, 16, 16), R.rid(9, R.F_IMAGE, 3, 16, 16)} | {R.rid(9, R.F_HIMAGE, 0, 16, k) for k in (1, 2, 3, 4)}
    want |= {R.rid(9, R.F_HGRAD, 0, a, b) for a in (16, 32) for b in (16, 32)} | {R.rid(1, R.F_HGRAD, 0, a, b) for a in (16, 32, 64) for b in (16, 32, 64)}
    assert want <= have, sorted(want - have)
    for fam in (R.F_HALO, R.F_SPLIT, R.F_HGRAD):       # volume geometry at taps 27: one plane, two planes, two volumes of three
        geo = {(c["nv"], c["d3"]) for c in R.CASES if c["fam"] == fam and c["taps"] == 27}
        assert {(1, 1), (1, 2), (2, 3)} <= geo, (fam, geo)


# ---- the slab sweep ------------------------------------------------------------------------------------------------------------------
CH = (1, 4, 16, 20, 32, 64, 192)
HW = (1, 2, 4, 7, 16, 17, 40, 64, 250)
TABLE = [c for c in R.CASES if c["table"]]


@pytest.mark.parametrize("taps,mma,h", [(t, m, h) for t in (1, 9, 27) for m in range(5) for h in HW])
def test_slab_sweep(L, taps, mma, h):
    """the whole grid: taps x mma x Cout x Cin x NB x H x W x (aligned | odd strides), 714 420 shapes, each compared with the earlier formulas"""
    n = 0
    ws_floats = L.load().arco_wgrad_ws_floats
    for cout, cin, nb, w, odd in itertools.product(CH, CH, (1, 7, 64, 200, 512, 2000), HW, (0, 1)):
        ldz, ldi = cout + odd, cin + (odd if mma != 4 else 0)
        route, slabs, sf, red = config(L, 0, taps, nb, 1, h, w, cin, cout, ldz, ldi, mma)
        if route == ERR_UNSUPPORTED:                       # f16 storage: Cin % 8, odd ld_dz off the 3x3, f16 dZ on an fp32 kernel (Cin = 1)
            assert mma == 4 and (cin % 8 != 0 or (ldz % 2 and taps != 9)) and not (taps >= 9 and cin == 1 and cout in (4, 16) and not odd)
            continue
        need = ws_floats(cout, cin, taps, nb * h * w)
        assert route > 0 and slabs >= 1 and slabs * sf <= need, (taps, mma, cout, cin, nb, h, w, ldz, slabs, sf, need)
        # the clamp only ever lowers the count, and only where the reservation was exceeded
        was = earlier_slabs(taps, nb, h, w, cin, cout, ldz, ldi, mma, need)
        assert slabs == min(was, need // sf), (taps, mma, cout, cin, nb, h, w, slabs, was)
        n += 1
    assert n > (200 if mma == 4 else 5000)


def test_slab_sweep_image_entry(L):
    for k, nb, (h, w) in itertools.product((1, 2, 3, 4), (1, 7, 200, 2000), ((1, 1), (4, 4), (17, 40), (250, 250))):
        route, slabs, sf, _ = config(L, 1, 9, nb, 1, h, w, k, 16, 16, k, 4)
        assert route == R.rid(9, R.F_HIMAGE, 0, 16, k) and slabs >= 1
        assert slabs * sf <= L.query("arco_wgrad_ws_floats", 16, k, 9, nb * h * w)


@pytest.mark.parametrize("c", TABLE, ids=[c["name"] for c in TABLE])
def test_many_small_planes_exceeded_the_reservation(L, c):
    """the earlier formulas wrote one slab per tile: more than arco_wgrad_ws_floats reserves; the launch now takes what is reserved"""
    need = L.query("arco_wgrad_ws_floats", c["n"], c["k"], c["taps"], c["M"])
    was = earlier_slabs(c["taps"], c["nv"] * c["d3"], c["h"], c["w"], c["k"], c["n"], c["ld_dz"], c["ld_in"], c["mma"], need)
    route, slabs, sf, _ = case_config(L, c)
    assert was * sf > need, "the earlier dispatcher stayed inside the reservation here"
    assert slabs == need // sf < was and was <= R.target_slabs(c)


def model_convs(net):
    """(taps, Cin, Cout) of every convolution the model declares; a k2 s2 (transposed) convolution runs as the GEMM of its eight taps"""
    out = set()
    for m in net.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv3d)):
            k = m.kernel_size[0]
            out.add((1, m.in_channels * k ** len(m.kernel_size), m.out_channels) if m.stride[0] == 2 else (k ** len(m.kernel_size), m.in_channels, m.out_channels))
        elif isinstance(m, torch.nn.ConvTranspose3d):
            out.add((1, m.in_channels, m.out_channels * 8))
    return sorted(out)


def trainer_shapes():
    """(taps, NV, D3, H, W, Cin, Cout): every convolution that the U-Net (4 and 19 classes) and the V-Net declare, read from the modules
    themselves, at every level's size of a 256 x 256 image resp. of the LA (112 x 112 x 80) and LiTS (160 x 160 x 96) patches (the
    trainers' default --patch_size and the benchmark's LiTS configuration) - a superset of the (layer, level) pairs that occur"""
    from arco_amd.networks.unetWithArgs import UNet
    from arco_amd.networks.vnetWithArgs import VNet
    from arco_amd import train_arco_2d, train_arco_3d
    assert train_arco_2d.build_parser().get_default("patch_size") == [256, 256]
    assert train_arco_3d.build_parser().get_default("patch_size") == [112, 112, 80]
    out = []
    convs2 = sorted(set(model_convs(UNet(1, 4)) + model_convs(UNet(1, 19))))
    assert (9, 1, 16) in convs2 and (9, 256, 256) in convs2 and (9, 16, 19) in convs2
    for nb, lv, (taps, cin, cout) in itertools.product((2, 4, 8, 16), range(5), convs2):
        out.append((taps, nb, 1, 256 >> lv, 256 >> lv, cin, cout))
    out += [(1, nb, 1, 256, 256, 496, 496) for nb in (2, 4, 8)]          # the widest head GEMM (wgrad_q_kernel)
    convs3 = model_convs(VNet(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True))
    assert (27, 1, 16) in convs3 and (27, 256, 256) in convs3 and (1, 16, 2) in convs3
    for (h, w, d), nv, lv, (taps, cin, cout) in itertools.product(((112, 112, 80), (160, 160, 96)), (1, 2, 4), range(5), convs3):
        out.append((taps, nv, d >> lv, h >> lv, w >> lv, cin, cout))
    return out


def test_trainer_launches_are_unchanged(L):
    n = nq = npro = 0
    for (taps, nv, d3, h, w, cin, cout) in trainer_shapes():
        for mma, pro in ((0, 0), (3, 0), (4, 0), (3, 1), (3, 2)):
            ldi = cin if not (mma == 4 and cin % 8) else cin + 8 - cin % 8
            route, slabs, sf, _ = config(L, 0, taps, nv, d3, h, w, cin, cout, cout, ldi, mma, pro=pro)
            if route == ERR_UNSUPPORTED:
                continue
            need = L.query("arco_wgrad_ws_floats", cout, cin, taps, nv * d3 * h * w)
            was = earlier_slabs(taps, nv * d3, h, w, cin, cout, cout, ldi, mma, need)
            assert slabs == was, (taps, nv, d3, h, w, cin, cout, mma, pro, slabs, was)
            n, nq, npro = n + 1, nq + ((route // 100000) % 10 == R.F_Q), npro + (pro > 0)
    assert n > 2000 and nq >= 3 and npro > 20, (n, nq, npro)


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------
SMALL = [c for c in R.CASES if c["M"] * c["k"] * c["taps"] <= 2 ** 21 and not c["pro"]]


@pytest.mark.parametrize("c", SMALL, ids=[c["name"] for c in SMALL])
def test_input_conditions(c):
    d = R.data(c, "fixed")
    assert R.exactness_budget(c, d) < 2 ** 24
    assert bool((d["ref"] / R.QUANT == (d["ref"] / R.QUANT).round()).all())
    assert d["dz"].dtype == (torch.float16 if c["zh"] else torch.float32) and d["x"].dtype == (torch.float16 if c["xh"] else torch.float32)
    if c["fam"] == R.F_SPLIT:                          # both kept planes of both operands take part
        from conv_kernel_refs import n_terms, split_act
        assert int(n_terms(split_act(d["dz"].numpy())).max()) == 2 and int(n_terms(split_act(d["x"].numpy())).max()) == 2
    if "impulse" not in c["kinds"]:
        return
    pos = R.impulse_pixels(c)
    assert len(set(pos)) == len(pos) and pos[0] == 0 and pos[1] == c["M"] - 1
    planes = {p // (c["h"] * c["w"]) % c["d3"] for p in pos}
    assert {0, c["d3"] - 1} <= planes
    for kind in ("impulse", "impulse_x"):
        d = R.data(c, kind)
        unit = d["dz"] if kind == "impulse" else d["x"]
        assert bool((unit.sum(0) <= 1).all()) and float(unit.sum()) == len(d["pos"]) >= 1
        assert torch.equal(R.impulse_expected(c, d) + d["dw0"].double(), d["ref"])      # one operand row or zero per element
        full = (d["x"] if kind == "impulse" else d["dz"]).float()
        if not (c["zh"] or c["xh"]):                   # full 24-bit values: plane 2 of the split
            from conv_kernel_refs import n_terms, split_act
            assert int(n_terms(split_act(full.numpy())).max()) == 3


# ---- fp32 emulation of the wide kind, one case per family ----------------------------------------------------------------------------------
EMU = ["g1-32x32", "g1-m3-scalar", "halo-rect-16x16", "halo-flat-32x16", "halo-bf16-rect-16x16", "halo-bf16-flat-16x32", "split-16x16-w10",
       "split-vol-d2", "image1-n8", "image3-n8", "h9-16x16", "h1-16x32", "h27-vol-d2", "himage-k2", "red-s17", "ws-200x4x4-m3"]


@pytest.mark.parametrize("name", EMU)
def test_fp32_emulation_is_inside_the_bounds(L, name):
    c = R.by_name(name)
    d = R.data(c, "wide")
    _, slabs, _, red = case_config(L, c)
    got = R.emulate(c, d, slabs, red)
    r = R.held(f"emulation {name}", got, c, d, slabs, red)
    assert r <= 1.0
    assert worst(got, d["ref"], 2.0 ** -40 * d["Sacc"]) > 1.0, "the emulation does not round at all"


def test_fp32_emulation_of_the_activation(L):
    c = R.by_name("pro-16x16-g2")
    for kind in R.TWO:
        d = dict(R.data(c, kind))
        keep = (torch.rand((c["M"], c["k"]), generator=R.gen(5)) < 0.5).double()
        R.pro_finish(c, d, R.pro_params(c, kind), keep)
        _, slabs, _, red = case_config(L, c)
        got = R.emulate(c, d, slabs, red)
        if kind == "fixed":
            assert R.exactness_budget(c, d) < 2 ** 24 and equal_bits(got, d["ref"])
        else:
            assert R.held("emulation pro-16x16-g2", got, c, d, slabs, red) <= 1.0


def test_colsum_emulation_and_geometry():
    nblk, rpb = R.colsum_blocks(1024 * 512 + 1)
    assert nblk == 1024 and rpb == 513 and (nblk - 1) * rpb >= 1024 * 512 + 1          # the last block owns no row, the others more than 512
    nblk, rpb = R.colsum_blocks(1024 * 600 + 77)
    assert rpb == 601 and (nblk - 1) * rpb >= 1024 * 600 + 77 > (nblk - 2) * rpb        # ... here too, after blocks of 601 rows
    assert {cs["C"] for cs in R.COLSUM} >= {12, 1024, 2, 19, 255, 257, 1028} and {cs["M"] for cs in R.COLSUM} >= {1, 511, 513}
    for cs in R.COLSUM[:13]:
        d = R.colsum_data(cs, "wide")
        got = R.colsum_emulate(cs, d)
        r = worst(got, d["ref"], R.colsum_tol(cs, d))
        print(f"emulation colsum {cs['name']}: worst err / bound {r:.4f} (n = {R.colsum_n(cs)})")
        assert r <= 1.0
        f = R.colsum_data(cs, "fixed")
        assert float(f["S"].max()) / R.QZ < 2 ** 24 and equal_bits(R.colsum_emulate(cs, f), f["ref"])


# ---- planted errors: each must be caught by the helpers the GPU file uses -------------------------------------------------------------
def _held(c, d, got, L):
    _, slabs, _, red = case_config(L, c)
    return R.held("planted", got, c, d, slabs, red)


def test_planted_dropped_last_tile(L):
    c = R.by_name("halo-rect-16x16")                   # 2 images of 9 x 16: the last tile is the ragged row 8 of image 1
    for kind in ("fixed", "wide"):
        d = R.data(c, kind)
        dz = d["dz"].double().clone()
        dz[-16:] = 0
        got = (R.wgrad64(dz, d["x"].double(), c) + (d["dw0"].double() if c["acc"] else 0)).float()
        assert not equal_bits(got, d["ref"]) if kind == "fixed" else _held(c, d, got, L) > 1.0
    d = R.data(c, "impulse")
    dz = d["dz"].double().clone()
    dz[-16:] = 0
    assert not equal_bits(R.wgrad64(dz, d["x"].double(), c).float(), d["ref"])


def test_planted_plane_from_the_neighbouring_volume(L):
    c = R.by_name("halo-vol-nv2")                      # two volumes of three planes: treated as one volume of six, plane 3 sees plane 2
    one = dict(c, nv=1, d3=6)
    for kind in ("fixed", "wide", "impulse"):
        d = R.data(c, kind)
        got = (torch.einsum("mo,mtk->okt", d["dz"].double(), im2col(d["x"].double(), one)) + (d["dw0"].double() if c["acc"] else 0)).float()
        assert not equal_bits(got, d["ref"]) if kind != "wide" else _held(c, d, got, L) > 1.0


def test_planted_transposed_tap(L):
    c = R.by_name("split-16x16-w10")
    for kind in ("fixed", "wide", "impulse_x"):
        d = R.data(c, kind)
        got = d["ref"].clone().view(c["n"], c["k"], 3, 3).transpose(2, 3).reshape(c["n"], c["k"], 9).float()
        assert not equal_bits(got, d["ref"]) if kind != "wide" else _held(c, d, got, L) > 1.0


def test_planted_omitted_slab(L):
    c = R.by_name("red-s17")                           # 17 slabs, one plane each: the last one left out of the sum
    for kind in ("fixed", "wide"):
        d = R.data(c, kind)
        dz = d["dz"].double().clone()
        dz[16 * 128:] = 0
        got = R.wgrad64(dz, d["x"].double(), c).float()
        assert not equal_bits(got, d["ref"]) if kind == "fixed" else _held(c, d, got, L) > 1.0


def test_planted_accumulate_ignored(L):
    c = R.by_name("red4-s17")
    assert c["acc"] == 1
    for kind in ("fixed", "wide"):
        d = R.data(c, kind)
        got = d["ref0"].float()
        assert not equal_bits(got, d["ref"]) if kind == "fixed" else _held(c, d, got, L) > 1.0
    cs = [x for x in R.COLSUM if x["acc"]][0]
    d = R.colsum_data(cs, "wide")
    assert worst((d["ref"] - d["out0"].double()).float(), d["ref"], R.colsum_tol(cs, d)) > 1.0


def test_planted_leaking_pad_channel(L):
    """Cin = 20 in rows of 24: the NaN of the first pad column read as a 21st channel reaches dW only if the kernel lets it; a kernel that
    lets a pad column into channel 19 instead shows as NaN there - the sentinel is what makes the leak visible"""
    c = R.by_name("g1-16x32")
    d = R.data(c, "wide")
    x = d["x"].double().clone()
    x[:, -1] = float("nan")
    got = R.wgrad64(d["dz"].double(), x, c).float()
    assert _held(c, d, got, L) == float("inf")
    assert not equal_bits(torch.where(torch.isnan(got), torch.zeros_like(got), got), R.data(c, "fixed")["ref"])


# ---- host-side rejections --------------------------------------------------------------------------------------------------------------
P = ctypes.c_void_p(4096)                              # a pointer no rejected call ever dereferences


def test_wgrad_rejections(L):
    lib = L.load()
    f = lib.arco_conv3d_wgrad
    good = [P, 16, 16, P, 16, 16, 9, 2, 1, 8, 16, P, P, 0, 0, None]
    for i in (0, 3, 11, 12):                           # dZ, in, ws, dW
        a = list(good); a[i] = None
        assert f(*a) == ERR_ARG
    for i, v in ((6, 3), (6, 0), (6, 25), (14, -1), (14, 5), (2, 0), (5, 0), (7, 0), (8, 0), (9, 0), (10, 0), (1, 15), (4, 15), (13, 2)):
        a = list(good); a[i] = v
        assert f(*a) == ERR_ARG, (i, v)
    g = lib.arco_conv_wgrad
    good2 = [P, 16, 16, P, 16, 16, 9, 2, 8, 16, P, P, 0, None]
    for i, v in ((0, None), (3, None), (10, None), (11, None), (6, 4), (7, 0), (1, 8)):
        a = list(good2); a[i] = v
        assert g(*a) == ERR_ARG, (i, v)
    for (_, taps, cin, cout, ldz, ldi) in R.H_UNSUPPORTED:
        assert f(P, ldz, cout, P, ldi, cin, taps, 2, 1, 8, 16, P, P, 0, 4, None) == ERR_UNSUPPORTED
        assert L.query("arco_wgrad_last_route") == 0
        assert config(L, 0, taps, 2, 1, 8, 16, cin, cout, ldz, ldi, 4)[0] == ERR_UNSUPPORTED


def test_wgrad_pro_rejections(L):
    lib = L.load()
    f = lib.arco_conv3d_wgrad_pro
    t = torch.ones(64)
    ok = L.act_pro(t, t, t, t, 0.01, 2, 0, 0.0, 0, None)
    assert f(P, 16, 16, P, 16, 16, 9, 2, 1, 16, 16, P, P, 0, 3, None, None) == ERR_ARG
    for bad in (L.act_pro(t, t, t, t, 0.01, 0, 0, 0.0, 0, None), L.act_pro(t, t, t, t, 0.01, 2, 2, 0.0, 0, None),
                L.act_pro(t, t, t, t, 0.01, 2, 1, 1.0, 0, None)):
        assert f(P, 16, 16, P, 16, 16, 9, 2, 1, 16, 16, P, P, 0, 3, bad, None) == ERR_ARG
    assert f(None, 16, 16, P, 16, 16, 9, 2, 1, 16, 16, P, P, 0, 3, ok, None) == ERR_ARG
    for (_, taps, mma, nv, d3, h, w, cin, cout, ldz, groups) in R.PRO_UNSUPPORTED:
        pro = L.act_pro(t, t, t, t, 0.01, groups, 0, 0.0, 0, None)
        assert f(P, ldz, cout, P, cin, cin, taps, nv, d3, h, w, P, P, 0, mma, pro, None) == ERR_UNSUPPORTED
        assert L.query("arco_wgrad_last_route") == 0
        assert config(L, 0, taps, nv, d3, h, w, cin, cout, ldz, cin, mma, pro=groups)[0] == ERR_UNSUPPORTED


def test_image_wgrad_h_rejections(L):
    f = L.load().arco_conv3x3_image_wgrad_h
    good = [P, 16, 16, P, 4, 4, 2, 8, 16, P, P, 0, None]
    for i, v in ((0, None), (3, None), (9, None), (10, None), (5, 0), (5, 5), (4, 3), (6, 0), (7, 0), (8, 0), (1, 8), (11, 3)):
        a = list(good); a[i] = v
        assert f(*a) == ERR_ARG, (i, v)
    for i, v in ((2, 8), (1, 20), (0, ctypes.c_void_p(4104))):                         # Cout != 16 (ld_dz 16), ld_dz & 7, dZ not 16-byte aligned
        a = list(good); a[i] = v
        assert f(*a) == ERR_UNSUPPORTED, (i, v)
        assert L.query("arco_wgrad_last_route") == 0


def test_colsum_and_transpose_rejections(L):
    lib = L.load()
    for f in (lib.arco_colsum, lib.arco_colsum_h):
        good = [P, 16, 100, 16, P, P, 0, None]
        for i, v in ((0, None), (4, None), (5, None), (2, 0), (3, 0), (1, 15), (6, 2)):
            a = list(good); a[i] = v
            assert f(*a) == ERR_ARG, (i, v)
    good = [P, 40, 33, 40, P, 33, None]
    for i, v in ((0, None), (4, None), (2, 0), (3, 0), (1, 39), (5, 32)):
        a = list(good); a[i] = v
        assert lib.arco_transpose2d(*a) == ERR_ARG, (i, v)


def test_config_rejections(L):
    good = dict(entry=0, taps=9, nv=2, d3=1, h=8, w=16, cin=16, cout=16, ldz=16, ldi=16, mma=0)
    assert config(L, **good)[0] == R.rid(9, R.F_HALO, 0, 16, 16)
    for k, v in (("entry", 2), ("taps", 3), ("mma", 5), ("mma", -1), ("nv", 0), ("d3", 0), ("h", 0), ("w", 0), ("cin", 0), ("cout", 0), ("ldz", 15), ("ldi", 15)):
        assert config(L, **dict(good, **{k: v}))[0] == ERR_ARG, (k, v)
    for k, v in (("cin", 5), ("d3", 2), ("taps", 27)):     # arco_conv3x3_image_wgrad_h: K <= 4, 3x3, planes
        assert config(L, **dict(dict(good, entry=1, cin=4, ldi=8, mma=4), **{k: v}))[0] == ERR_ARG, (k, v)
    assert config(L, **dict(good, entry=1, cin=4, ldi=8, mma=4))[0] == R.rid(9, R.F_HIMAGE, 0, 16, 4)
    assert L.query("arco_wgrad_config", 0, 9, 2, 1, 8, 16, 16, 16, 16, 16, 0, 0, 1, None, None, None) == R.rid(9, R.F_HALO, 0, 16, 16)
