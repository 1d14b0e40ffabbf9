"""Every weight- and bias-gradient route of csrc/wgrad.hip and conv_h.hip called DIRECTLY through arco_amd._lib
(arco_conv_wgrad, arco_conv3d_wgrad, arco_conv3d_wgrad_pro, arco_conv3x3_image_wgrad_h, arco_colsum, arco_colsum_h, arco_transpose2d),
one route per test, against the float64 reference of tests/wgrad_kernel_refs.py computed from the same fp32 / f16 operand values.
Every test asserts the kernel that ran through arco_wgrad_last_route and the same id, slab count, slab size and reduction kernel
through arco_wgrad_config.  Operands carry NaN in their stride padding, in front of their first and behind their last row; dW / out
are guarded on both sides; operands are passed as channel slices with offsets.

Workspace guard: ws is allocated at the dispatcher's documented slab target (768 or 512 divided by ydim * zdim) times the slab size and
prefilled with a sentinel, so a dispatcher that writes one slab per tile stays inside the allocation; every word past
arco_wgrad_ws_floats(Cout, Cin, taps, M) must keep the sentinel.  The `ws-*` cases are the shapes whose tile count is above the slab
reservation (many small planes).

Kinds (wgrad_kernel_refs.py): `fixed`, `impulse`, `impulse_x` equal float64 BIT FOR BIT; `wide` is held per element to the derived bound.

Worst err / bound of the wide kind per route (MI355X, this file | fp32 emulation, tests/test_wgrad_kernels_cpu.py):
  route                                             MI355X    emulation
  wgrad_kernel<COB,CIB> (nine tiles)                0.087     0.047
  wgrad_q_kernel<64> (n = 1167: nine tiles a chain) 0.0015    -
  wgrad_halo2_kernel rectangular, fp32              0.077     0.047
  wgrad_halo2_kernel flat, fp32                     0.064     0.030
  wgrad_halo2_kernel rectangular, bf16 operands     0.73      0.61
  wgrad_halo2_kernel flat, bf16 operands            0.75      0.64
  wgrad_split_kernel                                0.025     0.037
  wgrad_split_kernel with the activation            0.017     0.022
  wgrad_image3d_kernel<1> / <3>                     0.019 / 0.021   0.015 / 0.025
  hwgrad_kernel<.,.,9> (taps 9 and 27)              0.091     0.113
  hwgrad_kernel<.,.,1>                              0.078     0.055
  himage_wgrad_kernel                               0.014     0.017
  arco_colsum / arco_colsum_h                       0.20 / 0.013    (sequential fp32 sum inside gamma(M + 1))
  The bounds are rigorous worst cases, linear in the chain length n, where independent roundings add up as sqrt(n): the fp32 routes sit
  at 0.02 .. 0.09 on the hardware as in the emulation, the longest chain (wgrad_q_kernel, n = 1167) lowest.  What binds on those routes are
  the three exact kinds; the bf16-operand routes are bound by their operand rounding term and sit at 0.75.
  Every exact case (fixed, impulse, impulse_x) held bit for bit on every route, every guard and sentinel stayed intact, and no word past
  arco_wgrad_ws_floats was written: no kernel had to be changed.  With the dispatcher as it was before the slab clamp the six `ws-*`
  shapes wrote 36 .. 192 slabs past the reservation (the image path 2.2 slabs' worth of words) while still returning the exact dW.

Routes covered: wgrad_kernel in nine tiles (incl. the scalar-load form and three persistent rounds); wgrad_q_kernel<64> and the ordinary tile
a step below its M and Cin thresholds; wgrad_halo2_kernel rectangular and flat in four tiles each with fp32 and bf16 operands, and as
the fall-back of mma 3; wgrad_split_kernel in four tiles at taps 9 and 27 with and without the consumer-side activation;
wgrad_image3d_kernel<1|3> (fp32 and f16 dZ); hwgrad_kernel<.,.,9> in four tiles at taps 9 and 27 and <.,.,1> in nine;
himage_wgrad_kernel at K = 1 .. 4; the three slab reductions at 1, 16 and 17 slabs; the three branches of colsum_partial_kernel for
float and f16; transpose2d_kernel."""
import ctypes

import pytest
import torch

import wgrad_kernel_refs as R
from conv_kernel_refs import ERR_UNSUPPORTED, equal_bits
from loss_kernel_refs import SENTINEL, worst
from test_side_kernels_gpu import DEV, dev

pytestmark = pytest.mark.gpu
GUARD = 8                                              # elements in front of and behind every buffer (8 fp32 / f16: 16-byte multiples)


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


@pytest.fixture(autouse=True)
def stop_on_device_error():
    """a device error ends the session: nothing more is launched on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, nothing more is launched: {e}", returncode=3)


def having(kind):
    cs = [c for c in R.CASES if kind in c["kinds"] and not c["pro"]]
    return pytest.mark.parametrize("c", cs, ids=[c["name"] for c in cs])


def put_nan(t, ld, off=0):
    """[rows, C] CPU tensor -> (device buffer [GUARD | rows x ld | GUARD], NaN everywhere but columns off .. off + C; the operand's
    pointer-carrying view)"""
    rows, Cc = t.shape
    assert off + Cc <= ld
    buf = torch.full((GUARD + rows * ld + GUARD,), float("nan"), dtype=t.dtype)
    buf[GUARD:GUARD + rows * ld].view(rows, ld)[:, off:off + Cc] = t
    buf = buf.to(DEV)
    return buf, buf[GUARD + off:]


def guarded(n, init=None):
    """[GUARD | n | GUARD] fp32 holding the sentinel (the body: init, if given) -> (buffer, the body's view)"""
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32)
    if init is not None:
        buf[GUARD:GUARD + n] = init.reshape(-1)
    buf = buf.to(DEV)
    return buf, buf[GUARD:]


def body_of(buf, n, what):
    torch.cuda.synchronize()
    b = buf.cpu()
    assert bool((b[:GUARD] == SENTINEL).all()), f"the guard in front of {what} was written"
    assert bool((b[GUARD + n:] == SENTINEL).all()), f"the guard behind {what} was written"
    return b[GUARD:GUARD + n]


def config(L, c, aligned=1):
    s, f, r = ctypes.c_long(), ctypes.c_long(), ctypes.c_int()
    route = L.query("arco_wgrad_config", c["entry"], c["taps"], c["nv"], c["d3"], c["h"], c["w"], c["k"], c["n"], c["ld_dz"], c["ld_in"],
                    c["mma"], c["pro"], aligned, ctypes.byref(s), ctypes.byref(f), ctypes.byref(r))
    return route, s.value, f.value, r.value


def run(L, c, d, pro=None):
    """one launch of the case's entry point -> (dW [Cout, Cin, taps] on the CPU, slabs, reduction kind), every guard checked"""
    M, K, N, T = c["M"], c["k"], c["n"], c["taps"]
    zb, z = put_nan(d["dz"], c["ld_dz"], c["dz_off"])
    xb, x = put_nan(d["x"], c["ld_in"], c["in_off"])
    cnt = N * K * T
    dwb, dw = guarded(cnt, d["dw0"] if c["acc"] else None)
    need = L.query("arco_wgrad_ws_floats", N, K, T, M)
    assert R.target_slabs(c) * R.slab_floats(c) * 4 <= 34 * 2 ** 20
    cap = max(need, R.target_slabs(c) * R.slab_floats(c))
    ws = torch.full((cap + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    aligned = int(z.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0)
    route, slabs, sf, kind = config(L, c, aligned)
    if c["entry"] == 1:
        L.call("arco_conv3x3_image_wgrad_h", L.ptr(z), c["ld_dz"], N, L.ptr(x), c["ld_in"], K, c["nv"], c["h"], c["w"], L.ptr(ws), L.ptr(dw), c["acc"])
    elif pro is not None:
        L.call("arco_conv3d_wgrad_pro", L.ptr(z), c["ld_dz"], N, L.ptr(x), c["ld_in"], K, T, c["nv"], c["d3"], c["h"], c["w"], L.ptr(ws), L.ptr(dw),
               c["acc"], c["mma"], pro)
    elif c["mma"] == 0 and T != 27 and c["d3"] == 1:
        L.call("arco_conv_wgrad", L.ptr(z), c["ld_dz"], N, L.ptr(x), c["ld_in"], K, T, c["nv"], c["h"], c["w"], L.ptr(ws), L.ptr(dw), c["acc"])
    else:
        L.call("arco_conv3d_wgrad", L.ptr(z), c["ld_dz"], N, L.ptr(x), c["ld_in"], K, T, c["nv"], c["d3"], c["h"], c["w"], L.ptr(ws), L.ptr(dw),
               c["acc"], c["mma"])
    took = L.query("arco_wgrad_last_route")
    got = body_of(dwb, cnt, "dW").view(N, K, T)
    w = ws.cpu()
    assert bool((w[need:] == SENTINEL).all()), \
        f"{c['name']}: {int((w[need:] != SENTINEL).sum())} words past arco_wgrad_ws_floats = {need} were written"
    assert took == c["route"] and route == c["route"], (c["name"], took, route)
    assert sf == R.slab_floats(c) and 1 <= slabs and slabs * sf <= need, (slabs, sf, need)
    assert not c["red"] or kind == c["red"], (c["name"], kind)
    for b, t, ld, off in ((zb, d["dz"], c["ld_dz"], c["dz_off"]), (xb, d["x"], c["ld_in"], c["in_off"])):      # the operands are read-only
        inner = b.cpu()[GUARD:GUARD + M * ld].view(M, ld)
        assert torch.equal(inner[:, off:off + t.shape[1]], t) and bool(torch.isnan(b.cpu()[:GUARD]).all())
    return got, slabs, kind


@having("fixed")
def test_fixed_point_is_exact(L, c):
    d = R.data(c, "fixed")
    assert R.exactness_budget(c, d) < 2 ** 24
    got, slabs, kind = run(L, c, d)
    assert equal_bits(got, d["ref"])
    print(f"{c['name']} route {c['route']}: fixed exact, {slabs} slabs, reduction {kind}")


@having("impulse")
def test_impulses_in_dz_return_the_shifted_input(L, c):
    d = R.data(c, "impulse")
    assert equal_bits(run(L, c, d)[0], d["ref"])


@having("impulse_x")
def test_impulses_in_x_return_the_shifted_dz(L, c):
    d = R.data(c, "impulse_x")
    assert equal_bits(run(L, c, d)[0], d["ref"])


@having("wide")
def test_wide_range_is_bounded_per_element(L, c):
    d = R.data(c, "wide")
    got, slabs, kind = run(L, c, d)
    r = R.held(f"{c['name']} route {c['route']}", got, c, d, slabs, kind)
    assert r <= 1.0, (c["name"], r)


# ---- arco_conv3d_wgrad_pro ------------------------------------------------------------------------------------------------------------
PRO = [c for c in R.CASES if c["pro"]]
SEED = 0x1234567887654321


def keep_mask(L, c):
    """the dropout mask of the project's own generator: arco_bn_act_fwd on ones (mean 0, istd 1, gamma 1, beta 0) keeps or zeroes"""
    M, K, G = c["M"], c["k"], c["pro"]
    one, zero = torch.ones(G * K, device=DEV), torch.zeros(G * K, device=DEV)
    a = torch.zeros((M, K), device=DEV)
    L.call("arco_bn_act_fwd", L.ptr(torch.ones((M, K), device=DEV)), K, M, K, L.ptr(zero), L.ptr(one), L.ptr(one), L.ptr(zero), R.SLOPE, 1, R.P_DROP,
           SEED, c["h"] * c["w"], L.ptr(a), K, None, G)
    torch.cuda.synchronize()
    keep = (a.cpu() != 0)
    assert 0.4 < float(keep.float().mean()) < 0.6
    return keep.double()


@pytest.mark.parametrize("kind", R.TWO)
@pytest.mark.parametrize("c", PRO, ids=[c["name"] for c in PRO])
def test_consumer_side_activation(L, c, kind):
    assert L.query("arco_conv_pro_ok", c["taps"], c["nv"], c["d3"], c["h"], c["w"], c["k"], c["n"], c["ld_in"], c["mma"], c["pro"]) == 1
    d = dict(R.data(c, kind))
    prm = R.pro_params(c, kind)
    keep = keep_mask(L, c) if c["drop"] else None
    R.pro_finish(c, d, prm, keep)
    dp = [dev(t) for t in prm]
    pro = L.act_pro(dp[0], dp[1], dp[2], dp[3], R.SLOPE, c["pro"], c["drop"], R.P_DROP if c["drop"] else 0.0, SEED, None)
    got, slabs, rk = run(L, c, d, pro=pro)
    if kind == "fixed":
        assert R.exactness_budget(c, d) < 2 ** 24
        assert equal_bits(got, d["ref"])
    else:
        r = R.held(f"{c['name']} route {c['route']}", got, c, d, slabs, rk)
        assert r <= 1.0, (c["name"], r)


@pytest.mark.parametrize("u", R.PRO_UNSUPPORTED, ids=[u[0] for u in R.PRO_UNSUPPORTED])
def test_consumer_side_activation_unsupported(L, u):
    _, taps, mma, nv, d3, h, w, cin, cout, ldz, groups = u
    M = nv * d3 * h * w
    z, x = torch.zeros(M * ldz, device=DEV), torch.zeros((M, cin), device=DEV)
    one = torch.ones(groups * cin, device=DEV)
    ws = torch.zeros(L.query("arco_wgrad_ws_floats", cout, cin, taps, M), device=DEV)
    dwb, dw = guarded(cout * cin * taps)
    pro = L.act_pro(one, one, one, one, 0.01, groups, 0, 0.0, 0, None)
    rc = L.load().arco_conv3d_wgrad_pro(L.ptr(z), ldz, cout, L.ptr(x), cin, cin, taps, nv, d3, h, w, L.ptr(ws), L.ptr(dw), 0, mma, pro, L.stream())
    assert rc == ERR_UNSUPPORTED and L.query("arco_wgrad_last_route") == 0
    assert bool((body_of(dwb, cout * cin * taps, "dW") == SENTINEL).all())


@pytest.mark.parametrize("u", R.H_UNSUPPORTED, ids=[u[0] for u in R.H_UNSUPPORTED])
def test_f16_rejections(L, u):
    _, taps, cin, cout, ldz, ldi = u
    M = 2 * 8 * 16
    z, x = torch.zeros(M * ldz, dtype=torch.float16, device=DEV), torch.zeros(M * ldi, dtype=torch.float16, device=DEV)
    ws = torch.zeros(L.query("arco_wgrad_ws_floats", cout, cin, taps, M), device=DEV)
    dwb, dw = guarded(cout * cin * taps)
    rc = L.load().arco_conv3d_wgrad(L.ptr(z), ldz, cout, L.ptr(x), ldi, cin, taps, 2, 1, 8, 16, L.ptr(ws), L.ptr(dw), 0, 4, L.stream())
    assert rc == ERR_UNSUPPORTED and L.query("arco_wgrad_last_route") == 0
    assert bool((body_of(dwb, cout * cin * taps, "dW") == SENTINEL).all())


def test_image_wgrad_h_rejections(L):
    M = 2 * 8 * 16
    z = torch.zeros(M * 24 + 8, dtype=torch.float16, device=DEV)
    x, ws = torch.zeros(M * 4, device=DEV), torch.zeros(L.query("arco_wgrad_ws_floats", 16, 4, 9, M), device=DEV)
    dwb, dw = guarded(16 * 4 * 9)
    f = L.load().arco_conv3x3_image_wgrad_h
    for cout, ldz, zz in ((8, 16, z), (16, 20, z), (16, 16, z[4:])):               # Cout != 16, ld_dz & 7, dZ not 16-byte aligned
        assert f(L.ptr(zz), ldz, cout, L.ptr(x), 4, 4, 2, 8, 16, L.ptr(ws), L.ptr(dw), 0, L.stream()) == ERR_UNSUPPORTED
        assert L.query("arco_wgrad_last_route") == 0
    assert bool((body_of(dwb, 16 * 4 * 9, "dW") == SENTINEL).all())


def test_rejected_arguments_leave_the_last_route(L):
    """ARCO_ERR_ARG leaves arco_wgrad_last_route as the last launch set it; ARCO_ERR_UNSUPPORTED sets 0"""
    c = R.by_name("halo-rect-16x16")
    run(L, c, R.data(c, "fixed"))
    assert L.query("arco_wgrad_last_route") == c["route"] != 0
    z = torch.zeros(c["M"] * c["ld_dz"], device=DEV)
    f = L.load().arco_conv3d_wgrad
    assert f(L.ptr(z), c["ld_dz"], c["n"], L.ptr(z), c["ld_in"], c["k"], 9, c["nv"], 1, c["h"], c["w"], None, L.ptr(z), 0, 0, L.stream()) == R.ERR_ARG
    assert L.query("arco_wgrad_last_route") == c["route"]
    assert f(L.ptr(z), 16, 16, L.ptr(z), 20, 12, 9, 1, 1, 4, 4, L.ptr(z), L.ptr(z), 0, 4, L.stream()) == ERR_UNSUPPORTED
    assert L.query("arco_wgrad_last_route") == 0


# ---- arco_colsum / arco_colsum_h -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.TWO)
@pytest.mark.parametrize("cs", R.COLSUM, ids=[c["name"] for c in R.COLSUM])
def test_colsum(L, cs, kind):
    d = R.colsum_data(cs, kind)
    xb, x = put_nan(d["x"], cs["ldx"])
    ob, out = guarded(cs["C"], d["out0"] if cs["acc"] else None)
    wsb, ws = guarded(1024 * cs["C"])
    L.call("arco_colsum_h" if cs["half"] else "arco_colsum", L.ptr(x), cs["ldx"], cs["M"], cs["C"], L.ptr(ws), L.ptr(out), cs["acc"])
    got = body_of(ob, cs["C"], "out")
    body_of(wsb, 1024 * cs["C"], "ws")
    if kind == "fixed":
        assert equal_bits(got, d["ref"])
    else:
        r = worst(got, d["ref"], R.colsum_tol(cs, d))
        print(f"colsum {cs['name']}: worst err / bound {r:.4f} (n = {R.colsum_n(cs)})")
        assert r <= 1.0


# ---- arco_transpose2d ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", R.TRANSPOSE, ids=str)
def test_transpose2d_bit_for_bit(L, t):
    rows, cols_, pr, pc = t
    x = R._wide_values((rows, cols_), R.gen(rows, cols_), 3, 0.1)
    ldx, ldy = cols_ + pr, rows + pc
    xb, xv = put_nan(x, ldx)
    yb, y = guarded(cols_ * ldy)
    L.call("arco_transpose2d", L.ptr(xv), ldx, rows, cols_, L.ptr(y), ldy)
    got = body_of(yb, cols_ * ldy, "y").view(cols_, ldy)
    assert torch.equal(got[:, :rows].contiguous().view(torch.int32), x.t().contiguous().view(torch.int32))
    assert bool((got[:, rows:] == SENTINEL).all()), "a pad column of ldy > rows was written"
