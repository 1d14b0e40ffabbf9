"""CPU companion of tests/test_augment_kernels_gpu.py: what makes that file trustworthy on a machine without a GPU.
  * the reference of the GPU file - the integer restatement of oracle/arco_oracle.py (q8, color_jitter_u8, gaussian_blur_u8) - is held
    to Pillow ITSELF: always to its recordings (tests/golden/g20_blur_sigmas.npz: GaussianBlur at the sigmas where the box radius is
    sensitive to its rounding; g12_jitter.npz), and where Pillow is installed to live Pillow on every image of every call of the
    GPU file's case table and over 6100 sigmas (0.150 ... 3.249 in steps of 0.001 and 3000 draws of the trainer's uniform(0.15, 1.15));
  * the package's own box-radius restatement (arco_amd.augment._gaussian_blur_radius) is bit-equal to the oracle's over that sweep,
    and the formula both used before - Pillow's expression evaluated in double and rounded once - is rejected at sigma 0.3;
  * the case table covers the listed edges, the comparison helper rejects a planted error;
  * the argument checks of the two entry points reject on the host (ARCO_ERR_ARG before anything is launched: no GPU needed)."""
import ctypes
import math
import os
import random
import struct

import numpy as np
import pytest
import torch

import arco_oracle as orc
import augment_kernel_refs as A
import fixture_inputs as fx

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def sweep_sigmas():
    rnd = random.Random(20)
    return [round(0.150 + 0.001 * i, 3) for i in range(3100)] + [rnd.uniform(0.15, 1.15) for _ in range(3000)]


def radius_in_double(sigma, passes=3):
    """Pillow's expression evaluated in double and rounded to float once at the end: NOT what BoxBlur.c computes"""
    sigma2 = float(np.float32(sigma)) * float(np.float32(sigma)) / passes
    L = math.sqrt(12.0 * sigma2 + 1.0)
    l = math.floor((L - 1.0) / 2.0)
    a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2)
    a /= 6 * (sigma2 - (l + 1) * (l + 1))
    return float(np.float32(l + a))


def blur_with(radius_fn, a, sigma):
    real = orc.gaussian_blur_radius
    orc.gaussian_blur_radius = radius_fn
    try:
        return orc.gaussian_blur_u8(a, sigma)
    finally:
        orc.gaussian_blur_radius = real


# ---- (a) the recordings ------------------------------------------------------------------------------------------------------------------------
def test_restatement_matches_the_g20_recordings_of_pillow():
    g = np.load(os.path.join(GOLDEN, "g20_blur_sigmas.npz"))
    sig = g["sigmas"]
    assert sig.dtype == np.float64 and tuple(sig.tolist()) == fx.BLUR_SIGMAS
    assert sorted({int(orc.gaussian_blur_radius(s)) for s in sig}) == [0, 1, 2]
    for tag in fx.BLUR_IMAGES:
        a = fx.blur_image(tag)
        for k, s in enumerate(sig.tolist()):
            np.testing.assert_array_equal(orc.gaussian_blur_u8(a, s), g[f"{tag}_{k}"], err_msg=f"{tag} sigma {s!r}")


def test_radius_evaluated_in_double_is_rejected_at_sigma_0_3():
    """the formula the package and the oracle shared before: one ulp off in the box radius, one level off in the pixels"""
    g = np.load(os.path.join(GOLDEN, "g20_blur_sigmas.npz"))
    k = fx.BLUR_SIGMAS.index(0.3)
    assert radius_in_double(0.3) != orc.gaussian_blur_radius(0.3)
    for tag in fx.BLUR_IMAGES:
        got = blur_with(radius_in_double, fx.blur_image(tag), 0.3)
        d = np.abs(got.astype(np.int32) - g[f"{tag}_{k}"].astype(np.int32))
        print(f"double-precision radius, sigma 0.3, image {tag}: {int((d != 0).sum())} pixels differ, by at most {int(d.max())}")
        assert (d != 0).any() and d.max() == 1


@pytest.mark.parametrize("tag", list(fx.JITTER_CASES))
def test_restatement_matches_the_g12_recordings_of_pillow(tag):
    g12 = np.load(os.path.join(GOLDEN, "g12_jitter.npz"))
    C, H, W, seed, order, factors, sigma = fx.JITTER_CASES[tag]
    p = A.P(order, factors, sigma)
    np.testing.assert_array_equal(A.ref_image(fx.jitter_image(seed, C, H, W), p), g12[tag])


# ---- (b) live Pillow -----------------------------------------------------------------------------------------------------------------------------
def pillow_image(a):
    from PIL import Image
    return Image.fromarray(a[0], 'L') if a.shape[0] == 1 else Image.fromarray(np.ascontiguousarray(a.transpose(1, 2, 0)), 'RGB')


def pillow_array(img):
    arr = np.array(img)
    return arr[None] if arr.ndim == 2 else np.ascontiguousarray(arr.transpose(2, 0, 1))


def pillow_jitter_blur(x, p):
    """torchvision's ColorJitter glue on top of Pillow's ImageEnhance / convert('HSV'), then ImageFilter.GaussianBlur - exactly as
    oracle/gen_golden.py g12 produces its recordings"""
    from PIL import Image, ImageEnhance, ImageFilter
    # to_pil_image is pic.mul(255).byte(): torch's own conversion wherever it is defined (0 <= x <= 1); outside, a float -> uint8
    # conversion is undefined in C (torch's CPU build wraps), and the project clips (q8 of the kernel and of the oracle)
    t = torch.from_numpy(x)
    u8 = orc.q8(x)
    inside = ((t >= 0) & (t <= 1)).numpy()
    assert np.array_equal(t.mul(255).byte().numpy()[inside], u8[inside])
    img = pillow_image(u8)
    if p["order"] is not None:
        for op in p["order"]:
            f = p["factors"][op]
            if op == 0:
                img = ImageEnhance.Brightness(img).enhance(f)
            elif op == 1:
                img = ImageEnhance.Contrast(img).enhance(f)
            elif op == 2:
                img = ImageEnhance.Color(img).enhance(f)
            elif op == 3 and img.mode == 'RGB':
                h, s_, v = img.convert('HSV').split()
                np_h = np.array(h, dtype=np.uint8)
                np_h = (np_h.astype(np.int32) + (int(np.float32(f) * np.float32(255.0)) & 0xff)).astype(np.uint8)
                img = Image.merge('HSV', (Image.fromarray(np_h, 'L'), s_, v)).convert('RGB')
    if p["sigma"] is not None:
        img = img.filter(ImageFilter.GaussianBlur(radius=p["sigma"]))
    return pillow_array(img)


def test_restatement_matches_live_pillow_over_the_sigma_sweep():
    pytest.importorskip("PIL")
    from PIL import ImageFilter
    a = np.random.RandomState(48).randint(0, 256, size=(1, 48, 48)).astype(np.uint8)
    img = pillow_image(a)
    sig = sweep_sigmas()
    bad = [s for s in sig if not np.array_equal(orc.gaussian_blur_u8(a, s), pillow_array(img.filter(ImageFilter.GaussianBlur(radius=s))))]
    print(f"sigma sweep: {len(bad)} of {len(sig)} sigmas differ from Pillow {bad[:8]}")
    assert not bad
    old = [s for s in (0.3, 1.249) if not np.array_equal(blur_with(radius_in_double, a, s),
                                                        pillow_array(img.filter(ImageFilter.GaussianBlur(radius=s))))]
    assert 0.3 in old                                                                     # the sweep notices the former formula


@pytest.mark.parametrize("name", A.CALLS + [A.PACKAGE_CALL])
def test_restatement_matches_live_pillow_on_every_image_of_the_case_table(name):
    pytest.importorskip("PIL")
    c = A.call_case(name)
    for i, p in enumerate(c["params"]):
        want = pillow_jitter_blur(c["x"][i].numpy(), p)
        np.testing.assert_array_equal(c["ref"][i].numpy(), want.astype(np.int32), err_msg=f"{name} image {i} {p}")


# ---- (c) the package's radius ------------------------------------------------------------------------------------------------------------------
def test_package_radius_is_bit_equal_to_the_oracle_radius():
    from arco_amd import augment
    bits = lambda v: struct.pack("<f", v)
    sig = sweep_sigmas() + list(fx.BLUR_SIGMAS) + [v[6] for v in fx.JITTER_CASES.values() if v[6] is not None]
    diff = [s for s in sig if bits(augment._gaussian_blur_radius(s)) != bits(orc.gaussian_blur_radius(s))]
    assert not diff, diff[:8]
    n_old = sum(radius_in_double(s) != orc.gaussian_blur_radius(s) for s in sig)
    print(f"radius in double differs from the float restatement at {n_old} of {len(sig)} sigmas")
    assert n_old > len(sig) // 5                                                          # about a third: the sweep can tell the two apart


# ---- the case table ----------------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_listed_edges():
    names = A.CALLS
    assert len(set(names)) == len(names)
    planes = {(c["H"], c["W"], c["C"]) for c in map(A.call_case, names) if c["name"].startswith("plane")}
    assert planes == {(H, W, C) for (H, W) in A.PLANES for C in (1, 3)}
    for (H, W) in A.PLANES:                                                               # every radius class and unblurred, +- jitter
        c = A.call_case(f"plane:{H}:{W}:3")
        cls = {(p["order"] is not None, None if p["sigma"] is None else int(orc.gaussian_blur_radius(p["sigma"]))) for p in c["params"]}
        assert cls == {(j, r) for j in (False, True) for r in (None, 0, 1, 2)}
    assert all(orc.gaussian_blur_radius(s) < 3.0 for s in A.CLASS_SIGMA)
    assert any(H < 3 and W < 3 for H, W in A.PLANES) and any(H > 32 and W > 64 for H, W in A.PLANES)      # below the halo; > 1 tile
    s = A.call_case("stride:1")
    assert s["H"] * s["W"] > 128 * 256 and s["params"][0]["order"] is not None and 1 in s["params"][0]["order"]
    for C in (1, 3):
        a, b = A.call_case(f"mixed:{C}:0"), A.call_case(f"mixed:{C}:1")
        assert sorted(map(str, a["params"])) == sorted(map(str, b["params"])) and a["params"] != b["params"] and a["B"] == 6
    assert A.call_case("full:3:32")["B"] == A.MAX_IMG and A.call_case(A.PACKAGE_CALL)["B"] == A.MAX_IMG + 1
    assert {p["order"] for p in A.call_case("orders:3")["params"]} == set(A.ORDERS24) and len(A.ORDERS24) == 24
    o1 = [p["order"] for p in A.call_case("orders:1")["params"]]
    assert o1[0][0] == 1 and o1[1][3] == 1 and o1[2].index(1) == o1[2].index(0) + 1
    f3 = A.call_case("factors:3")["params"]
    for op, want in ((0, A.FACTORS), (1, A.FACTORS), (2, A.FACTORS), (3, A.HUES)):
        assert {p["factors"][op] for p in f3} >= set(want)
    pal = orc.q8(A.palette_image(3)).reshape(3, -1).T
    assert np.array_equal(pal, np.array(A.PALETTE, dtype=np.uint8))                        # levels() survives q8
    mx = pal.max(1)
    two = lambda i, j, k: ((pal[:, i] == mx) & (pal[:, j] == mx) & (pal[:, k] < mx)).any()
    assert two(0, 1, 2) and two(1, 2, 0) and two(0, 2, 1) and (pal.min(1) == mx).sum() >= 4
    for k in (0, 100, 254):                                                               # mean luminance exactly k + 0.5
        for C in (1, 3):
            a = orc.q8(A.half_mean_image(C, k))
            lum = orc._lum8(a) if C == 3 else a[0]
            assert float(lum.astype(np.float64).mean()) == k + 0.5
            assert (orc.color_jitter_u8(a, [1, 0, 2, 3], (1.0, 0.0, 1.0, 0.0)) == k + 1).all()
    v = A.input_values()
    k255 = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    assert np.isin(k255, v).all() and np.isin(np.nextafter(k255, np.float32(-1)), v).all()
    assert (v < 0).any() and (v > 1).any() and np.signbit(v[v == 0]).any() and not np.isnan(v).any()
    # fl(fl(k / 255) * 255) == k for every k, and one ulp below k / 255 truncates to k - 1: both sides of every level's threshold
    assert np.array_equal(orc.q8(k255), np.arange(256))
    assert np.array_equal(orc.q8(np.nextafter(k255, np.float32(-1)))[1:], np.arange(255))
    assert A.QUANT_N == (0, 1, 255, 256, 257, 2048 * 256 + 1)
    qc = A.quant_case(257)
    sub = qc["x"][(qc["x"] != 0) & (qc["x"].abs() < 2.0 ** -126)]
    assert sub.numel() > 0 and not bool(torch.isnan(qc["x"]).any())
    assert torch.equal(qc["ref"], torch.from_numpy(orc.q8(qc["x"].numpy()).astype(np.float32) / np.float32(255.0)))
    assert not bool(torch.signbit(qc["ref"]).any())


def test_helper_rejects_planted_errors():
    c = A.call_case("plane:7:9:3")
    good = c["ref"].float() / 255.0
    A.check_images("the restatement itself", good, c["ref"])
    one = good.clone()
    one[5, 2, 6, 8] = (c["ref"][5, 2, 6, 8].float() + (1 if c["ref"][5, 2, 6, 8] < 255 else -1)) / 255.0
    with pytest.raises(AssertionError, match="pixels differ"):
        A.check_images("one level", one, c["ref"])
    off = good.clone()
    off[0, 0, 0, 1] = float(np.nextafter(np.float32(off[0, 0, 0, 1]), np.float32(2)))
    if float(off[0, 0, 0, 1]) * 255 != round(float(off[0, 0, 0, 1]) * 255):
        with pytest.raises(AssertionError, match="not k / 255"):
            A.check_images("one ulp", off, c["ref"])
    buf = A.sentinel_buffer(5)
    assert buf.numel() == 5 + A.GUARD and bool((buf == A.SENTINEL).all())


# ---- argument checks (host side) -----------------------------------------------------------------------------------------------------------------
def test_argument_checks_reject_on_the_host():
    """ARCO_ERR_ARG (-1) is returned before anything is launched, so this needs no GPU; data / ws / out are host addresses (or null)
    that are never dereferenced, the descriptor table is a real host array (it is read on the host).  Every list below is a VALID call
    with one argument spoilt at a time; the valid call itself is never made."""
    import arco_amd._lib as L
    L.load()
    assert L.query("arco_jitter_desc_bytes") == A.DESC_BYTES
    buf = torch.zeros(64, dtype=torch.float64)
    p = ctypes.c_void_p(buf.data_ptr())
    bad = -1
    ok_desc = A.desc([A.with_sigma(A.JIT, 0.9)] * 33)
    # arco_jitter_blur: data, B, C, H, W, desc_host, ws, out
    ok = [p, 2, 3, 4, 5, ok_desc, p, p]
    for pos, val in [(0, None), (5, None), (6, None), (7, None), (1, 0), (1, 33), (1, -1), (2, 2), (2, 0), (2, 4), (3, 0), (4, 0), (3, -1)]:
        args = list(ok)
        args[pos] = val
        assert L.query("arco_jitter_blur", *args, None) == bad, (pos, val)
    for fr in (-0.5, 3.0, 3.5):                                                           # blur_r < 0 and >= 3, in the second record
        rec = struct.pack("<4i4fiif", 0, 1, 2, 3, 1.0, 1.0, 1.0, 0.0, 0, 1, fr)
        assert L.query("arco_jitter_blur", p, 2, 3, 4, 5, ok_desc[:44] + rec, p, p, None) == bad, fr
    # arco_quantize8: x, n, out
    for pos, val in [(0, None), (2, None), (1, -1)]:
        args = [p, 4, p]
        args[pos] = val
        assert L.query("arco_quantize8", *args, None) == bad, (pos, val)
    assert L.query("arco_quantize8", p, 0, p, None) == 0                                  # n == 0: nothing to do
