"""train_arco_2d --act_dtype f16 --fm_rows f16: the row-sparse 2-D heads read the U-Net's finest feature maps as stored (f16 rows,
f16 row-sparse gradients), the logits-only passes cast no map.  Kernels, heads (eager) and the step at the benchmarked size
(8 + 8 images of 256 x 256, 4 classes, --queue_size 4096, default schedule)."""
import numpy as np
import pytest
import torch

from test_configs_at_size_gpu import _acdc_batch, _check_step_invariants, _drop_off, seed_all
from test_step2d_f16_gpu import TERMS, THRESH, TRAJ_RTOL, _make, _reset as _reset_f16, _three_steps

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, F32 = torch.float16, torch.float32
ROWS = ["--act_dtype", "f16", "--fm_rows", "f16"]


def _reset():
    from arco_amd import ops
    _reset_f16()
    assert ops.FM_CAST is True          # every context of the step restores it


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rnd(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(DEV)


def _pix(rs, n, n_img, ho, wo):
    """n high-res pixel ids over n_img images: random, with repeated entries and the image-border pixels of both images."""
    per = ho * wo
    pix = torch.from_numpy(rs.randint(0, n_img * per, size=n))
    border = [0, wo - 1, per - wo, per - 1, per, per + wo - 1, 2 * per - wo, n_img * per - 1, (ho // 2) * wo, (ho // 2) * wo + wo - 1]
    pix[:len(border)] = torch.tensor(border)
    pix[20] = pix[3]; pix[21] = pix[3]; pix[n - 1] = pix[40]; pix[n - 2] = pix[0]      # repeated entries
    return pix.to(DEV)


# ------------------------------------------------------------------------------------------------------------------------------
# kernels: the f16-`hi` entry point on (lo fp32, hi f16) is bit-equal to the fp32 one on (lo, hi.float()) - the widening is exact and
# the fp32 arithmetic is the same code
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chi", [16, 32, 64])
@pytest.mark.parametrize("clo", [384, 448, 480])
def test_gather_upcat_rows_h_is_bit_equal_to_fp32(clo, chi):
    from arco_amd import _lib as L
    rs = np.random.RandomState(clo + chi)
    nb, hi_h, hi_w, ho, wo, n, pad = 2, 9, 12, 18, 24, 203, 8
    assert n % 4 != 0
    lo = _rnd(rs, nb * hi_h * hi_w, clo)
    store = _rnd(rs, nb * ho * wo, chi + pad).half()            # rows with ldhi > Chi: the map is a channel slice of a wider tensor
    hi16 = store[:, :chi]
    assert hi16.stride(0) == chi + pad and not hi16.is_contiguous()
    hi32 = hi16.float().contiguous()
    pix = _pix(rs, n, nb, ho, wo)
    k = clo + chi
    X16 = torch.full((n, k), float("nan"), dtype=F32, device=DEV)
    X32 = torch.full((n, k), float("nan"), dtype=F32, device=DEV)
    L.call("arco_gather_upcat_rows_h", L.ptr(lo), clo, clo, hi_h, hi_w, L.ptr(hi16), chi + pad, chi, ho, wo, L.ptr(pix), n, L.ptr(X16), k)
    L.call("arco_gather_upcat_rows", L.ptr(lo), clo, clo, hi_h, hi_w, L.ptr(hi32), chi, chi, ho, wo, L.ptr(pix), n, L.ptr(X32), k)
    assert bool(torch.isfinite(X32).all())
    assert torch.equal(X16, X32)
    assert torch.equal(X16[:, clo:], hi32[pix])                   # the hi part is the map's own rows
    # a contiguous f16 map (ldhi == Chi) too
    hc = hi16.contiguous()
    X16c = torch.empty((n, k), dtype=F32, device=DEV)
    L.call("arco_gather_upcat_rows_h", L.ptr(lo), clo, clo, hi_h, hi_w, L.ptr(hc), chi, chi, ho, wo, L.ptr(pix), n, L.ptr(X16c), k)
    assert torch.equal(X16c, X32)


@pytest.mark.parametrize("chi", [16, 32, 64])
@pytest.mark.parametrize("clo", [384, 448, 480])
def test_lerp4_cat_rows_h_is_bit_equal_to_fp32(clo, chi):
    from arco_amd import _lib as L
    rs = np.random.RandomState(7 * clo + chi)
    nb, ho, wo, n, pad = 2, 18, 24, 203, 8
    V = _rnd(rs, 4 * n, clo)
    lylx = torch.from_numpy(rs.uniform(size=2 * n).astype(np.float32)).to(DEV)
    lylx[:4] = torch.tensor([0.0, 0.0, 1.0, 0.5], device=DEV)
    store = _rnd(rs, nb * ho * wo, chi + pad).half()
    hi16 = store[:, :chi]
    hi32 = hi16.float().contiguous()
    pix = _pix(rs, n, nb, ho, wo)
    k = clo + chi
    X16 = torch.full((n, k), float("nan"), dtype=F32, device=DEV)
    X32 = torch.full((n, k), float("nan"), dtype=F32, device=DEV)
    L.call("arco_lerp4_cat_rows_h", L.ptr(V), clo, clo, L.ptr(lylx), L.ptr(hi16), chi + pad, chi, L.ptr(pix), n, L.ptr(X16), k)
    L.call("arco_lerp4_cat_rows", L.ptr(V), clo, clo, L.ptr(lylx), L.ptr(hi32), chi, chi, L.ptr(pix), n, L.ptr(X32), k)
    assert bool(torch.isfinite(X32).all())
    assert torch.equal(X16, X32)
    assert torch.equal(X16[:, clo:], hi32[pix])


def test_row_cast_and_zero_kernels_are_idempotent_under_duplicates():
    """The index lists of the 2-D heads repeat rows (nb4 / nb16 repeat neighbours): arco_cast_rows_f2h, arco_zero_rows and
    arco_zero_rows_h write a value that does not depend on the duplicate."""
    from arco_amd import _lib as L
    rs = np.random.RandomState(5)
    rows, c, scale = 500, 32, 256.0
    src = _rnd(rs, rows, c) * 1e-2
    idx = torch.from_numpy(rs.randint(0, rows, size=1203)).to(DEV)
    idx[:300] = idx[300:600]                                          # every one of these rows at least twice
    dst = torch.zeros((rows, c), dtype=F16, device=DEV)
    L.call("arco_cast_rows_f2h", L.ptr(src), c, c, L.ptr(idx), int(idx.numel()), scale, L.ptr(dst), c)
    touched = torch.zeros(rows, dtype=torch.bool, device=DEV)
    touched[idx] = True
    ref = torch.where(touched[:, None], (src * scale).to(F16), torch.zeros((), dtype=F16, device=DEV))
    assert torch.equal(dst, ref)
    s2 = src.clone()
    L.call("arco_zero_rows", L.ptr(s2), c, c, L.ptr(idx), int(idx.numel()))
    assert torch.equal(s2, torch.where(touched[:, None], torch.zeros((), device=DEV), src))
    L.call("arco_zero_rows_h", L.ptr(dst), c, c, L.ptr(idx), int(idx.numel()))
    assert float(dst.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# heads, eager (no graphs: the dense fallback of head._row_grad_buffer_h), at the step's shapes with 2 images
# ------------------------------------------------------------------------------------------------------------------------------
NB = 2
SHAPES = {"x1p": (384, 32), "x2p": (448, 64), "x3p": (480, 128), "f2": (64, 64), "f3": (32, 128), "f4": (16, 256)}
HEADS = {1: ("x3p", ["f4"], [496]), 2: ("x2p", ["f3", "f4"], [480, 496]), 3: ("x1p", ["f2", "f3", "f4"], [448, 480, 496])}


def _head_inputs(levels, seed=3):
    """(dense low-res input, the f16-representable maps as f16, the fea weights, w1, wq, pix, da)"""
    rs = np.random.RandomState(seed)
    lo_name, map_names, ks = HEADS[levels]
    c, s = SHAPES[lo_name]
    lo = _cl(_rnd(rs, NB, c, s, s))
    maps = [_cl(_rnd(rs, NB, SHAPES[m][0], SHAPES[m][1], SHAPES[m][1]).half()) for m in map_names]
    ws = [_rnd(rs, (496 if k == 496 else k), k, 1, 1) / np.sqrt(k) for k in ks]
    w1, wq = _rnd(rs, 496, 496, 1, 1) / np.sqrt(496), _rnd(rs, 496, 496, 1, 1) / np.sqrt(496)
    n = 1003                                                         # ~1000 anchors per step; not a multiple of 4
    pix = _pix(rs, n, NB, 256, 256)
    da = _rnd(rs, n, 496) * 1e-3
    return lo, maps, ws, w1, wq, pix, da


def _run_head(levels, lo, maps, ws, w1, wq, pix, da):
    """rows and every gradient of head.lazy_head2d on the given maps (f16 or fp32)."""
    from arco_amd import head
    lo_l = lo.clone().requires_grad_(True)
    maps_l = [m.clone().requires_grad_(True) for m in maps]
    par = [w.clone().requires_grad_(True) for w in ws + [w1, wq]]
    a = head.lazy_head2d(lo_l, maps_l, par[:levels], par[-2], par[-1], pix)
    a.backward(da)
    return a.detach(), lo_l.grad, [m.grad for m in maps_l], [p.grad for p in par]


def _f16_ulp(y):
    """one f16 unit in the last place of each element of y (fp32 values of f16 numbers); 2^-24 in the subnormal range and at 0"""
    e = torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


@pytest.mark.parametrize("levels,det,scale", [(1, 2, 16384.0), (2, 2, 16384.0), (3, 2, 16384.0), (3, 2, 256.0),
                                              (1, 0, 16384.0), (2, 0, 16384.0), (3, 0, 16384.0)])
def test_heads_on_f16_maps_equal_the_heads_on_their_fp32_copies(levels, det, scale, monkeypatch):
    """lazy_head2d at 1, 2 and 3 levels: an arm with the maps passed as f16 against an arm with the same maps upcast to fp32.
    (a) anchor rows bit-equal.  (b) order-independent scatter (DET_SCATTER = 2): weight gradients and the dense low-resolution input's
    gradient bit-equal, every f16 map gradient bit-equal to (fp32 gradient * LOSS_SCALE).to(f16) of the fp32 arm - what the dense
    boundary cast computes.  (c) fp32 atomics (DET_SCATTER = 0): fp32 gradients to 1e-5 of the tensor's maximum (the reproducibility
    tests' allowance for the atomics' arrival order), f16 map gradients to one f16 ulp of the element plus that 1e-5 x maximum.
    The three-level head runs at two loss scales (powers of two): the scale is applied exactly once."""
    from arco_amd import head, ops
    monkeypatch.setattr(head, "DET_SCATTER", det)
    ops.bump_weight_epoch()             # (no packed weight of an earlier test's tensors at a reused address)
    prev = ops.LOSS_SCALE
    ops.LOSS_SCALE = scale
    try:
        lo, maps, ws, w1, wq, pix, da = _head_inputs(levels)
        a16, dlo16, dm16, dp16 = _run_head(levels, lo, maps, ws, w1, wq, pix, da)
        a32, dlo32, dm32, dp32 = _run_head(levels, lo, [m.float() for m in maps], ws, w1, wq, pix, da)
        assert torch.equal(a16, a32) and bool(torch.isfinite(a32).all()) and float(a32.abs().max()) > 0       # (a)
        assert all(g.dtype == F16 for g in dm16) and all(g.dtype == F32 for g in dm32)
        assert all(g.shape == m.shape for g, m in zip(dm16, maps))
        ref16 = [(g * scale).to(F16) for g in dm32]
        for r in ref16:
            assert bool(torch.isfinite(r).all()) and float(r.float().abs().max()) > 1e-2     # neither saturated nor flushed away
        if det == 2:                                                                                            # (b)
            assert torch.equal(dlo16, dlo32)
            for x, y in zip(dp16, dp32):
                assert torch.equal(x, y)
            for i, (x, y) in enumerate(zip(dm16, ref16)):
                assert torch.equal(x, y), (i, float((x.float() - y.float()).abs().max()))
        else:                                                                                                   # (c)
            for x, y in zip([dlo16] + dp16, [dlo32] + dp32):
                assert float((x - y).abs().max()) <= 1e-5 * float(y.abs().max())
            for i, (x, y) in enumerate(zip(dm16, ref16)):
                x, y = x.float(), y.float()
                bound = _f16_ulp(y) + 1e-5 * float(y.abs().max())
                excess = float(((x - y).abs() - bound).max())
                print(f"levels {levels} map {i}: largest |f16 arm - rounded fp32 arm| {float((x - y).abs().max()):.3e}, excess over the bound {excess:.3e}")
                assert excess <= 0.0, (i, excess)
        # the gradient is row-sparse: untouched rows stay exactly zero
        g4 = dm16[-1].movedim(1, -1).reshape(-1, 16)
        assert 0 < int((g4.abs().sum(1) > 0).sum()) <= int(pix.numel())
    finally:
        ops.LOSS_SCALE = prev


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_teachers_on_f16_maps_equal_the_teachers_on_their_fp32_copies(levels):
    """LazyTeacher at 1, 2 and 3 levels: rows() and prototypes() bit-equal between f16 maps and their fp32 copies.  prototypes(): the f16
    form of arco_weighted_row_sum is the same template as the fp32 one (loss_front.hip weighted_row_sum_kernel<NDI, TS>): only the
    load differs (ld4f widens four f16 exactly), the accumulation order, the slab reduction and the finalize are shared - no
    tolerance."""
    from arco_amd import head, ops, _contrast as C_
    import fixture_inputs as fx
    ops.bump_weight_epoch()
    lo, maps, ws, w1, wq, pix, da = _head_inputs(levels, seed=4)
    inp = {k: v.to(DEV) for k, v in fx.loss_inputs(9, b=1, n_cls=4, feat=4, spatial=(256, 256)).items()}
    pl = C_.contrast_masks(inp["label_l"], inp["label_u"], inp["prob_l"], inp["prob_u"], inp["low_mask"], inp["high_mask"], 0.97)
    assert pl.n_img == NB
    t16 = head.LazyTeacher(lo, maps, ws)
    t32 = head.LazyTeacher(lo, [m.float() for m in maps], ws)
    r16, r32 = t16.rows(pix), t32.rows(pix)
    assert r16.shape == (int(pix.numel()), 496) and torch.equal(r16, r32) and float(r32.abs().max()) > 0
    p16, p32 = t16.prototypes(pl), t32.prototypes(pl)
    print(f"levels {levels}: prototypes, largest |f16 maps - fp32 copies| = {float((p16 - p32).abs().max()):.3e} of {float(p32.abs().max()):.3e}")
    assert p16.shape == (4, 496) and bool(torch.isfinite(p32).all()) and float(p32.abs().max()) > 0
    assert torch.equal(p16, p32)


# ------------------------------------------------------------------------------------------------------------------------------
# the step
# ------------------------------------------------------------------------------------------------------------------------------
def _hooks(st, seen):
    """Record (once per kind of pass) the dtypes a U-Net pass hands out: keyed by (net, images in the pass, grad mode)."""
    def note(net):
        def hook(m, i, o):
            seen.setdefault((net, int(i[0].shape[0]), torch.is_grad_enabled()), (o[0].dtype, o[1].dtype, [f.dtype for f in o[2]]))
        return hook
    return [st.model.register_forward_hook(note("s")), st.ema_model.register_forward_hook(note("t"))]


def _map_dtypes(keep):
    return [F32] * (5 - keep) + [F16] * keep


def test_fm_rows_graphs_captured_and_dtypes():
    """Six steps with --act_dtype f16 --fm_rows f16 in the default schedule (--head_levels 3, --teacher_levels 2)."""
    from arco_amd import ops
    try:
        st = _make(ROWS)
        assert ops.ACT_HALF and (st.args.graphs, st.args.graph_train, st.args.batch_transform, st.args.k2) == (1, 1, 1, 1.0)
        assert (st.args.head_levels, st.args.teacher_levels, st.fm_keep_s, st.fm_keep_t) == (3, 2, 3, 2)
        st.keep_debug = True
        seen = {}
        hs = _hooks(st, seen)
        for it in range(6):
            seed_all(700 + it)
            loss, reco = st.step(*_acdc_batch(it))
            assert bool(torch.isfinite(loss)) and bool(torch.isfinite(reco))
            assert all(bool(torch.isfinite(v)) for v in st.last_terms.values()), st.last_terms
            assert ops.FM_CAST is True
        for h in hs:
            h.remove()
        assert st.s_train_lu.captured and st.s_train_tps.captured
        assert st.s_train_lu.fm_cast == ("keep", 3) and st.s_train_tps.fm_cast is False
        # the f16 row gradients went through the graph's gradient sinks: no dense tensor, and both buffers of every f16 map are
        # back to zero after the step (the fp32 scratch re-zeroed by done(), the f16 gradient buffer by the registered cleanup)
        gt = st.s_train_lu
        torch.cuda.synchronize()
        assert gt.sink_uses > 0 and not gt.cleanup
        half_k = [k for k, i in enumerate(gt.diff_idx) if gt.flat_outs[i].dtype == F16]
        assert len(half_k) == 3 and sorted(gt._row_scratch) == half_k
        for k in half_k:
            assert gt.static_grads[k].dtype == F16 and float(gt.static_grads[k].float().abs().max()) == 0.0, k
            assert gt._row_scratch[k].dtype == F32 and float(gt._row_scratch[k].abs().max()) == 0.0, k
        # the grouped student pass: fp32 logits, fp32 bottleneck, the three finest maps as stored
        assert seen[("s", 16, True)] == (F32, F32, _map_dtypes(3)), seen
        # the teacher's grouped pass: the two finest maps as stored
        assert seen[("t", 16, False)] == (F32, F32, _map_dtypes(2)), seen
        # the logits-only passes cast no map: pseudo-label pass (teacher, 8 images), statistics pass (student, 8 images, no grad),
        # warped pass (student, 16 images with grad: same key as the grouped pass, seen second - checked through its capture above)
        assert seen[("t", 8, False)] == (F32, F16, [F16] * 5), seen
        assert seen[("s", 8, False)] == (F32, F16, [F16] * 5), seen
        assert st.overflow_steps == 0 and ops.LOSS_SCALE == 16384.0
        assert all(bool(torch.isfinite(p).all()) for p in st.ema_model.parameters())
        assert all(bool(torch.isfinite(m[0]).all()) for m in st.memobank)
        _check_step_invariants(st, "smc", 4096, 496, 705)
        assert "f16 rows of f2, f3, f4 (student) and f3, f4 (teacher)" in st.fm_rows_note()
    finally:
        st = None
        _reset()


def _one_step(extra, seed=11, steps=1):
    st = _make(THRESH + list(extra), seed)
    _drop_off(st)
    seen = {}
    hs = _hooks(st, seen)
    terms = []
    for it in range(steps):
        seed_all(600 + 10 * seed + it)
        st.step(*_acdc_batch(it))
        terms.append([float(st.last_terms[k]) for k in TERMS])
    for h in hs:
        h.remove()
    return st, np.array(terms), seen


def test_fm_rows_first_step_equals_plain_f16():
    """Same seed, same batches, dropout off, one step each: the five logged terms come from forwards that are bit-identical between
    --act_dtype f16 and --act_dtype f16 --fm_rows f16 (exact widening in the row kernels and the weighted row sums)."""
    from arco_amd import ops
    try:
        st_a, t_a, _ = _one_step(["--act_dtype", "f16"])
        del st_a
        _reset()
        st_b, t_b, seen = _one_step(ROWS)
        assert ops.ACT_HALF and seen[("s", 16, True)][2] == _map_dtypes(3)
        for i, k in enumerate(TERMS):
            print(f"{k}: plain f16 {t_a[0, i]!r}  fm_rows f16 {t_b[0, i]!r}")
        assert np.all(np.isfinite(t_a)) and np.all(np.abs(t_a) > 1e-3), t_a
        np.testing.assert_allclose(t_b, t_a, rtol=1e-6, atol=0)
        assert st_b.overflow_steps == 0
    finally:
        st_a = st_b = None
        _reset()


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_fm_rows_step_tracks_fp32(seed):
    """test_f16_2d_step_tracks_fp32 with --fm_rows f16, held to the same bounds (TRAJ_RTOL, imported): the new mode's forward is
    bit-identical to the plain f16 mode's and its map gradients are the same roundings of the same sums, so its distance to the
    --conv_mma f32 arm is the plain mode's up to the atomics' order - and those bounds are 3 x that measured distance."""
    from arco_amd import ops
    try:
        st32, t32 = _three_steps(["--conv_mma", "f32"], seed)
        assert not ops.ACT_HALF and ops.CONV_MMA == 0
        del st32
        _reset()
        st16, t16 = _three_steps(ROWS, seed)
        assert ops.ACT_HALF and ops.CONV_MMA == 3 and st16.fm_keep_s == 3
        rel = np.abs(t16 - t32) / np.abs(t32)
        for i, k in enumerate(TERMS):
            print(f"seed {seed} {k}: fp32 {t32[:, i]}  f16 rows {t16[:, i]}  relative distance {rel[:, i]}")
        assert np.all(np.isfinite(t16)) and np.all(np.isfinite(t32))
        assert np.all(np.abs(t32) > 1e-3), t32
        assert not np.array_equal(t16, t32)
        np.testing.assert_allclose(t16[0, :2], t32[0, :2], rtol=1e-2)
        for i, k in enumerate(TERMS):
            np.testing.assert_allclose(t16[:, i], t32[:, i], rtol=TRAJ_RTOL[k], err_msg=k)
        assert st16.overflow_steps == 0
        _check_step_invariants(st16, "smc", 4096, 496, 600 + 10 * seed + 2)
    finally:
        st16 = None
        _reset()


@pytest.mark.parametrize("levels,keep_s,keep_t", [(2, 2, 2), (1, 1, 1)])
def test_fm_rows_other_head_levels(levels, keep_s, keep_t):
    """--head_levels 2 and 1, two steps each: finite terms, the maps the heads read as rows (and only those) are f16."""
    try:
        st, t, seen = _one_step(ROWS + ["--head_levels", str(levels)], steps=2)
        assert (st.fm_keep_s, st.fm_keep_t) == (keep_s, keep_t)
        assert np.all(np.isfinite(t)), t
        assert seen[("s", 16, True)] == (F32, F32, _map_dtypes(keep_s)), seen
        assert seen[("t", 16, False)] == (F32, F32, _map_dtypes(keep_t)), seen
        assert st.overflow_steps == 0
        assert all(bool(torch.isfinite(p).all()) for p in st.model.parameters())
    finally:
        st = None
        _reset()


def test_fm_rows_teacher_levels_3_keeps_three_teacher_maps():
    try:
        st, t, seen = _one_step(ROWS + ["--teacher_levels", "3"], steps=1)
        assert np.all(np.isfinite(t)), t
        assert seen[("t", 16, False)] == (F32, F32, _map_dtypes(3)), seen
    finally:
        st = None
        _reset()


def test_fm_rows_without_train_graphs_and_without_batched_passes():
    """--graph_train 0 (the dense fallback of head._row_grad_buffer_h on every step), --graphs 0 and --batched_passes 0: two steps each,
    first-step terms equal to the default schedule's first step (rtol 1e-6: the same forwards)."""
    try:
        st, t_ref, _ = _one_step(ROWS, steps=2)
        del st
        _reset()
        for extra in (["--graph_train", "0"], ["--graphs", "0"], ["--batched_passes", "0"]):
            st, t, seen = _one_step(ROWS + extra, steps=2)
            print(extra, t[0], t_ref[0])
            assert np.all(np.isfinite(t)), (extra, t)
            assert st.overflow_steps == 0
            if extra[0] == "--batched_passes":
                assert seen[("s", 8, True)] == (F32, F32, _map_dtypes(3)), seen
            else:
                np.testing.assert_allclose(t[0], t_ref[0], rtol=1e-6, err_msg=str(extra))
            assert all(bool(torch.isfinite(p).all()) for p in st.model.parameters())
            del st
            _reset()
    finally:
        st = None
        _reset()


def test_default_stepper_after_fm_rows_hands_out_fp32_maps():
    from arco_amd import ops
    try:
        st, _, _ = _one_step(ROWS)
        del st
        torch.cuda.empty_cache()
        st, t, seen = _one_step([])
        assert not ops.ACT_HALF and ops.FM_CAST is True and st.fm_keep_s == 0
        assert np.all(np.isfinite(t))
        for key, (lg, x4, maps) in seen.items():
            assert lg == F32 and x4 == F32 and maps == [F32] * 5, (key, maps)
        assert ("s", 16, True) in seen and ("t", 16, False) in seen
        del st
        _reset()
        st, t, seen = _one_step(["--act_dtype", "f16"])            # plain f16 after it: five fp32 maps from every pass
        for key, (lg, x4, maps) in seen.items():
            assert lg == F32 and x4 == F32 and maps == [F32] * 5, (key, maps)
    finally:
        st = None
        _reset()
