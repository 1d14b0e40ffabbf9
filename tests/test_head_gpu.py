"""Row-sparse student head vs the dense reference dataflow (same step, same seeds) (-m gpu)."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _run(dense, steps=2, levels=2, dense_teacher=1):
    from arco_amd import ops
    from arco_amd import train_arco_2d as T
    random.seed(3); np.random.seed(3); torch.manual_seed(3)
    ops.reseed_dropout(99)
    args = T.build_parser().parse_args(["--batch_size", "2", "--queue_size", "300", "--synthetic", "1",
                                        "--num_queries", "64", "--num_negatives", "32", "--dense_head", str(dense),
                                        "--k1", "1.0", "--base_lr", "0.05", "--head_levels", str(levels), "--dense_teacher", str(dense_teacher),
                                        "--teacher_levels", str(min(levels, 3) if levels >= 2 else 2)])
    args.patch_size = [64, 64]
    st = T.ArcoStep2D(args, "cuda:0")
    losses = []
    for i in range(steps):
        l_img, l_lab = T.synthetic_batch(2, args.patch_size, 4, 10 + i, "cuda:0")
        u_img, _ = T.synthetic_batch(2, args.patch_size, 4, 20 + i, "cuda:0")
        loss, reco = st.step(l_img, l_lab, u_img)
        losses.append(float(reco.detach()))
    params = torch.cat([p.detach().reshape(-1) for p in st.optimizer.params]).cpu()
    teacher = torch.cat([p.detach().reshape(-1) for p in st.ema_model.parameters()]).cpu()
    banks = [b[0].cpu() for b in st.memobank]
    return losses, params, teacher, banks


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_lazy_head_matches_dense_step(levels):
    l_d, p_d, t_d, b_d = _run(1)
    l_s, p_s, t_s, b_s = _run(0, levels=levels)
    assert all(abs(l) > 1e-3 for l in l_d)
    np.testing.assert_allclose(l_s, l_d, rtol=1e-5, atol=1e-6)
    for x, y in zip(b_s, b_d):
        np.testing.assert_allclose(x.numpy(), y.numpy(), rtol=1e-3, atol=1e-5)   # teacher = EMA of students that differ by summation order
    # parameters after 2 SGD steps: identical up to fp32 summation order of the weight gradients
    np.testing.assert_allclose(p_s.numpy(), p_d.numpy(), rtol=1e-3, atol=1e-4)      # (float-atomics scatters: one of 3.2 M weights was seen 7.5e-5 off)
    np.testing.assert_allclose(t_s.numpy(), t_d.numpy(), rtol=1e-4, atol=1e-6)
    assert float((p_s - p_d).abs().max()) < 1e-3


@pytest.mark.parametrize("levels", [2, 3])
def test_lazy_teacher_matches_dense_teacher(levels):
    """Linear-prototype + lazy-key teacher path vs the dense teacher representation (same sparse student head)."""
    l_d, p_d, t_d, b_d = _run(0, dense_teacher=1, levels=levels)
    l_s, p_s, t_s, b_s = _run(0, dense_teacher=0, levels=levels)
    # (both runs scatter row gradients with float atomics - DESIGN.md 7 - so step 2 sees weights that differ in the last
    #  bits from run to run; the tolerances leave room for that: one run in ~6 crossed 5e-5 / 2e-5)
    np.testing.assert_allclose(l_s, l_d, rtol=2e-4, atol=1e-6)
    for x, y in zip(b_s, b_d):
        assert x.shape == y.shape
        np.testing.assert_allclose(x.numpy(), y.numpy(), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(p_s.numpy(), p_d.numpy(), rtol=1e-3, atol=1e-4)      # (float-atomics scatters: one of 3.2 M weights was seen 7.5e-5 off)


@pytest.mark.parametrize("half", [False, True])
def test_three_level_3d_head_and_teacher_match_the_two_level_ones_on_the_dense_map(half):
    """head.lazy_head3d / LazyTeacher with three maps (fea2 evaluated on the eight corner rows of every sampled voxel; model_3D.py:46-58 one level
    further down than with two maps) against the two-level head fed the DENSE x2p = fea2(cat(up(x1p), f2)) + cat(...) built with
    autograd-capable ops in the reference's order: anchors' rows, every gradient (x1p, f2, f3, f4, fea2 / fea3 / fea4 / q_representation
    weights), the teacher's prototypes and key rows.  half: f3 / f4 read as stored f16 (ops.fm_rows_half)."""
    from arco_amd import head, ops, _contrast as C_
    import fixture_inputs as fx
    dev = "cuda:0"
    rs = np.random.RandomState(11)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last_3d)
    nb, c1, c2, c3, c4 = 2, 192, 32, 16, 16
    sp1, sp2, sp3 = (4, 5, 3), (8, 10, 6), (16, 20, 12)
    k2, k3 = c1 + c2, c1 + c2 + c3
    rnd = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(dev)
    x1p, f2 = cl(rnd(nb, c1, *sp1)), cl(rnd(nb, c2, *sp2))
    f3, f4 = cl(rnd(nb, c3, *sp3)), cl(rnd(nb, c4, *sp3))
    if half:
        f3, f4 = cl(f3.half()), cl(f4.half())
    w2 = rnd(k2, k2, 1, 1, 1) / np.sqrt(k2)
    w3 = rnd(k3, k3, 1, 1, 1) / np.sqrt(k3)
    w4 = rnd(16, k3 + c4, 1, 1, 1) / np.sqrt(k3 + c4)
    w1, wq = rnd(16, 16, 1, 1, 1) / 4, rnd(16, 16, 1, 1, 1) / 4
    n_vox = nb * sp3[0] * sp3[1] * sp3[2]
    pix = torch.from_numpy(rs.randint(0, n_vox, size=200)).to(dev)
    pix[5] = pix[2]; pix[60] = pix[2]; pix[0] = 0; pix[1] = n_vox - 1          # repeated voxels, the two extreme corners
    da = rnd(200, 16) * 1e-2
    prev_scale = ops.LOSS_SCALE
    ops.LOSS_SCALE = 256.0
    try:
        res = {}
        for mode in ("l3", "l2"):
            lv = [t.clone().requires_grad_(True) for t in (x1p, f2, w2, w3, w4, w1, wq)]
            f3l, f4l = f3.clone().requires_grad_(True), f4.clone().requires_grad_(True)
            if mode == "l3":
                a = head.lazy_head3d(lv[0], [lv[1], f3l, f4l], lv[2:5], lv[5], lv[6], pix)
            else:
                X2 = torch.cat((ops.trilinear(lv[0], sp2), lv[1]), dim=1)
                x2p = ops.conv(X2, lv[2], None, residual=True)
                a = head.lazy_head3d(x2p, [f3l, f4l], lv[3:5], lv[5], lv[6], pix)
            a.backward(da)
            res[mode] = [a.detach()] + [t.grad for t in lv] + [f3l.grad, f4l.grad]
        names = ["rows", "dx1p", "df2", "dw2", "dw3", "dw4", "dw1", "dwq", "df3", "df4"]
        for nme, x, y in zip(names, res["l3"], res["l2"]):
            assert x.shape == y.shape and x.dtype == y.dtype, nme
            tol = 2.0 ** -9 if (half and nme in ("df3", "df4")) else 2e-5        # (f16 gradients: one rounding of sums that differ in the last fp32 bits)
            err = float((x.float() - y.float()).abs().max()) / max(1e-20, float(y.float().abs().max()))
            assert err <= tol, (nme, err)
        assert float(res["l3"][2].abs().max()) > 0 and float(res["l3"][1].abs().max()) > 0
        # untouched f2 rows stay exactly zero (row-sparse gradient)
        touched = int((res["l3"][2].movedim(1, -1).reshape(-1, c2).abs().sum(1) > 0).sum())
        assert 0 < touched <= 8 * 200
        # teacher
        inp = {k: v.to(dev) for k, v in fx.loss_inputs(9, b=1, n_cls=3, feat=16, spatial=sp3).items()}
        pl = C_.contrast_masks(inp["label_l"], inp["label_u"], inp["prob_l"], inp["prob_u"], inp["low_mask"], inp["high_mask"], 0.97)
        with torch.no_grad():
            x2p = ops.conv(torch.cat((ops.trilinear(x1p, sp2), f2), dim=1), w2, None, residual=True)
        t3 = head.LazyTeacher(x1p, [f2, f3, f4], [w2, w3, w4])
        t2 = head.LazyTeacher(x2p, [f3, f4], [w3, w4])
        p3, p2 = t3.prototypes(pl), t2.prototypes(pl)
        assert p3.shape == p2.shape and float((p3 - p2).abs().max()) <= 2e-5 * float(p2.abs().max())
        r3, r2 = t3.rows(pix), t2.rows(pix)
        assert float((r3 - r2).abs().max()) <= 2e-5 * float(r2.abs().max())
    finally:
        ops.LOSS_SCALE = prev_scale


_F64_SIDES = [(5, 7), (11, 9), (22, 18), (44, 36)]        # not x2, not square: a swapped H / W or a wrong level order shows
_F64_REF = {}


def _float64_head_case(levels):
    """(fp32 CPU inputs, float64 reference outputs) of the 2-D head at `levels` levels, built once per depth and left unchanged:
    2 images, the last levels + 1 sides of _F64_SIDES, 64 channels on lo, 16 on every map, D = 32, weights scaled by 1 / sqrt(K),
    203 pixels with pixel 0, the last pixel and one pixel three times.  The reference is the dense module in float64:
    x <- fea_i(cat(up(x), f_i)) + cat(up(x), f_i) (model_2D.py:43-50), fea4 without the residual, q_representation, row selection."""
    if levels in _F64_REF:
        return _F64_REF[levels]
    import torch.nn.functional as F
    rs = np.random.RandomState(40 + levels)
    rnd = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    nb, clo, cm, D, n = 2, 64, 16, 32, 203
    sides = _F64_SIDES[3 - levels:]
    lo = rnd(nb, clo, *sides[0])
    maps = [rnd(nb, cm, *s) for s in sides[1:]]
    ks = [clo + cm * (i + 1) for i in range(levels)]
    feas = [rnd(k, k, 1, 1) / np.sqrt(k) for k in ks[:-1]] + [rnd(D, ks[-1], 1, 1) / np.sqrt(ks[-1])]
    q1, q2 = rnd(D, D, 1, 1) / np.sqrt(D), rnd(D, D, 1, 1) / np.sqrt(D)
    n_pix = nb * sides[-1][0] * sides[-1][1]
    pix = torch.from_numpy(rs.randint(0, n_pix, size=n))
    pix[0] = 0; pix[1] = n_pix - 1; pix[10] = pix[20] = pix[30]
    da = rnd(n, D)
    lv = [t.double().requires_grad_(True) for t in (lo, *maps, *feas, q1, q2)]
    x = lv[0]
    for i in range(levels):
        m, w = lv[1 + i], lv[1 + levels + i]
        x = torch.cat((F.interpolate(x, size=m.shape[2:], mode="bilinear", align_corners=True), m), dim=1)
        x = F.conv2d(x, w) + x if i < levels - 1 else F.conv2d(x, w)
    x = F.conv2d(F.conv2d(x, lv[-2]), lv[-1])
    rows = x.permute(0, 2, 3, 1).reshape(n_pix, D)[pix]
    rows.backward(da.double())
    _F64_REF[levels] = ((lo, maps, feas, q1, q2, pix, da), [rows.detach()] + [t.grad for t in lv])
    return _F64_REF[levels]


@pytest.mark.parametrize("det", [0, 2])
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_lazy_head_2d_vs_float64(levels, det, monkeypatch):
    """head.lazy_head2d at every depth, with fp32 atomics and with the order-independent scatter, against the dense module restated in
    float64 on the CPU (_float64_head_case): the rows, the gradient of lo, of every map and of every weight to 1e-4 of the tensor's
    largest magnitude (the standing bar for fp32 kernels against float64), and the finest map's gradient exactly zero on every row
    that `pix` does not name."""
    from arco_amd import head, ops
    monkeypatch.setattr(head, "DET_SCATTER", det)
    ops.bump_weight_epoch()
    dev = "cuda:0"
    (lo, maps, feas, q1, q2, pix, da), ref = _float64_head_case(levels)
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    lo_g, maps_g = cl(lo), [cl(m) for m in maps]
    par = [w.to(dev).requires_grad_(True) for w in (*feas, q1, q2)]
    a = head.lazy_head2d(lo_g, maps_g, par[:levels], par[-2], par[-1], pix.to(dev))
    a.backward(da.to(dev))
    got = [a.detach()] + [t.grad for t in (lo_g, *maps_g, *par)]
    names = ["rows", "dlo"] + [f"dmap{i}" for i in range(levels)] + [f"dfea{i}" for i in range(levels)] + ["dq1", "dq2"]
    errs = []
    for nme, x, y in zip(names, got, ref):
        assert x is not None and x.shape == y.shape, nme
        peak = float(y.abs().max())
        errs.append((nme, float((x.double().cpu() - y).abs().max()) / peak, peak))
    print(f"levels {levels} det {det}: " + ", ".join(f"{nme} {e:.2e}" for nme, e, _ in errs))
    for nme, e, peak in errs:
        assert peak > 0 and e <= 1e-4, (nme, e)
    g = got[1 + levels].movedim(1, -1).reshape(-1, int(maps[-1].shape[1]))
    named = torch.zeros(g.shape[0], dtype=torch.bool, device=g.device)
    named[pix.to(dev)] = True
    assert float(g[~named].abs().max()) == 0.0 and float(g[named].abs().max()) > 0
