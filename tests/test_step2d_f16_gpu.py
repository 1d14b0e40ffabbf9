"""The 2-D step on f16 activation storage (train_arco_2d --act_dtype f16) at the benchmarked size (8 + 8 images of 256 x 256,
4 classes, --queue_size 4096) in the trainer's default schedule (graphs, batched passes, side streams, batch_transform, k2 = 1)."""
import numpy as np
import pytest
import torch

from test_configs_at_size_gpu import _acdc_batch, _check_step_invariants, _drop_off, seed_all

pytestmark = pytest.mark.gpu

TERMS = ("ce", "dice", "unsup", "reco", "eqv")
# Trajectory bounds per term: 3 x the largest relative distance measured over seeds 11-13 and three steps (profiles/f16_2d_notes.md:
# ce 7.3e-4, dice 1.2e-4, unsup 2.8e-4, reco 3.4e-4, eqv 8.2e-3; two runs of each seed - the third step differs from run to run by
# ~1e-4 through the fp32 atomics), never looser than the 5e-2 the 3-D test allows a trajectory
TRAJ_RTOL = {"ce": 2.2e-3, "dice": 3.5e-4, "unsup": 8.4e-4, "reco": 1.02e-3, "eqv": 2.5e-2}


def _make(extra, seed=11):
    from arco_amd import train_arco_2d as T
    args = T.build_parser().parse_args(["--batch_size", "8", "--queue_size", "4096", "--synthetic", "1", "--k1", "1.0"] + list(extra))
    args.patch_size = [256, 256]
    seed_all(seed)
    return T.ArcoStep2D(args, "cuda:0")


def _reset():
    from arco_amd import ops
    ops.ACT_HALF = False
    ops.LOSS_SCALE = 16384.0
    ops.CONV_MMA = 3
    ops.bump_weight_epoch()
    torch.cuda.empty_cache()


# thresholds that leave no compared term an exact zero with untrained 4-class weights (the defaults 0.97 / 0.7 mask every pixel)
THRESH = ["--strong_threshold", "0.3", "--weak_threshold", "0.3"]


def _three_steps(extra, seed):
    st = _make(THRESH + list(extra), seed)
    _drop_off(st)
    st.keep_debug = True
    terms = []
    for it in range(3):
        seed_all(600 + 10 * seed + it)
        st.step(*_acdc_batch(it))
        terms.append([float(st.last_terms[k]) for k in TERMS])
    return st, np.array(terms)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_f16_2d_step_tracks_fp32(seed):
    """test_cfg5_lits_f16_step_at_full_size_tracks_fp32 restated for the 2-D step: three steps from the same weights and batches,
    dropout off, f16 storage against --conv_mma f32.  First step's CE / Dice: rtol 1e-2 (BASELINE.json configs[4]'s budget for the f16
    mode).  Later steps and the other terms: TRAJ_RTOL, 3 x the largest measured distance per term (profiles/f16_2d_notes.md)."""
    from arco_amd import ops
    try:
        st32, t32 = _three_steps(["--conv_mma", "f32"], seed)
        assert not ops.ACT_HALF and ops.CONV_MMA == 0
        del st32
        _reset()
        st16, t16 = _three_steps(["--act_dtype", "f16"], seed)
        assert ops.ACT_HALF and ops.CONV_MMA == 3
        rel = np.abs(t16 - t32) / np.abs(t32)
        for i, k in enumerate(TERMS):
            print(f"seed {seed} {k}: fp32 {t32[:, i]}  f16 {t16[:, i]}  relative distance {rel[:, i]}")
        assert np.all(np.isfinite(t16)) and np.all(np.isfinite(t32))
        assert np.all(np.abs(t32) > 1e-3), t32                    # no compared term is an exact zero in the fp32 arm
        assert not np.array_equal(t16, t32)                       # the f16 kernels really ran
        np.testing.assert_allclose(t16[0, :2], t32[0, :2], rtol=1e-2)
        for i, k in enumerate(TERMS):
            np.testing.assert_allclose(t16[:, i], t32[:, i], rtol=TRAJ_RTOL[k], err_msg=k)
        assert st16.overflow_steps == 0
        _check_step_invariants(st16, "smc", 4096, 496, 600 + 10 * seed + 2)
    finally:
        st16 = None
        _reset()


def test_f16_2d_graphs_captured_and_replayed():
    """Six steps in the default schedule: the student passes replay as HIP graphs; the activations inside the U-Net are f16, the
    logits and the heads' inputs fp32."""
    from arco_amd import ops
    try:
        st = _make(["--act_dtype", "f16"])
        assert ops.ACT_HALF and (st.args.graphs, st.args.graph_train, st.args.batch_transform, st.args.k2) == (1, 1, 1, 1.0)
        seen = {}
        def note(key, value):           # (a forward hook that returns a value would replace the module's output)
            seen.setdefault(key, value)

        h1 = st.model.encoder.down2.maxpool_conv[1].register_forward_hook(
            lambda m, i, o: note("block", (o[0] if isinstance(o, tuple) else o).dtype))
        h2 = st.model.register_forward_hook(lambda m, i, o: note("out", (o[0].dtype, o[1].dtype, [f.dtype for f in o[2]])))
        h3 = st.q_feature_extractor.register_forward_pre_hook(lambda m, i: note("head_in", [f.dtype for f in i[0]]))
        for it in range(6):
            seed_all(700 + it)
            loss, reco = st.step(*_acdc_batch(it))
            assert bool(torch.isfinite(loss)) and bool(torch.isfinite(reco))
        for h in (h1, h2, h3):
            h.remove()
        assert st.s_train_lu.captured and st.s_train_tps.captured
        assert seen["block"] == torch.float16
        assert seen["out"] == (torch.float32, torch.float32, [torch.float32] * 5)
        assert all(d == torch.float32 for d in seen.get("head_in", [torch.float32]))
        assert st.overflow_steps == 0 and ops.LOSS_SCALE == 16384.0
        assert all(torch.isfinite(p).all() for p in st.ema_model.parameters())
    finally:
        st = None
        _reset()


def test_f16_2d_overflow_is_survived():
    """One rank, six steps, an inf written into one element of the U-Net's stretch of the flat gradient at step 3 (a value in a
    buffer, as tools/ddp_check3d.py does it for the V-Net): the U-Net's gradient of that step is all zeros when SGD reads it, the
    heads' update is applied, teacher and banks stay finite, the next step halves the loss scale."""
    from arco_amd import ops
    try:
        st = _make(["--act_dtype", "f16"])
        scale0 = ops.LOSS_SCALE
        real_guard, real_step = st._unscale_and_guard, st.optimizer.step
        state = {"i": -1}

        def guard():
            if state["i"] == 3:
                st.optimizer.flat_g[7] = float("inf")
            return real_guard()

        def opt_step():
            if state["i"] == 3:
                state["unet_g"] = st.optimizer.flat_g[:st.heads_start].clone()
                state["heads_g"] = st.optimizer.flat_g[st.heads_start:].clone()
                state["heads_p"] = st.optimizer.flat_p[st.heads_start:].clone()
            return real_step()

        st._unscale_and_guard, st.optimizer.step = guard, opt_step
        flags = []
        for i in range(6):
            state["i"] = i
            seed_all(800 + i)
            loss, reco = st.step(*_acdc_batch(i))
            torch.cuda.synchronize()
            flags.append(bool(st._ovf_host[0]))
            if i == 3:
                assert float(state["unet_g"].abs().max()) == 0.0                 # a zero-gradient step for the U-Net
                assert float(state["heads_g"].abs().max()) > 0.0 and bool(torch.isfinite(state["heads_g"]).all())
                assert not torch.equal(state["heads_p"], st.optimizer.flat_p[st.heads_start:])      # the heads' update was applied
            if i == 4:
                assert ops.LOSS_SCALE == scale0 / 2
            if i > 3:
                assert all(bool(torch.isfinite(v)) for v in st.last_terms.values()), st.last_terms
        assert flags == [True, True, True, False, True, True], flags
        assert st.overflow_steps == 1
        assert all(bool(torch.isfinite(p).all()) for p in st.ema_model.parameters())
        assert bool(torch.isfinite(st.optimizer.flat_p).all())
        assert all(bool(torch.isfinite(m[0]).all()) for m in st.memobank)
    finally:
        st = None
        _reset()


def test_default_stepper_after_f16_is_fp32():
    """An f16 stepper, then a default one in the same process: ops.ACT_HALF is off again and the default stepper's first step equals
    that of a default stepper built in a fresh state (up to the 1e-5 the reproducibility tests grant the atomics)."""
    from arco_amd import ops

    def first_step():
        st = _make([])
        seed_all(900)
        ops.reseed_dropout(900)          # (the dropout seeds come from a process-wide generator: rewind it for both steppers)
        st.step(*_acdc_batch(0))
        out = (np.array([float(st.last_terms[k]) for k in TERMS]), st.optimizer.flat_g.clone())
        del st
        torch.cuda.empty_cache()
        return out

    try:
        t_ref, g_ref = first_step()
        st16 = _make(["--act_dtype", "f16", "--loss_scale", "1024"])
        assert ops.ACT_HALF and ops.LOSS_SCALE == 1024.0
        seed_all(900)
        st16.step(*_acdc_batch(0))
        del st16
        torch.cuda.empty_cache()
        t_new, g_new = first_step()
        assert not ops.ACT_HALF
        np.testing.assert_allclose(t_new, t_ref, rtol=1e-5)
        assert float((g_new - g_ref).abs().max()) <= 1e-5 * float(g_ref.abs().max())
    finally:
        _reset()
