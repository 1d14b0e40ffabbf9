"""--gpu_ingest 1 of the pre-trainers on the device (-m gpu): the two kernels of csrc/stage1_aug.hip against the numpy restatements of
tests/stage1_aug_refs.py (which tests/test_pretrain_ingest_cpu.py holds to jitter_gray_ and to Pillow) - exactly -, the bank loader
against the host loader, the device transforms against the restatement chain, and both trainers with the flag against without."""
import os
import random

import numpy as np
import pytest
import torch

import ingest_refs as R
import stage1_aug_refs as S

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(got, want):
    want = torch.from_numpy(np.array(want)) if isinstance(want, np.ndarray) else want          # (a copy: the cases are read-only)
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape
    return torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("kind", sorted(S.FACTOR_SETS))
@pytest.mark.parametrize("shape", S.SHAPES_2D + S.SHAPES_3D)
def test_jitter_kernel_equals_restatement(shape, kind):
    """Bit for bit, all 24 orders dealt over the planes of as many launches as that takes, values inside and outside [0, 1]; a second
    launch on the same input gives the same bits."""
    from arco_amd.dataloaders import stage1_aug as A
    for start in S.case_starts(shape):
        x, params, want = S.jitter_case(shape, kind, start)
        recs = A.jitter_records(params)
        runs = []
        for _ in range(2):
            img = torch.from_numpy(x.copy()).cuda()
            assert A.gray_jitter_planes(img, recs) is img
            runs.append(img)
        assert _same_bits(runs[0], want), (shape, kind, start)
        assert _same_bits(runs[1], runs[0].cpu())


@pytest.mark.parametrize("shape", [S.SHAPES_2D[1], S.SHAPES_3D[0], S.SHAPES_3D[1]])
def test_jitter_kernel_leaves_unnamed_planes_alone(shape):
    """A buffer of one image more than the records name, and records that stop two planes short of the named images' end: the named
    planes get the jitter, every other plane keeps its bits."""
    from arco_amd import _lib
    from arco_amd.dataloaders import stage1_aug as A
    x, params, want = S.jitter_case(shape, "both", 0)
    n = max(len(params) - 2, 1)
    big = np.concatenate([x, S.jitter_input((1,) + shape[1:], 5)])
    exp = big.copy()
    for v, w in list(zip(S.plane_views(exp), S.plane_views(want)))[:n]:
        v[...] = w
    buf = torch.from_numpy(big.copy()).cuda()
    n_elems, B, T, H, W, strides = A._planes(buf)
    recs = torch.from_numpy(A.jitter_records(params[:n]).view(np.uint8).reshape(-1)).cuda()
    _lib.call("arco_gray_jitter_planes", _lib.ptr(buf), n_elems, n, T, H, W, *strides, _lib.ptr(recs))
    assert _same_bits(buf, exp)
    with pytest.raises(RuntimeError, match="arco_gray_jitter_planes"):          # more planes than the buffer holds
        _lib.call("arco_gray_jitter_planes", _lib.ptr(buf), n_elems, (B + 1) * T, T, H, W, *strides, _lib.ptr(recs))


@pytest.mark.parametrize("sigma", S.SIGMAS)
@pytest.mark.parametrize("hw", S.BLUR_PLANES)
def test_blur_kernel_equals_restatement(hw, sigma):
    """Exactly, both output modes, planes larger than a tile (tile borders inside the image, where the in-place mode would race if
    it stored into the buffer it reads); T = 5 and 17 of the volume layout, T = 3 (the wide tile on a group of planes) and the slice
    layout."""
    from arco_amd.dataloaders import stage1_aug as A
    for T in S.BLUR_T + (3, None):
        shape = (3, 1) + hw if T is None else (2, 1) + hw + (T,)
        x = S.jitter_input(shape, 40 + (T or 0))                                      # values inside and outside [0, 1]
        want = S.blur_image(x, sigma)                                                  # uint8 [B * T, H, W]
        img = torch.from_numpy(x.copy()).cuda()
        out = A.blur_planes(img, sigma, inplace=False)
        assert out is not img and _same_bits(img, x)                                  # a new tensor, the input untouched
        assert _same_bits(out, want.astype(np.float32) / np.float32(255.0)), (shape, sigma)
        if T is not None:
            back = np.empty(shape, np.float32)
            for v, w in zip(S.plane_views(back), want):
                v[...] = w
            assert A.blur_planes(img, sigma, inplace=True) is img
            assert _same_bits(img, back), (shape, sigma)


def test_blur_kernel_refuses_other_radius_classes():
    from arco_amd import _lib
    from arco_amd.dataloaders import stage1_aug as A
    img = torch.zeros(2, 1, 16, 16, device="cuda")
    n_elems, B, T, H, W, strides = A._planes(img)
    out = torch.empty(2, 16, 16, device="cuda")
    for radius in (1.0, 1.5, -0.25):
        with pytest.raises(RuntimeError, match="arco_blur_planes"):
            _lib.call("arco_blur_planes", _lib.ptr(img), n_elems, B, T, H, W, *strides, radius, _lib.ptr(out), None)
    with pytest.raises(RuntimeError, match="arco_blur_planes"):
        A.blur_planes(img, 2.0, inplace=False)                                        # a sigma RandomNoise never draws: radius >= 1
    _lib.call("arco_blur_planes", _lib.ptr(img), n_elems, B, T, H, W, *strides, 0.999, _lib.ptr(out), None)
    with pytest.raises(ValueError):
        A.blur_planes(img.double(), 0.5, inplace=False)


def _batches(loader, n):
    """The trainer's loop over `n` iterations: a fresh iterator per epoch; image / label / idx on the CPU."""
    out = []
    while len(out) < n:
        for b in loader:
            out.append({k: b[k].cpu() for k in ("image", "label", "idx")})
            if len(out) == n:
                break
    return out


def _assert_bank_loader_equals_host_loader(host, seed):
    from arco_amd.dataloaders import gpu_ingest as G
    S.seed_all(seed)
    h = _batches(host, 6)
    dev = G.bank_loader(host, "cuda:0")
    assert len(dev) == len(host) < 6                                                  # 6 iterations cross an epoch boundary
    S.seed_all(seed)
    d = _batches(dev, 6)
    for hb, db in zip(h, d):
        assert torch.equal(hb["idx"], db["idx"])
        assert db["image"].dtype == torch.float32 and _same_bits(db["image"], hb["image"])
        assert db["label"].dtype == torch.int64 and torch.equal(hb["label"].long(), db["label"])
    return dev


def test_bank_loader_equals_host_loader_2d(tmp_path):
    from arco_amd import pretrain_2D as P
    root = R.write_slice_dataset(tmp_path)
    args = P.build_parser().parse_args(["--root_path", str(root), "--exp", "ACDC/ingest_test", "--labeled_num", "1", "--batch_size", "12",
                                        "--labeled_bs", "6"])
    dev = _assert_bank_loader_equals_host_loader(P.build_loader(args), 3)
    assert dev.bank.n_cases == 30 and dev.bank.nbytes == 30 * 40 * 36 * 5 + 30 * 32


def test_bank_loader_equals_host_loader_3d(tmp_path):
    from arco_amd import pretrain_3D as P3
    base = R.write_volume_dataset(tmp_path)
    args = P3.build_parser().parse_args(["--root_path", str(base)])
    args.patch_size = [32, 32, 32]
    _assert_bank_loader_equals_host_loader(P3.build_loader(args), 4)


def _replay(shape, color):
    """The draws of one transform call, replayed: (jitter params or None, sigma or None)."""
    from arco_amd.dataloaders.dataset_withAug import _jitter_params
    params = sigma = None
    if not (np.random.uniform(low=0, high=1, size=1) > 0.5):
        params = [_jitter_params(color) for _ in range(S.n_planes(shape))]
    if not (np.random.uniform(low=0, high=1, size=1) > 0.5):
        sigma = random.uniform(0.15, 1.15)
    return params, sigma


def test_device_transform_2d_equals_the_restatement_chain():
    """The semantics of test_transform_student_semantics, exactly: the jitter edits the shared tensor in place, the noise returns a
    new [B, H, W] tensor = blur(q8(jitter restatement)) / 255."""
    from arco_amd import pretrain_2D as P
    from arco_amd.dataloaders import stage1_aug as A
    shape = (3, 1, 32, 40)
    x = np.random.RandomState(0).uniform(size=shape).astype(np.float32)
    ts = A.device_transform(P.make_transform_student())
    hits = set()
    for seed in range(12):
        S.seed_all(seed)
        batch = {'image': torch.from_numpy(x.copy()).cuda(), 'label': torch.zeros(3, 32, 40).cuda()}
        tensor = batch['image']
        student, teacher = P.student_teacher_batches(batch, 2, ts)
        state = S.rng_states()
        S.seed_all(seed)
        params, sigma = _replay(shape, (0.2, 0.2, 0.2, 0.1))
        S.assert_same_states(state, S.rng_states())
        exp = S.jitter_image(x, params) if params else x
        assert student is batch and batch['image'] is tensor and _same_bits(tensor, exp)
        if sigma is not None:
            assert teacher is not batch and teacher['image'] is not tensor and teacher['image'].shape == (3, 32, 40)
            assert _same_bits(teacher['image'], S.blur_image(exp, sigma).astype(np.float32) / np.float32(255.0))
        else:
            assert teacher['image'] is tensor
        hits.add((params is not None, sigma is not None))
    assert len(hits) == 4


def test_device_transform_3d_equals_the_restatement_chain():
    """The semantics of test_transform_student_3d_semantics, exactly: both ops edit the volume in place, slice by slice along the
    last axis; the noise stores the byte values 0 .. 255."""
    from arco_amd import pretrain_3D as P3
    from arco_amd.dataloaders import stage1_aug as A
    shape = (2, 1, 24, 20, 5)
    x = np.random.RandomState(1).uniform(size=shape).astype(np.float32)
    ts = A.device_transform(P3.make_transform_student())
    hits = set()
    for seed in range(12):
        S.seed_all(seed)
        batch = {'image': torch.from_numpy(x.copy()).cuda(), 'label': torch.zeros(2, 24, 20, 5).cuda()}
        tensor = batch['image']
        student, teacher = P3.student_teacher_batches(batch, 1, ts)
        state = S.rng_states()
        assert student['image'] is tensor and teacher is batch and batch['image'] is tensor
        S.seed_all(seed)
        params, sigma = _replay(shape, (0.02, 0.02, 0.02, 0.01))
        S.assert_same_states(state, S.rng_states())
        exp = S.jitter_image(x, params) if params else x.copy()
        if sigma is not None:
            blurred = S.blur_image(exp, sigma)
            exp = exp.copy()
            for v, w in zip(S.plane_views(exp), blurred):
                v[...] = w
        assert _same_bits(tensor, exp)
        hits.add((params is not None, sigma is not None))
    assert len(hits) == 4


def _train_recording(mod, cls, argv, patch, seed, snap, monkeypatch, head_patch=None):
    """mod.train on `argv`; what every step was handed (on the CPU), the generators' states at the end, the checkpoints."""
    from arco_amd import ops
    args = mod.build_parser().parse_args(argv + ["--snapshot_path", str(snap)])
    args.patch_size = patch
    if head_patch:
        args.head_patch = head_patch
    seen, step = [], cls.step

    def recording(self, s_img, s_lab, t_img):
        seen.append((s_img.cpu(), s_lab.cpu().long(), t_img.cpu()))
        return step(self, s_img, s_lab, t_img)

    monkeypatch.setattr(cls, "step", recording)
    os.makedirs(snap)
    S.seed_all(seed)
    ops.reseed_dropout(seed)        # the dropout masks' private generator is seeded once per process: both runs start it alike
    assert mod.train(args, str(snap)) == "Training Finished!"
    monkeypatch.setattr(cls, "step", step)
    states = S.rng_states()
    for tag in ("", "_ema"):
        sd = torch.load(os.path.join(snap, f"iter_4{tag}.pth"), map_location="cpu")
        assert all(torch.isfinite(v.float()).all() for v in sd.values())
    return seen, states


def _assert_trainer_routes_agree(mod, cls, argv, patch, seed, tmp_path, monkeypatch, combination, head_patch=None):
    """4 iterations with --gpu_ingest 0, then 1.  --combinations 0 (no student transform): images and labels bit-equal.  The
    trainer's own combination: labels equal, the three generators in equal states (the images then differ by the jitter's mean:
    torch's fp32 sum against the kernel's float64 one)."""
    extra = ["--combinations", "0"] if combination == 0 else []
    runs = [_train_recording(mod, cls, argv + extra + ["--gpu_ingest", g], patch, seed, tmp_path / f"snap{combination}{g}", monkeypatch,
                             head_patch) for g in "01"]
    (seen0, states0), (seen1, states1) = runs
    assert len(seen0) == len(seen1) == 4
    for a, b in zip(seen0, seen1):
        assert torch.equal(a[1], b[1])
        if combination == 0:
            assert _same_bits(b[0], a[0]) and _same_bits(b[2], a[2])
    S.assert_same_states(states0, states1)


@pytest.mark.parametrize("combination", [0, "default"])
def test_pretrain_2d_routes_agree(tmp_path, monkeypatch, combination):
    """On the slice dataset at patch 64 x 64.  RandomGenerator's crop branch is wired to 256 x 256 and cannot be collated at another
    patch on either route; seed 13 draws none in these 4 iterations."""
    from arco_amd import pretrain_2D as P
    root = R.write_slice_dataset(tmp_path)
    argv = ["--root_path", str(root), "--exp", "ACDC/ingest_test", "--labeled_num", "1", "--max_iterations", "4", "--save_every", "4",
            "--batch_size", "4", "--labeled_bs", "2", "--K", "12", "--cut_size", "16", "--output_pooling_size", "4",
            "--latent_feature_size", "32"]
    _assert_trainer_routes_agree(P, P.PretrainStep2D, argv, [64, 64], 13, tmp_path, monkeypatch, combination)


@pytest.mark.parametrize("combination", [0, "default"])
def test_pretrain_3d_routes_agree(tmp_path, monkeypatch, combination):
    from arco_amd import pretrain_3D as P3
    import arco_amd.model_3D as M3
    base = R.write_volume_dataset(tmp_path)
    argv = ["--root_path", str(base), "--max_iterations", "4", "--save_every", "4", "--K", "4", "--output_pooling_size", "2",
            "--latent_feature_size", "16"]
    real = M3.ISD_3d.__init__

    def small_queue(self, *a, **k):            # 27 patches instead of the hard-wired 700, as test_pretrain3d_trainer_runs
        real(self, *a, **k)
        self.queue_mask = torch.nn.functional.normalize(torch.randn(self.K, 27, self.num_classes * 8), dim=-1)

    monkeypatch.setattr(M3.ISD_3d, "__init__", small_queue)
    _assert_trainer_routes_agree(P3, P3.PretrainStep3D, argv, [32, 32, 32], 5, tmp_path, monkeypatch, combination, head_patch=16)


def test_synthetic_route_uses_the_device_transform(tmp_path, monkeypatch):
    """--gpu_ingest 1 with --synthetic 1: no bank, the device transform alone."""
    from arco_amd import pretrain_2D as P
    from arco_amd.dataloaders import stage1_aug as A
    made = []
    real = A.device_transform
    monkeypatch.setattr(A, "device_transform", lambda t: made.append(real(t)) or made[-1])
    argv = ["--synthetic", "1", "--max_iterations", "2", "--save_every", "2", "--batch_size", "4", "--labeled_bs", "2", "--K", "12",
            "--cut_size", "16", "--output_pooling_size", "4", "--latent_feature_size", "32", "--snapshot_path", str(tmp_path), "--gpu_ingest", "1"]
    args = P.build_parser().parse_args(argv)
    args.patch_size = [64, 64]
    S.seed_all(args.seed)
    assert P.train(args, str(tmp_path)) == "Training Finished!"
    assert len(made) == 1 and [type(t) for t in made[0].transforms] == [A.GrayJitter, A.Noise]
