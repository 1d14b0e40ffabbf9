"""--gpu_ingest 1 of the pre-trainers without a device: the numpy restatements of csrc/stage1_aug.hip (tests/stage1_aug_refs.py) against
what they restate - `jitter_gray_` on CPU tensors, Pillow's GaussianBlur - and the loader and transform twins against the host
classes' consumption of the three generators.  tests/test_pretrain_ingest_gpu.py holds the kernels to the restatements."""
import numpy as np
import pytest
import torch

import ingest_refs as R
import stage1_aug_refs as S


def _torch_jitter(plane, order, fb, fc):
    from arco_amd.dataloaders.dataset_withAug import jitter_gray_
    return jitter_gray_(torch.from_numpy(plane.copy())[None], order, (fb, fc, 1.0, 0.0))[0].numpy()


@pytest.mark.parametrize("shape", [(40, 36), (33, 47), (24, 20)])
def test_jitter_restatement_equals_jitter_gray(shape):
    """Bit-equal whenever fc == 1 (the mean drops out); elsewhere within 2^-23 per pixel: torch's fp32 mean is within one fp32 ulp of
    a value below 1 (2^-24) of the restatement's, and two roundings follow it (the product with 1 - fc, the sum)."""
    rs = np.random.RandomState(sum(shape))
    for k, order in enumerate(S.ORDERS):
        plane = S.jitter_input(shape, 100 + k)
        assert plane.min() < 0 and plane.max() > 1
        fb, fc = (float(np.float32(v)) for v in rs.uniform(0.8, 1.2, size=2))
        for fb_, fc_ in ((fb, fc), (1.0, fc), (fb, 1.0)):
            want, got = _torch_jitter(plane, order, fb_, fc_), S.jitter_plane(plane, order, fb_, fc_)
            if fc_ == 1.0:
                assert np.array_equal(want, got)
            else:
                assert np.abs(want.astype(np.float64) - got.astype(np.float64)).max() <= 2.0 ** -23


def test_jitter_restatement_is_bit_equal_given_the_same_mean():
    """With torch's own mean handed in, the restatement's arithmetic is jitter_gray_'s bit for bit."""
    torch_mean = lambda x: np.float32(torch.from_numpy(np.ascontiguousarray(x)).mean().item())
    for k, order in enumerate(S.ORDERS):
        plane = S.jitter_input((40, 36), 200 + k)
        got = S.jitter_plane(plane, order, 0.9, 1.1, mean_fn=torch_mean)
        assert np.array_equal(_torch_jitter(plane, order, float(np.float32(0.9)), float(np.float32(1.1))), got)


@pytest.mark.parametrize("shape", S.SHAPES_2D + S.SHAPES_3D)
@pytest.mark.parametrize("kind", sorted(S.FACTOR_SETS))
def test_device_cases_have_order_free_means(shape, kind):
    """Every plane of the device tests' inputs satisfies plane_mean's condition (asserted inside it), and their launches deal all 24
    orders."""
    orders = set()
    for start in S.case_starts(shape):
        x, params, want = S.jitter_case(shape, kind, start)
        orders |= {tuple(o) for o, _ in params}
        assert want.shape == x.shape and (want != x).any() and want.min() >= 0 and want.max() <= 1
    assert len(orders) == 24


@pytest.mark.parametrize("sigma", S.SIGMAS)
def test_blur_restatement_equals_pillow(sigma):
    from PIL import Image, ImageFilter
    rs = np.random.RandomState(int(sigma * 100))
    for shape in S.BLUR_PLANES:
        plane = (rs.rand(*shape) * 1.3 - 0.1).astype(np.float32)
        want = np.asarray(Image.fromarray(S.orc.q8(plane), mode="L").filter(ImageFilter.GaussianBlur(radius=sigma)))
        assert np.array_equal(S.blur_planes(plane[None], sigma)[0], want)


def _loop(loader, n):
    """The trainer's loop over n iterations: a fresh iterator per epoch; the drawn case indices."""
    seen = []
    while len(seen) < n:
        for batch in loader:
            seen.append(batch['idx'].tolist())
            if len(seen) == n:
                break
    return seen


def _host_and_twin(host, monkeypatch, seed):
    from arco_amd import _lib
    from arco_amd.dataloaders import gpu_ingest as G
    S.seed_all(seed)
    h_idx, h_state = _loop(host, 6), S.rng_states()
    monkeypatch.setattr(_lib, "require_gpu", lambda *t: None)          # the bank on the host: only its descriptor loader is run
    twin = G.bank_loader(host, "cpu")
    assert isinstance(twin, G.BankLoader) and twin.labels and twin.loader.batch_sampler is host.batch_sampler
    assert twin.bank.n_cases == len(host.dataset) and len(twin) == len(host) < 6          # 6 iterations cross an epoch boundary
    S.seed_all(seed)
    t_idx, t_state = _loop(twin.loader, 6), S.rng_states()
    assert t_idx == h_idx
    S.assert_same_states(h_state, t_state)
    return twin


def test_bank_loader_draws_like_the_host_loader_2d(tmp_path, monkeypatch):
    from arco_amd import pretrain_2D as P
    root = R.write_slice_dataset(tmp_path)
    args = P.build_parser().parse_args(["--root_path", str(root), "--exp", "ACDC/ingest_test", "--labeled_num", "1", "--batch_size", "12",
                                        "--labeled_bs", "6"])           # the default 256 x 256 patch: the crop branch is wired to it
    twin = _host_and_twin(P.build_loader(args), monkeypatch, 7)
    assert twin.patch_size == (256, 256) and twin.bank.rank == 2


def test_bank_loader_draws_like_the_host_loader_3d(tmp_path, monkeypatch):
    from arco_amd import pretrain_3D as P3
    base = R.write_volume_dataset(tmp_path)
    args = P3.build_parser().parse_args(["--root_path", str(base)])
    args.patch_size = [32, 32, 32]
    twin = _host_and_twin(P3.build_loader(args), monkeypatch, 8)
    assert twin.patch_size == (32, 32, 32) and twin.bank.rank == 3


@pytest.mark.parametrize("rank", [2, 3])
def test_transform_twins_draw_like_the_host_classes(rank, monkeypatch):
    """Launches stubbed out (the host classes' blur too, which has no CPU route): over a dozen seeds that reach all four (jitter,
    noise) outcomes, both leave python's, numpy's and torch's generators in the same state, and the twins keep the aliasing."""
    from arco_amd import augment, pretrain_2D as P, pretrain_3D as P3
    from arco_amd.dataloaders import stage1_aug as A
    host = (P if rank == 2 else P3).make_transform_student()
    twin = A.device_transform(host)
    shape = (3, 1, 8, 10) if rank == 2 else (2, 1, 8, 6, 5)
    calls = []
    monkeypatch.setattr(augment, "jitter_blur", lambda data, params: torch.zeros_like(data))
    monkeypatch.setattr(A, "gray_jitter_planes", lambda image, recs: calls.append(("jitter", len(recs))) or image)
    monkeypatch.setattr(A, "blur_planes", lambda image, sigma, inplace: calls.append(("blur", inplace)) or
                        (image if inplace else torch.zeros(image.shape[0], *image.shape[2:4])))
    hits = set()
    for seed in range(12):
        S.seed_all(seed)
        host({'image': torch.rand(shape), 'label': torch.zeros(shape[0])})
        h_state = S.rng_states()
        S.seed_all(seed)
        del calls[:]
        sample = {'image': torch.rand(shape), 'label': torch.zeros(shape[0])}
        out = twin(sample)
        S.assert_same_states(h_state, S.rng_states())
        jit, blur = any(c[0] == "jitter" for c in calls), any(c[0] == "blur" for c in calls)
        if jit:
            assert calls[0] == ("jitter", shape[0] * (shape[4] if rank == 3 else 1))
        if blur:
            assert calls[-1] == ("blur", rank == 3)
        if not (jit or blur):
            assert out is sample
        elif blur and rank == 2:
            assert out is not sample and out['image'] is not sample['image'] and out['image'].shape == (3, 8, 10)
        else:
            assert out is not sample and out['image'] is sample['image']
        hits.add((jit, blur))
    assert len(hits) == 4


def test_jitter_records_match_the_kernels_layout():
    from arco_amd import _lib
    from arco_amd.dataloaders import stage1_aug as A
    recs = A.jitter_records([([3, 0, 1, 2], [0.9, 1.1, 1.0, 0.0]), ([1, 2, 3, 0], [1.2, 0.8, 1.0, 0.0])])
    assert recs.itemsize == _lib.query("arco_jit_record_bytes") == 24
    raw = np.frombuffer(recs.tobytes(), dtype=np.int32).reshape(2, 6)
    assert raw[:, :4].tolist() == [[3, 0, 1, 2], [1, 2, 3, 0]]
    assert raw[:, 4:].view(np.float32).tolist() == [[np.float32(0.9), np.float32(1.1)], [np.float32(1.2), np.float32(0.8)]]


def test_pretrainers_have_the_flag_and_refuse_a_transform_without_a_twin():
    from arco_amd import pretrain_2D as P, pretrain_3D as P3
    from arco_amd.dataloaders import Compose, stage1_aug as A
    from arco_amd.dataloaders.la_heart import ToTensor
    for mod in (P, P3):
        assert mod.build_parser().parse_args([]).gpu_ingest == 0
        assert mod.build_parser().parse_args(["--gpu_ingest", "1"]).gpu_ingest == 1
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--gpu_ingest", "2"])
    with pytest.raises(ValueError, match="no device twin"):
        A.device_transform(Compose([ToTensor()]))
