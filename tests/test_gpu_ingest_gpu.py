"""GPU ingest on the device (-m gpu): the two kernels of csrc/ingest.hip against the numpy reference of tests/ingest_refs.py (which
tests/test_gpu_ingest_cpu.py holds to the host transforms), the bank loaders against the host loaders, and both trainers with
--gpu_ingest 1 against --gpu_ingest 0 - everything bit for bit."""
import os
import random

import numpy as np
import pytest
import torch

import ingest_refs as R

pytestmark = pytest.mark.gpu


def _seed(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def _slice_bank():
    from arco_amd.dataloaders.gpu_ingest import GpuBank
    src = R.slice_sources()
    return GpuBank([s[0] for s in src], [s[1] for s in src], "cuda:0")


@pytest.mark.parametrize("kind", [32, 256, "crop"])
def test_slices_kernel_equals_reference(kind):
    """One launch per kind: 32 / 256 = no op, the 8 (k, axis) and the 40 angles on the four sources (256 adds the crop: all four
    branches in one launch), 'crop' = the crop on zoomed shapes above, below and astride 256.  The (5, 256) source at 32 carries the
    zoom's zeroed last column."""
    bank = _slice_bank()
    rows, ref_img, ref_lab = R.slice_batch(kind)
    if kind != "crop":
        assert set(rows[:, 1]) == ({0, 1, 2, 3} if kind == 256 else {0, 1, 2})
    H = W = 256 if kind == "crop" else kind
    img, lab = bank.slices(torch.from_numpy(rows.copy()), (H, W))
    assert img.dtype == torch.float32 and tuple(img.shape) == (len(rows), 1, H, W)
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (len(rows), H, W)
    assert torch.equal(img.cpu(), torch.from_numpy(ref_img.copy()))
    assert torch.equal(lab.cpu(), torch.from_numpy(ref_lab.copy()))
    img2, none = bank.slices(torch.from_numpy(rows.copy()), (H, W), labels=False)      # the unlabeled stream: no label store
    assert none is None and torch.equal(img2, img)


def test_volumes_kernel_equals_reference():
    """All 8 (k, axis) on a source that RandomCrop pads and one it does not, windows at both ends and inside, one launch."""
    from arco_amd.dataloaders.gpu_ingest import GpuBank
    src = R.volume_sources()
    bank = GpuBank([s[0] for s in src], [s[1] for s in src], "cuda:0")
    rows, ref_img, ref_lab = R.volume_batch()
    assert {any(c["pads"]) for c in R.volume_cases()} == {True, False}
    img, lab = bank.volumes(torch.from_numpy(rows.copy()), R.VOLUME_PATCH)
    assert img.dtype == torch.float32 and tuple(img.shape) == (len(rows), 1, *R.VOLUME_PATCH)
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (len(rows), *R.VOLUME_PATCH)
    assert torch.equal(img.cpu(), torch.from_numpy(ref_img.copy()))
    assert torch.equal(lab.cpu(), torch.from_numpy(ref_lab.copy()))


def test_entry_points_refuse_bad_arguments():
    bank = _slice_bank()
    rows = torch.from_numpy(R.slice_batch(32)[0][:2].copy())
    with pytest.raises(RuntimeError, match="arco_ingest_slices"):
        bank.slices(rows, (32, 30))                               # the fastest axis is written four at a time
    bad = rows.clone(); bad[0, 0] = 99
    with pytest.raises(ValueError, match="outside the bank"):
        bank.slices(bad, (32, 32))
    with pytest.raises(ValueError):
        bank.volumes(rows.long(), (32, 32, 32))                   # a bank of slices


def _batches(loaders, n):
    """The trainer's loop over `n` iterations: fresh iterators per epoch; (labeled, unlabeled) batches, image / label on the CPU."""
    out, l_iter, u_iter = [], None, None
    for it in range(n):
        if it % len(loaders[1]) == 0:
            l_iter, u_iter = iter(loaders[0]), iter(loaders[1])
        out.append(tuple({k: b[k].cpu() for k in ("image", "label", "idx")} for b in (next(l_iter), next(u_iter))))
    return out


def _assert_same_batches(host, dev):
    assert len(host) == len(dev) == 6
    for hb, db in zip(host, dev):
        for h, d in zip(hb, db):
            assert torch.equal(h["idx"], d["idx"])
            assert d["image"].dtype == torch.float32 and torch.equal(h["image"], d["image"])
            assert d["label"].dtype == torch.int64 and torch.equal(h["label"].long(), d["label"])


def test_bank_loaders_equal_host_loaders_2d(tmp_path):
    from arco_amd import stepper, train_arco_2d as T
    from arco_amd.dataloaders import gpu_ingest as G
    root = R.write_slice_dataset(tmp_path)
    args = T.build_parser().parse_args(["--synthetic", "0", "--root_path", str(root), "--exp", "ACDC/ingest_test", "--labeled_num", "1",
                                        "--batch_size", "2"])
    host = T.build_loaders(args)
    _seed(3)
    h = _batches(host, 6)
    dev = G.bank_loaders(host, stepper.paired_loaders, 2, "cuda:0", unlabeled_labels=True)
    assert dev[0].bank.n_cases == 23 and dev[1].bank.n_cases == 7 and dev[0].bank.nbytes == 23 * 40 * 36 * 5 + 23 * 32
    _seed(3)
    _assert_same_batches(h, _batches(dev, 6))


def test_bank_loaders_equal_host_loaders_3d(tmp_path):
    from arco_amd import stepper, train_arco_3d as T3
    from arco_amd.dataloaders import gpu_ingest as G
    base = R.write_volume_dataset(tmp_path)
    args = T3.build_parser().parse_args(["--synthetic", "0", "--root_path", str(base), "--exp", "LA/ingest_test", "--labeled_num", "2",
                                         "--batch_size", "1", "--num_classes", "2"])
    args.patch_size = [32, 32, 32]
    host = T3.build_loaders(args)
    _seed(4)
    h = _batches(host, 6)
    dev = G.bank_loaders(host, stepper.paired_loaders, 1, "cuda:0", unlabeled_labels=True)
    _seed(4)
    _assert_same_batches(h, _batches(dev, 6))


def _train_recording(mod, cls, argv, patch, seed, tmp_path, monkeypatch, tag):
    """mod.train on `argv`; what every step was handed, on the CPU."""
    from arco_amd import ops
    args = mod.build_parser().parse_args(argv)
    if patch is not None:
        args.patch_size = patch
    seen, step = [], cls.step

    def recording(self, l_img, l_lab, u_img, *a, **kw):
        seen.append((l_img.cpu(), l_lab.cpu(), u_img.cpu()))
        return step(self, l_img, l_lab, u_img, *a, **kw)

    monkeypatch.setattr(cls, "step", recording)
    snap = tmp_path / tag
    os.makedirs(snap)
    _seed(seed)
    ops.reseed_dropout(seed)        # the dropout masks' private generator is seeded once per process: both runs start it alike
    assert mod.train(args, str(snap)) == "Training Finished!"
    monkeypatch.setattr(cls, "step", step)
    return seen


def _assert_same_inputs(a, b, n):
    assert len(a) == len(b) == n
    for x, y in zip(a, b):
        for t, u in zip(x, y):
            assert t.dtype == u.dtype and torch.equal(t, u)


def test_2d_trainer_sees_the_same_batches(tmp_path, monkeypatch):
    from arco_amd import train_arco_2d as T
    root = R.write_slice_dataset(tmp_path)
    monkeypatch.chdir(tmp_path)
    argv = ["--synthetic", "0", "--root_path", str(root), "--exp", "ACDC/ingest_test", "--labeled_num", "1", "--batch_size", "2",
            "--queue_size", "256", "--num_queries", "32", "--num_negatives", "16", "--max_iterations", "4"]
    runs = [_train_recording(T, T.ArcoStep2D, argv + ["--gpu_ingest", g], None, 1, tmp_path, monkeypatch, "snap" + g) for g in "01"]
    _assert_same_inputs(*runs, 4)


def test_3d_trainer_sees_the_same_batches(tmp_path, monkeypatch):
    from arco_amd import train_arco_3d as T3
    base = R.write_volume_dataset(tmp_path)
    monkeypatch.chdir(tmp_path)
    argv = ["--synthetic", "0", "--root_path", str(base), "--exp", "LA/ingest_test", "--labeled_num", "2", "--batch_size", "1",
            "--num_classes", "2", "--queue_size", "256", "--num_queries", "32", "--num_negatives", "16", "--max_iterations", "4",
            "--eqv_pass", "0"]
    runs = [_train_recording(T3, T3.ArcoStep3D, argv + ["--gpu_ingest", g], [32, 32, 32], 2, tmp_path, monkeypatch, "snap3" + g)
            for g in "01"]
    _assert_same_inputs(*runs, 4)
