"""GPU ingest, the parts that need no GPU: the numpy reference of the kernels' coordinate rule (tests/ingest_refs.py) against the real
host transforms, the descriptor datasets' generator consumption against the host datasets', and the bank's refusals."""
import os
import random

import numpy as np
import pytest
import torch

import fixture_inputs as fx
import ingest_refs as R
from arco_amd.dataloaders import gpu_ingest as G


def _host_slice(src, patch, op, draws, monkeypatch):
    from arco_amd.dataloaders.dataset import RandomGenerator
    img, lab = R.slice_sources()[src]
    with monkeypatch.context() as m:
        R.slice_draws(op, draws).install(m)
        out = RandomGenerator(list(patch))({'image': img, 'label': lab})
    return out['image'].numpy(), out['label'].numpy()


@pytest.mark.parametrize("patch", R.SLICE_PATCHES, ids=lambda p: f"patch{p[0]}")
def test_reference_equals_random_generator(patch, monkeypatch):
    """Every branch of RandomGenerator - no op, the 8 (k, axis), all 40 angles, the crop at 256 - on the four sources: the row the
    descriptor dataset draws, put through apply_slice_descriptor, is the host sample."""
    twin = G.SliceDescriptors(R.SLICE_SOURCES, patch)
    for c in R.slice_cases(patch):
        h_img, h_lab = _host_slice(c["src"], patch, c["op"], c["draws"], monkeypatch)
        with monkeypatch.context() as m:
            R.slice_draws(c["op"], c["draws"]).install(m)
            item = twin[c["src"]]
        d = item['desc'].numpy()
        assert item['idx'] == c["src"] and d.dtype == np.float64 and d[1] == c["op"]
        np.testing.assert_array_equal(d, G.slice_row(c["src"], R.SLICE_SOURCES[c["src"]], patch, c["op"], **c["draws"])[0])
        img, lab = R.apply_slice_descriptor(*R.slice_sources()[c["src"]], d, patch)
        assert h_img.dtype == np.float32 and h_img.shape == (1, *patch), c
        assert np.array_equal(img[None], h_img), c
        assert np.array_equal(lab, h_lab.astype(np.int64)), c


def test_zoom_zeroes_the_last_column(monkeypatch):
    """The (5, 256) source at patch 32: along the columns (256 -> 32) the coordinate of the last index lands an ulp above n_in - 1,
    and scipy writes the constant there - a whole zero column that the reference must reproduce; along the rows it does not."""
    src, patch = R.SLICE_SOURCES.index((5, 256)), (32, 32)
    d, out = G.slice_row(src, (5, 256), patch, 0)
    assert 31 * d[4] <= 4 and 31 * d[5] > 255                      # the case still covers the rule
    h_img, _ = _host_slice(src, patch, 0, {}, monkeypatch)
    img, _ = R.apply_slice_descriptor(*R.slice_sources()[src], d, out)
    assert np.all(img[:, -1] == 0) and np.all(img[:, :-1] != 0)
    assert np.array_equal(img[None], h_img)


def test_reference_equals_random_crop_at_other_sizes():
    """random_crop returns 256 x 256 whatever it is given; zoomed shapes above, below and astride 256."""
    from arco_amd.dataloaders.dataset import random_crop
    from scipy.ndimage import zoom
    for c in R.crop_cases():
        img, lab = R.slice_sources()[c["src"]]
        x, y = img.shape
        f = (c["patch"][0] / x, c["patch"][1] / y)
        h_img, h_lab = random_crop(zoom(img, f, order=0), zoom(lab, f, order=0))
        d, out = G.slice_row(c["src"], img.shape, c["patch"], 3)
        assert out == h_img.shape == (256, 256), c
        r_img, r_lab = R.apply_slice_descriptor(img, lab, d, out)
        assert np.array_equal(r_img, h_img) and np.array_equal(r_lab, h_lab.astype(np.int64)), c


def test_uncollatable_samples_raise(monkeypatch):
    """Where the host path yields a sample no batch can hold, the descriptor dataset raises instead of inventing a behaviour."""
    with monkeypatch.context() as m:                               # the 256-hard-wired crop at patch 32
        R.slice_draws(3, {}).install(m)
        with pytest.raises(RuntimeError):
            G.SliceDescriptors(R.SLICE_SOURCES, (32, 32))[0]
    with monkeypatch.context() as m:                               # an odd k on a non-square patch
        R.slice_draws(1, dict(k=1, axis=0)).install(m)
        with pytest.raises(RuntimeError):
            G.SliceDescriptors(R.SLICE_SOURCES, (32, 48))[0]
    with monkeypatch.context() as m:                               # ... an even k is fine
        R.slice_draws(1, dict(k=2, axis=0)).install(m)
        assert G.SliceDescriptors(R.SLICE_SOURCES, (32, 48))[0]['desc'][6] == 2


def test_reference_equals_volume_transforms(monkeypatch):
    """RandomRotFlip -> RandomCrop -> ToTensor on both sources (the second is padded), all 8 (k, axis), windows at both ends."""
    from arco_amd.dataloaders import Compose
    from arco_amd.dataloaders.la_heart import RandomCrop, RandomRotFlip, ToTensor
    tf = Compose([RandomRotFlip(), RandomCrop(R.VOLUME_PATCH), ToTensor()])
    twin = G.VolumeDescriptors(R.VOLUME_SOURCES, R.VOLUME_PATCH)
    padded = set()
    for c in R.volume_cases():
        vol, lab = R.volume_sources()[c["src"]]
        ints = [c["k"], c["axis"], *c["start"]]
        with monkeypatch.context() as m:
            R.ForcedDraws(ints=ints).install(m)
            host = tf({'image': vol, 'label': lab})
        with monkeypatch.context() as m:
            R.ForcedDraws(ints=ints).install(m)
            item = twin[c["src"]]
        d = item['desc'].numpy()
        assert d.dtype == np.int64 and item['idx'] == c["src"]
        padded.add(any(c["pads"]))
        img, lb = R.apply_volume_descriptor(vol, lab, d, R.VOLUME_PATCH)
        assert host['image'].dtype == torch.float32 and host['label'].dtype == torch.int64
        assert np.array_equal(img[None], host['image'].numpy()), c
        assert np.array_equal(lb, host['label'].numpy()), c
    assert padded == {True, False}                                 # both RandomCrop paths were taken


def _seed(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def _states():
    return random.getstate(), np.random.get_state(), torch.get_rng_state()


def _same_states(a, b):
    assert a[0] == b[0]
    assert a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]
    assert torch.equal(a[2], b[2])


def _epochs(loaders, n_epochs):
    """The trainer's loop: fresh iterators per epoch, one labeled and one unlabeled batch per iteration; the drawn case indices."""
    seen = []
    for _ in range(n_epochs):
        l_iter, u_iter = iter(loaders[0]), iter(loaders[1])
        for _ in range(len(loaders[1])):
            seen.append((next(l_iter)['idx'].tolist(), next(u_iter)['idx'].tolist()))
    return seen


def _twin_loaders(host_loaders, batch_size):
    """stepper.paired_loaders around the descriptor twins of the host loaders' datasets (no device: shapes read from the files)."""
    from arco_amd import stepper
    twins = []
    for ld in host_loaders:
        ds = G._base(ld.dataset)
        tf, ds.transform = ds.transform, None
        shapes = [ds[i]['image'].shape for i in range(len(ds))]
        ds.transform = tf
        ts = tf.transforms
        twins.append(G.SliceDescriptors(shapes, ts[0].output_size) if len(ts) == 1 else G.VolumeDescriptors(shapes, ts[1].output_size))
    return stepper.paired_loaders(*twins, batch_size)


def test_descriptor_loaders_consume_the_generators_like_the_host_loaders_2d(tmp_path):
    from arco_amd import train_arco_2d as T
    root = R.write_slice_dataset(tmp_path)
    args = T.build_parser().parse_args(["--synthetic", "0", "--root_path", str(root), "--exp", "ACDC/ingest_test", "--labeled_num", "1",
                                        "--batch_size", "2"])          # the default 256 x 256 patch: the crop branch is wired to it
    host = T.build_loaders(args)
    _seed(5)
    h_idx, h_state = _epochs(host, 3), _states()
    twin = _twin_loaders(host, 2)
    assert len(twin[0].dataset) == len(host[0].dataset) and len(twin[1]) == len(host[1])
    _seed(5)
    t_idx, t_state = _epochs(twin, 3), _states()
    assert t_idx == h_idx and len(h_idx) == 3 * len(host[1])
    _same_states(h_state, t_state)


def test_descriptor_loaders_consume_the_generators_like_the_host_loaders_3d(tmp_path):
    from arco_amd import train_arco_3d as T3
    base = R.write_volume_dataset(tmp_path)
    args = T3.build_parser().parse_args(["--synthetic", "0", "--root_path", str(base), "--exp", "LA/ingest_test", "--labeled_num", "2",
                                         "--batch_size", "1", "--num_classes", "2"])
    args.patch_size = [32, 32, 32]
    host = T3.build_loaders(args)
    _seed(6)
    h_idx, h_state = _epochs(host, 3), _states()
    twin = _twin_loaders(host, 1)
    _seed(6)
    t_idx, t_state = _epochs(twin, 3), _states()
    assert t_idx == h_idx and len(h_idx) == 3 * len(host[1])
    _same_states(h_state, t_state)


def test_bank_refuses_labels_outside_uint8():
    img, lab = fx.ingest_slice(1, (8, 8))
    for bad in (lab.astype(np.int64) + 300, lab.astype(np.int64) - 1):
        with pytest.raises(ValueError, match="0 .. 255"):
            G.GpuBank([img], [bad], "cpu")


def test_bank_refuses_mixed_ranks():
    img, lab = fx.ingest_slice(1, (8, 8))
    vol, vlab = fx.ingest_volume(1, (8, 8, 8))
    with pytest.raises(ValueError, match="all be 2-D slices or all be 3-D"):
        G.GpuBank([img, vol], [lab, vlab], "cpu")


def test_bank_has_no_twin_for_another_transform():
    from arco_amd.dataloaders import Compose
    from arco_amd.dataloaders.la_heart import RandomCrop, ToTensor
    bank = G.GpuBank.__new__(G.GpuBank)
    bank.rank, bank.shapes = 3, [(8, 8, 8)]
    with pytest.raises(ValueError, match="no descriptor twin"):
        bank.descriptors(Compose([RandomCrop((4, 4, 4)), ToTensor()]))


def test_trainers_have_the_flag():
    from arco_amd import train_arco_2d as T, train_arco_3d as T3
    for mod in (T, T3):
        assert mod.build_parser().parse_args([]).gpu_ingest == 0
        assert mod.build_parser().parse_args(["--gpu_ingest", "1"]).gpu_ingest == 1
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--gpu_ingest", "2"])
