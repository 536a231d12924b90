"""CPU checks of the device dataset's DEFINITION (include/iaf_hip.h, iaf_data_*): the numpy statement of it
(tests/data_reference.py) is a bijection at the sizes where the Feistel domain changes, spreads images over slots evenly (three
chi-square figures over 4000 epochs), hands disjoint rows to the ranks, and iaf_amd.DeviceDataset / TrainStep(data=) refuse bad
arguments on the host (no device)."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import data_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HostModel(object):
    """a host stand-in with CVAE1's training interface (as in tests/test_train_step_api.py): obj = 0.5 x[0] |p|^2 + x[1]"""

    def __init__(self):
        self.params = {"a/V": torch.arange(12.0).reshape(3, 4) / 7, "b/odd": torch.ones(7)}

    def completion_order(self):
        return list(self.params)

    def load(self, params):
        self.params = params

    def set_grad_buckets(self, n_buckets=1):
        return [list(self.params)]

    def prepare_weights(self):
        pass

    def fb_begin(self, x, noise, grads=None):
        self._fb = (x, noise, grads)
        return {"obj": (0.5 * x[0] * sum((p * p).sum() for p in self.params.values()) + x[1]).reshape(1)}

    def fb_segment(self, i):
        x, noise, grads = self._fb
        for k, p in self.params.items():
            grads[k].copy_(x[0] * p + (noise[0] if k == "b/odd" else 0))


SIZES = [1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 1000, 10000, 50000]


def test_half_width():
    assert [D.half_width(n) for n in (2, 3, 4, 5, 16, 17, 64, 65, 256, 257, 1 << 31, (1 << 32) - 1)] == \
        [1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 16, 16]


@pytest.mark.parametrize("n", SIZES)
def test_permutation_is_a_bijection(n):
    worst = 0
    for seed, epoch in ((99, 0), (99, 1), (0, (1 << 32) + 3), ((1 << 64) - 1, 7)):
        count = np.zeros(n, np.int64)
        p = D.perm(np.arange(n), n, seed, epoch, count=count)
        assert p.min() >= 0 and p.max() < n and np.array_equal(np.sort(p), np.arange(n)), (n, seed, epoch)
        worst = max(worst, int(count.max()))
    print("n = %d: most passes %d" % (n, worst))


def test_epochs_and_seeds_share_almost_no_slot():
    n = 50000
    a, b, c = D.epoch_order(n, 99, 0), D.epoch_order(n, 99, 1), D.epoch_order(n, 100, 0)
    for what, u, v in (("epochs", a, b), ("seeds", a, c)):
        same = float((u == v).mean())
        print("two %s agree in %.4f %% of the slots" % (what, 100 * same))
        assert same <= 1e-3


def test_chi_square_over_4000_epochs():
    """n = 1000, seed 99, epochs 0..3999, 50 bins: the image in slot 0, the slot of image 17 and (p[1] - p[0]) mod n, each below the
    1 - 1e-4 quantile of chi-square with 49 degrees of freedom (Wilson-Hilferty: 94.8).  Measured: 53.7, 48.0, 39.6."""
    n, E, bins = 1000, 4000, 50
    bound = D.chi2_quantile(1.0 - 1e-4, bins - 1)
    assert 94.5 < bound < 95.1, bound
    j, e = np.tile(np.arange(n), E), np.repeat(np.arange(E), n)
    p = D.perm(j, n, 99, e).reshape(E, n)
    assert np.array_equal(np.sort(p, axis=1), np.broadcast_to(np.arange(n), (E, n)))

    def chi2(v):
        h = np.bincount(v * bins // n, minlength=bins).astype(np.float64)
        return float(((h - E / bins) ** 2 / (E / bins)).sum())

    figures = [chi2(p[:, 0]), chi2(np.argmax(p == 17, axis=1)), chi2((p[:, 1] - p[:, 0]) % n)]
    print("chi-square (image in slot 0, slot of image 17, (p[1] - p[0]) mod n): %s; bound %.1f" % (" ".join("%.1f" % v for v in figures), bound))
    for v in figures:
        assert v < bound, (figures, bound)


def test_ranks_take_disjoint_images_that_cover_the_epoch():
    n, B, world, seed = 47, 5, 3, 2024
    bpe = D.batches_per_epoch(n, B, world)
    assert bpe == 3
    for epoch in (0, 1, 5):
        per_rank = [np.concatenate([D.batch_indices(n, seed, epoch * bpe + t, B, rank, world) for t in range(bpe)]) for rank in range(world)]
        for r in range(world):
            assert len(set(per_rank[r])) == bpe * B
            for q in range(r):
                assert not set(per_rank[r]) & set(per_rank[q]), (epoch, r, q)
        union = np.concatenate(per_rank)
        assert len(set(union)) == bpe * B * world and union.min() >= 0 and union.max() < n
        # the slots of the epoch are the first bpe * G of its order; the remainder is dropped
        assert set(union) == set(D.epoch_order(n, seed, epoch)[:bpe * B * world])
    np.testing.assert_array_equal(D.batch_indices(n, seed, bpe + 1, B, 1, world, deterministic=True), np.arange(20, 25))


def test_device_dataset_value_errors_on_the_host():
    import iaf_amd
    ok = torch.zeros(4, 3, 2, 2, dtype=torch.uint8)                 # right in everything but the device
    for seed in (-1, 1 << 64, 1.0, True, None):
        with pytest.raises(ValueError, match="seed"):
            iaf_amd.DeviceDataset(ok, seed)
    with pytest.raises(ValueError, match="deterministic"):
        iaf_amd.DeviceDataset(ok, 1, deterministic=1)
    for world in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="world"):
            iaf_amd.DeviceDataset(ok, 1, world=world)
    for rank, world in ((-1, 1), (1, 1), (3, 3), (True, 2), (0.0, 1)):
        with pytest.raises(ValueError, match="rank"):
            iaf_amd.DeviceDataset(ok, 1, rank=rank, world=world)
    for images in (ok, ok.numpy(), None, ok.float(), ok[:, :, :, :1], ok.reshape(4, 12), torch.zeros(4, 1, 2, 2, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="images"):
            iaf_amd.DeviceDataset(images, 1)


def _host_dataset(n=16, world=1):
    """a DeviceDataset's host bookkeeping without a device: what TrainStep's own checks look at"""
    import iaf_amd
    ds = iaf_amd.DeviceDataset.__new__(iaf_amd.DeviceDataset)
    ds.n, ds.rank, ds.world, ds._h = n, 0, world, None
    return ds


def test_train_step_data_value_errors_on_the_host():
    import iaf_amd
    m = HostModel()
    with pytest.raises(ValueError, match="DeviceDataset"):
        iaf_amd.TrainStep(m, 1e-3, graph=False, data=object(), batch_size=4)
    ds = _host_dataset()
    assert ds.batches_per_epoch(5) == 3
    for bs in (None, 0, -4, 2.0, True, "4"):
        with pytest.raises(ValueError, match="batch_size"):
            iaf_amd.TrainStep(m, 1e-3, graph=False, data=ds, batch_size=bs)
    with pytest.raises(ValueError, match="more than the dataset"):
        iaf_amd.TrainStep(m, 1e-3, graph=False, data=ds, batch_size=17)
    with pytest.raises(ValueError, match="batch_size goes with data"):
        iaf_amd.TrainStep(m, 1e-3, graph=False, batch_size=4)
    with pytest.raises(ValueError, match="device parameters"):
        iaf_amd.TrainStep(m, 1e-3, graph=False, data=ds, batch_size=4)          # host replicas take their batches from the caller
    ts = iaf_amd.TrainStep(m, 1e-3, graph=False)
    with pytest.raises(ValueError, match="data="):
        ts()                                                                    # no batch and no dataset
    with pytest.raises(ValueError, match="data="):
        ts(noise=[torch.zeros(7)])
    x = torch.tensor([1.0, 0.25])
    assert bool(torch.isfinite(ts(x, [torch.zeros(7)])).all())                  # every existing call keeps its meaning
    assert bool(torch.isfinite(ts(x, noise=[torch.zeros(7)])).all())
    assert bool(torch.isfinite(ts(x=x, noise=[torch.zeros(7)])).all())


def test_abi_argument_errors_answer_before_any_device_work():
    from iaf_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _capi.lib()
    h = ctypes.c_void_p()
    fake = ctypes.c_void_p(4096)                                    # never dereferenced: every call below is refused first
    assert lib.iaf_data_create(None, fake, 5, 12, 1, 0) == _capi.IAF_ERR_NULL
    assert lib.iaf_data_create(ctypes.byref(h), None, 5, 12, 1, 0) == _capi.IAF_ERR_NULL
    for n, bpi in ((0, 12), (1 << 32, 12), (5, 0)):
        assert lib.iaf_data_create(ctypes.byref(h), fake, n, bpi, 1, 0) == _capi.IAF_ERR_SHAPE
        assert not h.value
    assert lib.iaf_data_next_batch(None, fake, None, 1, 0, 1, 1, None) == _capi.IAF_ERR_NULL
    assert lib.iaf_data_seek(None, 0, None) == _capi.IAF_ERR_NULL
    assert lib.iaf_data_skip(None, 0, None) == _capi.IAF_ERR_NULL
    assert lib.iaf_data_tell(None, None, None) == _capi.IAF_ERR_NULL
    assert lib.iaf_data_destroy(None) == _capi.IAF_OK
    assert lib.iaf_abi_version() == 8


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_gather_kernel_uses_no_scratch(tmp_path):
    """the gather keeps its state in registers (hipcc's kernel-resource-usage remarks, device code only, of a unit that includes just the
    noise source's and the dataset's headers -- seconds instead of the whole engine)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    src = tmp_path / "data_kernels.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include "iaf_hip.h"\n#include "iaf_kernels_rng.hpp"\n'
                   '#include "iaf_kernels_data.hpp"\n')
    rows = [r for r in kr.unit_resources(str(src), str(tmp_path / "data_kernels.o"), []) if "iaf_data_gather" in r["name"]]
    assert len(rows) == 1, [r["name"] for r in rows]
    bad = [(r["name"], r.get("scratch"), r.get("vspill")) for r in rows if r.get("scratch", 0) or r.get("vspill", 0) or r.get("sspill", 0)]
    assert not bad, bad
