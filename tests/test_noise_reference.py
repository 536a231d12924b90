"""CPU checks of the device noise source's DEFINITION (include/iaf_hip.h, iaf_rng_*): the numpy statement of it
(tests/noise_reference.py) against the published Philox4x32-10 known answers and the two normal vectors the header prints, its
statistics, CVAE1.noise_shapes against the golden noise lists, and the new C symbols with their argument errors (no device)."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

import torch

import golden_inputs as gi
import noise_reference as R

from noise_reference import KA1, KA2, KA2_ARGS, check_statistics, STAT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_known_answers():
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(int(v[0]) for v in R.philox4x32_10(ctr, key)) == want


def test_normal_known_answers():
    np.testing.assert_allclose(R.normals(0, 0, 0, 8), KA1, rtol=0, atol=1e-6)
    np.testing.assert_allclose(R.normals(count=6, first=1000, **KA2_ARGS), KA2, rtol=0, atol=1e-6)
    # a window of a tensor is that window: partial counters at either end
    np.testing.assert_array_equal(R.normals(5, 1, 2, 11, first=3), R.normals(5, 1, 2, 14)[3:])
    np.testing.assert_array_equal(R.normals(5, 1, 2, 7, scale=0.7), 0.7 * R.normals(5, 1, 2, 7))
    assert np.abs(R.normals(1, 2, 3, 1 << 16)).max() <= np.sqrt(48 * np.log(2))


def test_reference_statistics():
    check_statistics(R.normals(STAT["seed"], STAT["substream"], STAT["step"], STAT["N"]))


@pytest.mark.parametrize("name", ["model_tiny", "model_cfg", "model_sample"])
def test_noise_shapes_equal_the_golden_noise_lists(name):
    import iaf_amd
    c = gi.model_case_inputs(name)
    # (building a CVAE1 creates engine objects on the device: the instance form, model.noise_shapes(B), is held to the same lists in
    # tests/test_hip_noise_model.py; this is the bookkeeping under it)
    shapes = iaf_amd.CVAE1.noise_shapes_for(c["B"] * c["k"], c["z_size"], c["depth"], c["num_blocks"], c["image_size"])
    assert shapes == [tuple(e.shape) for e in c["noise"]]
    assert len(shapes) == 2 * c["depth"] * c["num_blocks"]


def test_library_exports_the_noise_source_and_checks_arguments_without_a_device():
    from iaf_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _capi.lib()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    for s in ("iaf_rng_create", "iaf_rng_destroy", "iaf_rng_fill_normal", "iaf_rng_seek", "iaf_rng_skip", "iaf_rng_tell"):
        assert hasattr(raw, s) and s in _capi.SIGNATURES, s
    assert lib.iaf_abi_version() == 8                        # additive: the version the existing symbol test pins
    outs, counts = (ctypes.c_void_p * 65)(*([64] * 65)), (ctypes.c_size_t * 65)(*([4] * 65))
    subs = (ctypes.c_uint * 65)()
    # the argument checks come before the handle is looked into and before any device work: a stand-in handle is never read
    fake = ctypes.create_string_buffer(256)
    h = ctypes.cast(fake, ctypes.c_void_p)
    assert lib.iaf_rng_create(None, 1) == _capi.IAF_ERR_NULL
    assert lib.iaf_rng_fill_normal(None, outs, counts, subs, None, 1, 1, None) == _capi.IAF_ERR_NULL
    assert lib.iaf_rng_fill_normal(h, outs, counts, subs, None, 0, 1, None) == _capi.IAF_ERR_SHAPE
    assert lib.iaf_rng_fill_normal(h, outs, counts, subs, None, 65, 1, None) == _capi.IAF_ERR_SHAPE
    assert lib.iaf_rng_fill_normal(h, None, counts, subs, None, 1, 1, None) == _capi.IAF_ERR_NULL
    assert lib.iaf_rng_fill_normal(h, outs, None, subs, None, 1, 1, None) == _capi.IAF_ERR_NULL
    assert lib.iaf_rng_fill_normal(h, outs, counts, None, None, 1, 1, None) == _capi.IAF_ERR_NULL
    outs[1] = None
    assert lib.iaf_rng_fill_normal(h, outs, counts, subs, None, 2, 1, None) == _capi.IAF_ERR_NULL        # a null entry
    outs[1] = 64
    counts[1] = 0
    assert lib.iaf_rng_fill_normal(h, outs, counts, subs, None, 2, 1, None) == _capi.IAF_ERR_SHAPE
    counts[1] = (1 << 34) + 1
    assert lib.iaf_rng_fill_normal(h, outs, counts, subs, None, 2, 1, None) == _capi.IAF_ERR_SHAPE
    assert lib.iaf_rng_seek(None, 0, None) == _capi.IAF_ERR_NULL
    assert lib.iaf_rng_skip(None, 1, None) == _capi.IAF_ERR_NULL
    assert lib.iaf_rng_tell(None, None, None) == _capi.IAF_ERR_NULL
    assert lib.iaf_rng_destroy(None) == _capi.IAF_OK


class HostModel(object):
    """a host stand-in with CVAE1's training interface (as tests/test_train_step_api.py uses): obj = 0.5 x[0] |p|^2"""

    def __init__(self):
        self.params = {"a/V": torch.ones(3, 4), "b/g": torch.ones(5)}

    def completion_order(self):
        return list(self.params)

    def load(self, params):
        self.params = params

    def set_grad_buckets(self, n_buckets=1):
        return [list(self.params)]

    def prepare_weights(self):
        pass

    def fb_begin(self, x, noise, grads=None):
        self._g = grads
        return {"obj": (0.5 * x[0] * sum((p * p).sum() for p in self.params.values())).reshape(1)}

    def fb_segment(self, i):
        for k, p in self.params.items():
            self._g[k].copy_(p)


def test_train_step_noise_arguments_on_host_replicas():
    import iaf_amd
    ts = iaf_amd.TrainStep(HostModel(), 1e-3, graph=False)
    with pytest.raises(ValueError):
        ts(torch.ones(1))                                    # neither a source nor a noise list
    ts(torch.ones(1), [])                                    # the existing call form
    ts(torch.ones(1), noise=[])
    with pytest.raises(ValueError):
        iaf_amd.TrainStep(HostModel(), 1e-3, graph=False, noise_source=object())      # a source needs device parameters


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_noise_kernels_use_no_scratch(tmp_path):
    """hipcc's kernel-resource-usage remarks, device code only, of a unit that includes just the noise kernels' header"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    src = tmp_path / "rng_kernels.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include "iaf_hip.h"\n#include "iaf_kernels_rng.hpp"\n')
    rows = [r for r in kr.unit_resources(str(src), str(tmp_path / "rng_kernels.o"), []) if "iaf_rng_" in r["name"]]
    assert len(rows) == 2, [r["name"] for r in rows]
    bad = [(r["name"], r.get("scratch"), r.get("vspill")) for r in rows if r.get("scratch", 0) or r.get("vspill", 0)]
    assert not bad, bad
