"""CPU-side checks of the h_det-only entry point behind CVAE1.decode (iaf_conv3x3_forward_hdet) and of the latent API's surface: the
library exports the symbol, the ctypes table binds it as the header declares it, a missing argument is refused before any device call,
and the Python entry points exist (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "iaf_conv3x3_forward_hdet"


@pytest.fixture(scope="module")
def capi():
    from iaf_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _capi.lib()
    return _capi


def test_hdet_symbol_is_exported_and_declared(capi):
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), NAME)
    txt = open(os.path.join(ROOT, "include", "iaf_hip.h")).read()
    m = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)", txt)
    assert m, "header does not declare " + NAME
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    res, args = capi.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == n_args == 10


def test_hdet_validates_arguments_before_device_work(capi):
    """null pointers -> IAF_ERR_NULL, impossible sizes -> IAF_ERR_SHAPE (n_out != 4 n_z + 2 n_h among them), both before the conv object is
    written or any device memory is touched (the handle here is a zeroed host buffer and the tensor pointers point nowhere)"""
    lib = capi.lib()
    fn = getattr(lib, NAME)
    handle = ctypes.create_string_buffer(4096)
    h, fake = ctypes.cast(handle, ctypes.c_void_p), ctypes.c_void_p(16)
    full = [h, fake, 1, 32, 160, fake, 2, 8, 8, None]
    for i in (0, 1, 5):                   # conv, x, h_det
        args = list(full)
        args[i] = None
        assert fn(*args) == capi.IAF_ERR_NULL, i
    for i, v in ((3, 0), (4, -16), (6, 0), (7, 0), (8, -1)):      # n_z, n_h, B, H, W
        args = list(full)
        args[i] = v
        assert fn(*args) == capi.IAF_ERR_SHAPE, i
    assert fn(*full) == capi.IAF_ERR_SHAPE                        # the zeroed object's n_out (0) is not 4 n_z + 2 n_h
    args = list(full)
    args[6] = 1 << 20                                             # B H W beyond what the pixel index arithmetic holds
    assert fn(*args) == capi.IAF_ERR_SHAPE
    assert not any(handle.raw), "the handle was written"


def test_latent_entry_points_exist():
    import iaf_amd
    for nm in ("encode", "decode", "reconstruct", "reconstruct_ladder", "_top_down_mixed"):
        assert callable(getattr(iaf_amd.CVAE1, nm))
    assert callable(iaf_amd.IAFLayer.down_from) and callable(iaf_amd.WNConv2d.hdet) and callable(iaf_amd.WNConv2d._hdet)
    assert callable(iaf_amd.lerp_latents) and "lerp_latents" in iaf_amd.__all__


def test_lerp_latents_validates_on_the_host():
    """alpha and the lists are checked before any tensor is looked at or any launch made"""
    import iaf_amd
    with pytest.raises(ValueError):
        iaf_amd.lerp_latents([], [], 0.5)
    with pytest.raises(ValueError):
        iaf_amd.lerp_latents([None], [None], float("nan"))
    with pytest.raises(ValueError):
        iaf_amd.lerp_latents([None], [None, None], 0.5)
    with pytest.raises(ValueError):
        iaf_amd.lerp_latents([None], [None], 0.5)                 # not tensors
