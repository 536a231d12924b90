"""CPU-side checks of the prior-sample entry point behind CVAE1.generate (iaf_conv3x3_forward_prior_sample): the library exports it,
the ctypes table binds it as the header declares it, and a missing argument is refused before any device call (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "iaf_conv3x3_forward_prior_sample"


@pytest.fixture(scope="module")
def capi():
    from iaf_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _capi.lib()
    return _capi


def test_prior_sample_symbol_is_exported_and_declared(capi):
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), NAME)
    txt = open(os.path.join(ROOT, "include", "iaf_hip.h")).read()
    m = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)", txt)
    assert m, "header does not declare " + NAME
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    res, args = capi.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == n_args == 12


def test_prior_sample_validates_arguments_before_device_work(capi):
    """null pointers -> IAF_ERR_NULL, impossible sizes -> IAF_ERR_SHAPE, both before the conv object or any device memory is touched (the
    handle here is a zeroed host buffer and the tensor pointers point nowhere)"""
    lib = capi.lib()
    fn = getattr(lib, NAME)
    handle = ctypes.create_string_buffer(4096)
    h, fake = ctypes.cast(handle, ctypes.c_void_p), ctypes.c_void_p(16)
    full = [h, fake, 1, 32, 160, fake, fake, fake, 2, 8, 8, None]
    for i in (0, 1, 5, 6, 7):             # conv, x, eps, z, h_det
        args = list(full)
        args[i] = None
        assert fn(*args) == capi.IAF_ERR_NULL, i
    for i, v in ((3, 0), (4, -16), (8, 0), (9, 0), (10, -1)):     # n_z, n_h, B, H, W
        args = list(full)
        args[i] = v
        assert fn(*args) == capi.IAF_ERR_SHAPE, i
    assert not any(handle.raw), "the handle was written"
