"""CPU-side checks of the four elementwise entry points of the 'down_iaf2_nl2' chain (iaf_chain_head / _tail / _backward_pre /
_backward_post): the library exports them, the header declares them, the ctypes table binds them with the header's arity, and null
pointers and non-positive sizes are refused before any device work; and the Python surface of the posterior (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name: (arity, positions of the required pointers, positions of B, n_h, n_z, HW)
ENTRY_POINTS = {
    "iaf_chain_head": (11, (0, 1, 2, 3, 4, 5), (6, 7, 8, 9)),
    "iaf_chain_tail": (12, (0, 1, 2, 3, 4, 5, 6), (7, 8, 9, 10)),
    "iaf_chain_backward_pre": (14, (0, 1, 2, 6, 7, 8), (9, 10, 11, 12)),            # 3 = gate, 4 = gscale, 5 = dko
    "iaf_chain_backward_post": (15, (0, 1, 2, 3, 4, 5, 6, 8, 9), (10, 11, 12, 13)),  # 7 = d_up, optional
}


@pytest.fixture(scope="module")
def capi():
    from iaf_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _capi.lib()
    return _capi


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_chain_symbol_is_exported_declared_and_bound(capi, name):
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), name)
    txt = open(os.path.join(ROOT, "include", "iaf_hip.h")).read()
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", txt)
    assert m, "header does not declare " + name
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    res, args = capi.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == n_args == ENTRY_POINTS[name][0]
    assert capi.lib().iaf_abi_version() == 8, "the addition is backward compatible: the ABI version stays"


def _full_args(name, fake):
    n, ptrs, sizes = ENTRY_POINTS[name]
    args = [None] * n
    for i in ptrs:
        args[i] = fake
    for i, v in zip(sizes, (2, 5, 3, 7)):
        args[i] = v
    if name == "iaf_chain_backward_pre":
        args[3], args[4], args[5] = fake, 0.5, None
    return args


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_chain_entry_point_validates_arguments_before_device_work(capi, name):
    """every required pointer NULL -> IAF_ERR_NULL, every size zero or negative -> IAF_ERR_SHAPE; the tensor pointers point nowhere (address
    16) and no stream exists, so an answer at all means that nothing was launched or dereferenced"""
    fn = getattr(capi.lib(), name)
    n, ptrs, sizes = ENTRY_POINTS[name]
    fake = ctypes.c_void_p(16)
    for i in ptrs:
        args = _full_args(name, fake)
        args[i] = None
        assert fn(*args) == capi.IAF_ERR_NULL, i
    for i in sizes:
        for v in (0, -1):
            args = _full_args(name, fake)
            args[i] = v
            assert fn(*args) == capi.IAF_ERR_SHAPE, (i, v)
    if name == "iaf_chain_backward_pre":          # one of gate / dko is required
        args = _full_args(name, fake)
        args[3] = None
        assert fn(*args) == capi.IAF_ERR_NULL
    args = _full_args(name, fake)                 # null pointers are reported before bad sizes
    args[ptrs[0]], args[sizes[0]] = None, 0
    assert fn(*args) == capi.IAF_ERR_NULL


def test_chain_posterior_is_part_of_the_layer_surface():
    from iaf_amd import theano_layer
    assert "down_iaf2_nl2" in theano_layer.POSTERIORS
    for nm in ("_down_q_chain", "_backward_chain"):
        assert callable(getattr(theano_layer.CVAELayerIAF, nm))
    with pytest.raises(Exception, match="Unknown posterior"):
        theano_layer.CVAELayerIAF("1", 32, 16, 2, posterior="down_iaf2_nl3")
