"""CPU-side checks of the six elementwise entry points of the 'made' prior (iaf_made_head / _tail / _backward_pre / _backward_join /
_backward_post, iaf_diag_prior_sample): the library exports them, the header declares them, the ctypes table binds them with the header's
arity, and null pointers and non-positive sizes are refused before any device work; and the Python surface of the prior (no GPU
needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name: (arity, positions of the required pointers, positions of the sizes, the sizes of a valid call)
ENTRY_POINTS = {
    "iaf_made_head": (12, (0, 1, 2, 3, 4, 5, 6), (7, 8, 9, 10), (2, 5, 3, 7)),
    "iaf_made_tail": (14, (0, 1, 2, 4, 5, 6, 8), (9, 10, 11, 12), (2, 5, 3, 7)),      # 3 = logdet2, optional; 7 = kl_elem, see below
    "iaf_made_backward_pre": (13, (0, 1, 5, 6, 7), (8, 9, 10, 11), (2, 5, 3, 7)),     # 2 = gate, 3 = gscale, 4 = dko
    "iaf_made_backward_join": (10, (0, 1, 2, 3, 4), (5, 6, 7, 8), (2, 5, 3, 7)),
    "iaf_made_backward_post": (15, (0, 1, 2, 3, 4, 5, 8, 9), (10, 11, 12, 13), (2, 5, 3, 7)),   # 6 = dctx2, 7 = d_up: optional
    "iaf_diag_prior_sample": (9, (0, 1, 2), (3, 4, 5, 6, 7), (2, 11, 5, 3, 7)),        # B, n_down, n_h, n_z, HW
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
def test_made_symbol_is_exported_declared_and_bound(capi, name):
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), name)
    txt = open(os.path.join(ROOT, "include", "iaf_hip.h")).read()
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", txt)
    assert m, "header does not declare " + name
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    res, args = capi.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == n_args == ENTRY_POINTS[name][0]
    assert capi.lib().iaf_abi_version() == 8, "the addition is backward compatible: the ABI version stays"


def _full_args(name, fake):
    n, ptrs, sizes, vals = ENTRY_POINTS[name]
    args = [None] * n
    for i in ptrs:
        args[i] = fake
    for i, v in zip(sizes, vals):
        args[i] = v
    if name == "iaf_made_tail":
        args[7] = fake                            # kl_elem given: logq0, logdet1, u, s_p are required
    if name == "iaf_made_backward_pre":
        args[2], args[3], args[4] = fake, 0.5, None
    return args


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_made_entry_point_validates_arguments_before_device_work(capi, name):
    """every required pointer NULL -> IAF_ERR_NULL, every size zero or negative -> IAF_ERR_SHAPE; the tensor pointers point nowhere (address
    16) and no stream exists, so an answer at all means that nothing was launched or dereferenced"""
    fn = getattr(capi.lib(), name)
    n, ptrs, sizes, vals = ENTRY_POINTS[name]
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
    if name == "iaf_made_backward_pre":           # one of gate / dko is required
        args = _full_args(name, fake)
        args[2] = None
        assert fn(*args) == capi.IAF_ERR_NULL
    if name == "iaf_made_tail":                   # the pack alone (kl_elem NULL) still needs down, z and h_out
        for i in (0, 4, 8):
            args = _full_args(name, fake)
            args[1] = args[2] = args[5] = args[6] = args[7] = None
            args[i] = None
            assert fn(*args) == capi.IAF_ERR_NULL, i
    if name == "iaf_diag_prior_sample":           # n_down must hold [h_det | pz_mean | pz_logsd]
        args = _full_args(name, fake)
        args[4] = 5 + 2 * 3 - 1
        assert fn(*args) == capi.IAF_ERR_SHAPE
    args = _full_args(name, fake)                 # null pointers are reported before bad sizes
    args[ptrs[0]], args[sizes[0]] = None, 0
    assert fn(*args) == capi.IAF_ERR_NULL


def test_made_prior_is_part_of_the_layer_surface():
    import inspect

    from iaf_amd import theano_layer
    assert theano_layer.PRIORS == ("diag", "made")
    sig = inspect.signature(theano_layer.CVAELayerIAF.__init__)
    assert list(sig.parameters)[-1] == "prior" and sig.parameters["prior"].default == "diag"
    for nm in ("down_p", "_down_q_made", "_backward_made"):
        assert callable(getattr(theano_layer.CVAELayerIAF, nm))
    p = inspect.signature(theano_layer.CVAELayerIAF.down_p).parameters
    assert [p[k].default for k in ("exact", "max_sweeps", "tol", "check_every")] == [True, 64, 1e-6, 4]
    with pytest.raises(Exception, match="Unknown prior"):
        theano_layer.CVAELayerIAF("1", 32, 16, 2, prior="bernoulli")
    with pytest.raises(Exception, match="Unknown prior"):
        theano_layer.CVAELayerIAF("1", 32, 16, 2, posterior="down_iaf2_nl2", prior="diag2")
    with pytest.raises(ValueError, match="not built"):
        theano_layer.CVAELayerIAF("1", 32, 16, 2, posterior="up_iaf2_nl", prior="made")
