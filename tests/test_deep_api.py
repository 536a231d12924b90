"""CPU-side checks of the masked-ResNet stack's boundary: iaf_stack_create_resnet is declared, exported and bound, the ABI version is what
it was, its argument validation answers before any device call, 'down_iaf2_deep' is a known posterior, and layers.resnet refuses what
is not built by name.  No compute calls (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from iaf_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _capi.lib()
    return _capi


def test_create_resnet_is_declared_exported_and_bound(capi):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iaf_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+iaf_stack_create_resnet\s*\(\s*iaf_stack_t\s*\*\*\s*out\s*,\s*int n_z\s*,\s*int n_h\s*,\s*int depth\s*,\s*int variant\s*\)", txt)
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "iaf_stack_create_resnet")
    restype, argtypes = capi.SIGNATURES["iaf_stack_create_resnet"]
    assert restype is ctypes.c_int and len(argtypes) == 5
    assert capi.lib().iaf_abi_version() == 8 == capi.IAF_ABI_VERSION


def test_create_resnet_validates_its_arguments(capi):
    lib = capi.lib()
    h = ctypes.c_void_p()
    T = capi.IAF_VARIANT_THEANO
    assert lib.iaf_stack_create_resnet(None, 32, 64, 2, T) == capi.IAF_ERR_NULL
    assert lib.iaf_stack_create_resnet(ctypes.byref(h), 32, 64, 0, T) == capi.IAF_ERR_SHAPE
    assert lib.iaf_stack_create_resnet(ctypes.byref(h), 32, 64, 5, T) == capi.IAF_ERR_SHAPE          # 1 + 2 * 5 + 1 layers: more than the engine holds
    assert lib.iaf_stack_create_resnet(ctypes.byref(h), 32, 64, 2, capi.IAF_VARIANT_TF) == capi.IAF_ERR_UNSUPPORTED
    assert lib.iaf_stack_create_resnet(ctypes.byref(h), 32, 64, 2, capi.IAF_VARIANT_THEANO_FLIPMASK) == capi.IAF_ERR_UNSUPPORTED
    assert lib.iaf_stack_create_resnet(ctypes.byref(h), 24, 48, 2, T) == capi.IAF_ERR_UNSUPPORTED   # channels % 16
    assert lib.iaf_stack_create_resnet(ctypes.byref(h), 32, 48, 2, T) == capi.IAF_ERR_NOT_MULTIPLE
    assert lib.iaf_stack_create_resnet(ctypes.byref(h), 0, 64, 2, T) == capi.IAF_ERR_SHAPE
    assert not h.value
    assert lib.iaf_stack_get_dgrad_precision(None, 0, 1, 1, 1) == capi.IAF_ERR_NULL


def test_down_iaf2_deep_is_a_known_posterior():
    from iaf_amd import theano_layer
    assert "down_iaf2_deep" in theano_layer.POSTERIORS
    with pytest.raises(ValueError, match="made"):
        theano_layer.CVAELayerIAF("1", 32, 32, 1, posterior="down_iaf2_deep", prior="made")
    with pytest.raises(Exception, match="Unknown posterior"):
        theano_layer.CVAELayerIAF("1", 32, 32, 1, posterior="down_iaf1_deep")


def test_layers_resnet_refuses_what_is_not_built():
    import iaf_amd
    from iaf_amd import layers
    U = iaf_amd.UnsupportedError
    with pytest.raises(U, match="flipmask"):
        layers.resnet("r", 2, 32, 64, [32, 32], flipmask=True)
    with pytest.raises(U, match="layertype"):
        layers.resnet("r", 2, 32, 64, [32, 32], layertype="b")
    with pytest.raises(U, match="weight sharing"):
        layers.resnet("r", 2, 32, 64, [32, 32], weightsharing=True)
    with pytest.raises(U, match="nl="):
        layers.resnet("r", 2, 32, 64, [32, 32], nl="relu")
    with pytest.raises(U, match="size_kernel"):
        layers.resnet("r", 2, 32, 64, [32, 32], size_kernel=(5, 5))
    with pytest.raises(U, match="flipmask"):
        iaf_amd.CVAELayerIAF("1", 64, 32, 2, posterior="down_iaf2_deep", flipmask=True)
    assert layers.ResnetARStack._theano_bases(type("S", (), {"depth": 2})()) == ["input", "0_conv1", "0_conv2", "1_conv1", "1_conv2",
                                                                                 "out_0", "out_1"]
