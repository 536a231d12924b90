"""CPU tests of the plain Theano conv's restatement (tests/theano_conv_reference.py) and of the API surface of the feature: the torch-fp64
statement equals oracle.iaf_oracle.theano_conv2d and central finite differences; the 16 position classes and the geometry table that
reaches them; the tolerance of the GPU tests (1e-4) cannot hide a missing border addend or a missing flip; the new entry point is in
the header and the binding; CVAELayer's refusals; WNConv2d(theano=True) with ar_mask=None is no longer a ValueError."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import theano_conv_reference as TR
from oracle import iaf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_elu = lambda t: np.where(t < 0, np.exp(np.minimum(t, 0)) - 1, t)


def _case(seed, B, n_in, n_out, H, W):
    rng = np.random.RandomState(seed)
    w, s, b = TR.rand_conv(rng, n_in, n_out)
    x = 0.3 * rng.standard_normal((B, n_in, H, W))
    return x, w, s, b


@pytest.mark.parametrize("geom", TR.GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_torch_statement_equals_the_oracle(geom):
    H, W = geom
    x, w, s, b = _case(0, 2, 5, 7, H, W)
    ref = O.theano_conv2d(x, w, b, s)
    got = TR.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(s), torch.from_numpy(b)).numpy()
    assert got.shape == ref.shape == (2, 7, H, W)
    np.testing.assert_allclose(got, ref, atol=1e-12, rtol=0)


@pytest.mark.parametrize("geom", [(1, 1), (2, 2), (3, 4)], ids=lambda g: "%dx%d" % g)
def test_autograd_equals_central_differences(geom):
    """w (border channel included), s, b and x: d <dy, y> / d theta by autograd against (L(theta + h) - L(theta - h)) / 2h, h = 1e-6"""
    H, W = geom
    x, w, s, b = _case(1, 2, 3, 4, H, W)
    dy = np.random.RandomState(2).standard_normal((2, 4, H, W))
    ts = [torch.from_numpy(a.copy()).requires_grad_(True) for a in (x, w, s, b)]
    (TR.conv2d(*ts) * torch.from_numpy(dy)).sum().backward()
    L = lambda xx, ww, ss, bb: float((O.theano_conv2d(xx, ww, bb, ss) * dy).sum())
    args = [x, w, s, b]
    rng = np.random.RandomState(3)
    for k, name in enumerate(("x", "w", "s", "b")):
        g = ts[k].grad.numpy()
        flat = [np.unravel_index(i, args[k].shape) for i in rng.choice(args[k].size, size=min(args[k].size, 12), replace=False)]
        if name == "w":
            flat += [(o, 3, a, c) for o in (0, 3) for a in range(3) for c in range(3)]            # the border channel, every tap
        for idx in flat:
            hi, lo = [a.copy() for a in args], [a.copy() for a in args]
            hi[k][idx] += 1e-6
            lo[k][idx] -= 1e-6
            fd = (L(*hi) - L(*lo)) / 2e-6
            assert abs(fd - g[idx]) < 1e-6 * max(1.0, abs(fd)), (name, idx, fd, g[idx])


def test_border_channel_gradient_is_the_sum_of_dy_over_leaving_taps():
    """dK of the border channel, as the issue states it: tap (dh,dw) collects dY over the pixels whose neighbour (dh,dw) is outside;
    the centre tap collects nothing"""
    H, W = 3, 4
    x, w, s, b = _case(4, 2, 3, 4, H, W)
    dy = np.random.RandomState(5).standard_normal((2, 4, H, W))
    K = TR.effective_kernel(torch.from_numpy(w), torch.from_numpy(s)).detach().requires_grad_(True)
    kd, kb = K[:, :3].flip(2, 3), K[:, 3:].flip(2, 3)
    y = torch.nn.functional.conv2d(torch.from_numpy(x), kd, padding=1) + torch.nn.functional.conv2d(TR.border_indicator(H, W), kb)
    (y * torch.from_numpy(dy)).sum().backward()
    dK = K.grad.numpy()
    for dh in (-1, 0, 1):
        for dw in (-1, 0, 1):
            out = np.array([[not (0 <= i + dh < H and 0 <= j + dw < W) for j in range(W)] for i in range(H)])
            want = (dy * out[None, None]).sum(axis=(0, 2, 3))
            np.testing.assert_allclose(dK[:, 3, 1 - dh, 1 - dw], want, atol=1e-12)
    assert not dK[:, 3, 1, 1].any()


def test_sixteen_position_classes_and_the_table_reaches_them():
    seen = set()
    for H, W in TR.GEOMETRIES:
        seen |= set(TR.position_classes(H, W).ravel().tolist())
    assert seen == set(range(16))
    assert set(TR.position_classes(1, 1).ravel().tolist()) == {15}
    # without the degenerate shapes the table would miss classes: 3x7 and 6x5 alone reach only the nine ordinary ones
    assert len(set(TR.position_classes(3, 7).ravel().tolist()) | set(TR.position_classes(6, 5).ravel().tolist())) == 9


@pytest.mark.parametrize("geom", TR.GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_output_is_bias_table_plus_data_term(geom):
    """the form the kernels use: y = data term + table[class of the pixel], table[cls] = b + the class's border addend"""
    H, W = geom
    x, w, s, b = _case(6, 2, 5, 7, H, W)
    ts = [torch.from_numpy(a) for a in (x, w, s, b)]
    K = TR.effective_kernel(ts[1], ts[2])
    data = TR.conv2d(*ts, border=False) - ts[3].reshape(1, -1, 1, 1)
    cls = TR.position_classes(H, W)
    table = torch.stack([ts[3] + TR.class_addend(K, c) for c in range(16)])          # [16, n_out]
    y = data + table[torch.from_numpy(cls)].permute(2, 0, 1)[None]
    np.testing.assert_allclose(y.numpy(), TR.conv2d(*ts).numpy(), atol=1e-12, rtol=0)


@pytest.mark.parametrize("geom", TR.GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_tolerance_cannot_hide_a_missing_term(geom):
    """at the GPU tests' scales (seed 0, 32 -> 96) the output moves by more than 0.1 -- a thousand times ATOL = 1e-4 -- when the border
    addend is dropped with the norm kept, and when the flip is dropped (everywhere but 1x1, where the flip changes nothing)"""
    H, W = geom
    x, w, s, b = _case(0, 2, 32, 96, H, W)
    ts = [TR.t64(a) for a in (x, w, s, b)]
    y = TR.conv2d(*ts)
    d_border = float((y - TR.conv2d(*ts, border=False)).abs().max())
    d_flip = float((y - TR.conv2d(*ts, flip=False)).abs().max())
    print("%dx%d: border addend dropped %.3g, flip dropped %.3g" % (H, W, d_border, d_flip))
    assert d_border > 0.1
    if (H, W) != (1, 1):
        assert d_flip > 0.1
    else:
        assert d_flip < 1e-12


def test_conv_widths_follow_the_reference():
    assert TR.conv_widths(160, 32, "down_iaf2_nl", "diag") == {"_up_conv1_1": (160, 384), "_up_conv2": (160, 160), "_down_conv1": (160, 448),
                                                               "_down_conv2_1": (192, 160)}
    assert TR.conv_widths(160, 32, "up_iaf2_nl", "diag")["_up_conv2"] == (192, 160)
    assert TR.conv_widths(160, 32, "up_iaf2_nl", "diag")["_down_conv1"] == (160, 224)
    assert TR.conv_widths(160, 32, "down_iaf2_nl2", "made")["_down_conv1"] == (160, 3 * 160 + 2 * 32)


# ---------------------------------------------------------------- the API surface
def test_entry_point_is_in_the_header_and_the_binding():
    hdr = open(os.path.join(ROOT, "include", "iaf_hip.h")).read()
    assert re.search(r"int iaf_conv3x3_create_theano\(iaf_conv3x3_t\*\* out, int n_in, int n_out\);", hdr)
    from iaf_amd import _capi
    assert "iaf_conv3x3_create_theano" in _capi.SIGNATURES
    assert _capi.IAF_ABI_VERSION == 8          # an additive change: the ABI version stays (the loader compares it with the library's)


def test_public_names_and_signatures():
    import iaf_amd
    from iaf_amd import layers
    assert iaf_amd.CVAELayer is not None and iaf_amd.conv2d_theano is layers.conv2d_theano
    sig = inspect.signature(iaf_amd.CVAELayer.__init__)
    assert list(sig.parameters)[1:9] == ["name", "n_h", "n_z", "depth_ar", "posterior", "prior", "flipmask", "kl_min"]
    for m in ("load", "up", "down_q", "down_p", "backward_down", "backward_up", "grads", "set_training"):
        assert callable(getattr(iaf_amd.CVAELayer, m))
    U = iaf_amd._capi.UnsupportedError
    for kw in (dict(size_kernel=(5, 5)), dict(downsample=2), dict(upsample=2), dict(pad_channel=False)):
        with pytest.raises(U):
            layers.conv2d_theano("c", 16, 16, **kw)


def test_cvae_layer_refuses_downsampling_before_touching_the_device():
    import iaf_amd
    with pytest.raises(iaf_amd._capi.UnsupportedError) as e:
        iaf_amd.CVAELayer("1", 32, 16, 1, downsample=True)
    assert "strided" in str(e.value) and "nn" in str(e.value)
    with pytest.raises(Exception, match="Unknown posterior"):
        iaf_amd.CVAELayer("1", 32, 16, 1, posterior="nope", downsample=False)


def test_plain_theano_conv_is_no_longer_a_value_error():
    """WNConv2d(theano=True, ar_mask=None) used to raise ValueError before any library call; now it reaches iaf_conv3x3_create_theano
    (without a built library that is an OSError / RuntimeError from the loader, never the old ValueError); flipmask stays refused"""
    from iaf_amd import layers
    src = inspect.getsource(layers.WNConv2d.__init__)
    assert "iaf_conv3x3_create_theano" in src and "theano=True is the masked conv" not in src
    with pytest.raises(ValueError):
        layers.WNConv2d(16, 16, theano=True, flipmask=True)
