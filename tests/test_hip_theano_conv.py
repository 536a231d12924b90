"""GPU tests of the plain conv of the Theano path (iaf_conv3x3_create_theano / iaf_amd.WNConv2d(theano=True); graphy/nodes/conv.py:122-260):
forward against the fp64 statement over the geometry table that reaches all 16 position classes, on both kernel families and with every
fused form; every compiled launch shape; the batched prepare; the backward pass against torch-fp64 autograd; the refusals the header
lists; and a TF plain conv before and after a Theano conv ran.  Reference: tests/theano_conv_reference.py (pinned on the CPU by
tests/test_theano_conv_reference.py).  Bounds: those of tests/test_hip_deep.py -- forward 1e-4 absolute against fp64 on fp32-rounded
inputs, the split products at most twice the exact family's error + 1e-6, gradients 1e-4 (exact family) / 2e-4 (split products) of the
reference's largest entry.  Inputs at the fixtures' scales (weights 0.05, s and b 0.1, activations 0.3)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import theano_conv_reference as TR
from iaf_amd import build

pytestmark = pytest.mark.gpu

ATOL = 1e-4


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()      # raises if the HIP extension is missing: no silent fallback
    return iaf_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def _rel_err(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)


# name: (n_in, n_out, c_split of x2 or 0, elu_input, residual, split)
FORMS = {
    "16to16": (16, 16, 0, False, False, None),
    "32to96_split": (32, 96, 0, False, False, [32, 16, 16, 32]),
    "48to32_x2_elu_res": (48, 32, 32, True, True, None),
    "64to32_x2_res": (64, 32, 32, False, True, None),
    "32to128": (32, 128, 0, False, False, None),
}


@functools.lru_cache(maxsize=None)
def _fwd_case(form, B, H, W):
    n_in, n_out, c_split, elu_in, residual, split = FORMS[form]
    rng = np.random.RandomState(100 + 7 * n_in + n_out + 13 * H + W + B)
    w, s, b = TR.rand_conv(rng, n_in, n_out)
    x = 0.3 * rng.standard_normal((B, n_in, H, W))
    res = 0.3 * rng.standard_normal((B, n_out, H, W)) if residual else None
    a = TR.t64(x)
    y = TR.conv2d(TR.elu(a) if elu_in else a, TR.t64(w), TR.t64(s), TR.t64(b)).numpy()
    ref = TR.t64(res).numpy() + 0.1 * y if residual else y
    return x, w, s, b, res, ref


def _forward(conv, form, x, res):
    n_in, n_out, c_split, elu_in, residual, split = FORMS[form]
    xd = dev(x)
    x1, x2 = (xd[:, :c_split].contiguous(), xd[:, c_split:].contiguous()) if c_split else (xd, None)
    outs = conv(x1, x2=x2, elu_input=elu_in, split=split, residual=dev(res) if residual else None)
    return np.concatenate([host(o) for o in outs], axis=1)


def _pin_split(conv, n_out):
    """a split-product launch shape (ppw 2, ks 4, one co group) whose co tiles divide the conv's: launches below 4096 pixels stay on the
    exact-fp32 kernel otherwise"""
    nt = [n for n in (4, 2) if (n_out // 16) % n == 0][0]
    conv.set_tuning(-nt, 2, 1, 4)


# ---------------------------------------------------------------- 1. forward against fp64
@pytest.mark.parametrize("geom", TR.GEOMETRIES, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_forward_vs_fp64_over_the_geometry_table(amd, form, geom):
    """B = 2: the exact-fp32 family at 1e-4 and, where the conv has the split pack (c_in a multiple of 32), the split products (pinned,
    asserted) at twice the exact family's error + 1e-6"""
    H, W = geom
    n_in, n_out = FORMS[form][:2]
    x, w, s, b, res, ref = _fwd_case(form, 2, H, W)
    conv = amd.WNConv2d(n_in, n_out, theano=True)
    conv.set_precision("f32")
    conv.prepare(dev(w), dev(s), dev(b))
    assert not conv.runs_bf16x3(2, H, W) and not conv.runs_f16x2(2, H, W)
    got = _forward(conv, form, x, res)
    err32 = np.abs(got - ref).max()
    print("%s %dx%d exact: max |err| %.3g (max |ref| %.3g)" % (form, H, W, err32, np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, atol=ATOL, rtol=0)
    if n_in % 32:
        return
    conv.set_precision("bf16x3")
    conv.prepare(dev(w), dev(s), dev(b), force=True)
    _pin_split(conv, n_out)
    assert conv.runs_bf16x3(2, H, W) and not conv.runs_f16x2(2, H, W)
    got3 = _forward(conv, form, x, res)
    err3 = np.abs(got3 - ref).max()
    print("%s %dx%d split: max |err| %.3g" % (form, H, W, err3))
    np.testing.assert_allclose(got3, ref, atol=ATOL, rtol=0)
    assert err3 <= 2 * err32 + 1e-6, (err3, err32)


def test_forward_above_4096_pixels_chooses_the_split_products(amd):
    """(17, 32 -> 96, 16x16): 4352 pixels, the split products without a pin"""
    form, B, H, W = "32to96_split", 17, 16, 16
    x, w, s, b, res, ref = _fwd_case(form, B, H, W)
    conv = amd.WNConv2d(32, 96, theano=True)
    conv.prepare(dev(w), dev(s), dev(b))
    assert conv.runs_bf16x3(B, H, W) and not conv.runs_f16x2(B, H, W)
    got3 = _forward(conv, form, x, res)
    conv.set_precision("f32")
    conv.prepare(dev(w), dev(s), dev(b), force=True)
    assert not conv.runs_bf16x3(B, H, W)
    got = _forward(conv, form, x, res)
    err32, err3 = np.abs(got - ref).max(), np.abs(got3 - ref).max()
    print("B17 16x16: exact %.3g, split %.3g (max |ref| %.3g)" % (err32, err3, np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, atol=ATOL, rtol=0)
    np.testing.assert_allclose(got3, ref, atol=ATOL, rtol=0)
    assert err3 <= 2 * err32 + 1e-6


# ---------------------------------------------------------------- 2. every compiled launch shape
# 64 -> 96 at 3x7 (six co tiles), and 64 -> 128 beside it: no co tiling of the two-group split-product shape (4, 8 or 10 tiles per
# workgroup) wastes at most a quarter of SIX tiles, so that entry launches at eight
SWEEP_WIDTHS = (96, 128)


@functools.lru_cache(maxsize=None)
def _sweep_case(n_out):
    B, n_in, H, W = 2, 64, 3, 7
    rng = np.random.RandomState(211 + n_out)
    w, s, b = TR.rand_conv(rng, n_in, n_out)
    x = 0.3 * rng.standard_normal((B, n_in, H, W))
    ref = TR.conv2d(TR.t64(x), TR.t64(w), TR.t64(s), TR.t64(b)).numpy()
    return B, n_in, H, W, x, w, s, b, ref


@pytest.mark.parametrize("shape", build.SHAPES, ids=lambda s: "pxt%d_wco%d_ks%d" % s)
def test_every_exact_fp32_launch_shape(amd, shape):
    """every IAF_CONV entry of iaf_variants.def, every admissible co-tile count pinned; at least one must launch at 64 -> 96"""
    pxt, wco, ks = shape
    ran = []
    for n_out in SWEEP_WIDTHS:
        B, n_in, H, W, x, w, s, b, ref = _sweep_case(n_out)
        conv = amd.WNConv2d(n_in, n_out, theano=True)
        conv.prepare(dev(w), dev(s), dev(b))
        for nt in (1, 2, 3, 4, 5):
            if (n_out // 16) % (nt * wco) or n_in // 16 < ks:
                continue
            conv.set_tuning(nt, pxt, wco, ks)
            assert not conv.runs_bf16x3(B, H, W)
            np.testing.assert_allclose(host(conv(dev(x))[0]), ref, atol=ATOL, rtol=0, err_msg="n_out %d nt %d" % (n_out, nt))
            ran.append((n_out, nt))
    print(shape, "launched", ran)
    assert any(n == 96 for n, _ in ran), "no co-tile count of this shape launched at 64 -> 96"


@pytest.mark.parametrize("shape", build.BF3_PLAIN_SHAPES, ids=lambda s: "ppw%d_pxt%d_ks%d_wco%d_s%d" % s)
def test_every_split_product_launch_shape(amd, shape):
    """every IAF_BF3P entry: NT = 2, 4, 5 where the co tiling wastes at most a quarter of the conv's tiles and the form is compiled
    (NT = 5 is not at three co groups); at least one must launch"""
    ppw, pxt, ks, wco, _ = shape
    ran = []
    for n_out in SWEEP_WIDTHS:
        B, n_in, H, W, x, w, s, b, ref = _sweep_case(n_out)
        conv = amd.WNConv2d(n_in, n_out, theano=True)
        conv.set_precision("f32")
        conv.prepare(dev(w), dev(s), dev(b))
        err32 = np.abs(host(conv(dev(x))[0]) - ref).max()
        conv.set_precision("bf16x3")
        conv.prepare(dev(w), dev(s), dev(b), force=True)
        for nt in (2, 4, 5):
            tiles, per = n_out // 16, nt * wco
            if (-(-tiles // per) * per - tiles) * 4 > tiles or (nt == 5 and wco == 3):
                continue
            conv.set_tuning(-nt, ppw, wco, ks)
            assert conv.runs_bf16x3(B, H, W)
            err3 = np.abs(host(conv(dev(x))[0]) - ref).max()
            assert err3 <= ATOL and err3 <= 2 * err32 + 1e-6, (n_out, nt, err3, err32)
            ran.append((n_out, nt))
    print(shape, "launched", ran)
    assert ran, "no co-tile count of this shape launched"


# ---------------------------------------------------------------- 3. the batched prepare
def test_prep_batch_of_four_equals_four_single_prepares(amd):
    """the four convs of a layer (n_h 32, n_z 16) in one launch: every output bit for bit what four iaf_conv3x3_prepare calls give, on
    both families and in training mode (the data gradient reads the transposed packs)"""
    rng = np.random.RandomState(31)
    widths = [(32, 96), (32, 32), (32, 128), (48, 32)]
    params = [tuple(dev(a) for a in TR.rand_conv(rng, a, b)) for a, b in widths]
    B, H, W = 2, 3, 7
    xs = [dev(0.3 * rng.standard_normal((B, a, H, W))) for a, _ in widths]
    dys = [dev(rng.standard_normal((B, b, H, W))) for _, b in widths]

    def run(batched, prec):
        convs = [amd.WNConv2d(a, b, theano=True) for a, b in widths]
        for c in convs:
            c.set_precision(prec)
            c.set_training(True)
        if batched:
            amd.ConvPrepBatch(convs).run(params)
        else:
            for c, p in zip(convs, params):
                c.prepare(*p)
        out = []
        for c, p, x, dy, (a, b) in zip(convs, params, xs, dys, widths):
            if prec == "bf16x3" and a % 32 == 0:
                _pin_split(c, b)
            out.append(c(x)[0])
            dxs, dV, ds, db = c.backward(x, [dy], p[0], p[1])
            out += [dxs[0], dV, ds, db]
        return out

    for prec in ("f32", "bf16x3"):
        for i, (one, four) in enumerate(zip(run(False, prec), run(True, prec))):
            assert torch.equal(one, four), (prec, i)


# ---------------------------------------------------------------- 4. backward against fp64 autograd
@functools.lru_cache(maxsize=None)
def _bwd_case(n_in, n_out, c_split, B, H, W):
    rng = np.random.RandomState(300 + n_in + n_out + 11 * H + W + B)
    w, s, b = TR.rand_conv(rng, n_in, n_out)
    x = 0.3 * rng.standard_normal((B, n_in, H, W))
    dy = rng.standard_normal((B, n_out, H, W))
    x1, x2 = x[:, :c_split], x[:, c_split:]
    ref = TR.conv_grads(x1, w, s, b, dy, x2=x2, elu_input=True)
    return x1, x2, w, s, b, dy, ref


def _check_backward(amd, n_in, n_out, c_split, B, H, W, split, tol):
    x1, x2, w, s, b, dy, ref = _bwd_case(n_in, n_out, c_split, B, H, W)
    conv = amd.WNConv2d(n_in, n_out, theano=True)
    if not split:
        conv.set_precision("f32")
    conv.set_training(True)
    wd, sd, bd = dev(w), dev(s), dev(b)
    conv.prepare(wd, sd, bd)
    if split and B * H * W < 4096:
        conv.set_dgrad_tuning(2, 2, 1, 4)
    assert conv.dgrad_runs_bf16x3(B, H, W) == bool(split)
    y = conv(dev(x1), x2=dev(x2), elu_input=True)[0]
    np.testing.assert_allclose(host(y), ref["y"], atol=ATOL, rtol=0)
    # (dx_residual goes with a single dx tensor, iaf_conv3x3_backward's contract: test_backward_dx_residual_single_input)
    dxs, dV, ds, db = conv.backward(dev(x1), [dev(dy)], wd, sd, x2=dev(x2), elu_input=True)
    assert tuple(dV.shape) == (n_out, n_in + 1, 3, 3)
    errs = dict(dx2=_rel_err(host(dxs[1]), ref["dx2"]), dw=_rel_err(host(dV), ref["dw"]), ds=_rel_err(host(ds), ref["ds"]),
                db=_rel_err(host(db), ref["db"]), dw_border=_rel_err(host(dV)[:, n_in], ref["dw"][:, n_in]),
                dx=_rel_err(host(dxs[0]), ref["dx"]))
    print("%d->%d %dx%dx%d %s: %s" % (n_in, n_out, B, H, W, "split" if split else "exact", ", ".join("%s %.3g" % kv for kv in sorted(errs.items()))))
    for k, e in errs.items():
        assert e < tol, (k, e, tol)
    return conv, wd, sd


@pytest.mark.parametrize("geom", [(1, 1), (2, 2), (3, 7), (6, 5)], ids=lambda g: "%dx%d" % g)
def test_backward_vs_autograd_exact_family(amd, geom):
    """64 -> 32 with x2 at 32 and elu_input, B = 2: dx (both halves), dV (all n_in + 1 channels, the border channel also on its own), ds, db"""
    H, W = geom
    _check_backward(amd, 64, 32, 32, 2, H, W, False, 1e-4)


def test_backward_dx_residual_single_input(amd):
    """dx_residual (the `input + 0.1 h` path of the layer): one input, dy_scale 0.1, at 3x7"""
    B, n_in, n_out, H, W = 2, 32, 32, 3, 7
    rng = np.random.RandomState(77)
    w, s, b = TR.rand_conv(rng, n_in, n_out)
    x, dy = 0.3 * rng.standard_normal((B, n_in, H, W)), rng.standard_normal((B, n_out, H, W))
    ref = TR.conv_grads(x, w, s, b, dy, elu_input=True, residual=True)
    conv = amd.WNConv2d(n_in, n_out, theano=True)
    conv.set_precision("f32")
    conv.set_training(True)
    wd, sd = dev(w), dev(s)
    conv.prepare(wd, sd, dev(b))
    y = conv(dev(x), elu_input=True, residual=dev(x))[0]
    np.testing.assert_allclose(host(y), ref["y"], atol=ATOL, rtol=0)
    dxs, dV, ds, db = conv.backward(dev(x), [dev(dy)], wd, sd, elu_input=True, dy_scale=0.1, dx_residual=dev(dy))
    for name, got, want in (("dx", dxs[0], ref["dx"]), ("dw", dV, ref["dw"]), ("ds", ds, ref["ds"]), ("db", db, ref["db"])):
        e = _rel_err(host(got), want)
        print("residual form %s: %.3g" % (name, e))
        assert e < 1e-4, (name, e)


@pytest.mark.parametrize("case", [(2, 3, 7), (17, 16, 16)], ids=lambda c: "B%d_%dx%d" % c)
def test_backward_vs_autograd_data_gradient_on_the_split_products(amd, case):
    """the data gradient on the split products -- pinned at 3x7, by the size rule at 17 x 16x16 (4352 pixels) -- asserted with
    iaf_conv3x3_dgrad_runs_bf16x3; 2e-4 of the reference's largest entry"""
    B, H, W = case
    _check_backward(amd, 64, 32, 32, B, H, W, True, 2e-4)


# ---------------------------------------------------------------- 5. refusals
def test_refusals_the_header_lists(amd):
    """on an UNPREPARED conv: the kind is tested before anything else, so the answer is IAF_ERR_UNSUPPORTED, not 'not prepared'"""
    C = amd._capi
    lib, U = C.lib(), C.IAF_ERR_UNSUPPORTED
    h = ctypes.c_void_p()
    for n_in, n_out in ((6, 16), (16, 10), (272, 16)):
        assert lib.iaf_conv3x3_create_theano(ctypes.byref(h), n_in, n_out) == U and not h.value
    conv = amd.WNConv2d(32, 96, theano=True)
    ch = conv._h
    z = torch.zeros(1, 96, 2, 2, device="cuda")
    p = ctypes.c_void_p(z.data_ptr())
    outs, chans = (ctypes.c_void_p * 1)(z.data_ptr()), (ctypes.c_int * 1)(96)
    assert lib.iaf_conv3x3_set_precision(ch, C.IAF_PRECISION_F16X2) == U
    assert lib.iaf_conv3x3_set_packs(ch, C.IAF_PACK_F16X2) == U
    assert lib.iaf_conv3x3_runs_f16x2(ch, 32, 16, 16) == 0
    assert lib.iaf_conv3x3_prepare_deconv(ch, p, p, p, None) == U
    assert lib.iaf_conv3x3_forward_stride2(ch, p, 0, outs, chans, 1, 1, 1, 1, None) == U
    assert lib.iaf_conv3x3_forward_deconv(ch, p, None, 0, 0, None, p, 1, 1, 1, None) == U
    assert lib.iaf_conv3x3_forward_prior_sample(ch, p, 1, 16, 16, p, p, p, 1, 2, 2, None) == U
    assert lib.iaf_conv3x3_forward_hdet(ch, p, 1, 16, 16, p, 1, 2, 2, None) == U
    sh, us = (ctypes.c_int * 4)(), ctypes.c_float()
    assert lib.iaf_conv3x3_autotune(ch, p, None, 0, 0, None, outs, chans, 1, 1, 2, 2, 1, None, sh, ctypes.byref(us)) == U
    conv.set_training(True)
    assert lib.iaf_conv3x3_set_defer_weightnorm(ch, 1) == U
    arr, hb = (ctypes.c_void_p * 1)(ch.value), ctypes.c_void_p()
    assert lib.iaf_conv3x3_wn_bwd_batch_create(ctypes.byref(hb), arr, 1) == U and not hb.value
    assert lib.iaf_conv3x3_autotune_backward(ch, p, None, 0, 0, outs, chans, 1, 1.0, outs, chans, 1, None, p, p, p, p, p, 1, 2, 2, p, 0, 1,
                                             None, sh, ctypes.byref(us)) == U
    # what stays allowed
    conv.set_precision("bf16x3")
    conv.set_precision("f32")
    with pytest.raises(ValueError):
        conv.prepare(torch.zeros(3, 3, 32, 96, device="cuda"), torch.zeros(96, device="cuda"), torch.zeros(96, device="cuda"))
    # the mirror of N.conv.conv2d gives what the direct calls give
    rng = np.random.RandomState(5)
    w, s, b = TR.rand_conv(rng, 32, 96)
    wd = {"c_w": dev(w), "c_s": dev(s), "c_b": dev(b)}
    x = dev(0.3 * rng.standard_normal((2, 32, 3, 7)))
    f = amd.conv2d_theano("c", 32, 96, w=wd)
    ref = TR.conv2d(TR.t64(host(x)), TR.t64(w), TR.t64(s), TR.t64(b)).numpy()
    np.testing.assert_allclose(host(f(x, wd)), ref, atol=ATOL, rtol=0)


# ---------------------------------------------------------------- 6. the TF plain conv is what it was
def test_tf_plain_conv_is_bit_identical_before_and_after_a_theano_conv_ran(amd):
    import golden_inputs as gi
    rng = np.random.RandomState(91)
    B, n_in, n_out, H, W = 2, 32, 96, 3, 7
    p = gi.conv_params(rng, n_in, n_out)
    x, dy = rng.standard_normal((B, n_in, H, W)), rng.standard_normal((B, n_out, H, W))

    def tf():
        out = []
        for prec in ("f32", "bf16x3"):
            conv = amd.WNConv2d(n_in, n_out)
            conv.set_precision(prec)
            conv.set_training(True)
            V, g = dev(p["V"]), dev(p["g"])
            conv.prepare(V, g, dev(p["b"]))
            if prec == "bf16x3":
                conv.set_tuning(-2, 2, 1, 4)
            out.append(conv(dev(x), elu_input=True)[0].clone())
            dxs, dV, dg, db = conv.backward(dev(x), [dev(dy)], V, g, elu_input=True)
            out += [dxs[0].clone(), dV.clone(), dg.clone(), db.clone()]
        return out

    before = tf()
    w, s, b = TR.rand_conv(rng, n_in, n_out)
    th = amd.WNConv2d(n_in, n_out, theano=True)
    th.set_training(True)
    wd, sd = dev(w), dev(s)
    th.prepare(wd, sd, dev(b))
    th(dev(x))
    th.backward(dev(x), [dev(dy)], wd, sd)
    torch.cuda.synchronize()
    for i, (a, c) in enumerate(zip(before, tf())):
        assert torch.equal(a, c), i
