"""GPU tests of prior 'made' of iaf_amd.CVAELayerIAF (models.py:36-38, 304-309, 330-359) with the posteriors 'down_iaf2_nl' and
'down_iaf2_nl2', and of the six elementwise entry points around the steps (iaf_made_head / _tail / _backward_pre / _backward_join /
_backward_post, iaf_diag_prior_sample): the reference's own outputs (tests/golden/theano_cvae_layer_made.npz), the entry points one by one
against their NumPy contracts at sizes where the indexing can go wrong, the backward pass against fp64 autograd, training forward against
evaluation forward, captured down_q / down_p against the eager ones, and the ancestral sampler of down_p(exact=True) against the
sequential fp64 sampler.  References: tests/made_reference.py."""
import os

import numpy as np
import pytest
import torch

import made_reference as MR
import make_golden_made as MGM
from oracle import iaf_oracle as O

pytestmark = pytest.mark.gpu

ATOL = 1e-4
SENTINEL = 12345.0


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


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _rel_close(got, ref, tol, name):
    scale = max(np.abs(ref).max(), 1e-6)
    err = np.abs(got - ref).max() / scale
    print("%s: max err / max|ref| = %.3g (tol %g)" % (name, err, tol))
    assert err < tol, "%s: max err / max|ref| = %.3g (tol %g)" % (name, err, tol)


_elu = lambda t: np.where(t < 0, np.exp(np.minimum(t, 0)) - 1, t)


# ---------------------------------------------------------------- the reference's own outputs
@pytest.mark.parametrize("cname", MGM.MADE_CASES)
def test_made_layer_vs_reference_golden(amd, golden_dir, cname):
    """models.cvae_layer(..., 'made', posterior, ...) through iaf_amd.CVAELayerIAF: the plain Theano convs come from the NumPy statement
    (out of scope), the steps, the prior's density and the free bits run on the GPU; tolerances of test_chain_layer_vs_reference_golden.
    down_p(exact=False) is what the reference runs (z = eps)."""
    B, n_h, n_z, depth_ar, H, W, kl_min, posterior, prior = MGM.CASES[cname]
    g = np.load(os.path.join(golden_dir, MGM.FIXTURE))
    c = MGM.fixture_case(g, cname)
    w32 = {k: f32(v) for k, v in c["w"].items()}
    cw = lambda nm: (w32["1" + nm + "_w"], w32["1" + nm + "_b"], w32["1" + nm + "_s"])
    up_conv1 = O.theano_conv2d(_elu(f32(c["up_input"])), *cw("_up_conv1_1"))
    down_conv1 = O.theano_conv2d(_elu(f32(c["down_input"])), *cw("_down_conv1"))
    assert down_conv1.shape[1] == 3 * n_h + 2 * n_z
    layer = amd.CVAELayerIAF("1", n_h, n_z, depth_ar, posterior=posterior, kl_min=kl_min, prior="made")
    layer.load({k: dev(v) for k, v in c["w"].items()})
    hu = layer.up(dev(up_conv1), eps=dev(c["eps_up"]))
    up_out = f32(c["up_input"]) + 0.1 * O.theano_conv2d(_elu(host(hu)), *cw("_up_conv2"))
    np.testing.assert_allclose(up_out, g[cname + "/up_out"], atol=ATOL, rtol=0)
    d = layer.down_q(dev(down_conv1), eps=dev(c["eps_down"]))
    for k in ("kl", "kl_sum", "obj_kl"):
        print("%s %s: max abs err %.3g, max |ref| %.3g" % (cname, k, np.abs(host(d[k]) - g[cname + "/" + k]).max(), np.abs(g[cname + "/" + k]).max()))
    np.testing.assert_allclose(host(d["kl"]), g[cname + "/kl"], atol=ATOL, rtol=1e-5)
    np.testing.assert_allclose(host(d["kl_sum"]), g[cname + "/kl_sum"], atol=2e-3, rtol=1e-4)
    np.testing.assert_allclose(host(d["obj_kl"]), g[cname + "/obj_kl"], atol=2e-3, rtol=1e-4)
    down_out = f32(c["down_input"]) + 0.1 * O.theano_conv2d(_elu(host(d["h"])), *cw("_down_conv2_1"))
    np.testing.assert_allclose(down_out, g[cname + "/down_out"], atol=ATOL, rtol=0)
    assert torch.equal(d["h"][:, n_h:], d["z"])
    hp = layer.down_p(dev(down_conv1), dev(c["eps_p"]), exact=False)
    assert torch.equal(hp[:, n_h:], dev(c["eps_p"])) and torch.equal(hp[:, :n_h], dev(down_conv1)[:, :n_h])
    p_out = f32(c["down_input"]) + 0.1 * O.theano_conv2d(_elu(host(hp)), *cw("_down_conv2_1"))
    np.testing.assert_allclose(p_out, g[cname + "/down_p_out"], atol=ATOL, rtol=0)


def test_diag_down_p_vs_reference_golden(amd, golden_dir):
    """down_p with the diag prior (models.py:334-337) against the reference's output"""
    cname = "diag_p"
    B, n_h, n_z, depth_ar, H, W, kl_min, posterior, prior = MGM.CASES[cname]
    g = np.load(os.path.join(golden_dir, MGM.FIXTURE))
    c = MGM.fixture_case(g, cname)
    w32 = {k: f32(v) for k, v in c["w"].items()}
    cw = lambda nm: (w32["1" + nm + "_w"], w32["1" + nm + "_b"], w32["1" + nm + "_s"])
    down_conv1 = O.theano_conv2d(_elu(f32(c["down_input"])), *cw("_down_conv1"))
    layer = amd.CVAELayerIAF("1", n_h, n_z, depth_ar, posterior=posterior, kl_min=kl_min)
    assert layer.prior == "diag" and layer.prior_stack is None
    layer.load({k: dev(v) for k, v in c["w"].items()})
    hp = layer.down_p(dev(down_conv1), dev(c["eps_p"]))
    p_out = f32(c["down_input"]) + 0.1 * O.theano_conv2d(_elu(host(hp)), *cw("_down_conv2_1"))
    np.testing.assert_allclose(p_out, g[cname + "/down_p_out"], atol=ATOL, rtol=0)
    with pytest.raises(ValueError, match="depth_ar"):
        amd.CVAELayerIAF("1", n_h, n_z, 0, prior="made")


# ---------------------------------------------------------------- the six entry points, one by one
# B, n_h, n_z, HW: HW in {1, 30, 64}, n_z in {4, 32}, n_h in {8, 64}, B in {1, 3}; 64 is the 16-byte form
LEAF_SHAPES = [(3, 8, 4, 1), (1, 64, 4, 30), (3, 8, 32, 30), (1, 8, 32, 64), (3, 64, 4, 64)]
# Every output is a copy, a sum of two or three operands of order one, or a short fp32 expression (exp of a quarter-scale logsd times a
# standard normal; (log 2pi)/2 + s_p + u^2/2 with u^2/2 below ~40, asserted below): a few ulp of the largest term, 40 * 6e-8 = 2.4e-6
# each, lie an order below this bound.  The reference's own fp64 value of the contract is all the tests measure.
LEAF_TOL = 2e-5


def _leaf_inputs(seed, B, n_h, n_z, HW):
    rng = np.random.RandomState(seed)
    up, down = rng.standard_normal((B, 2 * n_h + 2 * n_z, HW)), rng.standard_normal((B, 3 * n_h + 2 * n_z, HW))
    up[:, n_h:n_h + n_z] *= 0.5
    up[:, n_h + n_z:n_h + 2 * n_z] *= 0.25
    down[:, 2 * n_h:2 * n_h + n_z] *= 0.5
    down[:, 2 * n_h + n_z:2 * n_h + 2 * n_z] *= 0.25
    f = lambda c, s=1.0: s * rng.standard_normal((B, c, HW))
    x = dict(up=up, down=down, eps=f(n_z), s1=f(n_z, 0.3), s2=f(n_z, 0.3), s_p=f(n_z, 0.3), z=f(n_z, 0.5), u=f(n_z), d_h=f(n_h + n_z),
             d_up=f(n_h), dz0=f(n_z), dz_p=f(n_z), d_mctx=f(n_h), dctx1=f(n_h), dctx2=f(n_h),
             gate=(rng.uniform(size=n_z) > 0.4).astype(np.float64), dko=rng.uniform(0.2, 1.0, size=B))
    assert 0.5 * (x["u"] ** 2).max() < 40.0
    return x


def _misaligned(a):
    """the same values in a contiguous tensor whose address is 4 bytes past a 16-byte boundary"""
    flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    t = flat[1:].view(a.shape)
    t.copy_(dev(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _full(*shape):
    return torch.full(shape, SENTINEL, device="cuda")


_ids = lambda s: "B%d_h%d_z%d_hw%d" % s
HEAD_TAIL_CASES = [(s, False) for s in LEAF_SHAPES] + [((1, 8, 32, 64), True)]


@pytest.mark.parametrize("two_flows", [True, False], ids=["s2", "s2_null"])
@pytest.mark.parametrize("shape,misalign", HEAD_TAIL_CASES, ids=[_ids(s) + ("_off_by_4_bytes" if m else "") for s, m in HEAD_TAIL_CASES])
def test_made_head_and_tail_vs_numpy(amd, shape, misalign, two_flows):
    """iaf_made_head and iaf_made_tail (with kl, and as the pack alone) against head_np / tail_np; `misalign`: one operand 4 bytes off a
    16-byte boundary, so that the 16-byte form must not be chosen at HW = 64 either"""
    from iaf_amd import _capi
    from iaf_amd.layers import _ptr, _stream
    B, n_h, n_z, HW = shape
    x = _leaf_inputs(100 + HW + n_h, *shape)
    up, down = dev(x["up"]), dev(x["down"])
    eps = _misaligned(x["eps"]) if misalign else dev(x["eps"])
    z0, logq0, context, mctx = _full(B, n_z, HW), _full(B, n_z, HW), _full(B, n_h, HW), _full(B, n_h, HW)
    _capi.check(_capi.lib().iaf_made_head(_ptr(up), _ptr(down), _ptr(eps), _ptr(z0), _ptr(logq0), _ptr(context), _ptr(mctx), B, n_h, n_z, HW,
                                          _stream()))
    ez0, elq, ectx, emctx = MR.head_np(f32(x["up"]), f32(x["down"]), f32(x["eps"]), n_h, n_z)
    np.testing.assert_allclose(host(z0), ez0, atol=LEAF_TOL, rtol=0)
    np.testing.assert_allclose(host(logq0), elq, atol=LEAF_TOL, rtol=0)
    np.testing.assert_allclose(host(context), ectx, atol=LEAF_TOL, rtol=0)
    np.testing.assert_array_equal(host(mctx), emctx)                                 # a copy: exact
    s1 = _misaligned(x["s1"]) if misalign else dev(x["s1"])
    s2 = dev(x["s2"]) if two_flows else None
    z, u, s_p = dev(x["z"]), dev(x["u"]), dev(x["s_p"])
    kl, h_out = _full(B, n_z, HW), _full(B, n_h + n_z, HW)
    _capi.check(_capi.lib().iaf_made_tail(_ptr(down), _ptr(logq0), _ptr(s1), _ptr(s2), _ptr(z), _ptr(u), _ptr(s_p), _ptr(kl), _ptr(h_out), B,
                                          n_h, n_z, HW, _stream()))
    ekl, eh = MR.tail_np(f32(x["down"]), host(logq0), f32(x["s1"]), f32(x["s2"]) if two_flows else None, f32(x["z"]), f32(x["u"]),
                         f32(x["s_p"]), n_h, n_z)
    np.testing.assert_allclose(host(kl), ekl, atol=LEAF_TOL, rtol=0)
    np.testing.assert_array_equal(host(h_out), eh)                                   # copies: exact
    zp = _misaligned(x["eps"]) if misalign else dev(x["eps"])                         # the pack alone, as down_p calls it
    h_p = _full(B, n_h + n_z, HW)
    _capi.check(_capi.lib().iaf_made_tail(_ptr(down), None, None, None, _ptr(zp), None, None, None, _ptr(h_p), B, n_h, n_z, HW, _stream()))
    np.testing.assert_array_equal(host(h_p), np.concatenate([f32(x["down"])[:, :n_h], f32(x["eps"])], axis=1))
    for t in (up, down):                                                             # the conv outputs are read only
        assert torch.equal(t, dev(x["up"] if t is up else x["down"]))


BWD_CASES = [(s, False) for s in LEAF_SHAPES] + [((1, 8, 32, 64), True)]


@pytest.mark.parametrize("with_up,two_flows", [(True, True), (False, False), (True, False), (False, True)],
                         ids=["d_up_dctx2", "d_up_null_dctx2_null", "d_up_dctx2_null", "d_up_null_dctx2"])
@pytest.mark.parametrize("free_bits", [True, False], ids=["gate", "dko"])
@pytest.mark.parametrize("shape,misalign", BWD_CASES, ids=[_ids(s) + ("_off_by_4_bytes" if m else "") for s, m in BWD_CASES])
def test_made_backward_pre_join_and_post_vs_numpy(amd, shape, misalign, free_bits, with_up, two_flows):
    """iaf_made_backward_pre / _join / _post against pre_np / join_np / post_np; d_down_conv1 starts as a sentinel: pre writes its first
    n_h channels, join the next n_h, post the rest, and each leaves the others' channels as it found them, bit for bit"""
    from iaf_amd import _capi
    from iaf_amd.layers import _ptr, _stream
    B, n_h, n_z, HW = shape
    x = _leaf_inputs(200 + HW + n_h, *shape)
    lib = _capi.lib()
    up, down, d_h = dev(x["up"]), dev(x["down"]), dev(x["d_h"])
    u = _misaligned(x["u"]) if misalign else dev(x["u"])
    gate, gscale, dko = (dev(x["gate"]), 0.7 / B, None) if free_bits else (None, 0.0, dev(x["dko"]))
    du, G, dz = _full(B, n_z, HW), _full(B, n_z, HW), _full(B, n_z, HW)
    d_dc1 = _full(B, 3 * n_h + 2 * n_z, HW)
    _capi.check(lib.iaf_made_backward_pre(_ptr(u), _ptr(d_h), _ptr(gate), gscale, _ptr(dko), _ptr(du), _ptr(G), _ptr(d_dc1), B, n_h, n_z, HW,
                                          _stream()))
    gs32 = float(np.float32(gscale))
    edu, eG, efirst = MR.pre_np(f32(x["u"]), f32(x["d_h"]), n_h, n_z, x["gate"] if free_bits else None, gs32,
                                None if free_bits else f32(x["dko"]))
    np.testing.assert_allclose(host(du), edu, atol=LEAF_TOL, rtol=0)
    np.testing.assert_allclose(host(G), eG, atol=1e-6, rtol=0)
    np.testing.assert_array_equal(host(d_dc1[:, :n_h]), efirst)
    assert bool((d_dc1[:, n_h:] == SENTINEL).all()), "pre wrote outside its channels"
    after_pre = d_dc1.clone()
    dz_p = _misaligned(x["dz_p"]) if misalign else dev(x["dz_p"])
    d_mctx = dev(x["d_mctx"])
    _capi.check(lib.iaf_made_backward_join(_ptr(d_h), _ptr(dz_p), _ptr(d_mctx), _ptr(dz), _ptr(d_dc1), B, n_h, n_z, HW, _stream()))
    edz, emid = MR.join_np(f32(x["d_h"]), f32(x["dz_p"]), f32(x["d_mctx"]), n_h, n_z)
    np.testing.assert_allclose(host(dz), edz, atol=LEAF_TOL, rtol=0)
    np.testing.assert_array_equal(host(d_dc1[:, n_h:2 * n_h]), emid)
    assert torch.equal(d_dc1[:, :n_h], after_pre[:, :n_h]) and bool((d_dc1[:, 2 * n_h:] == SENTINEL).all()), "join wrote outside its channels"
    after_join = d_dc1.clone()
    z0 = dev(MR.head_np(f32(x["up"]), f32(x["down"]), f32(x["eps"]), n_h, n_z)[0])
    dz0 = _misaligned(x["dz0"]) if misalign else dev(x["dz0"])
    dctx1, dctx2 = dev(x["dctx1"]), (dev(x["dctx2"]) if two_flows else None)
    d_up = dev(x["d_up"]) if with_up else None
    d_uc1 = _full(B, 2 * n_h + 2 * n_z, HW)
    _capi.check(lib.iaf_made_backward_post(_ptr(up), _ptr(down), _ptr(z0), _ptr(dz0), _ptr(G), _ptr(dctx1), _ptr(dctx2), _ptr(d_up),
                                           _ptr(d_uc1), _ptr(d_dc1), B, n_h, n_z, HW, _stream()))
    e_uc1, e_rest = MR.post_np(f32(x["up"]), f32(x["down"]), host(z0), f32(x["dz0"]), host(G), f32(x["dctx1"]),
                               f32(x["dctx2"]) if two_flows else None, f32(x["d_up"]) if with_up else None, n_h, n_z)
    np.testing.assert_allclose(host(d_uc1), e_uc1, atol=LEAF_TOL, rtol=0)
    np.testing.assert_allclose(host(d_dc1[:, 2 * n_h:]), e_rest, atol=LEAF_TOL, rtol=0)
    assert torch.equal(d_dc1[:, :2 * n_h], after_join[:, :2 * n_h]), "post wrote outside its channels"
    assert torch.equal(d_uc1[:, n_h:], d_dc1[:, 2 * n_h:])                           # the q and the r channels get the same gradient


@pytest.mark.parametrize("extra", [0, 1], ids=["layout_up_iaf2_nl", "layout_down_iaf2_nl"])
@pytest.mark.parametrize("shape,misalign", HEAD_TAIL_CASES, ids=[_ids(s) + ("_off_by_4_bytes" if m else "") for s, m in HEAD_TAIL_CASES])
def test_diag_prior_sample_vs_numpy(amd, shape, misalign, extra):
    """iaf_diag_prior_sample against diag_sample_np on both diag layouts of down_conv1 (n_h + 2 n_z and 2 n_h + 4 n_z channels)"""
    from iaf_amd import _capi
    from iaf_amd.layers import _ptr, _stream
    B, n_h, n_z, HW = shape
    n_down = n_h + 2 * n_z + extra * (n_h + 2 * n_z)
    rng = np.random.RandomState(300 + HW + n_h)
    down, eps_np = rng.standard_normal((B, n_down, HW)), rng.standard_normal((B, n_z, HW))
    down[:, n_h + n_z:n_h + 2 * n_z] *= 0.25
    eps = _misaligned(eps_np) if misalign else dev(eps_np)
    h_out = _full(B, n_h + n_z, HW)
    _capi.check(_capi.lib().iaf_diag_prior_sample(_ptr(dev(down)), _ptr(eps), _ptr(h_out), B, n_down, n_h, n_z, HW, _stream()))
    e = MR.diag_sample_np(f32(down), f32(eps_np), n_h, n_z)
    np.testing.assert_array_equal(host(h_out[:, :n_h]), e[:, :n_h])
    np.testing.assert_allclose(host(h_out), e, atol=LEAF_TOL, rtol=0)


# ---------------------------------------------------------------- the layer: backward, training forward, capture
def _layer_case(seed, B, n_h, n_z, d, H, W, posterior):
    rng = np.random.RandomState(seed)
    w = MR.rand_params(rng, "1", n_z, [n_h] * d, posterior)
    h_up, h_dn = MR.rand_conv_outputs(rng, B, n_h, n_z, H, W)
    eps = rng.standard_normal((B, n_z, H, W))
    d_up, d_h = rng.standard_normal((B, n_h, H, W)), rng.standard_normal((B, n_h + n_z, H, W))
    return w, h_up, h_dn, eps, d_up, d_h, rng


def _backward_reference(shape, posterior, kl_min, with_up):
    """the case and its fp64 autograd reference"""
    B, n_h, n_z, d, H, W = shape
    w, h_up, h_dn, eps, d_up, d_h, rng = _layer_case(5 + int(kl_min * 8) + H + (posterior == "down_iaf2_nl2"), *shape, posterior)
    d_obj = np.asarray(0.7) if kl_min > 0 else rng.standard_normal(B)
    ref, fw = MR.made_iaf_grads(f32(h_up), f32(h_dn), f32(eps), {k: f32(v) for k, v in w.items()}, "1", n_h, n_z, d, posterior, kl_min,
                                f32(d_up) if with_up else None, f32(d_h), f32(d_obj))
    return w, h_up, h_dn, eps, d_up, d_h, d_obj, ref, fw


# B, n_h, n_z, depth_ar, H, W of the three fixture cases
BWD_SHAPES = [(3, 32, 16, 2, 6, 5), (2, 64, 32, 2, 8, 8), (2, 32, 32, 1, 3, 7)]


@pytest.mark.parametrize("with_up", [True, False], ids=["d_up", "d_up_none"])
@pytest.mark.parametrize("kl_min", [0.0, 0.25])
@pytest.mark.parametrize("posterior", ["down_iaf2_nl", "down_iaf2_nl2"])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "B%d_h%d_z%d_d%d_%dx%d" % s)
def test_made_layer_backward_vs_autograd(amd, shape, posterior, kl_min, with_up):
    """training with the MADE prior: gradients of both conv outputs (reference channel order) and of every weight of ALL stacks (one or
    two posterior stacks and the prior's), incl. the scalar free-bits objective, against torch-fp64 autograd of the restated forward
    (logps the reference's way).  The criterion: 1e-4 of the reference's largest entry, on the conv-output gradients and on every
    weight gradient of all stacks."""
    B, n_h, n_z, d, H, W = shape
    w, h_up, h_dn, eps, d_up, d_h, d_obj, ref, fw = _backward_reference(shape, posterior, kl_min, with_up)
    layer = amd.CVAELayerIAF("1", n_h, n_z, d, posterior=posterior, kl_min=kl_min, prior="made")
    layer.set_training(True)
    layer.load({k: dev(v) for k, v in w.items()})
    up_out = layer.up(dev(h_up))
    dq = layer.down_q(dev(h_dn), eps=dev(eps))
    bw = layer.backward(dev(d_h), d_obj=(0.7 if kl_min > 0 else dev(d_obj)), d_up=dev(d_up) if with_up else None)
    np.testing.assert_allclose(host(up_out), fw["up_out"], atol=0, rtol=0)
    np.testing.assert_allclose(host(dq["h"]), fw["h"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(dq["kl"]), fw["kl"], atol=ATOL, rtol=1e-5)
    np.testing.assert_allclose(host(dq["obj_kl"]), fw["obj_kl"], atol=2e-3, rtol=1e-4)
    assert tuple(bw["d_up_conv1"].shape) == (B, 2 * n_h + 2 * n_z, H, W) and tuple(bw["d_down_conv1"].shape) == (B, 3 * n_h + 2 * n_z, H, W)
    if not with_up:
        assert not bw["d_up_conv1"][:, :n_h].any()
    _rel_close(host(bw["d_up_conv1"]), ref["h_up"], 1e-4, "d_up_conv1")
    _rel_close(host(bw["d_down_conv1"]), ref["h_dn"], 1e-4, "d_down_conv1")
    assert set(bw["grads"]) == set(w)
    assert any(k.startswith("1_prior_conv1_") for k in w)
    assert any(k.startswith("1_posterior_conv2_") for k in w) == (posterior == "down_iaf2_nl2")
    for k in sorted(w):
        _rel_close(host(bw["grads"][k]), ref["w"][k], 1e-4, k)


@pytest.mark.parametrize("kl_min", [0.0, 0.25])
def test_made_layer_on_embedded_stacks_vs_autograd(amd, kl_min):
    """n_z = 4, n_h = 8: both stacks run embedded in stacks four times as wide (EmbeddedTheanoStack, iaf_amd/layers.py); forward and
    every gradient against fp64 autograd at the bounds of test_made_layer_backward_vs_autograd.  An embedded stack is a wrapper of its
    own with the narrow sizes, not an ARStack with the wide handle; a bare ARStack and the flipped ordering still refuse these sizes."""
    shape = (2, 8, 4, 2, 3, 2)
    B, n_h, n_z, d, H, W = shape
    w, h_up, h_dn, eps, d_up, d_h, d_obj, ref, fw = _backward_reference(shape, "down_iaf2_nl", kl_min, True)
    layer = amd.CVAELayerIAF("1", n_h, n_z, d, posterior="down_iaf2_nl", kl_min=kl_min, prior="made")
    layer.set_training(True)
    layer.load({k: dev(v) for k, v in w.items()})
    layer.up(dev(h_up))
    dq = layer.down_q(dev(h_dn), eps=dev(eps))
    bw = layer.backward(dev(d_h), d_obj=(0.7 if kl_min > 0 else dev(d_obj)), d_up=dev(d_up))
    np.testing.assert_allclose(host(dq["h"]), fw["h"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(dq["kl"]), fw["kl"], atol=ATOL, rtol=1e-5)
    np.testing.assert_allclose(host(dq["obj_kl"]), fw["obj_kl"], atol=2e-3, rtol=1e-4)
    _rel_close(host(bw["d_up_conv1"]), ref["h_up"], 1e-4, "d_up_conv1")
    _rel_close(host(bw["d_down_conv1"]), ref["h_dn"], 1e-4, "d_down_conv1")
    assert set(bw["grads"]) == set(w)
    for k in sorted(w):
        assert tuple(bw["grads"][k].shape) == w[k].shape, k
        _rel_close(host(bw["grads"][k]), ref["w"][k], 1e-4, k)
    from iaf_amd.layers import ARStack, EmbeddedTheanoStack
    for st in (layer.stack, layer.prior_stack):
        assert isinstance(st, EmbeddedTheanoStack) and not isinstance(st, ARStack)
        assert (st.n_z, st.n_h, st.t) == (n_z, n_h, 4) and (st.wide.n_z, st.wide.n_h) == (16, 32)
        assert not hasattr(st, "posterior_block") and not hasattr(st, "workspace") and not hasattr(st, "set_tuning")
    with pytest.raises(amd._capi.UnsupportedError):                 # a bare stack of these sizes is refused, as it always was
        ARStack(n_z, [n_h] * d, variant="theano")
    with pytest.raises(amd._capi.UnsupportedError):                 # the flipped ordering is not embedded
        amd.CVAELayerIAF("1", n_h, n_z, d, posterior="down_iaf2_nl2", prior="made")


@pytest.mark.parametrize("posterior", ["down_iaf2_nl", "down_iaf2_nl2"])
def test_made_training_forward_equals_evaluation_forward(amd, posterior):
    B, n_h, n_z, d, H, W = 3, 64, 32, 2, 8, 8
    w, h_up, h_dn, eps, _, _, _ = _layer_case(31, B, n_h, n_z, d, H, W, posterior)
    wd = {k: dev(v) for k, v in w.items()}
    outs = []
    for training in (False, True):
        layer = amd.CVAELayerIAF("1", n_h, n_z, d, posterior=posterior, kl_min=0.25, prior="made")
        layer.set_training(training)
        layer.load(wd)
        hu = layer.up(dev(h_up))
        assert torch.equal(hu, dev(h_up)[:, :n_h])
        outs.append(layer.down_q(dev(h_dn), eps=dev(eps)))
    ev, tr = outs
    assert set(tr) == set(ev) == {"h", "z", "kl", "kl_sum", "obj_kl"}
    np.testing.assert_allclose(host(tr["h"]), host(ev["h"]), atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(tr["z"]), host(ev["z"]), atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(tr["kl"]), host(ev["kl"]), atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(tr["kl_sum"]), host(ev["kl_sum"]), atol=2e-3, rtol=1e-4)      # sums of B n_z H W / B terms: the sums' tolerance
    np.testing.assert_allclose(host(tr["obj_kl"]), host(ev["obj_kl"]), atol=2e-3, rtol=1e-4)
    assert tr["obj_kl"].dim() == 0


def test_made_down_q_and_down_p_captured_in_a_graph_equal_eager(amd):
    """down_q and down_p(exact=True) launch on the current stream only: captured after a warm-up on the capturing stream, replayed twice
    with new noise written into the captured buffer, they give what the eager calls give, bit for bit"""
    B, n_h, n_z, d, H, W = 2, 32, 16, 2, 6, 5
    w, h_up, h_dn, eps, _, _, rng = _layer_case(41, B, n_h, n_z, d, H, W, "down_iaf2_nl2")
    layer = amd.CVAELayerIAF("1", n_h, n_z, d, posterior="down_iaf2_nl2", kl_min=0.25, prior="made")
    layer.load({k: dev(v) for k, v in w.items()})
    t_up, t_dn, eps_buf = dev(h_up), dev(h_dn), dev(eps)
    stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    keys = ("h", "z", "kl", "kl_sum", "obj_kl")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = []
    with torch.cuda.stream(s):
        layer.up(t_up)
        layer.down_q(t_dn, eps=eps_buf)                             # warm-up: workspaces exist before the capture
        layer.down_p(t_dn, eps_buf, stats=stats)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = layer.down_q(t_dn, eps=eps_buf)
            out_p = layer.down_p(t_dn, eps_buf, stats=stats)
        noises = [rng.standard_normal((B, n_z, H, W)) for _ in range(2)]
        for e in noises:
            eps_buf.copy_(dev(e))
            g.replay()
            s.synchronize()
            got.append(dict({k: out[k].clone() for k in keys}, p=out_p.clone(), stats=stats.clone()))
        s.synchronize()
    torch.cuda.synchronize()
    assert not torch.equal(got[0]["z"], got[1]["z"]) and not torch.equal(got[0]["p"], got[1]["p"])
    for e, gk in zip(noises, got):
        eager = layer.down_q(t_dn, eps=dev(e))
        for k in keys:
            assert torch.equal(eager[k], gk[k]), k
        st2 = torch.zeros(2, dtype=torch.int32, device="cuda")
        assert torch.equal(layer.down_p(t_dn, dev(e), stats=st2), gk["p"])
        assert torch.equal(st2, gk["stats"]) and int(st2[0]) > 0


# ---------------------------------------------------------------- the sampler
def _stats(t):
    sweeps, bits = (int(v) for v in t.cpu().numpy())
    return sweeps, float(np.array([bits], dtype=np.int32).view(np.float32)[0])


# B, n_z, n_h, depth_ar, H, W.  tiny_2x2 is the geometry of test_inverse_flow_is_exact_after_one_sweep_per_position.  The engine states
# the Theano operator for channel counts that are multiples of 16 only, so at n_z = 4, n_h = 8 the layer runs the stack embedded in one
# four times as wide (EmbeddedTheanoStack, iaf_amd/layers.py); tiny_2x2_z16 is the smallest geometry that needs no embedding: H W n_z = 64 sweeps.
TINY = {"tiny_2x2": (2, 4, 8, 2, 2, 2), "tiny_2x2_z16": (2, 16, 16, 2, 2, 2)}


def _sampler_case(name, golden_dir):
    """(n_h, n_z, depth_ar, weights, down_conv1 output, eps) of a fixture case, or of a 2x2 case at the fixture's weight scale"""
    if name in TINY:
        B, n_z, n_h, d, H, W = TINY[name]
        rng = np.random.RandomState(51)
        w = MR.rand_params(rng, "1", n_z, [n_h] * d, "down_iaf2_nl")
        return n_h, n_z, d, w, MR.rand_conv_outputs(rng, B, n_h, n_z, H, W)[1], rng.standard_normal((B, n_z, H, W))
    B, n_h, n_z, d, H, W = MGM.CASES[name][:6]
    g = np.load(os.path.join(golden_dir, MGM.FIXTURE))
    c = MGM.fixture_case(g, name)
    w32 = {k: f32(v) for k, v in c["w"].items()}
    down_conv1 = O.theano_conv2d(_elu(f32(c["down_input"])), w32["1_down_conv1_w"], w32["1_down_conv1_b"], w32["1_down_conv1_s"])
    return n_h, n_z, d, c["w"], down_conv1, c["eps_p"]


@pytest.mark.parametrize("name", ["made_small", "made_64", "tiny_2x2", "tiny_2x2_z16"])
def test_made_down_p_exact_is_the_ancestral_sample(amd, golden_dir, name):
    """down_p(exact=True): the prior's step at the sample gives eps back within 2e-5, the residual is <= tol and the sweep count below 60
    (the bounds test_inverse_flow_round_trip holds the same solver to); the sample equals the sequential fp64 sampler within 1e-4; and it
    is not the reference's placeholder z = eps.  On the 2x2 cases, tol = 0 and H W n_z sweeps give the exact sample too."""
    n_h, n_z, d, w, down_conv1, eps = _sampler_case(name, golden_dir)
    B, _, H, W = eps.shape
    layer = amd.CVAELayerIAF("1", n_h, n_z, d, posterior="down_iaf2_nl", prior="made")
    layer.load({k: dev(v) for k, v in w.items() if "_prior_conv1_" in k or "_posterior_conv1_" in k})
    stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    t_dn, t_eps = dev(down_conv1), dev(eps)
    h = layer.down_p(t_dn, t_eps, max_sweeps=200, tol=1e-6, check_every=2, stats=stats)
    sweeps, res = _stats(stats)
    print("%s: %d sweeps, residual %.3g" % (name, sweeps, res))
    assert res <= 1e-6 and 0 < sweeps < 60, (sweeps, res)
    assert torch.equal(h[:, :n_h], t_dn[:, :n_h])
    z = h[:, n_h:].contiguous()
    mctx = t_dn[:, n_h:2 * n_h].contiguous()
    np.testing.assert_allclose(host(layer.prior_stack.iaf_step(z, mctx)[0]), f32(eps), atol=2e-5, rtol=0)
    ref = MR.sample_exact(f32(down_conv1)[:, n_h:2 * n_h], f32(eps), {k: f32(v) for k, v in w.items()}, "1", n_h, n_z, d)
    np.testing.assert_allclose(host(z), ref, atol=1e-4, rtol=0)
    assert np.abs(host(z) - f32(eps)).max() > 1e-2, "the sample must not be the reference's placeholder z = eps"
    if name in TINY:
        h_all = layer.down_p(t_dn, t_eps, max_sweeps=H * W * n_z, tol=0.0, stats=stats)
        assert _stats(stats)[0] == H * W * n_z
        np.testing.assert_allclose(host(h_all[:, n_h:]), ref, atol=1e-4 * max(1.0, np.abs(ref).max()), rtol=0)
