"""GPU tests of the 'down_iaf2_nl2' posterior of iaf_amd.CVAELayerIAF -- a chain of two IAF steps, the second with the flipped ordering
(models.py:93-98, 272-291) -- and of the four elementwise entry points around the steps (iaf_chain_head / _tail / _backward_pre /
_backward_post): the reference's own outputs (tests/golden/theano_cvae_layer_nl2.npz), the entry points one by one against their NumPy
contracts at sizes where the indexing can go wrong, the backward pass against fp64 autograd, training forward against evaluation forward,
and a captured down_q against the eager one.  References: tests/chain_reference.py."""
import os

import numpy as np
import pytest
import torch

import chain_reference as CR
import make_golden_chain as MGC
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


def _params(rng, name, n_z, n_h_list):
    """both stacks' weights in the reference's layout (ar.py:288-296)"""
    w = {}
    sizes = [n_z] + n_h_list
    for conv in ("_posterior_conv1", "_posterior_conv2"):
        for i in range(len(n_h_list)):
            w["%s%s_%d_w" % (name, conv, i)] = 0.05 * rng.standard_normal((sizes[i + 1], sizes[i] + 1, 3, 3))
            w["%s%s_%d_b" % (name, conv, i)] = 0.1 * rng.standard_normal(sizes[i + 1])
            w["%s%s_%d_s" % (name, conv, i)] = 0.1 * rng.standard_normal(sizes[i + 1])
        for i in range(2):
            w["%s%s_out_%d_w" % (name, conv, i)] = 0.05 * rng.standard_normal((n_z, sizes[-1] + 1, 3, 3))
            w["%s%s_out_%d_b" % (name, conv, i)] = 0.1 * rng.standard_normal(n_z)
            w["%s%s_out_%d_s" % (name, conv, i)] = 0.1 * rng.standard_normal(n_z)
    return w


def _conv_outputs(rng, B, n_h, n_z, H, W):
    """the input scheme of test_cvae_layer_wrapper_backward_vs_autograd_oracle: standard normal, the logsd channels scaled by 0.25"""
    h_up, h_dn = rng.standard_normal((B, 2 * n_h + 2 * n_z, H, W)), rng.standard_normal((B, 2 * n_h + 4 * n_z, H, W))
    h_up[:, n_h + n_z:n_h + 2 * n_z] *= 0.25                        # qz_logsd
    h_dn[:, n_h + n_z:n_h + 2 * n_z] *= 0.25                        # pz_logsd
    h_dn[:, n_h + 3 * n_z:n_h + 4 * n_z] *= 0.25                    # rz_logsd
    return h_up, h_dn


# ---------------------------------------------------------------- the reference's own outputs
@pytest.mark.parametrize("cname", sorted(MGC.CASES))
def test_chain_layer_vs_reference_golden(amd, golden_dir, cname):
    """models.cvae_layer(..., 'down_iaf2_nl2', ...) through iaf_amd.CVAELayerIAF: the plain Theano convs come from the NumPy statement
    (out of scope), the chain and the free bits run on the GPU; tolerances of test_cvae_layer_wrapper_vs_reference_golden"""
    B, n_h, n_z, depth_ar, H, W, kl_min = MGC.CASES[cname]
    g = np.load(os.path.join(golden_dir, MGC.FIXTURE))
    c = MGC.fixture_case(g, cname)
    w32 = {k: f32(v) for k, v in c["w"].items()}
    ref = CR.chain_layer("1", w32, n_h, n_z, depth_ar, f32(c["up_input"]), f32(c["down_input"]), f32(c["eps_down"]))
    layer = amd.CVAELayerIAF("1", n_h, n_z, depth_ar, posterior="down_iaf2_nl2", kl_min=kl_min)
    layer.load({k: dev(v) for k, v in c["w"].items()})
    hu = layer.up(dev(ref["up_conv1"]), eps=dev(c["eps_up"]))
    cw = lambda nm: (w32["1" + nm + "_w"], w32["1" + nm + "_b"], w32["1" + nm + "_s"])
    elu = lambda t: np.where(t < 0, np.exp(np.minimum(t, 0)) - 1, t)
    up_out = f32(c["up_input"]) + 0.1 * O.theano_conv2d(elu(host(hu)), *cw("_up_conv2"))
    np.testing.assert_allclose(up_out, g[cname + "/up_out"], atol=ATOL, rtol=0)
    d = layer.down_q(dev(ref["down_conv1"]), eps=dev(c["eps_down"]))
    for k in ("kl", "kl_sum", "obj_kl"):
        print("%s %s: max abs err %.3g, max |ref| %.3g" % (cname, k, np.abs(host(d[k]) - g[cname + "/" + k]).max(), np.abs(g[cname + "/" + k]).max()))
    np.testing.assert_allclose(host(d["kl"]), g[cname + "/kl"], atol=ATOL, rtol=1e-5)
    np.testing.assert_allclose(host(d["kl_sum"]), g[cname + "/kl_sum"], atol=2e-3, rtol=1e-4)
    np.testing.assert_allclose(host(d["obj_kl"]), g[cname + "/obj_kl"], atol=2e-3, rtol=1e-4)
    down_out = f32(c["down_input"]) + 0.1 * O.theano_conv2d(elu(host(d["h"])), *cw("_down_conv2_1"))
    np.testing.assert_allclose(down_out, g[cname + "/down_out"], atol=ATOL, rtol=0)
    assert torch.equal(d["h"][:, n_h:], d["z"])


# ---------------------------------------------------------------- the four entry points, one by one
LEAF_SHAPES = [(3, 5, 3, 7), (2, 48, 16, 15), (1, 16, 32, 64)]     # B, n_h, n_z, HW: nothing aligned; HW odd; n_z > n_h, 16-byte form
LEAF_TOL = 2e-5


def _leaf_inputs(seed, B, n_h, n_z, HW):
    """Means at half scale, log standard deviations at quarter scale, |G| <= 1: every output is a short fp32 expression whose largest
    term, G dlt^2 exp(-2 pz_logsd), stays below ~40 here, so a few ulp of it (6e-8 relative each) lie an order below LEAF_TOL."""
    rng = np.random.RandomState(seed)
    up, down = rng.standard_normal((B, 2 * n_h + 2 * n_z, HW)), rng.standard_normal((B, 2 * n_h + 4 * n_z, HW))
    up[:, n_h:n_h + n_z] *= 0.5
    up[:, n_h + n_z:n_h + 2 * n_z] *= 0.25
    down[:, n_h:n_h + n_z] *= 0.5
    down[:, n_h + n_z:n_h + 2 * n_z] *= 0.25
    down[:, n_h + 2 * n_z:n_h + 3 * n_z] *= 0.5
    down[:, n_h + 3 * n_z:n_h + 4 * n_z] *= 0.25
    f = lambda c, s=1.0: s * rng.standard_normal((B, c, HW))
    return dict(up=up, down=down, eps=f(n_z), s1=f(n_z, 0.3), s2=f(n_z, 0.3), z2=f(n_z, 0.5), d_h=f(n_h + n_z), d_up=f(n_h), dz0=f(n_z),
                dctx1=f(n_h), dctx2=f(n_h), gate=(rng.uniform(size=n_z) > 0.4).astype(np.float64), dko=rng.uniform(0.2, 1.0, size=B))


def _misaligned(a):
    """the same values in a contiguous tensor whose address is 4 bytes past a 16-byte boundary"""
    flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    t = flat[1:].view(a.shape)
    t.copy_(dev(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "eps_off_by_4_bytes"])
@pytest.mark.parametrize("shape", LEAF_SHAPES, ids=lambda s: "B%d_h%d_z%d_hw%d" % s)
def test_chain_head_and_tail_vs_numpy(amd, shape, misalign):
    """iaf_chain_head and iaf_chain_tail against head_np / tail_np; `misalign`: one operand 4 bytes off a 16-byte boundary, so that the
    16-byte form must not be chosen at HW = 64 either"""
    from iaf_amd import _capi
    from iaf_amd.layers import _ptr, _stream
    B, n_h, n_z, HW = shape
    x = _leaf_inputs(100 + HW, *shape)
    up, down = dev(x["up"]), dev(x["down"])
    eps = _misaligned(x["eps"]) if misalign else dev(x["eps"])
    z0, logq0 = torch.full((B, n_z, HW), SENTINEL, device="cuda"), torch.full((B, n_z, HW), SENTINEL, device="cuda")
    context = torch.full((B, n_h, HW), SENTINEL, device="cuda")
    _capi.check(_capi.lib().iaf_chain_head(_ptr(up), _ptr(down), _ptr(eps), _ptr(z0), _ptr(logq0), _ptr(context), B, n_h, n_z, HW, _stream()))
    ez0, elq, ectx = CR.head_np(f32(x["up"]), f32(x["down"]), f32(x["eps"]), n_h, n_z)
    np.testing.assert_allclose(host(z0), ez0, atol=LEAF_TOL, rtol=0)
    np.testing.assert_allclose(host(logq0), elq, atol=LEAF_TOL, rtol=0)
    np.testing.assert_allclose(host(context), ectx, atol=LEAF_TOL, rtol=0)
    s1 = _misaligned(x["s1"]) if misalign else dev(x["s1"])
    s2, z2 = dev(x["s2"]), dev(x["z2"])
    kl, h_out = torch.full((B, n_z, HW), SENTINEL, device="cuda"), torch.full((B, n_h + n_z, HW), SENTINEL, device="cuda")
    _capi.check(_capi.lib().iaf_chain_tail(_ptr(down), _ptr(logq0), _ptr(s1), _ptr(s2), _ptr(z2), _ptr(kl), _ptr(h_out), B, n_h, n_z, HW,
                                           _stream()))
    ekl, eh = CR.tail_np(f32(x["down"]), host(logq0), f32(x["s1"]), f32(x["s2"]), f32(x["z2"]), n_h, n_z)
    np.testing.assert_allclose(host(kl), ekl, atol=LEAF_TOL, rtol=0)
    np.testing.assert_array_equal(host(h_out), eh)                                   # copies: exact
    for t in (up, down):                                                             # the conv outputs are read only
        assert torch.equal(t, dev(x["up"] if t is up else x["down"]))


@pytest.mark.parametrize("with_up", [True, False], ids=["d_up", "d_up_null"])
@pytest.mark.parametrize("free_bits", [True, False], ids=["gate", "dko"])
@pytest.mark.parametrize("shape", LEAF_SHAPES, ids=lambda s: "B%d_h%d_z%d_hw%d" % s)
def test_chain_backward_pre_and_post_vs_numpy(amd, shape, free_bits, with_up):
    """iaf_chain_backward_pre / _post against pre_np / post_np; d_down_conv1 starts as a sentinel: pre writes its first n_h + 2 n_z
    channels and leaves the rest, post writes the rest and leaves what pre wrote, bit for bit"""
    from iaf_amd import _capi
    from iaf_amd.layers import _ptr, _stream
    B, n_h, n_z, HW = shape
    x = _leaf_inputs(200 + HW, *shape)
    up, down, z2, d_h = dev(x["up"]), dev(x["down"]), dev(x["z2"]), dev(x["d_h"])
    gate, gscale, dko = (dev(x["gate"]), 0.7 / B, None) if free_bits else (None, 0.0, dev(x["dko"]))
    dz2, G = torch.full((B, n_z, HW), SENTINEL, device="cuda"), torch.full((B, n_z, HW), SENTINEL, device="cuda")
    d_dc1 = torch.full((B, 2 * n_h + 4 * n_z, HW), SENTINEL, device="cuda")
    _capi.check(_capi.lib().iaf_chain_backward_pre(_ptr(down), _ptr(z2), _ptr(d_h), _ptr(gate), gscale, _ptr(dko), _ptr(dz2), _ptr(G),
                                                   _ptr(d_dc1), B, n_h, n_z, HW, _stream()))
    gs32 = float(np.float32(gscale))
    edz2, eG, efirst = CR.pre_np(f32(x["down"]), f32(x["z2"]), f32(x["d_h"]), n_h, n_z, x["gate"] if free_bits else None, gs32,
                                 None if free_bits else f32(x["dko"]))
    np.testing.assert_allclose(host(dz2), edz2, atol=LEAF_TOL, rtol=0)
    np.testing.assert_allclose(host(G), eG, atol=1e-6, rtol=0)
    split_at = n_h + 2 * n_z
    np.testing.assert_allclose(host(d_dc1[:, :split_at]), efirst, atol=LEAF_TOL, rtol=0)
    assert bool((d_dc1[:, split_at:] == SENTINEL).all()), "pre wrote outside its channels"
    after_pre = d_dc1.clone()
    z0 = dev(CR.head_np(f32(x["up"]), f32(x["down"]), f32(x["eps"]), n_h, n_z)[0])
    dz0, dctx1, dctx2 = dev(x["dz0"]), dev(x["dctx1"]), dev(x["dctx2"])
    d_up = dev(x["d_up"]) if with_up else None
    d_uc1 = torch.full((B, 2 * n_h + 2 * n_z, HW), SENTINEL, device="cuda")
    _capi.check(_capi.lib().iaf_chain_backward_post(_ptr(up), _ptr(down), _ptr(z0), _ptr(dz0), _ptr(G), _ptr(dctx1), _ptr(dctx2), _ptr(d_up),
                                                    _ptr(d_uc1), _ptr(d_dc1), B, n_h, n_z, HW, _stream()))
    e_uc1, e_rest = CR.post_np(f32(x["up"]), f32(x["down"]), host(z0), f32(x["dz0"]), host(G), f32(x["dctx1"]), f32(x["dctx2"]),
                               f32(x["d_up"]) if with_up else None, n_h, n_z)
    np.testing.assert_allclose(host(d_uc1), e_uc1, atol=LEAF_TOL, rtol=0)
    np.testing.assert_allclose(host(d_dc1[:, split_at:]), e_rest, atol=LEAF_TOL, rtol=0)
    assert torch.equal(d_dc1[:, :split_at], after_pre[:, :split_at]), "post wrote outside its channels"
    assert torch.equal(d_uc1[:, n_h:], d_dc1[:, split_at:])                          # the q and the r channels get the same gradient


# ---------------------------------------------------------------- the layer: backward, training forward, capture
def _layer_case(seed, B, n_h, n_z, d, H, W):
    rng = np.random.RandomState(seed)
    w = _params(rng, "1", n_z, [n_h] * d)
    h_up, h_dn = _conv_outputs(rng, B, n_h, n_z, H, W)
    eps = rng.standard_normal((B, n_z, H, W))
    d_up, d_h = rng.standard_normal((B, n_h, H, W)), rng.standard_normal((B, n_h + n_z, H, W))
    return w, h_up, h_dn, eps, d_up, d_h, rng


@pytest.mark.parametrize("kl_min", [0.0, 0.25])
@pytest.mark.parametrize("shape", [(3, 64, 32, 2, 8, 8), (2, 32, 16, 1, 5, 3)], ids=lambda s: "B%d_h%d_z%d_d%d_%dx%d" % s)
def test_chain_layer_backward_vs_autograd(amd, shape, kl_min):
    """training through the chain: gradients of both conv outputs (reference channel order) and of every weight of BOTH stacks, incl.
    the scalar free-bits objective, against torch-fp64 autograd of the restated forward"""
    B, n_h, n_z, d, H, W = shape
    w, h_up, h_dn, eps, d_up, d_h, rng = _layer_case(5 + int(kl_min * 8) + H, *shape)
    d_obj = np.asarray(0.7) if kl_min > 0 else rng.standard_normal(B)
    layer = amd.CVAELayerIAF("1", n_h, n_z, d, posterior="down_iaf2_nl2", kl_min=kl_min)
    layer.set_training(True)
    layer.load({k: dev(v) for k, v in w.items()})
    print("one-launch steps: %s / %s" % (bool(layer.stack.step_is_fused(B, H, W)), bool(layer.stack2.step_is_fused(B, H, W))))
    up_out = layer.up(dev(h_up))
    dq = layer.down_q(dev(h_dn), eps=dev(eps))
    bw = layer.backward(dev(d_h), d_obj=(0.7 if kl_min > 0 else dev(d_obj)), d_up=dev(d_up))
    ref, fw = CR.chain_iaf_grads(f32(h_up), f32(h_dn), f32(eps), {k: f32(v) for k, v in w.items()}, "1", n_h, n_z, d, kl_min, f32(d_up),
                                 f32(d_h), f32(d_obj))
    np.testing.assert_allclose(host(up_out), fw["up_out"], atol=0, rtol=0)
    np.testing.assert_allclose(host(dq["h"]), fw["h"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(dq["kl"]), fw["kl"], atol=ATOL, rtol=1e-5)
    np.testing.assert_allclose(host(dq["obj_kl"]), fw["obj_kl"], atol=2e-3, rtol=1e-4)
    assert tuple(bw["d_up_conv1"].shape) == (B, 2 * n_h + 2 * n_z, H, W) and tuple(bw["d_down_conv1"].shape) == (B, 2 * n_h + 4 * n_z, H, W)
    _rel_close(host(bw["d_up_conv1"]), ref["h_up"], 1e-4, "d_up_conv1")
    _rel_close(host(bw["d_down_conv1"]), ref["h_dn"], 1e-4, "d_down_conv1")
    assert set(bw["grads"]) == set(w)
    assert any(k.startswith("1_posterior_conv1_") for k in w) and any(k.startswith("1_posterior_conv2_") for k in w)
    for k in sorted(w):
        _rel_close(host(bw["grads"][k]), ref["w"][k], 2e-4, k)


def test_chain_training_forward_equals_evaluation_forward(amd):
    B, n_h, n_z, d, H, W = 3, 64, 32, 2, 8, 8
    w, h_up, h_dn, eps, _, _, _ = _layer_case(31, B, n_h, n_z, d, H, W)
    wd = {k: dev(v) for k, v in w.items()}
    outs = []
    for training in (False, True):
        layer = amd.CVAELayerIAF("1", n_h, n_z, d, posterior="down_iaf2_nl2", kl_min=0.25)
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


def test_chain_down_q_captured_in_a_graph_equals_eager(amd):
    """down_q launches on the current stream only: captured after a warm-up on the capturing stream, replayed twice with new noise written
    into the captured buffer, it gives what the eager call gives"""
    B, n_h, n_z, d, H, W = 2, 32, 16, 2, 6, 5
    w, h_up, h_dn, eps, _, _, rng = _layer_case(41, B, n_h, n_z, d, H, W)
    layer = amd.CVAELayerIAF("1", n_h, n_z, d, posterior="down_iaf2_nl2", kl_min=0.25)
    layer.load({k: dev(v) for k, v in w.items()})
    t_up, t_dn, eps_buf = dev(h_up), dev(h_dn), dev(eps)
    keys = ("h", "z", "kl", "kl_sum", "obj_kl")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = []
    with torch.cuda.stream(s):
        layer.up(t_up)
        layer.down_q(t_dn, eps=eps_buf)                             # warm-up: workspaces exist before the capture
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = layer.down_q(t_dn, eps=eps_buf)
        noises = [rng.standard_normal((B, n_z, H, W)) for _ in range(2)]
        for e in noises:
            eps_buf.copy_(dev(e))
            g.replay()
            s.synchronize()
            got.append({k: out[k].clone() for k in keys})
        s.synchronize()
    torch.cuda.synchronize()
    assert not torch.equal(got[0]["z"], got[1]["z"])
    for e, gk in zip(noises, got):
        eager = layer.down_q(t_dn, eps=dev(e))
        for k in keys:
            assert torch.equal(eager[k], gk[k]), k
