"""The reference statements of the 'down_iaf2_nl2' posterior (tests/chain_reference.py) against what pins them: the NumPy chain against
the outputs of the reference's own models.cvae_layer (tests/golden/theano_cvae_layer_nl2.npz), the torch chain against the NumPy chain
and against central finite differences, and the NumPy contracts of the two backward entry points against torch autograd of the
elementwise parts.  CPU only, fp64 throughout."""
import os

import numpy as np
import pytest
import torch

import chain_reference as CR
import make_golden_chain as MGC
from oracle import iaf_grad_oracle as G
from oracle import iaf_oracle as O


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
    h_up, h_dn = rng.standard_normal((B, 2 * n_h + 2 * n_z, H, W)), rng.standard_normal((B, 2 * n_h + 4 * n_z, H, W))
    h_up[:, n_h + n_z:n_h + 2 * n_z] *= 0.25                        # qz_logsd
    h_dn[:, n_h + n_z:n_h + 2 * n_z] *= 0.25                        # pz_logsd
    h_dn[:, n_h + 3 * n_z:n_h + 4 * n_z] *= 0.25                    # rz_logsd
    return h_up, h_dn


@pytest.mark.parametrize("cname", sorted(MGC.CASES))
def test_numpy_chain_reproduces_the_reference_fixture(golden_dir, cname):
    """fp64 against fp64: kl, kl_sum, obj_kl to rtol 1e-9, up_out / down_out to atol 1e-12; and one flow alone is far from the fixture"""
    B, n_h, n_z, depth_ar, H, W, kl_min = MGC.CASES[cname]
    g = np.load(os.path.join(golden_dir, MGC.FIXTURE))
    c = MGC.fixture_case(g, cname)
    assert any(k.startswith("1_posterior_conv2_") for k in c["w"])
    r = CR.chain_layer("1", c["w"], n_h, n_z, depth_ar, c["up_input"], c["down_input"], c["eps_down"])
    kl_sum, obj_kl = CR.free_bits(r["kl"], kl_min)
    np.testing.assert_allclose(r["kl"], g[cname + "/kl"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(kl_sum, g[cname + "/kl_sum"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(obj_kl, g[cname + "/obj_kl"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(r["up_out"], g[cname + "/up_out"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["down_out"], g[cname + "/down_out"], rtol=0, atol=1e-12)
    one = O.theano_cvae_layer("1", "down_iaf2_nl", c["w"], n_h, n_z, depth_ar, c["up_input"], c["down_input"], c["eps_up"], c["eps_down"])
    assert np.abs(one["kl"] - g[cname + "/kl"]).max() > 1.0, "a single flow must not pass for the chain"


def test_torch_chain_equals_numpy_chain_and_contracts_compose():
    """the torch forward equals the NumPy chain; head_np and tail_np around the NumPy steps give the chain's z0, logq0, context, kl, h"""
    B, n_h, n_z, d, H, W = 2, 8, 4, 2, 3, 4
    rng = np.random.RandomState(3)
    w = _params(rng, "1", n_z, [n_h] * d)
    h_up, h_dn = _conv_outputs(rng, B, n_h, n_z, H, W)
    eps = rng.standard_normal((B, n_z, H, W))
    c = CR.chain_iaf(h_up, h_dn, eps, w, "1", n_h, n_z, d)
    for kl_min in (0.0, 0.25):
        with torch.no_grad():
            up_out, h_out, kl, obj = CR.chain_iaf_torch(G._t(h_up), G._t(h_dn), G._t(eps), {k: G._t(v) for k, v in w.items()}, "1", n_h, n_z,
                                                        d, kl_min)
        np.testing.assert_allclose(up_out.numpy(), h_up[:, :n_h], rtol=0, atol=0)
        np.testing.assert_allclose(h_out.numpy(), c["h"], rtol=1e-11, atol=1e-12)
        np.testing.assert_allclose(kl.numpy(), c["kl"], rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(obj.numpy(), CR.free_bits(c["kl"], kl_min)[1], rtol=1e-11)
    z0, logq0, context = CR.head_np(h_up, h_dn, eps, n_h, n_z)
    np.testing.assert_allclose(z0, c["z0"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(logq0, c["logq0"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(context, c["context"], rtol=0, atol=0)
    kl, h = CR.tail_np(h_dn, logq0, c["s1"], c["s2"], c["z"], n_h, n_z)
    np.testing.assert_allclose(kl, c["kl"], rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(h, c["h"], rtol=0, atol=0)


@pytest.mark.parametrize("kl_min", [0.0, 0.25])
def test_torch_chain_gradients_match_finite_differences(kl_min):
    """central differences of the NumPy chain's loss at random entries of both conv outputs and of weights of BOTH stacks"""
    B, n_h, n_z, d, H, W = 2, 8, 4, 1, 3, 2
    rng = np.random.RandomState(11)
    w = _params(rng, "1", n_z, [n_h] * d)
    h_up, h_dn = _conv_outputs(rng, B, n_h, n_z, H, W)
    eps = rng.standard_normal((B, n_z, H, W))
    d_up, d_h = rng.standard_normal((B, n_h, H, W)), rng.standard_normal((B, n_h + n_z, H, W))
    d_obj = np.asarray(0.7) if kl_min > 0 else rng.standard_normal(B)
    grads, fw = CR.chain_iaf_grads(h_up, h_dn, eps, w, "1", n_h, n_z, d, kl_min, d_up, d_h, d_obj)
    if kl_min > 0:      # the case must exercise both sides of the max() of the free bits, away from its kink
        per_c = fw["kl"].sum(axis=(2, 3)).mean(axis=0)
        assert np.abs(per_c - kl_min).min() > 1e-3

    def loss(hu, hd, ww):
        c = CR.chain_iaf(hu, hd, eps, ww, "1", n_h, n_z, d)
        return (hu[:, :n_h] * d_up).sum() + (c["h"] * d_h).sum() + (CR.free_bits(c["kl"], kl_min)[1] * d_obj).sum()

    pick = np.random.RandomState(0)
    step = 1e-6
    names = ["h_up", "h_dn", "1_posterior_conv1_0_w", "1_posterior_conv1_out_1_s", "1_posterior_conv1_out_0_b", "1_posterior_conv2_0_w",
             "1_posterior_conv2_0_s", "1_posterior_conv2_out_0_w", "1_posterior_conv2_out_1_b"]
    for name in names:
        base = h_up if name == "h_up" else h_dn if name == "h_dn" else w[name]
        got = grads[name] if name in ("h_up", "h_dn") else grads["w"][name]
        for _ in range(8 if name.startswith("h_") else 4):
            idx = tuple(pick.randint(0, s) for s in base.shape)

            def at(delta):
                arr = base.copy()
                arr[idx] += delta
                if name == "h_up":
                    return loss(arr, h_dn, w)
                if name == "h_dn":
                    return loss(h_up, arr, w)
                ww = dict(w)
                ww[name] = arr
                return loss(h_up, h_dn, ww)

            fd = (at(step) - at(-step)) / (2 * step)
            assert abs(fd - got[idx]) < 1e-6 * max(1.0, abs(fd)), (name, idx, fd, got[idx])


@pytest.mark.parametrize("with_up", [True, False], ids=["d_up", "d_up_none"])
@pytest.mark.parametrize("free_bits", [True, False], ids=["free_bits", "dko"])
def test_numpy_pre_and_post_reproduce_autograd_of_the_elementwise_parts(free_bits, with_up):
    """torch autograd of  <d_up, up h_det> + <d_h, [h_det | z2]> + <G, logq0 + s1 + s2 - logp(z2)> + <dz0, z0> + <dctx1 + dctx2, context>
    with z2, s1, s2 as leaves: what flows into z2 is pre_np's dz2, the gradients of the conv outputs are pre_np's and post_np's channels
    (dz0, dctx1, dctx2 stand for what the two steps' backward passes return)"""
    B, n_h, n_z, H, W = 3, 5, 3, 2, 4
    rng = np.random.RandomState(21 + 2 * free_bits + with_up)
    h_up, h_dn = _conv_outputs(rng, B, n_h, n_z, H, W)
    f = lambda c: rng.standard_normal((B, c, H, W))
    eps, z2, d_h, dz0, dctx1, dctx2 = f(n_z), f(n_z), f(n_h + n_z), f(n_z), f(n_h), f(n_h)
    d_up = f(n_h) if with_up else None
    gate, gscale, dko = (((rng.uniform(size=n_z) > 0.4).astype(np.float64), 0.7 / B, None) if free_bits else
                         (None, 0.0, rng.standard_normal(B)))
    Gf = CR.expand_G(z2.shape, gate, gscale, dko)
    ut, dt, zt = G._t(h_up, True), G._t(h_dn, True), G._t(z2, True)
    _, qm, ql, uctx = torch.split(ut, [n_h, n_z, n_z, n_h], dim=1)
    h_det, pm, pl, rm, rl, dctx = torch.split(dt, [n_h, n_z, n_z, n_z, n_z, n_h], dim=1)
    mean, logvar = qm + rm, 2 * ql + 2 * rl
    z0 = mean + torch.exp(0.5 * logvar) * G._t(eps)
    logq0 = CR._logps(mean, logvar, z0)
    kl = logq0 - CR._logps(pm, 2 * pl, zt)                     # (s1 + s2 are leaves of their own: their gradient is G itself)
    loss = (torch.cat([h_det, zt], dim=1) * G._t(d_h)).sum() + (kl * G._t(Gf)).sum() + (z0 * G._t(dz0)).sum() \
        + ((uctx + dctx) * G._t(dctx1 + dctx2)).sum()
    if with_up:
        loss = loss + (ut[:, :n_h] * G._t(d_up)).sum()
    loss.backward()
    z0_np = CR.head_np(h_up, h_dn, eps, n_h, n_z)[0]
    dz2, G_out, dd_first = CR.pre_np(h_dn, z2, d_h, n_h, n_z, gate, gscale, dko)
    d_uc1, dd_rest = CR.post_np(h_up, h_dn, z0_np, dz0, Gf, dctx1, dctx2, d_up, n_h, n_z)
    np.testing.assert_array_equal(G_out, Gf)
    np.testing.assert_allclose(dz2, zt.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(d_uc1, ut.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(np.concatenate([dd_first, dd_rest], axis=1), dt.grad.numpy(), rtol=1e-12, atol=1e-12)
