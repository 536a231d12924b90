"""The reference statements of the 'made' prior (tests/made_reference.py) against what pins them: the NumPy layer against the outputs of the
reference's own models.cvae_layer (tests/golden/theano_cvae_layer_made.npz: up, down_q, down_p), the u-form of the KL that the kernels
compute against the reference's form, the torch statement against the NumPy one, the step-by-step gradient decomposition that
CVAELayerIAF.backward runs against autograd of the whole statement, and the sequential sampler against the density it samples.  CPU
only, fp64 throughout."""
import os

import numpy as np
import pytest
import torch

import made_reference as MR
import make_golden_made as MGM
from oracle import iaf_grad_oracle as G
from oracle import iaf_oracle as O


@pytest.mark.parametrize("cname", MGM.MADE_CASES)
def test_numpy_made_layer_reproduces_the_reference_fixture(golden_dir, cname):
    """fp64 against fp64, every array of the fixture, at the bounds test_oracle_golden.py holds the Theano layer to (up_out / down_out
    rtol 1e-9 atol 1e-10, kl rtol 1e-9 atol 1e-9, the sums rtol 1e-10); and the diag prior is far from the fixture"""
    B, n_h, n_z, depth_ar, H, W, kl_min, posterior, prior = MGM.CASES[cname]
    g = np.load(os.path.join(golden_dir, MGM.FIXTURE))
    c = MGM.fixture_case(g, cname)
    assert any(k.startswith("1_prior_conv1_") for k in c["w"])
    assert any(k.startswith("1_posterior_conv2_") for k in c["w"]) == (posterior == "down_iaf2_nl2")
    assert c["w"]["1_down_conv1_w"].shape[0] == 3 * n_h + 2 * n_z
    r = MR.made_layer("1", c["w"], n_h, n_z, depth_ar, posterior, c["up_input"], c["down_input"], c["eps_down"])
    kl_sum, obj_kl = MR.free_bits(r["kl"], kl_min)
    np.testing.assert_allclose(r["up_out"], g[cname + "/up_out"], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(r["down_out"], g[cname + "/down_out"], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(r["kl"], g[cname + "/kl"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(kl_sum, g[cname + "/kl_sum"], rtol=1e-10)
    np.testing.assert_allclose(obj_kl, g[cname + "/obj_kl"], rtol=1e-10)
    # the u-form of the same KL (what iaf_made_tail computes): 1e-12, relative where |kl| > 1 -- the fixtures hold entries of order 1e5,
    # whose fp64 spacing alone is 1.5e-11
    np.testing.assert_allclose(r["kl_u"], r["kl"], rtol=1e-12, atol=1e-12)
    # a standard-normal prior in place of the MADE one must not pass
    std = r["kl"] + r["logps"] - O.gaussian_diag_logps(np.zeros_like(r["z"]), np.zeros_like(r["z"]), r["z"])
    assert np.abs(std - g[cname + "/kl"]).max() > 1e-2
    # down_p as the reference runs it: z = eps (models.py:338-340)
    _, h_p, p_out = MR.down_p_layer("1", c["w"], n_h, n_z, depth_ar, "made", c["down_input"], c["eps_p"], exact=False)
    np.testing.assert_array_equal(h_p[:, n_h:], c["eps_p"])
    np.testing.assert_allclose(p_out, g[cname + "/down_p_out"], rtol=1e-9, atol=1e-10)


def test_numpy_diag_down_p_reproduces_the_reference_fixture(golden_dir):
    cname = "diag_p"
    B, n_h, n_z, depth_ar, H, W, kl_min, posterior, prior = MGM.CASES[cname]
    assert prior == "diag"
    g = np.load(os.path.join(golden_dir, MGM.FIXTURE))
    c = MGM.fixture_case(g, cname)
    assert not any(k.startswith("1_prior_conv1_") for k in c["w"])
    down_conv1, h_p, p_out = MR.down_p_layer("1", c["w"], n_h, n_z, depth_ar, "diag", c["down_input"], c["eps_p"])
    assert down_conv1.shape[1] == 2 * n_h + 4 * n_z
    np.testing.assert_allclose(p_out, g[cname + "/down_p_out"], rtol=1e-9, atol=1e-10)
    np.testing.assert_array_equal(h_p, MR.diag_sample_np(down_conv1, c["eps_p"], n_h, n_z))
    one = O.theano_cvae_layer("1", posterior, c["w"], n_h, n_z, depth_ar, c["up_input"], c["down_input"], c["eps_up"], c["eps_down"])
    np.testing.assert_allclose(one["kl"], g[cname + "/kl"], rtol=1e-9, atol=1e-9)      # the fixture's diag case is the known layer


@pytest.mark.parametrize("posterior", ["down_iaf2_nl", "down_iaf2_nl2"])
def test_u_form_torch_statement_and_contracts_agree(posterior):
    """kl through u equals the reference's form to 1e-12; the torch forward equals the NumPy one; head_np and tail_np around the NumPy
    steps give the statement's z0, logq0, context, made_context, kl, h"""
    B, n_h, n_z, d, H, W = 2, 8, 4, 2, 3, 4
    rng = np.random.RandomState(3)
    w = MR.rand_params(rng, "1", n_z, [n_h] * d, posterior)
    h_up, h_dn = MR.rand_conv_outputs(rng, B, n_h, n_z, H, W)
    eps = rng.standard_normal((B, n_z, H, W))
    c = MR.made_iaf(h_up, h_dn, eps, w, "1", n_h, n_z, d, posterior)
    np.testing.assert_allclose(c["kl_u"], c["kl"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(-(0.5 * MR.LOG2PI + c["s_p"] + 0.5 * c["u"] ** 2), c["logps"], rtol=0, atol=1e-12)
    for kl_min in (0.0, 0.25):
        with torch.no_grad():
            up_out, h_out, kl, obj = MR.made_iaf_torch(G._t(h_up), G._t(h_dn), G._t(eps), {k: G._t(v) for k, v in w.items()}, "1", n_h, n_z,
                                                       d, posterior, kl_min)
        np.testing.assert_allclose(up_out.numpy(), h_up[:, :n_h], rtol=0, atol=0)
        np.testing.assert_allclose(h_out.numpy(), c["h"], rtol=1e-11, atol=1e-12)
        np.testing.assert_allclose(kl.numpy(), c["kl"], rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(obj.numpy(), MR.free_bits(c["kl"], kl_min)[1], rtol=1e-11)
    z0, logq0, context, mctx = MR.head_np(h_up, h_dn, eps, n_h, n_z)
    np.testing.assert_allclose(z0, c["z0"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(logq0, c["logq0"], rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(context, c["context"])
    np.testing.assert_array_equal(mctx, h_dn[:, n_h:2 * n_h])
    kl, h = MR.tail_np(h_dn, logq0, c["s1"], c["s2"], c["z"], c["u"], c["s_p"], n_h, n_z)
    np.testing.assert_allclose(kl, c["kl"], rtol=1e-11, atol=1e-11)
    np.testing.assert_array_equal(h, c["h"])


@pytest.mark.parametrize("with_up", [True, False], ids=["d_up", "d_up_none"])
@pytest.mark.parametrize("free_bits", [False, True], ids=["dko", "free_bits"])
@pytest.mark.parametrize("posterior", ["down_iaf2_nl", "down_iaf2_nl2"])
def test_gradient_decomposition_equals_autograd_of_the_whole_statement(posterior, free_bits, with_up):
    """the two- / three-step decomposition of CVAELayerIAF.backward -- prior step backward with (G u, G), join, posterior steps in reverse
    with dlogsd = G, the reparametrised sample -- against torch autograd of the whole statement (logps the reference's way), to 1e-10.
    With free bits kl_min lies between the per-channel KLs of this case, so that both sides of the max() carry channels."""
    B, n_h, n_z, d, H, W = 2, 8, 4, 1, 3, 2
    rng = np.random.RandomState(11)
    w = MR.rand_params(rng, "1", n_z, [n_h] * d, posterior)
    h_up, h_dn = MR.rand_conv_outputs(rng, B, n_h, n_z, H, W)
    eps = rng.standard_normal((B, n_z, H, W))
    kl_min = 0.0
    if free_bits:
        per_c = np.sort(MR.made_iaf(h_up, h_dn, eps, w, "1", n_h, n_z, d, posterior)["kl"].sum(axis=(2, 3)).mean(axis=0))
        kl_min = float(0.5 * (per_c[1] + per_c[2]))
    d_up = rng.standard_normal((B, n_h, H, W)) if with_up else None
    d_h = rng.standard_normal((B, n_h + n_z, H, W))
    d_obj = np.asarray(0.7) if kl_min > 0 else rng.standard_normal(B)
    ref, fw = MR.made_iaf_grads(h_up, h_dn, eps, w, "1", n_h, n_z, d, posterior, kl_min, d_up, d_h, d_obj)
    if kl_min > 0:      # both sides of the max() of the free bits, away from its kink
        per_c = fw["kl"].sum(axis=(2, 3)).mean(axis=0)
        assert np.abs(per_c - kl_min).min() > 1e-3 and (per_c > kl_min).any() and (per_c < kl_min).any(), per_c
    got = MR.made_iaf_grads_by_steps(h_up, h_dn, eps, w, "1", n_h, n_z, d, posterior, kl_min, d_up, d_h, d_obj)
    np.testing.assert_allclose(got["h_up"], ref["h_up"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(got["h_dn"], ref["h_dn"], rtol=0, atol=1e-10)
    assert set(got["w"]) == set(ref["w"]) == set(w)
    for k in sorted(w):
        np.testing.assert_allclose(got["w"][k], ref["w"][k], rtol=0, atol=1e-10, err_msg=k)
    assert np.abs(ref["h_dn"][:, n_h:2 * n_h]).max() > 1e-4, "made_context must receive a gradient"


def test_sequential_sampler_inverts_the_prior_step():
    """sample_exact's z is the point whose prior step gives eps back: u(z) = eps to rounding, so z ~ the MADE prior when eps ~ N(0, 1);
    and z differs from eps, the reference's placeholder"""
    B, n_h, n_z, d, H, W = 2, 8, 4, 2, 2, 3
    rng = np.random.RandomState(5)
    w = MR.rand_params(rng, "1", n_z, [n_h] * d, "down_iaf2_nl")
    mctx, eps = rng.standard_normal((B, n_h, H, W)), rng.standard_normal((B, n_z, H, W))
    z = MR.sample_exact(mctx, eps, w, "1", n_h, n_z, d)
    u, _ = O.theano_iaf2_nl(z, mctx, w, "1_prior_conv1", n_z, [n_h] * d, flipmask=False)
    np.testing.assert_allclose(u, eps, rtol=0, atol=1e-13)
    assert np.abs(z - eps).max() > 1e-2
    few = MR.sample_exact(mctx, eps, w, "1", n_h, n_z, d, sweeps=1)
    assert np.abs(few - z).max() > 1e-6, "one sweep is not the sample"


@pytest.mark.parametrize("n_z,n_h,d", [(4, 8, 2), (8, 8, 1), (4, 12, 2), (16, 32, 1)])
def test_a_narrow_theano_stack_embedded_in_a_wide_one_is_the_same_function(n_z, n_h, d):
    """what iaf_amd.layers.EmbeddedTheanoStack relies on for Theano stacks whose channel counts are not multiples of 16 (plain ordering, n_z | n_h): with
    channel c at position t c of a stack t times as wide and zeros elsewhere, the wide stack's (m, s) at the real positions are the
    narrow stack's, to fp64 rounding, and its other outputs are zero"""
    import math
    t = 16 // math.gcd(16, math.gcd(n_z, n_h))
    rng = np.random.RandomState(n_z + n_h)
    w = MR.rand_params(rng, "1", n_z, [n_h] * d, "down_iaf2_nl")
    B, H, W = 2, 3, 2
    z, c = rng.standard_normal((B, n_z, H, W)), rng.standard_normal((B, n_h, H, W))
    m, s = O.theano_multiconv2d(z, c, w, "1_prior_conv1", n_z, [n_h] * d, [n_z, n_z], False)
    we = MR.embed_params(w, "1_prior_conv1", n_z, [n_h] * d, t)
    ze, ce = np.zeros((B, n_z * t, H, W)), np.zeros((B, n_h * t, H, W))
    ze[:, ::t], ce[:, ::t] = z, c
    me, se = O.theano_multiconv2d(ze, ce, we, "1_prior_conv1", n_z * t, [n_h * t] * d, [n_z * t, n_z * t], False)
    np.testing.assert_allclose(me[:, ::t], m, rtol=0, atol=1e-13)
    np.testing.assert_allclose(se[:, ::t], s, rtol=0, atol=1e-13)
    keep = np.zeros(n_z * t, dtype=bool)
    keep[::t] = True
    assert not me[:, ~keep].any() and not se[:, ~keep].any()
