"""The reference statements of the 'down_iaf2_deep' posterior (tests/deep_reference.py) against what pins them: the NumPy layer and the
torch statement against the outputs of the reference's own models.cvae_layer (tests/golden/theano_cvae_layer_deep.npz: up, down_q,
down_p), torch gradients against central finite differences, the decomposition CVAELayerIAF.backward runs against autograd of the whole
statement, the exact inverse against the step, and the generator's case table against the fixture.  CPU only, fp64 throughout."""
import os

import numpy as np
import pytest
import torch

import deep_reference as DR
import make_golden_deep as MGD
from oracle import iaf_grad_oracle as G

CASES = sorted(MGD.CASES)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, MGD.FIXTURE))


def test_case_table_matches_the_fixture(fixture):
    """the issue's four cases, and every key of the fixture belongs to one of them"""
    assert MGD.CASES == {"deep_d1": (2, 32, 32, 1, 3, 7, 0.0), "deep_d2": (3, 64, 32, 2, 6, 5, 0.25),
                         "deep_nz16": (2, 32, 16, 1, 4, 6, 0.25), "deep_d4": (1, 32, 32, 4, 4, 4, 0.0)}
    outs = ("up_out", "down_out", "down_p_out", "kl", "kl_sum", "obj_kl")
    assert sorted(set(k.split("/")[0] for k in fixture.files)) == CASES
    for cname, (B, n_h, n_z, depth, H, W, kl_min) in MGD.CASES.items():
        keys = [k for k in fixture.files if k.startswith(cname + "/")]
        assert sorted(k for k in keys if "/w_shape/" not in k) == sorted(cname + "/" + o for o in outs)
        wnames = sorted(k.split("/w_shape/")[1] for k in keys if "/w_shape/" in k)
        deep = [nm + sfx for nm in MGD.deep_names("1", depth) for sfx in ("_w", "_s", "_b")]
        assert sorted(n for n in wnames if "_deepiaf_" in n) == sorted(deep)
        assert not any("posterior_conv" in n for n in wnames)
        assert tuple(fixture[cname + "/w_shape/1_deepiaf_input_w"]) == (n_h, n_z + 1, 3, 3)
        assert tuple(fixture[cname + "/w_shape/1_deepiaf_0_conv2_w"]) == (n_h, n_h + 1, 3, 3)
        assert tuple(fixture[cname + "/w_shape/1_deepiaf_out_1_w"]) == (n_z, n_h + 1, 3, 3)
        assert fixture[cname + "/kl"].shape == (B, n_z, H, W) and np.abs(fixture[cname + "/kl"]).max() < MGD.KL_BOUND
        assert fixture[cname + "/obj_kl"].shape == (() if kl_min > 0 else (B,))


@pytest.mark.parametrize("cname", CASES)
def test_numpy_statement_reproduces_the_reference_fixture(fixture, cname):
    B, n_h, n_z, depth, H, W, kl_min = MGD.CASES[cname]
    c = MGD.fixture_case(fixture, cname)
    r = DR.deep_layer("1", c["w"], n_h, n_z, depth, c["up_input"], c["down_input"], c["eps_down"])
    kl_sum, obj_kl = DR.free_bits(r["kl"], kl_min)
    np.testing.assert_allclose(r["up_out"], fixture[cname + "/up_out"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(r["down_out"], fixture[cname + "/down_out"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(r["kl"], fixture[cname + "/kl"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(kl_sum, fixture[cname + "/kl_sum"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(obj_kl, fixture[cname + "/obj_kl"], rtol=1e-9, atol=1e-9)
    _, _, p_out = DR.down_p_layer("1", c["w"], n_h, n_z, c["down_input"], c["eps_p"])
    np.testing.assert_allclose(p_out, fixture[cname + "/down_p_out"], rtol=1e-9, atol=1e-9)
    # the points that are easy to get wrong must not pass: a nonlinearity in front of the output convs, or no 0.1 on the residual
    hs, _ = DR.resnet(r["z0"], r["context"], c["w"], "1_deepiaf", n_z, n_h, depth, return_hiddens=True)
    wrong = [DR._conv(DR._elu(hs[-1]), c["w"], "1_deepiaf_out_%d" % j, n_h, n_z, True) for j in range(2)]
    z_wrong = (r["z0"] - 0.1 * wrong[0]) / np.exp(0.1 * wrong[1])
    assert np.abs(z_wrong - r["z"]).max() > 1e-4


@pytest.mark.parametrize("cname", CASES)
def test_torch_statement_reproduces_the_reference_fixture(fixture, cname):
    B, n_h, n_z, depth, H, W, kl_min = MGD.CASES[cname]
    c = MGD.fixture_case(fixture, cname)
    r = DR.deep_layer("1", c["w"], n_h, n_z, depth, c["up_input"], c["down_input"], c["eps_down"])
    with torch.no_grad():
        up_out, h_out, kl, obj = DR.deep_iaf_torch(G._t(r["up_conv1"]), G._t(r["down_conv1"]), G._t(c["eps_down"]),
                                                   {k: G._t(v) for k, v in c["w"].items()}, "1", n_h, n_z, depth, kl_min)
    np.testing.assert_array_equal(up_out.numpy(), r["up_conv1"][:, :n_h])
    np.testing.assert_allclose(h_out.numpy(), r["h"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(kl.numpy(), fixture[cname + "/kl"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(obj.numpy(), fixture[cname + "/obj_kl"], rtol=1e-9, atol=1e-9)


def test_torch_gradients_agree_with_central_differences_on_deep_d1(fixture):
    """L = <dz_new, z_new> + <dlogsd, logsd> of the step at deep_d1's geometry and weights: autograd against (L(x + e) - L(x - e)) / 2e of
    the NumPy statement, e = 1e-5, at entries of z, of the context and of every kind of weight (relative to the largest entry probed:
    the differences' own error is O(e^2) plus rounding / e, some 1e-9 here)"""
    cname = "deep_d1"
    B, n_h, n_z, depth, H, W, kl_min = MGD.CASES[cname]
    c = MGD.fixture_case(fixture, cname)
    pre = "1_deepiaf"
    w = {k: v for k, v in c["w"].items() if k.startswith(pre + "_")}
    rng = np.random.RandomState(7)
    z, ctx = rng.standard_normal((B, n_z, H, W)), 0.5 * rng.standard_normal((B, n_h, H, W))
    dz_new, dlogsd = rng.standard_normal(z.shape), rng.standard_normal(z.shape)
    g, z_new, logsd = DR.deep_step_grads(z, ctx, w, pre, n_z, n_h, depth, dz_new, dlogsd)
    zn, ls = DR.deep_step(z, ctx, w, pre, n_z, n_h, depth)
    np.testing.assert_allclose(z_new, zn, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(logsd, ls, rtol=1e-11, atol=1e-12)

    def loss(zz, cc, ww):
        a, b = DR.deep_step(zz, cc, ww, pre, n_z, n_h, depth)
        return (a * dz_new).sum() + (b * dlogsd).sum()

    e = 1e-5
    probes = [("z", z, (0, 3, 1, 2)), ("z", z, (1, n_z - 1, 2, 6)), ("context", ctx, (1, 5, 0, 0)), ("context", ctx, (0, n_h - 1, 2, 3))]
    for nm in DR.conv_names(depth):
        k = "%s_%s" % (pre, nm)
        probes += [(k + "_w", w[k + "_w"], (1, 0, 2, 1)), (k + "_w", w[k + "_w"], (3, w[k + "_w"].shape[1] - 1, 2, 2)),   # (.., last): the border channel
                   (k + "_s", w[k + "_s"], (2,)), (k + "_b", w[k + "_b"], (1,))]
    got, want = [], []
    for key, arr, idx in probes:
        old = arr[idx]
        arr[idx] = old + e
        lp = loss(z, ctx, w)
        arr[idx] = old - e
        lm = loss(z, ctx, w)
        arr[idx] = old
        want.append((lp - lm) / (2 * e))
        got.append(g[key][idx])
    got, want = np.asarray(got), np.asarray(want)
    assert np.abs(want).max() > 1e-3
    assert np.abs(got - want).max() <= 1e-7 * np.abs(want).max(), (got, want)


@pytest.mark.parametrize("with_up", [True, False], ids=["d_up", "d_up_none"])
@pytest.mark.parametrize("free_bits", [False, True], ids=["dko", "free_bits"])
def test_gradient_decomposition_equals_autograd_of_the_whole_statement(free_bits, with_up):
    B, n_h, n_z, depth, H, W = 2, 8, 4, 2, 3, 2
    rng = np.random.RandomState(11)
    w = DR.rand_params(rng, "1_deepiaf", n_z, n_h, depth)
    h_up, h_dn = rng.standard_normal((B, 2 * n_h + 2 * n_z, H, W)), rng.standard_normal((B, 2 * n_h + 4 * n_z, H, W))
    h_up[:, n_h + n_z:n_h + 2 * n_z] *= 0.25
    h_dn[:, n_h + n_z:n_h + 2 * n_z] *= 0.25
    h_dn[:, n_h + 3 * n_z:n_h + 4 * n_z] *= 0.25
    eps = rng.standard_normal((B, n_z, H, W))
    kl_min = 0.0
    if free_bits:
        per_c = np.sort(DR.deep_iaf(h_up, h_dn, eps, w, "1", n_h, n_z, depth)["kl"].sum(axis=(2, 3)).mean(axis=0))
        kl_min = float(0.5 * (per_c[1] + per_c[2]))
    d_up = rng.standard_normal((B, n_h, H, W)) if with_up else None
    d_h = rng.standard_normal((B, n_h + n_z, H, W))
    d_obj = np.asarray(0.7) if kl_min > 0 else rng.standard_normal(B)
    ref, fw = DR.deep_iaf_grads(h_up, h_dn, eps, w, "1", n_h, n_z, depth, kl_min, d_up, d_h, d_obj)
    got = DR.deep_iaf_grads_by_steps(h_up, h_dn, eps, w, "1", n_h, n_z, depth, kl_min, d_up, d_h, d_obj)
    np.testing.assert_allclose(got["h_up"], ref["h_up"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(got["h_dn"], ref["h_dn"], rtol=0, atol=1e-10)
    assert set(got["w"]) == set(ref["w"]) == set(w)
    for k in sorted(w):
        np.testing.assert_allclose(got["w"][k], ref["w"][k], rtol=0, atol=1e-10, err_msg=k)
        assert np.abs(ref["w"][k]).max() > 0, k


def test_exact_inverse_inverts_the_step():
    B, n_h, n_z, depth, H, W = 2, 8, 4, 2, 2, 3
    rng = np.random.RandomState(5)
    w = DR.rand_params(rng, "r", n_z, n_h, depth)
    ctx, z = rng.standard_normal((B, n_h, H, W)), rng.standard_normal((B, n_z, H, W))
    z_new, _ = DR.deep_step(z, ctx, w, "r", n_z, n_h, depth)
    np.testing.assert_allclose(DR.inverse_exact(z_new, ctx, w, "r", n_z, n_h, depth), z, rtol=0, atol=1e-12)
    assert np.abs(DR.inverse_exact(z_new, ctx, w, "r", n_z, n_h, depth, sweeps=1) - z).max() > 1e-6
