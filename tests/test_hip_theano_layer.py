"""GPU tests of iaf_amd.CVAELayer, the whole models.cvae_layer (downsample=False) on the device: every case of the four reference
fixtures (tests/golden/theano_cvae_layer*.npz: 15 cases, the reference's own up_out / down_out / down_p_out / kl) through CVAELayer
ALONE -- no conv on the host --, the two-phase backward against torch-fp64 autograd of the restated layer, and up() + down_q()
captured in one graph.  References: tests/theano_conv_reference.py around chain_reference / deep_reference / made_reference and
oracle.iaf_grad_oracle.  Bounds: those of the fixtures' existing tests (tests/test_hip_deep.py, test_hip_chain.py, test_hip_made.py,
test_hip_parity.py)."""
import functools
import os

import numpy as np
import pytest
import torch

import chain_reference as CR
import deep_reference as DR
import golden_inputs as gi
import made_reference as MR
import make_golden_chain as MGC
import make_golden_deep as MGD
import make_golden_made as MGM
import theano_conv_reference as TR
from oracle import iaf_grad_oracle as G

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


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _rel_close(got, ref, tol, name):
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)
    print("%s: max err / max|ref| = %.3g (tol %g)" % (name, err, tol))
    assert err < tol, "%s: max err / max|ref| = %.3g (tol %g)" % (name, err, tol)


# (fixture file, case) -> (posterior, prior, B, n_h, n_z, depth_ar, H, W, kl_min)
def _all_cases():
    out = {}
    for c, (post, B, n_h, n_z, d, H, W, kl_min) in gi.CVAE_CASES.items():
        out[c] = ("theano_cvae_layer.npz", post, "diag", B, n_h, n_z, d, H, W, kl_min)
    for c, (B, n_h, n_z, d, H, W, kl_min) in MGC.CASES.items():
        out[c] = (MGC.FIXTURE, "down_iaf2_nl2", "diag", B, n_h, n_z, d, H, W, kl_min)
    for c, (B, n_h, n_z, d, H, W, kl_min, post, prior) in MGM.CASES.items():
        out[c] = (MGM.FIXTURE, post, prior, B, n_h, n_z, d, H, W, kl_min)
    for c, (B, n_h, n_z, d, H, W, kl_min) in MGD.CASES.items():
        out[c] = (MGD.FIXTURE, "down_iaf2_deep", "diag", B, n_h, n_z, d, H, W, kl_min)
    return out


CASES = _all_cases()
assert len(CASES) == 15


def _case_inputs(cname, golden_dir):
    fixture = CASES[cname][0]
    g = np.load(os.path.join(golden_dir, fixture))
    if fixture == "theano_cvae_layer.npz":
        pre = cname + "/w_shape/"
        c = gi.cvae_case_inputs(cname, {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)})
    else:
        c = {MGC.FIXTURE: MGC, MGM.FIXTURE: MGM, MGD.FIXTURE: MGD}[fixture].fixture_case(g, cname)
    return g, c


# ---------------------------------------------------------------- 1. the reference's own outputs, through CVAELayer alone
@pytest.mark.parametrize("cname", sorted(CASES))
def test_whole_layer_vs_reference_golden(amd, golden_dir, cname):
    """load() from the reference's weight dict, up(), down_q() and, where the fixture records it, down_p(): the reference's own up_out,
    down_out, down_p_out at 1e-4, kl / kl_sum / obj_kl at the bounds of the fixture's existing test"""
    _, post, prior, B, n_h, n_z, depth, H, W, kl_min = CASES[cname]
    g, c = _case_inputs(cname, golden_dir)
    layer = amd.CVAELayer("1", n_h, n_z, depth, posterior=post, prior=prior, kl_min=kl_min)
    for nm, (a, b) in TR.conv_widths(n_h, n_z, post, prior).items():
        assert (layer.convs[nm].n_in, layer.convs[nm].n_out) == (a, b) and tuple(c["w"]["1" + nm + "_w"].shape) == (b, a + 1, 3, 3), nm
    layer.load({k: dev(v) for k, v in c["w"].items()})
    up_in, dn_in = dev(c["up_input"]), dev(c["down_input"])
    up_out = layer.up(up_in, eps=dev(c["eps_up"]))
    d = layer.down_q(dn_in, eps=dev(c["eps_down"]))
    assert set(d) == {"output", "kl", "kl_sum", "obj_kl", "z"}
    worst = {k: np.abs(host(v) - g[cname + "/" + k]).max() for k, v in (("up_out", up_out), ("down_out", d["output"]), ("kl", d["kl"]),
                                                                        ("kl_sum", d["kl_sum"]), ("obj_kl", d["obj_kl"]))}
    print(cname, ", ".join("%s %.3g" % kv for kv in sorted(worst.items())), "max |kl| %.3g" % np.abs(g[cname + "/kl"]).max())
    np.testing.assert_allclose(host(up_out), g[cname + "/up_out"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(d["output"]), g[cname + "/down_out"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(d["kl"]), g[cname + "/kl"], atol=ATOL, rtol=1e-5)
    np.testing.assert_allclose(host(d["kl_sum"]), g[cname + "/kl_sum"], atol=2e-3, rtol=1e-4)
    np.testing.assert_allclose(host(d["obj_kl"]), g[cname + "/obj_kl"], atol=2e-3, rtol=1e-4)
    if cname + "/down_p_out" in g.files:
        kw = dict(exact=False) if prior == "made" else {}          # the reference leaves z = eps for 'made' (models.py:338-340)
        p_out = layer.down_p(dn_in, dev(c["eps_p"]), **kw)
        print(cname, "down_p_out %.3g" % np.abs(host(p_out) - g[cname + "/down_p_out"]).max())
        np.testing.assert_allclose(host(p_out), g[cname + "/down_p_out"], atol=ATOL, rtol=0)


# ---------------------------------------------------------------- 2. the two-phase backward against fp64 autograd
# posterior, prior, B, n_h, n_z, depth_ar, H, W: one small case each (3x7: rows that are no multiple of anything, all nine ordinary
# position classes); kl_min 0 and 0.25
BWD_CASES = {
    "down_iaf2_nl": ("down_iaf2_nl", "diag", 2, 32, 16, 2, 3, 7),
    "down_iaf2_nl2": ("down_iaf2_nl2", "diag", 2, 32, 32, 1, 3, 7),
    "down_iaf2_deep": ("down_iaf2_deep", "diag", 2, 32, 32, 1, 3, 7),
    "made": ("down_iaf2_nl", "made", 2, 32, 16, 2, 3, 7),
}


def _iaf_params(rng, post, prior, n_h, n_z, depth):
    if post == "down_iaf2_deep":
        return DR.rand_params(rng, "1_deepiaf", n_z, n_h, depth)
    return MR.rand_params(rng, "1", n_z, [n_h] * depth, post) if prior == "made" else \
        {k: v for k, v in MR.rand_params(rng, "1", n_z, [n_h] * depth, post).items() if "_prior_conv1_" not in k}


def _iaf_torch(post, prior, w, eps, n_h, n_z, depth, kl_min):
    if prior == "made":
        return lambda hu, hd: MR.made_iaf_torch(hu, hd, eps, w, "1", n_h, n_z, depth, post, kl_min)
    if post == "down_iaf2_deep":
        return lambda hu, hd: DR.deep_iaf_torch(hu, hd, eps, w, "1", n_h, n_z, depth, kl_min)
    if post == "down_iaf2_nl2":
        return lambda hu, hd: CR.chain_iaf_torch(hu, hd, eps, w, "1", n_h, n_z, depth, kl_min)
    return lambda hu, hd: G.theano_cvae_iaf(post, hu, hd, eps, w, "1", n_h, n_z, depth, kl_min)


@functools.lru_cache(maxsize=None)
def _bwd_reference(name, free_bits):
    post, prior, B, n_h, n_z, depth, H, W = BWD_CASES[name]
    kl_min = 0.25 if free_bits else 0.0
    rng = np.random.RandomState(1300 + len(name) + int(free_bits))
    w = _iaf_params(rng, post, prior, n_h, n_z, depth)
    w.update(TR.rand_layer_convs(rng, "1", n_h, n_z, post, prior))
    up_in, dn_in = 0.3 * rng.standard_normal((B, n_h, H, W)), 0.3 * rng.standard_normal((B, n_h, H, W))
    eps = rng.standard_normal((B, n_z, H, W))
    d_up_out, d_dn_out = rng.standard_normal((B, n_h, H, W)), rng.standard_normal((B, n_h, H, W))
    d_obj = np.asarray(0.7) if free_bits else rng.standard_normal(B)
    wt = {k: TR.t64(v, True) for k, v in w.items()}
    ut, dt = TR.t64(up_in, True), TR.t64(dn_in, True)
    up_out, dn_out, kl, obj = TR.layer_torch("1", wt, ut, dt, _iaf_torch(post, prior, wt, TR.t64(eps), n_h, n_z, depth, kl_min))
    ((up_out * TR.t64(d_up_out)).sum() + (dn_out * TR.t64(d_dn_out)).sum() + (obj * TR.t64(d_obj)).sum()).backward()
    ref = dict(up_out=up_out.detach().numpy(), down_out=dn_out.detach().numpy(), kl=kl.detach().numpy(), obj_kl=obj.detach().numpy(),
               d_up_input=ut.grad.numpy(), d_down_input=dt.grad.numpy(), w={k: v.grad.numpy() for k, v in wt.items()})
    return w, up_in, dn_in, eps, d_up_out, d_dn_out, d_obj, kl_min, ref


@pytest.mark.parametrize("free_bits", [False, True], ids=["dko", "free_bits"])
@pytest.mark.parametrize("name", sorted(BWD_CASES))
def test_two_phase_backward_vs_autograd(amd, name, free_bits):
    """backward_down() then backward_up(): d_down_input, d_up_input and EVERY gradient (the four convs' w -- border channel included --,
    s, b, and the IAF part's) against torch-fp64 autograd of  <d_up_out, up_out> + <d_down_out, down_out> + <d_obj, obj_kl>:
    1e-4 of the reference's largest entry, 2e-4 for the stack weights as tests/test_hip_parity.py"""
    post, prior, B, n_h, n_z, depth, H, W = BWD_CASES[name]
    w, up_in, dn_in, eps, d_up_out, d_dn_out, d_obj, kl_min, ref = _bwd_reference(name, free_bits)
    layer = amd.CVAELayer("1", n_h, n_z, depth, posterior=post, prior=prior, kl_min=kl_min)
    layer.set_training(True)
    for c in layer.convs.values():
        c.set_precision("f32")
    layer.load({k: dev(v) for k, v in w.items()})
    up_out = layer.up(dev(up_in))
    d = layer.down_q(dev(dn_in), eps=dev(eps))
    np.testing.assert_allclose(host(up_out), ref["up_out"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(d["output"]), ref["down_out"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(d["obj_kl"]), ref["obj_kl"], atol=2e-3, rtol=1e-4)
    d_dn_in = layer.backward_down(dev(d_dn_out), d_obj=(0.7 if free_bits else dev(d_obj)))
    d_up_in = layer.backward_up(dev(d_up_out))
    _rel_close(host(d_dn_in), ref["d_down_input"], 1e-4, "d_down_input")
    _rel_close(host(d_up_in), ref["d_up_input"], 1e-4, "d_up_input")
    grads = layer.grads()
    assert set(grads) == set(w)
    for k in sorted(w):
        _rel_close(host(grads[k]), ref["w"][k], 2e-4 if "_posterior_conv" in k or "_prior_conv" in k or "_deepiaf_" in k else 1e-4, k)


def test_up_iaf2_nl_forward_runs_and_its_whole_layer_backward_is_refused(amd, golden_dir):
    cname = "cvae_up_iaf2_nl"
    _, post, prior, B, n_h, n_z, depth, H, W, kl_min = CASES[cname]
    g, c = _case_inputs(cname, golden_dir)
    layer = amd.CVAELayer("1", n_h, n_z, depth, posterior=post, kl_min=kl_min)
    assert layer.convs["_up_conv2"].n_in == n_h + n_z and layer.convs["_down_conv1"].n_out == n_h + 2 * n_z
    layer.set_training(True)
    layer.load({k: dev(v) for k, v in c["w"].items()})
    layer.up(dev(c["up_input"]), eps=dev(c["eps_up"]))
    d = layer.down_q(dev(c["down_input"]))
    with pytest.raises(amd._capi.UnsupportedError):
        layer.backward_down(torch.zeros_like(d["output"]))


# ---------------------------------------------------------------- 3. capture
def test_up_and_down_q_captured_in_one_graph_equal_eager(amd, golden_dir):
    """up() + down_q() launch on the current stream only: captured after a warm-up and replayed with new inputs and noise in the captured
    buffers, they give what the eager calls give, bit for bit"""
    cname = "nl2_64"
    _, post, prior, B, n_h, n_z, depth, H, W, kl_min = CASES[cname]
    g, c = _case_inputs(cname, golden_dir)
    layer = amd.CVAELayer("1", n_h, n_z, depth, posterior=post, prior=prior, kl_min=kl_min)
    layer.load({k: dev(v) for k, v in c["w"].items()})
    up_buf, dn_buf, eps_buf = dev(c["up_input"]), dev(c["down_input"]), dev(c["eps_down"])
    keys = ("output", "kl", "kl_sum", "obj_kl", "z")
    rng = np.random.RandomState(73)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = []
    with torch.cuda.stream(s):
        layer.up(up_buf)
        layer.down_q(dn_buf, eps=eps_buf)                    # warm-up: workspaces exist before the capture
        s.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            up_out = layer.up(up_buf)
            out = layer.down_q(dn_buf, eps=eps_buf)
        trials = [(rng.standard_normal((B, n_h, H, W)), rng.standard_normal((B, n_h, H, W)), rng.standard_normal((B, n_z, H, W))) for _ in range(2)]
        for u, dn, e in trials:
            up_buf.copy_(dev(u))
            dn_buf.copy_(dev(dn))
            eps_buf.copy_(dev(e))
            gr.replay()
            s.synchronize()
            got.append(dict({k: out[k].clone() for k in keys}, up_out=up_out.clone()))
        s.synchronize()
    torch.cuda.synchronize()
    assert not torch.equal(got[0]["z"], got[1]["z"])
    for (u, dn, e), gk in zip(trials, got):
        eager_up = layer.up(dev(u))
        eager = layer.down_q(dev(dn), eps=dev(e))
        assert torch.equal(eager_up, gk["up_out"])
        for k in keys:
            assert torch.equal(eager[k], gk[k]), k
