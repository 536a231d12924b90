"""The fp16-plane step kernels with branch-free epilogues and one final-loop body per mode (iaf_step_fused.hpp, FLAT = 1).

The change is a re-ordering of the same arithmetic, so what can go wrong is WHICH lanes write what: a lane past a half-filled pixel
tile now stores (the same bytes to the same slot as the last pixel's lane), a row past the image bottom is a select, the training
stores run in a block of their own behind the LDS stores, and the final loop picks its mode once.  Hence: every mode of the final loop,
the training stores, batches that leave ticket lists empty or fill them unevenly, both BASELINE geometries (8x8: three rows of the first
hidden layer per workgroup = one and a half pixel tiles; 16x16: halo rows exchanged), and graph replays.

The kernels exist for n_z = 32, n_h = 160, depth_ar = 2.  Gate of the step: tests/test_hip_f16x2.py.
Reference operator: tf_utils/layers.py:31-64,158-166; tf_train.py:56-85."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from oracle import iaf_oracle as O

pytestmark = pytest.mark.gpu
N_Z, N_H, D = 32, 160, 2


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()
    return iaf_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _stack(amd, params, precision, training=False, fuse=None):
    """fuse: None = "always" for the fp16 planes (the kernels under test), the stack's own choice for the exact-fp32 yardstick"""
    st = amd.ARStack(N_Z, [N_H] * D)
    st.set_precision(precision)
    if training:
        st.set_training(True)
    if fuse or precision == "f16x2":
        st.set_fuse_step(fuse or "always")
    dp = {k: dev(v) for k, v in params.items()}
    st.prepare(dp)
    return st


@pytest.fixture(scope="module")
def case():
    """one set of weights and, per image size, inputs for nine images with their fp64 results (computed once; tests slice the batch)"""
    rng = np.random.RandomState(2025)
    params = gi.ar_multiconv2d_params(rng, N_Z, [N_H] * D, [N_Z, N_Z])
    p32 = {k: f32(v) for k, v in params.items()}
    data = {}
    for H in (8, 16):
        z, ctx = rng.standard_normal((9, N_Z, H, H)), rng.standard_normal((9, N_H, H, H))
        m, s = O.ar_multiconv2d(f32(z), f32(ctx), p32, [N_H] * D, [N_Z, N_Z])
        data[H] = dict(z=z, ctx=ctx, m_raw=m, s_raw=s, z_new=(f32(z) - 0.1 * m) / np.exp(0.1 * s), logsd=0.1 * s)
    return params, p32, data


@pytest.mark.parametrize("H", [8, 16])
@pytest.mark.parametrize("B", [1, 3, 9])
def test_iaf_step_vs_fp64_within_1p5x_of_the_exact_fp32_kernels(amd, case, B, H):
    """B = 1 leaves seven of the eight ticket lists empty, B = 3 and 9 fill them unevenly"""
    params, _, data = case
    d = data[H]
    z, ctx = d["z"][:B], d["ctx"][:B]
    errs = {}
    for prec in ("f32", "f16x2"):
        st = _stack(amd, params, prec)
        if prec == "f16x2":
            assert st.step_is_f16(B, H, H)
        zn, ls = st.iaf_step(dev(z), dev(ctx))
        errs[prec] = max(np.abs(host(zn) - d["z_new"][:B]).max(), np.abs(host(ls) - d["logsd"][:B]).max())
        assert st.range_errors() == 0 and st.exchange_errors() == 0
    print("B=%d %dx%d: max |. - fp64 oracle|: %s" % (B, H, H, ", ".join("%s %.3g" % kv for kv in errs.items())))
    assert errs["f16x2"] <= 1.5 * errs["f32"], errs
    assert errs["f16x2"] < 1e-4


@pytest.mark.parametrize("H", [8, 16])
def test_posterior_block_vs_oracle(amd, case, H):
    """the posterior body of the final loop: sample in front, KL elements and the free-bits reductions behind (tolerances of
    tests/test_hip_f16x2.py)"""
    params, p32, _ = case
    B, kl_min = 2, 0.25
    rng = np.random.RandomState(310 + H)
    f = lambda c: rng.standard_normal((B, c, H, H))
    qm, ql, rm, rl, pm, pl = f(N_Z), 0.25 * f(N_Z), f(N_Z), 0.25 * f(N_Z), f(N_Z), 0.25 * f(N_Z)
    uc, dc, eps = f(N_H), f(N_H), f(N_Z)
    st = _stack(amd, params, "f16x2")
    assert st.step_is_f16(B, H, H)
    out = st.posterior_block(dev(qm), dev(ql), dev(rm), dev(rl), dev(pm), dev(pl), dev(uc), dev(dc), dev(eps), kl_min, want_kl_elem=True)
    e = O.posterior_block(f32(qm), f32(ql), f32(rm), f32(rl), f32(pm), f32(pl), f32(uc), f32(dc), f32(eps), p32, [N_H] * D, kl_min)
    np.testing.assert_allclose(host(out["z"]), e["z"], atol=1e-4, rtol=0)
    ekl = e["logqs"] - e["logps"]
    np.testing.assert_allclose(host(out["kl_elem"]), ekl, atol=1e-4, rtol=1e-5)
    np.testing.assert_allclose(host(out["kl_cost"]), ekl.sum(axis=(1, 2, 3)), atol=2e-3, rtol=1e-4)
    kl_obj = np.tile(np.maximum(ekl.sum(axis=(2, 3)).mean(axis=0, keepdims=True), kl_min), (B, 1)).sum(axis=1)
    np.testing.assert_allclose(host(out["kl_obj"]), kl_obj, atol=2e-3, rtol=1e-4)
    assert st.range_errors() == 0 and st.exchange_errors() == 0


def _saved_hidden(st, P):
    """the hidden activations a training forward keeps: pixel-major [P][n_h] per layer, at the head of the training workspace"""
    torch.cuda.synchronize()
    ws = st._train_ws.view(torch.float32)
    n = (P * N_H + 63) // 64 * 64
    return [ws[l * n: l * n + P * N_H].reshape(P, N_H).cpu().numpy().astype(np.float64) for l in range(D)]


@pytest.mark.parametrize("H", [8, 16])
def test_training_forward_saves_the_hidden_activations_of_the_layerwise_path(amd, case, H):
    """posterior_block_train: the epilogue's stores for the backward pass left the per-unit loop.  What they write equals what the same
    stack saves layer by layer (set_fuse_step("never")) within the gate of the step: each against fp64, the fp16-plane launch at most
    1.5 x the exact-fp32 kernels' error and below 1e-4"""
    params, p32, _ = case
    B, kl_min = 2, 0.25
    P = B * H * H
    rng = np.random.RandomState(330 + H)
    f = lambda c: rng.standard_normal((B, c, H, H))
    qm, ql, rm, rl, pm, pl = f(N_Z), 0.25 * f(N_Z), f(N_Z), 0.25 * f(N_Z), f(N_Z), 0.25 * f(N_Z)
    uc, dc, eps = f(N_H), f(N_H), f(N_Z)
    args = [dev(a) for a in (qm, ql, rm, rl, pm, pl, uc, dc, eps)]
    # fp64 hidden activations (tf_train.py:57-63, layers.py:158-165), pixel-major
    z0 = (f32(qm) + f32(rm)) + np.exp(f32(ql) + f32(rl)) * f32(eps)
    want, x = [], z0
    for l in range(D):
        q = "layer_%d/" % l
        x = O.ar_conv2d(x, p32[q + "V"], p32[q + "g"], p32[q + "b"], zerodiagonal=False)
        x = O.elu(x + (f32(uc) + f32(dc)) if l == 0 else x)
        want.append(x.transpose(0, 2, 3, 1).reshape(P, N_H))
    got = {}
    for name, prec, fuse in (("one launch", "f16x2", "always"), ("layer by layer", "f16x2", "never"), ("exact fp32", "f32", "never")):
        st = _stack(amd, params, prec, training=True, fuse=fuse)
        if fuse == "always":
            assert st.step_is_f16(B, H, H)
        out = st.posterior_block_train(*args, kl_min)
        got[name] = _saved_hidden(st, P)
        if name == "one launch":
            z_fused = host(out["z"])
            assert st.range_errors() == 0 and st.exchange_errors() == 0
    for l in range(D):
        err = {k: np.abs(v[l] - want[l]).max() for k, v in got.items()}
        print("%dx%d hidden layer %d: max |. - fp64|: %s" % (H, H, l, ", ".join("%s %.3g" % kv for kv in err.items())))
        assert err["one launch"] <= 1.5 * err["exact fp32"], (l, err)
        assert err["one launch"] < 1e-4
        assert np.abs(got["one launch"][l] - got["layer by layer"][l]).max() < 1e-4
    e = O.posterior_block(f32(qm), f32(ql), f32(rm), f32(rl), f32(pm), f32(pl), f32(uc), f32(dc), f32(eps), p32, [N_H] * D, kl_min)
    np.testing.assert_allclose(z_fused, e["z"], atol=1e-4, rtol=0)


def test_raw_outputs_and_inverse_sweeps_at_8x8(amd, case):
    """the two other bodies of the final loop: MODE_RAW (m_raw, s_raw as they leave the output pair) and the Jacobi sweeps of the inverse
    flow, which converge on the z0 the fp64 oracle maps to z"""
    params, _, data = case
    B, H = 2, 8
    d = data[H]
    z0, ctx = d["z"][:B], d["ctx"][:B]
    st = _stack(amd, params, "f16x2")
    assert st.step_is_f16(B, H, H)
    m, s = st.ar_multiconv2d(dev(z0), dev(ctx))
    # (raw outputs are ten times the step's m and s: the step's bound of 1e-4 on 0.1 m_raw)
    assert np.abs(host(m) - d["m_raw"][:B]).max() < 1e-3 and np.abs(host(s) - d["s_raw"][:B]).max() < 1e-3
    back, logsd, sweeps, res = st.iaf_step_inverse(dev(d["z_new"][:B]), dev(ctx), max_sweeps=200, tol=1e-6, check_every=2)
    assert res <= 1e-6 and sweeps < 60, (sweeps, res)
    np.testing.assert_allclose(host(back), f32(z0), atol=1e-4, rtol=0)
    np.testing.assert_allclose(host(logsd), d["logsd"][:B], atol=1e-4, rtol=0)
    assert st.range_errors() == 0 and st.exchange_errors() == 0


@pytest.mark.parametrize("H", [8, 16])
def test_two_replays_of_a_graph_of_three_steps_are_bit_equal(amd, case, H):
    params, _, data = case
    B = 3
    d = data[H]
    st = _stack(amd, params, "f16x2")
    assert st.step_is_f16(B, H, H)
    ctx = dev(d["ctx"][:B])
    zs = [dev(d["z"][:B])] + [torch.empty(B, N_Z, H, H, device="cuda") for _ in range(3)]
    ls = [torch.empty(B, N_Z, H, H, device="cuda") for _ in range(3)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for i in range(3):                                    # warm-up on the capture stream: its own exchange set
            st.iaf_step(zs[i], ctx, out=(zs[i + 1], ls[i]))
        side.synchronize()
        assert st.exchange_errors() == 0 and st.range_errors() == 0
        first = [t.clone() for t in zs[1:] + ls]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for i in range(3):
                st.iaf_step(zs[i], ctx, out=(zs[i + 1], ls[i]))
    runs = []
    for _ in range(2):
        for t in zs[1:] + ls:
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert st.exchange_errors() == 0 and st.range_errors() == 0
        runs.append([t.clone() for t in zs[1:] + ls])
    for a, b, c in zip(runs[0], runs[1], first):
        assert torch.equal(a, b) and torch.equal(a, c)
    # the first of the three steps against fp64
    assert np.abs(host(runs[0][0]) - d["z_new"][:B]).max() < 1e-4
