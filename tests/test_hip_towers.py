"""GPU tests of the towers feature (free bits per row group, include/iaf_hip.h: iaf_stack_set_free_bits_groups,
iaf_kl_free_bits_grouped): the leaf entry point against the fp64 statement per group (tests/towers_reference.py), the posterior
block on each of its reduction routes, its backward against torch-fp64 autograd composed per tower, CVAE1(towers=2) against the
reference's own _forward per tower (tests/golden/cvae1_towers.npz) and the per-tower oracle gradients, and TrainStep on a model
with towers against the hand-composed step with divisor world * towers."""
import math
import os

import numpy as np
import pytest
import torch

import golden_inputs as gi
import objective_reference as R
import towers_reference as T
from oracle import iaf_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
FINISH_LAUNCH = 16      # test knob of iaf_stack_set_halo_exchange_debug: the reductions by iaf_kl_finish_kernel even where the step's launch can do them
LR = 2e-3


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


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def abi(amd):
    return amd._capi.lib(), amd.layers._ptr, amd.layers._stream, amd._capi.check


f32 = R.f32


def _check_grouped(tag, obj, cost, kl, kl_min, d_row, groups):
    """kl_cost and kl_obj against the fp64 statement per group on kl [B, C, HW] within the derived bounds (B := G)"""
    ref, bound = T.free_bits_grouped(kl, kl_min, groups), T.free_bits_grouped_bounds(kl, kl_min, d_row, groups)
    assert np.isfinite(obj).all() and np.isfinite(cost).all()
    r_cost = float((np.abs(cost - ref["kl_cost"]) / bound["kl_cost"]).max())
    r_obj = float((np.abs(obj - ref["kl_obj"]) / bound["kl_obj"]).max())
    print("%s: kl_cost error / bound %.3f, kl_obj error / bound %.3f" % (tag, r_cost, r_obj))
    assert r_cost <= 1.0 and r_obj <= 1.0, (r_cost, r_obj)
    return ref


# ---- 1. the leaf entry point -------------------------------------------------------------------------------------------------
def _grouped(amd, kl, kl_min, groups, want_gate):
    lib, P, st, check = abi(amd)
    B, C, HW = kl.shape
    kd, obj, cost, scratch = dev(kl), nans(B), nans(B), nans(B * C)
    gate = nans(groups, C) if want_gate else None
    check(lib.iaf_kl_free_bits_grouped(P(kd), P(obj), P(cost), P(gate), B, C, HW, groups, kl_min, P(scratch), st()))
    return host(obj), host(cost), (host(gate) if want_gate else None)


@pytest.mark.parametrize("shape", T.FBG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kl_free_bits_grouped(amd, shape):
    """iaf_kl_free_bits_grouped against fp64 per group: the bounds of the one-batch entry points with B := G; the gate exactly (every
    mean is further from kl_min than its bound: tests/test_towers_reference.py); kl_min = 0; one group = iaf_kl_free_bits_gate bit
    for bit; a batch the groups do not divide is refused"""
    lib, P, st, check = abi(amd)
    B, C, HW, groups = shape
    kl = T.fbg_case(shape)
    d_row = R.fb_d_row(HW)
    obj0, cost0, _ = _grouped(amd, kl, 0.0, groups, False)
    _check_grouped("grouped free bits %s kl_min 0" % (shape,), obj0, cost0, kl, 0.0, d_row, groups)
    assert np.array_equal(obj0, cost0)                              # tf_train.py:84: the same sum
    obj, cost, gate = _grouped(amd, kl, T.KL_MIN, groups, True)
    ref = _check_grouped("grouped free bits %s kl_min %.2f" % (shape, T.KL_MIN), obj, cost, kl, T.KL_MIN, d_row, groups)
    assert np.array_equal(cost, cost0)
    assert np.array_equal(gate, ref["gate"])
    assert (gate[1:] != gate[:-1]).all()                            # the case's point: the groups' gates differ
    G = B // groups
    for r in range(groups):
        assert (obj[r * G:(r + 1) * G] == obj[r * G]).all()         # one value per group (:81)
    plain = _grouped(amd, kl, T.KL_MIN, groups, False)              # without a gate: the same numbers
    assert np.array_equal(plain[0], obj) and np.array_equal(plain[1], cost)
    # one group: the one-batch entry point, bit for bit
    one = _grouped(amd, kl, T.KL_MIN, 1, True)
    kd, o1, c1, g1, scratch = dev(kl), nans(B), nans(B), nans(C), nans(B * C)
    check(lib.iaf_kl_free_bits_gate(P(kd), P(o1), P(c1), P(g1), B, C, HW, T.KL_MIN, P(scratch), st()))
    assert np.array_equal(one[0], host(o1)) and np.array_equal(one[1], host(c1)) and np.array_equal(one[2][0], host(g1))
    # groups that do not divide B, and groups out of range
    for bad in (B + 1, 0, 65):
        if bad == 0 or bad > 64 or B % bad:
            assert lib.iaf_kl_free_bits_grouped(P(kd), P(o1), P(c1), None, B, C, HW, bad, T.KL_MIN, P(scratch), st()) == amd._capi.IAF_ERR_SHAPE
    torch.cuda.synchronize()


# ---- 2. the posterior block's routes ------------------------------------------------------------------------------------------
def _block_inputs(seed, B, n_z, n_h, H, W, groups):
    """small posterior / prior offsets, growing from group to group: at kl_min = 0.25 channels fall on both sides of the free-bits max
    and the groups' gates differ"""
    rng = np.random.RandomState(seed)
    G = B // groups
    grow = np.repeat(1.0 + 0.75 * np.arange(groups), G).reshape(B, 1, 1, 1)
    f = lambda c, sc=1.0, g=False: f32(sc * (grow if g else 1.0) * rng.standard_normal((B, c, H, W)))
    return dict(qm=f(n_z, 0.1, True), ql=f(n_z, 0.05), rm=f(n_z, 0.1, True), rl=f(n_z, 0.05), pm=f(n_z, 0.1, True), pl=f(n_z, 0.05),
                uc=f(n_h), dc=f(n_h), eps=f(n_z, 0.05))


ORDER = ("qm", "ql", "rm", "rl", "pm", "pl", "uc", "dc", "eps")


def _forward(amd, stack, di, kl_min, B, n_z, H, W):
    lib, P, st, check = abi(amd)
    z, obj, cost, kl_elem = nans(B, n_z, H, W), nans(B), nans(B), nans(B, n_z, H, W)
    ws, need = stack.workspace(B, H, W, z.device)
    a = [P(di[k]) for k in ORDER]
    check(lib.iaf_posterior_block_forward(stack._h, *a, kl_min, P(z), P(obj), P(cost), P(kl_elem), B, H, W, P(ws), need, st()))
    torch.cuda.synchronize()
    return z, obj, cost, host(kl_elem).reshape(B, n_z, H * W)


_params = {}


def _stack(amd, n_z, n_h, depth, groups, knob=0, training=False):
    key = (n_z, n_h, depth)
    if key not in _params:
        _params[key] = {k: dev(v) for k, v in gi.ar_multiconv2d_params(np.random.RandomState(71), n_z, [n_h] * depth, [n_z, n_z]).items()}
    stack = amd.ARStack(n_z, [n_h] * depth)
    if knob:
        stack.set_halo_exchange_debug(knob)
    if training:
        stack.set_training(True)
    stack.set_free_bits_groups(groups)
    assert stack.free_bits_groups() == groups
    stack.prepare(_params[key])
    return stack


@pytest.mark.parametrize("B,H,groups", [(4, 8, 2), (4, 8, 4), (6, 8, 3), (4, 16, 2), (4, 16, 4), (6, 16, 3), (72, 16, 8)],
                         ids=lambda v: str(v))
def test_posterior_block_groups_on_the_one_launch_step(amd, B, H, groups):
    """n_z 32 / n_h 160 / depth 2 (BASELINE): as shipped -- the step's own launch finishes the reductions, one launch -- and with the
    test knob that hands them to iaf_kl_finish_kernel: bit-identical to each other, inside the per-group bound of the posterior block
    (tests/test_hip_objective_kernels.py: H W + 16 additions inside a row sum) on the kl_elem the same call returned, and the training
    forward returns the same bits.  B = 72 at 16x16: 18432 partial sums, the many-workgroup sum over the row blocks in front of the
    finish launch on either setting."""
    n_z, n_h, depth, W = 32, 160, 2, H
    inp = _block_inputs(300 + B + H + groups, B, n_z, n_h, H, W, groups)
    di = {k: dev(v) for k, v in inp.items()}
    res = []
    for knob, route in ((0, "as shipped"), (FINISH_LAUNCH, "finish launch")):
        stack = _stack(amd, n_z, n_h, depth, groups, knob)
        rows = stack.step_is_fused(B, H, W)
        assert rows > 0
        nrb = -(-H // rows)
        if B * nrb * n_z <= 16384 and knob == 0:
            assert "1 launch" in stack.posterior_block_launches(B, H, W)
        elif B * nrb * n_z > 16384:
            assert "2 KL reduction" in stack.posterior_block_launches(B, H, W)
        for kl_min in (T.KL_MIN, 0.0):
            z, obj, cost, kl = _forward(amd, stack, di, kl_min, B, n_z, H, W)
            assert stack.exchange_errors() == 0
            ref = _check_grouped("posterior block B=%d %dx%d groups %d kl_min %.2f, %s" % (B, H, W, groups, kl_min, route), host(obj),
                                 host(cost), kl, kl_min, H * W + 16, groups)
            if kl_min > 0:
                g = ref["gate"]
                print("    channels above kl_min per group: %s of %d" % (g.sum(axis=1).astype(int).tolist(), n_z))
                assert g.any() and not g.all() and (g[0] != g[-1]).any()
            else:
                assert torch.equal(obj, cost)
            res.append((z, obj, cost))
    for a, b in zip(res[:2], res[2:]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))         # the two routes: the same bits
    tr = _stack(amd, n_z, n_h, depth, groups, training=True)
    out = tr.posterior_block_train(*[di[k] for k in ORDER], T.KL_MIN)
    torch.cuda.synchronize()
    assert torch.equal(out["z"], res[0][0]) and torch.equal(out["kl_obj"], res[0][1]) and torch.equal(out["kl_cost"], res[0][2])
    # a batch the groups do not divide
    if (B + 1) % groups:
        bad = {k: dev(np.concatenate([v, v[:1]])) for k, v in inp.items()}
        with pytest.raises(ValueError):
            stack.posterior_block(*[bad[k] for k in ORDER], T.KL_MIN)
        with pytest.raises(ValueError):
            tr.posterior_block_train(*[bad[k] for k in ORDER], T.KL_MIN)


def test_posterior_block_groups_on_the_generic_path(amd):
    """n_z 24 / n_h 72 (no multiple of 16: the direct-conv kernels, row sums + finish launch), B = 4, 4x4, two groups"""
    B, n_z, n_h, depth, H, W, groups = 4, 24, 72, 2, 4, 4, 2
    inp = _block_inputs(340, B, n_z, n_h, H, W, groups)
    di = {k: dev(v) for k, v in inp.items()}
    stack = _stack(amd, n_z, n_h, depth, groups)
    assert stack.step_is_fused(B, H, W) == 0
    z, obj, cost, kl = _forward(amd, stack, di, T.KL_MIN, B, n_z, H, W)
    ref = _check_grouped("generic posterior block", host(obj), host(cost), kl, T.KL_MIN, R.fb_d_row(H * W), groups)
    assert (ref["gate"][0] != ref["gate"][1]).any()
    tr = _stack(amd, n_z, n_h, depth, groups, training=True)
    out = tr.posterior_block_train(*[di[k] for k in ORDER], T.KL_MIN)
    torch.cuda.synchronize()
    assert torch.equal(out["kl_obj"], obj) and torch.equal(out["kl_cost"], cost)


def test_theano_stacks_refuse_groups(amd):
    stack = amd.ARStack(32, [64], variant="theano")
    stack.set_free_bits_groups(1)
    with pytest.raises(amd._capi.UnsupportedError):
        stack.set_free_bits_groups(2)
    assert stack.free_bits_groups() == 1


# ---- 3. the backward -----------------------------------------------------------------------------------------------------------
def _rel_close(got, ref, tol, name):
    scale = max(np.abs(ref).max(), 1e-6)
    err = np.abs(got - ref).max() / scale
    print("    %s: max err / max|ref| = %.3g" % (name, err))
    assert err < tol, "%s: max err / max|ref| = %.3g (tol %g)" % (name, err, tol)


@pytest.mark.parametrize("shape", [(4, 2, 32, 160, 2, 8, 8), (6, 3, 32, 160, 2, 16, 16), (4, 2, 24, 72, 2, 4, 4)],
                         ids=lambda s: "B%d_groups%d_z%d_h%d_d%d_%dx%d" % s)
def test_posterior_block_backward_per_group_vs_autograd_oracle(amd, shape):
    """iaf_posterior_block_backward with groups: every input gradient against torch-fp64 autograd of the restated forward run per
    tower (a tower = one group's rows), the weight gradients against the sum over the towers; random dkl_obj per row; the bounds of
    tests/test_hip_parity.py's posterior-block backward test.  The last shape is generic (the direct-conv kernels)."""
    from oracle import iaf_grad_oracle as G
    B, groups, n_z, n_h, d, H, W = shape
    Gr = B // groups
    rng = np.random.RandomState(67 + B)
    params = gi.ar_multiconv2d_params(rng, n_z, [n_h] * d, [n_z, n_z])
    p32 = {k: f32(v) for k, v in params.items()}
    # (seeds picked on the CPU oracle: every group's channel means stay 0.02 or more away from kl_min, asserted below -- the fp32 gate
    # is then the fp64 gate)
    inp = _block_inputs({8: 354, 16: 361, 4: 360}[H], B, n_z, n_h, H, W, groups)
    dz, dko = f32(rng.standard_normal((B, n_z, H, W))), f32(1.0 + 0.3 * rng.standard_normal(B))
    stack = amd.ARStack(n_z, [n_h] * d)
    stack.set_training(True)
    stack.set_free_bits_groups(groups)
    dp = {k: dev(v) for k, v in params.items()}
    stack.prepare(dp)
    di = {k: dev(v) for k, v in inp.items()}
    fw = stack.posterior_block_train(*[di[k] for k in ORDER], T.KL_MIN)
    bw = stack.posterior_block_backward(di["qm"], di["ql"], di["rm"], di["rl"], di["pm"], di["pl"], di["eps"], T.KL_MIN, fw["z"],
                                        dev(dz), dev(dko), dp)
    refs, gates = [], []
    for r in range(groups):
        rows = slice(r * Gr, (r + 1) * Gr)
        refs.append(G.posterior_block_grads({k: v[rows] for k, v in inp.items()}, p32, [n_h] * d, T.KL_MIN, dz[rows], dko[rows]))
        e = O.posterior_block(*[inp[k][rows] for k in ORDER], p32, [n_h] * d, T.KL_MIN)
        mean_c = (e["logqs"] - e["logps"]).sum(axis=(2, 3)).mean(axis=0)
        assert np.abs(mean_c - T.KL_MIN).min() > 0.02
        gates.append(mean_c > T.KL_MIN)
    gates = np.stack(gates)
    print("    channels above kl_min per group: %s of %d" % (gates.sum(axis=1).tolist(), n_z))
    assert gates.any() and not gates.all() and (gates[0] != gates[-1]).any()
    cat = lambda k: np.concatenate([ref[0][k] for ref in refs], axis=0)
    np.testing.assert_allclose(host(fw["z"]), np.concatenate([ref[1] for ref in refs]), atol=1e-4, rtol=0)
    np.testing.assert_allclose(host(fw["kl_obj"]), np.concatenate([ref[2] for ref in refs]), atol=2e-3, rtol=1e-4)
    np.testing.assert_allclose(host(fw["kl_cost"]), np.concatenate([ref[3] for ref in refs]), atol=2e-3, rtol=1e-4)
    _rel_close(host(bw["dmean"]), cat("qm"), 2e-4, "d qz_mean")
    _rel_close(host(bw["dmean"]), cat("rm"), 2e-4, "d rz_mean")
    _rel_close(host(bw["dlogsd"]), cat("ql"), 2e-4, "d qz_logsd")
    _rel_close(host(bw["dlogsd"]), cat("rl"), 2e-4, "d rz_logsd")
    _rel_close(host(bw["dpz_mean"]), cat("pm"), 2e-4, "d pz_mean")
    _rel_close(host(bw["dpz_logsd"]), cat("pl"), 2e-4, "d pz_logsd")
    _rel_close(host(bw["dcontext"]), cat("uc"), 2e-4, "d up_context")
    _rel_close(host(bw["dcontext"]), cat("dc"), 2e-4, "d down_context")
    for k in sorted(params):
        _rel_close(host(bw["grads"][k]), sum(ref[0][k] for ref in refs), 3e-4, k)


# ---- 4. the model --------------------------------------------------------------------------------------------------------------
def _model(amd, c, params, towers=T.N_TOWERS, training=False):
    model = amd.CVAE1(z_size=c["z_size"], h_size=c["h_size"], kl_min=c["kl_min"], depth=c["depth"], num_blocks=c["num_blocks"], k=1,
                      image_size=c["image_size"], towers=towers)
    if training:
        model.set_training(True)
    model.load({k: dev(v) if isinstance(v, np.ndarray) else v.clone() for k, v in params.items()})
    return model


def test_cvae1_towers_forward_vs_the_references_own_forward_per_tower(amd, golden_dir):
    """CVAE1(towers=2).forward on the towers' rows as one batch against the reference's _forward run per tower on the TF shim: x_out
    per row, obj = the sum of the towers' objectives, loss, bits/dim as tf_train.py:142; with the bounds of tests/test_hip_model.py.
    The same rows through a model without towers give the one-batch objective, which the fixture's inputs keep far away."""
    g = np.load(os.path.join(golden_dir, "cvae1_towers.npz"))
    c = gi.model_case_inputs(T.TOWERS_CASE)
    x, noise = T.towers_batch()
    xd, nd = torch.from_numpy(x).cuda(), [dev(e) for e in noise]
    model = _model(amd, c, c["params"])
    assert model.towers == T.N_TOWERS and all(l.posterior.stack.free_bits_groups() == T.N_TOWERS for lv in model.layers for l in lv)
    x_out, obj, loss = model.forward(xd, nd)
    want_x = np.concatenate([g["tower%d/x_out" % t] for t in range(T.N_TOWERS)], axis=0)
    want_obj = sum(float(g["tower%d/obj" % t]) for t in range(T.N_TOWERS))
    want_loss = sum(float(g["tower%d/loss" % t]) for t in range(T.N_TOWERS))
    np.testing.assert_allclose(host(x_out), want_x, rtol=0, atol=2e-4)
    print("obj %.6f (towers' sum %.6f), loss %.6f (%.6f)" % (host(obj)[0], want_obj, host(loss)[0], want_loss))
    np.testing.assert_allclose(host(obj)[0], want_obj, rtol=2e-5)
    np.testing.assert_allclose(host(loss)[0], want_loss, rtol=2e-5)
    np.testing.assert_allclose(model.bits_per_dim(host(loss)[0], c["B"] * T.N_TOWERS), g["bits_per_dim"], rtol=2e-5)
    plain = _model(amd, c, c["params"], towers=1)
    _, obj1, loss1 = plain.forward(xd, nd)
    assert abs(host(obj1)[0] - want_obj) > 100 * 2e-5 * want_obj
    np.testing.assert_allclose(host(loss1)[0], want_loss, rtol=2e-5)
    with pytest.raises(ValueError):
        model.forward(xd[:3].contiguous(), [e[:3].contiguous() for e in nd])
    model3 = _model(amd, c, c["params"], towers=3)
    with pytest.raises(ValueError):
        model3.forward(xd, nd)


def test_cvae1_towers_forward_backward_vs_the_per_tower_oracle(amd):
    """d obj / d every variable: the sum over the towers of torch-fp64 autograd of the restated forward on each tower's rows
    (opt.compute_gradients per tower, average_grads' sum, tf_train.py:138, 146), with the bound of tests/test_hip_model.py's
    gradient test"""
    from oracle import iaf_grad_oracle as G
    c = gi.model_case_inputs(T.TOWERS_CASE)
    p32 = {k: f32(v) for k, v in c["params"].items()}
    want, want_obj = None, 0.0
    for t in range(T.N_TOWERS):
        x, noise = T.tower_inputs(t)
        gr, _, o = G.cvae1_grads(x, p32, c["z_size"], c["h_size"], c["depth"], c["num_blocks"], c["kl_min"], [f32(e) for e in noise])
        want = gr if want is None else {k: want[k] + gr[k] for k in want}
        want_obj += float(o)
    x, noise = T.towers_batch()
    model = _model(amd, c, c["params"], training=True)
    x_out, obj, grads = model.forward_backward(torch.from_numpy(x).cuda(), [dev(e) for e in noise])
    np.testing.assert_allclose(host(obj)[0], want_obj, rtol=2e-5)
    assert set(grads) == set(want)
    worst = (0.0, None)
    for k in sorted(want):
        got, w = host(grads[k]), want[k]
        err = float(np.abs(got - w).max() / (np.abs(w).max() + 1e-3))
        worst = max(worst, (err, k))
        assert err < 2e-3, (k, err, float(np.abs(w).max()))
    print("worst relative gradient error %.2e (%s)" % worst)


# ---- 5. TrainStep ---------------------------------------------------------------------------------------------------------------
def _step_inputs(step):
    """step 0: the towers' batch; step 1: the towers swapped (every group's gates change); step 2: another mix"""
    x, noise = T.towers_batch()
    B = x.shape[0] // T.N_TOWERS
    sh = (0, B, 1)[step]
    return torch.from_numpy(np.roll(x, sh, axis=0)).cuda(), [dev(np.roll(e, sh, axis=0) * (1.0 + 0.05 * step)) for e in noise]


def test_train_step_with_towers_equals_the_hand_composed_step(amd):
    """a towers = 2 model in graph mode, three steps on different inputs: bit-identical to prepare_weights -> forward_backward ->
    FlatParams.adamax_ema_step(world = world * towers = 2) on a second model; the summaries' bits/dim is the steps' mean of
    loss / (ln 2 * 3 S^2 * 2 B) (tf_train.py:142)"""
    import iaf_amd.parallel as par
    c = gi.model_case_inputs(T.TOWERS_CASE)
    ts = amd.TrainStep(_model(amd, c, c["params"], training=True), LR, graph=True, summaries=True)
    assert ts.towers == T.N_TOWERS and ts.world == 1
    hm = _model(amd, c, c["params"], training=True)
    flat = par.FlatParams({k: hm.params[k] for k in hm.completion_order()})
    hm.load(flat.p)
    S, n = c["image_size"], c["B"] * T.N_TOWERS
    bpd = []
    for step in range(3):
        x, noise = _step_inputs(step)
        obj = ts(x, noise)
        hm.prepare_weights()
        _, _, loss = hm.forward(x, noise)
        bpd.append(float(loss.item()) / (math.log(2.) * 3 * S * S * n))
        _, want, _ = hm.forward_backward(x, noise, grads=flat.g)
        flat.adamax_ema_step(LR, world=T.N_TOWERS)
        torch.cuda.synchronize()
        assert torch.equal(obj, want), (step, float(obj.item()), float(want.item()))
        for k in ("grads", "params", "slot_m", "slot_v", "ema"):
            a, b = getattr(ts.flat, k), getattr(flat, k)
            assert torch.equal(a, b), (step, k, float((a - b).abs().max()))
    assert ts.skipped == 0 and ts.graphed and ts.graph_refused is None
    s = ts.summaries()
    print("bits/dim %.8f, by hand %.8f" % (s["model/bits_per_dim"], float(np.mean(bpd))))
    assert s["steps"] == 3
    np.testing.assert_allclose(s["model/bits_per_dim"], np.mean(bpd), rtol=2e-6)
