"""The backward pass over awkward geometry: the counterpart of the forward sweep in test_hip_fuzz.py for the training kernels.

The backward host code chooses kernels and splits work from P = B H W, W, c_in and c_out (wgrad_plan / launch_wgrad / iaf_step_backward in
iaf_engine.hip, iaf_conv3x3_backward / conv3x3_bf3_shape in iaf_conv3x3_host.hpp).  The case tables in tests/backward_plan_reference.py put a
case into every class of that plan -- every compiled weight-gradient kernel shape, empty and ragged pixel ranges, both sides of every
threshold of the range count, of the split-precision kernels and of the bias-gradient slabs, and the images whose taps see only padding --
and tests/test_backward_plan_reference.py proves on the CPU that they do.  Here every gradient of every case is compared with torch-fp64
autograd of the restated forward (oracle/iaf_grad_oracle.py) on the fp32-rounded inputs.

Metric and bounds are those of the existing backward tests for the same quantities (test_hip_layer.py, test_hip_parity.py,
test_hip_generic_backward.py): max|got - want| / max|want| below 1e-4 for a plain conv and for the stack's data gradients, 2e-4 for the stack's
parameter gradients, 2e-4 / 3e-4 for the posterior block; a split-precision path within 2 x the exact-fp32 path's error + 1e-6 on the same
inputs.  A quantity whose reference is identically zero must be exactly zero."""
import collections

import numpy as np
import pytest
import torch

import backward_plan_reference as R
import golden_inputs as gi
from oracle import iaf_oracle as O

pytestmark = pytest.mark.gpu
ATOL = 1e-4
WORST = collections.defaultdict(float)          # (family, precision, quantity) -> worst relative error seen


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()
    yield iaf_amd
    for key in sorted(WORST):
        print("worst rel err  %-10s %-7s %-10s %.3g" % (key + (WORST[key],)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _relerr(got, want, key=None):
    """max|got - want| / max|want|; a reference that is identically zero asks for exact zeros"""
    scale = np.abs(want).max() if want.size else 0.0
    if scale < 1e-30:
        assert np.count_nonzero(got) == 0, "the reference is identically zero, the GPU value is not"
        return 0.0
    err = np.abs(got - want).max() / scale
    assert np.isfinite(got).all()
    if key is not None:
        WORST[key] = max(WORST[key], err)
    return err


def _close(got, want, tol, name, key=None):
    err = _relerr(got, want, key)
    assert err < tol, "%s: max err / max|ref| = %.3g (tol %g)" % (name, err, tol)
    return err


# ---------------------------------------------------------------- a. plain conv, WNConv2d.backward
def _conv_inputs(case, seed):
    B, ci, co, H, W = case[:5]
    rng = np.random.RandomState(seed)
    p = gi.conv_params(rng, ci, co)
    return p, rng.standard_normal((B, ci, H, W)), rng.standard_normal((B, co, H, W)), rng.standard_normal((B, ci, H, W))


def _conv_reference(p, x, dy, elu, scale):
    """fp64 autograd of L = <dy, scale * conv2d([elu](x))> (layers.py:52-64) in slices of the batch (memory): dx, dV, dg, db"""
    from oracle import iaf_grad_oracle as G
    pt = {k: G._t(f32(v), True) for k, v in p.items()}
    B, _, H, W = x.shape
    chunk = max(1, 4096 // (H * W))
    gx = []
    for b0 in range(0, B, chunk):
        xs = G._t(f32(x[b0:b0 + chunk]), True)
        y = scale * G.conv2d(torch.nn.functional.elu(xs) if elu else xs, pt["V"], pt["g"], pt["b"])
        (y * G._t(f32(dy[b0:b0 + chunk]))).sum().backward()
        gx.append(xs.grad.numpy())
    return dict(dx=np.concatenate(gx), dV=pt["V"].grad.numpy(), dg=pt["g"].grad.numpy(), db=pt["b"].grad.numpy())


def _conv_backward(amd, case, prec, p, x, dy, res, forms):
    """one WNConv2d.backward in the surrounding form `forms` (e elu, x split input, y split dys, s dy_scale 0.1, r residual, n no dx)"""
    B, ci, co, H, W = case[:5]
    conv = amd.WNConv2d(ci, co)
    conv.set_precision(prec)
    conv.set_training(True)
    V, g, b = dev(p["V"]), dev(p["g"]), dev(p["b"])
    conv.prepare(V, g, b)
    xd, dyd = dev(x), dev(dy)
    x1, x2 = xd, None
    if "x" in forms:
        split = ci // 2 // 4 * 4
        x1, x2 = xd[:, :split].contiguous(), xd[:, split:].contiguous()
    dys = [dyd]
    if "y" in forms:
        half = co // 2 // 4 * 4
        dys = [dyd[:, :half].contiguous(), dyd[:, half:].contiguous()]
    resd = dev(res) if "r" in forms else None
    # the scratch buffer holds NaN before the call: a range partial or a bias slab that the plan counts and no workgroup writes
    # (an empty trailing range, an empty slab) shows in the sums instead of passing on whatever an earlier call left there
    need = int(amd._capi.lib().iaf_conv3x3_train_workspace_bytes(conv._h, B, H, W))
    ws = amd.WNConv2d._shared_ws.get(xd.device)
    if ws is None or ws.numel() * 4 < need:
        ws = amd.WNConv2d._shared_ws[xd.device] = torch.empty((need + 3) // 4, dtype=torch.float32, device=xd.device)
    ws.fill_(float("nan"))
    dxs, dV, dg, db = conv.backward(x1, dys, V, g, x2=x2, elu_input="e" in forms, dy_scale=0.1 if "s" in forms else 1.0,
                                    want_dx="n" not in forms, dx_residual=resd)
    torch.cuda.synchronize()
    out = dict(dV=host(dV), dg=host(dg), db=host(db), raw_dx=dxs)
    if "n" in forms:
        assert dxs is None
    else:
        out["dx"] = [host(d) - host(resd) if resd is not None else host(d) for d in dxs]      # one per input part
    if prec != "f32":
        assert conv.range_errors() == 0
    return out


@pytest.mark.parametrize("case", R.CONV_CASES, ids=R.conv_id)
def test_wnconv2d_backward_geometry(amd, case):
    """dx (each part), dV, dg, db of a plain conv at every class of launch plan, in the surrounding forms the API has, at "f32" and -- where
    a split kernel can take part of the backward -- at "bf16x3" and "f16x2" (the id carries the fp32 plan; conv_labels gives the others)"""
    forms = case[5]
    p, x, dy, res = _conv_inputs(case, 4000 + R.CONV_CASES.index(case))
    want = _conv_reference(p, x, dy, "e" in forms, 0.1 if "s" in forms else 1.0)
    errs = {}
    for prec in R.conv_precisions(case):
        got = _conv_backward(amd, case, prec, p, x, dy, res, forms)
        errs[prec] = {q: _close(got[q], want[q], 1e-4, "%s %s" % (prec, q), ("conv", prec, q)) for q in ("dV", "dg", "db")}
        if "dx" in got:                           # each part against its own channels of the reference
            ends = np.cumsum([0] + [d.shape[1] for d in got["dx"]])
            assert ends[-1] == want["dx"].shape[1]
            errs[prec]["dx"] = max(_close(d, want["dx"][:, a:b], 1e-4, "%s dx[%d:%d]" % (prec, a, b), ("conv", prec, "dx"))
                                   for d, a, b in zip(got["dx"], ends[:-1], ends[1:]))
        print("%s %-6s %s" % (R.conv_id(case), prec, "  ".join("%s %.3g" % kv for kv in sorted(errs[prec].items()))))
    for prec in errs:
        if prec == "f32":
            continue
        for q in ("dx", "dV"):                   # what the split kernels compute: the data gradient and the weight gradient
            if q in errs[prec]:
                assert errs[prec][q] <= 2.0 * errs["f32"][q] + 1e-6, "%s %s: %.3g against exact fp32 %.3g" % (prec, q, errs[prec][q], errs["f32"][q])


# ---------------------------------------------------------------- b. single masked conv
@pytest.mark.parametrize("zerodiagonal", [False, True])
def test_single_masked_conv_has_no_backward(amd, zerodiagonal):
    """a single ar_conv2d object is forward only: iaf_conv3x3_set_training reports IAF_ERR_UNSUPPORTED for it (masked convs train inside
    an ARStack, family c), so there is no masked plain-conv backward to sweep"""
    conv = amd.WNConv2d(16, 32, ar_mask=zerodiagonal)
    assert amd._capi.lib().iaf_conv3x3_set_training(conv._h, 1) == amd._capi.IAF_ERR_UNSUPPORTED
    with pytest.raises(amd._capi.UnsupportedError):
        conv.set_training(True)


# ---------------------------------------------------------------- c. stack
def _stack_inputs(seed, n_z, n_h, d, B, H, W):
    rng = np.random.RandomState(seed)
    params = gi.ar_multiconv2d_params(rng, n_z, [n_h] * d, [n_z, n_z])
    f = lambda c: rng.standard_normal((B, c, H, W))
    return params, f(n_z), f(n_h), f(n_z), f(n_z)


def _poison_train_workspace(stack, z):
    """NaN in every word of the stack's training scratch before the forward: what the backward sums without having written it shows"""
    B, _, H, W = (int(v) for v in z.shape)
    ws, _ = stack._train_workspace(B, H, W, z.device)
    ws.fill_(0xFF)


def _stack_step(amd, prec, params, z, ctx, dzn, dls, n_z, n_h, d, check_forward=True):
    stack = amd.ARStack(n_z, [n_h] * d)
    if prec is not None:
        stack.set_precision(prec)
    stack.set_training(True)
    dp = {k: dev(v) for k, v in params.items()}
    stack.prepare(dp)
    zd, cd = dev(z), (dev(ctx) if d > 0 else None)
    _poison_train_workspace(stack, zd)
    z_new, logsd = stack.iaf_step_train(zd, cd)
    if check_forward:          # training forward == inference forward, bit for bit
        z_ref, l_ref = stack.iaf_step(zd, cd)
        assert torch.equal(z_new, z_ref) and torch.equal(logsd, l_ref)
    dz, dctx, grads = stack.iaf_step_backward(zd, cd, z_new, logsd, dev(dzn), dev(dls), dp)
    torch.cuda.synchronize()
    assert stack.exchange_errors() == 0
    return stack, dp, (zd, cd, z_new, logsd), dz, dctx, grads


def _masked_entries_are_zero(grads, params):
    for k in params:
        if k.endswith("/V"):                      # masked entries get exact zeros
            V = params[k]
            mask = O.get_conv_ar_mask(3, 3, V.shape[2], V.shape[3], k.startswith("layer_out"))
            assert torch.count_nonzero(grads[k][torch.from_numpy(mask == 0).cuda()]).item() == 0, k


@pytest.mark.parametrize("case", R.stack_cases(), ids=R.stack_id)
def test_stack_backward_geometry(amd, case):
    """dz, dcontext and every parameter gradient of ARStack.iaf_step_backward at the stack's default precision; where the data gradient's
    size rule takes the bf16x3 kernels, also at "f32", and the split data gradients within 2 x the exact path's error"""
    from oracle import iaf_grad_oracle as G
    seed, n_z, n_h, d, B, H, W = case
    params, z, ctx, dzn, dls = _stack_inputs(3000 + seed, n_z, n_h, d, B, H, W)
    p32 = {k: f32(v) for k, v in params.items()}
    ref, ez, es = G.iaf_step_grads(f32(z), f32(ctx), p32, [n_h] * d, f32(dzn), f32(dls))
    split_dx = any(R.stack_plan(B, H, W, n_z, n_h, d)["dgrad_split"])
    errs = {}
    for prec in ((None, "f32") if split_dx else (None,)):
        name = prec or "default"
        _, dp, (zd, cd, z_new, logsd), dz, dctx, grads = _stack_step(amd, prec, params, z, ctx, dzn, dls, n_z, n_h, d)
        np.testing.assert_allclose(host(z_new), ez, atol=ATOL, rtol=0)
        np.testing.assert_allclose(host(logsd), es, atol=ATOL, rtol=0)
        e = errs[name] = {"dz": _close(host(dz), ref["z"], 1e-4, "dz", ("stack", name, "dz"))}
        if d > 0:
            e["dcontext"] = _close(host(dctx), ref["context"], 1e-4, "dcontext", ("stack", name, "dcontext"))
        assert sorted(grads) == sorted(params)
        for k in sorted(params):
            e[k] = _close(host(grads[k]), ref[k], 2e-4, k, ("stack", name, "d" + k.split("/")[1]))
        _masked_entries_are_zero(grads, params)
        print("%s %-7s %s" % (R.stack_id(case), name, "  ".join("%s %.3g" % kv for kv in sorted(e.items()))))
    if split_dx:
        for q in ("dz", "dcontext"):
            if q in errs["default"]:
                assert errs["default"][q] <= 2.0 * errs["f32"][q] + 1e-6, "%s: %.3g against exact fp32 %.3g" % (q, errs["default"][q], errs["f32"][q])


def _theano_params(rng, name, n_z, n_h_list):
    w = {}
    sizes = [n_z] + n_h_list
    for i in range(len(n_h_list)):
        w["%s_%d_w" % (name, i)] = 0.05 * rng.standard_normal((sizes[i + 1], sizes[i] + 1, 3, 3))
        w["%s_%d_b" % (name, i)] = 0.1 * rng.standard_normal(sizes[i + 1])
        w["%s_%d_s" % (name, i)] = 0.1 * rng.standard_normal(sizes[i + 1])
    for i in range(2):
        w["%s_out_%d_w" % (name, i)] = 0.05 * rng.standard_normal((n_z, sizes[-1] + 1, 3, 3))
        w["%s_out_%d_b" % (name, i)] = 0.1 * rng.standard_normal(n_z)
        w["%s_out_%d_s" % (name, i)] = 0.1 * rng.standard_normal(n_z)
    return w


@pytest.mark.parametrize("case", R.THEANO_CASES, ids=lambda c: "z%d_h%d_d%d_B%d_%dx%d_flip%d" % c)
def test_theano_stack_backward_geometry(amd, case):
    """the Theano statement (tap_sign = -1: the taps look left / above, plus the border-indicator channel) at odd geometry"""
    from oracle import iaf_grad_oracle as G
    n_z, n_h, d, B, H, W, flip = case
    rng = np.random.RandomState(3300 + H + 7 * W + d)
    w = _theano_params(rng, "q", n_z, [n_h] * d)
    z, ctx = rng.standard_normal((B, n_z, H, W)), rng.standard_normal((B, n_h, H, W))
    dzn, dls = rng.standard_normal(z.shape), rng.standard_normal(z.shape)
    stack = amd.ARStack(n_z, [n_h] * d, variant="theano_flipmask" if flip else "theano")
    stack.set_training(True)
    rel = {k[2:]: dev(v) for k, v in w.items()}
    stack.prepare(rel)
    zd, cd = dev(z), dev(ctx)
    _poison_train_workspace(stack, zd)
    z_new, logsd = stack.iaf_step_train(zd, cd)
    z_ref, l_ref = stack.iaf_step(zd, cd)
    assert torch.equal(z_new, z_ref) and torch.equal(logsd, l_ref)
    dz, dctx, grads = stack.iaf_step_backward(zd, cd, z_new, logsd, dev(dzn), dev(dls), rel)
    ref, ez, el = G.theano_iaf2_nl_grads(f32(z), f32(ctx), {k: f32(v) for k, v in w.items()}, "q", n_z, [n_h] * d, f32(dzn), f32(dls),
                                         flipmask=flip)
    np.testing.assert_allclose(host(z_new), ez, atol=ATOL, rtol=0)
    _close(host(dz), ref["z"], 1e-4, "dz", ("theano", "default", "dz"))
    _close(host(dctx), ref["context"], 1e-4, "dcontext", ("theano", "default", "dcontext"))
    sizes = [n_z] + [n_h] * d
    for k in sorted(rel):
        _close(host(grads[k]), ref["q_" + k], 2e-4, k, ("theano", "default", "d" + k.split("_")[-1]))
        if k.endswith("_w"):
            out = k.startswith("out_")
            n_in = sizes[-1] if out else sizes[int(k.split("_")[0])]
            mask = np.ascontiguousarray(O.theano_ar_mask(n_in, w["q_" + k].shape[0], 3, out, flip, True))
            assert torch.count_nonzero(grads[k][torch.from_numpy(mask == 0).cuda()]).item() == 0


@pytest.mark.parametrize("case", R.POSTERIOR_CASES, ids=lambda c: "z%d_h%d_d%d_B%d_%dx%d_klmin%g" % c)
def test_posterior_block_backward_geometry(amd, case):
    """tf_train.py:56-85 with and without free bits around the stack's backward at odd geometry"""
    from oracle import iaf_grad_oracle as G
    n_z, n_h, d, B, H, W, kl_min = case
    rng = np.random.RandomState(3600 + H + 7 * W)
    params = gi.ar_multiconv2d_params(rng, n_z, [n_h] * d, [n_z, n_z])
    f = lambda c: rng.standard_normal((B, c, H, W))
    inp = dict(qm=0.1 * f(n_z), ql=0.05 * f(n_z), rm=0.1 * f(n_z), rl=0.05 * f(n_z), pm=0.1 * f(n_z), pl=0.05 * f(n_z), uc=f(n_h), dc=f(n_h),
               eps=0.05 * f(n_z))
    dz, dko = rng.standard_normal((B, n_z, H, W)), 1.0 + 0.1 * rng.standard_normal(B)
    stack = amd.ARStack(n_z, [n_h] * d)
    stack.set_training(True)
    dp = {k: dev(v) for k, v in params.items()}
    stack.prepare(dp)
    di = {k: dev(v) for k, v in inp.items()}
    _poison_train_workspace(stack, di["qm"])
    fw = stack.posterior_block_train(di["qm"], di["ql"], di["rm"], di["rl"], di["pm"], di["pl"], di["uc"], di["dc"], di["eps"], kl_min)
    bw = stack.posterior_block_backward(di["qm"], di["ql"], di["rm"], di["rl"], di["pm"], di["pl"], di["eps"], kl_min, fw["z"], dev(dz),
                                        dev(dko), dp)
    ref, z_ref, klo_ref, klc_ref = G.posterior_block_grads({k: f32(v) for k, v in inp.items()}, {k: f32(v) for k, v in params.items()},
                                                           [n_h] * d, kl_min, f32(dz), f32(dko))
    np.testing.assert_allclose(host(fw["z"]), z_ref, atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(fw["kl_obj"]), klo_ref, atol=2e-3, rtol=1e-4)
    np.testing.assert_allclose(host(fw["kl_cost"]), klc_ref, atol=2e-3, rtol=1e-4)
    for nm, keys in (("dmean", ("qm", "rm")), ("dlogsd", ("ql", "rl")), ("dpz_mean", ("pm",)), ("dpz_logsd", ("pl",)), ("dcontext", ("uc", "dc"))):
        for key in keys:
            _close(host(bw[nm]), ref[key], 2e-4, "%s vs d %s" % (nm, key), ("posterior", "default", nm))
    for k in sorted(params):
        _close(host(bw["grads"][k]), ref[k], 3e-4, k, ("posterior", "default", "d" + k.split("/")[1]))
    _masked_entries_are_zero(bw["grads"], params)


def test_deferred_weightnorm_backward_at_odd_geometry(amd):
    """the weight-norm pass of the stack left to WnBwdBatch gives exactly the gradients of the immediate call"""
    n_z, n_h, d, B, H, W = R.DEFERRED_CASE
    params, z, ctx, dzn, dls = _stack_inputs(3900, n_z, n_h, d, B, H, W)
    stack, dp, (zd, cd, z_new, logsd), dz, dctx, grads = _stack_step(amd, None, params, z, ctx, dzn, dls, n_z, n_h, d)
    batch = amd.WnBwdBatch(stacks=[stack])
    g2 = {k: torch.zeros_like(v) for k, v in dp.items()}
    _poison_train_workspace(stack, zd)
    stack.iaf_step_train(zd, cd)
    dz2, dctx2, _ = stack.iaf_step_backward(zd, cd, z_new, logsd, dev(dzn), dev(dls), dp)
    batch.run(stack_params=[dp], stack_grads=[g2])
    torch.cuda.synchronize()
    assert torch.equal(dz2, dz) and torch.equal(dctx2, dctx)
    for k in dp:
        assert torch.equal(g2[k], grads[k]), k


# ---------------------------------------------------------------- d. border property
def _padding_only_taps(H, W):
    """boolean [3, 3]: the taps (kh, kw) that see nothing but padding on an H x W image"""
    t = np.zeros((3, 3), bool)
    if H == 1:
        t[0, :] = t[2, :] = True
    if W == 1:
        t[:, 0] = t[:, 2] = True
    return t


@pytest.mark.parametrize("case", R.BORDER_CONV_CASES, ids=lambda c: "B%d_%dto%d_%dx%d" % c)
def test_conv_backward_on_images_whose_taps_see_only_padding(amd, case):
    """1 x 1, 1 x W and H x 1 images: the weight gradient of a tap that sees only padding is zero, so dV at those taps is what the weight
    norm alone couples in (compared with the reference, on those taps alone), and the data gradient of an image does not read its
    neighbours in the batch: replacing their dy leaves it unchanged bit for bit"""
    B, ci, co, H, W = case
    p, x, dy, res = _conv_inputs(case, 4500 + H + 3 * W + ci)
    want = _conv_reference(p, x, dy, True, 1.0)
    taps = _padding_only_taps(H, W)
    assert taps.any() and not taps[1, 1]
    rng = np.random.RandomState(4600)
    for prec in (("f32", "bf16x3") if ci % 32 == 0 else ("f32",)):
        got = _conv_backward(amd, case, prec, p, x, dy, res, "e")
        _close(got["dV"][taps], want["dV"][taps], 1e-4, "dV on the padding-only taps", ("border", prec, "dV"))
        _close(got["dV"], want["dV"], 1e-4, "dV", ("border", prec, "dV_all"))
        _close(got["dx"][0], want["dx"], 1e-4, "dx", ("border", prec, "dx"))
        for b in range(B):                        # new dy for every image but b
            dy2 = np.where((np.arange(B) == b).reshape(B, 1, 1, 1), dy, 3.0 * rng.standard_normal(dy.shape))
            got2 = _conv_backward(amd, case, prec, p, x, dy2, res, "e")
            assert torch.equal(got2["raw_dx"][0][b], got["raw_dx"][0][b]), "dx of image %d changed with the other images' dy" % b
            assert not torch.equal(got2["raw_dx"][0], got["raw_dx"][0])


@pytest.mark.parametrize("case", R.BORDER_STACK_CASES, ids=lambda c: "z%d_h%d_d%d_B%d_%dx%d" % c)
def test_stack_backward_on_images_whose_taps_see_only_padding(amd, case):
    """the same for the masked stack: dV on the unmasked taps that see only padding against the reference, and dz / dcontext of an image
    unchanged, bit for bit, when the other images' incoming gradients are replaced"""
    from oracle import iaf_grad_oracle as G
    n_z, n_h, d, B, H, W = case
    params, z, ctx, dzn, dls = _stack_inputs(4700 + H + 3 * W + n_h, n_z, n_h, d, B, H, W)
    ref, _, _ = G.iaf_step_grads(f32(z), f32(ctx), {k: f32(v) for k, v in params.items()}, [n_h] * d, f32(dzn), f32(dls))
    taps = _padding_only_taps(H, W)
    _, _, _, dz, dctx, grads = _stack_step(amd, None, params, z, ctx, dzn, dls, n_z, n_h, d)
    for k in sorted(params):
        if k.endswith("/V"):
            _close(host(grads[k])[taps], ref[k][taps], 2e-4, k + " on the padding-only taps", ("border", "default", "stack_dV"))
    _masked_entries_are_zero(grads, params)
    _close(host(dz), ref["z"], 1e-4, "dz", ("border", "default", "stack_dz"))
    rng = np.random.RandomState(4800)
    for b in range(B):
        keep = (np.arange(B) == b).reshape(B, 1, 1, 1)
        dzn2, dls2 = np.where(keep, dzn, 3.0 * rng.standard_normal(dzn.shape)), np.where(keep, dls, 3.0 * rng.standard_normal(dls.shape))
        _, _, _, dz2, dctx2, _ = _stack_step(amd, None, params, z, ctx, dzn2, dls2, n_z, n_h, d, check_forward=False)
        assert torch.equal(dz2[b], dz[b]) and torch.equal(dctx2[b], dctx[b]), "gradients of image %d changed with the other images'" % b
        assert not torch.equal(dz2, dz)
