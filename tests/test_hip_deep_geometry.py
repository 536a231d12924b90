"""The backward pass of the masked ResNet stack (iaf_amd.ResnetARStack.iaf_step_backward) over awkward geometry: what
tests/test_hip_backward_geometry.py is for the plain stack, step for step.

The data gradients of a resnet stack are launched on the transposed problems with the launch shape the host's model chooses from
(P, W, n_h, n_z), in two modes of the epilogue EPI_DGRAD_RES (MODE_DGRAD_RAW: the output pair read the raw stream; MODE_DGRAD_SKIP: a
conv1's gradient joins the stream's, in place) and, from 4096 pixels on, on the split products.  tests/deep_plan_reference.py restates
that plan and holds the case table RESNET_CASES; tests/test_deep_plan_reference.py proves on the CPU that the table reaches every launch
shape the model can return for these channel sets in both modes, both output forms of the SKIP mode, both kernel families, every
weight-gradient kernel class, both sides of the 4096-pixel rule, and the 1 x 1, 1 x W and H x 1 images, where every off-centre tap sees
only the border channel.  Here every gradient of every case is compared with torch-fp64 autograd of the restated step
(deep_reference.deep_step_grads) on the fp32-rounded inputs.

Metric and bounds are those of tests/test_hip_backward_geometry.py: max|got - want| / max|want| below 1e-4 for dz and dcontext, 2e-4 for
the parameter gradients; split data gradients within 2 x the exact-fp32 path's error + 1e-6 on the same inputs; a quantity whose
reference is identically zero must be exactly zero; masked entries of every _w gradient are exactly zero.
Weights: deep_plan_reference.rand_params (the _s scale at 0.2)."""
import collections

import numpy as np
import pytest
import torch

import deep_plan_reference as D
import deep_reference as DR
from oracle import iaf_oracle as O

pytestmark = pytest.mark.gpu
ATOL = 1e-4
WORST = collections.defaultdict(float)          # (precision, quantity) -> worst relative error seen


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()
    yield iaf_amd
    for key in sorted(WORST):
        print("worst rel err  resnet  %-7s %-10s %.3g" % (key + (WORST[key],)))


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


def _inputs(seed, n_z, n_h, depth, B, H, W):
    rng = np.random.RandomState(seed)
    w = D.rand_params(rng, "r", n_z, n_h, depth)
    f = lambda c: rng.standard_normal((B, c, H, W))
    return w, f(n_z), f(n_h), f(n_z), f(n_z)


def _poison_train_workspace(stack, z):
    """0xFF in every byte of the stack's training scratch (NaN as floats) before the forward: what the backward reads without the
    forward or itself having written it shows"""
    B, _, H, W = (int(v) for v in z.shape)
    ws, _ = stack._train_workspace(B, H, W, z.device)
    ws.fill_(0xFF)


def _step(amd, prec, w, z, ctx, dzn, dls, n_z, n_h, depth):
    st = amd.ResnetARStack(n_z, n_h, depth)
    if prec is not None:
        st.set_precision(prec)
    st.set_training(True)
    rel = {k[2:]: dev(v) for k, v in w.items()}
    st.prepare(rel)
    zd, cd = dev(z), dev(ctx)
    _poison_train_workspace(st, zd)
    z_new, logsd = st.iaf_step_train(zd, cd)
    z_ref, l_ref = st.iaf_step(zd, cd)          # training forward == evaluation forward, bit for bit
    assert torch.equal(z_new, z_ref) and torch.equal(logsd, l_ref)
    dz, dctx, grads = st.iaf_step_backward(zd, cd, z_new, logsd, dev(dzn), dev(dls), rel)
    torch.cuda.synchronize()
    return st, rel, (zd, cd, z_new, logsd), dz, dctx, grads


def _ar_mask(n_in, n_out, zerodiagonal):
    """the entries of a conv's w that the statement reads: the Theano mask, and on a zero-diagonal conv without the centre tap of its
    first rows (ar.py:268-276), as _live_macs_per_pixel of tests/test_hip_deep.py"""
    m = np.array(O.theano_ar_mask(n_in, n_out, 3, zerodiagonal, False, True), dtype=np.float64)
    if zerodiagonal:
        m[:(n_out // n_in if n_out >= n_in else 1), :, 1, 1] = 0.0
    return m


def _masked_entries_are_zero(grads, n_z, n_h):
    for k, g in grads.items():
        if k.endswith("_w"):
            out = k.startswith("out_")
            n_in, n_out = (n_z if k.startswith("input") else n_h), (n_z if out else n_h)
            mask = _ar_mask(n_in, n_out, out)
            assert tuple(g.shape) == mask.shape
            assert torch.count_nonzero(g[torch.from_numpy(mask == 0).cuda()]).item() == 0, k


@pytest.mark.parametrize("case", D.RESNET_CASES, ids=D.resnet_id)
def test_resnet_backward_geometry(amd, case):
    """dz, dcontext and every parameter gradient at the stack's default precision; where the plan says a data gradient runs split
    (asserted through dgrad_precision), also at "f32", and the split data gradients within 2 x the exact path's error"""
    n_z, n_h, depth, B, H, W = case
    w, z, ctx, dzn, dls = _inputs(7000 + D.RESNET_CASES.index(case), *case)
    ref, ez, es = DR.deep_step_grads(f32(z), f32(ctx), {k: f32(v) for k, v in w.items()}, "r", n_z, n_h, depth, f32(dzn), f32(dls))
    plan = D.resnet_plan(n_z, n_h, depth, B, H, W)
    split_dx = any(plan["dgrad_split"])
    errs = {}
    for prec in ((None, "f32") if split_dx else (None,)):
        name = prec or "default"
        st, rel, (zd, cd, z_new, logsd), dz, dctx, grads = _step(amd, prec, w, z, ctx, dzn, dls, n_z, n_h, depth)
        layers = range(st.depth_ar + 1)
        want_split = [s and prec is None for s in plan["dgrad_split"]]
        assert [st.dgrad_precision(l, B, H, W) == "bf16x3" for l in layers] == want_split
        if B * H * W < 4096:          # (4095 among them: the last below the rule)
            assert all(st.layer_precision(l, B, H, W) == "f32" and st.dgrad_precision(l, B, H, W) == "f32" for l in layers)
        np.testing.assert_allclose(host(z_new), ez, atol=ATOL, rtol=0)
        np.testing.assert_allclose(host(logsd), es, atol=ATOL, rtol=0)
        e = errs[name] = {"dz": _close(host(dz), ref["z"], 1e-4, "dz", (name, "dz")),
                          "dcontext": _close(host(dctx), ref["context"], 1e-4, "dcontext", (name, "dcontext"))}
        assert sorted(grads) == sorted(rel) and len(grads) == 3 * (2 * depth + 3)
        for k in sorted(rel):
            e[k] = _close(host(grads[k]), ref["r_" + k], 2e-4, k, (name, "d" + k.split("_")[-1]))
        _masked_entries_are_zero(grads, n_z, n_h)
        print("%s %-7s %s" % (D.resnet_id(case), name, "  ".join("%s %.3g" % kv for kv in sorted(e.items()))))
    if split_dx:
        for q in ("dz", "dcontext"):
            assert errs["default"][q] <= 2.0 * errs["f32"][q] + 1e-6, "%s: %.3g against exact fp32 %.3g" % (q, errs["default"][q], errs["f32"][q])


def test_resnet_deferred_weightnorm_backward_at_odd_geometry(amd):
    """the weight-norm pass of a resnet stack left to WnBwdBatch gives exactly the gradients of the immediate call"""
    n_z, n_h, depth, B, H, W = D.DEFERRED_CASE
    w, z, ctx, dzn, dls = _inputs(7900, *D.DEFERRED_CASE)
    st, rel, (zd, cd, z_new, logsd), dz, dctx, grads = _step(amd, None, w, z, ctx, dzn, dls, n_z, n_h, depth)
    ref, _, _ = DR.deep_step_grads(f32(z), f32(ctx), {k: f32(v) for k, v in w.items()}, "r", n_z, n_h, depth, f32(dzn), f32(dls))
    for k in sorted(rel):          # the direct path itself against fp64: bit-identity with it then says the same of the deferred one
        _close(host(grads[k]), ref["r_" + k], 2e-4, k)
    batch = amd.WnBwdBatch(stacks=[st])
    g2 = {k: torch.zeros_like(v) for k, v in rel.items()}
    _poison_train_workspace(st, zd)
    st.iaf_step_train(zd, cd)
    dz2, dctx2, _ = st.iaf_step_backward(zd, cd, z_new, logsd, dev(dzn), dev(dls), rel)
    batch.run(stack_params=[rel], stack_grads=[g2])
    torch.cuda.synchronize()
    assert torch.equal(dz2, dz) and torch.equal(dctx2, dctx)
    for k in rel:
        assert torch.equal(g2[k], grads[k]), k
