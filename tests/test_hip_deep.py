"""GPU tests of the masked ResNet inside the IAF step (iaf_stack_create_resnet / iaf_amd.ResnetARStack) and of the posterior
'down_iaf2_deep' of iaf_amd.CVAELayerIAF (models.py:104-108, 272-285; graphy/nodes/ar.py:428-448, 478-528): the reference's own outputs
(tests/golden/theano_cvae_layer_deep.npz), the stack against the fp64 statement on both kernel families, the backward pass against
torch-fp64 autograd of the whole layer (directly and through the deferred weight-norm batch), training forward against evaluation
forward, the inverse step, a captured down_q against the eager one, and a plain stack before and after a resnet stack ran.
References: tests/deep_reference.py.  Bounds: those of tests/test_hip_made.py."""
import functools
import os

import numpy as np
import pytest
import torch

import deep_reference as DR
import make_golden_deep as MGD
from oracle import iaf_oracle as O

pytestmark = pytest.mark.gpu

ATOL = 1e-4
CASES = sorted(MGD.CASES)


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


def _rel_params(w, pre):
    return {k[len(pre):]: dev(v) for k, v in w.items() if k.startswith(pre)}


def _pin_split(st, B, H, W):
    """a split-product launch shape on every layer that has the pack (c_in a multiple of 32): launches of fewer than 4096 pixels would
    otherwise stay on the exact-fp32 kernel (auto_shape_bf3), and the split-product form of the new epilogues would go untested.  The
    shape is the one tests/test_hip_bf3.py pins.  Returns the layers that now run the split products."""
    nt_h = [n for n in (5, 4, 2) if (st.n_h // 16) % n == 0][0]
    nt_o = [n for n in (4, 2) if (2 * st.n_z // 16) % n == 0][0]
    split = []
    for layer in range(st.depth_ar + 1):
        c_in = st.n_z if layer == 0 else st.n_h
        if c_in % 32:
            continue
        st.set_tuning_bf3(layer, nt_o if layer == st.depth_ar else nt_h, 2, 1, 4)
        split.append(layer)
    for layer in range(st.depth_ar + 1):
        assert st.layer_precision(layer, B, H, W) == ("bf16x3" if layer in split else "f32"), layer
    return split


# ---------------------------------------------------------------- 1. the reference's own outputs
@pytest.mark.parametrize("cname", CASES)
def test_deep_layer_vs_reference_golden(amd, golden_dir, cname):
    """models.cvae_layer(..., 'diag', 'down_iaf2_deep', ...) through iaf_amd.CVAELayerIAF: the plain Theano convs come from the NumPy
    statement (out of scope), the step, the KL and the free bits run on the GPU"""
    B, n_h, n_z, depth, H, W, kl_min = MGD.CASES[cname]
    g = np.load(os.path.join(golden_dir, MGD.FIXTURE))
    c = MGD.fixture_case(g, cname)
    w32 = {k: f32(v) for k, v in c["w"].items()}
    cw = lambda nm: (w32["1" + nm + "_w"], w32["1" + nm + "_b"], w32["1" + nm + "_s"])
    up_conv1 = O.theano_conv2d(_elu(f32(c["up_input"])), *cw("_up_conv1_1"))
    down_conv1 = O.theano_conv2d(_elu(f32(c["down_input"])), *cw("_down_conv1"))
    assert down_conv1.shape[1] == 2 * n_h + 4 * n_z
    layer = amd.CVAELayerIAF("1", n_h, n_z, depth, posterior="down_iaf2_deep", kl_min=kl_min)
    assert isinstance(layer.stack, amd.ResnetARStack) and layer.stack.depth == depth and layer.stack2 is None
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
    hp = layer.down_p(dev(down_conv1), dev(c["eps_p"]))
    p_out = f32(c["down_input"]) + 0.1 * O.theano_conv2d(_elu(host(hp)), *cw("_down_conv2_1"))
    np.testing.assert_allclose(p_out, g[cname + "/down_p_out"], atol=ATOL, rtol=0)


# ---------------------------------------------------------------- 2. the stack against fp64, both kernel families
# B, n_h, n_z, depth, H, W: the four fixture geometries, the BASELINE width (ten co tiles), 16-pixel rows with more than one block, and
# one launch above the 4096 pixels from which the split products are chosen without a pinned shape
STACK_SHAPES = [MGD.CASES[c][:6] for c in CASES] + [(2, 160, 32, 2, 8, 8), (5, 64, 32, 1, 16, 16), (17, 64, 32, 1, 16, 16)]
MUST_SPLIT = [(2, 160, 32, 2, 8, 8), (5, 64, 32, 1, 16, 16)]
_sid = lambda s: "B%d_h%d_z%d_d%d_%dx%d" % s


@functools.lru_cache(maxsize=None)
def _stack_case(shape):
    B, n_h, n_z, depth, H, W = shape
    rng = np.random.RandomState(700 + 3 * n_h + 5 * depth + H + B)
    w = DR.rand_params(rng, "r", n_z, n_h, depth)
    z, ctx = rng.standard_normal((B, n_z, H, W)), rng.standard_normal((B, n_h, H, W))
    w32 = {k: f32(v) for k, v in w.items()}
    m, s = DR.resnet(f32(z), f32(ctx), w32, "r", n_z, n_h, depth)
    return w, z, ctx, m, s


def _live_macs_per_pixel(n_in, n_out, zerodiagonal):
    """live multiply-adds per pixel of one masked 3x3 conv, counted from the Theano mask itself (the border channel is no MAC of the GEMM)"""
    m = np.array(O.theano_ar_mask(n_in, n_out, 3, zerodiagonal, False, True), dtype=np.float64)
    if zerodiagonal:
        m[:(n_out // n_in if n_out >= n_in else 1), :, 1, 1] = 0.0                  # ar.py:268-276
    return int((m[:, :n_in] != 0).sum())


@pytest.mark.parametrize("prec", ["f32", "split"])
@pytest.mark.parametrize("shape", STACK_SHAPES, ids=_sid)
def test_resnet_stack_vs_fp64(amd, shape, prec):
    """iaf_ar_multiconv2d_forward (raw m, s) and iaf_step_forward of a resnet stack against the fp64 statement, 1e-4 absolute, on the
    exact-fp32 family (IAF_PRECISION_F32) and, under the default precision, on the split products ("split").  The default precision
    chooses the split products by itself from 4096 pixels on (B = 17 at 16x16 here, asserted); below, a launch shape is PINNED so that
    the n_h = 160 and the 16x16 case run them as well (the engine's own choice there is the fp32 kernel)."""
    B, n_h, n_z, depth, H, W = shape
    w, z, ctx, em, es = _stack_case(shape)
    st = amd.ResnetARStack(n_z, n_h, depth)
    assert st.depth_ar == 2 * depth + 1 and st.step_is_fused(B, H, W) == 0 and not st.step_exchanges(B, H, W) and not st.step_pairs(B, H, W)
    if prec == "f32":
        st.set_precision("f32")
    st.prepare(_rel_params(w, "r_"))
    layers = list(range(st.depth_ar + 1))
    if prec == "f32":
        assert all(st.layer_precision(l, B, H, W) == "f32" for l in layers)
    elif B * H * W >= 4096:
        assert all(st.layer_precision(l, B, H, W) == "bf16x3" for l in layers), [st.layer_precision(l, B, H, W) for l in layers]
    else:
        split = _pin_split(st, B, H, W)
        if shape in MUST_SPLIT:
            assert split == layers          # the input conv and a conv2 (EPI_RES), a conv1, the output pair: all on the split products
    m_raw, s_raw = st.ar_multiconv2d(dev(z), dev(ctx))
    print("%s %s: max |raw - fp64| = %.3g (max |ref| %.3g)" % (_sid(shape), prec, max(np.abs(host(m_raw) - em).max(), np.abs(host(s_raw) - es).max()),
                                                                  max(np.abs(em).max(), np.abs(es).max())))
    np.testing.assert_allclose(host(m_raw), em, atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(s_raw), es, atol=ATOL, rtol=0)
    z_new, logsd = st.iaf_step(dev(z), dev(ctx))
    np.testing.assert_allclose(host(z_new), (f32(z) - 0.1 * em) / np.exp(0.1 * es), atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(logsd), 0.1 * es, atol=ATOL, rtol=0)
    # live work: every layer against a count from the mask itself, and the step against their sum
    P = B * H * W
    want = [_live_macs_per_pixel(n_z, n_h, False)] + [_live_macs_per_pixel(n_h, n_h, False)] * (2 * depth) + [2 * _live_macs_per_pixel(n_h, n_z, True)]
    for l in layers:
        assert st.layer_work(l, B, H, W)["live_flops"] == 2.0 * want[l] * P, l
    assert st.step_work(B, H, W)["live_flops"] == 2.0 * sum(want) * P
    # bytes of the residual-stream layers: input, raw stream out, context or skip in, elu(stream) out unless the block is the last
    wl = lambda l: st.layer_work(l, B, H, W)["bytes"]
    assert wl(2) - wl(1) == 4.0 * P * n_h * ((2 if depth == 1 else 3) - 1)


def test_resnet_stack_refuses_what_the_header_says(amd):
    """on an UNPREPARED stack: the kind is tested before anything else, so the answer is UnsupportedError, not 'not prepared'"""
    st = amd.ResnetARStack(32, 32, 1)
    U = amd._capi.UnsupportedError
    z, c = torch.zeros(1, 32, 2, 2, device="cuda"), torch.zeros(1, 32, 2, 2, device="cuda")
    for call in (lambda: st.set_fuse_step(0), lambda: st.set_fuse_first(0), lambda: st.set_halo_exchange(False),
                 lambda: st.set_packs(f32=False), lambda: st.set_precision("f16x2"), lambda: st.autotune(z, c),
                 lambda: st.time_layer(0, z, c), lambda: st.posterior_block(z, z, z, z, z, z, c, c, z, 0.0)):
        with pytest.raises(U):
            call()
    st.set_precision("bf16x3")
    st.set_precision("f32")


def test_layers_resnet_callable_prep_batch_and_queued_inverse(amd):
    """the mirror of N.ar.resnet, iaf_prep_batch_* and iaf_step_inverse_device on a resnet stack: each gives what the direct calls give"""
    shape = MGD.CASES["deep_d2"][:6]
    B, n_h, n_z, depth, H, W = shape
    w, z, ctx, em, es = _stack_case(shape)
    wd = {k: dev(v) for k, v in w.items()}
    net = amd.resnet("r", depth, n_z, n_h, [n_z, n_z], w=wd)
    m_raw, s_raw = net(dev(z), dev(ctx), wd)
    np.testing.assert_allclose(host(m_raw), em, atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(s_raw), es, atol=ATOL, rtol=0)
    with pytest.raises(amd.UnsupportedError, match="h_context"):
        net(dev(z), None, wd)
    a, b = amd.ResnetARStack(n_z, n_h, depth), amd.ARStack(n_z, [n_h], variant="theano")
    rel_b = {k[2:].replace("input", "0"): v for k, v in wd.items() if k.startswith("r_input") or k.startswith("r_out_")}
    amd.PrepBatch([a, b]).run([_rel_params(w, "r_"), rel_b])
    m2, s2 = a.ar_multiconv2d(dev(z), dev(ctx))
    assert torch.equal(m2, m_raw) and torch.equal(s2, s_raw)          # the batch wrote what iaf_stack_prepare writes
    z_new, logsd = a.iaf_step(dev(z), dev(ctx))
    stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    z0, _ = a.iaf_step_inverse_queued(z_new, dev(ctx), max_sweeps=64, tol=1e-6, check_every=2, stats=stats)
    sweeps = int(stats.cpu().numpy()[0])
    assert 0 < sweeps <= 64
    np.testing.assert_allclose(host(z0), f32(z), atol=ATOL, rtol=0)


# ---------------------------------------------------------------- 3. backward against fp64 autograd of the whole layer
def _layer_inputs(cname, golden_dir):
    """the fixture case between its plain convs: weights of the network, both conv outputs, the noise"""
    B, n_h, n_z, depth, H, W, _ = MGD.CASES[cname]
    g = np.load(os.path.join(golden_dir, MGD.FIXTURE))
    c = MGD.fixture_case(g, cname)
    w32 = {k: f32(v) for k, v in c["w"].items()}
    cw = lambda nm: (w32["1" + nm + "_w"], w32["1" + nm + "_b"], w32["1" + nm + "_s"])
    h_up = O.theano_conv2d(_elu(f32(c["up_input"])), *cw("_up_conv1_1"))
    h_dn = O.theano_conv2d(_elu(f32(c["down_input"])), *cw("_down_conv1"))
    w = {k: v for k, v in c["w"].items() if k.startswith("1_deepiaf_")}
    return w, h_up, h_dn, c["eps_down"]


_BWD_REF = {}


def _backward_reference(cname, kl_min, with_up, golden_dir):
    key = (cname, kl_min, with_up)
    if key not in _BWD_REF:
        B, n_h, n_z, depth, H, W, _ = MGD.CASES[cname]
        w, h_up, h_dn, eps = _layer_inputs(cname, golden_dir)
        rng = np.random.RandomState(900 + H + int(8 * kl_min))
        d_up, d_h = rng.standard_normal((B, n_h, H, W)), rng.standard_normal((B, n_h + n_z, H, W))
        d_obj = np.asarray(0.7) if kl_min > 0 else rng.standard_normal(B)
        ref, fw = DR.deep_iaf_grads(f32(h_up), f32(h_dn), f32(eps), {k: f32(v) for k, v in w.items()}, "1", n_h, n_z, depth, kl_min,
                                    f32(d_up) if with_up else None, f32(d_h), f32(d_obj))
        _BWD_REF[key] = (w, h_up, h_dn, eps, d_up, d_h, d_obj, ref, fw)
    return _BWD_REF[key]


def _run_backward(amd, cname, kl_min, with_up, case, deferred=False):
    B, n_h, n_z, depth, H, W, _ = MGD.CASES[cname]
    w, h_up, h_dn, eps, d_up, d_h, d_obj, ref, fw = case
    layer = amd.CVAELayerIAF("1", n_h, n_z, depth, posterior="down_iaf2_deep", kl_min=kl_min)
    layer.set_training(True)
    wd = {k: dev(v) for k, v in w.items()}
    layer.load(wd)
    batch = None
    if deferred:
        batch = amd.WnBwdBatch(stacks=[layer.stack])      # (sets iaf_stack_set_defer_weightnorm on the stack)
    up_out = layer.up(dev(h_up))
    dq = layer.down_q(dev(h_dn), eps=dev(eps))
    bw = layer.backward(dev(d_h), d_obj=(0.7 if kl_min > 0 else dev(d_obj)), d_up=dev(d_up) if with_up else None)
    if deferred:
        pre = "1_deepiaf_"
        batch.run(stack_params=[layer._rel], stack_grads=[{k[len(pre):]: v for k, v in bw["grads"].items()}])
    return up_out, dq, bw


@pytest.mark.parametrize("with_up", [True, False], ids=["d_up", "d_up_none"])
@pytest.mark.parametrize("kl_min", [0.0, 0.25])
@pytest.mark.parametrize("cname", CASES)
def test_deep_layer_backward_vs_autograd(amd, golden_dir, cname, kl_min, with_up):
    """gradients of both conv outputs (reference channel order; d context rides in both) and of every w / s / b of the network against
    torch-fp64 autograd of the restated forward: 1e-4 of the reference's largest entry"""
    B, n_h, n_z, depth, H, W, _ = MGD.CASES[cname]
    case = _backward_reference(cname, kl_min, with_up, golden_dir)
    w, ref, fw = case[0], case[7], case[8]
    up_out, dq, bw = _run_backward(amd, cname, kl_min, with_up, case)
    np.testing.assert_allclose(host(up_out), fw["up_out"], atol=0, rtol=0)
    np.testing.assert_allclose(host(dq["h"]), fw["h"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(dq["kl"]), fw["kl"], atol=ATOL, rtol=1e-5)
    np.testing.assert_allclose(host(dq["obj_kl"]), fw["obj_kl"], atol=2e-3, rtol=1e-4)
    assert tuple(bw["d_up_conv1"].shape) == (B, 2 * n_h + 2 * n_z, H, W) and tuple(bw["d_down_conv1"].shape) == (B, 2 * n_h + 4 * n_z, H, W)
    if not with_up:
        assert not bw["d_up_conv1"][:, :n_h].any()
    _rel_close(host(bw["d_up_conv1"]), ref["h_up"], 1e-4, "d_up_conv1")
    _rel_close(host(bw["d_down_conv1"]), ref["h_dn"], 1e-4, "d_down_conv1")
    _rel_close(host(bw["d_up_conv1"][:, n_h + 2 * n_z:]), ref["h_up"][:, n_h + 2 * n_z:], 1e-4, "d context")
    assert set(bw["grads"]) == set(w) and len(w) == 3 * (2 * depth + 3)
    for k in sorted(w):
        _rel_close(host(bw["grads"][k]), ref["w"][k], 1e-4, k)


@pytest.mark.parametrize("free_bits,with_up", [(False, False), (True, True)], ids=["dko_d_up_none", "free_bits_d_up"])
def test_deep_layer_backward_on_the_split_products_vs_autograd(amd, free_bits, with_up):
    """B = 17, n_h = 64, n_z = 32, depth 2 at 16x16: 4352 pixels, from which the engine runs the training forward AND every data gradient
    on the split products (asserted through iaf_stack_get_precision / iaf_stack_get_dgrad_precision) -- the bf16x3 form of EPI_RES and
    of EPI_DGRAD_RES in both modes (block 1 ends the stream, block 0 continues it and writes d context), the in-place update of the
    stream's gradient and the 0.1 d h beside it.  Every gradient against torch-fp64 autograd of the whole layer: 1e-4 of the
    reference's largest entry, the bound of the small cases.  With free bits, kl_min lies in the widest gap between the per-channel KLs
    of the case's middle half, so that both sides of the max() carry channels and none sits at its kink."""
    B, n_h, n_z, depth, H, W = 17, 64, 32, 2, 16, 16
    rng = np.random.RandomState(1000 + int(free_bits))
    w = DR.rand_params(rng, "1_deepiaf", n_z, n_h, depth)
    h_up, h_dn = 0.3 * rng.standard_normal((B, 2 * n_h + 2 * n_z, H, W)), 0.3 * rng.standard_normal((B, 2 * n_h + 4 * n_z, H, W))
    for t, at in ((h_up, n_h + n_z), (h_dn, n_h + n_z), (h_dn, n_h + 3 * n_z)):          # the three logsd groups
        t[:, at:at + n_z] *= 0.25
    eps = rng.standard_normal((B, n_z, H, W))
    kl_min = 0.0
    if free_bits:
        per_c = np.sort(DR.deep_iaf(f32(h_up), f32(h_dn), f32(eps), {k: f32(v) for k, v in w.items()}, "1", n_h, n_z, depth)["kl"]
                        .sum(axis=(2, 3)).mean(axis=0))[n_z // 4:3 * n_z // 4]
        i = int(np.argmax(np.diff(per_c)))
        kl_min = float(0.5 * (per_c[i] + per_c[i + 1]))
        assert per_c[i + 1] - per_c[i] > 1e-2, per_c
    d_up, d_h = rng.standard_normal((B, n_h, H, W)), rng.standard_normal((B, n_h + n_z, H, W))
    d_obj = np.asarray(0.7) if kl_min > 0 else rng.standard_normal(B)
    ref, fw = DR.deep_iaf_grads(f32(h_up), f32(h_dn), f32(eps), {k: f32(v) for k, v in w.items()}, "1", n_h, n_z, depth, kl_min,
                                f32(d_up) if with_up else None, f32(d_h), f32(d_obj))
    assert np.abs(fw["kl"]).max() < 100.0
    layer = amd.CVAELayerIAF("1", n_h, n_z, depth, posterior="down_iaf2_deep", kl_min=kl_min)
    layer.set_training(True)
    layer.load({k: dev(v) for k, v in w.items()})
    st = layer.stack
    for l in range(st.depth_ar + 1):
        assert st.layer_precision(l, B, H, W) == "bf16x3" and st.dgrad_precision(l, B, H, W) == "bf16x3", l
    layer.up(dev(h_up))
    dq = layer.down_q(dev(h_dn), eps=dev(eps))
    bw = layer.backward(dev(d_h), d_obj=(0.7 if kl_min > 0 else dev(d_obj)), d_up=dev(d_up) if with_up else None)
    np.testing.assert_allclose(host(dq["h"]), fw["h"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(dq["kl"]), fw["kl"], atol=ATOL, rtol=1e-5)
    _rel_close(host(bw["d_up_conv1"]), ref["h_up"], 1e-4, "d_up_conv1")
    _rel_close(host(bw["d_down_conv1"]), ref["h_dn"], 1e-4, "d_down_conv1")
    _rel_close(host(bw["d_up_conv1"][:, n_h + 2 * n_z:]), ref["h_up"][:, n_h + 2 * n_z:], 1e-4, "d context")
    assert set(bw["grads"]) == set(w)
    for k in sorted(w):
        _rel_close(host(bw["grads"][k]), ref["w"][k], 1e-4, k)


@pytest.mark.parametrize("cname", ["deep_d2", "deep_nz16"])
def test_deferred_weightnorm_batch_equals_the_direct_path(amd, golden_dir, cname):
    """iaf_stack_set_defer_weightnorm + iaf_wn_bwd_batch_run on a resnet stack: every dV / dg / db bit for bit what the direct path writes"""
    kl_min = MGD.CASES[cname][6]
    case = _backward_reference(cname, kl_min, True, golden_dir)
    _, _, direct = _run_backward(amd, cname, kl_min, True, case)
    _, _, later = _run_backward(amd, cname, kl_min, True, case, deferred=True)
    assert set(direct["grads"]) == set(later["grads"]) == set(case[0])
    for k in sorted(direct["grads"]):
        assert torch.equal(direct["grads"][k], later["grads"][k]), k
    assert torch.equal(direct["d_up_conv1"], later["d_up_conv1"]) and torch.equal(direct["d_down_conv1"], later["d_down_conv1"])


# ---------------------------------------------------------------- 4. training forward equals evaluation forward
@pytest.mark.parametrize("cname", ["deep_d2", "deep_d4"])
def test_deep_training_forward_equals_evaluation_forward(amd, golden_dir, cname):
    B, n_h, n_z, depth, H, W, _ = MGD.CASES[cname]
    w, h_up, h_dn, eps = _layer_inputs(cname, golden_dir)
    wd = {k: dev(v) for k, v in w.items()}
    outs = []
    for training in (False, True):
        layer = amd.CVAELayerIAF("1", n_h, n_z, depth, posterior="down_iaf2_deep", kl_min=0.25)
        layer.set_training(training)
        layer.load(wd)
        assert torch.equal(layer.up(dev(h_up)), dev(h_up)[:, :n_h])
        outs.append(layer.down_q(dev(h_dn), eps=dev(eps)))
    ev, tr = outs
    assert set(tr) == set(ev) == {"h", "z", "kl", "kl_sum", "obj_kl"}
    for k in ("h", "z", "kl"):
        np.testing.assert_allclose(host(tr[k]), host(ev[k]), atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(tr["kl_sum"]), host(ev["kl_sum"]), atol=2e-3, rtol=1e-4)
    np.testing.assert_allclose(host(tr["obj_kl"]), host(ev["obj_kl"]), atol=2e-3, rtol=1e-4)
    assert tr["obj_kl"].dim() == 0


# ---------------------------------------------------------------- 5. the inverse step
def test_inverse_round_trip_at_deep_d2(amd):
    shape = MGD.CASES["deep_d2"][:6]
    B, n_h, n_z, depth, H, W = shape
    w, z, ctx, _, _ = _stack_case(shape)
    st = amd.ResnetARStack(n_z, n_h, depth)
    st.prepare(_rel_params(w, "r_"))
    z_new, logsd = st.iaf_step(dev(z), dev(ctx))
    z0, logsd0, sweeps, res = st.iaf_step_inverse(z_new, dev(ctx), max_sweeps=200, tol=1e-6, check_every=2)
    print("inverse at deep_d2's geometry: %d sweeps, residual %.3g, max |z0 - z| %.3g" % (sweeps, res, np.abs(host(z0) - f32(z)).max()))
    assert 0 < sweeps < 200 and res <= 1e-6
    np.testing.assert_allclose(host(z0), f32(z), atol=ATOL, rtol=0)
    np.testing.assert_allclose(host(logsd0), host(logsd), atol=ATOL, rtol=0)


def test_inverse_is_exact_after_one_sweep_per_position(amd):
    """2x2, n_z = 16: H W n_z sweeps with tol 0 (no early out) against the fp64 ancestral solution"""
    B, n_h, n_z, depth, H, W = 2, 16, 16, 2, 2, 2
    rng = np.random.RandomState(61)
    w = DR.rand_params(rng, "r", n_z, n_h, depth)
    z_new, ctx = rng.standard_normal((B, n_z, H, W)), rng.standard_normal((B, n_h, H, W))
    ref = DR.inverse_exact(f32(z_new), f32(ctx), {k: f32(v) for k, v in w.items()}, "r", n_z, n_h, depth)
    st = amd.ResnetARStack(n_z, n_h, depth)
    st.prepare(_rel_params(w, "r_"))
    z0, _, sweeps, _ = st.iaf_step_inverse(dev(z_new), dev(ctx), max_sweeps=H * W * n_z, tol=0.0)
    assert sweeps == H * W * n_z
    np.testing.assert_allclose(host(z0), ref, atol=ATOL, rtol=0)
    assert np.abs(ref - f32(z_new)).max() > 1e-2


# ---------------------------------------------------------------- 6. capture
def test_deep_down_q_captured_in_a_graph_equals_eager(amd, golden_dir):
    """down_q launches on the current stream only: captured after a warm-up on the capturing stream and replayed twice with new noise in
    the captured buffer, it gives what the eager call gives, bit for bit"""
    cname = "deep_d2"
    B, n_h, n_z, depth, H, W, kl_min = MGD.CASES[cname]
    w, h_up, h_dn, eps = _layer_inputs(cname, golden_dir)
    rng = np.random.RandomState(71)
    layer = amd.CVAELayerIAF("1", n_h, n_z, depth, posterior="down_iaf2_deep", kl_min=kl_min)
    layer.load({k: dev(v) for k, v in w.items()})
    t_up, t_dn, eps_buf = dev(h_up), dev(h_dn), dev(eps)
    keys = ("h", "z", "kl", "kl_sum", "obj_kl")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = []
    with torch.cuda.stream(s):
        layer.up(t_up)
        layer.down_q(t_dn, eps=eps_buf)                             # warm-up: workspaces and the zeros exist before the capture
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


# ---------------------------------------------------------------- 7. the plain stacks are what they were
def test_plain_layer_is_bit_identical_before_and_after_a_resnet_stack_ran(amd):
    """one 'down_iaf2_nl' layer at deep_d2's geometry: the same bits whether or not a resnet stack was created and run before it"""
    import made_reference as MR
    B, n_h, n_z, depth, H, W = MGD.CASES["deep_d2"][:6]
    rng = np.random.RandomState(81)
    w = {k: v for k, v in MR.rand_params(rng, "1", n_z, [n_h] * 2, "down_iaf2_nl").items() if "_posterior_conv1_" in k}
    h_up, h_dn = 0.5 * rng.standard_normal((B, 2 * n_h + 2 * n_z, H, W)), 0.5 * rng.standard_normal((B, 2 * n_h + 4 * n_z, H, W))
    eps = rng.standard_normal((B, n_z, H, W))

    def plain():
        layer = amd.CVAELayerIAF("1", n_h, n_z, 2, posterior="down_iaf2_nl", kl_min=0.25)
        layer.load({k: dev(v) for k, v in w.items()})
        layer.up(dev(h_up))
        d = layer.down_q(dev(h_dn), eps=dev(eps))
        return {k: d[k].clone() for k in ("h", "z", "kl", "kl_sum", "obj_kl")}

    before = plain()
    shape = MGD.CASES["deep_d2"][:6]
    wr, z, ctx, _, _ = _stack_case(shape)
    st = amd.ResnetARStack(n_z, n_h, depth)
    st.prepare(_rel_params(wr, "r_"))
    st.iaf_step(dev(z), dev(ctx))
    torch.cuda.synchronize()
    after = plain()
    for k in before:
        assert torch.equal(before[k], after[k]), k
