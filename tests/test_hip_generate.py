"""GPU tests of image generation from the prior: CVAE1.generate -- the reference's m_trunc[0] of CVAE1(hps, "sample") with no image fed
(tf_train.py:300, 358-362: only the top-down pass runs) -- and the layers under it: IAFLayer.generate_down and down_conv1 in prior form
(WNConv2d.prior_sample, iaf_conv3x3_forward_prior_sample: only the pz_mean / pz_logsd / h_det tiles, the prior sample drawn in the epilogue).
Against the reference's own sample-mode output (tests/golden/cvae1_forward.npz), the CPU oracle, and the full-forward path on the GPU."""
import os
import warnings

import numpy as np
import pytest
import torch

import golden_inputs as gi
from oracle import iaf_oracle as O

pytestmark = pytest.mark.gpu


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


def build_model(amd, c, mode=None):
    m = amd.CVAE1(z_size=c["z_size"], h_size=c["h_size"], kl_min=c["kl_min"], depth=c["depth"], num_blocks=c["num_blocks"], k=c["k"],
                  image_size=c["image_size"], mode=mode or c["mode"])
    m.load({k: dev(v) for k, v in c["params"].items()})
    return m


def prior_noise(c, B, seed):
    rng = np.random.RandomState(seed)
    out = []
    for i in reversed(range(c["depth"])):
        Sl = c["image_size"] // 2 ** (i + 1)
        out += [rng.standard_normal((B, c["z_size"], Sl, Sl)) for _ in range(c["num_blocks"])]
    return out


def oracle_sample(c, eps_prior):
    """O.cvae1_forward in mode "sample" (its output does not depend on x): the posterior slots of the noise list are never read"""
    B = eps_prior[0].shape[0]
    noise = []
    for e in eps_prior:
        noise += [f32(e), np.zeros_like(e)]
    x = np.zeros((B, 3, c["image_size"], c["image_size"]), np.uint8)
    p32 = {k: f32(v) for k, v in c["params"].items()}
    x_out, _, _ = O.cvae1_forward(x, p32, c["z_size"], c["h_size"], c["depth"], c["num_blocks"], c["kl_min"], 1, noise, mode="sample")
    return x_out


# -- 1. the reference's own output -------------------------------------------------------------------------------------------------
def test_generate_matches_reference_sample_golden(amd, golden_dir):
    g = np.load(os.path.join(golden_dir, "cvae1_forward.npz"))
    c = gi.model_case_inputs("model_sample")
    model = build_model(amd, c)
    x_out = model.generate([dev(e) for e in c["noise"][0::2]])
    assert tuple(x_out.shape) == (c["B"], 3, c["image_size"], c["image_size"])
    np.testing.assert_allclose(host(x_out), g["model_sample/x_out"], rtol=0, atol=2e-4)


# -- 2. the oracle: the generic fallback (z 4 / h 8) and the BASELINE geometry -----------------------------------------------------------
@pytest.mark.parametrize("name", ["model_tiny", "model_cfg"])
def test_generate_matches_oracle_sample_mode(amd, name):
    c = gi.model_case_inputs(name)
    model = build_model(amd, c, mode="train")              # (the mode the model was built with does not matter: the variables are the same)
    eps = prior_noise(c, 2, 5)
    x_out = model.generate([dev(e) for e in eps])
    np.testing.assert_allclose(host(x_out), oracle_sample(c, eps), rtol=0, atol=2e-4)


# -- 3. the current path, at sizes that select each pack kind --------------------------------------------------------------------------
@pytest.mark.parametrize("B", [7, 32], ids=["B7_bf16x3", "B32_f16x2"])
def test_generate_matches_forward_sample_mode(amd, B):
    c = gi.model_case_inputs("model_cfg")                  # z 32, h 160, 32x32 images: latent levels 16x16 and 8x8
    model = build_model(amd, c, mode="sample")
    dc1 = model.layers[0][1].down_conv1                    # a 16x16 layer
    assert dc1.runs_f16x2(B, 16, 16) == (B == 32)          # 1792 pixels: below the fp16-plane size rule; 8192: two fp16 planes
    eps = [dev(e) for e in prior_noise(c, B, 11)]
    noise = []
    for e in eps:
        noise += [e, torch.zeros_like(e)]
    x = torch.zeros((B, 3, 32, 32), dtype=torch.uint8, device="cuda")
    want, _, _ = model.forward(x, noise)
    got = model.generate(eps)
    np.testing.assert_allclose(host(got), host(want), rtol=0, atol=2e-5)


# -- 4. the kernel: down_conv1 in prior form -----------------------------------------------------------------------------------------
KERNEL_CASES = [(16, 32, 1, 5, 7, True), (16, 32, 3, 16, 16, False), (32, 160, 1, 5, 7, False), (32, 160, 3, 8, 8, True),
                (32, 160, 3, 16, 16, True), (32, 160, 32, 8, 8, True), (32, 160, 32, 16, 16, False), (32, 160, 32, 16, 16, True)]


@pytest.mark.parametrize("zs,hs,B,H,W,elu", KERNEL_CASES)
def test_prior_sample_kernel_vs_oracle_and_unfused_path(amd, zs, hs, B, H, W, elu):
    rng = np.random.RandomState(zs + hs + B + H * W)
    p = gi.conv_params(rng, hs, 4 * zs + 2 * hs)
    x = rng.standard_normal((B, hs, H, W))
    eps = rng.standard_normal((B, zs, H, W))
    conv = amd.WNConv2d(hs, 4 * zs + 2 * hs)
    conv.prepare(dev(p["V"]), dev(p["g"]), dev(p["b"]))
    xd, ed = dev(x), dev(eps)
    z, h_det = conv.prior_sample(xd, ed, zs, elu_input=elu)
    # oracle: conv2d + split + gaussian_diag_sample (tf_train.py:52-54, 56, 60-61)
    xin = O.elu(f32(x)) if elu else f32(x)
    y = O.conv2d(xin, f32(p["V"]), f32(p["g"]), f32(p["b"]))
    pm, pl, _, _, _, hd = O.split_channels(y, [zs] * 4 + [hs] * 2)
    ez = O.gaussian_diag_sample(pm, 2 * pl, f32(eps))
    np.testing.assert_allclose(host(z), ez, rtol=4e-6, atol=2e-4)      # (exp(pz_logsd) carries the conv's relative error into large z)
    np.testing.assert_allclose(host(h_det), hd, rtol=0, atol=1e-4)
    # the unfused path on the GPU: the full conv, then the sample in a launch of its own
    pzm, pzl, _, _, _, hd2 = conv(xd, elu_input=elu, split=[zs] * 4 + [hs] * 2)
    z2 = amd.iaf_layer.gaussian_sample(pzm, pzl, ed)
    # (fp32 round-off: the same arithmetic at the fp16-plane sizes, bf16x3 against the fp32 kernel below them)
    tol = 1e-5 * max(1.0, float(np.abs(host(z2)).max()))
    np.testing.assert_allclose(host(z), host(z2), rtol=0, atol=tol)
    np.testing.assert_allclose(host(h_det), host(hd2), rtol=0, atol=1e-5)


def test_prior_sample_argument_errors(amd):
    lib, P = amd._capi.lib(), amd.layers._ptr
    conv = amd.WNConv2d(32, 4 * 16 + 2 * 32)
    x = torch.zeros((1, 32, 4, 4), device="cuda")
    e = torch.zeros((1, 16, 4, 4), device="cuda")
    h = torch.zeros((1, 32, 4, 4), device="cuda")
    st = amd.layers._stream()
    # argument errors come before the prepare check and before any device work
    assert lib.iaf_conv3x3_forward_prior_sample(conv._h, P(x), 1, 16, 16, P(e), P(e), P(h), 1, 4, 4, st) == amd._capi.IAF_ERR_SHAPE
    assert lib.iaf_conv3x3_forward_prior_sample(conv._h, P(x), 1, 16, 32, P(e), P(e), P(h), 0, 4, 4, st) == amd._capi.IAF_ERR_SHAPE
    assert lib.iaf_conv3x3_forward_prior_sample(conv._h, P(x), 1, 16, 32, None, P(e), P(h), 1, 4, 4, st) == amd._capi.IAF_ERR_NULL
    assert lib.iaf_conv3x3_forward_prior_sample(conv._h, P(x), 1, 16, 32, P(e), P(e), P(h), 1, 4, 4, st) == amd._capi.IAF_ERR_NOT_PREPARED
    masked = amd.WNConv2d(32, 128, ar_mask=False)
    assert lib.iaf_conv3x3_forward_prior_sample(masked._h, P(x), 1, 16, 32, P(e), P(e), P(h), 1, 4, 4, st) == amd._capi.IAF_ERR_UNSUPPORTED
    tiny = amd.WNConv2d(8, 4 * 4 + 2 * 8)                  # generic channel counts: no fused form
    assert lib.iaf_conv3x3_forward_prior_sample(tiny._h, P(x), 1, 4, 8, P(e), P(e), P(h), 1, 4, 4, st) == amd._capi.IAF_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        conv.prior_sample(x, torch.zeros((1, 16, 4, 5), device="cuda"), 16)


# -- 5. the layer: generate_down on a freshly loaded layer (no up pass) ---------------------------------------------------------------
@pytest.mark.parametrize("ds", [False, True], ids=["plain", "downsample"])
def test_generate_down_matches_oracle_layer(amd, ds):
    zs, hs, B, H = 32, 160, 3, 8
    rng = np.random.RandomState(31 + ds)
    p = {}
    for nm, (ci, co) in (("up_conv1", (hs, 2 * zs + 2 * hs)), ("up_conv3", (hs, hs)), ("down_conv1", (hs, 4 * zs + 2 * hs))):
        for k, v in gi.conv_params(rng, ci, co).items():
            p[nm + "/" + k] = v
    for k, v in gi.ar_multiconv2d_params(rng, zs, [hs, hs], [zs, zs]).items():
        p["ar_multiconv2d/" + k] = v
    last = gi.deconv_params(rng, hs + zs, hs) if ds else gi.conv_params(rng, hs + zs, hs)
    for k, v in last.items():
        p[("down_deconv2/" if ds else "down_conv2/") + k] = v
    layer = amd.IAFLayer(zs, hs, depth_ar=2, kl_min=0.25, downsample=ds, mode="sample")
    layer.load({k: dev(v) for k, v in p.items()})
    inp = rng.standard_normal((B, hs, H, H))
    eps = rng.standard_normal((B, zs, H, H))
    out = layer.generate_down(dev(inp), dev(eps))
    assert layer.posterior.qz_mean is None                 # the up-pass state was neither needed nor touched
    p32 = {k: f32(v) for k, v in p.items()}
    want, _, _, _ = O.iaf_layer_down(f32(inp), p32, None, None, None, None, zs, hs, 0.25, mode="sample", downsample=ds,
                                     eps_prior=f32(eps))
    assert tuple(out.shape) == want.shape
    np.testing.assert_allclose(host(out), want, rtol=0, atol=2e-4)


# -- 6. fallbacks and protocols ------------------------------------------------------------------------------------------------------
def test_generate_with_down_conv1_pinned_to_fp32(amd, golden_dir):
    c = gi.model_case_inputs("model_sample")
    model = build_model(amd, c)
    for level in model.layers:
        for layer in level:
            layer.down_conv1.set_precision("f32")
    model.load({k: dev(v) for k, v in c["params"].items()})
    lay = model.layers[0][0]
    B = c["B"]
    rc, _, _ = lay.down_conv1._prior_sample(torch.zeros((B, c["h_size"], 8, 8), device="cuda"),
                                           torch.zeros((B, c["z_size"], 8, 8), device="cuda"), c["z_size"])
    assert rc == amd._capi.IAF_ERR_UNSUPPORTED            # no fused form: generate_down takes the full conv + the sample launch
    g = np.load(os.path.join(golden_dir, "cvae1_forward.npz"))
    x_out = model.generate([dev(e) for e in c["noise"][0::2]])
    np.testing.assert_allclose(host(x_out), g["model_sample/x_out"], rtol=0, atol=2e-4)


def test_prior_form_range_report_then_bf16_planes(amd):
    """an input beyond fp16's range on the fp16-plane form: inf / NaN that call, IAF_ERR_RANGE once on the next (RuntimeWarning at layer
    level, the call repeated), then bf16 planes that match the oracle -- as the forward does"""
    zs, hs, B, H = 32, 160, 32, 8
    rng = np.random.RandomState(41)
    p = {}
    for nm, (ci, co) in (("up_conv1", (hs, 2 * zs + 2 * hs)), ("up_conv3", (hs, hs)), ("down_conv1", (hs, 4 * zs + 2 * hs))):
        for k, v in gi.conv_params(rng, ci, co).items():
            p[nm + "/" + k] = v
    for k, v in gi.ar_multiconv2d_params(rng, zs, [hs, hs], [zs, zs]).items():
        p["ar_multiconv2d/" + k] = v
    for k, v in gi.conv_params(rng, hs + zs, hs).items():
        p["down_conv2/" + k] = v
    p["down_conv1/g"] = np.full(4 * zs + 2 * hs, -9.0)     # small filters: the operand beyond 65504 moves the outputs by ~0.2 (all finite)
    layer = amd.IAFLayer(zs, hs, depth_ar=2, kl_min=0.25, mode="sample")
    layer.load({k: dev(v) for k, v in p.items()})
    assert layer.down_conv1.runs_f16x2(B, H, H)
    inp = 0.5 * rng.standard_normal((B, hs, H, H))
    inp[1, 3, 2, 2] = 7e4                                  # elu(7e4) = 7e4 > 65504
    eps = rng.standard_normal((B, zs, H, H))
    layer.generate_down(dev(inp), dev(eps))                # the launch that meets the operand (its output carries inf / NaN)
    torch.cuda.synchronize()
    assert layer.down_conv1.range_errors() != 0
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = layer.generate_down(dev(inp), dev(eps))
    assert any(issubclass(x.category, RuntimeWarning) for x in w)
    assert not layer.down_conv1.runs_f16x2(B, H, H)
    p32 = {k: f32(v) for k, v in p.items()}
    want, _, _, _ = O.iaf_layer_down(f32(inp), p32, None, None, None, None, zs, hs, 0.25, mode="sample", eps_prior=f32(eps))
    got = host(out)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-4)


def test_generate_validates_noise(amd):
    c = gi.model_case_inputs("model_sample")
    model = build_model(amd, c)
    eps = [dev(e) for e in c["noise"][0::2]]
    with pytest.raises(ValueError):
        model.generate(eps[:-1])                           # one tensor short
    bad = list(eps)
    bad[2] = torch.zeros((c["B"], c["z_size"], 4, 4), device="cuda")      # wrong resolution for that layer (8x8: the finer level)
    with pytest.raises(ValueError):
        model.generate(bad)
    bad = list(eps)
    bad[3] = eps[3][:1].clone()                            # batch differs from the first tensor
    with pytest.raises(ValueError):
        model.generate(bad)
    bad = list(eps)
    bad[0] = eps[0].double()
    with pytest.raises(ValueError):
        model.generate(bad)
    fresh = amd.CVAE1(z_size=c["z_size"], h_size=c["h_size"], depth=c["depth"], num_blocks=c["num_blocks"], image_size=c["image_size"])
    with pytest.raises(RuntimeError):
        fresh.generate(eps)


# -- 7. graph capture --------------------------------------------------------------------------------------------------------------
def test_generate_graph_replay_equals_eager(amd):
    c = gi.model_case_inputs("model_cfg")
    model = build_model(amd, c, mode="sample")
    B = 8
    eps_static = [dev(e) for e in prior_noise(c, B, 1)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.generate(eps_static)                         # eager warm-up on the capture stream
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out_static = model.generate(eps_static)
    for seed in (2, 3):
        new = [dev(e) for e in prior_noise(c, B, seed)]
        for s, n in zip(eps_static, new):
            s.copy_(n)
        torch.cuda.synchronize()
        g.replay()
        want = model.generate(new)
        torch.cuda.synchronize()
        assert torch.equal(out_static, want)
