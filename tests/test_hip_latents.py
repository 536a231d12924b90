"""GPU tests of latent access: CVAE1.encode / decode / reconstruct / reconstruct_ladder, IAFLayer.down_from under them, iaf_amd.lerp_latents,
and down_conv1 in h_det-only form (WNConv2d.hdet, iaf_conv3x3_forward_hdet: the prior-form kernel with no (mean, logsd) unit, only the
n_h / 16 h_det tiles launched).  Against the CPU oracle and its mixed-pass restatement (tests/latents_reference.py), and -- exactly -- against
forward() / generate() on the GPU, whose launches the posterior and prior layers repeat.

Tolerances are those of tests/test_hip_generate.py for the same comparisons: h_det against the oracle conv 1e-4, against the full conv on the
GPU 1e-5; a model's x_out against the oracle 2e-4, against another GPU path 2e-5."""
import warnings

import numpy as np
import pytest
import torch

import golden_inputs as gi
import latents_reference as R
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


f32 = R.f32


def build_model(amd, c, mode="train"):
    m = amd.CVAE1(z_size=c["z_size"], h_size=c["h_size"], kl_min=c["kl_min"], depth=c["depth"], num_blocks=c["num_blocks"], k=1,
                  image_size=c["image_size"], mode=mode)
    m.load({k: dev(v) for k, v in c["params"].items()})
    return m


def case_b32():
    """model_cfg's geometry with 32 random images (the size at which the plain convs run two fp16 planes)"""
    gi.MODEL_CASES["latents_b32"] = (32, 1, 32, 160, 2, 2, 32, 0.25)
    return gi.model_case_inputs("latents_b32")


def layer_params(rng, zs, hs, ds=False):
    p = {}
    for nm, (ci, co) in (("up_conv1", (hs, 2 * zs + 2 * hs)), ("up_conv3", (hs, hs)), ("down_conv1", (hs, 4 * zs + 2 * hs))):
        for k, v in gi.conv_params(rng, ci, co).items():
            p[nm + "/" + k] = v
    for k, v in gi.ar_multiconv2d_params(rng, zs, [hs, hs], [zs, zs]).items():
        p["ar_multiconv2d/" + k] = v
    last = gi.deconv_params(rng, hs + zs, hs) if ds else gi.conv_params(rng, hs + zs, hs)
    for k, v in last.items():
        p[("down_deconv2/" if ds else "down_conv2/") + k] = v
    return p


# -- 1. the kernel: down_conv1 in h_det-only form ---------------------------------------------------------------------------------------
# one unit (2 tiles), 6, 8, the ragged 10 and 12 tiles; a partial last pixel block (5x7; 3 x 64 = 192 px fills its blocks, 35 does not);
# both arithmetics (32 x 16 x 16 = 8192 pixels run two fp16 planes, the small ones the bf16x3 planes)
KERNEL_CASES = [(16, 32, 1, 5, 7, True), (32, 96, 3, 8, 8, False), (32, 128, 3, 16, 16, True), (32, 160, 1, 5, 7, False),
                (32, 160, 3, 8, 8, True), (32, 160, 32, 16, 16, True), (64, 192, 2, 4, 4, True)]
GUARD = 64                  # floats in front of and behind h_det in one allocation
SENTINEL = -12345.5


def run_hdet_guarded(amd, conv, xd, zs, hs, elu):
    B, _, H, W = (int(v) for v in xd.shape)
    n = B * hs * H * W
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    h_det = buf[GUARD:GUARD + n].view(B, hs, H, W)
    rc = amd._capi.lib().iaf_conv3x3_forward_hdet(conv._h, amd.layers._ptr(xd), 1 if elu else 0, zs, hs, amd.layers._ptr(h_det), B, H, W,
                                                  amd.layers._stream())
    amd._capi.check(rc)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), "wrote outside h_det"
    return h_det


@pytest.mark.parametrize("zs,hs,B,H,W,elu", KERNEL_CASES)
def test_hdet_kernel_vs_oracle_and_full_conv(amd, zs, hs, B, H, W, elu):
    rng = np.random.RandomState(zs + hs + B + H * W)
    p = gi.conv_params(rng, hs, 4 * zs + 2 * hs)
    x = rng.standard_normal((B, hs, H, W))
    conv = amd.WNConv2d(hs, 4 * zs + 2 * hs)
    conv.prepare(dev(p["V"]), dev(p["g"]), dev(p["b"]))
    f16 = conv.runs_f16x2(B, H, W)
    if (B, H, W) == (32, 16, 16):
        assert f16                                             # 8192 pixels: two fp16 planes
    if B == 1:
        assert not f16                                         # 35 pixels: below the forward's size rule, the bf16x3 planes
    xd = dev(x)
    h_det = run_hdet_guarded(amd, conv, xd, zs, hs, elu)
    assert torch.equal(conv.hdet(xd, zs, elu_input=elu), h_det)
    xin = O.elu(f32(x)) if elu else f32(x)
    hd = O.split_channels(O.conv2d(xin, f32(p["V"]), f32(p["g"]), f32(p["b"])), [zs] * 4 + [hs] * 2)[5]
    err_o = float(np.abs(host(h_det) - hd).max())
    hd2 = conv(xd, elu_input=elu, split=[zs] * 4 + [hs] * 2)[5]
    err_g = float(np.abs(host(h_det) - host(hd2)).max())
    print("h_det z %d h %d B %d %dx%d: max err vs oracle %.3e, vs the full conv %.3e" % (zs, hs, B, H, W, err_o, err_g))
    assert err_o <= 1e-4
    assert err_g <= 1e-5


@pytest.mark.parametrize("shape", ["4,3", "4,2", "2,3", "4,1", "2,2", "2,1"])
def test_hdet_every_compiled_launch_shape_on_the_ragged_case(amd, shape, monkeypatch):
    """10 h_det tiles under every compiled (NT, WCO) of the prior form, chosen by the dev override IAF_HDET_SHAPE: 12 or 16 launched tiles
    for 10 -- tiles past the last read a valid one and store nothing"""
    zs, hs, B, H, W = 32, 160, 3, 8, 8
    rng = np.random.RandomState(77)
    p = gi.conv_params(rng, hs, 4 * zs + 2 * hs)
    conv = amd.WNConv2d(hs, 4 * zs + 2 * hs)
    conv.prepare(dev(p["V"]), dev(p["g"]), dev(p["b"]))
    xd = dev(rng.standard_normal((B, hs, H, W)))
    want = conv(xd, elu_input=True, split=[zs] * 4 + [hs] * 2)[5]
    monkeypatch.setenv("IAF_HDET_SHAPE", shape)
    h_det = run_hdet_guarded(amd, conv, xd, zs, hs, True)
    assert float(np.abs(host(h_det) - host(want)).max()) <= 1e-5


def test_hdet_argument_errors(amd):
    lib, P, E = amd._capi.lib(), amd.layers._ptr, amd._capi
    conv = amd.WNConv2d(32, 4 * 16 + 2 * 32)
    x = torch.zeros((1, 32, 4, 4), device="cuda")
    h = torch.zeros((1, 32, 4, 4), device="cuda")
    st = amd.layers._stream()
    # argument errors come before the prepare check and before any device work
    assert lib.iaf_conv3x3_forward_hdet(conv._h, P(x), 1, 16, 16, P(h), 1, 4, 4, st) == E.IAF_ERR_SHAPE
    assert lib.iaf_conv3x3_forward_hdet(conv._h, P(x), 1, 16, 32, P(h), 0, 4, 4, st) == E.IAF_ERR_SHAPE
    assert lib.iaf_conv3x3_forward_hdet(conv._h, P(x), 1, 16, 32, None, 1, 4, 4, st) == E.IAF_ERR_NULL
    assert lib.iaf_conv3x3_forward_hdet(conv._h, P(x), 1, 16, 32, P(h), 1, 4, 4, st) == E.IAF_ERR_NOT_PREPARED
    masked = amd.WNConv2d(32, 128, ar_mask=False)
    assert lib.iaf_conv3x3_forward_hdet(masked._h, P(x), 1, 16, 32, P(h), 1, 4, 4, st) == E.IAF_ERR_UNSUPPORTED
    tiny = amd.WNConv2d(8, 4 * 4 + 2 * 8)                  # generic channel counts: no such form
    assert lib.iaf_conv3x3_forward_hdet(tiny._h, P(x), 1, 4, 8, P(h), 1, 4, 4, st) == E.IAF_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        conv.hdet(torch.zeros((1, 16, 4, 4), device="cuda"), 16)          # wrong channel count
    with pytest.raises(ValueError):
        conv.hdet(x, 40)                                                   # n_out = 128 is not 4 n_z + 2 n_h for any n_h


# -- 2. the layer: down_from ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds", [False, True], ids=["plain", "downsample"])
def test_down_from_given_z_matches_reference_layer(amd, ds):
    zs, hs, B, H = 32, 160, 3, 8
    rng = np.random.RandomState(51 + ds)
    p = layer_params(rng, zs, hs, ds)
    layer = amd.IAFLayer(zs, hs, depth_ar=2, kl_min=0.25, downsample=ds, mode="train")
    layer.load({k: dev(v) for k, v in p.items()})
    inp, z = rng.standard_normal((B, hs, H, H)), rng.standard_normal((B, zs, H, H))
    zd = dev(z)
    out, z_ret, cost = layer.down_from(dev(inp), zd)
    assert z_ret is zd and cost is None and layer.posterior.qz_mean is None
    want = R.given_z_down(f32(inp), {k: f32(v) for k, v in p.items()}, f32(z), zs, hs, ds)
    assert tuple(out.shape) == want.shape
    np.testing.assert_allclose(host(out), want, rtol=0, atol=2e-4)


def test_down_from_posterior_and_prior_repeat_down_and_generate_down(amd):
    zs, hs, B, H = 32, 160, 3, 8
    rng = np.random.RandomState(53)
    p = layer_params(rng, zs, hs)
    layer = amd.IAFLayer(zs, hs, depth_ar=2, kl_min=0.25, mode="train")
    layer.load({k: dev(v) for k, v in p.items()})
    inp, eps = dev(rng.standard_normal((B, hs, H, H))), dev(rng.standard_normal((B, zs, H, H)))
    with pytest.raises(RuntimeError):
        layer.down_from(inp, "posterior", eps)             # no up pass yet
    with pytest.raises(ValueError):
        layer.down_from(inp, "posteriour", eps)
    with pytest.raises(ValueError):
        layer.down_from(inp, "prior")
    layer.up(dev(rng.standard_normal((B, hs, H, H))))
    want, _, want_cost = layer.down(inp, eps)
    want_z = layer.last_block["z"]
    out, z, cost = layer.down_from(inp, "posterior", eps)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(z, want_z) and torch.equal(cost, want_cost)
    out, z, cost = layer.down_from(inp, "prior", eps)
    torch.cuda.synchronize()
    assert cost is None and torch.equal(out, layer.generate_down(inp, eps))
    assert torch.equal(z, layer.down_conv1.prior_sample(inp, eps, zs)[0])


def test_hdet_form_range_report_then_bf16_planes(amd):
    """an input beyond fp16's range on the fp16-plane form (the 7e4 operand of test_prior_form_range_report_then_bf16_planes), on down_from
    with a given z: inf / NaN that call, IAF_ERR_RANGE once on the next (RuntimeWarning at layer level, the call repeated), then bf16
    planes that match the reference"""
    zs, hs, B, H = 32, 160, 32, 8
    rng = np.random.RandomState(41)
    p = layer_params(rng, zs, hs)
    p["down_conv1/g"] = np.full(4 * zs + 2 * hs, -9.0)     # small filters: the operand beyond 65504 moves the outputs by ~0.2 (all finite)
    layer = amd.IAFLayer(zs, hs, depth_ar=2, kl_min=0.25, mode="sample")
    layer.load({k: dev(v) for k, v in p.items()})
    assert layer.down_conv1.runs_f16x2(B, H, H)
    inp = 0.5 * rng.standard_normal((B, hs, H, H))
    inp[1, 3, 2, 2] = 7e4                                  # elu(7e4) = 7e4 > 65504
    z = rng.standard_normal((B, zs, H, H))
    layer.down_from(dev(inp), dev(z))                      # the launch that meets the operand (its output carries inf / NaN)
    torch.cuda.synchronize()
    assert layer.down_conv1.range_errors() != 0
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out, _, _ = layer.down_from(dev(inp), dev(z))
    assert any(issubclass(x.category, RuntimeWarning) for x in w)
    assert not layer.down_conv1.runs_f16x2(B, H, H)
    want = R.given_z_down(f32(inp), {k: f32(v) for k, v in p.items()}, f32(z), zs, hs, False)
    got = host(out)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-4)


# -- 3. the model, exactly: the posterior and prior layers repeat forward()'s and generate()'s launches -------------------------------------
@pytest.mark.parametrize("which", ["B2_bf16x3", "B32_f16x2"])
def test_model_exactness_against_forward_and_generate(amd, which):
    c = gi.model_case_inputs("model_cfg") if which == "B2_bf16x3" else case_b32()
    B, nl = c["B"], c["depth"] * c["num_blocks"]
    model = build_model(amd, c, mode="train")
    assert model.layers[0][1].down_conv1.runs_f16x2(B, 16, 16) == (B == 32)
    x, noise = torch.from_numpy(c["x"]).cuda(), [dev(e) for e in c["noise"]]
    x_fwd, _, _ = model.forward(x, noise)
    z_fwd = [layer.last_block["z"] for layer, _ in model._layers_top_down()]
    kl_fwd = [layer.last_block["kl_cost"] for layer, _ in model._layers_top_down()]
    x_gen = model.generate(noise[0::2])
    assert torch.equal(model.reconstruct(x, noise, nl), x_fwd)
    enc = model.encode(x, [None if i % 2 == 0 else e for i, e in enumerate(noise)])
    torch.cuda.synchronize()
    assert torch.equal(enc["x_out"], x_fwd) and tuple(enc["kl_cost"].shape) == (nl, B)
    for li in range(nl):
        assert tuple(enc["z"][li].shape) == tuple(noise[2 * li].shape)
        assert torch.equal(enc["z"][li], z_fwd[li]), li
        assert torch.equal(enc["kl_cost"][li], kl_fwd[li]), li
    assert torch.equal(model.decode([None] * nl, noise[0::2]), x_gen)
    assert torch.equal(model.reconstruct(x, [e if i % 2 == 0 else None for i, e in enumerate(noise)], 0), x_gen)
    # decode(encode(x).z) against forward: another path on the GPU (h_det from the h_det-only form)
    np.testing.assert_allclose(host(model.decode(enc["z"])), host(x_fwd), rtol=0, atol=2e-5)


# -- 4. the model against the reference: the generic fallback (z 4 / h 8) and the BASELINE geometry ----------------------------------------
@pytest.mark.parametrize("name", ["model_tiny", "model_cfg"])
def test_model_against_reference(amd, name):
    ref = R.case_reference(name)
    c, nl = ref["c"], ref["nl"]
    model = build_model(amd, c, mode="sample")             # (the mode the model was built with does not matter)
    x, noise = torch.from_numpy(c["x"]).cuda(), [dev(e) for e in c["noise"]]
    for n in range(nl + 1):
        err = float(np.abs(host(model.reconstruct(x, noise, n)) - ref["recs"][n][0]).max())
        print("%s: reconstruct(%d) max err %.3e" % (name, n, err))
        assert err <= 2e-4
    x_ref, z_ref, _ = ref["recs"][nl]
    err = float(np.abs(host(model.decode([dev(z) for z in z_ref])) - x_ref).max())
    print("%s: decode(reference z) max err %.3e" % (name, err))
    assert err <= 2e-4
    # given latents on top, the prior below: the three sources in one pass
    n = nl // 2
    got = model.decode([dev(z) for z in ref["recs"][n][1][:n]] + [None] * (nl - n), [None] * n + noise[2 * n::2])
    assert float(np.abs(host(got) - ref["recs"][n][0]).max()) <= 2e-4
    enc = model.encode(x, noise)
    x_fwd = build_model(amd, c, mode="train").forward(x, noise)[0]
    np.testing.assert_allclose(host(model.decode(enc["z"])), host(x_fwd), rtol=0, atol=2e-5)


def test_decode_with_down_conv1_pinned_to_fp32_or_trimmed(amd):
    """no h_det-only form (fp32 pinned: IAF_ERR_UNSUPPORTED) or its pack trimmed away (IAF_ERR_NOT_PREPARED): the full down_conv1's sixth piece"""
    ref = R.case_reference("model_cfg")
    c, nl = ref["c"], ref["nl"]
    x_ref, z_ref, _ = ref["recs"][nl]
    model = build_model(amd, c)
    for layer, _ in model._layers_top_down():
        layer.down_conv1.set_precision("f32")
    model.load({k: dev(v) for k, v in c["params"].items()})
    lay = model.layers[0][0]
    rc, _ = lay.down_conv1._hdet(torch.zeros((c["B"], c["h_size"], 16, 16), device="cuda"), c["z_size"])
    assert rc == amd._capi.IAF_ERR_UNSUPPORTED
    assert float(np.abs(host(model.decode([dev(z) for z in z_ref])) - x_ref).max()) <= 2e-4
    model = build_model(amd, c)
    kept = model.trim_packs(c["B"])
    # the h_det-only form reads the fp16-plane pack where the forward runs that, else the bf16x3 pack: a conv whose forward keeps another one
    # has none for it (2 x 16 x 16 pixels are below the forward's split-product size rule: only the fp32 pack is kept)
    dc1 = model.layers[0][0].down_conv1
    rc, _ = dc1._hdet(torch.zeros((c["B"], c["h_size"], 16, 16), device="cuda"), c["z_size"])
    assert kept[(0, 0)]["down_conv1"] == "f32" and rc == amd._capi.IAF_ERR_NOT_PREPARED
    assert float(np.abs(host(model.decode([dev(z) for z in z_ref])) - x_ref).max()) <= 2e-4


# -- 5. ladder, interpolation, capture -----------------------------------------------------------------------------------------------------
def test_ladder_slices_equal_reconstruct_and_feed_image_grid(amd):
    c = gi.model_case_inputs("model_cfg")
    B, nl, S = c["B"], c["depth"] * c["num_blocks"], c["image_size"]
    model = build_model(amd, c)
    x, noise = torch.from_numpy(c["x"]).cuda(), [dev(e) for e in c["noise"]]
    steps = [0, 3, nl, 1]
    lad = model.reconstruct_ladder(x, noise, steps)
    assert tuple(lad.shape) == (len(steps) * B, 3, S, S) and lad.is_contiguous()
    for s, n in enumerate(steps):
        assert torch.equal(lad[s * B:(s + 1) * B], model.reconstruct(x, noise, n)), n
    _, grid, records = amd.image_grid([(lad, len(steps) * B)], len(steps) * B)
    torch.cuda.synchronize()
    assert grid.dim() == 3 and bool(torch.isfinite(grid).all()) and int(records[:, 2].sum()) == 0


def test_lerp_latents_endpoints_and_midpoint(amd):
    rng = np.random.RandomState(3)
    za = [dev(rng.standard_normal(s)) for s in ((2, 4, 8, 8), (2, 4, 16, 16))]
    zb = [dev(rng.standard_normal(s)) for s in ((2, 4, 8, 8), (2, 4, 16, 16))]
    for alpha, want in ((0, za), (1, zb), (0.0, za), (1.0, zb)):
        got = amd.lerp_latents(za, zb, alpha)
        torch.cuda.synchronize()
        assert all(torch.equal(g, w) for g, w in zip(got, want))
    out = [torch.empty_like(a) for a in za]
    got = amd.lerp_latents(za, zb, 0.25, out=out)
    assert all(g is o for g, o in zip(got, out))
    for g, a, b in zip(got, za, zb):
        np.testing.assert_allclose(host(g), 0.75 * host(a) + 0.25 * host(b), rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        amd.lerp_latents(za, zb[:1], 0.5)
    with pytest.raises(ValueError):
        amd.lerp_latents(za, [zb[0], zb[1][:1].clone()], 0.5)
    with pytest.raises(ValueError):
        amd.lerp_latents(za, zb, True)


def test_decode_and_reconstruct_graph_replay_equals_eager(amd):
    c = gi.model_case_inputs("model_cfg")
    B, nl = c["B"], c["depth"] * c["num_blocks"]
    model = build_model(amd, c)
    rng = np.random.RandomState(9)
    draw = lambda: ([dev(rng.standard_normal(e.shape)) for e in c["noise"]],
                    torch.from_numpy(rng.randint(0, 256, size=c["x"].shape).astype(np.uint8)).cuda())
    noise_s, x_s = draw()
    z_s = [torch.empty_like(e) for e in noise_s[1::2]]
    given = lambda zs_: [zs_[0], None, zs_[2], zs_[3]]      # one layer from the prior among given ones
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.decode(given(z_s), noise_s[0::2])            # eager warm-up on the capture stream
        model.reconstruct(x_s, noise_s, 2)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            dec_s = model.decode(given(z_s), noise_s[0::2])
            rec_s = model.reconstruct(x_s, noise_s, 2)
    for _ in range(2):
        noise_n, x_n = draw()
        z_n = [dev(rng.standard_normal(e.shape)) for e in z_s]
        for s, n in zip(noise_s + z_s + [x_s], noise_n + z_n + [x_n]):
            s.copy_(n)
        torch.cuda.synchronize()
        g.replay()
        want_d, want_r = model.decode(given(z_n), noise_n[0::2]), model.reconstruct(x_n, noise_n, 2)
        torch.cuda.synchronize()
        assert torch.equal(dec_s, want_d) and torch.equal(rec_s, want_r)


# -- 6. validation: host-only, before any launch --------------------------------------------------------------------------------------------
def test_latent_calls_validate_their_inputs(amd):
    c = gi.model_case_inputs("model_cfg")
    B, nl, zs = c["B"], c["depth"] * c["num_blocks"], c["z_size"]
    model = build_model(amd, c)
    x, noise = torch.from_numpy(c["x"]).cuda(), [dev(e) for e in c["noise"]]
    z = [torch.zeros_like(e) for e in noise[1::2]]
    for bad in (z[:-1], z + [z[0]]):                       # wrong list length
        with pytest.raises(ValueError):
            model.decode(bad)
    with pytest.raises(ValueError):
        model.encode(x, noise[:-1])
    bad = list(z)
    bad[2] = torch.zeros((B, zs, 8, 8), device="cuda")     # wrong resolution for that layer (16x16: the finer level)
    with pytest.raises(ValueError):
        model.decode(bad)
    bad = list(z)
    bad[3] = z[3][:1].clone()                              # batch differs from the first tensor
    with pytest.raises(ValueError):
        model.decode(bad)
    bad = list(z)
    bad[0] = z[0].double()                                 # dtype
    with pytest.raises(ValueError):
        model.decode(bad)
    bad = list(z)
    bad[1] = None                                          # a layer from the prior without its noise
    with pytest.raises(ValueError):
        model.decode(bad)
    with pytest.raises(ValueError):
        model.decode(bad, [None] * nl)
    bad_noise = list(noise)
    bad_noise[1] = noise[1][:1].clone()                    # noise batch differs from x
    with pytest.raises(ValueError):
        model.reconstruct(x, bad_noise, nl)
    for n in (-1, nl + 1, 1.0, True):                      # posterior_layers outside 0 .. nl
        with pytest.raises(ValueError):
            model.reconstruct(x, noise, n)
    with pytest.raises(ValueError):
        model.reconstruct_ladder(x, noise, [])
    with pytest.raises(ValueError):
        model.reconstruct(x, [None] * len(noise), 1)       # the posterior noise of layer 0 is read
    with pytest.raises(RuntimeError):
        model._top_down_mixed(["posterior"] * nl, noise)   # a "posterior" layer without a bottom-up pass
    k2 = amd.CVAE1(z_size=zs, h_size=c["h_size"], depth=c["depth"], num_blocks=c["num_blocks"], image_size=c["image_size"], k=2)
    k2.load({k: dev(v) for k, v in c["params"].items()})
    for call in (lambda: k2.decode(z), lambda: k2.encode(x, noise), lambda: k2.reconstruct(x, noise, 1), lambda: k2.reconstruct_ladder(x, noise, [1])):
        with pytest.raises(ValueError):
            call()
    fresh = amd.CVAE1(z_size=zs, h_size=c["h_size"], depth=c["depth"], num_blocks=c["num_blocks"], image_size=c["image_size"])
    for call in (lambda: fresh.decode(z), lambda: fresh.encode(x, noise), lambda: fresh.reconstruct(x, noise, 1)):
        with pytest.raises(RuntimeError):
            call()
