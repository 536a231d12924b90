"""GPU tests of the noise source inside the model (iaf_amd.NoiseSource behind CVAE1.draw_noise / sample / iw_eval and
TrainStep(noise_source=)): the drawn lists have forward()'s layout, and every path that draws its own noise computes, bit for bit,
what the same path computes on the lists a same-seed source draws at the same steps."""
import numpy as np
import pytest
import torch

import golden_inputs as gi

pytestmark = pytest.mark.gpu

LR = 2e-3
SEED = 2024


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()
    return iaf_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def build_model(amd, c, mode=None, k=None):
    m = amd.CVAE1(z_size=c["z_size"], h_size=c["h_size"], kl_min=c["kl_min"], depth=c["depth"], num_blocks=c["num_blocks"],
                  k=c["k"] if k is None else k, image_size=c["image_size"], mode=mode or c["mode"])
    m.load({k_: dev(v) for k_, v in c["params"].items()})
    return m


def train_model(amd, c):
    model = amd.CVAE1(z_size=c["z_size"], h_size=c["h_size"], kl_min=c["kl_min"], depth=c["depth"], num_blocks=c["num_blocks"], k=1,
                      image_size=c["image_size"])
    model.set_training(True)
    model.load({k: dev(v) for k, v in c["params"].items()})
    return model


# -- draw_noise -------------------------------------------------------------------------------------------------------------------------
def test_draw_noise_layout_and_forward(amd):
    c = gi.model_case_inputs("model_cfg")
    model = build_model(amd, c)
    B = c["B"]
    shapes = model.noise_shapes(B)
    assert shapes == [tuple(e.shape) for e in c["noise"]]
    lists = {}
    for which in ("both", "posterior", "prior"):
        src = amd.NoiseSource(SEED)
        src.seek(7)
        out = model.draw_noise(B, src, which=which)
        assert src.tell() == 8 and len(out) == len(shapes)
        for i, (t, sh) in enumerate(zip(out, shapes)):
            drawn = which == "both" or (i % 2 == 1) == (which == "posterior")
            assert (t is not None) == drawn, (which, i)
            if drawn:
                assert tuple(t.shape) == sh and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()
        lists[which] = out
    torch.cuda.synchronize()
    for i in range(len(shapes)):
        # a tensor's substream is its index in the FULL list: what is drawn does not depend on what is drawn with it
        assert torch.equal(lists["both"][i], lists["posterior" if i % 2 else "prior"][i]), i
        for j in range(i):
            assert shapes[i] != shapes[j] or not torch.equal(lists["both"][i], lists["both"][j]), (i, j)
    x = torch.from_numpy(c["x"]).cuda()
    x_out, obj, loss = model.forward(x, lists["both"])
    x_out2, obj2, _ = model.forward(x, lists["posterior"])         # mode "train" reads the posterior slots only
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x_out).all()) and bool(torch.isfinite(obj).all()) and bool(torch.isfinite(loss).all())
    assert torch.equal(x_out, x_out2) and torch.equal(obj, obj2)
    # out= refills the same buffers; temperature scales the prior entries only; advance=False repeats the step
    src = amd.NoiseSource(SEED)
    src.seek(7)
    buf = model.draw_noise(B, src, advance=False)
    ptrs = [t.data_ptr() for t in buf]
    again = model.draw_noise(B, src, out=buf, temperature=0.5, advance=False)
    assert again is buf and [t.data_ptr() for t in buf] == ptrs and src.tell() == 7
    torch.cuda.synchronize()
    for i, t in enumerate(buf):
        assert torch.equal(t, lists["both"][i] * 0.5 if i % 2 == 0 else lists["both"][i]), i
    with pytest.raises(ValueError):
        model.draw_noise(B, src, which="posterior", out=buf)       # a list drawn with another `which`
    with pytest.raises(ValueError):
        model.draw_noise(B + 1, src, out=buf)
    with pytest.raises(ValueError):
        model.draw_noise(B, src, which="neither")


# -- sample ---------------------------------------------------------------------------------------------------------------------------
def test_sample_equals_generate_on_the_drawn_prior_noise(amd):
    c = gi.model_case_inputs("model_cfg")
    model = build_model(amd, c, mode="sample")
    B = 8
    a, b = amd.NoiseSource(SEED), amd.NoiseSource(SEED)
    got = model.sample(B, a)
    eps = model.draw_noise(B, b, which="prior")[0::2]
    want = model.generate(eps)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, 3, c["image_size"], c["image_size"])
    assert torch.equal(got, want) and a.tell() == 1 == b.tell()
    cold = model.sample(B, a, temperature=0.5)                     # step 1
    eps = model.draw_noise(B, b, which="prior")[0::2]
    want = model.generate([e * 0.5 for e in eps])
    torch.cuda.synchronize()
    rel = float((cold - want).abs().max() / want.abs().max())
    print("sample(temperature=0.5) vs generate(0.5 * eps): max relative difference %.3e" % rel)
    assert rel <= 1e-6
    assert not torch.equal(cold, got)


def test_sample_graph_replay_equals_eager(amd):
    c = gi.model_case_inputs("model_cfg")
    model = build_model(amd, c, mode="sample")
    B = 8
    src, eager = amd.NoiseSource(SEED + 1), amd.NoiseSource(SEED + 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.sample(B, src)                                       # eager warm-up on the capture stream (step 0)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out_static = model.sample(B, src)
    torch.cuda.current_stream().wait_stream(side)
    for step in (1, 2, 3):
        g.replay()
        eager.seek(step)
        want = model.sample(B, eager)
        torch.cuda.synchronize()
        assert torch.equal(out_static, want), step
    assert src.tell() == 4
    del g


# -- iw_eval ----------------------------------------------------------------------------------------------------------------------------
def test_iw_eval_with_a_source_equals_the_lists_it_draws(amd):
    c = gi.model_case_inputs("model_cfg")
    model = build_model(amd, c, k=1)
    x = torch.from_numpy(c["x"]).cuda()
    a, b = amd.NoiseSource(SEED), amd.NoiseSource(SEED)
    a.seek(3)
    b.seek(3)
    got = model.iw_eval(x, k=5, noise_source=a)
    passes = [model.draw_noise(c["B"], b, which="posterior") for _ in range(5)]
    want = model.iw_eval(x, passes)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert a.tell() == 8
    for bad in (dict(), dict(noise_passes=passes, noise_source=a, k=5), dict(noise_source=a), dict(noise_source=a, k=0),
                dict(noise_passes=passes, k=5)):
        with pytest.raises(ValueError):
            model.iw_eval(x, **bad)


# -- TrainStep --------------------------------------------------------------------------------------------------------------------------
def _flat_equal(a, b, what):
    torch.cuda.synchronize()
    for k in ("params", "slot_m", "slot_v", "ema"):
        p, q = getattr(a.flat, k), getattr(b.flat, k)
        assert torch.equal(p, q), (what, k, float((p - q).abs().max()))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_train_step_draws_what_a_same_seed_source_draws(amd, graph):
    c = gi.model_case_inputs("model_cfg")                          # the case tests/test_hip_train_step.py trains
    B, s0 = c["B"], (1 << 32) - 2                                  # (the counter crosses 2^32 on the way)
    src, twin = amd.NoiseSource(SEED), amd.NoiseSource(SEED)
    src.seek(s0)
    ts = amd.TrainStep(train_model(amd, c), LR, graph=graph, noise_source=src)
    ref = amd.TrainStep(train_model(amd, c), LR, graph=graph)
    x = torch.from_numpy(c["x"]).cuda()
    for t in range(4):
        xt = torch.roll(x, t, 0)
        obj = ts(xt).clone()
        twin.seek(s0 + t)
        want = ref(xt, ref.model.draw_noise(B, twin, which="posterior")).clone()
        torch.cuda.synchronize()
        assert torch.equal(obj, want), (t, float(obj), float(want))
        _flat_equal(ts, ref, "call %d" % t)
    assert src.tell() == s0 + 4
    assert ts.skipped == 0 and ref.skipped == 0
    assert ts.graphed == graph and ref.graphed == graph
    if graph:
        assert ts.captures == 1 and ref.captures == 1


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_a_skipped_call_still_moves_the_source_on(amd, graph):
    """call 2 brings its own, poisoned list (the way tests/test_hip_train_step.py skips a step): it is skipped, it counts as a call,
    and call 3 draws at s0 + 3 -- not at s0 + 2 again"""
    c = gi.model_case_inputs("model_cfg")
    B, s0 = c["B"], 100
    src, twin = amd.NoiseSource(SEED), amd.NoiseSource(SEED)
    src.seek(s0)
    ts = amd.TrainStep(train_model(amd, c), LR, graph=graph, noise_source=src)
    ref = amd.TrainStep(train_model(amd, c), LR, graph=graph)
    x = torch.from_numpy(c["x"]).cuda()
    for t in range(4):
        twin.seek(s0 + t)
        noise = ref.model.draw_noise(B, twin, which="posterior")
        if t == 2:
            noise[5][1, 3, 4, 5] = float("nan")                    # one posterior eps of the 16x16 level
            ts(x, [None if e is None else e.clone() for e in noise])
            ref(x, noise)
            assert ts.skipped == 1 and ref.skipped == 1
        else:
            obj, want = ts(x).clone(), ref(x, noise).clone()
            torch.cuda.synchronize()
            assert torch.equal(obj, want), t
        if graph and t == 2:
            continue                  # (ts ran that call as eager launches, ref replayed its graph: both skipped, nothing moved in either)
        _flat_equal(ts, ref, "call %d" % t)
    _flat_equal(ts, ref, "end")
    assert src.tell() == s0 + 4 and ts.skipped == 1


def test_train_step_value_errors(amd):
    c = gi.model_case_inputs("model_cfg")
    x = torch.from_numpy(c["x"]).cuda()
    ts = amd.TrainStep(train_model(amd, c), LR, graph=False)
    with pytest.raises(ValueError):
        ts(x)                                                      # neither a source nor a list
    src = amd.NoiseSource(1)
    ts = amd.TrainStep(train_model(amd, c), LR, graph=False, noise_source=src)
    assert bool(torch.isfinite(ts(x)).all()) and src.tell() == 1
    assert bool(torch.isfinite(ts(x, noise=[dev(e) for e in c["noise"]])).all()) and src.tell() == 2    # a list still works, and counts
