"""GPU test of iaf_amd.EvalPass -- the reference's run_eval epoch (tf_train.py:293-327) as captured head / pass graphs over a device
dataset with the engine's own noise -- on the variables of golden_inputs.model_case_inputs("model_tiny") (z 4, h 8, depth 2, 2
blocks, 16x16) and a data set of 6 random uint8 images, against the CPU oracle (oracle.cvae1_forward, as tests/test_hip_model.py)
fed the very noise the pass drew: a second NoiseSource of the same seed through CVAE1.draw_noise(which="posterior") at steps
noise_step + (batch * k + pass), copied to the host.  rtol 2e-5 is that file's model-level tolerance.  kl_cost and log_pxz are per
row, so a row's bound does not depend on its batch: per_image[i] is checked against the oracle fed image i alone."""
import warnings

import numpy as np
import pytest
import torch

import golden_inputs as gi
from oracle import iaf_oracle as O

pytestmark = pytest.mark.gpu

SEED, DATA_SEED, N_IMAGES, RTOL = 1234, 77, 6, 2e-5


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()      # raises if the HIP extension is missing: no silent fallback
    return iaf_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _kw(c):
    return dict(z_size=c["z_size"], h_size=c["h_size"], kl_min=c["kl_min"], depth=c["depth"], num_blocks=c["num_blocks"],
                image_size=c["image_size"])


def _model(amd, c, params=None, **over):
    m = amd.CVAE1(**dict(_kw(c), **over))
    m.load({k: dev(v) for k, v in c["params"].items()} if params is None else params)
    return m


@pytest.fixture(scope="module")
def tiny(amd):
    """the case, its images on the host and on the device, and one loaded evaluation model the tests share"""
    c = gi.model_case_inputs("model_tiny")
    images = np.random.RandomState(6).randint(0, 256, size=(N_IMAGES, 3, c["image_size"], c["image_size"])).astype(np.uint8)
    return dict(c=c, images=images, dimages=torch.from_numpy(images).cuda(), model=_model(amd, c),
                p64={k: f32(v) for k, v in c["params"].items()}, cache={})


def _bits_per_dim(c, loss, images):
    return loss / (np.log(2.0) * 3 * c["image_size"] ** 2 * images)


def _oracle_bounds(amd, t, B, k, noise_step, order, params64=None):
    """{image index: the oracle's k-sample bound of that image alone}, for the batches whose image indices are order[b], with the
    noise rows the pass gave them: step noise_step + b k + s, row r of the [B, ...] tensors; the k passes merged image-major, as
    the k-sample forward wants them (tests/test_hip_model.py)"""
    c, model = t["c"], t["model"]
    src = amd.NoiseSource(SEED)
    out = {}
    for b, idx in enumerate(order):
        passes = []
        for s in range(k):
            src.seek(noise_step + b * k + s)
            lst = model.draw_noise(B, src, which="posterior")
            torch.cuda.synchronize()
            passes.append([None if e is None else e.cpu().numpy().astype(np.float64) for e in lst])
        for r, i in enumerate(idx):
            merged = []
            for li in range(len(passes[0])):
                if passes[0][li] is None:                     # (the prior's draw: not read in mode "train")
                    shape = passes[0][li + 1].shape[1:] if li + 1 < len(passes[0]) else None
                    merged.append(np.zeros((k,) + shape))
                else:
                    merged.append(np.stack([passes[s][li][r] for s in range(k)], axis=0))
            loss = O.cvae1_forward(t["images"][i:i + 1], params64 or t["p64"], c["z_size"], c["h_size"], c["depth"], c["num_blocks"],
                                   c["kl_min"], k, merged)[2]
            out[int(i)] = float(loss)
    return out


def _in_order(B):
    return [list(range(b * B, (b + 1) * B)) for b in range(N_IMAGES // B)]


def _check_against(r, per_image, want, c):
    total = sum(want.values())
    got = per_image.cpu().numpy().astype(np.float64)
    worst = max(abs(got[i] - w) / abs(w) for i, w in want.items())
    print("loss %.9g (oracle %.9g, rel %.2e), worst per-image rel %.2e" % (r["loss"], total, abs(r["loss"] - total) / abs(total), worst))
    np.testing.assert_allclose(r["loss"], total, rtol=RTOL)
    np.testing.assert_allclose(r["eval_bits_per_dim"], _bits_per_dim(c, total, len(want)), rtol=RTOL)
    for i, w in want.items():
        np.testing.assert_allclose(got[i], w, rtol=RTOL, err_msg="image %d" % i)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("B", [2, 3])
def test_eval_pass_vs_oracle(amd, tiny, B, graph, k):
    c = tiny["c"]
    data = amd.DeviceDataset(tiny["dimages"], DATA_SEED, deterministic=True)
    src = amd.NoiseSource(SEED)
    src.seek(5)
    ev = amd.EvalPass(tiny["model"], data, B, src, k=k, graph=graph, per_image=True)
    r = ev.run()
    assert ev.graphed == graph and ev.graph_refused is None
    assert (r["images"], r["nonfinite"], r["batches"], r["k"], r["noise_step"]) == (N_IMAGES, 0, N_IMAGES // B, k, 5)
    assert src.tell() == 5 + (N_IMAGES // B) * k, "the source is left where the last pass put it"
    key = (B, k)
    if key not in tiny["cache"]:                              # one oracle evaluation per (B, k), shared by graph / eager
        tiny["cache"][key] = _oracle_bounds(amd, tiny, B, k, 5, _in_order(B))
    want = tiny["cache"][key]
    assert sorted(want) == list(range(N_IMAGES))
    _check_against(r, ev.per_image, want, c)
    if "loss" in tiny["cache"].get(("seen", B, k), {}):       # the result does not depend on `graph`
        assert tiny["cache"][("seen", B, k)]["loss"] == r["loss"]
        assert torch.equal(tiny["cache"][("seen", B, k)]["per_image"], ev.per_image.cpu())
    tiny["cache"][("seen", B, k)] = dict(loss=r["loss"], per_image=ev.per_image.cpu())


def test_shuffled_dataset_lands_every_image_under_its_index(amd, tiny):
    B, k = 2, 1
    data = amd.DeviceDataset(tiny["dimages"], DATA_SEED, deterministic=False)
    twin = amd.DeviceDataset(tiny["dimages"], DATA_SEED, deterministic=False)
    ev = amd.EvalPass(tiny["model"], data, B, amd.NoiseSource(SEED), k=k, per_image=True)
    r = ev.run()
    assert bool(torch.isfinite(ev.per_image).all()) and r["images"] == N_IMAGES and r["nonfinite"] == 0
    order = []
    for _ in range(N_IMAGES // B):
        idx = torch.zeros(B, dtype=torch.int64, device="cuda")
        twin.next_batch(B, indices=idx)
        order.append([int(v) for v in idx.cpu()])
    assert sorted(i for o in order for i in o) == list(range(N_IMAGES)), "one epoch of the shuffled set is a permutation"
    assert order != _in_order(B), "this seed does shuffle"
    _check_against(r, ev.per_image, _oracle_bounds(amd, tiny, B, k, 0, order), tiny["c"])


def test_repeat_runs_draw_later_noise_and_a_seek_repeats_a_run_bit_for_bit(amd, tiny):
    B, k = 3, 2
    data = amd.DeviceDataset(tiny["dimages"], DATA_SEED, deterministic=True)
    src = amd.NoiseSource(SEED)
    ev = amd.EvalPass(tiny["model"], data, B, src, k=k, per_image=True)
    r1 = ev.run()
    p1 = ev.per_image.clone()
    r2 = ev.run()
    assert r1["noise_step"] == 0 and r2["noise_step"] == r1["batches"] * k == 4
    assert r2["loss"] != r1["loss"] and np.isfinite(r2["loss"])
    src.seek(0)
    r3 = ev.run()
    assert r3 == r1 and torch.equal(ev.per_image.view(torch.int32), p1.view(torch.int32))
    assert ev.graphed and ev.captures == {"head": 1, "pass": 1}
    half = ev.run(batches=1)
    assert (half["images"], half["batches"]) == (B, 1)
    got = ev.per_image.cpu()
    assert bool(torch.isfinite(got[:B]).all()) and bool(torch.isnan(got[B:]).all()), "NaN where the run did not come"
    assert ev.captures == {"head": 1, "pass": 1}


def test_in_place_changes_of_the_loaded_variables_are_picked_up_by_the_next_run(amd, tiny):
    """run() re-derives the weight norms; at these channel counts (the generic stacks, which the batched prep launches do not cover)
    prepare_weights goes through every object's own prep launch"""
    c, B = tiny["c"], 3
    params = {k: dev(v) for k, v in c["params"].items()}
    src = amd.NoiseSource(SEED)
    ev = amd.EvalPass(_model(amd, c, params=params), amd.DeviceDataset(tiny["dimages"], DATA_SEED, deterministic=True), B, src)
    r1 = ev.run()
    with torch.no_grad():
        params["IAF_1_0/up_conv1/g"].add_(0.25)
        params["IAF_0_1/ar_multiconv2d/layer_out_0/g"].sub_(0.5)
        params["x_dec/g"].add_(0.125)
    src.seek(0)
    r2 = ev.run()
    fresh = _model(amd, c, params={k: v.detach().clone() for k, v in params.items()})
    want = amd.EvalPass(fresh, amd.DeviceDataset(tiny["dimages"], DATA_SEED, deterministic=True), B, amd.NoiseSource(SEED)).run()
    assert r2 == want and r2["loss"] != r1["loss"] and ev.captures == {"head": 1, "pass": 1}


def test_ema_views_are_evaluated_as_they_stand(amd):
    """on "model_cfg" (z 32, h 160, 2 blocks, 32x32: the case tests/test_hip_train_step.py trains) and 6 random images: the channel
    counts of "model_tiny" run the generic kernels, which have no batched weight-norm backward, so no TrainStep can be built on it"""
    c = gi.model_case_inputs("model_cfg")
    B = 2
    images = np.random.RandomState(8).randint(0, 256, size=(N_IMAGES, 3, c["image_size"], c["image_size"])).astype(np.uint8)
    tiny = dict(dimages=torch.from_numpy(images).cuda())
    trainee = amd.CVAE1(**_kw(c))
    trainee.set_training(True)
    trainee.load({k: dev(v) for k, v in c["params"].items()})
    ts = amd.TrainStep(trainee, 0.01, noise_source=amd.NoiseSource(SEED + 1), data=amd.DeviceDataset(tiny["dimages"], DATA_SEED), batch_size=B,
                       ema_decay=0.9)
    for _ in range(3):
        ts()
    assert ts.skipped == 0
    ema = ts.ema_params()
    assert list(ema) == list(ts.flat.p) and all(ema[k].shape == ts.flat.p[k].shape for k in ema)
    eval_model = _model(amd, c, params=ema)                  # loaded ONCE

    def fresh_run(params):
        m = _model(amd, c, params={k: v.detach().clone() for k, v in params.items()})
        return amd.EvalPass(m, amd.DeviceDataset(tiny["dimages"], DATA_SEED, deterministic=True), B, amd.NoiseSource(SEED)).run()

    src = amd.NoiseSource(SEED)
    ev = amd.EvalPass(eval_model, amd.DeviceDataset(tiny["dimages"], DATA_SEED, deterministic=True), B, src)
    r = ev.run()
    assert r["nonfinite"] == 0 and r["images"] == N_IMAGES
    assert r == fresh_run(ema), "a model loaded from the EMA views == one loaded from copies of them"
    assert r["loss"] != fresh_run(ts.flat.p)["loss"], "the average is not the parameters"
    ts()                                                      # the views move under the loaded model
    assert ts.skipped == 0
    src.seek(0)
    r2 = ev.run()                                             # no load in between
    assert r2["loss"] != r["loss"]
    assert r2 == fresh_run(ema)
    assert ev.captures == {"head": 1, "pass": 1}


def test_an_fp16_overflow_is_moved_to_bf16_planes_and_the_run_repeated(amd):
    """the geometry and weights of test_a_real_fp16_overflow_is_skipped_then_trained_through_on_bf16_planes
    (tests/test_hip_train_step.py): exp(g) + 15 on the first hidden layer of one IAF stack and -15 on its two output layers -- put
    into the loaded variables in place AFTER a first run has captured the pass on fp16 planes, as that test does behind its first
    step (weights that overflow from the start are already met, and moved, by the compute-only batch in front of the capture)"""
    from iaf_amd.train import _range_objects
    c = gi.model_case_inputs("model_cfg")
    B = c["B"]
    images = torch.from_numpy(c["x"]).cuda()
    params = {k: dev(v) for k, v in c["params"].items()}
    model = _model(amd, c, params=params)
    st = model.layers[0][0].posterior.stack
    src = amd.NoiseSource(SEED)
    ev = amd.EvalPass(model, amd.DeviceDataset(images, DATA_SEED, deterministic=True), B, src)
    first = ev.run()
    assert first["nonfinite"] == 0 and ev.captures == {"head": 1, "pass": 1}
    assert st.step_is_f16(B, 16, 16), "the 16x16 stack must run its step on two fp16 planes at B = %d" % B
    pre = "IAF_0_0/ar_multiconv2d/"
    with torch.no_grad():
        params[pre + "layer_1/g"].add_(15.0)
        params[pre + "layer_out_0/g"].sub_(15.0)
        params[pre + "layer_out_1/g"].sub_(15.0)
    torch.cuda.synchronize()
    p = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in params.items()}
    src.seek(0)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        r = ev.run()
    mine = [w for w in seen if issubclass(w.category, RuntimeWarning) and str(w.message).startswith("EvalPass")]
    assert len(mine) == 1, "the first run was finite (%d EvalPass warnings): the test's weights do not overflow the fp16-plane step" % len(mine)
    assert not st.step_is_f16(B, 16, 16), "the stack has moved to bf16 planes"
    assert (r["nonfinite"], r["images"], r["noise_step"]) == (0, B, 0) and np.isfinite(r["loss"])
    assert src.tell() == 1, "the repeated run drew the first run's noise again"
    assert ev.graphed and ev.captures == {"head": 2, "pass": 2}
    moved = amd.CVAE1(**_kw(c))
    for o in _range_objects(moved):
        o.set_precision("bf16x3")
    moved.load({k: dev(v) for k, v in p.items()})
    want = amd.EvalPass(moved, amd.DeviceDataset(images, DATA_SEED, deterministic=True), B, amd.NoiseSource(SEED)).run()
    assert want["nonfinite"] == 0
    print("after the move: loss %.9g, on bf16 planes from the start %.9g" % (r["loss"], want["loss"]))
    np.testing.assert_allclose(r["loss"], want["loss"], rtol=RTOL)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        src.seek(0)
        again = ev.run()
    assert not [w for w in seen if str(w.message).startswith("EvalPass")] and again == r


def test_value_errors(amd, tiny):
    c, model, images = tiny["c"], tiny["model"], tiny["dimages"]
    data = amd.DeviceDataset(images, DATA_SEED, deterministic=True)
    src = amd.NoiseSource(SEED)
    for bad_k in (0, -1, True, 1.5):
        with pytest.raises(ValueError):
            amd.EvalPass(model, data, 2, src, k=bad_k)
    with pytest.raises(ValueError):
        amd.EvalPass(_model(amd, c, k=2), data, 2, src)
    with pytest.raises(ValueError):
        amd.EvalPass(_model(amd, c, towers=2), data, 2, src)
    with pytest.raises(ValueError):
        amd.EvalPass(amd.CVAE1(**_kw(c)), data, 2, src)       # not loaded
    with pytest.raises(ValueError):
        amd.EvalPass(model, data, 4, src)                     # 6 % 4
    with pytest.raises(ValueError):
        amd.EvalPass(model, amd.DeviceDataset(images, DATA_SEED, deterministic=True, rank=0, world=2), 2, src)
    with pytest.raises(ValueError):
        amd.EvalPass(model, data, 2, None)
    with pytest.raises(ValueError):
        amd.EvalPass(model, images, 2, src)
    ev = amd.EvalPass(model, data, 2, src, graph=False)
    for bad in (0, 4, -1, True, 1.0):
        with pytest.raises(ValueError):
            ev.run(batches=bad)
    assert ev._buf is None and src.tell() == 0, "a refused call launches nothing"
