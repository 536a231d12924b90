"""GPU test of EvalPass.images() -- run_eval's reconstruction and sample grids (tf_train.py:329-376) -- on the variables of
golden_inputs.model_case_inputs("model_tiny") (16x16 images) and a data set of 6 random uint8 images, B = 6, total = 4.

The tensors it returns are held BIT FOR BIT to the package's own launches at the steps it reports (CVAE1.forward on the dataset's
batch with the posterior noise of a second NoiseSource, CVAE1.sample at the step behind it): the launches are the same, and what they
compute is covered by tests/test_hip_model.py and tests/test_hip_generate.py.  The grids are held to tests/images_reference.py
applied to those returned tensors, within 2**-22 (tests/test_images_reference.py says why), the byte grids to the package's rule."""
import warnings

import numpy as np
import pytest
import torch

import golden_inputs as gi
import images_reference as R

pytestmark = pytest.mark.gpu

SEED, DATA_SEED, N_IMAGES, B, TOTAL, TOL = 1234, 77, 6, 6, 4, 2.0 ** -22


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()      # raises if the HIP extension is missing: no silent fallback
    return iaf_amd


@pytest.fixture(scope="module")
def tiny(amd):
    c = gi.model_case_inputs("model_tiny")
    images = np.random.RandomState(6).randint(0, 256, size=(N_IMAGES, 3, c["image_size"], c["image_size"])).astype(np.uint8)
    m = amd.CVAE1(z_size=c["z_size"], h_size=c["h_size"], kl_min=c["kl_min"], depth=c["depth"], num_blocks=c["num_blocks"],
                  image_size=c["image_size"])
    m.load({k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda() for k, v in c["params"].items()})
    return dict(c=c, images=images, dimages=torch.from_numpy(images).cuda(), model=m)


def _pass(amd, tiny, **kw):
    data = amd.DeviceDataset(tiny["dimages"], DATA_SEED, deterministic=True)
    src = amd.NoiseSource(SEED)
    return amd.EvalPass(tiny["model"], data, B, src, **kw), data, src


def test_images_returns_what_the_models_own_launches_give(amd, tiny):
    ev, data, src = _pass(amd, tiny)
    src.seek(5)
    r = ev.images(total=TOTAL)
    assert (r["data_step"], r["noise_step"], r["nonfinite"]) == (0, 5, 0)
    assert data.tell() == 1 and src.tell() == 7                                 # one batch, two steps of noise
    m, S = tiny["model"], tiny["c"]["image_size"]
    other = amd.NoiseSource(SEED)
    batch = amd.DeviceDataset(tiny["dimages"], DATA_SEED, deterministic=True)
    batch.seek(r["data_step"])
    x = batch.next_batch(B)
    assert torch.equal(r["inputs"], x[:TOTAL // 2]) and r["inputs"].dtype == torch.uint8
    np.testing.assert_array_equal(r["inputs"].cpu().numpy(), tiny["images"][:TOTAL // 2])
    other.seek(r["noise_step"])
    x_mean = m.forward(x, m.draw_noise(B, other, which="posterior"))[0]
    assert tuple(r["x_mean"].shape) == (TOTAL // 2, 3, S, S) and tuple(r["x_gen"].shape) == (B, 3, S, S)
    assert torch.equal(r["x_mean"].view(torch.int32), x_mean[:TOTAL // 2].view(torch.int32))
    x_gen = m.sample(B, other)                                                  # (the source stands at noise_step + 1)
    assert torch.equal(r["x_gen"].view(torch.int32), x_gen.view(torch.int32))

    # the grids: the restatement applied to the returned tensors
    inputs, xm, xg = (r[k].cpu().numpy() for k in ("inputs", "x_mean", "x_gen"))
    want_rec = R.grid([(inputs, TOTAL // 2, None), (xm, TOTAL // 2, None)], TOTAL)
    want_smp = R.grid([(xg, B, TOTAL)], TOTAL)
    for name, want in (("reconstructions", want_rec), ("samples", want_smp)):
        gf = r[name + "_f32"].cpu().numpy()
        g8 = r[name]
        assert isinstance(g8, np.ndarray) and g8.dtype == np.uint8 and g8.shape == gf.shape == (2 * S, 2 * S, 3) == (32, 32, 3)
        err = float(np.max(np.abs(gf.astype(np.float64) - want.astype(np.float64))))
        print("%s: max abs err %.3e (bound %.3e)" % (name, err, TOL))
        assert err <= TOL
        np.testing.assert_array_equal(g8, R.quantise(gf))
        assert gf.min() == 0.0 and gf.max() > 0.99                              # a stretched slice spans [0, 1]
    # the even slots hold the inputs: tile (0, 0) is image 0 of the batch, stretched over the two inputs shown
    np.testing.assert_array_equal(r["reconstructions_f32"].cpu().numpy()[:S, :S], np.transpose(R.stretch(inputs)[0], (1, 2, 0)))


def test_images_leaves_the_evaluation_alone(amd, tiny):
    ev, data, src = _pass(amd, tiny, per_image=True)
    src.seek(0)
    a = ev.run()
    per_image = ev.per_image.clone()
    captures, graphs, rec = dict(ev.captures), ev._graphs, ev._buf["rec"].clone()
    assert data.tell() == N_IMAGES // B                                         # behind the epoch: the next batch is the wrap to batch 0
    r = ev.images(total=TOTAL)
    assert r["data_step"] == N_IMAGES // B and r["noise_step"] == a["noise_step"] + N_IMAGES // B
    np.testing.assert_array_equal(r["inputs"].cpu().numpy(), tiny["images"][:TOTAL // 2])
    assert torch.equal(ev.per_image.view(torch.int32), per_image.view(torch.int32))
    assert torch.equal(ev._buf["rec"], rec)
    assert ev.captures == captures and ev._graphs is graphs
    src.seek(a["noise_step"])
    b = ev.run()
    assert np.float64(b["loss"]).tobytes() == np.float64(a["loss"]).tobytes() and b["nonfinite"] == a["nonfinite"] == 0
    assert torch.equal(ev.per_image.view(torch.int32), per_image.view(torch.int32))
    assert ev.captures == captures


def test_images_argument_errors_come_before_any_launch(amd, tiny):
    ev3, data3, src3 = _pass(amd, tiny, k=3)
    with pytest.raises(ValueError, match="k = 1"):
        ev3.images(total=TOTAL)
    ev, data, src = _pass(amd, tiny)
    for total in (3, 8, 0, 2.0, True):
        with pytest.raises(ValueError, match="several batches"):
            ev.images(total=total)
    for t in (float("inf"), float("nan"), "1", None):
        with pytest.raises(ValueError, match="temperature"):
            ev.images(total=TOTAL, temperature=t)
    assert data.tell() == 0 and src.tell() == 0 and data3.tell() == 0 and src3.tell() == 0       # nothing was drawn


def test_temperature_zero_makes_every_sample_equal(amd, tiny):
    ev, data, src = _pass(amd, tiny)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                          # (no non-finite warning: the stretch of a constant is 0)
        r = ev.images(total=TOTAL, temperature=0)
    xg = r["x_gen"]
    assert torch.equal(xg.view(torch.int32), xg[:1].expand_as(xg).contiguous().view(torch.int32))
    s = r["samples_f32"].cpu().numpy()
    S = tiny["c"]["image_size"]
    for ty in range(2):
        for tx in range(2):
            np.testing.assert_array_equal(s[ty * S:(ty + 1) * S, tx * S:(tx + 1) * S], s[:S, :S])
