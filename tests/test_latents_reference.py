"""CPU-side checks of tests/latents_reference.py, the fp64 restatement the GPU tests of encode / decode / reconstruct are held to: composed
from the oracle's leaves it must reproduce O.cvae1_forward at both ends (all layers from the posterior = mode "train", all from the prior =
mode "sample"), and decode(encode(x).z) must be the forward's x_out, all exactly (the same fp64 operations in the same order).

Two conditions keep the GPU tests from passing on a wrong layer order, checked here on the reference alone: consecutive steps of the
reconstruction ladder differ visibly (more than 1e-2 in at least 30 % of the entries), and a good part of x_out (at least 25 %) lies strictly
inside the clip range, where a difference is not clipped away.  No GPU needed."""
import numpy as np
import pytest

import latents_reference as R
from oracle import iaf_oracle as O

CASES = ["model_tiny", "model_cfg"]
LO, HI = -0.5 + 1 / 512., 0.5 - 1 / 512.


def forward(ref, mode):
    c = ref["c"]
    return O.cvae1_forward(c["x"], ref["p"], c["z_size"], c["h_size"], c["depth"], c["num_blocks"], c["kl_min"], 1,
                           [R.f32(e) for e in c["noise"]], mode=mode)[0]


@pytest.mark.parametrize("name", CASES)
def test_all_posterior_is_the_train_forward(name):
    ref = R.case_reference(name)
    assert float(np.abs(ref["recs"][ref["nl"]][0] - forward(ref, "train")).max()) == 0.0


@pytest.mark.parametrize("name", CASES)
def test_all_prior_is_the_sample_forward(name):
    ref = R.case_reference(name)
    assert float(np.abs(ref["recs"][0][0] - forward(ref, "sample")).max()) == 0.0


@pytest.mark.parametrize("name", CASES)
def test_decode_of_encode_is_the_forward(name):
    ref = R.case_reference(name)
    x_enc, z, costs = ref["recs"][ref["nl"]]
    assert all(k is not None and k.shape == (ref["c"]["B"],) for k in costs)
    x_dec, z2, _ = R.top_down_mixed(ref["p"], ref["c"], list(z), [None] * (2 * ref["nl"]))
    assert float(np.abs(x_dec - x_enc).max()) == 0.0
    assert all(np.array_equal(a, b) for a, b in zip(z, z2))


@pytest.mark.parametrize("name", CASES)
def test_mixed_given_and_prior_layers(name):
    """the first n latents given, the rest from the prior = reconstruct(n): the three sources compose"""
    ref = R.case_reference(name)
    c, nl = ref["c"], ref["nl"]
    n = nl // 2
    want, z, _ = ref["recs"][n]
    got, _, _ = R.top_down_mixed(ref["p"], c, list(z[:n]) + ["prior"] * (nl - n), c["noise"])
    assert float(np.abs(got - want).max()) == 0.0


@pytest.mark.parametrize("name", CASES)
def test_ladder_steps_differ_and_are_not_clipped_away(name):
    ref = R.case_reference(name)
    for n in range(ref["nl"]):
        a, b = ref["recs"][n][0], ref["recs"][n + 1][0]
        frac = float(np.mean(np.abs(a - b) > 1e-2))
        print("%s: %d -> %d posterior layers: %.1f %% of entries differ by > 1e-2, max %.3f" % (name, n, n + 1, 100 * frac, np.abs(a - b).max()))
        assert frac >= 0.30
    for n in range(ref["nl"] + 1):
        xo = ref["recs"][n][0]
        inside = float(np.mean((xo > LO) & (xo < HI)))
        print("%s: %d posterior layers: %.1f %% strictly inside the clip range" % (name, n, 100 * inside))
        assert inside >= 0.25
