"""CPU pins of the towers statement (tests/towers_reference.py): the fixture tests/golden/cvae1_towers.npz -- the reference's own
_forward per tower on the TF shim -- against the oracle run per tower; that the fixture's inputs separate the N-tower objective
from the one-batch objective on the same rows by far more than the GPU test's tolerance; and the grouped free-bits statement with
its bounds, which a per-batch mean misses."""
import os

import numpy as np
import pytest

import golden_inputs as gi
import objective_reference as R
import towers_reference as T

GPU_RTOL = 2e-5           # what tests/test_hip_towers.py (as tests/test_hip_model.py) allows obj and loss


@pytest.fixture(scope="module")
def towers():
    """the oracle per tower and on the concatenated rows, computed once: [(x_out, obj, loss, means)] per tower, (obj, loss) ungrouped"""
    per = [T.oracle_forward(*T.tower_inputs(t), want_means=True) for t in range(T.N_TOWERS)]
    x, noise = T.towers_batch()
    _, obj, loss = T.oracle_forward(x, noise)
    return per, (obj, loss)


def test_fixture_equals_the_oracle_per_tower(golden_dir, towers):
    g = np.load(os.path.join(golden_dir, "cvae1_towers.npz"))
    c = gi.model_case_inputs(T.TOWERS_CASE)
    per, _ = towers
    for t, (xo, obj, loss, _) in enumerate(per):
        np.testing.assert_allclose(xo, g["tower%d/x_out" % t], rtol=0, atol=1e-12)
        np.testing.assert_allclose(obj, g["tower%d/obj" % t], rtol=1e-12)
        np.testing.assert_allclose(loss, g["tower%d/loss" % t], rtol=1e-12)
    bpd = sum(p[2] for p in per) / (np.log(2.) * 3 * c["image_size"] ** 2 * c["B"] * T.N_TOWERS)       # tf_train.py:142
    np.testing.assert_allclose(bpd, g["bits_per_dim"], rtol=1e-12)
    # tower 0 is the one-tower fixture's batch
    g1 = np.load(os.path.join(golden_dir, "cvae1_forward.npz"))
    np.testing.assert_allclose(g["tower0/obj"], g1[T.TOWERS_CASE + "/obj"], rtol=1e-12)


def test_fixture_inputs_separate_towers_from_one_batch(towers):
    per, (obj_all, loss_all) = towers
    want = sum(p[1] for p in per)
    miss = abs(obj_all - want) / abs(want)
    print("one free-bits mean over all rows misses the towers' objective by %.2e relative (GPU tolerance %.0e)" % (miss, GPU_RTOL))
    assert miss > 100 * GPU_RTOL
    # the loss has no free bits in it (tf_train.py:85, 218): per row, so the same either way
    np.testing.assert_allclose(loss_all, sum(p[2] for p in per), rtol=1e-12)
    means = np.stack([np.stack(p[3]) for p in per])                       # [tower, layer, channel]
    kl_min = gi.model_case_inputs(T.TOWERS_CASE)["kl_min"]
    gates = means > kl_min
    differ = (gates[0] != gates[1]).sum(axis=1)
    print("channels whose gate differs between the towers, per layer:", differ.tolist())
    assert differ.max() >= 1
    margin = np.abs(means / kl_min - 1.0).min()
    print("closest (tower, layer, channel) mean to kl_min: %.0f %% away" % (100 * margin))
    assert margin > 0.2


@pytest.mark.parametrize("shape", T.FBG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grouped_free_bits_statement_and_bounds(shape):
    B, C, HW, groups = shape
    kl = T.fbg_case(shape)
    d_row = R.fb_d_row(HW)
    # one group is the one-batch statement
    one, ref1 = T.free_bits_grouped(kl, T.KL_MIN, 1), R.free_bits(kl, T.KL_MIN)
    for k in ("kl_cost", "kl_obj"):
        assert np.array_equal(one[k], ref1[k])
    assert np.array_equal(one["gate"][0], ref1["gate"]) and np.array_equal(one["mean_c"][0], ref1["mean_c"])
    b1, br1 = T.free_bits_grouped_bounds(kl, T.KL_MIN, d_row, 1), R.free_bits_bounds(kl, T.KL_MIN, d_row)
    assert np.array_equal(b1["kl_cost"], br1["kl_cost"]) and np.allclose(b1["kl_obj"], br1["kl_obj"], rtol=0, atol=0)
    # the groups: every mean at least 20 % from kl_min and further than its own bound (the fp32 gate is the fp64 gate); the gates
    # of neighbouring groups differ in every channel
    ref, bound = T.free_bits_grouped(kl, T.KL_MIN, groups), T.free_bits_grouped_bounds(kl, T.KL_MIN, d_row, groups)
    assert ref["gate"].shape == (groups, C) and ref["kl_obj"].shape == (B,) and bound["kl_obj"].shape == (B,)
    dist = np.abs(ref["mean_c"] - T.KL_MIN)
    assert (dist >= 0.19 * T.KL_MIN).all() and (dist > 4 * bound["mean_c"]).all()
    assert (ref["gate"][1:] != ref["gate"][:-1]).all()
    G = B // groups
    for r in range(groups):
        assert (ref["kl_obj"][r * G:(r + 1) * G] == ref["kl_obj"][r * G]).all()
    # kl_cost is per row: the same with and without groups; kl_min = 0: kl_obj too
    assert np.array_equal(ref["kl_cost"], ref1["kl_cost"])
    assert np.array_equal(T.free_bits_grouped(kl, 0.0, groups)["kl_obj"], ref1["kl_cost"])
    # a per-batch mean misses the bounds
    wrong = T.free_bits_batch_mean(kl, T.KL_MIN, groups)
    r = np.abs(wrong - ref["kl_obj"]) / bound["kl_obj"]
    print("per-batch mean instead of per-group: error / bound up to %.1e" % r.max())
    assert r.max() > 100
