"""The reference's N-tower training step (tf_train.py:124-147: tf.split(0, num_gpus, x), one _forward per tower on shared variables,
gradients summed and divided by N) stated for ONE batch of N * B rows: everything in _forward is per row except the free-bits mean
(tf_train.py:79-82), which each tower takes over its own rows.  Here: the fp64 free-bits statement per contiguous row group with its
derived bounds (objective_reference's, with B := the group's G rows), the seed-fixed leaf cases whose gates differ between the
groups, and the inputs of the towers of the model-level fixture tests/golden/cvae1_towers.npz (tests/golden/make_golden_towers.py
runs the reference's own _forward on them).  Shared by the CPU tests (tests/test_towers_reference.py) and the GPU tests
(tests/test_hip_towers.py); does not import the GPU library."""
import numpy as np

import golden_inputs as gi
import objective_reference as R
from oracle import iaf_oracle as O

f32 = R.f32
KL_MIN = R.FB_KL_MIN


# --------------------------------------------------------------------------------------
# free bits per row group on kl [B, C, HW]
# --------------------------------------------------------------------------------------
def free_bits_grouped(kl, kl_min, groups):
    """objective_reference.free_bits per contiguous group of G = B / groups rows
    -> dict(kl_cost [B], kl_obj [B], gate [groups, C], mean_c [groups, C]) in fp64"""
    kl = np.asarray(kl, np.float64)
    B = kl.shape[0]
    assert groups >= 1 and B % groups == 0
    G = B // groups
    per = [R.free_bits(kl[r * G:(r + 1) * G], kl_min) for r in range(groups)]
    return dict(kl_cost=np.concatenate([p["kl_cost"] for p in per]), kl_obj=np.concatenate([p["kl_obj"] for p in per]),
                gate=np.stack([p["gate"] for p in per]), mean_c=np.stack([p["mean_c"] for p in per]))


def free_bits_grouped_bounds(kl, kl_min, d_row, groups):
    """objective_reference.free_bits_bounds per group, i.e. with B := G: a group's numbers are a stand-alone G-row batch's
    -> dict(kl_cost [B], mean_c [groups, C], kl_obj [B])"""
    kl = np.asarray(kl, np.float64)
    B = kl.shape[0]
    G = B // groups
    per = [R.free_bits_bounds(kl[r * G:(r + 1) * G], kl_min, d_row) for r in range(groups)]
    return dict(kl_cost=np.concatenate([p["kl_cost"] for p in per]), mean_c=np.stack([p["mean_c"] for p in per]),
                kl_obj=np.concatenate([np.broadcast_to(p["kl_obj"], (G,)) for p in per]))


def free_bits_batch_mean(kl, kl_min, groups):
    """WRONG on purpose (the CPU test shows the bounds see it): one free-bits mean over all B rows, whatever `groups` says"""
    return R.free_bits(kl, kl_min)["kl_obj"]


# (B, C, HW, groups): G = 1; small odd sizes; more rows than the finish kernel has threads; exactly the 8192 floats its LDS stages;
# beyond them (the global route)
FBG_SHAPES = [(2, 1, 1, 2), (6, 8, 20, 3), (4, 7, 65, 2), (300, 3, 5, 4), (128, 64, 4, 8), (264, 32, 4, 8)]


def fbg_case(shape):
    """kl [B, C, HW], fp32-rounded: N(0, 1) elements shifted per (group, channel) so that the group's mean of the channel's sums sits on
    a target at least 20 % away from KL_MIN, alternately above and below it along the channels, the phase moved on by one per group:
    every channel's gate differs between neighbouring groups"""
    B, C, HW, groups = shape
    G = B // groups
    rng = np.random.RandomState(4000 + FBG_SHAPES.index(shape))
    x = rng.standard_normal((B, C, HW))
    for r in range(groups):
        lo, hi = rng.uniform(0.02, 0.2, C), rng.uniform(0.3, 1.5, C)
        target = np.where((np.arange(C) + r) % 2 == 0, hi, lo)
        g = x[r * G:(r + 1) * G]
        g += ((target - g.sum(axis=2).mean(axis=0)) / HW)[None, :, None]
    return f32(x)


# --------------------------------------------------------------------------------------
# the towers of the model-level fixture
# --------------------------------------------------------------------------------------
TOWERS_CASE = "model_cfg"          # an entry of golden_inputs.MODEL_CASES: the BASELINE channel counts, B = 2 rows per tower
N_TOWERS = 2
# tower 1 draws its posterior noise narrower: its per-channel KL sums move, many of them across kl_min.  Seed and scale were picked, on the
# CPU oracle, so that no (tower, layer, channel) mean lies within 20 % of kl_min (tests/test_towers_reference.py asserts it): the fp32
# gates then equal the fp64 ones
TOWER1_NOISE_SCALE = 0.5


def tower_inputs(t):
    """(x uint8 [B,3,S,S], noise list) of tower t: tower 0 is the case's own batch; tower 1's images and noise come from a generator
    seeded with the case's seed + 3, its posterior noise scaled by TOWER1_NOISE_SCALE"""
    c = gi.model_case_inputs(TOWERS_CASE)
    if t == 0:
        return c["x"], c["noise"]
    assert t == 1
    rng = np.random.RandomState(gi.case_seed(TOWERS_CASE) + 3)
    x = rng.randint(0, 256, size=c["x"].shape).astype(np.uint8)
    noise = []
    for i, e in enumerate(c["noise"]):
        d = rng.standard_normal(e.shape)
        noise.append(d * TOWER1_NOISE_SCALE if i % 2 else d)             # (odd entries: the posterior's draws)
    return x, noise


def towers_batch():
    """the towers' rows as ONE batch, tower-major: rows t B .. (t + 1) B are tower t (tf.split(0, num_gpus, x), tf_train.py:126)"""
    parts = [tower_inputs(t) for t in range(N_TOWERS)]
    x = np.concatenate([p[0] for p in parts], axis=0)
    noise = [np.concatenate([p[1][i] for p in parts], axis=0) for i in range(len(parts[0][1]))]
    return x, noise


def oracle_forward(x, noise, params=None, want_means=False):
    """oracle.cvae1_forward on the case's variables -> (x_out, obj, loss[, per layer in top-down order the batch means [C] of the
    channels' KL sums, tf_train.py:79])"""
    c = gi.model_case_inputs(TOWERS_CASE)
    params = c["params"] if params is None else params
    means = []
    inner = O.posterior_block

    def recording(*a, **kw):
        blk = inner(*a, **kw)
        means.append(np.sum(blk["logqs"] - blk["logps"], axis=(2, 3)).mean(axis=0))
        return blk
    O.posterior_block = recording
    try:
        out = O.cvae1_forward(x, params, c["z_size"], c["h_size"], c["depth"], c["num_blocks"], c["kl_min"], 1, noise)
    finally:
        O.posterior_block = inner
    return out + (means,) if want_means else out
