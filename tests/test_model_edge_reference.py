"""CPU checks of tests/model_edge_reference.py, the torch-fp64 references the GPU test of the model-edge backward kernels rests on
(tests/test_hip_model_edge_backward.py): each agrees with the NumPy oracle's own forward functions (oracle/iaf_oracle.py), directly
where the operation is linear and through central finite differences where it is not, and the fp32 yardstick of the likelihood's
gradient stays within the caps the kernel's tolerance is derived from, on the very inputs the GPU test uses."""
import numpy as np
import pytest

import model_edge_reference as R
from oracle import iaf_oracle as O


@pytest.mark.parametrize("shape", [(2, 3, 20, 9, 7, 5, 2), (2, 3, 17, 11, 8, 4, 2)])
def test_convk_wgrad_is_the_filter_gradient_of_the_oracles_conv(shape):
    """the conv is linear in its filter: d <conv(x; w), dy> / d w[a, c, ci, o] = <conv(x; one-hot (a, c, ci)), dy[:, o]>, exactly.
    O.conv2d with a one-hot V of one output channel, g = 0, b = 0 is the conv with that one-hot filter (its norm is 1)."""
    B, ns, nb, H, W, k, s = shape
    rng = np.random.RandomState(11)
    x = rng.standard_normal((B, ns, H, W))
    dy = rng.standard_normal((B, nb, -(-H // s), -(-W // s)))
    for elu_x, elu_dy in ((0, 0), (0, 1), (1, 1)):
        got = R.convk_wgrad(x, dy, k, k, s, elu_x, elu_dy)
        assert got.shape == (k, k, ns, nb)
        xe, de = (O.elu(x) if elu_x else x), (O.elu(dy) if elu_dy else dy)
        want = np.zeros_like(got)
        for a in range(k):
            for c in range(k):
                for ci in range(ns):
                    V = np.zeros((k, k, ns, 1))
                    V[a, c, ci, 0] = 1.0
                    y1 = O.conv2d(xe, V, np.zeros(1), np.zeros(1), stride=(s, s))
                    want[a, c, ci] = np.einsum("nhw,nohw->o", y1[:, 0], de)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("shape", [(2, 8, 2, 3, 5, 4), (2, 24, 3, 5, 7, 5)])
def test_deconvk_is_the_oracles_deconv2d(shape):
    B, ci, co, H, W, k = shape
    rng = np.random.RandomState(12)
    V, g = 0.05 * rng.standard_normal((k, k, co, ci)), 0.3 * rng.standard_normal(co)
    x = rng.standard_normal((B, ci, H, W))
    w = np.exp(g).reshape(1, 1, co, 1) * O.l2_normalize(V, (0, 1, 2))
    want = O.deconv2d(x, V, g, np.zeros(co), stride=(2, 2))
    got = R.deconvk(x, w, 2)
    assert got.shape == want.shape == (B, co, 2 * H, 2 * W)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("deconv", [0, 1])
def test_weightnorm_backward_vs_central_differences_of_the_oracles_weights(deconv):
    k, n_in, n_out = 3, 4, 3
    rng = np.random.RandomState(13)
    V = 0.05 * rng.standard_normal((k, k, n_out, n_in) if deconv else (k, k, n_in, n_out))
    g, dW = 0.3 * rng.standard_normal(n_out), rng.standard_normal(V.shape)

    def obj(V, g):
        w = np.exp(g).reshape(1, 1, n_out, 1) * O.l2_normalize(V, (0, 1, 2)) if deconv else O.weightnorm_weights(V, g)
        return np.sum(w * dW)

    dV, dg = R.weightnorm_backward(V, g, dW, deconv)
    h = 1e-6
    fdV, fdg = np.zeros_like(V), np.zeros_like(g)
    for i in np.ndindex(V.shape):
        e = np.zeros_like(V)
        e[i] = h
        fdV[i] = (obj(V + e, g) - obj(V - e, g)) / (2 * h)
    for i in range(n_out):
        e = np.zeros_like(g)
        e[i] = h
        fdg[i] = (obj(V, g + e) - obj(V, g - e)) / (2 * h)
    # central differences: truncation h^2 f''' / 6 and round-off eps |f| / h, both below 1e-6 of the largest entry here
    assert np.abs(dV - fdV).max() <= 1e-6 * np.abs(fdV).max()
    assert np.abs(dg - fdg).max() <= 1e-6 * np.abs(fdg).max()


@pytest.mark.parametrize("logscale,clip", [(-1.3, False), (-3.0, False), (-2.0, True)])
def test_dl_backward_vs_central_differences_of_the_oracles_likelihood(logscale, clip):
    rng = np.random.RandomState(14)
    B, shape = 2, (2, 1, 3, 4)
    k = rng.randint(0, 256, size=shape)
    sample = (k + 0.5) / 256.0 - 0.5
    pre = sample + 0.2 * rng.standard_normal(shape)
    lo, hi = R.DL_CLIP if clip else (0.0, 0.0)
    h = 1e-6
    if clip:
        pre.reshape(-1)[:3] = (0.7, -0.6, 0.55)                       # some beyond a bound, whatever the draw
        assert (np.abs(np.abs(pre) - hi) > 10 * h).all()
    fwd = lambda m, ls: R.DL_UP * O.discretized_logistic(np.clip(m, lo, hi) if clip else m, ls, sample)
    d_mean, d_rows = R.dl_backward(pre, logscale, sample, lo, hi, R.DL_UP)
    fd = np.zeros(shape)
    for i in np.ndindex(shape):
        e = np.zeros(shape)
        e[i] = h
        fd[i] = (fwd(pre + e, logscale) - fwd(pre - e, logscale))[i[0]] / (2 * h)
    fd_rows = (fwd(pre, logscale + h) - fwd(pre, logscale - h)) / (2 * h)
    if clip:
        outside = (pre < lo) | (pre > hi)
        assert outside.sum() >= 3 and (d_mean[outside] == 0).all() and (d_mean[~outside] != 0).all()
    assert np.abs(d_mean - fd).max() <= 1e-6 * np.abs(fd).max()
    assert np.abs(d_rows - fd_rows).max() <= 1e-6 * np.abs(fd_rows).max()
    assert d_rows.shape == (B,)


def _case_refs(case):
    args = (case["pre_clip_mean"], case["logscale"], case["sample"], case["lo"], case["hi"], R.DL_UP)
    return R.dl_backward(*args), R.fp32_yardstick_dl_backward(*args)


@pytest.mark.parametrize("name", sorted(R.DL_CASES))
def test_fp32_yardstick_meets_its_caps_on_the_gpu_tests_inputs(name):
    """a plain fp32 evaluation in the mirrored form is within 5e-4 of fp64 autograd at logscale = 0 (the cancellation inherent to a
    1/256-wide bin in fp32) and within 5e-5 in every other case and subset, both tails included: the reference alone meets the
    conditions the kernel's bound (4 x this error + 1e-6) is derived from"""
    for case in (R.dl_case(name), R.dl_mirrored(R.dl_case(name))):
        ref, yard = _case_refs(case)
        masks = R.dl_subsets(case)
        err = R.dl_errors(yard[0], yard[1], ref[0], ref[1], masks)
        print(name, {k: "%.1e" % v for k, v in err.items()}, {k: int(m.sum()) for k, m in masks.items()})
        cap = 5e-4 if case["logscale"] == 0.0 else 5e-5
        for key, v in err.items():
            assert v <= cap, (name, key, v)
        assert np.isfinite(yard[0]).all() and np.isfinite(yard[1]).all()
        assert (np.abs(yard[0]) * np.exp(case["logscale"]) <= 1 + 1e-5).all()


@pytest.mark.parametrize("name", ["tails_-4", "tails_-5"])
def test_tail_cases_reach_both_tails(name):
    case = R.dl_case(name)
    masks = R.dl_subsets(case)
    assert all(masks[k].sum() >= 10 for k in ("lower", "centre", "upper")), {k: int(m.sum()) for k, m in masks.items()}
    assert np.abs(R.dl_s(case["mean"], case["logscale"], case["sample"])).max() >= 35


def test_clip_case_clips_some_on_each_side_and_none_on_a_bound():
    case = R.dl_case("clip_-2")
    pre, lo, hi = case["pre_clip_mean"], case["lo"], case["hi"]
    assert lo == np.float32(lo) and hi == np.float32(hi)
    assert not ((pre == lo) | (pre == hi)).any()
    assert (pre < lo).sum() >= 1 and (pre > hi).sum() >= 1
    assert 0.05 <= np.mean((pre < lo) | (pre > hi)) <= 0.30
    d_mean, _ = R.dl_backward(pre, case["logscale"], case["sample"], lo, hi, R.DL_UP)
    assert np.array_equal(d_mean == 0, (pre < lo) | (pre > hi))


@pytest.mark.parametrize("name", sorted(R.DL_CASES))
def test_mirror_identity_of_the_fp64_reference(name):
    """(255 - k, -mean) maps s -> -t and t -> -s, and the logistic is symmetric: d_mean is negated element by element, d_logscale is
    unchanged.  In fp64 the two sides differ by the rounding of sig(t) - sig(s), at most 2 * 2^-53 absolute against P >= 1e-7: a few
    1e-9 of the largest entry, where the floor dominates P; bound 1e-8."""
    case = R.dl_case(name)
    (a_mean, a_rows), _ = _case_refs(case)
    (b_mean, b_rows), _ = _case_refs(R.dl_mirrored(case))
    assert np.abs(a_mean + b_mean).max() <= 1e-8 * np.abs(a_mean).max()
    assert np.abs(a_rows - b_rows).max() <= 1e-8 * np.abs(a_rows).max()
