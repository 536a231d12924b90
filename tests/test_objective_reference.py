"""CPU checks of tests/objective_reference.py, the fp64 references, fp32 yardsticks and derived bounds that the GPU test of the
objective-side kernels rests on (tests/test_hip_objective_kernels.py): each reference agrees with the reference project's recorded
outputs (tests/golden/distributions.npz), its known-answer tests and the NumPy oracle (oracle/iaf_oracle.py); every yardstick is
finite and stays under a stated cap on the very inputs the GPU test uses; the free-bits gate is decided by the fp64 reference
alone (every channel's margin exceeds the derived bound of its mean); and every check has teeth: a wrong variant of each
operation, evaluated here with no kernel involved, misses the bound that the right one meets."""
import os

import numpy as np
import pytest

import objective_reference as R
from oracle import iaf_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the references are the reference's operations ---------------------------------------------------------------------------
def test_gaussian_and_bound_vs_reference_golden_and_kats():
    g = np.load(os.path.join(GOLDEN, "distributions.npz"))
    mean, logvar, eps, other = (g[k].astype(np.float64) for k in ("mean", "logvar", "eps", "other"))
    np.testing.assert_allclose(O.gaussian_diag_sample(mean, logvar, eps), g["sample"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(O.gaussian_diag_logps(mean, logvar, other), g["logps_fn"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(R.fp32_yardstick_gauss_sample(mean, logvar, eps), g["sample"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(R.fp32_yardstick_gauss_logps(mean, logvar, other), g["logps_fn"], rtol=1e-5, atol=1e-5)
    for k in (1, 4, 12):
        lp, kl = g["lb_log_pxz"].astype(np.float64), g["lb_kl"].astype(np.float64)
        np.testing.assert_allclose(R.lowerbound(lp, kl, k), g["lb_k%d" % k], rtol=1e-5, atol=1e-5)
        if k > 1:
            yard = R.fp32_yardstick_lowerbound(lp.reshape(-1, k), kl.reshape(-1, k), (1, k - 1))
            np.testing.assert_allclose(yard, g["lb_k%d" % k], rtol=1e-5, atol=1e-5)
    # the reference's KATs (tf_utils/distributions_test.py:7-31)
    a = np.log(np.array([0.3, 0.3, 0.3, 0.3])).reshape([1, -1])
    b = np.log(np.array([0.1, 0.5, 0.9, 0.6])).reshape([1, -1])
    res = -(-np.log(4) + np.log(np.sum(np.exp(a - b))))
    assert abs(R.lowerbound(a, b, 4).sum() - res) < 1e-12
    assert abs(R.fp32_yardstick_lowerbound(a, b, (3, 1)).sum() - res) < 1e-6
    assert abs(R.lowerbound(a, b, 1).sum() - (b - a).sum()) < 1e-12
    chunks = [(a - b)[:, :1], (a - b)[:, 1:]]
    assert abs(O.streaming_lowerbound(chunks, 4).sum() - res) < 1e-12


def test_logistic_reference_is_the_oracles():
    for name in sorted(R.DL_CASES):
        c = R.dl_case(name)
        want = O.discretized_logistic(c["mean"][:, None, None, :], c["logscale"], c["sample"][:, None, None, :])
        got = R.dl_logp(c["mean"], c["logscale"], c["sample"]).sum(axis=1)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    c = R.dl_fwd_case("per-element logscale")
    assert c["logscale"].shape == c["mean"].shape and c["logscale"].min() < -4.9 and c["logscale"].max() > -0.1
    m = R.dl_fwd_case("tails_-4 (mirrored)")
    assert all(np.array_equal(m[k], R.dl_mirrored(R.dl_case("tails_-4"))[k]) for k in ("k", "sample", "mean"))
    want = O.discretized_logistic(c["mean"][:, None, None, :], c["logscale"][:, None, None, :], c["sample"][:, None, None, :])
    assert np.abs(R.dl_logp(c["mean"], c["logscale"], c["sample"]).sum(axis=1) - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("kl_min", [0.0, R.FB_KL_MIN])
def test_free_bits_reference_is_the_oracles(kl_min):
    kl = R.fb_case((3, 8, 20), "both")
    r = R.free_bits(kl, kl_min)
    obj, cost = O.theano_free_bits(kl[..., None], kl_min)           # models.py:455-466: the same objective, once per layer
    np.testing.assert_allclose(r["kl_cost"], cost, rtol=1e-13)
    np.testing.assert_allclose(r["kl_obj"], obj * np.ones(3) if kl_min > 0 else obj, rtol=1e-13)


def test_datainit_reference_is_the_oracles():
    """O.conv2d_init with a 1x1 identity filter (unit columns: its l2-normalised form is itself) is the init of x itself"""
    x, _ = R.di_case("3x5x85")
    B, C, HW = x.shape
    y, g, b = O.conv2d_init(x.reshape(B, C, 5, 17), np.eye(C).reshape(1, 1, C, C), init_scale=R.DI_INIT_SCALE)
    r = R.datainit(x)
    np.testing.assert_allclose(r["g"], g, rtol=1e-12)
    np.testing.assert_allclose(r["b"], b, rtol=1e-12)
    np.testing.assert_allclose(r["y"], y.reshape(B, C, HW), rtol=1e-10, atol=1e-13)


# ---- free bits: the gate is the reference's alone; the bound sees a per-image clamp -----------------------------------------------
@pytest.mark.parametrize("mode", R.FB_MODES)
@pytest.mark.parametrize("shape", R.FB_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_free_bits_gate_margin(shape, mode):
    """every channel's batch mean lies at least 1 % of kl_min from kl_min, and further from it than the derived bound of the
    kernel's mean: any evaluation inside the bound produces exactly the fp64 gate"""
    kl = R.fb_case(shape, mode)
    r = R.free_bits(kl, R.FB_KL_MIN)
    bounds = R.free_bits_bounds(kl, R.FB_KL_MIN, R.fb_d_row(shape[2]))
    margin = np.abs(r["mean_c"] - R.FB_KL_MIN)
    print("free bits %s %s: least margin %.3e, largest mean bound %.3e" % (shape, mode, margin.min(), bounds["mean_c"].max()))
    assert (margin >= 0.01 * R.FB_KL_MIN).all()
    assert (bounds["mean_c"] < margin).all()
    if shape[0] * shape[2] > 1:
        assert (kl > 0).any() and (kl < 0).any()
    if mode == "below":
        assert not r["gate"].any() and abs(r["kl_obj"][0] - shape[1] * R.FB_KL_MIN) <= 1e-12
    elif mode == "above":
        assert r["gate"].all()
    elif shape[1] > 1:
        assert r["gate"].any() and not r["gate"].all()


def test_free_bits_bound_sees_a_per_image_clamp():
    for shape in R.FB_SHAPES:
        if shape[0] == 1:
            continue                                                # one image: its own mean
        kl = R.fb_case(shape, "both")
        r, bounds = R.free_bits(kl, R.FB_KL_MIN), R.free_bits_bounds(kl, R.FB_KL_MIN, R.fb_d_row(shape[2]))
        wrong = R.free_bits_per_image_clamp(kl, R.FB_KL_MIN)
        assert np.abs(wrong - r["kl_obj"]).min() > 10 * bounds["kl_obj"], shape          # every image


# ---- the k-sample bound ---------------------------------------------------------------------------------------------------------
LB_CAP_ULP = 2.0


def _lb_orders(k):
    return [(k,)] + ([R.LB_CHUNKS, R.LB_CHUNKS[::-1]] if k == R.LB_K else [])


@pytest.mark.parametrize("kind", R.LB_KINDS)
def test_lowerbound_yardstick_within_its_cap(kind):
    """cap: 2 ulp of max|ref|.  The weights lp - kl near -7.9e3 are each rounded to half an ulp before anything is summed, which moves
    the result by up to half an ulp, the final sum -log k + max + log(sum) rounds twice more, and exp / log contribute 1e-7 of an
    O(10) term: 1.5 ulp and a little.  Worst seen: 1.32 ulp."""
    worst = 0.0
    for n in R.LB_NS:
        for k in R.LB_KS:
            lp, kl = R.lb_case(kind, n, k)
            ref = R.lowerbound(lp, kl, k)
            assert np.isfinite(ref).all()
            for chunks in _lb_orders(k):
                yard = R.fp32_yardstick_lowerbound(lp, kl, chunks)
                assert np.isfinite(yard).all()
                worst = max(worst, float(np.abs(yard - ref).max() / R.ulp32(np.abs(ref).max())))
                if kind == "equal":
                    assert np.abs(yard + (-7900.0)).max() <= R.ulp32(7900.0)
    print("lowerbound yardstick %s: worst %.2f ulp of max|ref|" % (kind, worst))
    assert worst <= LB_CAP_ULP


def test_lowerbound_cases_are_what_they_claim():
    lp, kl = R.lb_case("spread300", 5, R.LB_K)
    w = lp - kl
    assert (w.max(axis=1) - w.min(axis=1) > 290).all()
    assert (np.exp((w - w.max(axis=1, keepdims=True)).astype(np.float32)) == 0).mean() > 0.5     # most terms underflow in fp32
    lp, kl = R.lb_case("latemax", 8, R.LB_K)
    assert [int(np.argmax((lp - kl)[i])) for i in range(8)] == list(R.LB_MAX_POS) * 2
    edges = np.cumsum((0,) + R.LB_CHUNKS)
    assert [int(np.searchsorted(edges, p, side="right") - 1) for p in R.LB_MAX_POS] == [0, 2, 3, 3]
    edges = np.cumsum((0,) + R.LB_CHUNKS[::-1])
    assert [int(np.searchsorted(edges, p, side="right") - 1) for p in R.LB_MAX_POS] == [0, 0, 1, 3]


def test_lowerbound_bound_sees_a_sum_that_is_never_rescaled():
    lp, kl = R.lb_case("latemax", 5, R.LB_K)
    ref = R.lowerbound(lp, kl, R.LB_K)
    for chunks in (R.LB_CHUNKS, R.LB_CHUNKS[::-1]):
        right, wrong = R.fp32_yardstick_lowerbound(lp, kl, chunks), R.fp32_yardstick_lowerbound(lp, kl, chunks, rescale=False)
        bound = R.lb_bound(right, ref)
        assert np.abs(right - ref).max() <= bound
        assert np.abs(wrong - ref).max() > 100 * bound


# ---- discretized logistic, forward ------------------------------------------------------------------------------------------
DL_CAP_ELEM, DL_CAP_UPPER, DL_CAP_ROWS, DL_CAP_ROWS_WIDE = 2e-4, 1e-5, 2e-7, 7e-7


def _dl_all_cases():
    return [(name, R.dl_fwd_case(name)) for name in R.DL_FWD_CASES]


def test_logistic_yardstick_within_its_caps():
    """caps: 2e-4 per element over all cases (the centre at logscale 0: a difference of 1e-3 between two values near 0.5), 1e-5 per
    element in the upper tail (s > 8) of the cases with logscale <= -3, 2e-7 relative on the row sums of the cases with logscale <= -2
    (worst seen 1.4e-7).  Wider scales: the per-element errors of the centre (up to 9e-5 each at logscale 0, independent of one
    another) add up to 3.3e-7 of a 192-element row, whatever the order of the sum: 7e-7 there, twice the worst seen.  A row of
    one element is an element."""
    for name, c in _dl_all_cases():
        ref = R.dl_logp(c["mean"], c["logscale"], c["sample"])
        yard, yard_rows = R.fp32_yardstick_dl(c["mean"], c["logscale"], c["sample"])
        assert np.isfinite(yard).all() and np.isfinite(yard_rows).all()
        masks = R.dl_masks(c)
        e = R.dl_fwd_errors(yard, yard_rows, ref, ref.sum(axis=-1), masks)
        print("logistic yardstick %s: " % name + ", ".join("%s %.2e" % kv for kv in sorted(e.items())))
        assert e["all"] <= DL_CAP_ELEM
        if c["n_per_row"] > 1:
            assert e["rows"] <= (DL_CAP_ROWS if np.max(c["logscale"]) <= -2 else DL_CAP_ROWS_WIDE)
        if np.max(c["logscale"]) <= -3:
            assert e["upper"] <= DL_CAP_UPPER


def test_logistic_bound_sees_the_literal_form():
    """the literal fp32 form sig(t) - sig(s) misses, per element in the upper tail and on the row sums, the bound that the mirrored
    yardstick defines (and meets with a factor of 4 to spare), on every case with logscale <= -3"""
    seen = 0
    for name, c in _dl_all_cases():
        if np.max(c["logscale"]) > -3 or c["n_per_row"] < 192 or not name.startswith(("tails", "size")):
            continue
        ref = R.dl_logp(c["mean"], c["logscale"], c["sample"])
        rows = ref.sum(axis=-1)
        masks = R.dl_masks(c)
        assert masks["upper"].sum() >= 10
        yard = R.dl_fwd_errors(*R.fp32_yardstick_dl(c["mean"], c["logscale"], c["sample"]), ref, rows, masks)
        lit = R.dl_fwd_errors(*R.fp32_yardstick_dl(c["mean"], c["logscale"], c["sample"], literal=True), ref, rows, masks)
        print("logistic literal form %s: upper %.2e (bound %.2e), rows %.2e (bound %.2e)"
              % (name, lit["upper"], R.dl_fwd_bound(yard, "upper", rows), lit["rows"], R.dl_fwd_bound(yard, "rows", rows)))
        assert lit["upper"] > 100 * R.dl_fwd_bound(yard, "upper", rows)
        assert lit["all"] > 100 * R.dl_fwd_bound(yard, "all", rows)
        assert lit["rows"] > R.dl_fwd_bound(yard, "rows", rows)
        seen += 1
    assert seen >= 10


# ---- Gaussian sample / log-density ------------------------------------------------------------------------------------------
GAUSS_CAP = 4.5e-7
GAUSS_CAP_ELEM = 5.5e-7


@pytest.mark.parametrize("n", R.GAUSS_NS)
def test_gaussian_yardsticks_within_their_cap(n):
    """cap: 4.5e-7 of max|ref|, twice the worst seen (1.2e-7 on the sample, 2.2e-7 on the log-density: a few roundings of the largest
    element), and inside the 2e-6 the outputs are allowed; element by element against the magnitude of the element's own terms
    (objective_reference.gauss_scales) 5.5e-7, twice the worst seen (1.6e-7 and 2.7e-7)"""
    c = R.gauss_case(n)
    assert np.abs(c["logvar"]).max() <= 20 and np.abs(c["noise"]).max() <= 30
    if n > 100:
        assert np.abs(c["noise"]).max() == 30 and np.abs(c["logvar"]).max() > 19
    sc_sample, sc_logps = R.gauss_scales(c)
    ref_s = O.gaussian_diag_sample(c["mean"], c["logvar"], c["noise"])
    yard_s = R.fp32_yardstick_gauss_sample(c["mean"], c["logvar"], c["noise"])
    ref = O.gaussian_diag_logps(c["mean"], c["logvar"], c["sample"])
    yard = R.fp32_yardstick_gauss_logps(c["mean"], c["logvar"], c["sample"])
    assert np.isfinite(yard).all() and np.isfinite(yard_s).all()
    e_s, e_l = R.rel_err(yard_s, ref_s), R.rel_err(yard, ref)
    p_s, p_l = R.scaled_err(yard_s, ref_s, sc_sample), R.scaled_err(yard, ref, sc_logps)
    print("gaussian yardsticks n=%d: sample %.2e, logps %.2e of max|ref|; per element %.2e, %.2e of the element's own terms" % (n, e_s, e_l, p_s, p_l))
    assert e_s <= GAUSS_CAP and e_l <= GAUSS_CAP
    assert p_s <= GAUSS_CAP_ELEM and p_l <= GAUSS_CAP_ELEM
    assert (sc_sample > 0).all() and (np.abs(ref_s) <= sc_sample * (1 + 1e-12)).all() and (np.abs(ref) <= sc_logps * (1 + 1e-12)).all()


# ---- data-dependent init ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("name", sorted(R.DI_CASES))
def test_datainit_two_pass_fp32_meets_the_derived_bounds(name, with_add):
    x, add = R.di_case(name)
    add = add if with_add else None
    ref, got, bound = R.datainit(x, add), R.fp32_datainit(x, add), R.datainit_bounds(x, add)
    for k in ("mean", "var", "g", "b", "y"):
        assert np.isfinite(got[k]).all()
        ratio = float((np.abs(got[k] - ref[k]) / bound[k]).max())
        print("datainit two-pass fp32 %s %s: error / bound %.3f" % (name, k, ratio))
        assert ratio <= 1.0, (k, ratio)


def test_datainit_bounds_see_a_one_pass_variance():
    x, _ = R.di_case("large_mean")
    ref, wrong, bound = R.datainit(x), R.fp32_datainit(x, one_pass=True), R.datainit_bounds(x)
    np.testing.assert_allclose(ref["mean"], 100.0, atol=1e-2)
    np.testing.assert_allclose(np.sqrt(ref["var"]), 0.01, rtol=0.1)
    with np.errstate(invalid="ignore"):
        assert not (np.abs(wrong["var"] - ref["var"]) <= bound["var"]).any()
        assert not (np.abs(wrong["g"] - ref["g"]) <= bound["g"]).any()
        # ... and the rule the kernel is held to, 4 x the two-pass yardstick's error + 1e-6, which the yardstick meets by definition
        right = R.fp32_datainit(x)
        for k in ("g", "b", "y"):
            assert not np.abs(wrong[k] - ref[k]).max() <= 100 * (4 * np.abs(right[k] - ref[k]).max() + 1e-6), k


# ---- the exponential bound's inputs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.EW_NS)
def test_exponential_cases_keep_their_promises(n):
    z, m, s = R.affine_case(n)
    ref, x = R.affine_transform(z, m, s)
    assert np.abs(x).max() <= R.EXP_X_MAX and (np.abs(z) >= 2 * np.abs(R.AFFINE_SCALE * m)).all()
    assert (np.abs(ref) > 1e-30).all() and (np.abs(ref) < 1e30).all()
    z, qm, ql, rm, rl = R.noise_case(n)
    ref, x = R.noise_from_sample(z, qm, ql, rm, rl)
    assert np.abs(x).max() <= R.EXP_X_MAX and (qm * rm >= 0).all() and (np.abs(z) >= 2 * np.abs(qm + rm)).all()
    assert (np.abs(ref) > 1e-30).all() and (np.abs(ref) < 1e30).all()
    if n > 1:
        assert (z > 0).any() and (z < 0).any()
