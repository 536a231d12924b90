"""GPU leaf tests of the backward kernels of the model's two ends (iaf_amd/csrc/iaf_kernels_edge.hpp) and of the adjoint modes of
iaf_resample2, one by one through the raw C ABI against the torch-fp64 references of tests/model_edge_reference.py (pinned on the
CPU by tests/test_model_edge_reference.py): iaf_discretized_logistic_backward (centre, both tails, mirror identity, clip gate),
iaf_convk_wgrad (every tap on its own), iaf_convk_weightnorm_backward (conv and deconv form, clamped channel), iaf_channel_sum,
iaf_mul_elu_grad, iaf_convk_forward as the adjoint of iaf_deconvk_forward, and the six modes of iaf_resample2.  References see the
fp32-rounded inputs, as the device does.  Error measure: max|got - ref| / max|ref| per output tensor unless stated otherwise.

The likelihood's gradient has no fixed tolerance: the kernel's error, per case and subset, is at most 4 x the error of a plain fp32
restatement in the same (mirrored) formulation on the same inputs (model_edge_reference.fp32_yardstick_dl_backward: correctly
rounded exp; the kernel may spend a few ulp on its exponential and sums its row in another order) plus a floor of 1e-6, both errors
against fp64 autograd.  The factor does not cover another formulation: the literal fp32 form sig(t) - sig(s), sig (1 - sig) misses
it by five orders of magnitude in the upper tail."""
import numpy as np
import pytest
import torch

import model_edge_reference as R

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


def rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---- a. iaf_discretized_logistic_backward ------------------------------------------------------------------------------------
_dl_cache = {}


def dl_run(amd, name, mirrored=False):
    """one case through the kernel, the fp64 reference and the fp32 yardstick (each computed once per module)"""
    key = (name, mirrored)
    if key not in _dl_cache:
        lib, P, st = amd._capi.lib(), amd.layers._ptr, amd.layers._stream
        case = R.dl_mirrored(R.dl_case(name)) if mirrored else R.dl_case(name)
        n = case["n_per_row"]
        mean, sample, ls = dev(case["mean"]), dev(case["sample"]), dev(np.array([case["logscale"]]))
        d_mean, rows = torch.full((R.DL_B, n), np.nan, device="cuda"), torch.full((R.DL_B,), np.nan, device="cuda")
        amd._capi.check(lib.iaf_discretized_logistic_backward(P(mean), P(ls), P(sample), R.DL_UP, case["lo"], case["hi"], P(d_mean), P(rows),
                                                              R.DL_B, n, R.BINSIZE, st()))
        got = (host(d_mean), host(rows))
        args = (case["pre_clip_mean"], case["logscale"], case["sample"], case["lo"], case["hi"], R.DL_UP)
        ref, yard = R.dl_backward(*args), R.fp32_yardstick_dl_backward(*args)
        masks = R.dl_subsets(case)
        kern_err, yard_err = R.dl_errors(got[0], got[1], ref[0], ref[1], masks), R.dl_errors(yard[0], yard[1], ref[0], ref[1], masks)
        print("%s%s kernel / yardstick error: " % (name, " (mirrored)" if mirrored else "")
              + ", ".join("%s %.2e / %.2e = %.2f" % (k, kern_err[k], yard_err[k], kern_err[k] / max(yard_err[k], 1e-30))
                          for k in kern_err if k == "rows" or masks[k].any()))
        _dl_cache[key] = dict(case=case, got=got, ref=ref, masks=masks, kern_err=kern_err, yard_err=yard_err)
    return _dl_cache[key]


def dl_invariants(r):
    d_mean, rows = r["got"]
    assert np.isfinite(d_mean).all() and np.isfinite(rows).all()
    assert (np.abs(d_mean) * np.exp(r["case"]["logscale"]) <= 1 + 1e-5).all()          # |sig'(t) - sig'(s)| <= P: the true bound is 1


def dl_bound(r, key):
    return 4 * r["yard_err"][key] + 1e-6


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("name", sorted(R.DL_CASES))
def test_dl_backward_d_mean(amd, name, mirrored):
    """d_mean on every element and, separately, on the elements with s < -8, |s| <= 8 and s > 8 (each against the whole tensor's
    max|ref|): the tail cases hold all three, with |s| up to 35-100"""
    r = dl_run(amd, name, mirrored)
    dl_invariants(r)
    if name.startswith("tails"):
        assert all(r["masks"][k].sum() >= 10 for k in ("lower", "centre", "upper"))
    failed = [(k, r["kern_err"][k], dl_bound(r, k)) for k in R.DL_SUBSETS if r["kern_err"][k] > dl_bound(r, k)]
    assert not failed, failed


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("name", sorted(R.DL_CASES))
def test_dl_backward_d_logscale_rows(amd, name, mirrored):
    r = dl_run(amd, name, mirrored)
    dl_invariants(r)
    assert r["kern_err"]["rows"] <= dl_bound(r, "rows"), (r["kern_err"]["rows"], dl_bound(r, "rows"))


@pytest.mark.parametrize("name", sorted(R.DL_CASES))
def test_dl_backward_mirror_identity(amd, name):
    """(255 - k, -mean) against (k, mean): s -> -t, t -> -s and the logistic is symmetric, so d_mean comes back negated element by
    element and d_logscale_rows equal.  A one-sided evaluation does not satisfy this; no yardstick is needed to see it."""
    a, b = dl_run(amd, name), dl_run(amd, name, True)
    tol = lambda key: max(dl_bound(a, key), dl_bound(b, key))
    e_mean = float(np.abs(a["got"][0] + b["got"][0]).max() / np.abs(a["ref"][0]).max())
    e_rows = float(np.abs(a["got"][1] - b["got"][1]).max() / np.abs(a["ref"][1]).max())
    print("%s mirror identity: d_mean %.2e (bound %.2e), rows %.2e (bound %.2e)" % (name, e_mean, tol("all"), e_rows, tol("rows")))
    assert e_mean <= tol("all"), (e_mean, tol("all"))
    assert e_rows <= tol("rows"), (e_rows, tol("rows"))


def test_dl_backward_clip_gate(amd):
    """the kernel receives the clipped means (as x_dec's clip hands them on) and must return exactly 0 where torch.clamp of the pre-clip
    means does, on both sides, and a non-zero gradient everywhere else"""
    r = dl_run(amd, "clip_-2")
    pre, lo, hi = r["case"]["pre_clip_mean"], r["case"]["lo"], r["case"]["hi"]
    assert lo == np.float32(lo) and hi == np.float32(hi)
    assert not ((pre == lo) | (pre == hi)).any()                    # the derivative on a bound is a convention
    clipped = (pre < lo) | (pre > hi)
    assert (pre < lo).sum() >= 1 and (pre > hi).sum() >= 1 and 0.05 <= clipped.mean() <= 0.30
    assert np.array_equal(r["ref"][0] == 0, clipped)
    assert np.array_equal(r["got"][0] == 0, clipped)
    assert r["kern_err"]["all"] <= dl_bound(r, "all")


# ---- b. iaf_convk_wgrad ------------------------------------------------------------------------------------------------------
WGRAD_CASES = [
    # B, n_small, n_big, H, W, k, stride, elu_x, elu_dy
    (2, 3, 24, 10, 14, 5, 2, 0, 0),
    (2, 3, 24, 10, 14, 5, 2, 0, 1),      # the x_dec use: X = d x_out, DY = elu(h)
    (2, 3, 20, 9, 7, 5, 2, 0, 0),        # odd sizes, n_big % 16 = 4, OW < 16
    (2, 3, 20, 9, 7, 5, 2, 0, 1),
    (1, 1, 16, 6, 6, 3, 1, 0, 0),
    (2, 5, 7, 7, 9, 3, 1, 1, 1),         # n_big < 16
    (2, 5, 7, 7, 9, 3, 1, 0, 0),
    (1, 3, 33, 35, 34, 5, 2, 0, 0),      # OW = 17: one lane takes two columns
    (2, 3, 17, 11, 8, 4, 2, 0, 0),       # even filter: unequal SAME halves
    (1, 2, 16, 10, 10, 5, 3, 0, 0),
]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_convk_wgrad_every_tap(amd, case):
    """sums of at most B OH OW <= 612 fp32 terms of O(1): 1e-5 of the tensor's largest entry, and the same bound for every (a, c) tap
    slice against that slice's own largest entry -- a border tap wrong by one row cannot hide under a large centre tap"""
    lib, P, st = amd._capi.lib(), amd.layers._ptr, amd.layers._stream
    B, ns, nb, H, W, k, s, elu_x, elu_dy = case
    rng = np.random.RandomState(21)
    OH, OW = -(-H // s), -(-W // s)
    assert B * OH * OW <= 612
    x, dy = rng.standard_normal((B, ns, H, W)), rng.standard_normal((B, nb, OH, OW))
    dx, ddy = dev(x), dev(dy)
    dW = torch.full((k, k, ns, nb), np.nan, device="cuda")
    amd._capi.check(lib.iaf_convk_wgrad(P(dx), P(ddy), P(dW), B, ns, H, W, nb, k, k, s, elu_x, elu_dy, st()))
    got, want = host(dW), R.convk_wgrad(f32(x), f32(dy), k, k, s, elu_x, elu_dy)
    worst_tap = max(rel(got[a, c], want[a, c]) for a in range(k) for c in range(k))
    print("convk_wgrad %s: tensor %.2e, worst tap %.2e" % (case, rel(got, want), worst_tap))
    assert np.isfinite(got).all()
    assert rel(got, want) <= 1e-5
    for a in range(k):
        for c in range(k):
            assert rel(got[a, c], want[a, c]) <= 1e-5, (a, c, rel(got[a, c], want[a, c]))


# ---- c. iaf_convk_weightnorm_backward ----------------------------------------------------------------------------------------
def _wn_run(amd, V, g, dW, deconv):
    lib, P, st = amd._capi.lib(), amd.layers._ptr, amd.layers._stream
    k = V.shape[0]
    n_in, n_out = (V.shape[3], V.shape[2]) if deconv else (V.shape[2], V.shape[3])
    dVd, dgd, dWd = dev(V), dev(g), dev(dW)
    dV, dg = torch.full(V.shape, np.nan, device="cuda"), torch.full((n_out,), np.nan, device="cuda")
    scratch = torch.full((n_in * n_out,), np.nan, device="cuda") if deconv else None
    amd._capi.check(lib.iaf_convk_weightnorm_backward(P(dVd), P(dgd), P(dWd), P(dV), P(dg), P(scratch), k, k, n_in, n_out, deconv, st()))
    return host(dV), host(dg)


WN_CASES = [
    # deconv, k, n_in, n_out
    (0, 5, 3, 24),       # taps n_in = 75 < 256
    (0, 3, 40, 7),       # 360 > 256: more than one pass per thread
    (0, 1, 1, 1),
    (1, 5, 24, 3),
    (1, 3, 20, 4),
    (1, 5, 160, 1),
    (1, 3, 6, 5),
]


def _wn_inputs(deconv, k, n_in, n_out):
    rng = np.random.RandomState(31)
    shape = (k, k, n_out, n_in) if deconv else (k, k, n_in, n_out)
    return 0.05 * rng.standard_normal(shape), 0.3 * rng.standard_normal(n_out), rng.standard_normal(shape)


@pytest.mark.parametrize("case", WN_CASES, ids=lambda c: "%s_k%d_%d_%d" % ((("conv", "deconv")[c[0]],) + c[1:]))
def test_convk_weightnorm_backward(amd, case):
    """dots of at most a few hundred fp32 terms: 1e-5 of the largest entry on dV and dg each"""
    deconv = case[0]
    V, g, dW = _wn_inputs(*case)
    dV, dg = _wn_run(amd, V, g, dW, deconv)
    want_dV, want_dg = R.weightnorm_backward(f32(V), f32(g), f32(dW), deconv)
    if V.size == 1:
        # one weight per channel: w = e V / |V| does not depend on |V|, dV = (e / n) (dW - V (dW V) / V^2) is identically 0 and the
        # reference holds only its own round-off (4e-16).  Measured against the two terms that cancel, e |dW| / n each.
        term = float(np.exp(f32(g)[0]) * np.abs(f32(dW)).max() / np.abs(f32(V)).max())
        print("weightnorm_backward %s: |dV| / term %.2e, dg %.2e" % (case, np.abs(dV).max() / term, rel(dg, want_dg)))
        assert np.abs(want_dV).max() <= 1e-12 * term
        assert np.abs(dV).max() <= 1e-5 * term
    else:
        print("weightnorm_backward %s: dV %.2e, dg %.2e" % (case, rel(dV, want_dV), rel(dg, want_dg)))
        assert rel(dV, want_dV) <= 1e-5
    assert rel(dg, want_dg) <= 1e-5


@pytest.mark.parametrize("case", [(0, 3, 40, 7), (1, 3, 6, 5)], ids=["conv", "deconv"])
def test_convk_weightnorm_backward_all_zero_channel(amd, case):
    """one normalised channel of V all zeros: the clamp max(sum V^2, 1e-12) is active, both sides give dV = e dW / 1e-6 there and nothing
    is NaN.  That channel is 1e6 times the others, so it and the rest are measured separately, each against its own largest entry."""
    deconv = case[0]
    V, g, dW = _wn_inputs(*case)
    zc = 2
    V[..., zc] = 0.0                                               # the normalised channel is the last axis in both layouts
    dV, dg = _wn_run(amd, V, g, dW, deconv)
    want_dV, want_dg = R.weightnorm_backward(f32(V), f32(g), f32(dW), deconv)
    assert np.isfinite(dV).all() and np.isfinite(dg).all()
    gain = np.exp(f32(g)).reshape(1, 1, -1, 1) * np.ones(V.shape) if deconv else np.exp(f32(g))[zc]
    np.testing.assert_allclose(want_dV[..., zc], (gain * f32(dW) / 1e-6)[..., zc], rtol=1e-12)
    rest = np.arange(V.shape[-1]) != zc
    assert rel(dV[..., zc], want_dV[..., zc]) <= 1e-5
    assert rel(dV[..., rest], want_dV[..., rest]) <= 1e-5
    if deconv:
        assert rel(dg, want_dg) <= 1e-5                            # (every gain also scales the other input channels)
    else:
        assert dg[zc] == 0.0 and want_dg[zc] == 0.0
        assert rel(dg[rest], want_dg[rest]) <= 1e-5


# ---- d. iaf_channel_sum, iaf_mul_elu_grad ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 9), (2, 3, 300), (1, 17, 1)])
def test_channel_sum(amd, shape):
    lib, P, st = amd._capi.lib(), amd.layers._ptr, amd.layers._stream
    B, C, HW = shape
    x = np.random.RandomState(41).standard_normal(shape)
    xd, out = dev(x), torch.full((C,), np.nan, device="cuda")
    amd._capi.check(lib.iaf_channel_sum(P(xd), P(out), B, C, HW, st()))
    want, mag = f32(x).sum(axis=(0, 2)), np.abs(f32(x)).sum(axis=(0, 2))
    err = float((np.abs(host(out) - want) / mag).max())
    print("channel_sum %s: %.2e of sum|x|" % (shape, err))
    assert err <= 1e-6


@pytest.mark.parametrize("n", [1, 255, 1000])
def test_mul_elu_grad(amd, n):
    """out = g * (h > 0 ? 1 : exp(h)), with exact 0.0, -0.0, +-1e-30 and -90 among normal draws; at h = +-0 the result is g itself
    (exp(0) = 1: both branches agree)"""
    lib, P, st = amd._capi.lib(), amd.layers._ptr, amd.layers._stream
    rng = np.random.RandomState(42)
    g, h = rng.standard_normal(n), rng.standard_normal(n)
    special = np.array([0.0, -0.0, 1e-30, -1e-30, -90.0])
    pos = (np.arange(special.size) * 37) % n if n > 1 else np.array([0])
    h[pos] = special[:pos.size]
    gd, hd, out = dev(g), dev(h), torch.full((n,), np.nan, device="cuda")
    amd._capi.check(lib.iaf_mul_elu_grad(P(gd), P(hd), P(out), n, st()))
    got, h32 = host(out), f32(h)
    want = f32(g) * np.where(h32 > 0, 1.0, np.exp(np.minimum(h32, 0.0)))
    zero = h32 == 0
    assert zero.sum() >= 1 and np.array_equal(got[zero], f32(g)[zero])
    print("mul_elu_grad n=%d: %.2e" % (n, rel(got, want)))
    assert np.isfinite(got).all()
    assert rel(got, want) <= 2e-6


# ---- e. the data gradient of x_dec as an adjoint -----------------------------------------------------------------------------
def _deconvk(amd, x, w, n_out):
    lib, P, st = amd._capi.lib(), amd.layers._ptr, amd.layers._stream
    B, n_in, H, W = x.shape
    k = w.shape[0]
    xd, wd, bd = dev(x), dev(w), torch.zeros(n_out, device="cuda")
    y = torch.full((B, n_out, 2 * H, 2 * W), np.nan, device="cuda")
    amd._capi.check(lib.iaf_deconvk_forward(P(xd), P(wd), P(bd), P(y), B, n_in, H, W, n_out, k, k, 2, 0, 0.0, 0.0, st()))
    return host(y)


@pytest.mark.parametrize("shape", [(2, 24, 3, 5, 7, 5), (1, 16, 3, 4, 4, 3), (2, 8, 2, 3, 5, 4)])
def test_convk_forward_is_the_adjoint_of_deconvk_forward(amd, shape):
    """<deconvk(x; w), y> = <x, convk(y; w)> with the same filter memory read as [k, k, n_out, n_in] by the transposed conv and as
    [k, k, n_in', n_out'] by the strided conv: what the data gradient of x_dec relies on.  Dot products in fp64 on the host; agreement
    to 1e-5 of the sum of the terms' magnitudes."""
    lib, P, st = amd._capi.lib(), amd.layers._ptr, amd.layers._stream
    B, n_in, n_out, H, W, k = shape
    rng = np.random.RandomState(51)
    x, y = rng.standard_normal((B, n_in, H, W)), rng.standard_normal((B, n_out, 2 * H, 2 * W))
    w = 0.1 * rng.standard_normal((k, k, n_out, n_in))
    Ax = _deconvk(amd, x, w, n_out)
    yd, wd, bd = dev(y), dev(w), torch.zeros(n_in, device="cuda")
    Aty = torch.full((B, n_in, H, W), np.nan, device="cuda")
    amd._capi.check(lib.iaf_convk_forward(P(yd), P(wd), P(bd), P(Aty), B, n_out, 2 * H, 2 * W, n_in, k, k, 2, 0, st()))
    lhs_terms, rhs_terms = Ax * f32(y), f32(x) * host(Aty)
    lhs, rhs, mag = lhs_terms.sum(), rhs_terms.sum(), min(np.abs(lhs_terms).sum(), np.abs(rhs_terms).sum())
    print("x_dec adjoint %s: |lhs - rhs| / sum|terms| = %.2e" % (shape, abs(lhs - rhs) / mag))
    assert np.isfinite(lhs) and np.isfinite(rhs)
    assert abs(lhs - rhs) <= 1e-5 * mag


def test_deconvk_forward_even_filter(amd):
    """iaf_deconvk_forward itself at a 4x4 filter (unequal SAME halves) against F.conv_transpose2d: sums of n_in ceil(k/2)^2 = 32 fp32 terms,
    1e-5 of the largest output"""
    B, n_in, n_out, H, W, k = (2, 8, 2, 3, 5, 4)
    rng = np.random.RandomState(52)
    x, w = rng.standard_normal((B, n_in, H, W)), 0.1 * rng.standard_normal((k, k, n_out, n_in))
    got, want = _deconvk(amd, x, w, n_out), R.deconvk(f32(x), f32(w), 2)
    print("deconvk_forward k=4: %.2e" % rel(got, want))
    assert rel(got, want) <= 1e-5


# ---- f. iaf_resample2, all six modes -----------------------------------------------------------------------------------------
DOWN_EVEN, DOWN_ODD, UP_NEAREST, UP_ZERO_ODD, UP_ZERO_EVEN, DOWN_SUM4 = range(6)


def _resample(amd, src, mode, B, C, H, W):
    """H, W: the size of the smaller tensor"""
    lib, P, st = amd._capi.lib(), amd.layers._ptr, amd.layers._stream
    down = mode in (DOWN_EVEN, DOWN_ODD, DOWN_SUM4)
    assert src.shape == ((B, C, 2 * H, 2 * W) if down else (B, C, H, W))
    sd = dev(src)
    dst = torch.full((B, C, H, W) if down else (B, C, 2 * H, 2 * W), np.nan, device="cuda")
    amd._capi.check(lib.iaf_resample2(P(sd), P(dst), B, C, H, W, mode, st()))
    return host(dst)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 3, 5), (1, 5, 4, 2)])
def test_resample2_all_modes(amd, shape):
    B, C, H, W = shape
    rng = np.random.RandomState(61)
    big, small = f32(rng.standard_normal((B, C, 2 * H, 2 * W))), f32(rng.standard_normal(shape))
    run = lambda src, mode: _resample(amd, src, mode, B, C, H, W)
    # the copying modes and the zero-inserting ones: bit-exact against numpy indexing
    np.testing.assert_array_equal(run(big, DOWN_EVEN), big[:, :, 0::2, 0::2])
    np.testing.assert_array_equal(run(big, DOWN_ODD), big[:, :, 1::2, 1::2])
    np.testing.assert_array_equal(run(small, UP_NEAREST), small.repeat(2, axis=2).repeat(2, axis=3))
    for mode, o in ((UP_ZERO_ODD, 1), (UP_ZERO_EVEN, 0)):
        want = np.zeros_like(big)
        want[:, :, o::2, o::2] = small
        np.testing.assert_array_equal(run(small, mode), want)
    # the block sum: three fp32 additions, within 2e-7 of sum|block|
    blocks = big.reshape(B, C, H, 2, W, 2)
    got = run(big, DOWN_SUM4)
    err = float((np.abs(got - blocks.sum(axis=(3, 5))) / np.abs(blocks).sum(axis=(3, 5))).max())
    print("resample2 DOWN_SUM4 %s: %.2e of sum|block|" % (shape, err))
    assert err <= 2e-7
    # the three adjoint pairs: <A x, y> = <x, A^T y>, dot products in fp64
    for A, At in ((DOWN_EVEN, UP_ZERO_EVEN), (DOWN_ODD, UP_ZERO_ODD)):
        lhs, rhs = run(big, A) * small, big * run(small, At)
        assert abs(lhs.sum() - rhs.sum()) <= 1e-6 * min(np.abs(lhs).sum(), np.abs(rhs).sum()), (A, At)
    lhs, rhs = run(small, UP_NEAREST) * big, small * got
    assert abs(lhs.sum() - rhs.sum()) <= 1e-6 * min(np.abs(lhs).sum(), np.abs(rhs).sum())
