"""GPU leaf tests of the objective-side kernels (iaf_amd/csrc/iaf_kernels_objective.hpp, the free-bits kernels of iaf_kernels_misc.hpp and the
elementwise entry points of the init pass, iaf_kernels_edge.hpp), one by one through the raw C ABI against the fp64 references of tests/objective_reference.py (pinned on the CPU by
tests/test_objective_reference.py): iaf_kl_free_bits / iaf_kl_free_bits_gate on every route of the finish kernel that takes plain row sums, the same
reductions behind iaf_posterior_block_forward, iaf_compute_lowerbound and the streaming trio, iaf_discretized_logistic per element
and per row, the four iaf_gaussian_* entry points, iaf_datainit_normalize, iaf_colsum, iaf_kl_combine, iaf_axpby,
iaf_affine_transform, iaf_clip and iaf_noise_from_sample.  References see the fp32-rounded inputs, as the device does; outputs
are pre-filled with NaN; every test prints what it measured.

No fixed tolerances.  Reductions meet the bound derived from their documented order, (d + 2) 2^-24 sum|terms| with d the longest
chain of additions (stated per test).  The logistic, the k-sample bound and the Gaussian outputs are held to 4 x the error of a
plain fp32 restatement in the kernel's own formulation on the same inputs, plus a floor (1e-6 elementwise; one fp32 ulp of max|ref|
for the bound and for row sums).  The two kernels on the hardware exponential meet (4 + |x|) 2^-23 |ref| elementwise."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
import objective_reference as R
from oracle import iaf_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")


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


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def abi(amd):
    return amd._capi.lib(), amd.layers._ptr, amd.layers._stream, amd._capi.check


f32 = R.f32


# ---- a. iaf_kl_free_bits / iaf_kl_free_bits_gate -----------------------------------------------------------------------------
def _free_bits(amd, kl, kl_min, want_gate):
    lib, P, st, check = abi(amd)
    B, C, HW = kl.shape
    kd, obj, cost, scratch = dev(kl), nans(B), nans(B), nans(B * C)
    gate = nans(C) if want_gate else None
    if want_gate:
        check(lib.iaf_kl_free_bits_gate(P(kd), P(obj), P(cost), P(gate), B, C, HW, kl_min, P(scratch), st()))
    else:
        check(lib.iaf_kl_free_bits(P(kd), P(obj), P(cost), B, C, HW, kl_min, P(scratch), st()))
    return host(obj), host(cost), (host(gate) if want_gate else None)


def _check_free_bits(tag, obj, cost, kl, kl_min, d_row):
    """kl_cost and kl_obj against the fp64 statement on kl [B, C, HW] within the derived bounds -> the worst error / bound"""
    ref, bound = R.free_bits(kl, kl_min), R.free_bits_bounds(kl, kl_min, d_row)
    assert np.isfinite(obj).all() and np.isfinite(cost).all()
    r_cost = float((np.abs(cost - ref["kl_cost"]) / bound["kl_cost"]).max())
    r_obj = float((np.abs(obj - ref["kl_obj"]) / bound["kl_obj"]).max())
    print("%s: kl_cost error / bound %.3f, kl_obj error / bound %.3f" % (tag, r_cost, r_obj))
    assert r_cost <= 1.0 and r_obj <= 1.0, (r_cost, r_obj)
    return max(r_cost, r_obj)


@pytest.mark.parametrize("mode", R.FB_MODES)
@pytest.mark.parametrize("shape", R.FB_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kl_free_bits(amd, shape, mode):
    """d: ceil(HW / 64) + 6 inside a row sum (one wave per row), then C more for kl_cost[b]; B more, a division and the
    ceil(C / 256) + 8 of the sum over channels for kl_obj.  The gate is exactly the fp64 gate (its margins exceed the bound of the
    mean: test_objective_reference.test_free_bits_gate_margin), and a second run returns the same bits."""
    B, C, HW = shape
    kl = R.fb_case(shape, mode)
    d_row = R.fb_d_row(HW)
    obj0, cost0, _ = _free_bits(amd, kl, 0.0, False)
    _check_free_bits("free bits %s %s kl_min 0" % (shape, mode), obj0, cost0, kl, 0.0, d_row)
    assert np.array_equal(obj0, cost0)                              # tf_train.py:84: the same sum
    obj, cost, gate = _free_bits(amd, kl, R.FB_KL_MIN, True)
    _check_free_bits("free bits %s %s kl_min %.2f" % (shape, mode, R.FB_KL_MIN), obj, cost, kl, R.FB_KL_MIN, d_row)
    assert np.array_equal(cost, cost0)
    assert (obj == obj[0]).all()                                    # one value for the batch (:81)
    ref = R.free_bits(kl, R.FB_KL_MIN)
    assert np.array_equal(gate, ref["gate"])
    if mode == "below":
        assert not gate.any() and abs(obj[0] - C * R.FB_KL_MIN) <= R.free_bits_bounds(kl, R.FB_KL_MIN, d_row)["kl_obj"]
    elif mode == "above":
        assert gate.all()
    elif C > 1:
        assert gate.any() and not gate.all()
    again = _free_bits(amd, kl, R.FB_KL_MIN, True)
    plain = _free_bits(amd, kl, R.FB_KL_MIN, False)
    assert all(np.array_equal(a, b) for a, b in zip(again, (obj, cost, gate)))
    assert np.array_equal(plain[0], obj) and np.array_equal(plain[1], cost)


# ---- b. the same reductions behind iaf_posterior_block_forward ---------------------------------------------------------------
_stacks = {}
FINISH_LAUNCH = 16      # test knob of iaf_stack_set_halo_exchange_debug: the reductions by iaf_kl_finish_kernel even where the step's launch can do them


def _posterior_stack(amd, n_z, n_h, depth, knob):
    if knob not in _stacks:
        params = gi.ar_multiconv2d_params(np.random.RandomState(71), n_z, [n_h] * depth, [n_z, n_z])
        stack = amd.ARStack(n_z, [n_h] * depth)
        stack.set_halo_exchange_debug(knob)
        stack.prepare({k: dev(v) for k, v in params.items()})
        _stacks[knob] = stack
    return _stacks[knob]


@pytest.mark.parametrize("kl_min", [0.0, R.FB_KL_MIN])
@pytest.mark.parametrize("B,H", [(5, 16), (64, 16), (65, 16), (5, 8), (33, 8)])
def test_posterior_block_reductions(amd, B, H, kl_min):
    """kl_cost and kl_obj of one call against the fp64 free-bits statement applied to the kl_elem the SAME call returned (the conv
    arithmetic is judged elsewhere).  16x16 runs in 8 row blocks: B = 64 and 65 sit on either side of the 16384 loads at which the
    sum over the row blocks becomes a launch of its own.  d: the step kernel's order inside a row block is its own, so the row sum
    is bounded by its length, HW additions in any order, + 16 for the row blocks; then Z or B as above.  Each size runs as
    shipped (up to B n_rb Z = 16384 the step's own launch finishes the reductions) and with the existing test knob that hands them
    to iaf_kl_finish_kernel: its sum over the row blocks in rounds of eight, four channels at a time, staged in LDS.  Not reached
    here or by any caller of the one-launch step, whose n_z is a multiple of 16 and whose geometries have several row blocks: the
    scalar form of that sum (Z no multiple of 4), a last round cut short (both geometries have exactly 8 row blocks) and its write
    to global scratch (B Z > 8192 with B n_rb Z <= 16384, i.e. one row block)."""
    lib, P, st, check = abi(amd)
    n_z, n_h, depth, W = 32, 160, 2, H
    rng = np.random.RandomState(72 + B + H)
    f = lambda c, sc: dev(sc * rng.standard_normal((B, c, H, W)))
    # small posterior / prior offsets: at kl_min = 0.25 channels fall on both sides of the free-bits max
    qm, ql, rm, rl, pm, pl = f(n_z, 0.1), f(n_z, 0.05), f(n_z, 0.1), f(n_z, 0.05), f(n_z, 0.1), f(n_z, 0.05)
    uc, dc, eps = f(n_h, 1.0), f(n_h, 1.0), f(n_z, 0.05)
    results = []
    for knob, route in ((0, "as shipped"), (FINISH_LAUNCH, "finish launch")):
        stack = _posterior_stack(amd, n_z, n_h, depth, knob)
        rows = stack.step_is_fused(B, H, W)                         # rows per workgroup of the one-launch step
        assert rows > 0
        nrb = -(-H // rows)
        if H == 16:
            assert nrb == 8                                         # what puts B = 64 and 65 on either side of 16384 = 64 * 8 * 32
        if B * nrb * n_z > 16384:
            how = "iaf_kl_partsum_kernel, then iaf_kl_finish_kernel on plain sums"
        elif knob == 0:
            assert B * n_z <= 8192
            how = "inside the step's launch (where its kernel has helper waves; else as below)"
        else:
            how = "iaf_kl_finish_kernel on the row blocks' partial sums"
        print("    %d row blocks, reductions: %s" % (nrb, how))
        z, obj, cost, kl_elem = nans(B, n_z, H, W), nans(B), nans(B), nans(B, n_z, H, W)
        ws, need = stack.workspace(B, H, W, z.device)
        check(lib.iaf_posterior_block_forward(stack._h, P(qm), P(ql), P(rm), P(rl), P(pm), P(pl), P(uc), P(dc), P(eps), kl_min, P(z),
                                              P(obj), P(cost), P(kl_elem), B, H, W, P(ws), need, st()))
        torch.cuda.synchronize()
        assert stack.exchange_errors() == 0
        kl = host(kl_elem).reshape(B, n_z, H * W)
        assert np.isfinite(kl).all() and np.isfinite(host(z)).all()
        _check_free_bits("posterior block B=%d %dx%d kl_min %.2f, %s" % (B, H, W, kl_min, route), host(obj), host(cost), kl, kl_min,
                         H * W + 16)
        if kl_min > 0:
            gate = R.free_bits(kl, kl_min)["gate"]
            print("    channels above kl_min: %d of %d" % (int(gate.sum()), n_z))
            assert gate.any() and not gate.all()
            assert (host(obj) == host(obj)[0]).all()
        else:
            assert np.array_equal(host(obj), host(cost))
        results.append(kl)
    assert np.array_equal(results[0], results[1])                   # the same step either way: only the reductions' route differs


# ---- c. iaf_compute_lowerbound and the streaming trio ------------------------------------------------------------------------
def _lb_oneshot(amd, lp, kl):
    lib, P, st, check = abi(amd)
    n, k = lp.shape
    a, b, out = dev(lp.reshape(-1)), dev(kl.reshape(-1)), nans(n)
    check(lib.iaf_compute_lowerbound(P(a), P(b), P(out), n, k, st()))
    return host(out)


def _lb_streamed(amd, lp, kl, chunks):
    lib, P, st, check = abi(amd)
    n, k = lp.shape
    run_max, run_sum, out = nans(n), nans(n), nans(n)
    check(lib.iaf_lowerbound_stream_init(P(run_max), P(run_sum), n, st()))
    o = 0
    for kc in chunks:
        a, b = dev(lp[:, o:o + kc]), dev(kl[:, o:o + kc])
        check(lib.iaf_lowerbound_stream_update(P(run_max), P(run_sum), P(a), P(b), n, kc, st()))
        o += kc
    assert o == k
    check(lib.iaf_lowerbound_stream_finalize(P(run_max), P(run_sum), P(out), n, k, st()))
    return host(out)


@pytest.mark.parametrize("n", R.LB_NS)
@pytest.mark.parametrize("kind", R.LB_KINDS)
def test_lowerbound(amd, kind, n):
    """k = 2, 63, 64, 65, 1000 in one shot; k = 1000 also streamed in chunks of (1, 63, 65, 871) and the reverse, and in one shot with
    every image's samples permuted.  Each result within 4 x the fp32 yardstick's error (run over the same chunks) + one ulp of
    max|ref|; the permuted result within that bound of the unpermuted one; equal weights give -w within one ulp."""
    worst = (0.0, 0.0)
    for k in R.LB_KS:
        lp, kl = R.lb_case(kind, n, k)
        ref = R.lowerbound(lp, kl, k)
        runs = [("one shot", (k,), _lb_oneshot(amd, lp, kl))]
        if k == R.LB_K:
            runs += [("streamed %s" % (c,), c, _lb_streamed(amd, lp, kl, c)) for c in (R.LB_CHUNKS, R.LB_CHUNKS[::-1])]
        for tag, chunks, got in runs:
            yard = R.fp32_yardstick_lowerbound(lp, kl, chunks)
            err, y_err, bound = float(np.abs(got - ref).max()), float(np.abs(yard - ref).max()), R.lb_bound(yard, ref)
            ulp = float(R.ulp32(np.abs(ref).max()))
            print("lowerbound %s n=%d k=%d %s: kernel %.2f ulp, yardstick %.2f ulp, bound %.2f ulp" % (kind, n, k, tag, err / ulp, y_err / ulp, bound / ulp))
            assert np.isfinite(got).all()
            assert err <= bound, (tag, err, bound)
            worst = max(worst, (err / ulp, y_err / ulp))
            if kind == "equal":
                assert np.abs(got - 7900.0).max() <= R.ulp32(7900.0)
        if k == R.LB_K:
            rng = np.random.RandomState(33)
            perm = np.stack([rng.permutation(k) for _ in range(n)])
            moved = _lb_oneshot(amd, np.take_along_axis(lp, perm, axis=1), np.take_along_axis(kl, perm, axis=1))
            bound = R.lb_bound(R.fp32_yardstick_lowerbound(lp, kl, (k,)), ref)
            print("lowerbound %s n=%d k=%d permuted: moved by %.2e (bound %.2e)" % (kind, n, k, np.abs(moved - runs[0][2]).max(), bound))
            assert np.abs(moved - runs[0][2]).max() <= bound
    print("lowerbound %s n=%d: worst kernel %.2f ulp, worst yardstick %.2f ulp of max|ref|" % ((kind, n) + worst))


@pytest.mark.parametrize("n", R.LB_NS)
def test_lowerbound_k1_is_the_fp32_difference(amd, n):
    lp, kl = R.lb_case("today", n, 1)
    got = _lb_oneshot(amd, lp, kl)
    assert np.array_equal(got, (kl.astype(np.float32) - lp.astype(np.float32)).reshape(-1).astype(np.float64))


# ---- d. iaf_discretized_logistic ----------------------------------------------------------------------------------------------
DL_MAX_ELEMS = 4096
_dl_cache = {}


def _dl_launch(amd, mean, logscale, sample, B, n):
    lib, P, st, check = abi(amd)
    scalar = np.ndim(logscale) == 0
    m, x, ls, out = dev(mean), dev(sample), dev(np.array([logscale]) if scalar else logscale), nans(B)
    check(lib.iaf_discretized_logistic(P(m), P(ls), 1 if scalar else 0, P(x), P(out), B, n, R.BINSIZE, st()))
    return host(out)


def dl_run(amd, name):
    """one case through the kernel twice -- its rows at the case's own row length, and the first DL_MAX_ELEMS elements as rows of
    one element -- and through the fp64 reference and the fp32 yardstick (each computed once per module)"""
    if name not in _dl_cache:
        c = R.dl_fwd_case(name)
        B, n = c["mean"].shape
        scalar = np.ndim(c["logscale"]) == 0
        rows = _dl_launch(amd, c["mean"], c["logscale"], c["sample"], B, n)
        ne = min(B * n, DL_MAX_ELEMS)
        flat = lambda a: np.ascontiguousarray(a).reshape(-1)[:ne]
        elem = _dl_launch(amd, flat(c["mean"]), c["logscale"] if scalar else flat(c["logscale"]), flat(c["sample"]), ne, 1)
        ref = R.dl_logp(c["mean"], c["logscale"], c["sample"])
        yard, yard_rows = R.fp32_yardstick_dl(c["mean"], c["logscale"], c["sample"])
        masks = {k: flat(m) for k, m in R.dl_masks(c).items()}
        ref_rows = ref.sum(axis=1)
        kern_err = R.dl_fwd_errors(elem, rows, flat(ref), ref_rows, masks)
        yard_err = R.dl_fwd_errors(flat(yard), yard_rows, flat(ref), ref_rows, masks)
        print("logistic %s kernel / yardstick error: " % name
              + ", ".join("%s %.2e / %.2e = %.2f" % (k, kern_err[k], yard_err[k], kern_err[k] / max(yard_err[k], 1e-30))
                          for k in kern_err if k == "rows" or masks[k].any()))
        _dl_cache[name] = dict(case=c, rows=rows, elem=elem, ref=flat(ref), ref_rows=ref_rows, masks=masks, kern_err=kern_err,
                               yard_err=yard_err)
    return _dl_cache[name]


@pytest.mark.parametrize("name", R.DL_FWD_CASES)
def test_discretized_logistic(amd, name):
    """every element (launched as rows of one element) and, separately, the elements with s < -8, |s| <= 8 and s > 8; and the row
    sums at the case's own row length (n_per_row 1, 192, 193, 255, 256, 257, 3072).  log P lies in [log 1e-7, 0]."""
    r = dl_run(amd, name)
    assert np.isfinite(r["elem"]).all() and np.isfinite(r["rows"]).all()
    assert (r["elem"] <= 1e-6).all() and (r["elem"] >= np.log(1e-7) - 1e-5).all()
    if name.startswith(("tails", "size")) and r["case"]["n_per_row"] >= 192:
        assert all(r["masks"][k].sum() >= 10 for k in ("lower", "centre", "upper"))
    keys = ("all", "lower", "centre", "upper", "rows")
    failed = [(k, r["kern_err"][k], R.dl_fwd_bound(r["yard_err"], k, r["ref_rows"])) for k in keys
              if r["kern_err"][k] > R.dl_fwd_bound(r["yard_err"], k, r["ref_rows"])]
    assert not failed, failed


@pytest.mark.parametrize("name", [n for n in R.DL_FWD_CASES if n + " (mirrored)" in R.DL_FWD_CASES])
def test_discretized_logistic_mirror_identity(amd, name):
    """(255 - k, -mean) against (k, mean): s -> -(s + d) and the logistic is symmetric, so every element's log-probability comes back
    equal.  A one-sided evaluation does not satisfy this; no yardstick is needed to see it."""
    a, b = dl_run(amd, name), dl_run(amd, name + " (mirrored)")
    tol = lambda key: max(R.dl_fwd_bound(a["yard_err"], key, a["ref_rows"]), R.dl_fwd_bound(b["yard_err"], key, b["ref_rows"]))
    e_elem = float(np.abs(a["elem"] - b["elem"]).max())
    e_rows = float(np.abs(a["rows"] - b["rows"]).max() / np.abs(a["ref_rows"]).max())
    print("logistic %s mirror identity: elements %.2e (bound %.2e), rows %.2e (bound %.2e)" % (name, e_elem, tol("all"), e_rows, tol("rows")))
    assert e_elem <= tol("all") and e_rows <= tol("rows")


# ---- e. iaf_gaussian_sample, _sample_logsd, _logps, _logps_logsd -------------------------------------------------------------
def _gauss(amd, fn, a, b, c):
    lib, P, st, check = abi(amd)
    out = nans(a.numel())
    check(getattr(lib, fn)(P(a), P(b), P(c), P(out), a.numel(), st()))
    return out


@pytest.mark.parametrize("n", R.GAUSS_NS)
def test_gaussian_entry_points(amd, n):
    """logvar in [-20, 20], (x - mean) / sd up to 30; n = 2048 * 256 + 3 takes the second trip of the stride loop.  Against fp64 within
    4 x the fp32 yardstick's error + 1e-6, relative to max|ref| and, element by element, relative to the magnitude of the element's
    own terms (objective_reference.gauss_scales: max|ref| of the sample is 6.6e5, which alone would hide every small element); the
    logsd forms bit-equal to the logvar forms at 2 logsd; the
    log-density at sample = mean equal to -(log 2 pi + logvar) / 2 within one ulp at |ref| + log 2 pi (the constant's and the
    sum's rounding)."""
    c = R.gauss_case(n)
    mean, logsd, logvar, noise, sample = (dev(c[k]) for k in ("mean", "logsd", "logvar", "noise", "sample"))
    s_lv, s_sd = _gauss(amd, "iaf_gaussian_sample", mean, logvar, noise), _gauss(amd, "iaf_gaussian_sample_logsd", mean, logsd, noise)
    l_lv, l_sd = _gauss(amd, "iaf_gaussian_logps", mean, logvar, sample), _gauss(amd, "iaf_gaussian_logps_logsd", mean, logsd, sample)
    torch.cuda.synchronize()
    assert torch.equal(s_lv, s_sd) and torch.equal(l_lv, l_sd)
    sc_sample, sc_logps = R.gauss_scales(c)
    for tag, got, ref, yard, scale in (("sample", host(s_lv), O.gaussian_diag_sample(c["mean"], c["logvar"], c["noise"]),
                                        R.fp32_yardstick_gauss_sample(c["mean"], c["logvar"], c["noise"]), sc_sample),
                                       ("logps", host(l_lv), O.gaussian_diag_logps(c["mean"], c["logvar"], c["sample"]),
                                        R.fp32_yardstick_gauss_logps(c["mean"], c["logvar"], c["sample"]), sc_logps)):
        err, y_err = R.rel_err(got, ref), R.rel_err(yard, ref)
        e_el, y_el = R.scaled_err(got, ref, scale), R.scaled_err(yard, ref, scale)
        print("gaussian %s n=%d kernel / yardstick error: of max|ref| %.2e / %.2e = %.2f; per element, of its own terms %.2e / %.2e = %.2f"
              % (tag, n, err, y_err, err / max(y_err, 1e-30), e_el, y_el, e_el / max(y_el, 1e-30)))
        assert np.isfinite(got).all()
        assert err <= 4 * y_err + 1e-6, (tag, err, y_err)
        assert e_el <= 4 * y_el + 1e-6, (tag, e_el, y_el)
    at_mean = host(_gauss(amd, "iaf_gaussian_logps", mean, logvar, mean))
    want = -0.5 * (np.log(2 * np.pi) + c["logvar"])
    assert (np.abs(at_mean - want) <= R.ulp32(np.abs(want) + np.log(2 * np.pi))).all()


# ---- f. iaf_datainit_normalize -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("name", sorted(R.DI_CASES))
def test_datainit_normalize(amd, name, with_add):
    """g, b and y each within 4 x the error of a plain two-pass fp32 restatement on the same inputs + 1e-6, absolute (worst error over the
    tensor; b reaches 1.3e4 and 1e3 in two cases, where 1e-6 is far below an ulp: the factor alone carries them), and inside the
    looser bounds derived from the kernel's two passes (objective_reference.datainit_bounds: d = ceil(n / 256) + 9 per sum); the
    same g and b with y = NULL"""
    lib, P, st, check = abi(amd)
    B, C, HW, _ = R.DI_CASES[name]
    x, add = R.di_case(name)
    add = add if with_add else None
    xd, ad = dev(x), (dev(add) if with_add else None)
    y, g, b = nans(B, C, HW), nans(C), nans(C)
    check(lib.iaf_datainit_normalize(P(xd), P(ad), P(y), P(g), P(b), B, C, HW, R.DI_INIT_SCALE, st()))
    g0, b0 = nans(C), nans(C)
    check(lib.iaf_datainit_normalize(P(xd), P(ad), P(None), P(g0), P(b0), B, C, HW, R.DI_INIT_SCALE, st()))
    got = dict(g=host(g), b=host(b), y=host(y))
    assert np.array_equal(host(g0), got["g"]) and np.array_equal(host(b0), got["b"])
    ref, bound, yard = R.datainit(x, add), R.datainit_bounds(x, add), R.fp32_datainit(x, add)
    for k in ("g", "b", "y"):
        assert np.isfinite(got[k]).all()
        err, y_err = float(np.abs(got[k] - ref[k]).max()), float(np.abs(yard[k] - ref[k]).max())
        ratio = float((np.abs(got[k] - ref[k]) / bound[k]).max())
        print("datainit %s%s %s: kernel / two-pass fp32 error %.2e / %.2e = %.2f (max|ref| %.3g); error / derived bound %.3f"
              % (name, " +add" if with_add else "", k, err, y_err, err / max(y_err, 1e-30), np.abs(ref[k]).max(), ratio))
        assert err <= 4 * y_err + 1e-6, (k, err, y_err)
        assert ratio <= 1.0, (k, ratio)


# ---- g. the entry points no test named ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(m, n) for m in (1, 20) for n in (1, 255, 257)])
def test_colsum(amd, m, n):
    """d = m additions down a column"""
    lib, P, st, check = abi(amd)
    mat = f32(np.random.RandomState(81).standard_normal((m, n)) * 900.0)
    md, out = dev(mat), nans(n)
    check(lib.iaf_colsum(P(md), P(out), m, n, st()))
    ratio = float((np.abs(host(out) - mat.sum(axis=0)) / R.sum_bound(m, np.abs(mat).sum(axis=0))).max())
    print("colsum %dx%d: error / bound %.3f" % (m, n, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("n", R.EW_NS)
def test_kl_combine_axpby_clip(amd, n):
    lib, P, st, check = abi(amd)
    a, b, c = R.ew_case(n, 3, 1)
    ad, bd, cd = dev(a), dev(b), dev(c)
    a32, b32, c32 = (v.astype(np.float32) for v in (a, b, c))
    out = nans(n)
    check(lib.iaf_kl_combine(P(ad), P(bd), P(cd), P(out), n, st()))
    assert np.array_equal(host(out), ((a32 + b32) - c32).astype(np.float64))                    # models.py:175: (logq0 + logdet) - logp
    # axpby: each product rounds at most once (not at all where it is contracted into an FMA) and so does the sum: half an ulp of each
    # product and half an ulp of the result.  (One ulp of each product alone, without the result's, is not a bound that fp32 can
    # keep: a sum that lands one binade above both products is exceeded 1.43-fold by a correctly rounded FMA.)
    sa, sb = float(np.float32(0.1)), float(np.float32(-1.7))
    out = nans(n)
    check(lib.iaf_axpby(P(ad), sa, P(bd), sb, P(out), n, st()))
    exact = sa * a + sb * b
    err = np.abs(host(out) - exact)
    tol = 0.5 * (R.ulp32(sa * a) + R.ulp32(sb * b) + R.ulp32(exact))
    print("axpby n=%d: worst error / (half an ulp of each product and of the result) %.3f; / (one ulp of each product) %.3f"
          % (n, float((err / tol).max()), float((err / (R.ulp32(sa * a) + R.ulp32(sb * b))).max())))
    assert np.isfinite(host(out)).all()
    assert (err <= tol).all()
    # clip: bit-exact, the bounds included
    lo, hi = -0.5 + 1 / 512.0, 0.5 - 1 / 512.0
    x = a.copy()
    x[::7], x[3::7] = lo, hi
    x = x[:n]
    assert (x == lo).any() and (n < 4 or (x == hi).any())
    xd, out = dev(x), nans(n)
    check(lib.iaf_clip(P(xd), lo, hi, P(out), n, st()))
    assert np.array_equal(host(out), np.minimum(np.maximum(x, lo), hi))


@pytest.mark.parametrize("n", R.EW_NS)
def test_affine_transform(amd, n):
    """(z - scale m) / exp(scale s) under objective_reference.hw_exp_bound, |scale s| <= 8"""
    lib, P, st, check = abi(amd)
    z, m, s = R.affine_case(n)
    zd, md, sd, out = dev(z), dev(m), dev(s), nans(n)
    check(lib.iaf_affine_transform(P(zd), P(md), P(sd), R.AFFINE_SCALE, P(out), n, st()))
    ref, x = R.affine_transform(z, m, s)
    ratio = np.abs(host(out) - ref) / R.hw_exp_bound(x, ref)
    print("affine_transform n=%d: worst error / bound %.3f (at x = %.2f); worst relative error %.2e"
          % (n, ratio.max(), x[np.argmax(ratio)], (np.abs(host(out) - ref) / np.abs(ref)).max()))
    assert np.isfinite(host(out)).all()
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("n", R.EW_NS)
def test_noise_from_sample(amd, n):
    """eps' = (z - (qm + rm)) exp(-(ql + rl)) under the same bound, and as a round trip: iaf_gaussian_sample_logsd(qm + rm, ql + rl,
    eps') gives z back within (6 + |x|) 2^-23 (|z| + |qm + rm|): eps' as bounded, expf and its product another 1.5 2^-23 of the
    difference, the final sum 2^-24 |z|"""
    lib, P, st, check = abi(amd)
    z, qm, ql, rm, rl = R.noise_case(n)
    zd, qmd, qld, rmd, rld = (dev(a) for a in (z, qm, ql, rm, rl))
    eps = nans(n)
    check(lib.iaf_noise_from_sample(P(zd), P(qmd), P(qld), P(rmd), P(rld), P(eps), n, st()))
    ref, x = R.noise_from_sample(z, qm, ql, rm, rl)
    ratio = np.abs(host(eps) - ref) / R.hw_exp_bound(x, ref)
    print("noise_from_sample n=%d: worst error / bound %.3f (at x = %.2f); worst relative error %.2e"
          % (n, ratio.max(), x[np.argmax(ratio)], (np.abs(host(eps) - ref) / np.abs(ref)).max()))
    assert np.isfinite(host(eps)).all()
    assert ratio.max() <= 1.0
    mean, logsd, back = qmd + rmd, qld + rld, nans(n)
    check(lib.iaf_gaussian_sample_logsd(P(mean), P(logsd), P(eps), P(back), n, st()))
    trip = np.abs(host(back) - z) / ((6.0 + np.abs(x)) * 2.0 ** -23 * (np.abs(z) + np.abs(qm + rm)))
    print("noise_from_sample n=%d round trip: worst error / bound %.3f" % (n, trip.max()))
    assert trip.max() <= 1.0
