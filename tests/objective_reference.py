"""NumPy-fp64 statements of the objective-side operations (the numbers the project reports: kl_obj, kl_cost, the free-bits gate, log_pxz,
the k-sample bound, the data-dependent init), written from the reference's lines as the kernels cite them (tf_train.py:77-85,
tf_utils/distributions.py:5-62, tf_utils/layers.py:45-51) and reusing oracle/iaf_oracle.py where it already states the operation;
plain fp32 yardsticks in the kernels' own formulation that a kernel's error is measured against; the derived bounds of the
reductions; and the seed-fixed case generators, so that the CPU test of the references and the GPU test of the kernels see the same
numbers.  What tests/test_hip_objective_kernels.py compares the kernels with; pinned by tests/test_objective_reference.py.  Does
not import the GPU library.

Bounds.  A reduction whose longest chain of fp32 additions is d meets |got - ref| <= (d + 2) 2^-24 sum|terms| (sum_bound): the
standard forward bound of a summation of depth d, with two roundings to spare.  Everything else is held to 4 x the error of its
fp32 yardstick on the same inputs plus a floor (the rule of tests/test_hip_model_edge_backward.py)."""
import numpy as np

from model_edge_reference import BINSIZE, DL_B, DL_CASES, dl_case, dl_mirrored, dl_s, dl_subsets, f32  # noqa: F401 (shared with the tests)
from oracle import iaf_oracle as O

U = 2.0 ** -24                                                      # unit roundoff of fp32
F = np.float32


def ulp32(v):
    """one fp32 ulp at |v| (v a float64 scalar or array)"""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def exp32(x):
    """correctly rounded fp32 exp (through fp64)"""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.asarray(x, dtype=np.float32).astype(np.float64)).astype(np.float32)


def log32(x):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(x, dtype=np.float32).astype(np.float64)).astype(np.float32)


def sum_bound(d, terms_abs_sum):
    return (d + 2) * U * terms_abs_sum


# --------------------------------------------------------------------------------------
# free bits (tf_train.py:77-85) on kl [B, C, HW]
# --------------------------------------------------------------------------------------
FB_KL_MIN = 0.25
FB_SHAPES = [(1, 1, 1), (3, 8, 20), (2, 7, 65), (2, 300, 5), (300, 3, 5), (128, 64, 4), (129, 64, 4), (2, 32, 1024)]
FB_MODES = ("both", "below", "above")                              # the channels' batch means relative to FB_KL_MIN


def free_bits(kl, kl_min):
    """-> dict(kl_cost [B], kl_obj [B], gate [C], mean_c [C]) in fp64; the gate is where max() passes the gradient (:79-80)"""
    kl = np.asarray(kl, np.float64)
    B = kl.shape[0]
    S = kl.sum(axis=2)                                               # sum over (H, W)
    kl_cost = S.sum(axis=1)                                          # :85
    mean_c = S.mean(axis=0)                                          # :79
    if kl_min > 0:
        kl_obj = np.tile(np.maximum(mean_c, kl_min)[None], [B, 1]).sum(axis=1)   # :80-82
    else:
        kl_obj = kl_cost.copy()                                      # :84
    return dict(kl_cost=kl_cost, kl_obj=kl_obj, gate=(mean_c > kl_min).astype(np.float64), mean_c=mean_c)


def free_bits_per_image_clamp(kl, kl_min):
    """WRONG on purpose (the CPU test shows the bound sees it): clamps every image's channel sums instead of their batch mean"""
    return np.maximum(np.asarray(kl, np.float64).sum(axis=2), kl_min).sum(axis=1)


def free_bits_bounds(kl, kl_min, d_row):
    """the derived bounds of the three outputs; d_row: the longest chain of additions inside one (b, c) row sum.
    kl_cost[b]: d_row + C additions over all of image b.  mean_c: d_row + B additions and one division, over channel c of every
    image, / B.  kl_obj (kl_min > 0): max() is 1-Lipschitz, so the means' errors add up, plus the sum over the C clamped means
    (ceil(C / 256) per thread, then an 8-level tree).  -> dict(kl_cost [B], mean_c [C], kl_obj scalar or [B])"""
    A = np.abs(np.asarray(kl, np.float64))
    B, C = A.shape[0], A.shape[1]
    cost = sum_bound(d_row + C, A.sum(axis=(1, 2)))
    mean_c = sum_bound(d_row + B + 1, A.sum(axis=(0, 2)) / B)
    if kl_min > 0:
        clamped = np.maximum(np.asarray(kl, np.float64).sum(axis=2).mean(axis=0), kl_min)
        obj = mean_c.sum() + sum_bound(-(-C // 256) + 8, np.abs(clamped).sum())
    else:
        obj = cost
    return dict(kl_cost=cost, mean_c=mean_c, kl_obj=obj)


def fb_d_row(HW):
    """iaf_kl_rowsum_kernel: one wave per row, ceil(HW / 64) additions per lane, then six shuffle steps"""
    return -(-HW // 64) + 6


def fb_case(shape, mode):
    """kl [B, C, HW], fp32-rounded: N(0, 1) elements (both signs) shifted per channel so that its batch mean sits on a target at least
    20 % away from FB_KL_MIN -- below it, above it, or alternating ("both"; a single channel sits above)"""
    B, C, HW = shape
    rng = np.random.RandomState(2000 + 10 * FB_SHAPES.index(shape) + FB_MODES.index(mode))
    x = rng.standard_normal(shape)
    lo, hi = rng.uniform(0.02, 0.2, C), rng.uniform(0.3, 1.5, C)
    target = {"below": lo, "above": hi, "both": np.where(np.arange(C) % 2 == 0, hi, lo)}[mode]
    x += ((target - x.sum(axis=2).mean(axis=0)) / HW)[None, :, None]
    return f32(x)


# --------------------------------------------------------------------------------------
# the k-sample bound (distributions.py:55-62), one shot and streamed
# --------------------------------------------------------------------------------------
LB_N, LB_K = 257, 1000
LB_NS = (1, 3, 5, 257)
LB_KS = (2, 63, 64, 65, 1000)
LB_CHUNKS = (1, 63, 65, 871)
LB_KINDS = ("today", "spread300", "equal", "latemax")
LB_MAX_POS = (0, 100, 900, 999)     # of image i: LB_MAX_POS[i % 4], the first / a middle / the last chunk of LB_CHUNKS and of its reverse


def lb_case(kind, n, k):
    """(log_pxz, sum_kl) [n, k], fp32-rounded.  today: lp ~ -7000 +- 30, kl ~ 900 +- 20; spread300: the weights spread over 300 nats
    (most terms underflow against the maximum); equal: every weight -7900 exactly; latemax: today's, with one weight per image
    raised by 20 nats at position LB_MAX_POS[i % 4] (clipped to k - 1)"""
    rng = np.random.RandomState(3000 + LB_KINDS.index(kind))
    lp = -7000 + 30 * rng.standard_normal((LB_N, LB_K))
    kl = 900 + 20 * rng.standard_normal((LB_N, LB_K))
    if kind == "spread300":
        lp = -7000 - 300 * rng.uniform(size=(LB_N, LB_K))
    elif kind == "equal":
        lp[:], kl[:] = -7000.0, 900.0
    lp, kl = lp[:n, :k].copy(), kl[:n, :k].copy()
    if kind == "latemax":
        for i in range(n):
            p = min(LB_MAX_POS[i % 4], k - 1)
            lp[i, p], kl[i, p] = (lp[i] - kl[i]).max() + 20.0 + 900.0, 900.0
    return f32(lp), f32(kl)


def lowerbound(lp, kl, k):
    """fp64, [n, k] -> [n]"""
    return O.compute_lowerbound(np.asarray(lp, np.float64).reshape(-1), np.asarray(kl, np.float64).reshape(-1), k)


def fp32_yardstick_lowerbound(lp, kl, chunks, rescale=True):
    """the kernels' formulation in numpy float32, chunk by chunk: w = lp - kl, a running maximum and a sum rescaled by
    exp(old max - new max) whenever the maximum moves, correctly rounded exp and log; each chunk's sum is numpy's.
    rescale=False is WRONG on purpose: the running sum is never rescaled."""
    w = np.asarray(lp, F) - np.asarray(kl, F)
    n, k = w.shape
    assert sum(chunks) == k
    run_max, run_sum = np.full(n, -np.inf, F), np.zeros(n, F)
    o = 0
    for kc in chunks:
        c = w[:, o:o + kc]
        o += kc
        new_max = np.maximum(run_max, c.max(axis=1))
        s = np.sum(exp32(c - new_max[:, None]), axis=1, dtype=F)
        old = np.where(np.isinf(run_max), F(0), run_sum * exp32(run_max - new_max)) if rescale else run_sum
        run_sum, run_max = (old + s).astype(F), new_max
    out = -((-log32(F(k)) + run_max) + log32(run_sum))
    assert out.dtype == F
    return out.astype(np.float64)


def lb_bound(yard, ref):
    """4 x the yardstick's worst error + one fp32 ulp of max|ref|, absolute"""
    return 4 * float(np.abs(yard - ref).max()) + float(ulp32(np.abs(ref).max()))


# --------------------------------------------------------------------------------------
# discretized logistic, forward (distributions.py:28-32)
# --------------------------------------------------------------------------------------
def dl_logp(mean, logscale, sample, binsize=BINSIZE):
    """fp64, elementwise: log(sig(s + b / scale) - sig(s) + 1e-7), s = (floor(x / b) b - mean) / scale; logscale a scalar or an array"""
    mean, sample = np.asarray(mean, np.float64), np.asarray(sample, np.float64)
    scale = np.exp(np.asarray(logscale, np.float64))
    s = (np.floor(sample / binsize) * binsize - mean) / scale
    sig = lambda t: 1.0 / (1.0 + np.exp(-t))
    return np.log(sig(s + binsize / scale) - sig(s) + 1e-7)


def fp32_yardstick_dl(mean, logscale, sample, binsize=BINSIZE, literal=False):
    """the same in numpy float32 with correctly rounded exp and log, in the kernel's formulation: where s > 0 the difference is taken
    on the mirrored side, e / (1 + e) with e = exp(-s) and exp(-(s + d)) (both terms small); elsewhere the literal
    sig(s + d) - sig(s).  literal=True is WRONG on purpose: the literal form everywhere.  -> (logp elementwise, row sums over the
    last axis: numpy's)"""
    m, x = np.asarray(mean, F), np.asarray(sample, F)
    b = F(binsize)
    scale = exp32(np.broadcast_to(np.asarray(logscale, F), m.shape))
    s = (np.floor(x / b) * b - m) / scale
    d = b / scale
    with np.errstate(over="ignore"):
        e0, e1 = exp32(-s), exp32(-(s + d))
        lit = F(1) / (F(1) + e1) - F(1) / (F(1) + e0)
        with np.errstate(invalid="ignore"):
            mir = e0 / (F(1) + e0) - e1 / (F(1) + e1)               # (inf / inf where s << 0: not selected there)
    diff = lit if literal else np.where(s > 0, mir, lit)
    logp = log32(diff + F(1e-7))
    rows = np.sum(logp, axis=-1, dtype=F)
    assert logp.dtype == F and rows.dtype == F
    return logp.astype(np.float64), rows.astype(np.float64)


DL_SIZES = [(B, n) for B in (1, 3) for n in (1, 255, 256, 257, 3072)]
DL_TAIL = -3.0                                                       # the logscale of the size cases: the upper tail matters from here on


def dl_size_case(B, n, per_element_logscale=False):
    """the "tails" recipe of model_edge_reference.dl_case at [B, n]; logscale DL_TAIL, or drawn per element from [-5, 0]"""
    rng = np.random.RandomState(1500 + 7 * n + B + (50 if per_element_logscale else 0))
    k = rng.randint(0, 256, size=(B, n))
    sample = (k + 0.5) / 256.0 - 0.5
    mean = f32(np.clip(sample + 0.3 * rng.standard_normal((B, n)), -0.6, 0.6))
    logscale = f32(rng.uniform(-5.0, 0.0, size=(B, n))) if per_element_logscale else DL_TAIL
    return dict(k=k, sample=sample, mean=mean, logscale=logscale, n_per_row=n)


DL_FWD_CASES = ([n for name in sorted(DL_CASES) for n in (name, name + " (mirrored)")] + ["size %dx%d" % bn for bn in DL_SIZES]
                + ["per-element logscale", "per-element logscale (mirrored)"])


def dl_fwd_case(name):
    """every case of the forward checks by name: model_edge_reference's likelihood cases and their mirror images, the size cases,
    and one case with a logscale per element"""
    if name.endswith(" (mirrored)"):
        c = dl_fwd_case(name[:-len(" (mirrored)")])
        m = dict(c, k=255 - c["k"], mean=-c["mean"])
        m["sample"] = (m["k"] + 0.5) / 256.0 - 0.5
        return m
    if name in DL_CASES:
        return dl_case(name)
    if name.startswith("size "):
        B, n = (int(v) for v in name[5:].split("x"))
        return dl_size_case(B, n)
    return dl_size_case(3, 257, per_element_logscale=True)


def dl_masks(case):
    """boolean masks of the subsets all, lower (s < -8), centre (|s| <= 8), upper (s > 8) over the elements, from the fp64 s"""
    s = (np.floor(case["sample"] / BINSIZE) * BINSIZE - case["mean"]) / np.exp(case["logscale"])
    return {"all": np.ones(s.shape, bool), "lower": s < -8, "centre": np.abs(s) <= 8, "upper": s > 8}


def dl_fwd_errors(got_logp, got_rows, ref_logp, ref_rows, masks):
    """per subset max|got - ref| of the elementwise log-probabilities, absolute (they are O(1) .. 16); "rows": the row sums' worst
    error relative to max|ref rows|"""
    err = np.abs(np.asarray(got_logp) - ref_logp)
    out = {name: (float(err[m].max()) if m.any() else 0.0) for name, m in masks.items()}
    out["rows"] = float(np.abs(np.asarray(got_rows) - ref_rows).max() / np.abs(ref_rows).max())
    return out


def dl_fwd_bound(yard_err, key, ref_rows):
    """4 x the yardstick's error + 1e-6 per element; + one fp32 ulp of max|ref rows| (relative) on the rows"""
    floor = float(ulp32(np.abs(ref_rows).max()) / np.abs(ref_rows).max()) if key == "rows" else 1e-6
    return 4 * yard_err[key] + floor


# --------------------------------------------------------------------------------------
# diagonal Gaussian (distributions.py:5-24)
# --------------------------------------------------------------------------------------
GAUSS_NS = (1, 255, 257, 2048 * 256 + 3)                             # the last: the second trip of the elementwise stride loop
EW_NS = (1, 257, 2048 * 256 + 3)


def gauss_case(n):
    """mean, logsd (logvar = 2 logsd in [-20, 20]), noise with |noise| <= 30 (exactly +-30 among them), sample = mean + exp(logsd) noise;
    every array fp32-rounded"""
    rng = np.random.RandomState(4000 + n % 1000)
    mean, logsd = rng.standard_normal(n), rng.uniform(-10.0, 10.0, n)
    noise = rng.uniform(-30.0, 30.0, n)
    noise[::5] = rng.standard_normal(noise[::5].size)
    noise[::97] = 30.0 * np.sign(noise[::97] + 1e-30)
    mean, logsd, noise = f32(mean), f32(logsd), f32(noise)
    return dict(mean=mean, logsd=logsd, logvar=2.0 * logsd, noise=noise, sample=f32(mean + np.exp(logsd) * noise))


def fp32_yardstick_gauss_sample(mean, logvar, noise):
    """iaf_gauss_sample_kernel's expression in numpy float32, correctly rounded exp"""
    out = np.asarray(mean, F) + exp32(F(0.5) * np.asarray(logvar, F)) * np.asarray(noise, F)
    assert out.dtype == F
    return out.astype(np.float64)


def fp32_yardstick_gauss_logps(mean, logvar, sample):
    """iaf_gauss_logps_kernel's expression in numpy float32, correctly rounded exp"""
    d, lv = np.asarray(sample, F) - np.asarray(mean, F), np.asarray(logvar, F)
    out = F(-0.5) * (F(1.8378770664093453) + lv + d * d / exp32(lv))
    assert out.dtype == F
    return out.astype(np.float64)


def gauss_scales(c):
    """per element, the magnitude of the terms each output is made of: |mean| + exp(logsd) |noise| for the sample,
    (log 2 pi + |logvar| + (x - mean)^2 / exp(logvar)) / 2 for the log-density.  An error measured against these bites on every element
    over the whole range of logvar, not only on the few largest -> (sample scale, logps scale)"""
    d = c["sample"] - c["mean"]
    return (np.abs(c["mean"]) + np.exp(c["logsd"]) * np.abs(c["noise"]),
            0.5 * (np.log(2 * np.pi) + np.abs(c["logvar"]) + d * d / np.exp(c["logvar"])))


def scaled_err(got, ref, scale):
    """max over the elements of |got - ref| / scale"""
    return float((np.abs(np.asarray(got) - ref) / scale).max())


def rel_err(got, ref):
    return float(np.abs(np.asarray(got) - ref).max() / np.abs(ref).max())


# --------------------------------------------------------------------------------------
# data-dependent init (layers.py:45-51) on x_init [B, C, HW]
# --------------------------------------------------------------------------------------
DI_INIT_SCALE = 0.1
DI_CASES = {                                                         # name -> (B, C, HW, recipe)
    "1x1x1": (1, 1, 1, "plain"),                                     # variance 0
    "3x5x85": (3, 5, 85, "plain"),                                   # 255 elements per channel
    "1x2x257": (1, 2, 257, "plain"),                                 # one past the 256-thread sweep
    "4x3x250": (4, 3, 250, "plain"),                                 # 1000 elements per channel
    "large_mean": (4, 3, 250, "large"),                              # mean 100, std 0.01: the variance under cancellation
}


def di_case(name):
    """(x [B, C, HW], add [B, C, HW]), fp32-rounded"""
    B, C, HW, recipe = DI_CASES[name]
    rng = np.random.RandomState(5000 + sorted(DI_CASES).index(name))
    x = rng.standard_normal((B, C, HW))
    if recipe == "large":
        x = 100.0 + 0.01 * x
    else:
        x = x * (0.5 + np.arange(C))[None, :, None] + (np.arange(C) - 1.0)[None, :, None]
    return f32(x), f32(rng.standard_normal((B, C, HW)))


def datainit(x, add=None, init_scale=DI_INIT_SCALE):
    """fp64: per channel over (N, H, W) m, v (biased) -> scale = init_scale / sqrt(v + 1e-10), g = log(scale) / 3, b = -m scale,
    y = scale (x - m) [+ add] -> dict(mean, var, scale, g, b, y)"""
    x = np.asarray(x, np.float64)
    m = x.mean(axis=(0, 2))                                          # :46 (tf.nn.moments)
    v = ((x - m[None, :, None]) ** 2).mean(axis=(0, 2))
    scale = init_scale / np.sqrt(v + 1e-10)                          # :47
    y = scale[None, :, None] * (x - m[None, :, None])                # :50-51
    if add is not None:
        y = y + np.asarray(add, np.float64)
    return dict(mean=m, var=v, scale=scale, g=np.log(scale) / 3.0, b=-m * scale, y=y)


def fp32_datainit(x, add=None, init_scale=DI_INIT_SCALE, one_pass=False):
    """the kernel's two passes in numpy float32 (its sums are numpy's).  one_pass=True is WRONG on purpose: the variance as
    E[x^2] - mean^2.  -> the same dict, float64 holding fp32 values"""
    x = np.asarray(x, F)
    n = F(x.shape[0] * x.shape[2])
    m = np.sum(x, axis=(0, 2), dtype=F) / n
    if one_pass:
        v = np.sum(x * x, axis=(0, 2), dtype=F) / n - m * m
    else:
        dlt = x - m[None, :, None]
        v = np.sum(dlt * dlt, axis=(0, 2), dtype=F) / n
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = F(init_scale) / np.sqrt(v + F(1e-10))
        g = log32(scale) / F(3)
    y = scale[None, :, None] * (x - m[None, :, None])
    if add is not None:
        y = y + np.asarray(add, F)
    out = dict(mean=m, var=v, scale=scale, g=g, b=-m * scale, y=y)
    assert all(a.dtype == F for a in out.values())
    return {k: a.astype(np.float64) for k, a in out.items()}


def datainit_bounds(x, add=None, init_scale=DI_INIT_SCALE):
    """derived from iaf_datainit_kernel's order: each of its two sums is ceil(n / 256) additions per thread, six shuffle steps and two
    more across the waves, then one division (d = ceil(n / 256) + 9).
      mean:  e_m = (d + 2) u mean|x|
      var:   the kernel's centred sum is taken about its own mean: sum (x - m')^2 / n = v + (m - m')^2 exactly, each term carrying
             three more roundings -> e_v = (d + 5) u (v + e_m^2) + e_m^2
      scale: relative r_s = e_v / (2 (v + 1e-10)) + 4 u      (the constant, the addition, sqrt, the division)
      g:     r_s / 3 + 4 u |g|                                (logf within an ulp, the division)
      b:     scale e_m + |b| (r_s + 2 u)
      y:     scale e_m + |y - add| (r_s + 3 u) + u |y|
    -> dict(mean, var, g, b [C]; y [B, C, HW])"""
    r = datainit(x, add, init_scale)
    x = np.asarray(x, np.float64)
    n = x.shape[0] * x.shape[2]
    d = -(-n // 256) + 9
    e_m = sum_bound(d, np.abs(x).mean(axis=(0, 2)))
    e_v = (d + 5) * U * (r["var"] + e_m ** 2) + e_m ** 2
    r_s = e_v / (2 * (r["var"] + 1e-10)) + 4 * U
    y0 = r["y"] - (np.asarray(add, np.float64) if add is not None else 0.0)
    return dict(mean=e_m, var=e_v, g=r_s / 3 + 4 * U * np.abs(r["g"]), b=r["scale"] * e_m + np.abs(r["b"]) * (r_s + 2 * U),
                y=(r["scale"] * e_m)[None, :, None] + np.abs(y0) * (r_s[None, :, None] + 3 * U) + U * np.abs(r["y"]))


# --------------------------------------------------------------------------------------
# the elementwise kernels of the init pass that call the hardware exponential
# --------------------------------------------------------------------------------------
EXP_X_MAX = 8.0


def hw_exp_bound(x, ref):
    """(4 + |x|) 2^-23 |ref|, elementwise, x the exponent's argument.  exp(x) = exp2(x log2 e): the exp2 instruction is good to one ulp
    (2^-23 relative), and the rounding of x log2 e (2^-24 relative in the ARGUMENT) is |x| 2^-24 relative in the result; x itself is a
    rounded product or sum (another |x| 2^-24) and the fp32 constant log2 e is 0.22 2^-24 off.  The factor in front, a difference of
    fp32 inputs built without cancellation (see the generators: its subtrahend is at most half the minuend), carries at most
    2^-23, and the final product 2^-24: (2.5 + 1.11 |x|) 2^-23 in all, inside (4 + |x|) 2^-23 for |x| <= 13."""
    return (4.0 + np.abs(x)) * 2.0 ** -23 * np.abs(ref)


AFFINE_SCALE = float(np.float32(0.1))                                # tf_train.py:70-71; what the kernel receives of 0.1


def affine_case(n):
    """z, m, s with |scale s| <= 8 and |z| >= 2 |scale m| (both signs): z - scale m does not cancel"""
    rng = np.random.RandomState(6000 + n % 1000)
    m, s = 3.0 * rng.standard_normal(n), rng.uniform(-79.0, 79.0, n)
    z = rng.choice([-1.0, 1.0], n) * (2.0 * np.abs(AFFINE_SCALE * m) + 0.01 + np.abs(rng.standard_normal(n)))
    return f32(z), f32(m), f32(s)


def affine_transform(z, m, s, scale=AFFINE_SCALE):
    """fp64: (z - scale m) / exp(scale s) (tf_train.py:70-71) -> (out, the exponent's argument -scale s)"""
    z, m, s = (np.asarray(a, np.float64) for a in (z, m, s))
    return (z - scale * m) / np.exp(scale * s), -scale * s


def noise_case(n):
    """z, qm, ql, rm, rl with |ql + rl| <= 8, qm and rm of one sign per element, |z| >= 2 |qm + rm| (both signs)"""
    rng = np.random.RandomState(7000 + n % 1000)
    sgn = rng.choice([-1.0, 1.0], n)
    qm, rm = sgn * np.abs(rng.standard_normal(n)), sgn * np.abs(rng.standard_normal(n))
    ql, rl = rng.uniform(-3.9, 3.9, n), rng.uniform(-3.9, 3.9, n)
    z = rng.choice([-1.0, 1.0], n) * (2.0 * np.abs(qm + rm) + 0.01 + np.abs(rng.standard_normal(n)))
    return tuple(f32(a) for a in (z, qm, ql, rm, rl))


def noise_from_sample(z, qm, ql, rm, rl):
    """fp64: eps' with (qm + rm) + exp(ql + rl) eps' = z -> (eps', the exponent's argument -(ql + rl))"""
    z, qm, ql, rm, rl = (np.asarray(a, np.float64) for a in (z, qm, ql, rm, rl))
    return (z - (qm + rm)) * np.exp(-(ql + rl)), -(ql + rl)


def ew_case(n, count, seed):
    """`count` fp32-rounded N(0, 1) arrays of n elements"""
    rng = np.random.RandomState(8000 + seed + n % 1000)
    return [f32(rng.standard_normal(n)) for _ in range(count)]
