"""torch-fp64 statements of the backward operations of the model's two ends (iaf_amd/csrc/iaf_kernels_edge.hpp), written from the
reference's lines as oracle/iaf_grad_oracle.py:cvae1_obj restates them (tf_train.py:183, 206-211; tf_utils/layers.py:56-60, 67-80,
104-111; tf_utils/distributions.py:28-32) and differentiated by autograd; a plain fp32 restatement of the likelihood's gradient that
the device kernel's error is measured against; and the seed-fixed inputs of the likelihood cases, so that the CPU test of the
yardstick and the GPU test of the kernel see the same numbers.  What tests/test_hip_model_edge_backward.py compares the kernels
with; pinned by tests/test_model_edge_reference.py.  Does not import the GPU library."""
import numpy as np
import torch
import torch.nn.functional as F

BINSIZE = 1 / 256.0


def _t(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
    return t.requires_grad_(True) if grad else t


def f32(a):
    """what the device holds of `a`, as float64"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def same_pad(n, k, s):
    """TF "SAME": out = ceil(n / s), total padding max((out - 1) s + k - n, 0), the smaller half first -> (out, before, after)"""
    out = -(-n // s)
    tot = max((out - 1) * s + k - n, 0)
    return out, tot // 2, tot - tot // 2


# --------------------------------------------------------------------------------------
# discretized logistic (distributions.py:28-32) behind clip_by_value (tf_train.py:208)
# --------------------------------------------------------------------------------------
def dl_s(mean, logscale, sample, binsize=BINSIZE):
    """s = (floor(x / b) b - mean) / scale in fp64 (mean: the value the likelihood sees, i.e. after the clip)"""
    mean, sample = np.asarray(mean, np.float64), np.asarray(sample, np.float64)
    return (np.floor(sample / binsize) * binsize - mean) / np.exp(float(logscale))


def dl_backward(pre_clip_mean, logscale, sample, lo, hi, up, binsize=BINSIZE):
    """autograd of up * sum log(sig(s + b/scale) - sig(s) + 1e-7) through torch.clamp(mean, lo, hi) (no clip when not lo < hi):
    -> d_mean (shape of the mean), d_logscale per row [B] (rows = the first axis)"""
    m = _t(pre_clip_mean, True)
    x = _t(sample)
    B = m.shape[0]
    ls = torch.full((B,), float(logscale), dtype=torch.float64, requires_grad=True)     # one copy per row: per-row gradients
    xo = torch.clamp(m, lo, hi) if lo < hi else m
    scale = torch.exp(ls).reshape([B] + [1] * (m.dim() - 1))
    s = (torch.floor(x / binsize) * binsize - xo) / scale
    logp = torch.log(torch.sigmoid(s + binsize / scale) - torch.sigmoid(s) + 1e-7)
    (up * logp.sum()).backward()
    return m.grad.numpy(), ls.grad.numpy()


def fp32_yardstick_dl_backward(pre_clip_mean, logscale, sample, lo, hi, up, binsize=BINSIZE):
    """The same gradient in numpy float32 with correctly rounded exp, in the mirrored form: e = exp(-|u|) gives sig(|u|) = 1 / (1 + e)
    and sig(-|u|) = e / (1 + e) each directly, sig'(u) = sig(u) sig(-u), and P - 1e-7 = sig(-s) - sig(-t) where s > 0 (both terms
    small), sig(t) - sig(s) elsewhere.  Every operation rounds to fp32; the row sum is numpy's."""
    f = np.float32
    m0 = np.asarray(pre_clip_mean, dtype=f)
    x = np.asarray(sample, dtype=f)
    clip = lo < hi
    m = np.minimum(np.maximum(m0, f(lo)), f(hi)) if clip else m0
    passes = (m0 > f(lo)) & (m0 < f(hi)) if clip else np.ones(m0.shape, bool)
    b = f(binsize)
    inv = f(1) / np.exp(f(logscale))
    s = (np.floor(x / b) * b - m) * inv
    t = s + b * inv
    es, et = np.exp(-np.abs(s)), np.exp(-np.abs(t))
    rs, rt = f(1) / (f(1) + es), f(1) / (f(1) + et)
    lo_s, lo_t = es * rs, et * rt                                   # sig(-|s|), sig(-|t|)
    sig_s, sig_t = np.where(s >= 0, rs, lo_s), np.where(t >= 0, rt, lo_t)
    diff = np.where(s > 0, lo_s - lo_t, sig_t - sig_s)
    P = diff + f(1e-7)
    ds, dt = lo_s * rs, lo_t * rt
    d_mean = np.where(passes, f(up) * (-(dt - ds) * inv / P), f(0))
    rows = f(up) * np.sum(((-t * dt + s * ds) / P).reshape(m0.shape[0], -1), axis=1, dtype=f)
    assert d_mean.dtype == f and rows.dtype == f
    return d_mean.astype(np.float64), rows.astype(np.float64)


# the likelihood cases of the GPU test: name -> (recipe, logscale, n_per_row)
DL_B = 2
DL_UP = -1.0
DL_CLIP = (-0.5 + 1 / 512.0, 0.5 - 1 / 512.0)                       # tf_train.py:208; both exact in fp32
DL_CASES = {
    "centre_0": ("centre", 0.0, 3 * 8 * 8),
    "centre_-1.3": ("centre", -1.3, 3 * 8 * 8),
    "centre_-2": ("centre", -2.0, 3 * 8 * 8),
    "centre_-3": ("centre", -3.0, 3 * 8 * 8),
    "centre_-2_n193": ("centre", -2.0, 193),                        # a row that is no multiple of 256 or of 4
    "tails_-4": ("tails", -4.0, 3 * 8 * 8),
    "tails_-5": ("tails", -5.0, 3 * 8 * 8),
    "clip_-2": ("clip", -2.0, 3 * 8 * 8),
}
DL_SUBSETS = ("all", "lower", "centre", "upper")                    # s < -8, |s| <= 8, s > 8 (s of the fp64 reference)


def dl_case(name):
    """seed-fixed inputs of one case, every array already rounded to fp32 (held as float64):
    dict(k, sample, pre_clip_mean, mean (what the kernel receives), logscale, lo, hi (0, 0: no clip), n_per_row)"""
    recipe, logscale, n = DL_CASES[name]
    rng = np.random.RandomState(1000 + sorted(DL_CASES).index(name))
    k = rng.randint(0, 256, size=(DL_B, n))
    sample = (k + 0.5) / 256.0 - 0.5                                 # exact in fp32
    noise = rng.standard_normal((DL_B, n))
    lo = hi = 0.0
    if recipe == "centre":
        pre = f32(sample + 0.15 * noise)
        mean = pre
    elif recipe == "tails":
        pre = f32(np.clip(sample + 0.3 * noise, -0.6, 0.6))
        mean = pre
    else:
        lo, hi = DL_CLIP
        pre = f32(sample + 0.2 * noise)
        mean = np.clip(pre, lo, hi)                                  # the kernel receives the clipped means (as x_dec's clip hands them on)
    assert np.array_equal(f32(sample), sample) and np.array_equal(f32(mean), mean)
    return dict(k=k, sample=sample, pre_clip_mean=pre, mean=mean, logscale=logscale, lo=lo, hi=hi, n_per_row=n)


def dl_mirrored(case):
    """the same case reflected about the bin grid: (255 - k, -mean).  s -> -t, t -> -s: d_mean negated, d_logscale equal."""
    c = dict(case)
    c["k"] = 255 - case["k"]
    c["sample"] = (c["k"] + 0.5) / 256.0 - 0.5
    c["pre_clip_mean"], c["mean"] = -case["pre_clip_mean"], -case["mean"]
    c["lo"], c["hi"] = -case["hi"], -case["lo"]
    return c


def dl_subsets(case):
    """boolean masks of DL_SUBSETS over the elements, from the fp64 s"""
    s = dl_s(case["mean"], case["logscale"], case["sample"])
    return {"all": np.ones(s.shape, bool), "lower": s < -8, "centre": np.abs(s) <= 8, "upper": s > 8}


def dl_errors(got_d_mean, got_rows, ref_d_mean, ref_rows, masks):
    """the measure of the likelihood checks: per subset max|got - ref| over the subset / max|ref| over the WHOLE tensor (0 for an
    empty subset), and the same for the row sums under the key "rows" """
    den = np.abs(ref_d_mean).max()
    err = np.abs(np.asarray(got_d_mean) - ref_d_mean)
    out = {name: (float(err[m].max() / den) if m.any() else 0.0) for name, m in masks.items()}
    out["rows"] = float(np.abs(np.asarray(got_rows) - ref_rows).max() / np.abs(ref_rows).max())
    return out


# --------------------------------------------------------------------------------------
# x_enc / x_dec: filter gradient, weight norm, transposed conv
# --------------------------------------------------------------------------------------
def convk_wgrad(x, dy, kh, kw, stride, elu_x, elu_dy):
    """d <conv2d_SAME([elu] x; w, stride), [elu] dy> / d w in the layout [kh, kw, n_small, n_big] (x [B, n_small, H, W],
    dy [B, n_big, ceil(H/s), ceil(W/s)]); SAME padding written out"""
    xt, dt = _t(x), _t(dy)
    if elu_x:
        xt = F.elu(xt)
    if elu_dy:
        dt = F.elu(dt)
    _, pt, pb = same_pad(xt.shape[2], kh, stride)
    _, pl, pr = same_pad(xt.shape[3], kw, stride)
    w = torch.zeros((dt.shape[1], xt.shape[1], kh, kw), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), w, stride=stride)
    assert y.shape == dt.shape, (y.shape, dt.shape)
    (y * dt).sum().backward()
    return w.grad.permute(2, 3, 1, 0).contiguous().numpy()


def weightnorm_weights(V, g, deconv):
    """w = exp(g) V / sqrt(clamp(sum V^2, 1e-12)) on torch tensors: conv V [kh, kw, n_in, n_out], deconv V [kh, kw, n_out, n_in]; the sum
    runs over the first three axes in both (per output channel of a conv, per INPUT channel of a deconv); g [n_out]"""
    gain = torch.exp(g).reshape(1, 1, -1, 1) if deconv else torch.exp(g).reshape(1, 1, 1, -1)
    return gain * V / torch.sqrt(torch.clamp((V * V).sum(dim=(0, 1, 2), keepdim=True), min=1e-12))


def weightnorm_backward(V, g, dW, deconv):
    """(dV, dg) of <dW, w(V, g)>"""
    Vt, gt = _t(V, True), _t(g, True)
    (weightnorm_weights(Vt, gt, deconv) * _t(dW)).sum().backward()
    return Vt.grad.numpy(), gt.grad.numpy()


def deconvk(x, w, stride):
    """conv2d_transpose(SAME, stride) with the raw filter w [kh, kw, n_out, n_in]: F.conv_transpose2d cropped to H s x W s, starting at
    the SAME pad_before of the conv it transposes"""
    xt, wt = _t(x), _t(w)
    kh, kw = wt.shape[0], wt.shape[1]
    oh, ow = xt.shape[2] * stride, xt.shape[3] * stride
    full = F.conv_transpose2d(xt, wt.permute(3, 2, 0, 1), stride=stride)
    _, pt, _ = same_pad(oh, kh, stride)
    _, pl, _ = same_pad(ow, kw, stride)
    full = F.pad(full, (0, max(pl + ow - full.shape[3], 0), 0, max(pt + oh - full.shape[2], 0)))
    return full[:, :, pt:pt + oh, pl:pl + ow].contiguous().numpy()
