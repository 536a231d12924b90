"""numpy (fp64) statement of the engine's noise definition (include/iaf_hip.h, iaf_rng_fill_normal): Philox4x32-10
counters -> two Box-Muller pairs per counter.  What the device fill is tested against."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars), key: two ints -> four uint32 arrays"""
    c = [np.atleast_1d(np.asarray(v)).astype(np.uint64) & MASK for v in ctr]
    n = max(v.size for v in c)
    c = [np.broadcast_to(v, (n,)).copy() for v in c]
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return [v.astype(np.uint32) for v in c]


def normals(seed, substream, step, count, scale=1.0, first=0):
    """elements first .. first+count-1 of the tensor filled with (seed, substream, step, scale), as float64"""
    i = np.arange(first, first + count, dtype=np.uint64)
    q, m = i // np.uint64(4), (i % np.uint64(4)).astype(np.int64)
    uq, inv = np.unique(q, return_inverse=True)
    x = philox4x32_10((uq, substream, step & 0xffffffff, step >> 32), (seed & 0xffffffff, seed >> 32))
    z = np.empty((4, uq.size))
    for a in (0, 1):
        u1 = ((x[2 * a] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (x[2 * a + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        z[2 * a], z[2 * a + 1] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
    return float(scale) * z[m, inv]


def statistics(z, others=()):
    """the figures the tests bound: mean, variance, skewness, kurtosis (each in units of its standard error), the Kolmogorov-Smirnov
    distance times sqrt(N), and sqrt(N) |mean(z z')| against the lag-1 shift and every array of `others`"""
    from math import sqrt
    import torch
    z = np.asarray(z, np.float64)
    n = z.size
    mu, d = z.mean(), z - z.mean()
    var = (d ** 2).mean()
    out = [abs(mu) * sqrt(n), abs(var - 1) * sqrt(n / 2), abs((d ** 3).mean() / var ** 1.5) * sqrt(n / 6),
           abs((d ** 4).mean() / var ** 2 - 3) * sqrt(n / 24)]
    s = np.sort(z)
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(s / sqrt(2.0))).numpy())
    k = np.arange(1, n + 1) / n
    out.append(max(np.abs(cdf - k).max(), np.abs(cdf - (k - 1.0 / n)).max()) * sqrt(n))
    out.append(sqrt(n - 1) * abs((z[1:] * z[:-1]).mean()))
    out += [sqrt(n) * abs((z * np.asarray(o, np.float64)).mean()) for o in others]
    return out


# -- what the CPU and the GPU tests share: the known answers of include/iaf_hip.h and the statistics bounds ------------------------------
KA1 = [0.9911375, -0.9246628, -0.6176091, -0.4820683, -0.1536381, 0.1808259, 0.8317351, 0.1974396]
KA2 = [2.3193574, -0.1994520, 1.3097198, -0.1905390, 0.1468710, 0.3309184]
KA2_ARGS = dict(seed=0x0123456789abcdef, substream=7, step=(1 << 32) + 5)
STAT = dict(seed=12345, substream=3, step=9, N=1 << 22)
# mean, variance, skewness, kurtosis (standard errors), KS distance * sqrt(N), correlations with lag 1 / substream + 1 / step + 1
STAT_BOUNDS = [4.0, 4.0, 4.0, 4.0, 1.95, 4.0, 4.0, 4.0]


def check_statistics(z, figures=None):
    """the bounds of the issue on a sample z of (STAT); prints each figure before it asserts"""
    N = STAT["N"]
    others = [normals(STAT["seed"], STAT["substream"] + 1, STAT["step"], N), normals(STAT["seed"], STAT["substream"], STAT["step"] + 1, N)]
    got = statistics(z, others)
    print("noise statistics (mean var skew kurt ks lag1 substream step):", " ".join("%.3f" % v for v in got))
    if figures is not None:
        figures.extend(got)
    for v, b in zip(got, STAT_BOUNDS):
        assert v < b, (got, STAT_BOUNDS)
