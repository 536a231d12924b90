"""numpy statement of the device dataset's definition (include/iaf_hip.h, iaf_data_next_batch): which image sits in which
row of which batch.  Built on noise_reference.philox4x32_10; what the device gather is tested against."""
import numpy as np

from noise_reference import philox4x32_10

KEY_XOR = (0x61746164, 0x5F666169)


def half_width(n):
    """w: half the bit width of the Feistel domain [0, 4^w) that covers [0, n)"""
    return max(1, (int(n - 1).bit_length() + 1) // 2)


def perm(j, n, seed, epoch, count=None):
    """perm_e(j) for an array of slots j < n (epoch: an int, or an array of j's shape): the 4-round Feistel pass, repeated on the entries
    that are still >= n.  count: an int64 array of j's size that receives each entry's number of passes"""
    y = np.atleast_1d(np.asarray(j)).astype(np.uint64).ravel()
    assert 1 <= n < 1 << 32 and (y < n).all()
    if n == 1:
        return np.zeros(y.shape, np.int64)
    e = np.broadcast_to(np.asarray(epoch, dtype=np.uint64).ravel(), y.shape)
    e_lo, e_hi = e & np.uint64(0xffffffff), e >> np.uint64(32)
    w = np.uint64(half_width(n))
    mask = np.uint64((1 << int(w)) - 1)
    key = ((seed & 0xffffffff) ^ KEY_XOR[0], (seed >> 32) ^ KEY_XOR[1])
    y = y.copy()
    todo = np.arange(y.size)
    while todo.size:
        v = y[todo]
        L, R = v >> w, v & mask
        for r in range(4):
            f = philox4x32_10((R, r, e_lo[todo], e_hi[todo]), key)[0].astype(np.uint64) & mask
            L, R = R, L ^ f
        y[todo] = (L << w) | R
        if count is not None:
            count[todo] += 1
        todo = todo[y[todo] >= np.uint64(n)]
    return y.astype(np.int64)


def batches_per_epoch(n, B, world=1):
    G = B * world
    assert 1 <= G <= n
    return n // G


def batch_indices(n, seed, step, B, rank=0, world=1, deterministic=False):
    """the image indices (int64 [B]) of rank `rank`'s batch at step `step`"""
    G = B * world
    bpe = batches_per_epoch(n, B, world)
    e, j0 = step // bpe, (step % bpe) * G + rank * B
    j = np.arange(j0, j0 + B, dtype=np.int64)
    return j if deterministic else perm(j, n, seed, e)


def epoch_order(n, seed, epoch):
    """perm_e(0 .. n-1)"""
    return perm(np.arange(n), n, seed, epoch)


def chi2_quantile(p, k):
    """the p-quantile of chi-square with k degrees of freedom by Wilson-Hilferty; the normal quantile by bisection on erf"""
    from math import erf, sqrt
    lo, hi = -10.0, 10.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * (1.0 + erf(mid / sqrt(2.0))) < p:
            lo = mid
        else:
            hi = mid
    z = 0.5 * (lo + hi)
    return k * (1.0 - 2.0 / (9.0 * k) + z * sqrt(2.0 / (9.0 * k))) ** 3
