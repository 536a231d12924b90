"""The checkpoint's definitions restated for the tests, from the format's description (include/iaf_hip.h) and not from
iaf_amd/checkpoint.py: the digest in numpy and in plain Python integers, and a reader and a writer of the file.

Digest of 32-bit words w_0 .. w_{n-1}:  k_i = ((2 i + 1) * 0x9E3779B1) mod 2^32;  digest = sum_i (w_i + 1) * k_i mod 2^64, (w_i + 1) in 64 bits.
File, little endian: b"IAFCKPT1", u64 header length, UTF-8 JSON header, then params, slot_m, slot_v, ema raw, each at the next 64-byte boundary."""
import json
import struct

import numpy as np

GOLD = 0x9E3779B1
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
NAMES = ("params", "slot_m", "slot_v", "ema")


def words_of(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype="<u4")


def digest_ints(a):
    """plain Python integers (small inputs)"""
    d = 0
    for i, w in enumerate(words_of(a).tolist()):
        d = (d + (w + 1) * (((2 * i + 1) * GOLD) & M32)) & M64
    return d


def digest(a):
    """numpy; the 64-bit products are split into 32-bit halves so that nothing relies on wrap-around of an overflowing multiply"""
    w = words_of(a).astype(np.uint64)
    n = w.size
    if n == 0:
        return 0
    i = np.arange(n, dtype=np.uint64)
    k = ((2 * i + 1) * np.uint64(GOLD)) & np.uint64(M32)          # (2n+1) * GOLD < 2^64 for n < 2^31
    lo = (w & np.uint64(0xFFFF)) * k                                # < 2^48 each
    hi = (w >> np.uint64(16)) * k                                   # < 2^48 each; weight 2^16
    s_lo, s_hi, s_k = 0, 0, 0
    for a0 in range(0, n, 1 << 15):                                 # 2^15 terms below 2^48: sums below 2^63
        s_lo += int(lo[a0:a0 + (1 << 15)].sum(dtype=np.uint64))
        s_hi += int(hi[a0:a0 + (1 << 15)].sum(dtype=np.uint64))
        s_k += int(k[a0:a0 + (1 << 15)].sum(dtype=np.uint64))
    return (s_lo + (s_hi << 16) + s_k) & M64


def _align(n):
    return (n + 63) // 64 * 64


def write(path, meta, arrays):
    """arrays: the four flat fp32 arrays in NAMES order"""
    head = json.dumps(meta).encode("utf-8")
    blob = bytearray(b"IAFCKPT1" + struct.pack("<Q", len(head)) + head)
    for a in arrays:
        blob += b"\0" * (_align(len(blob)) - len(blob))
        blob += np.ascontiguousarray(a, dtype="<f4").tobytes()
    with open(path, "wb") as f:
        f.write(bytes(blob))


def offsets(path):
    """(header dict, {name: (byte offset, byte count)})"""
    blob = open(path, "rb").read()
    assert blob[:8] == b"IAFCKPT1"
    (hlen,) = struct.unpack("<Q", blob[8:16])
    meta = json.loads(blob[16:16 + hlen].decode("utf-8"))
    nb, off, out = 4 * meta["layout"]["total_words"], 16 + hlen, {}
    for k in NAMES:
        off = _align(off)
        out[k] = (off, nb)
        off += nb
    assert off <= len(blob)
    return meta, out


def read(path):
    """(header dict, {name: flat fp32 array})"""
    meta, offs = offsets(path)
    blob = open(path, "rb").read()
    return meta, {k: np.frombuffer(blob[o:o + nb], dtype="<f4").copy() for k, (o, nb) in offs.items()}


def views(arr, meta):
    out = {}
    for v in meta["layout"]["variables"]:
        n = int(np.prod(v["shape"])) if v["shape"] else 1
        out[v["name"]] = arr[v["offset"]:v["offset"] + n].reshape(v["shape"])
    return out
