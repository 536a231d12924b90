"""GPU tests of the state snapshot's launch alone (include/iaf_hip.h: iaf_state_snapshot, csrc/iaf_kernels_data.hpp): the copy held to
torch.equal on the words and the digest to the numpy restatement (tests/state_reference.py), bit for bit -- at the sizes around the
16-byte pieces and the workgroup, at every relative alignment of source and destination, without a destination, with eight parts in one
launch, on bit patterns no float compare would pass, inside a replayed graph; the error codes; the kernel's resources."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import state_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 3, 4, 5, 63, 64, 65, 1000003]
CANARY = 0x5A5A5A5A
GUARD = 16                                            # words: 64 bytes


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()
    return iaf_amd


@pytest.fixture(scope="module")
def words():
    """the reference input, made once: random 32-bit words (as int32), shared and never written"""
    w = np.random.RandomState(7).randint(0, 1 << 32, size=max(SIZES) + 8, dtype=np.uint64).astype(np.uint32)
    return w


def dev_words(w, offset_words=0):
    """the words in device memory, `offset_words` 32-bit words behind a 256-byte boundary"""
    base = torch.zeros(offset_words + w.size, dtype=torch.int32, device="cuda")
    assert base.data_ptr() % 256 == 0
    view = base[offset_words:]
    view.copy_(torch.from_numpy(w.view(np.int32).copy()))
    return view


def guarded(n, offset_words=0):
    """a destination of n words with a guard band in front of it and behind it, everything canary"""
    buf = torch.full((GUARD + offset_words + n + GUARD,), CANARY, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf, buf[GUARD + offset_words:GUARD + offset_words + n]


def bands_intact(buf, n, offset_words=0):
    lo = GUARD + offset_words
    return bool((buf[:lo] == CANARY).all()) and bool((buf[lo + n:] == CANARY).all())


def snapshot(amd, parts, digests=None):
    """parts: (src tensor, dst tensor or None); returns the digests as Python ints (synchronises)"""
    capi = amd._capi
    table = (capi.StatePart * len(parts))(*[capi.StatePart(s.data_ptr(), None if d is None else d.data_ptr(), s.numel() * s.element_size())
                                            for s, d in parts])
    if digests is None:
        digests = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    got = capi.lib().iaf_state_snapshot(table, len(parts), ctypes.c_void_p(digests.data_ptr()),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert got == capi.IAF_OK, got
    torch.cuda.synchronize()
    return [int(v) & R.M64 for v in digests.cpu().tolist()][:len(parts)]


# (source offset, destination offset) in words behind a 16-byte boundary: both aligned; both one word off (congruent, misaligned to 16);
# only the destination off (the dword stores); the source off and the destination aligned
ALIGNMENTS = [(0, 0), (1, 1), (0, 1), (3, 0)]


@pytest.mark.parametrize("so,do", ALIGNMENTS, ids=["aligned", "both+4", "dst+4", "src+12"])
@pytest.mark.parametrize("n", SIZES)
def test_one_part_copy_and_digest(amd, words, n, so, do):
    w = words[:n]
    src = dev_words(w, so)
    assert src.data_ptr() % 16 == 4 * so
    buf, dst = guarded(n, do)
    assert dst.data_ptr() % 16 == 4 * do
    (d,) = snapshot(amd, [(src, dst)])
    assert d == R.digest(w), (hex(d), hex(R.digest(w)))
    assert torch.equal(dst, src) and np.array_equal(dst.cpu().numpy().view(np.uint32), w)
    assert bands_intact(buf, n, do)


@pytest.fixture(scope="module")
def many_words():
    return np.random.RandomState(8).randint(0, 1 << 32, size=13000003, dtype=np.uint64).astype(np.uint32)


# A lane loads its pieces in rounds of four on two register sets in turn, and a launch has at most 256 workgroups of 1024 lanes: only a part
# beyond 256 * 1024 * 16 words gives a lane more than one round.  9000001 words: two rounds (the loop ends behind the second set), then single
# pieces; 13000003: three (it ends behind the first set again), then single pieces.  Co-aligned and with the dword stores.
@pytest.mark.parametrize("so,do", [(1, 1), (0, 3)], ids=["both+4", "dst+12"])
@pytest.mark.parametrize("n", [9000001, 13000003])
def test_a_part_large_enough_for_several_rounds_per_lane(amd, many_words, n, so, do):
    w = many_words[:n]
    src = dev_words(w, so)
    buf, dst = guarded(n, do)
    (d,) = snapshot(amd, [(src, dst)])
    assert d == R.digest(w), (hex(d), hex(R.digest(w)))
    assert torch.equal(dst, src)
    assert bands_intact(buf, n, do)


def test_known_answers(amd):
    for w, want in ((np.zeros(1, np.uint32), 0x9e3779b1), (np.arange(5, dtype=np.uint32), 0x6b69628af),
                    (np.full(5, 0xFFFFFFFF, np.uint32), 0x736ae24900000000),
                    (np.random.RandomState(0).standard_normal(1000003).astype(np.float32).view(np.uint32), 0xc09b49ea2da1ee6d)):
        assert snapshot(amd, [(dev_words(w), None)]) == [want]


@pytest.mark.parametrize("n", SIZES)
def test_without_a_destination_nothing_is_written(amd, words, n):
    w = words[:n]
    src = dev_words(w, 2)
    canary = torch.full((4096,), CANARY, dtype=torch.int32, device="cuda")
    (d,) = snapshot(amd, [(src, None)])
    assert d == R.digest(w)
    assert np.array_equal(src.cpu().numpy().view(np.uint32), w)               # the source is only read
    assert bool((canary == CANARY).all())


def test_eight_parts_of_mixed_sizes_in_one_launch(amd, words):
    sizes = [1, 2, 100003, 5, 64, 4099, 2, 1]                                  # 4- and 8-byte parts among large ones
    offs = [(0, 0), (1, 1), (2, 2), (0, 3), (3, 3), (1, 0), (0, 0), (3, 1)]
    parts, bufs, lo = [], [], 0
    for n, (so, do) in zip(sizes, offs):
        src = dev_words(words[lo:lo + n], so)
        buf, dst = guarded(n, do)
        parts.append((src, dst))
        bufs.append((buf, n, do, words[lo:lo + n]))
        lo += 7
    got = snapshot(amd, parts)
    for p, (buf, n, do, w) in enumerate(bufs):
        assert got[p] == R.digest(w), p
        assert np.array_equal(parts[p][1].cpu().numpy().view(np.uint32), w), p
        assert bands_intact(buf, n, do), p


def test_bit_patterns_travel_exactly(amd):
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF800000, 0x7F800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF,
                        0xFFFFFFFF, 0x7F7FFFFF, 0x00800000], dtype=np.uint32)   # NaN payloads, infinities, -0.0, subnormals, all ones
    w = np.tile(special, 50)[:517]
    src = dev_words(w, 1).view(torch.float32)
    buf, dst = guarded(w.size, 1)
    (d,) = snapshot(amd, [(src, dst.view(torch.float32))])
    assert d == R.digest(w) == R.digest_ints(w)
    assert np.array_equal(dst.cpu().numpy().view(np.uint32), w)
    assert bands_intact(buf, w.size, 1)


def test_a_replayed_graph_leaves_the_digest_of_what_that_replay_read(amd, words):
    capi = amd._capi
    sizes = [70001, 2, 1]
    srcs = [dev_words(words[:n], o) for n, o in zip(sizes, (1, 0, 3))]
    dsts = [guarded(n, o) for n, o in zip(sizes, (1, 2, 3))]
    digests = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    table = (capi.StatePart * 3)(*[capi.StatePart(s.data_ptr(), d.data_ptr(), 4 * n) for s, (_, d), n in zip(srcs, dsts, sizes)])

    def launch():
        assert capi.lib().iaf_state_snapshot(table, 3, ctypes.c_void_p(digests.data_ptr()),
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == capi.IAF_OK
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                               # eager warm-up on the capture stream
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    torch.cuda.current_stream().wait_stream(side)
    for i in range(3):                                                         # the table went by value: nothing of it is read at replay
        table[i].src, table[i].dst, table[i].bytes = 0, 0, 0
    for shift in (11, 23):
        fresh = [words[shift:shift + n] for n in sizes]
        for s, f in zip(srcs, fresh):
            s.copy_(torch.from_numpy(f.view(np.int32).copy()))
        g.replay()
        torch.cuda.synchronize()
        got = [int(v) & R.M64 for v in digests.cpu().tolist()]
        for p, f in enumerate(fresh):
            assert got[p] == R.digest(f), (shift, p)
            assert np.array_equal(dsts[p][1].cpu().numpy().view(np.uint32), f), (shift, p)
    del g


def test_error_codes_come_before_any_launch(amd):
    capi = amd._capi
    lib = capi.lib()
    src = torch.arange(16, dtype=torch.int32, device="cuda")
    dst = torch.full((16,), CANARY, dtype=torch.int32, device="cuda")
    digests = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    dp, st = ctypes.c_void_p(digests.data_ptr()), None
    one = lambda s, d, n: (capi.StatePart * 1)(capi.StatePart(s, d, n))
    good = one(src.data_ptr(), dst.data_ptr(), 64)
    assert lib.iaf_state_snapshot(None, 1, dp, st) == capi.IAF_ERR_NULL
    assert lib.iaf_state_snapshot(good, 1, None, st) == capi.IAF_ERR_NULL
    assert lib.iaf_state_snapshot(one(None, dst.data_ptr(), 64), 1, dp, st) == capi.IAF_ERR_NULL
    for n_parts in (0, -1, 9):
        assert lib.iaf_state_snapshot((capi.StatePart * 9)(*[good[0]] * 9), n_parts, dp, st) == capi.IAF_ERR_SHAPE
    for nbytes in (0, 2, 6, 63):
        assert lib.iaf_state_snapshot(one(src.data_ptr(), dst.data_ptr(), nbytes), 1, dp, st) == capi.IAF_ERR_SHAPE
    two = (capi.StatePart * 2)(good[0], capi.StatePart(src.data_ptr(), None, 0))          # a bad second part refuses the whole call
    assert lib.iaf_state_snapshot(two, 2, dp, st) == capi.IAF_ERR_SHAPE
    assert lib.iaf_state_snapshot(one(src.data_ptr() + 2, dst.data_ptr(), 8), 1, dp, st) == capi.IAF_ERR_WORKSPACE
    assert lib.iaf_state_snapshot(good, 1, ctypes.c_void_p(digests.data_ptr() + 4), st) == capi.IAF_ERR_WORKSPACE
    p = ctypes.c_void_p()
    for fn in ("iaf_rng_step_ptr", "iaf_data_step_ptr", "iaf_skip_counter_ptr"):
        assert getattr(lib, fn)(None, ctypes.byref(p)) == capi.IAF_ERR_NULL
    torch.cuda.synchronize()
    assert bool((dst == CANARY).all()) and bool((digests == -1).all())        # no refused call launched anything


def test_the_getters_point_at_the_counters(amd):
    capi = amd._capi
    src = amd.NoiseSource(5)
    ds = amd.DeviceDataset(torch.zeros(4, 3, 2, 2, dtype=torch.uint8, device="cuda"), 5)
    src.seek((1 << 40) + 3)
    ds.seek(9)
    p, q = ctypes.c_void_p(), ctypes.c_void_p()
    assert capi.lib().iaf_rng_step_ptr(src._h, ctypes.byref(p)) == capi.IAF_OK and p.value
    assert capi.lib().iaf_data_step_ptr(ds._h, ctypes.byref(q)) == capi.IAF_OK and q.value
    assert capi.lib().iaf_rng_step_ptr(src._h, None) == capi.IAF_ERR_NULL
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    table = (capi.StatePart * 2)(capi.StatePart(p.value, out.data_ptr(), 8), capi.StatePart(q.value, out.data_ptr() + 8, 8))
    digests = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert capi.lib().iaf_state_snapshot(table, 2, ctypes.c_void_p(digests.data_ptr()),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == capi.IAF_OK
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    assert int(got[0]) == (1 << 40) + 3 and int(got[1]) == 9
    assert src.tell() == (1 << 40) + 3 and ds.tell() == 9                      # reading moved nothing


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_snapshot_kernel_uses_no_scratch(tmp_path):
    """hipcc's kernel-resource-usage remarks (device code only) of a unit that includes just the headers the kernel lives in: registers
    only, and no LDS beyond the block reduction's (one 64-bit sum per wave of a 1024-lane workgroup: 128 bytes)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    src = tmp_path / "state_kernels.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include "iaf_hip.h"\n#include "iaf_kernels_rng.hpp"\n'
                   '#include "iaf_kernels_data.hpp"\n')
    rows = [r for r in kr.unit_resources(str(src), str(tmp_path / "state_kernels.o"), []) if "state_snapshot" in r["name"]]
    assert len(rows) == 1, [r["name"] for r in rows]
    r = rows[0]
    assert not r.get("scratch", 0) and not r.get("vspill", 0) and not r.get("sspill", 0), r
    assert r.get("lds", 128) <= 128, r
