"""GPU tests of the device noise source (include/iaf_hip.h: iaf_rng_*, iaf_amd.NoiseSource, csrc/iaf_kernels_rng.hpp) against the numpy
statement of its definition (tests/noise_reference.py): values, independence of list / chunking / alignment, the step counter,
statistics of the device output, a fill inside a replayed graph, and a C client with no torch.

Tolerance of the value checks: atol 1e-5, rtol 0.  |z| <= 5.77; an angle rounded in fp32 (3.7e-7 rad) moves z by <= 2.2e-6 (the kernel
hands the angle over in half turns, which are exact, so it stays below that); a few ulp each from log, sqrt and sin / cos add
<~ 1.5e-6: a margin of about 2.5x.  test_fill_matches_the_reference prints the measured maximum."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import noise_reference as R
from noise_reference import KA1, KA2, KA2_ARGS, STAT, check_statistics

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-5
HI_SEED = 0xfedcba9876543210
HI_STEP = (1 << 40) + 3


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()
    return iaf_amd


def empty(n):
    return torch.empty(n, dtype=torch.float32, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def test_known_answer_vectors(amd):
    src = amd.NoiseSource(0)
    a = src.fill([empty(8)], advance=False)[0]
    np.testing.assert_allclose(host(a), KA1, rtol=0, atol=ATOL)
    src = amd.NoiseSource(KA2_ARGS["seed"])
    src.seek(KA2_ARGS["step"])
    b = src.fill([empty(1006)], substreams=[KA2_ARGS["substream"]])[0]
    np.testing.assert_allclose(host(b)[1000:], KA2, rtol=0, atol=ATOL)
    assert src.tell() == KA2_ARGS["step"] + 1


def test_fill_matches_the_reference(amd):
    """counts 1, 3, 4, 5, 1023, 2^20 + 1 in ONE list, a tensor 4 bytes into an allocation, scale 0.7, a step above 2^32, a seed
    with high bits set"""
    src = amd.NoiseSource(HI_SEED)
    src.seek(HI_STEP)
    counts = [1, 3, 4, 5, 1023, (1 << 20) + 1]
    big = empty(1000 + 1)
    off = big[1:]
    assert off.data_ptr() % 16 == 4
    tensors = [empty(n) for n in counts] + [off, empty(777)]
    subs = list(range(10, 10 + len(tensors)))
    scales = [1.0] * (len(tensors) - 1) + [0.7]
    src.fill(tensors, substreams=subs, scales=scales)
    worst = 0.0
    for t, s, sc in zip(tensors, subs, scales):
        want = R.normals(HI_SEED, s, HI_STEP, t.numel(), scale=sc)
        worst = max(worst, float(np.abs(host(t) - want).max()))
    print("device fill vs fp64 reference: max abs err %.3e (bound %.0e)" % (worst, ATOL))
    assert worst <= ATOL
    assert src.tell() == HI_STEP + 1
    # every other 4-byte alignment, and counts that end inside a counter
    for a in (1, 2, 3):
        for n in (1, 2, 3, 4, 6, 9, 1022):
            src.seek(5)
            base = torch.full((n + 8,), -7.0, dtype=torch.float32, device="cuda")
            src.fill([base[a:a + n]], substreams=[3])
            got = host(base)
            np.testing.assert_allclose(got[a:a + n], R.normals(HI_SEED, 3, 5, n), rtol=0, atol=ATOL)
            assert (got[:a] == -7.0).all() and (got[a + n:] == -7.0).all(), (a, n)     # nothing outside the tensor is written


def test_values_do_not_depend_on_the_list_the_chunking_or_the_alignment(amd):
    rng = np.random.RandomState(0)
    for n_t in (40, 70):                                       # one launch; two launches (64 + 6)
        counts = [int(c) for c in rng.randint(1, 5000, size=n_t)]
        src = amd.NoiseSource(77)
        src.seek(11)
        together = src.fill([empty(c) for c in counts])
        assert src.tell() == 12                                # one step per call, however many launches it took
        alone_src = amd.NoiseSource(77)
        for i, c in enumerate(counts):
            alone_src.seek(11)
            one = alone_src.fill([empty(c)], substreams=[i], advance=False)[0]
            torch.cuda.synchronize()
            assert torch.equal(one, together[i]), (n_t, i)
    # aligned against misaligned, bit for bit
    src = amd.NoiseSource(77)
    n = 4099
    a = src.fill([empty(n)], advance=False)[0]
    for o in (1, 2, 3):
        b = src.fill([empty(n + 4)[o:o + n]], advance=False)[0]
        torch.cuda.synchronize()
        assert torch.equal(a, b), o


def test_equal_seeds_seek_and_what_must_differ(amd):
    a, b = amd.NoiseSource(5), amd.NoiseSource(5)
    n = 10001
    xa = [a.fill([empty(n)])[0] for _ in range(3)]             # steps 0, 1, 2
    xb = [b.fill([empty(n)])[0] for _ in range(3)]
    torch.cuda.synchronize()
    for p, q in zip(xa, xb):
        assert torch.equal(p, q)
    assert a.tell() == 3
    a.seek(1)
    again = a.fill([empty(n)])[0]
    torch.cuda.synchronize()
    assert torch.equal(again, xa[1]) and a.tell() == 2
    assert not torch.equal(xa[0], xa[1]) and not torch.equal(xa[1], xa[2])                     # steps
    a.seek(0)
    other_sub = a.fill([empty(n)], substreams=[1], advance=False)[0]
    other_seed = amd.NoiseSource(6).fill([empty(n)])[0]
    based = amd.NoiseSource(5, substream_base=1).fill([empty(n)])[0]
    torch.cuda.synchronize()
    assert not torch.equal(other_sub, xa[0]) and not torch.equal(other_seed, xa[0])           # substreams, seeds
    assert torch.equal(based, other_sub)                                                       # substream_base + position


def test_advance_and_skip(amd):
    src = amd.NoiseSource(9)
    t = empty(100)
    assert src.tell() == 0
    src.fill([t], advance=False)
    first = t.clone()
    src.fill([t], advance=False)
    torch.cuda.synchronize()
    assert src.tell() == 0 and torch.equal(t, first)
    src.fill([t])
    src.fill([empty(10) for _ in range(130)])                  # three launches, one step
    assert src.tell() == 2
    src.skip(5)
    assert src.tell() == 7
    src.seek((1 << 63) + 1)
    assert src.tell() == (1 << 63) + 1


def test_host_side_checks(amd):
    src = amd.NoiseSource(1)
    for bad in ([], [torch.empty(4)], [torch.empty(4, dtype=torch.float64, device="cuda")], [empty(16)[::2]], [empty(0)]):
        with pytest.raises(ValueError):
            src.fill(bad)
    with pytest.raises(ValueError):
        src.fill([empty(4)], substreams=[1, 2])
    with pytest.raises(ValueError):
        src.fill([empty(4)], substreams=[-1])
    with pytest.raises(ValueError):
        src.seek(-1)
    for seed in (-1, 1 << 64, 1.5, True):
        with pytest.raises(ValueError):
            amd.NoiseSource(seed)
    assert src.tell() == 0                                     # nothing above reached the device


def test_device_statistics(amd):
    src = amd.NoiseSource(STAT["seed"])
    src.seek(STAT["step"])
    z = src.fill([empty(STAT["N"])], substreams=[STAT["substream"]])[0]
    check_statistics(host(z))


def test_fill_in_a_replayed_graph_draws_a_fresh_step_per_replay(amd):
    src = amd.NoiseSource(31)
    s0 = 1 << 33
    shapes = [(8, 32, 16, 16), (8, 32, 8, 8), (5,)]
    static = [torch.empty(sh, dtype=torch.float32, device="cuda") for sh in shapes]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        src.fill(static)                                       # eager warm-up on the capture stream
        side.synchronize()
        src.seek(s0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            src.fill(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert src.tell() == s0                                    # capturing ran nothing
    eager = amd.NoiseSource(31)
    for r in range(3):
        g.replay()
        eager.seek(s0 + r)
        want = eager.fill([torch.empty(sh, dtype=torch.float32, device="cuda") for sh in shapes])
        torch.cuda.synchronize()
        for a, b in zip(static, want):
            assert torch.equal(a, b), r
    assert src.tell() == s0 + 3
    del g


def test_c_client_without_torch_draws_the_known_answer(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    lib = os.path.join(ROOT, "iaf_amd", "_lib")
    exe = str(tmp_path / "iaf_noise_client")
    cmd = [hipcc, "-x", "c", os.path.join(ROOT, "tests", "c_abi", "iaf_noise_client.c"), "-D__HIP_PLATFORM_AMD__",
           "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-L" + lib, "-liaf_hip", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + lib, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, "C client does not build:\n" + b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(l.split(" ", 1) for l in r.stdout.strip().splitlines())
    np.testing.assert_allclose([float(v) for v in lines["z"].split()], KA1, rtol=0, atol=ATOL)
    assert int(lines["step"]) == 1
