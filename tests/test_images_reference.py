"""CPU-side checks of run_eval's image summaries: tests/images_reference.py (the NumPy restatement the GPU tests hold the kernels to)
against tests/golden/image_grids.npz, which the reference's own img_stretch / img_tile wrote (tests/golden/make_golden_images.py);
iaf_amd.grid_shape against the fixture's shapes; write_png decoded with zlib alone; the argument validation of iaf_img_range and
iaf_img_grid, which answers before any device call (as tests/test_capi_symbols.py).  No GPU needed.

TOL = 2**-22: the grids lie in [0, 1], and two ulps of 1.0 leave room for a reciprocal-multiply division and for the fp64 / fp32
promotion difference between NumPy versions in `max + 1e-12`."""
import ctypes
import io
import os
import struct
import zlib

import numpy as np
import pytest

import images_reference as R
import make_golden_images as G

TOL = 2.0 ** -22


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "image_grids.npz"))


def case_sources(golden, name):
    return [(golden["%s/%s" % (name, key)], over, then) for key, _, _, over, then in G.CASES[name][0]]


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_restatement_matches_the_reference_grids(golden, name):
    sources, n_imgs, C, border, color = G.CASES[name]
    want = golden["%s/grid" % name]
    got = R.grid(case_sources(golden, name), n_imgs, border, color)
    assert got.shape == want.shape and got.dtype == np.float32
    err = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))))
    print("%s: max abs err %.3e" % (name, err))
    assert err <= TOL
    assert want.min() >= 0.0 and want.max() <= 1.0
    if name.startswith("constant"):
        assert not want.any()             # 0 / 1e-12
    elif border == 0 and n_imgs in (1, 4, 6):
        assert want.max() > 0.99          # (a stretched slice reaches 1 up to the 1e-12)


def test_fixture_covers_the_cases_the_kernels_can_get_wrong(golden):
    ns = {c[1] for c in G.CASES.values()}
    assert {1, 4, 5, 6} <= ns
    assert {c[2] for c in G.CASES.values()} == {1, 3}
    assert {(c[3], c[4]) for c in G.CASES.values()} == {(0, 0.0), (1, 0.25)}
    assert any(len(c[0]) == 2 and {s[1] for s in c[0]} == {"u8", "f32"} for c in G.CASES.values())
    a = golden["twice_c3/a"]              # outer + inner stretch: the slice's extremes are not the batch's
    assert a[:4].min() > a.min() and a[:4].max() < a.max()
    n = golden["narrow/a"]
    assert 0 < n.max() - n.min() <= 1e-7
    assert G.H != G.W


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_grid_shape_matches_the_fixture(golden, name):
    import iaf_amd
    _, n_imgs, C, border, _ = G.CASES[name]
    th, tw = iaf_amd.grid_shape(n_imgs, G.H, G.W)
    assert (th, tw) == R.grid_shape(n_imgs, G.H, G.W)
    assert golden["%s/grid" % name].shape == ((G.H + border) * th - border, (G.W + border) * tw - border, C)
    assert th * tw >= n_imgs


def test_grid_shape_of_the_workload_and_bad_arguments():
    import iaf_amd
    assert iaf_amd.grid_shape(36, 32, 32) == (6, 6)
    assert iaf_amd.grid_shape(4, 16, 16) == (2, 2)
    assert iaf_amd.grid_shape(5, 3, 5) == (3, 2)
    assert iaf_amd.grid_shape(6, 3, 5, aspect_ratio=2.0) == R.grid_shape(6, 3, 5, 2.0)
    for bad in ((0, 3, 5), (4, 0, 5), (4, 3, -1), (4.0, 3, 5), (True, 3, 5)):
        with pytest.raises(ValueError):
            iaf_amd.grid_shape(*bad)
    for ar in (0.0, -1.0, float("inf"), float("nan"), "1"):
        with pytest.raises(ValueError):
            iaf_amd.grid_shape(4, 3, 5, aspect_ratio=ar)


def test_quantise_rule():
    v = np.array([0.0, 1.0, 0.5, 0.49999997, -0.1, 1.2, np.nan, 0.25, np.inf, -np.inf], dtype=np.float32)
    np.testing.assert_array_equal(R.quantise(v), np.array([0, 255, 128, 127, 0, 255, 0, 64, 255, 0], dtype=np.uint8))


# ---------------------------------------------------------------- write_png, decoded with zlib alone
def decode_png(blob):
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(blob):
        n, tag = struct.unpack(">I4s", blob[pos:pos + 8])
        data = blob[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + data) & 0xffffffff, "CRC of %r" % tag
        chunks.append((tag, data))
        pos += 12 + n
    assert pos == len(blob)
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"") and len(chunks[0][1]) == 13
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and colour in (0, 2)
    C = 3 if colour == 2 else 1
    raw = zlib.decompress(b"".join(d for t, d in chunks if t == b"IDAT"))
    assert len(raw) == H * (1 + W * C)
    rows = np.frombuffer(raw, np.uint8).reshape(H, 1 + W * C)
    assert not rows[:, 0].any()           # filter type 0 on every row
    return rows[:, 1:].reshape(H, W, C)


@pytest.mark.parametrize("shape", [(1, 1, 3), (7, 5, 3), (4, 9, 1), (6, 3)], ids=["1x1", "7x5rgb", "grey", "grey2d"])
def test_write_png_round_trip(tmp_path, shape):
    import torch
    import iaf_amd
    g = np.random.RandomState(sum(shape)).randint(0, 256, size=shape).astype(np.uint8)
    want = g.reshape(shape[0], shape[1], -1)
    buf = io.BytesIO()
    iaf_amd.write_png(buf, g)
    np.testing.assert_array_equal(decode_png(buf.getvalue()), want)
    path = str(tmp_path / "g.png")
    iaf_amd.write_png(path, torch.from_numpy(g))              # a host tensor, a path
    np.testing.assert_array_equal(decode_png(open(path, "rb").read()), want)


def test_write_png_refuses_what_it_cannot_write():
    import iaf_amd
    for bad in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 2), np.uint8), np.zeros((0, 4, 3), np.uint8), np.zeros((4,), np.uint8),
                [[1, 2], [3, 4]]):
        with pytest.raises(ValueError):
            iaf_amd.write_png(io.BytesIO(), bad)


# ---------------------------------------------------------------- the C ABI's argument validation: before any device call
@pytest.fixture(scope="module")
def capi():
    from iaf_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _capi.lib()
    return _capi


def test_img_range_argument_errors(capi):
    lib, p = capi.lib(), ctypes.c_void_p
    src, rec = p(0x1000), p(0x2000)       # never dereferenced: every call below is refused before any device work
    assert lib.iaf_img_range(None, 0, 16, rec, None) == capi.IAF_ERR_NULL
    assert lib.iaf_img_range(src, 0, 16, None, None) == capi.IAF_ERR_NULL
    assert lib.iaf_img_range(src, 2, 16, rec, None) == capi.IAF_ERR_SHAPE
    assert lib.iaf_img_range(src, -1, 16, rec, None) == capi.IAF_ERR_SHAPE
    assert lib.iaf_img_range(src, 1, 0, rec, None) == capi.IAF_ERR_SHAPE
    assert lib.iaf_img_range(src, 0, 16, p(0x2004), None) == capi.IAF_ERR_WORKSPACE
    assert lib.iaf_img_range(p(0x1002), 1, 16, rec, None) == capi.IAF_ERR_WORKSPACE


def _table(capi, n=1, **over):
    t = (capi.ImgSource * 2)()
    for s in range(n):
        t[s].ptr, t[s].dtype, t[s].outer, t[s].inner = 0x1000, 1, 0x2000, None
    for k, v in over.items():
        setattr(t[0], k, v)
    return t


def test_img_grid_argument_errors(capi):
    lib, p = capi.lib(), ctypes.c_void_p
    gf, g8 = p(0x3000), p(0x4000)         # never dereferenced, as above

    def call(table, n_src=1, n_imgs=4, C=3, H=3, W=5, border=0, f=gf, u=g8):
        return lib.iaf_img_grid(table, n_src, n_imgs, C, H, W, border, 0.0, f, u, None)
    ok = _table(capi)
    assert call(None) == capi.IAF_ERR_NULL
    assert call(ok, f=None, u=None) == capi.IAF_ERR_NULL
    assert call(_table(capi, ptr=None)) == capi.IAF_ERR_NULL
    assert call(_table(capi, outer=None)) == capi.IAF_ERR_NULL
    for kw in (dict(n_src=0), dict(n_src=3), dict(n_imgs=0), dict(C=2), dict(C=4), dict(C=0), dict(H=0), dict(W=0), dict(border=-1)):
        assert call(_table(capi, 2), **kw) == capi.IAF_ERR_SHAPE, kw
    assert call(_table(capi, dtype=2)) == capi.IAF_ERR_SHAPE
    assert call(_table(capi, outer=0x2004)) == capi.IAF_ERR_WORKSPACE
    assert call(_table(capi, inner=0x2004)) == capi.IAF_ERR_WORKSPACE
    two = _table(capi, 2)
    two[1].outer = None                   # the second source is checked as the first
    assert call(two, n_src=2) == capi.IAF_ERR_NULL
    with pytest.raises(ValueError):
        capi.check(capi.IAF_ERR_WORKSPACE)
