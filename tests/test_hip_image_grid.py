"""GPU tests of iaf_img_range and iaf_img_grid (include/iaf_hip.h; iaf_amd/images.py): the range record against NumPy's min / max --
exact, min and max do not depend on order --, the grids against tests/golden/image_grids.npz, which the reference's own img_stretch /
img_tile wrote, within 2**-22 (tests/test_images_reference.py says why), the byte grid against the package's rule applied to the
device's own float grid, and a capture of both launches in one graph."""
import os

import numpy as np
import pytest
import torch

import images_reference as R
import make_golden_images as G

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -22
SHARE = 16384                 # bytes of the aligned body one workgroup takes before another is added (iaf_kernels_image.hpp)


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()      # raises if the HIP extension is missing: no silent fallback
    return iaf_amd


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "image_grids.npz"))


def img_range(amd, t, n=None, record=None):
    """iaf_img_range over the first n elements of the 1-d device tensor t; the record as a host (lo, hi, nonfinite, arrivals)"""
    capi = amd._capi
    rec = torch.zeros(4, dtype=torch.int32, device="cuda") if record is None else record
    dt = capi.IAF_IMG_U8 if t.dtype == torch.uint8 else capi.IAF_IMG_F32
    capi.check(capi.lib().iaf_img_range(capi.ptr(t), dt, t.numel() if n is None else n, capi.ptr(rec), capi.stream()))
    h = rec.cpu()
    lo, hi = h[:2].view(torch.float32).tolist()
    return lo, hi, int(h[2]), int(h[3])


def _data(dtype, n, seed):
    rng = np.random.RandomState(seed)
    if dtype == "u8":
        return rng.randint(5, 250, size=n).astype(np.uint8)
    return (rng.standard_normal(n) * 3).astype(np.float32)


# 1 .. 4097: head / body / tail of one workgroup; the last two: beyond one workgroup's share (fp32: 3 and 17 workgroups, uint8: 1 and 4)
SIZES = [1, 63, 64, 65, 255, 4097, 2 * SHARE // 4 + 7, 4 * SHARE + 13]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_range_is_exact_and_repeats(amd, dtype, n, offset):
    a = _data(dtype, n + offset, n)
    a[offset], a[-1] = (250, 2) if dtype == "u8" else (40.0, -50.0)           # the maximum first, the minimum last
    t = torch.from_numpy(a).cuda()[offset:]
    assert t.data_ptr() % 16 == (offset * a.itemsize) % 16
    rec = torch.zeros(4, dtype=torch.int32, device="cuda")
    first = img_range(amd, t, record=rec)
    assert first == (float(a[offset:].min()), float(a[offset:].max()), 0, 0)
    assert img_range(amd, t, record=rec) == first                               # the record is reused: nothing to clear in between
    a2 = a.copy()
    a2[offset + n // 2] = 251 if dtype == "u8" else 41.5                        # another maximum, in the middle; the same record once more
    assert img_range(amd, torch.from_numpy(a2).cuda()[offset:], record=rec) == (float(a2[offset:].min()), float(a2[offset:].max()), 0, 0)


@pytest.mark.parametrize("n", [1, 65, 4097, 4 * SHARE + 13])
def test_range_counts_and_excludes_nonfinite(amd, n):
    a = _data("f32", n, 100 + n)
    finite = a.copy()
    bad = sorted({0, n - 1, n // 2, n // 3, (2 * n) // 3})
    for k, i in enumerate(bad):
        a[i] = (np.nan, np.inf, -np.inf)[k % 3]
    keep = np.delete(finite, bad)
    lo, hi, nf, arrivals = img_range(amd, torch.from_numpy(a).cuda())
    assert (nf, arrivals) == (len(bad), 0)
    if keep.size:
        assert (lo, hi) == (float(keep.min()), float(keep.max()))
    else:
        assert (lo, hi) == (float("inf"), float("-inf"))


def test_range_of_a_leading_slice_and_of_zeros(amd):
    a = _data("f32", 1000, 5)
    a[700] = 99.0
    t = torch.from_numpy(a).cuda()
    assert img_range(amd, t, n=700)[:2] == (float(a[:700].min()), float(a[:700].max()))
    z = torch.from_numpy(np.array([-0.0, 0.0, -0.0], np.float32)).cuda()
    lo, hi, _, _ = img_range(amd, z)
    assert (lo, hi) == (0.0, 0.0) and np.signbit(lo) == np.signbit(hi) == False          # noqa: E712  (either zero leaves as +0)


# ---------------------------------------------------------------- the grid
def case_sources(golden, name, dev=True):
    out = []
    for key, _, _, over, then in G.CASES[name][0]:
        a = golden["%s/%s" % (name, key)]
        out.append((torch.from_numpy(a).cuda() if dev else a, over, then))
    return out


def _tiles(n_imgs, C, border):
    """[(slot or None, y slice, x slice)] of every tile of the grid, and the mask of the border pixels"""
    th, tw = R.grid_shape(n_imgs, G.H, G.W)
    border_mask = np.ones(((G.H + border) * th - border, (G.W + border) * tw - border), bool)
    tiles = []
    for i in range(th * tw):
        ys, xs = slice((G.H + border) * (i // tw), (G.H + border) * (i // tw) + G.H), slice((G.W + border) * (i % tw), (G.W + border) * (i % tw) + G.W)
        tiles.append((i if i < n_imgs else None, ys, xs))
        border_mask[ys, xs] = False
    return tiles, border_mask


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_grid_matches_the_reference_fixture(amd, golden, name):
    _, n_imgs, C, border, color = G.CASES[name]
    want = golden["%s/grid" % name]
    g8, gf, rec = amd.image_grid(case_sources(golden, name), n_imgs, border=border, border_color=color)
    gf, g8, rec = gf.cpu().numpy(), g8.cpu().numpy(), rec.cpu().numpy()
    assert gf.shape == want.shape == g8.shape and gf.dtype == np.float32 and g8.dtype == np.uint8
    err = float(np.max(np.abs(gf.astype(np.float64) - want.astype(np.float64))))
    print("%s: max abs err %.3e (bound %.3e)" % (name, err, TOL))
    assert err <= TOL
    np.testing.assert_array_equal(g8, R.quantise(gf))                           # the byte is a function of the float grid's bits
    tiles, border_mask = _tiles(n_imgs, C, border)
    colour = np.float32(color)
    assert (gf[border_mask] == colour).all()
    for slot, ys, xs in tiles:
        if slot is None:
            assert (gf[ys, xs] == colour).all()
    assert not rec[:, 2].any() and not rec[:, 3].any()                          # nothing non-finite; every record closed
    # one output alone gives the same grid
    only8 = amd.image_grid(case_sources(golden, name), n_imgs, border=border, border_color=color, f32=False)
    onlyf = amd.image_grid(case_sources(golden, name), n_imgs, border=border, border_color=color, u8=False)
    assert only8[1] is None and onlyf[0] is None
    np.testing.assert_array_equal(only8[0].cpu().numpy(), g8)
    np.testing.assert_array_equal(onlyf[1].cpu().numpy().view(np.uint32), gf.view(np.uint32))


def test_a_nonfinite_source_blanks_its_own_slots_only(amd, golden):
    name = "pair_c1_b1"
    _, n_imgs, C, border, color = G.CASES[name]
    (a, oa, _), (b, ob, _) = case_sources(golden, name, dev=False)
    b = b.copy()
    b[1, 0, 2, 3] = np.nan
    b[0, 0, 0, 0] = np.inf
    clean = amd.image_grid(case_sources(golden, name), n_imgs, border=border, border_color=color)
    g8, gf, rec = amd.image_grid([(torch.from_numpy(a).cuda(), oa, None), (torch.from_numpy(b).cuda(), ob, None)], n_imgs, border=border,
                                 border_color=color)
    gf, g8, want = gf.cpu().numpy(), g8.cpu().numpy(), clean[1].cpu().numpy()
    assert rec.cpu().numpy()[:, 2].tolist() == [0, 2]
    tiles, border_mask = _tiles(n_imgs, C, border)
    for slot, ys, xs in tiles:
        if slot is not None and slot % 2 == 1:
            assert np.isnan(gf[ys, xs]).all() and not g8[ys, xs].any()
        else:
            np.testing.assert_array_equal(gf[ys, xs].view(np.uint32), want[ys, xs].view(np.uint32))
    np.testing.assert_array_equal(gf[border_mask], want[border_mask])
    np.testing.assert_array_equal(g8, R.quantise(gf))


def test_image_grid_refuses_bad_sources_before_any_launch(amd):
    u = torch.zeros((4, 3, 3, 5), dtype=torch.uint8, device="cuda")
    f = torch.zeros((4, 3, 3, 5), dtype=torch.float32, device="cuda")
    for bad in (lambda: amd.image_grid([], 1), lambda: amd.image_grid([(u, 4), (f, 4), (f, 4)], 2), lambda: amd.image_grid([(u, 5)], 1),
                lambda: amd.image_grid([(u, 0)], 1), lambda: amd.image_grid([(u, 2, 3)], 1), lambda: amd.image_grid([(u, 4, 2)], 3),
                lambda: amd.image_grid([(u, 4)], 5), lambda: amd.image_grid([(u, 4), (f[:, :1], 4)], 2),
                lambda: amd.image_grid([(f.double(), 4)], 1), lambda: amd.image_grid([(u.cpu(), 4)], 1),
                lambda: amd.image_grid([(f.permute(0, 1, 3, 2), 4)], 1), lambda: amd.image_grid([(u, 4)], 4, border=-1),
                lambda: amd.image_grid([(u, 4)], 4, border_color=float("nan")), lambda: amd.image_grid([(u, 4)], 4, u8=False, f32=False),
                lambda: amd.image_grid([(u, 4), (f, 1)], 4)):
        with pytest.raises(ValueError):
            bad()


def test_range_and_grid_replay_in_one_graph(amd, golden):
    """both launches captured once; the source changes in place between replays, and every replay's grids are bit for bit what an
    eager call gives on the same data (the records need nothing cleared in between: the range launch closes them itself)"""
    rng = np.random.RandomState(3)
    n = SHARE // 4 * 3 // (3 * G.H * G.W) + 2                                   # rows enough for more than one workgroup in the range launch
    src = torch.from_numpy((rng.standard_normal((n, 3, G.H, G.W))).astype(np.float32)).cuda()
    u = torch.from_numpy(rng.randint(0, 256, size=(3, 3, G.H, G.W)).astype(np.uint8)).cuda()
    assert n * 3 * G.H * G.W * 4 > SHARE

    def grids():
        return amd.image_grid([(u, 3), (src, n, 3)], 6, border=1, border_color=0.25)
    grids()                                                                     # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            c8, cf, crec = grids()
    torch.cuda.current_stream().wait_stream(side)
    for step in range(3):
        fresh = rng.standard_normal(tuple(src.shape)).astype(np.float32) * (step + 1)
        fresh[-1, 0, 0, 0] = 50.0 * (step + 1)                                  # the batch's maximum outside the rows shown
        src.copy_(torch.from_numpy(fresh).cuda())
        g.replay()
        e8, ef, erec = grids()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(cf.cpu().numpy().view(np.uint32), ef.cpu().numpy().view(np.uint32))
        np.testing.assert_array_equal(c8.cpu().numpy(), e8.cpu().numpy())
        np.testing.assert_array_equal(crec.cpu().numpy(), erec.cpu().numpy())
        want = R.grid([(u.cpu().numpy(), 3, None), (fresh, n, 3)], 6, 1, 0.25)
        assert float(np.max(np.abs(ef.cpu().numpy().astype(np.float64) - want))) <= TOL
