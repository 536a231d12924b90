"""GPU tests of the device-resident dataset (iaf_amd.DeviceDataset, include/iaf_hip.h: iaf_data_*): the gather against
the numpy statement of the definition (tests/data_reference.py) -- indices and bytes, exactly -- on both copy paths, at the sizes where
the Feistel domain changes, across an epoch boundary and across 2^32 steps; the step counter; the ABI's error codes; the gather inside a
replayed graph; and TrainStep(data=), which trains bit for bit on what a twin step is fed from the reference indices."""
import ctypes

import numpy as np
import pytest
import torch

import data_reference as D
import golden_inputs as gi

pytestmark = pytest.mark.gpu

LR = 2e-3
SEED = 2024


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()
    return iaf_amd


def make_images(n, S, offset=0, seed=0):
    """uint8 [n,3,S,S] random images on the device; offset: bytes between a 256-byte boundary and the first image"""
    g = torch.Generator(device="cuda")
    g.manual_seed(1000 * n + S + seed)
    flat = torch.randint(0, 256, (n * 3 * S * S + offset,), dtype=torch.uint8, device="cuda", generator=g)
    img = flat[offset:].view(n, 3, S, S)
    assert img.is_contiguous() and img.data_ptr() % 16 == offset % 16
    return img


def guarded_out(B, S, offset=0):
    """a [B,3,S,S] batch buffer with 64 sentinel bytes in front of it and behind it"""
    nb = B * 3 * S * S
    buf = torch.full((64 + offset + nb + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[64 + offset:64 + offset + nb].view(B, 3, S, S)


def sentinels_intact(buf, B, S, offset=0):
    nb = B * 3 * S * S
    return bool((buf[:64 + offset] == 0xA5).all()) and bool((buf[64 + offset + nb:] == 0xA5).all())


# -- the gather against the definition ---------------------------------------------------------------------------------------------------
# (S, image base offset): 12 bytes per image (byte path only), 48, 3072, 12288 (three workgroups per image), 3072 one byte off a boundary
GEOMETRIES = [(2, 0), (4, 0), (32, 0), (64, 0), (32, 1)]


@pytest.mark.parametrize("S,offset", GEOMETRIES, ids=["12B", "48B", "3072B", "12288B", "3072B-unaligned"])
def test_next_batch_equals_the_reference(amd, S, offset):
    checked = 0
    for n in (1, 2, 5, 17, 65, 1000):
        images = make_images(n, S, offset)
        for rank, world in ((0, 1), (1, 3)):
            ds = amd.DeviceDataset(images, SEED + n, rank=rank, world=world)
            assert ds.n == n and ds.bytes_per_image == 3 * S * S
            for B in (1, 3, 32):
                if B * world > n:
                    with pytest.raises(ValueError):
                        ds.next_batch(B)
                    continue
                bpe = ds.batches_per_epoch(B)
                assert bpe == D.batches_per_epoch(n, B, world)
                buf, out = guarded_out(B, S)
                idx = torch.full((B,), -1, dtype=torch.int64, device="cuda")
                for s0 in (0, bpe - 1, (1 << 32) - 1):
                    ds.seek(s0)
                    for step in (s0, s0 + 1):                          # (the second call is over the epoch boundary / past 2^32)
                        got = ds.next_batch(B, out=out, indices=idx)
                        assert got is out
                        want = torch.from_numpy(D.batch_indices(n, SEED + n, step, B, rank, world)).cuda()
                        assert torch.equal(idx, want), (n, B, rank, world, step, idx.tolist(), want.tolist())
                        assert torch.equal(out, images[want]), (n, B, rank, world, step)
                        checked += 1
                    assert ds.tell() == s0 + 2
                assert sentinels_intact(buf, B, S)
    assert checked >= 100, checked


def test_unaligned_output_and_no_index_buffer(amd):
    n, S, B = 17, 32, 3
    images = make_images(n, S)
    ds = amd.DeviceDataset(images, 5)
    buf, out = guarded_out(B, S, offset=3)
    ds.next_batch(B, out=out)
    want = torch.from_numpy(D.batch_indices(n, 5, 0, B)).cuda()
    assert torch.equal(out, images[want]) and sentinels_intact(buf, B, S, offset=3)
    fresh = ds.next_batch(B)                                           # step 1, a buffer of its own
    want = torch.from_numpy(D.batch_indices(n, 5, 1, B)).cuda()
    assert fresh.dtype == torch.uint8 and tuple(fresh.shape) == (B, 3, S, S) and torch.equal(fresh, images[want])


def test_counter_advance_seek_skip_tell(amd):
    n, S, B = 65, 4, 3
    images = make_images(n, S)
    ds = amd.DeviceDataset(images, 77)
    assert ds.tell() == 0
    a = ds.next_batch(B, advance=False).clone()
    b = ds.next_batch(B, advance=False).clone()
    assert torch.equal(a, b) and ds.tell() == 0
    c = ds.next_batch(B)
    assert torch.equal(a, c) and ds.tell() == 1
    ds.skip(4)
    assert ds.tell() == 5
    ds.skip(0)
    assert ds.tell() == 5
    ds.seek((1 << 64) - 2)
    assert ds.tell() == (1 << 64) - 2
    idx = torch.empty(B, dtype=torch.int64, device="cuda")
    ds.next_batch(B, indices=idx)
    assert idx.tolist() == D.batch_indices(n, 77, (1 << 64) - 2, B).tolist() and ds.tell() == (1 << 64) - 1
    ds.seek(5)
    ds.next_batch(B, indices=idx)
    assert idx.tolist() == D.batch_indices(n, 77, 5, B).tolist()
    # two datasets on the same images are independent; the seed matters
    other = amd.DeviceDataset(images, 78)
    jdx = torch.empty(B, dtype=torch.int64, device="cuda")
    other.seek(5)
    other.next_batch(B, indices=jdx)
    assert jdx.tolist() == D.batch_indices(n, 78, 5, B).tolist() and jdx.tolist() != idx.tolist()
    for bad in (-1, 1 << 64, 1.0, True):
        with pytest.raises(ValueError):
            ds.seek(bad)
        with pytest.raises(ValueError):
            ds.skip(bad)
    for kw in (dict(B=0), dict(B=True), dict(B=66), dict(B=3, out=torch.empty(3, 3, 4, 4, device="cuda")),
               dict(B=3, out=torch.empty(2, 3, 4, 4, dtype=torch.uint8, device="cuda")),
               dict(B=3, out=torch.empty(3, 3, 4, 4, dtype=torch.uint8)),
               dict(B=3, indices=torch.empty(3, dtype=torch.int32, device="cuda")),
               dict(B=3, indices=torch.empty(4, dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            ds.next_batch(**kw)
    assert ds.tell() == 6


def test_deterministic_walks_the_images_in_order(amd):
    n, S, B = 17, 2, 3
    images = make_images(n, S)
    ds = amd.DeviceDataset(images, 1, deterministic=True)
    bpe = ds.batches_per_epoch(B)
    assert bpe == 5
    idx = torch.empty(B, dtype=torch.int64, device="cuda")
    for step in range(2 * bpe + 1):
        out = ds.next_batch(B, indices=idx)
        first = (step % bpe) * B                                       # restarts at 0 after bpe batches; images 15, 16 are never drawn
        assert idx.tolist() == [first, first + 1, first + 2], step
        assert torch.equal(out, images[first:first + B]), step
    two = amd.DeviceDataset(images, 1, deterministic=True, rank=1, world=2)
    two.seek(3)
    two.next_batch(B, indices=idx)
    assert idx.tolist() == [9, 10, 11]                                 # bpe = 2: slot (3 % 2) * 6 + 1 * 3


# -- the C ABI's errors --------------------------------------------------------------------------------------------------------------------
def test_abi_error_codes(amd):
    capi = amd._capi
    lib = capi.lib()
    images = make_images(5, 2)
    ip = ctypes.c_void_p(images.data_ptr())
    out = torch.empty(5, 3, 2, 2, dtype=torch.uint8, device="cuda")
    op = ctypes.c_void_p(out.data_ptr())
    h = ctypes.c_void_p()
    assert lib.iaf_data_create(None, ip, 5, 12, 1, 0) == capi.IAF_ERR_NULL
    assert lib.iaf_data_create(ctypes.byref(h), None, 5, 12, 1, 0) == capi.IAF_ERR_NULL
    for n, bpi in ((0, 12), (1 << 32, 12), ((1 << 64) - 1, 12), (5, 0)):
        assert lib.iaf_data_create(ctypes.byref(h), ip, n, bpi, 1, 0) == capi.IAF_ERR_SHAPE, (n, bpi)
        assert not h.value
    assert lib.iaf_data_create(ctypes.byref(h), ip, 5, 12, 1, 0) == capi.IAF_OK and h.value
    try:
        assert lib.iaf_data_next_batch(None, op, None, 1, 0, 1, 1, None) == capi.IAF_ERR_NULL
        assert lib.iaf_data_next_batch(h, None, None, 1, 0, 1, 1, None) == capi.IAF_ERR_NULL
        for B, rank, world in ((0, 0, 1), (-1, 0, 1), (65536, 0, 1), (1, 0, 0), (1, 0, -1), (1, -1, 1), (1, 1, 1), (1, 3, 3), (6, 0, 1),
                               (2, 0, 3), (1 << 30, 0, 4)):
            assert lib.iaf_data_next_batch(h, op, None, B, rank, world, 1, None) == capi.IAF_ERR_SHAPE, (B, rank, world)
        v = ctypes.c_uint64(99)
        assert lib.iaf_data_seek(None, 1, None) == capi.IAF_ERR_NULL
        assert lib.iaf_data_skip(None, 1, None) == capi.IAF_ERR_NULL
        assert lib.iaf_data_tell(None, ctypes.byref(v), None) == capi.IAF_ERR_NULL
        assert lib.iaf_data_tell(h, None, None) == capi.IAF_ERR_NULL
        assert lib.iaf_data_tell(h, ctypes.byref(v), None) == capi.IAF_OK and v.value == 0          # no refused call moved the counter
        assert lib.iaf_data_next_batch(h, op, None, 5, 0, 1, 1, None) == capi.IAF_OK                # B * world == n is allowed
        assert lib.iaf_data_tell(h, ctypes.byref(v), None) == capi.IAF_OK and v.value == 1
        torch.cuda.synchronize()
        assert sorted(map(bytes, out.cpu().reshape(5, 12).numpy())) == sorted(map(bytes, images.cpu().reshape(5, 12).numpy()))
    finally:
        assert lib.iaf_data_destroy(h) == capi.IAF_OK
    assert lib.iaf_data_destroy(None) == capi.IAF_OK


# -- in a graph --------------------------------------------------------------------------------------------------------------------------
def test_a_captured_gather_draws_the_next_batch_at_every_replay(amd):
    n, S, B, s0 = 65, 32, 3, 20                                        # bpe = 21: the replays cross an epoch boundary
    images = make_images(n, S)
    ds = amd.DeviceDataset(images, SEED)
    out = torch.zeros(B, 3, S, S, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(B, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ds.seek(s0)
        ds.next_batch(B, out=out, indices=idx, advance=False)         # eager warm-up on the capture stream
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ds.next_batch(B, out=out, indices=idx)
    torch.cuda.current_stream().wait_stream(side)
    for step in (s0, s0 + 1, s0 + 2):
        g.replay()
        want = torch.from_numpy(D.batch_indices(n, SEED, step, B)).cuda()
        assert torch.equal(idx, want), step
        assert torch.equal(out, images[want]), step
    assert ds.tell() == s0 + 3
    del g


# -- TrainStep(data=) ----------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def train_model(amd, c):
    model = amd.CVAE1(z_size=c["z_size"], h_size=c["h_size"], kl_min=c["kl_min"], depth=c["depth"], num_blocks=c["num_blocks"], k=1,
                      image_size=c["image_size"])
    model.set_training(True)
    model.load({k: dev(v) for k, v in c["params"].items()})
    return model


def case_dataset(c):
    """n = 3 B + 1 images out of the case's batch: the batch rolled by 0, 1, 2 pixels, and one more image"""
    x = torch.from_numpy(c["x"]).cuda()
    return torch.cat([torch.roll(x, k, 3) for k in range(3)] + [torch.roll(x[:1], 3, 3)]).contiguous()


def _flat_equal(a, b, what):
    torch.cuda.synchronize()
    for k in ("params", "slot_m", "slot_v", "ema"):
        p, q = getattr(a.flat, k), getattr(b.flat, k)
        assert torch.equal(p, q), (what, k, float((p - q).abs().max()))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_train_step_trains_on_the_batches_of_the_reference_indices(amd, graph):
    c = gi.model_case_inputs("model_cfg")                          # the case tests/test_hip_train_step.py trains
    B = c["B"]
    images = case_dataset(c)
    n, s0, n0 = int(images.shape[0]), 1, 5                         # bpe = 3: steps 1, 2 | 3, 4 cross an epoch boundary
    assert n == 3 * B + 1
    ds = amd.DeviceDataset(images, SEED)
    assert ds.batches_per_epoch(B) == 3
    ds.seek(s0)
    src, twin = amd.NoiseSource(SEED), amd.NoiseSource(SEED)
    src.seek(n0)
    ts = amd.TrainStep(train_model(amd, c), LR, graph=graph, noise_source=src, data=ds, batch_size=B)
    ref = amd.TrainStep(train_model(amd, c), LR, graph=graph)
    seen = []
    for t in range(4):
        obj = ts().clone()
        idx = D.batch_indices(n, SEED, s0 + t, B)
        seen.append(idx)
        twin.seek(n0 + t)
        want = ref(images[torch.from_numpy(idx).cuda()], ref.model.draw_noise(B, twin, which="posterior")).clone()
        torch.cuda.synchronize()
        assert torch.equal(obj, want), (t, float(obj), float(want))
        _flat_equal(ts, ref, "call %d" % t)
    assert not np.array_equal(np.sort(np.concatenate(seen[:2])), np.sort(np.concatenate(seen[2:])))
    assert ds.tell() == s0 + 4 and src.tell() == n0 + 4
    assert ts.skipped == 0 and ref.skipped == 0
    assert ts.graphed == graph and ref.graphed == graph
    if graph:
        assert ts.captures == 1 and ref.captures == 1


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_a_call_with_an_explicit_batch_still_moves_the_dataset_on(amd, graph):
    """call 1 brings its own batch: it trains on that batch (as eager launches), counts as a call, and call 2 gathers step s0 + 2"""
    c = gi.model_case_inputs("model_cfg")
    B = c["B"]
    images = case_dataset(c)
    n, s0, n0 = int(images.shape[0]), 7, 0
    ds = amd.DeviceDataset(images, SEED)
    ds.seek(s0)
    src, twin = amd.NoiseSource(SEED), amd.NoiseSource(SEED)
    ts = amd.TrainStep(train_model(amd, c), LR, graph=graph, noise_source=src, data=ds, batch_size=B)
    ref = amd.TrainStep(train_model(amd, c), LR, graph=graph)
    own = torch.from_numpy(c["x"]).cuda().flip(0).contiguous()
    for t in range(4):
        xt = own if t == 1 else images[torch.from_numpy(D.batch_indices(n, SEED, s0 + t, B)).cuda()]
        obj = (ts(own) if t == 1 else ts()).clone()
        twin.seek(n0 + t)
        want = ref(xt, ref.model.draw_noise(B, twin, which="posterior")).clone()
        torch.cuda.synchronize()
        assert torch.equal(obj, want), (t, float(obj), float(want))
        _flat_equal(ts, ref, "call %d" % t)
        assert ds.tell() == s0 + t + 1 and src.tell() == n0 + t + 1
    if graph:
        assert ts.captures == 1


def test_train_step_with_a_dataset_and_the_callers_noise(amd):
    """data= without noise_source: ts(noise=list)"""
    c = gi.model_case_inputs("model_cfg")
    B = c["B"]
    images = case_dataset(c)
    n = int(images.shape[0])
    ds = amd.DeviceDataset(images, SEED)
    ts = amd.TrainStep(train_model(amd, c), LR, graph=True, data=ds, batch_size=B)
    ref = amd.TrainStep(train_model(amd, c), LR, graph=True)
    noise = [dev(e) for e in c["noise"]]
    with pytest.raises(ValueError):
        ts()                                                       # neither a source nor a list
    for t in range(2):
        obj = ts(noise=noise).clone()
        want = ref(images[torch.from_numpy(D.batch_indices(n, SEED, t, B)).cuda()], noise).clone()
        torch.cuda.synchronize()
        assert torch.equal(obj, want), t
        _flat_equal(ts, ref, "call %d" % t)
    assert ds.tell() == 2 and ts.graphed and ts.captures == 1
    with pytest.raises(ValueError):
        amd.TrainStep(train_model(amd, c), LR, data=amd.DeviceDataset(images, SEED, world=2), batch_size=B)    # the step's world is 1
