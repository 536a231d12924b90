"""CPU checks of the checkpoints (iaf_amd/checkpoint.py, TrainStep.snapshot / restore) on host replicas: the digest's known answers and
what it reacts to, the file against an independent reader and writer (tests/state_reference.py), the errors, and an exact resume across
a save with a skipped step on each side.  Every comparison is exact.  The model is the host stand-in of tests/test_train_step_api.py."""
import json
import os

import numpy as np
import pytest
import torch

import state_reference as R

LR = 0.01
FLAT = ("params", "slot_m", "slot_v", "ema")


class HostModel(object):
    """the host stand-in of tests/test_train_step_api.py with CVAE1's training interface:
    obj = 0.5 x[0] sum_k |p_k|^2 + x[1];  d obj / d p_k = x[0] p_k, plus noise[0] on the gradient of the third variable"""
    NAMES = ["top/V", "top/g", "mid/odd", "bottom/b"]
    SHAPES = [(3, 4), (5,), (7,), (2,)]

    def __init__(self, seed=3):
        rng = np.random.RandomState(seed)
        self.params = {k: torch.from_numpy(rng.standard_normal(s)).float() for k, s in zip(self.NAMES, self.SHAPES)}
        self._buckets = [list(self.NAMES)]

    def completion_order(self):
        return list(self.NAMES)

    def load(self, params):
        self.params = params

    def set_grad_buckets(self, n_buckets=1):
        n = max(1, min(n_buckets, len(self.NAMES)))
        self._buckets = [self.NAMES[q * len(self.NAMES) // n:(q + 1) * len(self.NAMES) // n] for q in range(n)]
        return [list(b) for b in self._buckets]

    def prepare_weights(self):
        pass

    def fb_begin(self, x, noise, grads=None):
        self._fb = (x, noise, grads)
        obj = 0.5 * x[0] * sum((p * p).sum() for p in self.params.values()) + x[1]
        return {"obj": obj.reshape(1)}

    def fb_segment(self, i):
        x, noise, grads = self._fb
        for k in self._buckets[i]:
            g = x[0] * self.params[k]
            if k == self.NAMES[2]:
                g = g + noise[0]
            grads[k].copy_(g)


def _batch(t):
    """step t's (x, noise); steps 1 and 4 are poisoned (a non-finite objective / gradient) and must be skipped"""
    x, noise = torch.tensor([1.0 + 0.25 * t, 0.25]), [torch.full((7,), 0.01 * t)]
    if t == 1:
        x = torch.tensor([1.0, float("nan")])
    if t == 4:
        noise = [torch.tensor([0.0] * 6 + [float("inf")])]
    return x, noise


def _step(seed=3, **kw):
    import iaf_amd
    return iaf_amd.TrainStep(HostModel(seed=seed), LR, n_buckets=2, graph=False, **kw)


def _state(ts):
    return {k: getattr(ts.flat, k).clone() for k in FLAT}


def _unchanged(ts, before):
    return all(torch.equal(getattr(ts.flat, k), before[k]) for k in FLAT)


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """a step after 3 calls (one skipped), its file, and the state at the save"""
    ts = _step()
    for t in range(3):
        ts(*_batch(t))
    path = str(tmp_path_factory.mktemp("ckpt") / "run.ckpt")
    snap = ts.snapshot()
    at_save = _state(ts)
    assert snap.save(path) == path
    return dict(ts=ts, path=path, state=at_save)


# -- the digest ---------------------------------------------------------------------------------------------------------------------------
KNOWN = [(np.zeros(0, np.uint32), 0),
         (np.zeros(1, np.uint32), 0x9e3779b1),
         (np.arange(5, dtype=np.uint32), 0x6b69628af),
         (np.full(5, 0xFFFFFFFF, np.uint32), 0x736ae24900000000)]


def test_digest_known_answers():
    from iaf_amd import checkpoint as C
    for words, want in KNOWN:
        assert C.digest(words) == want == R.digest(words) == R.digest_ints(words)
    big = np.random.RandomState(0).standard_normal(1000003).astype(np.float32)
    assert C.digest(big) == 0xc09b49ea2da1ee6d == R.digest(big)
    assert C.digest(torch.from_numpy(big)) == 0xc09b49ea2da1ee6d
    with pytest.raises(ValueError):
        C.digest(np.zeros(3, np.uint8))


def test_digest_sees_swaps_flips_and_appended_zeros():
    from iaf_amd import checkpoint as C
    w = np.random.RandomState(1).randint(0, 1 << 32, size=257, dtype=np.uint64).astype(np.uint32)
    base = C.digest(w)
    assert base == R.digest(w) == R.digest_ints(w)
    for a, b in ((0, 1), (5, 200), (255, 256)):
        assert w[a] != w[b]
        s = w.copy()
        s[a], s[b] = w[b], w[a]
        assert C.digest(s) != base and C.digest(s) == R.digest_ints(s)
    for i, bit in ((0, 0), (100, 31), (256, 17)):
        f = w.copy()
        f[i] ^= np.uint32(1 << bit)
        assert C.digest(f) != base
    grown = np.concatenate([w, np.zeros(1, np.uint32)])
    assert C.digest(grown) != base and C.digest(grown) == R.digest_ints(grown)
    assert C.digest(w[:-1]) != base


# -- the file -----------------------------------------------------------------------------------------------------------------------------
def test_round_trip_and_meta(saved):
    import iaf_amd
    ts, path = saved["ts"], saved["path"]
    ck = iaf_amd.load_checkpoint(path)
    for k in FLAT:
        np.testing.assert_array_equal(np.asarray(ck.arrays[k]), saved["state"][k].numpy())
    m = ck.meta
    assert json.loads(json.dumps(m, allow_nan=False)) == m                   # JSON-clean
    assert m["version"] == 1 and m["steps"] == 3 and m["skipped"] == 1 and m["global_step"] == 2
    assert m["noise_step"] is None and m["data_step"] is None and m["noise"] is None and m["data"] is None
    assert m["batch_size"] is None and m["world"] == 1 and m["towers"] == 1
    assert (m["lr"], m["beta1"], m["beta2"], m["eps"], m["ema_decay"]) == (LR, 0.9, 0.999, 1e-8, 0.999)
    assert m["moved"] == [] and m["range_objects"] == 0 and m["model"] == {}
    lay = m["layout"]
    assert [v["name"] for v in lay["variables"]] == HostModel.NAMES
    assert [tuple(v["shape"]) for v in lay["variables"]] == HostModel.SHAPES
    assert [v["offset"] for v in lay["variables"]] == [ts.flat.offset_of(k)[0] for k in HostModel.NAMES]
    assert lay["total_words"] == ts.flat.params.numel()
    for k in FLAT:
        assert int(m["digests"][k], 16) == R.digest(saved["state"][k].numpy())
    # the named views
    p, e, (sm, sv) = ck.params(), ck.ema_params(), ck.slots()
    for k, shape in zip(HostModel.NAMES, HostModel.SHAPES):
        lo, hi = ts.flat.offset_of(k)
        for got, flat in ((p, "params"), (e, "ema"), (sm, "slot_m"), (sv, "slot_v")):
            assert got[k].shape == shape
            np.testing.assert_array_equal(got[k].reshape(-1), saved["state"][flat].numpy()[lo:hi])
    t = ck.ema_params(device="cpu")
    assert all(torch.is_tensor(t[k]) and t[k].dtype == torch.float32 and torch.equal(t[k], torch.from_numpy(np.array(e[k])))
               for k in HostModel.NAMES)
    assert not os.path.exists(path + ".tmp")


def test_the_file_reads_with_the_independent_reader_and_the_other_way_round(saved, tmp_path):
    import iaf_amd
    meta, arrays = R.read(saved["path"])
    _, offs = R.offsets(saved["path"])
    assert all(o % 64 == 0 for o, _ in offs.values())
    assert open(saved["path"], "rb").read(8) == b"IAFCKPT1"
    for k in FLAT:
        np.testing.assert_array_equal(arrays[k], saved["state"][k].numpy())
        assert int(meta["digests"][k], 16) == R.digest(arrays[k])
    # a file from the independent writer, with other numbers, loads through the product and restores
    rng = np.random.RandomState(9)
    mine = [rng.standard_normal(meta["layout"]["total_words"]).astype(np.float32) for _ in FLAT]
    m2 = dict(meta, steps=11, skipped=4, global_step=7, digests={k: hex(R.digest(a)) for k, a in zip(FLAT, mine)})
    other = str(tmp_path / "other.ckpt")
    R.write(other, m2, mine)
    ck = iaf_amd.load_checkpoint(other)
    for k, a in zip(FLAT, mine):
        np.testing.assert_array_equal(np.asarray(ck.arrays[k]), a)
    ts = _step(seed=5)
    ts.restore(ck)
    for k, a in zip(FLAT, mine):
        np.testing.assert_array_equal(getattr(ts.flat, k).numpy(), a)
    assert (ts.steps, ts.skipped, ts.global_step) == (11, 4, 7)


def test_save_checkpoint_and_reuse_of_a_snapshot(saved, tmp_path):
    import iaf_amd
    ts = _step()
    for t in range(3):
        ts(*_batch(t))
    a, b = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    iaf_amd.save_checkpoint(ts, a)
    assert open(a, "rb").read() == open(saved["path"], "rb").read()         # the same run, the same bytes
    snap = ts.snapshot()
    ts(*_batch(3))
    assert ts.snapshot(into=snap) is snap
    snap.save(b)
    ck = iaf_amd.load_checkpoint(b)
    assert ck.meta["steps"] == 4
    np.testing.assert_array_equal(np.asarray(ck.arrays["params"]), ts.flat.params.numpy())
    with pytest.raises(ValueError):
        ts.snapshot(into=iaf_amd.Snapshot(ts.flat.params.numel() + 4, "cpu"))
    with pytest.raises(ValueError):
        ts.snapshot(into="snap")


# -- errors -------------------------------------------------------------------------------------------------------------------------------
def _refused(path, exc, tmp_path):
    """load_checkpoint and restore both refuse `path` with `exc`; the step is untouched and no .tmp file is about"""
    import iaf_amd
    ts = _step(seed=7)
    ts(*_batch(0))
    before = _state(ts)
    with pytest.raises(exc):
        iaf_amd.load_checkpoint(path)
    with pytest.raises(exc):
        ts.restore(path)
    assert _unchanged(ts, before) and ts.steps == 1
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]


def test_truncated_wrong_magic_wrong_version(saved, tmp_path):
    from iaf_amd import _capi
    blob = open(saved["path"], "rb").read()
    meta, offs = R.offsets(saved["path"])
    cases = {"short": blob[:-4], "header_only": blob[:offs["params"][0]], "inside_header": blob[:40], "tiny": blob[:7],
             "magic": b"IAFCKPT2" + blob[8:], "empty": b""}
    for name, data in cases.items():
        p = str(tmp_path / (name + ".ckpt"))
        open(p, "wb").write(data)
        _refused(p, ValueError, tmp_path)
    _, arrays = R.read(saved["path"])
    p = str(tmp_path / "version.ckpt")
    R.write(p, dict(meta, version=2), [arrays[k] for k in FLAT])
    _refused(p, ValueError, tmp_path)
    assert not issubclass(_capi.IafHipError, ValueError)                     # (the two kinds of refusal stay apart)


@pytest.mark.parametrize("which", FLAT)
def test_one_flipped_byte_in_each_array_is_caught(saved, tmp_path, which):
    import iaf_amd
    blob = bytearray(open(saved["path"], "rb").read())
    _, offs = R.offsets(saved["path"])
    off, nb = offs[which]
    blob[off + nb // 2] ^= 0x10
    p = str(tmp_path / ("flip_%s.ckpt" % which))
    open(p, "wb").write(bytes(blob))
    _refused(p, iaf_amd.IafHipError, tmp_path)
    ck = iaf_amd.load_checkpoint(p, verify=False)                            # (unverified, the file loads -- and restore still refuses it)
    ts = _step(seed=7)
    before = _state(ts)
    with pytest.raises(iaf_amd.IafHipError):
        ts.restore(ck)
    assert _unchanged(ts, before)


def test_save_verifies_the_bytes_it_writes(tmp_path):
    import iaf_amd
    ts = _step()
    ts(*_batch(0))
    snap = ts.snapshot()
    snap.bufs[2][3] += 1.0                                                   # the staging buffer altered behind the digest
    p = str(tmp_path / "torn.ckpt")
    with pytest.raises(iaf_amd.IafHipError):
        snap.save(p)
    assert os.listdir(str(tmp_path)) == []
    snap.save(p, verify=False)
    with pytest.raises(iaf_amd.IafHipError):
        iaf_amd.load_checkpoint(p)


class OtherModel(HostModel):
    NAMES = ["top/V", "top/g", "mid/even", "bottom/b"]


class WiderModel(HostModel):
    SHAPES = [(3, 4), (5,), (7,), (3,)]


class TowerModel(HostModel):
    towers = 2


@pytest.mark.parametrize("cls", [OtherModel, WiderModel, TowerModel], ids=["names", "shapes", "towers"])
def test_restore_into_another_variable_set_or_towers(saved, cls):
    import iaf_amd
    ts = iaf_amd.TrainStep(cls(seed=3), LR, graph=False)
    before = _state(ts)
    with pytest.raises(ValueError) as e:
        ts.restore(saved["path"])
    assert "not this step's" in str(e.value)
    assert _unchanged(ts, before) and ts.steps == 0 and ts.skipped == 0


def test_restore_refuses_counters_without_their_objects_and_bad_moved(saved):
    import iaf_amd
    ck = iaf_amd.load_checkpoint(saved["path"])
    ts = _step()
    before = _state(ts)
    for change in (dict(noise_step=5), dict(data_step=2), dict(moved=[0]), dict(moved="all"), dict(world=2), dict(steps=-1)):
        bad = iaf_amd.Checkpoint(dict(ck.meta, **change), ck.arrays)
        with pytest.raises(ValueError):
            ts.restore(bad)
        assert _unchanged(ts, before)


# -- resume -------------------------------------------------------------------------------------------------------------------------------
def test_resume_on_host_replicas_is_exact(saved):
    a = _step(seed=3)
    for t in range(3):
        a(*_batch(t))                                      # call 1 skipped
    assert _unchanged(a, saved["state"])                   # the saved run took and saved a snapshot here: that moved nothing
    for t in range(3, 6):
        a(*_batch(t))                                      # call 4 skipped
    b = _step(seed=3)
    b.restore(saved["path"])
    assert _unchanged(b, saved["state"])
    assert (b.steps, b.skipped, b.global_step) == (3, 1, 2)
    for t in range(3, 6):
        b(*_batch(t))
    for k in FLAT:
        assert torch.equal(getattr(a.flat, k), getattr(b.flat, k)), k
    assert (a.steps, a.skipped, a.global_step) == (6, 2, 4) == (b.steps, b.skipped, b.global_step)
    # roll back: the step that ran on is put back to the save and runs the same three steps again
    a.restore(saved["path"])
    assert (a.steps, a.skipped, a.global_step) == (3, 1, 2)
    for t in range(3, 6):
        a(*_batch(t))
    for k in FLAT:
        assert torch.equal(getattr(a.flat, k), getattr(b.flat, k)), k
    assert (a.steps, a.skipped, a.global_step) == (6, 2, 4)


def test_a_restored_step_starts_its_summaries_record_afresh(saved):
    """(the record is not part of a checkpoint) -- on a step without summaries restore has nothing to reset and says nothing"""
    b = _step(seed=3)
    b.restore(saved["path"])
    with pytest.raises(RuntimeError):
        b.summaries()
