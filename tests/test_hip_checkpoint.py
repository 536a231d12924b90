"""GPU tests of the checkpoints (iaf_amd/checkpoint.py, TrainStep.snapshot / restore) on the case
tests/test_hip_train_step.py trains (model_cfg, B = 2), with a noise source and a 6-image device dataset in the captured step: an exact
resume across a save -- the snapshot taken in the stream, the file written three steps later --, a run with a snapshot after every step
against one with none, a roll back, evaluation of the EMA from a file, the objects a checkpoint lists as moved to bf16 planes, and an
upload that does not arrive as written.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
import state_reference as R

pytestmark = pytest.mark.gpu

LR = 2e-3
SEED = 2024
FLAT = ("params", "slot_m", "slot_v", "ema")


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()
    return iaf_amd


@pytest.fixture(scope="module")
def case():
    c = gi.model_case_inputs("model_cfg")
    S = c["image_size"]
    images = np.random.RandomState(11).randint(0, 256, size=(6, 3, S, S)).astype(np.uint8)
    return dict(c=c, B=c["B"], images=torch.from_numpy(images).cuda())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _kw(c):
    return dict(z_size=c["z_size"], h_size=c["h_size"], kl_min=c["kl_min"], depth=c["depth"], num_blocks=c["num_blocks"],
                image_size=c["image_size"])


def make(amd, case, graph=True, plain=False):
    """a fresh model, source, dataset and step from the case's initial variables (plain: a step without source and dataset)"""
    c = case["c"]
    model = amd.CVAE1(k=1, **_kw(c))
    model.set_training(True)
    model.load({k: dev(v) for k, v in c["params"].items()})
    if plain:
        return amd.TrainStep(model, LR, graph=graph), None, None
    src, ds = amd.NoiseSource(SEED), amd.DeviceDataset(case["images"], SEED)
    ts = amd.TrainStep(model, LR, graph=graph, noise_source=src, data=ds, batch_size=case["B"])
    return ts, src, ds


def state(ts):
    torch.cuda.synchronize()
    return {k: getattr(ts.flat, k).clone() for k in FLAT}


def same(a, b, what):
    for k in FLAT:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))


def resume_runs(amd, case, graph, path):
    """run A: 3 steps, a snapshot, 3 more steps with nothing in between, and only then the file.  Run B: a fresh step that restores the
    file and takes 3 steps.  Run C: a fresh step that stops after step 3."""
    ts, src, ds = make(amd, case, graph)
    for _ in range(3):
        ts()
    snap = ts.snapshot()
    objs = [ts().clone() for _ in range(3)]
    snap.save(path)
    a = dict(state=state(ts), objs=objs, tells=(src.tell(), ds.tell()), steps=ts.steps, global_step=ts.global_step, skipped=ts.skipped,
             graphed=ts.graphed, captures=ts.captures)
    tb, srcb, dsb = make(amd, case, graph)
    tb.restore(path)
    at_restore = state(tb)
    objs = [tb().clone() for _ in range(3)]
    b = dict(state=state(tb), objs=objs, tells=(srcb.tell(), dsb.tell()), steps=tb.steps, global_step=tb.global_step, skipped=tb.skipped,
             graphed=tb.graphed, captures=tb.captures, at_restore=at_restore)
    tc, srcc, dsc = make(amd, case, graph)
    for _ in range(3):
        tc()
    c = dict(state=state(tc), tells=(srcc.tell(), dsc.tell()))
    return a, b, c


def check_resume(amd, a, b, c, path, graph):
    same(a["state"], b["state"], "A against B")
    for t, (x, y) in enumerate(zip(a["objs"], b["objs"])):
        assert torch.equal(x, y), (t, float(x), float(y))
    assert a["tells"] == b["tells"] == (6, 6)
    assert (a["steps"], a["global_step"], a["skipped"]) == (b["steps"], b["global_step"], b["skipped"]) == (6, 6, 0)
    assert a["graphed"] == b["graphed"] == graph
    if graph:
        assert a["captures"] == b["captures"] == 1                   # neither the snapshot nor the restore made a capture necessary
    # the file holds the state at the snapshot's place in the stream (after step 3), not the state at save time (after step 6)
    ck = amd.load_checkpoint(path)
    for k in FLAT:
        assert np.array_equal(np.asarray(ck.arrays[k]).view(np.uint32), c["state"][k].cpu().numpy().view(np.uint32)), k
        assert not torch.equal(c["state"][k], a["state"][k]), k
        assert int(ck.meta["digests"][k], 16) == R.digest(c["state"][k].cpu().numpy())
    same(b["at_restore"], c["state"], "B at its restore against C")
    m = ck.meta
    assert (m["steps"], m["skipped"], m["global_step"], m["noise_step"], m["data_step"]) == (3, 0, 3, 3, 3) and c["tells"] == (3, 3)
    assert m["noise"] == dict(seed=SEED, substream_base=0) and m["data"] == dict(seed=SEED, n=6, deterministic=False, world=1)
    assert (m["batch_size"], m["world"], m["towers"], m["lr"], m["moved"]) == (2, 1, 1, LR, [])
    assert sorted(m["model"]) == sorted(["z_size", "h_size", "depth", "num_blocks", "k", "image_size", "kl_min", "depth_ar"])
    assert all(m["model"][k] == v for k, v in dict(z_size=32, h_size=160, depth=2, num_blocks=2, k=1, image_size=32, kl_min=0.25).items())


@pytest.fixture(scope="module")
def graph_runs(amd, case, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ckpt") / "graph.ckpt")
    a, b, c = resume_runs(amd, case, True, path)
    return dict(a=a, b=b, c=c, path=path)


def test_exact_resume_in_a_captured_step(amd, graph_runs):
    g = graph_runs
    check_resume(amd, g["a"], g["b"], g["c"], g["path"], True)


def test_exact_resume_with_eager_launches(amd, case, tmp_path):
    path = str(tmp_path / "eager.ckpt")
    a, b, c = resume_runs(amd, case, False, path)
    check_resume(amd, a, b, c, path, False)


def test_the_file_reads_with_the_independent_reader(amd, graph_runs):
    """the product's file through the independent reader: the arrays at 64-byte boundaries, the digests the numpy restatement's"""
    meta, arrays = R.read(graph_runs["path"])
    _, offs = R.offsets(graph_runs["path"])
    assert all(o % 64 == 0 for o, _ in offs.values())
    for k in FLAT:
        assert np.array_equal(arrays[k].view(np.uint32), graph_runs["c"]["state"][k].cpu().numpy().view(np.uint32))
        assert int(meta["digests"][k], 16) == R.digest(arrays[k])


def test_a_snapshot_after_every_step_changes_nothing(amd, case, graph_runs, monkeypatch):
    """it only reads: the run it is taken from is the run without it (run C took 3 steps and no snapshot)"""
    ts, src, ds = make(amd, case, True)
    snap = None
    for t in range(3):
        ts()
        snap = ts.snapshot(into=snap)
        assert snap.steps == t + 1
    same(state(ts), graph_runs["c"]["state"], "with snapshots against without")
    assert (src.tell(), ds.tell()) == (3, 3) and ts.captures == 1 and ts.skipped == 0
    for b, k in zip(snap.bufs, FLAT):
        assert torch.equal(b, graph_runs["c"]["state"][k]), k                  # and the last snapshot is that state
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError):                                          # not while the current stream captures
        ts.snapshot(into=snap)


def test_roll_back_equals_a_fresh_restore(amd, case, graph_runs):
    ts, src, ds = make(amd, case, True)
    for _ in range(2):
        ts()
    ts.restore(graph_runs["path"])
    assert (ts.steps, ts.skipped, ts.global_step, src.tell(), ds.tell()) == (3, 0, 3, 3, 3)
    same(state(ts), graph_runs["b"]["at_restore"], "at the restore")
    objs = [ts().clone() for _ in range(3)]
    same(state(ts), graph_runs["b"]["state"], "rolled back against freshly restored")
    for x, y in zip(objs, graph_runs["b"]["objs"]):
        assert torch.equal(x, y)
    assert (ts.steps, ts.global_step, src.tell(), ds.tell()) == (6, 6, 6, 6)
    assert ts.captures == 1                                                    # the graph reads the buffers where they are


def test_evaluation_from_a_file_equals_evaluation_of_the_live_average(amd, case, tmp_path):
    c, B = case["c"], case["B"]

    def evaluate(params):
        m = amd.CVAE1(k=1, **_kw(c))
        m.load(params)
        return amd.EvalPass(m, amd.DeviceDataset(case["images"], 1, deterministic=True), B, amd.NoiseSource(7)).run()
    ts, _, _ = make(amd, case, True)
    for _ in range(3):
        ts()
    snap = ts.snapshot()
    live = evaluate(ts.ema_params())                                           # the average as it stands at the snapshot
    ts()                                                                       # ... and it moves on before the file is written
    path = str(tmp_path / "eval.ckpt")
    snap.save(path)
    ck = amd.load_checkpoint(path)
    loaded = ck.ema_params(device="cuda")
    assert all(v.is_cuda and v.dtype == torch.float32 for v in loaded.values()) and list(loaded) == list(ts.flat.p)
    got = evaluate(loaded)
    assert got == live and got["images"] == 6 and got["nonfinite"] == 0 and np.isfinite(got["loss"])
    assert evaluate(ts.ema_params())["loss"] != live["loss"]
    p = ck.params(device="cuda")
    assert all(tuple(p[k].shape) == tuple(ts.flat.p[k].shape) for k in p)


def _probe(o):
    """True if the object would run on two fp16 planes at one of the case's sizes (a stack's one-launch step, a conv's forward launch)"""
    if hasattr(o, "step_is_f16"):
        return any(o.step_is_f16(2, h, h) for h in (16, 8))
    return any(o.runs_f16x2(32, h, h) for h in (32, 16, 8))


def test_the_objects_a_checkpoint_lists_as_moved_are_moved(amd, case, graph_runs):
    ck = amd.load_checkpoint(graph_runs["path"])
    ts, _, _ = make(amd, case, True)
    objs = ts._objects
    before = [_probe(o) for o in objs]
    stacks = [i for i, o in enumerate(objs) if hasattr(o, "step_is_f16") and before[i]]
    convs = [i for i, o in enumerate(objs) if not hasattr(o, "step_is_f16") and before[i]]
    assert stacks and convs, "the case has no stack / conv on fp16 planes: the test would show nothing"
    moved = [stacks[0], convs[-1]]
    assert ck.meta["range_objects"] == len(objs)
    ck.meta["moved"] = sorted(moved)
    ts.restore(ck)
    after = [_probe(o) for o in objs]                                          # before any step
    assert objs[stacks[0]].step_is_f16(2, 16, 16) is False
    for i, (x, y) in enumerate(zip(before, after)):
        assert y == (x and i not in moved), (i, x, y)
    assert ts._seen == set(moved) and not ts._stale and not ts.graphed        # no graph yet: the first call captures anyway
    obj = ts().clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(obj).all()) and ts.graphed and ts.captures == 1 and ts.skipped == 0
    assert all(o.range_errors() == 0 for o in objs)                            # no overflow was provoked
    # a step that already replays a graph: the graph is captured again before its next replay
    t2, _, _ = make(amd, case, True)
    t2()
    assert t2.graphed and not t2._stale
    t2.restore(ck)
    assert t2._stale and t2._seen == set(moved)
    t2()
    torch.cuda.synchronize()
    assert t2.captures == 2 and t2.graphed and not t2._stale
    # and the file a moved step writes says so
    assert t2.snapshot().meta([0, 0, 0, 0], np.zeros(8, np.uint32))["moved"] == sorted(moved)


def test_an_upload_that_does_not_arrive_as_written_is_refused(amd, case, graph_runs):
    ck = amd.load_checkpoint(graph_runs["path"])
    ts, src, ds = make(amd, case, True)
    ts()
    before = state(ts)
    ck.arrays["slot_v"][12345] += 1.0                                          # altered in memory after loading (the file is not touched)
    with pytest.raises(amd.IafHipError):
        ts.restore(ck)
    same(state(ts), before, "after the refused restore")
    assert (ts.steps, src.tell(), ds.tell()) == (1, 1, 1)
    amd.load_checkpoint(graph_runs["path"])                                    # (still verifies)
    other = make(amd, case, False, plain=True)[0]                              # a step without source and dataset
    with pytest.raises(ValueError):
        other.restore(graph_runs["path"])
