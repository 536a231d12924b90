"""CPU checks of iaf_amd.TrainStep (iaf_amd/train.py): argument validation, the guard's decision on host replicas -- one process,
and a world-2 gloo run in which only rank 1's gradient, or only rank 1's objective, is non-finite: both ranks skip that update
and their parameters stay identical -- and the build of the two new kernels (no scratch).  The model here is a small host
stand-in with CVAE1's training interface (completion_order / load / set_grad_buckets / prepare_weights / fb_begin / fb_segment)."""
import os
import shutil
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HostModel(object):
    """obj = 0.5 x[0] sum_k |p_k|^2 + x[1];  d obj / d p_k = x[0] p_k, plus noise[0] on the gradient of "mid/odd"""
    NAMES = ["top/V", "top/g", "mid/odd", "bottom/b"]
    SHAPES = [(3, 4), (5,), (7,), (2,)]

    def __init__(self, seed=3):
        rng = np.random.RandomState(seed)
        self.params = {k: torch.from_numpy(rng.standard_normal(s)).float() for k, s in zip(self.NAMES, self.SHAPES)}
        self._buckets = [list(self.NAMES)]
        self.prepared = 0

    def completion_order(self):
        return list(self.NAMES)

    def load(self, params):
        self.params = params

    def set_grad_buckets(self, n_buckets=1):
        n = max(1, min(n_buckets, len(self.NAMES)))
        self._buckets = [self.NAMES[q * len(self.NAMES) // n:(q + 1) * len(self.NAMES) // n] for q in range(n)]
        return [list(b) for b in self._buckets]

    def prepare_weights(self):
        self.prepared += 1

    def fb_begin(self, x, noise, grads=None):
        self._fb = (x, noise, grads)
        obj = 0.5 * x[0] * sum((p * p).sum() for p in self.params.values()) + x[1]
        return {"obj": obj.reshape(1)}

    def fb_segment(self, i):
        x, noise, grads = self._fb
        for k in self._buckets[i]:
            g = x[0] * self.params[k]
            if k == "mid/odd":
                g = g + noise[0]
            grads[k].copy_(g)


def _clean(scale=1.0):
    return torch.tensor([scale, 0.25]), [torch.zeros(7)]


def test_argument_checks():
    import iaf_amd
    m = HostModel()
    for lr in (0, -1e-3, float("nan"), float("inf"), "1e-3", None, True):
        with pytest.raises(ValueError):
            iaf_amd.TrainStep(m, lr, graph=False)
    for nb in (0, -2, 1.5, True, "2"):
        with pytest.raises(ValueError):
            iaf_amd.TrainStep(m, 1e-3, n_buckets=nb, graph=False)
    with pytest.raises(ValueError):
        iaf_amd.TrainStep(m, 1e-3, graph="yes")
    with pytest.raises(ValueError):
        iaf_amd.TrainStep(m, 1e-3, graph=False, beta1=1.0)
    with pytest.raises(ValueError):
        iaf_amd.TrainStep(m, 1e-3)                         # graph=True (the default) needs device parameters
    unloaded = HostModel()
    unloaded.params = None
    with pytest.raises(RuntimeError):
        iaf_amd.TrainStep(unloaded, 1e-3, graph=False)


def test_one_process_steps_skip_exactly_the_non_finite_ones():
    import iaf_amd
    from iaf_amd import parallel as par
    m = HostModel()
    ts = iaf_amd.TrainStep(m, 0.01, n_buckets=3, graph=False)
    assert ts.n_buckets == 3 and ts.world == 1 and list(ts.flat.p) == HostModel.NAMES
    assert all(m.params[k].data_ptr() == ts.flat.p[k].data_ptr() for k in HostModel.NAMES)      # the model reads the flat views
    # the hand-composed step on a copy of the same state
    ref = par.FlatParams({k: v.clone() for k, v in ts.flat.p.items()})
    for step, (x, noise) in enumerate([_clean(1.0), (torch.tensor([1.0, float("nan")]), [torch.zeros(7)]), _clean(0.5),
                                       (torch.tensor([0.5, 0.0]), [torch.tensor([0.0] * 6 + [float("-inf")])]), _clean(2.0)]):
        before = {k: t.clone() for k, t in (("p", ts.flat.params), ("m", ts.flat.slot_m), ("v", ts.flat.slot_v), ("e", ts.flat.ema))}
        obj = ts(x, noise)
        finite = bool(torch.isfinite(x).all()) and bool(torch.isfinite(noise[0]).all())
        assert bool(torch.isfinite(obj).all()) == bool(torch.isfinite(x[1]) and torch.isfinite(x[0]))
        if finite:
            for k in HostModel.NAMES:
                ref.g[k].copy_(ts.flat.g[k])
            ref.adamax_ema_step(0.01)
            assert torch.equal(ts.flat.params, ref.params) and torch.equal(ts.flat.ema, ref.ema)
            assert not torch.equal(ts.flat.params, before["p"])
        else:
            for k, t in (("p", ts.flat.params), ("m", ts.flat.slot_m), ("v", ts.flat.slot_v), ("e", ts.flat.ema)):
                assert torch.equal(t, before[k]), (step, k)
    assert ts.skipped == 2
    assert m.prepared == 5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, case, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import iaf_amd
    ts = iaf_amd.TrainStep(HostModel(seed=3), 0.01, n_buckets=2, graph=False)     # identical initial parameters on every rank
    snaps = []
    for step in range(4):
        x, noise = _clean(1.0 + rank + step)                # rank-specific batches
        if step == 2 and rank == 1:
            if case == "grad":                              # one gradient element non-finite on rank 1 only; its objective is finite
                noise = [torch.tensor([0.0, 0.0, float("nan"), 0.0, 0.0, 0.0, 0.0])]
            else:                                           # rank 1's objective non-finite, every gradient finite
                x = torch.tensor([1.0 + rank + step, float("inf")])
        ts(x, noise)
        snaps.append(dict(params=ts.flat.params.numpy().copy(), ema=ts.flat.ema.numpy().copy(), m=ts.flat.slot_m.numpy().copy(),
                          v=ts.flat.slot_v.numpy().copy(), world=ts.world))
    out[rank] = dict(snaps=snaps, skipped=ts.skipped)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", ["grad", "obj"])
def test_two_ranks_gloo_one_ranks_non_finite_step_is_skipped_on_both(case):
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), case, out), nprocs=world, join=True)
    for r in range(world):
        assert out[r]["skipped"] == 1, (case, r, out[r]["skipped"])
        s = out[r]["snaps"]
        assert s[0]["world"] == 2
        for k in ("params", "ema", "m", "v"):
            np.testing.assert_array_equal(s[2][k], s[1][k])              # the poisoned step moved nothing
        assert not np.array_equal(s[1]["params"], s[0]["params"]) and not np.array_equal(s[3]["params"], s[2]["params"])
        assert np.isfinite(s[3]["params"]).all() and np.isfinite(s[3]["ema"]).all()
    for step in range(4):
        for k in ("params", "ema", "m", "v"):
            np.testing.assert_array_equal(out[0]["snaps"][step][k], out[1]["snaps"][step][k])     # replicas stay identical


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_guard_kernels_use_no_scratch(tmp_path):
    """the scan and the gated update keep their state in registers (hipcc's kernel-resource-usage remarks, device code only, of a unit
    that includes just the small kernels' header -- seconds instead of the whole engine)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    src = tmp_path / "guard_kernels.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "iaf_conv_kernel.hpp"\n#include "iaf_kernels_train.hpp"\n')
    rows = [r for r in kr.unit_resources(str(src), str(tmp_path / "guard_kernels.o"), [])
            if "nonfinite_scan" in r["name"] or "adamax_ema_guarded" in r["name"]]
    assert len(rows) == 2, [r["name"] for r in rows]
    bad = [(r["name"], r.get("scratch"), r.get("vspill")) for r in rows if r.get("scratch", 0) or r.get("vspill", 0)]
    assert not bad, bad
