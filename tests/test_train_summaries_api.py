"""CPU checks of TrainStep(summaries=True) (iaf_amd/train.py): argument validation, the summaries of host replicas (a small host
stand-in with CVAE1's training interface whose fb_begin returns "terms") against the same numbers worked out by hand in fp64 -- one
process, with a skipped step, and a world-2 gloo run in which the ranks' losses differ -- a stand-in without "terms", and the build
of the two new kernels (no scratch, no spills)."""
import math
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

S, N, LAYERS = 4, 3, [(1, 1), (1, 0), (0, 0)]          # image size, batch rows, the (i, j) of the table rows (top-down)


class HostModel(object):
    """obj = 0.5 x[0] sum_k |p_k|^2 + x[1], d obj / d p_k = x[0] p_k (+ noise[0] on "mid/odd"); its terms are made up from x so that
    every field differs: layer_obj[l][b] = x[0] (l + 1) + b, layer_cost[l][b] = layer_obj[l][b] / 2 - l, log_pxz[b] = -(3 + b) x[0],
    loss = sum_b (sum_l layer_cost[l][b] - log_pxz[b])"""
    NAMES = ["dec_log_stdv", "top/V", "mid/odd", "bottom/b"]
    SHAPES = [(), (3, 4), (7,), (2,)]
    image_size = S

    def __init__(self, seed=3):
        rng = np.random.RandomState(seed)
        self.params = {k: torch.from_numpy(np.asarray(rng.standard_normal(s))).float() for k, s in zip(self.NAMES, self.SHAPES)}
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

    @staticmethod
    def terms_of(x0):
        """(layer_obj, layer_cost, log_pxz, loss) as fp64 arrays for x[0] = x0"""
        b = np.arange(N, dtype=np.float64)
        lo = np.stack([x0 * (l + 1) + b for l in range(len(LAYERS))])
        lc = np.stack([lo[l] / 2 - l for l in range(len(LAYERS))])
        lp = -(3 + b) * x0
        return lo, lc, lp, float((lc.sum(axis=0) - lp).sum())

    def fb_begin(self, x, noise, grads=None, terms=False):
        self._fb = (x, noise, grads)
        obj = 0.5 * x[0] * sum((p * p).sum() for p in self.params.values()) + x[1]
        out = {"obj": obj.reshape(1)}
        if terms:
            lo, lc, lp, loss = self.terms_of(float(x[0]))
            out["terms"] = dict(layer_obj=torch.from_numpy(lo).float(), layer_cost=torch.from_numpy(lc).float(),
                                log_pxz=torch.from_numpy(lp).float(), loss=torch.tensor([loss], dtype=torch.float32), layers=list(LAYERS))
        return out

    def fb_segment(self, i):
        x, noise, grads = self._fb
        for k in self._buckets[i]:
            g = x[0] * self.params[k]
            if k == "mid/odd":
                g = g + noise[0]
            grads[k].copy_(g)


class NoTermsKeyword(HostModel):
    def fb_begin(self, x, noise, grads=None):
        return HostModel.fb_begin(self, x, noise, grads)


class NoTermsReturned(HostModel):
    def fb_begin(self, x, noise, grads=None, terms=False):
        return HostModel.fb_begin(self, x, noise, grads, terms=False)


def _clean(scale=1.0):
    return torch.tensor([scale, 0.25]), [torch.zeros(7)]


def _want(x0, loss_all, dec, grads, world):
    """the summaries of one step by hand: fp64 means of the fp32 terms"""
    lo, lc, lp, _ = HostModel.terms_of(x0)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    lo, lc, lp = f(lo), f(lc), f(lp)
    out = {"model/bits_per_dim": loss_all / (math.log(2.) * 3 * S * S * N * world), "model/dec_log_stdv": dec,
           "model/log_pxz": -lp.mean(), "model/kl_obj": lo.mean(axis=1).sum(), "model/kl_cost": lc.mean(axis=1).sum(),
           "grad_norm": float(np.sqrt((grads.astype(np.float64) ** 2).sum())) / world}
    for r, (i, j) in enumerate(LAYERS):
        out["model/kl_obj_%02d_%02d" % (i, j)] = lo[r].mean()
        out["model/kl_cost_%02d_%02d" % (i, j)] = lc[r].mean()
    return out


def _close(got, want, what):
    assert sorted(got) == sorted(list(want) + ["steps", "skipped"]), (what, sorted(got))
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-12 * max(1.0, abs(v)), (what, k, got[k], v)      # fp64 on both sides


def test_argument_checks():
    import iaf_amd
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError):
            iaf_amd.TrainStep(HostModel(), 1e-3, graph=False, summaries=bad)
    with pytest.raises(ValueError):
        iaf_amd.TrainStep(HostModel(), 1e-3, summaries=True)               # graph=True (the default) needs device parameters
    no_size = HostModel()
    no_size.image_size = None
    with pytest.raises(ValueError):
        iaf_amd.TrainStep(no_size, 1e-3, graph=False, summaries=True)
    ts = iaf_amd.TrainStep(HostModel(), 1e-3, graph=False)                 # the default: no summaries, and asking for them says so
    ts(*_clean())
    with pytest.raises(RuntimeError):
        ts.summaries()
    with pytest.raises(RuntimeError):
        ts.last_summaries()
    ts = iaf_amd.TrainStep(HostModel(), 1e-3, graph=False, summaries=True)
    with pytest.raises(RuntimeError):
        ts.summaries()                                                     # no step yet


def test_a_model_without_terms_raises():
    import iaf_amd
    with pytest.raises(ValueError):
        iaf_amd.TrainStep(NoTermsKeyword(), 1e-3, graph=False, summaries=True)
    ts = iaf_amd.TrainStep(NoTermsReturned(), 1e-3, graph=False, summaries=True)
    with pytest.raises(ValueError):
        ts(*_clean())
    iaf_amd.TrainStep(NoTermsKeyword(), 1e-3, graph=False)(*_clean())     # without summaries such a model trains as before


def test_one_process_summaries_are_the_means_of_the_accepted_steps():
    import iaf_amd
    ts = iaf_amd.TrainStep(HostModel(), 0.01, n_buckets=2, graph=False, summaries=True)
    plain = iaf_amd.TrainStep(HostModel(), 0.01, n_buckets=2, graph=False)
    steps = [_clean(1.0), (torch.tensor([1.5, float("nan")]), [torch.zeros(7)]), _clean(0.5),
             (torch.tensor([0.75, 0.0]), [torch.tensor([0.0] * 6 + [float("-inf")])]), _clean(2.0)]
    wants = []
    for t, (x, noise) in enumerate(steps):
        dec = float(ts.flat.p["dec_log_stdv"].double())
        ts(x, noise)
        plain(x, noise)
        assert torch.equal(ts.flat.params, plain.flat.params) and torch.equal(ts.flat.ema, plain.flat.ema)     # the update is untouched
        loss = float(np.float32(HostModel.terms_of(float(x[0]))[3]))
        want = _want(float(x[0]), loss, dec, ts.flat.grads.numpy(), 1)
        last = ts.last_summaries()
        if t == 3:                                            # the gradient holds -inf: its norm is not finite, the rest is readable
            assert not math.isfinite(last["grad_norm"])
            want.pop("grad_norm")
            last.pop("grad_norm")
        elif t != 1:                                          # (step 1: NaN objective, finite terms -- skipped, so not in the means)
            wants.append(want)
        _close(last, want, "step %d" % t)
    assert ts.skipped == 2
    got = ts.summaries(reset=False)
    assert (got["steps"], got["skipped"]) == (3, 2)
    _close(got, {k: sum(w[k] for w in wants) / 3 for k in wants[0]}, "means")
    again = ts.summaries()                                    # reset=True returns the same numbers, then zeroes the record
    assert again == got
    empty = ts.summaries()
    assert (empty["steps"], empty["skipped"]) == (0, 0)
    assert all(math.isnan(v) for k, v in empty.items() if k not in ("steps", "skipped"))
    ts(*_clean(3.0))
    one = ts.summaries()
    assert (one["steps"], one["skipped"]) == (1, 0) and math.isfinite(one["model/bits_per_dim"])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import iaf_amd
    ts = iaf_amd.TrainStep(HostModel(seed=3), 0.01, n_buckets=2, graph=False, summaries=True)
    x, noise = _clean(1.0 + rank)                             # rank-specific batches: the ranks' losses differ
    dec = float(ts.flat.p["dec_log_stdv"].double())
    ts(x, noise)
    out[rank] = dict(last=ts.last_summaries(), mean=ts.summaries(), grads=ts.flat.grads.numpy().copy(), dec=dec, world=ts.world)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_gloo_report_the_bits_per_dim_of_both_ranks_losses():
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    losses = [float(np.float32(HostModel.terms_of(1.0 + r)[3])) for r in range(world)]
    assert losses[0] != losses[1]
    bpd = float(np.float32(losses[0]) + np.float32(losses[1])) / (math.log(2.) * 3 * S * S * N * 2)
    for r in range(world):
        o = out[r]
        assert o["world"] == 2
        want = _want(1.0 + r, float(np.float32(losses[0]) + np.float32(losses[1])), o["dec"], o["grads"], 2)
        assert want["model/bits_per_dim"] == bpd
        _close(o["last"], want, "rank %d" % r)
        _close(o["mean"], want, "rank %d mean" % r)
        assert (o["mean"]["steps"], o["mean"]["skipped"]) == (1, 0)
    assert out[0]["last"]["model/bits_per_dim"] == out[1]["last"]["model/bits_per_dim"]
    assert out[0]["last"]["grad_norm"] == out[1]["last"]["grad_norm"]                 # the all-reduced gradient is the same on both


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_summary_kernels_use_no_scratch(tmp_path):
    """the fused scan and the summaries launch keep their state in registers and LDS (hipcc's kernel-resource-usage remarks, device
    code only, of a unit that includes just the small kernels' header)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    src = tmp_path / "summary_kernels.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "iaf_conv_kernel.hpp"\n#include "iaf_kernels_train.hpp"\n')
    rows = [r for r in kr.unit_resources(str(src), str(tmp_path / "summary_kernels.o"), [])
            if "guard_sumsq_scan" in r["name"] or "train_summaries_kernel" in r["name"]]
    assert len(rows) == 2, [r["name"] for r in rows]
    bad = [(r["name"], r.get("scratch"), r.get("vspill"), r.get("sspill")) for r in rows
           if r.get("scratch", 0) or r.get("vspill", 0) or r.get("sspill", 0)]
    assert not bad, bad
