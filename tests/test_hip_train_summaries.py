"""GPU tests of the training summaries (iaf_amd/train.py: TrainStep(summaries=True); include/iaf_hip.h: iaf_nonfinite_scan_sumsq,
iaf_train_summaries, iaf_train_summaries_reset): the fused scan against the plain scan (verdict) and a NumPy fp64 sum (sum of
squares, reproducible bit for bit, also in a replayed hipGraph), the summaries launch against NumPy fp64, and whole CVAE1 steps --
free bits at 30 nats so that the 8x8 layers clamp and kl_obj differs from kl_cost -- against the fp64 oracle evaluated on the very
parameters each step started from.

Tolerances.  sumsq: 1e-7 relative (squares of fp32 values are exact in fp64; n - 1 additions round by at most (n - 1) 2^-53 relative,
1.5e-8 up to 2^27 elements; the rest is margin).  The summaries launch: 1e-9 relative (fp32 inputs, fp64 arithmetic; no cancellation
in the test's data).  Model steps: 1e-4 relative, the project's tolerance for fp32 sums over thousands of elements (DESIGN.md
section 2); grad_norm 1e-7 relative of the fp64 norm of the step's own gradient buffer."""
import ctypes
import math

import numpy as np
import pytest
import torch

import golden_inputs as gi

pytestmark = pytest.mark.gpu

LR = 2e-3


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()
    return iaf_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Scan(object):
    """the buffers of one fused scan (guard, partials, sumsq) and of the plain scan beside it"""

    def __init__(self, amd):
        self.amd, self.lib = amd, amd._capi.lib()
        self.guard = torch.zeros(4, dtype=torch.int32, device="cuda")
        self.plain_guard = torch.zeros(4, dtype=torch.int32, device="cuda")
        self.partials = torch.full((2048,), float("nan"), dtype=torch.float64, device="cuda")      # (needs no initial value)
        self.sumsq = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")

    def fused(self, buf, extra=None):
        self.amd._capi.check(self.lib.iaf_nonfinite_scan_sumsq(ptr(buf), buf.numel(), ptr(extra), 0 if extra is None else extra.numel(),
                                                               ptr(self.guard), ptr(self.partials), ptr(self.sumsq), stream()))

    def plain(self, buf, extra=None):
        self.amd._capi.check(self.lib.iaf_nonfinite_scan(ptr(buf), buf.numel(), ptr(extra), 0 if extra is None else extra.numel(),
                                                         ptr(self.plain_guard), stream()))

    def verdicts(self, buf, extra=None):
        self.guard[0] = 7                                                        # (every scan writes its own verdict)
        self.fused(buf, extra)
        self.plain(buf, extra)
        torch.cuda.synchronize()
        assert self.guard[1:].tolist() == [0, 0, 0], self.guard.tolist()         # the arrival count is back to 0
        return int(self.guard[0].item()), int(self.plain_guard[0].item())

    def bits(self):
        torch.cuda.synchronize()
        return int(self.sumsq.view(torch.int64).item())


def _finite_data(n, seed):
    rng = np.random.RandomState(seed)
    base = rng.standard_normal(n).astype(np.float32)
    base[::7] = np.float32(1e25)                       # an fp32 accumulator overflows on the square of these ...
    base[1::5] = np.float32(-1e25)
    base[2::11] = np.float32(1e-25)                    # ... and flushes the square of these
    base[3::13] = np.float32(1e-40)                    # (subnormals are finite)
    return base


# -- the fused scan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1000003])
def test_fused_scan_gives_the_plain_scans_verdict(amd, n):
    sc = Scan(amd)
    base = _finite_data(n, n)
    extra = dev([1.0, -3.0e38])
    places = sorted({0, n - 1, max(0, n - 2), (n // 4) * 4 if (n // 4) * 4 < n else n - 1, n // 2})   # first, last, tail, middle
    for offset in (0, 1):                              # 1: a view 4 bytes off the 16-byte grid (every element through the scalar path)
        big = dev(np.concatenate([np.zeros(offset, np.float32), base]))
        buf = big[offset:]
        assert (buf.data_ptr() % 16 != 0) == bool(offset)
        assert sc.verdicts(buf, extra) == (0, 0), (n, offset)
        for bad in (float("nan"), float("inf"), float("-inf")):
            for i in places:
                keep = float(buf[i].item())
                buf[i] = bad
                assert sc.verdicts(buf, extra) == (1, 1), (n, offset, bad, i)
                buf[i] = keep
            assert sc.verdicts(buf, extra) == (0, 0), (n, offset, bad)         # cleared again by the next scan
            e = np.array([1.0, -3.0e38], np.float32)
            e[1] = bad
            assert sc.verdicts(buf, dev(e)) == (1, 1), (n, offset, bad, "extra")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1000003])
def test_fused_scan_sum_of_squares_is_fp64_and_reproducible(amd, n):
    sc = Scan(amd)
    for what, base in (("wide", _finite_data(n, n)), ("normal", np.random.RandomState(n + 1).standard_normal(n).astype(np.float32))):
        want = float(np.sum(base.astype(np.float64) ** 2))
        assert np.isfinite(want) and (what == "normal" or want > 1e49)         # (1e49: beyond any fp32 accumulator)
        for offset in (0, 1):
            big = dev(np.concatenate([np.zeros(offset, np.float32), base]))
            buf = big[offset:]
            sc.fused(buf)
            first = sc.bits()
            got = float(sc.sumsq.item())
            rel = abs(got - want) / want
            print("n %d %s offset %d: sumsq %.17g, relative error %.3g" % (n, what, offset, got, rel))
            assert rel <= 1e-7, (n, what, offset, got, want)
            sc.sumsq.fill_(-1.0)
            sc.fused(buf)
            assert sc.bits() == first, (n, what, offset)                       # a second launch: the same bits
            assert int(sc.guard[0].item()) == 0


def test_fused_scan_in_a_replayed_graph_repeats_its_bits(amd):
    sc = Scan(amd)
    n = 1000003
    base = _finite_data(n, 5)
    buf = dev(base)
    sc.fused(buf)
    eager = sc.bits()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            sc.fused(buf)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for r in range(3):
        sc.sumsq.fill_(-1.0)
        g.replay()
        assert sc.bits() == eager, r
        assert sc.guard.tolist() == [0, 0, 0, 0], r
    buf[n // 2] = float("nan")                                                 # the next replay judges the buffer as it is then
    g.replay()
    torch.cuda.synchronize()
    assert sc.guard.tolist() == [1, 0, 0, 0] and not math.isfinite(float(sc.sumsq.item()))
    del g


# -- the summaries launch ---------------------------------------------------------------------------------------------------------
def _fields(lo, lc, lp, dec, loss_all, sumsq, grad_scale):
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    lo, lc, lp = f(lo), f(lc), f(lp)
    mo, mc = lo.mean(axis=1), lc.mean(axis=1)
    head = [float(np.float32(loss_all)), float(np.float32(dec)), -lp.mean(), mo.sum(), mc.sum(), float(np.float32(grad_scale)) * math.sqrt(sumsq)]
    return np.concatenate([head, np.stack([mo, mc], axis=1).reshape(-1)])


@pytest.mark.parametrize("nl,n", [(4, 2), (20, 32), (3, 257)])
def test_summaries_launch_against_numpy(amd, nl, n):
    lib = amd._capi.lib()
    F = 6 + 2 * nl
    assert lib.iaf_train_summaries_bytes(nl) == (2 * F + 2) * 8
    assert lib.iaf_train_summaries_bytes(0) == 0 and lib.iaf_train_summaries_bytes(257) == 0
    rec = torch.full((2 * F + 2,), 3.0, dtype=torch.float64, device="cuda")
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    reset = lambda: amd._capi.check(lib.iaf_train_summaries_reset(ptr(rec), nl, stream()))
    reset()
    torch.cuda.synchronize()
    assert rec.view(torch.int64).abs().max().item() == 0
    rng = np.random.RandomState(nl * 1000 + n)
    total = np.zeros(F)
    steps = []
    for t in range(3):
        lo = (1000.0 + 50.0 * rng.standard_normal((nl, n))).astype(np.float32)      # positive, like a KL: the means do not cancel
        lc = (900.0 + 50.0 * rng.standard_normal((nl, n))).astype(np.float32)
        lp = (-7000.0 + 100.0 * rng.standard_normal(n)).astype(np.float32)
        dec, loss_all, sumsq, gs = -1.5 - t, 63362.1 + t, 12345.678 + t, 0.5
        steps.append((lo, lc, lp, dec, loss_all, sumsq, gs))
    def launch(step):
        lo, lc, lp, dec, loss_all, sumsq, gs = step
        keep = [dev(lo), dev(lc), dev(lp), dev([dec]), dev([loss_all]), torch.tensor([sumsq], dtype=torch.float64, device="cuda")]
        amd._capi.check(lib.iaf_train_summaries(*([ptr(k) for k in keep] + [gs, ptr(guard), ptr(rec), nl, n, stream()])))
        torch.cuda.synchronize()
        return rec.cpu()
    close = lambda got, want, what: np.testing.assert_allclose(got, want, rtol=1e-9, atol=0, err_msg=what)
    for t, step in enumerate(steps):
        host = launch(step)
        want = _fields(*step)
        total += want
        close(host[F:2 * F].numpy(), want, "last, step %d" % t)
        close(host[:F].numpy(), total, "acc, step %d" % t)
        assert host[2 * F:].view(torch.int64).tolist() == [t + 1, 0]
    # guard raised: acc untouched byte for byte, skipped counted, last written
    before = rec[:F].clone()
    guard[0] = 1
    lo, lc, lp, dec, loss_all, sumsq, gs = steps[0]
    host = launch((lc, lo, lp, 0.25, float("nan"), float("inf"), gs))
    assert torch.equal(rec[:F].view(torch.int64), before.view(torch.int64))
    assert host[2 * F:].view(torch.int64).tolist() == [3, 1]
    last = host[F:2 * F].numpy()
    assert math.isnan(last[0]) and last[1] == 0.25 and math.isinf(last[5])
    close(last[2:5], _fields(lc, lo, lp, 0.25, 0.0, 0.0, gs)[2:5], "last of the skipped step")
    close(last[6:], _fields(lc, lo, lp, 0.25, 0.0, 0.0, gs)[6:], "last of the skipped step, layers")
    reset()
    torch.cuda.synchronize()
    assert rec.view(torch.int64).abs().max().item() == 0


# -- the model step ---------------------------------------------------------------------------------------------------------------
KL_MIN = 30.0        # (the fixture's own 0.25 clamps no channel: every layer's kl_obj would equal its kl_cost and a swapped field pass)


@pytest.fixture(scope="module")
def case():
    c = dict(gi.model_case_inputs("model_cfg"))
    c["kl_min"] = KL_MIN
    return c


def _model(amd, c):
    model = amd.CVAE1(z_size=c["z_size"], h_size=c["h_size"], kl_min=c["kl_min"], depth=c["depth"], num_blocks=c["num_blocks"], k=1,
                      image_size=c["image_size"])
    model.set_training(True)
    model.load({k: dev(v) if isinstance(v, np.ndarray) else v.clone() for k, v in c["params"].items()})
    return model


def _inputs(c, step):
    """the inputs of tests/test_hip_train_step.py::_inputs"""
    x = torch.from_numpy(c["x"]).cuda()
    noise = [dev(np.roll(e, step, axis=0) * (1.0 + 0.05 * step)) for e in c["noise"]]
    return x, noise


def _oracle_summaries(c, flat_p, noise):
    """the step's terms in fp64 on the parameters the step starts from: the loop of oracle.iaf_oracle.cvae1_forward with every layer's
    values kept (tf_train.py:150-218), then the reference's summaries"""
    from oracle import iaf_oracle as O
    p = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in flat_p.items()}
    noise = [e.detach().cpu().numpy().astype(np.float64) for e in noise]
    depth, nb, zs, hs = c["depth"], c["num_blocks"], c["z_size"], c["h_size"]
    x = np.clip((c["x"].astype(np.float64) + 0.5) / 256.0, 0.0, 1.0) - 0.5
    q = O._sub(p, "x_enc/")
    h = O.conv2d(x, q["V"], q["g"], q["b"], stride=(2, 2))
    ups = {}
    for i in range(depth):
        for j in range(nb):
            h, qm, ql, uc = O.iaf_layer_up(h, O._sub(p, "IAF_%d_%d/" % (i, j)), zs, hs, downsample=(i > 0 and j == 0))
            ups[(i, j)] = (qm, ql, uc)
    n, hw = x.shape[0], x.shape[2] // 2 ** depth
    h = np.tile(np.asarray(p["h_top"]).reshape([1, -1, 1, 1]), [n, 1, hw, hw])
    out, kl_obj, kl_cost, it = {}, np.zeros(n), np.zeros(n), iter(noise)
    for i in reversed(range(depth)):
        for j in reversed(range(nb)):
            eps_prior, eps_post = next(it), next(it)
            qm, ql, uc = ups[(i, j)]
            h, cur_obj, cur_cost, _ = O.iaf_layer_down(h, O._sub(p, "IAF_%d_%d/" % (i, j)), qm, ql, uc, eps_post, zs, hs, c["kl_min"],
                                                       mode="train", downsample=(i > 0 and j == 0), eps_prior=eps_prior)
            kl_obj, kl_cost = kl_obj + cur_obj, kl_cost + cur_cost
            out["model/kl_obj_%02d_%02d" % (i, j)] = float(np.mean(cur_obj))
            out["model/kl_cost_%02d_%02d" % (i, j)] = float(np.mean(cur_cost))
    q = O._sub(p, "x_dec/")
    xo = np.clip(O.deconv2d(O.elu(h), q["V"], q["g"], q["b"]), -0.5 + 1 / 512., 0.5 - 1 / 512.)
    log_pxz = O.discretized_logistic(xo, p["dec_log_stdv"], x)
    loss = float(np.sum(O.compute_lowerbound(log_pxz, kl_cost, 1)))
    S = c["image_size"]
    out.update({"model/bits_per_dim": loss / (math.log(2.) * 3 * S * S * n), "model/dec_log_stdv": float(np.asarray(p["dec_log_stdv"]).reshape(-1)[0]),
                "model/log_pxz": -float(np.mean(log_pxz)), "model/kl_obj": float(np.mean(kl_obj)), "model/kl_cost": float(np.mean(kl_cost))})
    return out, float(np.sum(kl_obj - log_pxz))


def _compare_state(ts, other, exact, what):
    """tests/test_hip_train_step.py::_compare on what the update moves"""
    for k in ("params", "slot_m", "slot_v", "ema"):
        a, b = getattr(ts.flat, k), getattr(other.flat, k)
        if exact:
            assert torch.equal(a, b), (what, k, float((a - b).abs().max()))
        else:
            rel = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
            assert rel <= 1e-6, (what, k, rel)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_model_steps_report_the_oracles_summaries(amd, case, graph):
    c = case
    ts = amd.TrainStep(_model(amd, c), LR, graph=graph, summaries=True)
    plain = amd.TrainStep(_model(amd, c), LR, graph=graph)
    lasts = []
    for step in range(3):
        x, noise = _inputs(c, step)
        torch.cuda.synchronize()
        want, want_obj = _oracle_summaries(c, ts.flat.p, noise)
        if step == 0:       # the set-up does what it is for: the two 8x8 layers clamp (kl_obj above kl_cost), the 16x16 layers do not
            for j in range(c["num_blocks"]):
                assert want["model/kl_obj_01_%02d" % j] > want["model/kl_cost_01_%02d" % j] + 100.0, want
                assert abs(want["model/kl_obj_00_%02d" % j] - want["model/kl_cost_00_%02d" % j]) < 1e-6 * want["model/kl_obj_00_%02d" % j], want
        obj = ts(x, noise)
        plain(x, noise)
        last = ts.last_summaries()
        assert abs(float(obj.item()) - want_obj) <= 1e-4 * abs(want_obj), step
        assert sorted(last) == sorted(list(want) + ["grad_norm", "steps", "skipped"]), sorted(last)
        for k, v in sorted(want.items()):
            print("step %d %-24s got %.9g want %.9g (relative %.2e)" % (step, k, last[k], v, abs(last[k] - v) / abs(v)))
        for k, v in want.items():
            assert abs(last[k] - v) <= 1e-4 * abs(v), (step, k, last[k], v)
        norm = float(torch.sqrt((ts.flat.grads.double() ** 2).sum()).item())
        assert math.isfinite(norm) and norm > 0 and abs(last["grad_norm"] - norm) <= 1e-7 * norm, (step, last["grad_norm"], norm)
        assert (last["steps"], last["skipped"]) == (step + 1, 0)
        lasts.append(last)
    mean = ts.summaries()
    assert (mean["steps"], mean["skipped"]) == (3, 0)
    for k in lasts[0]:
        if k not in ("steps", "skipped"):
            w = (lasts[0][k] + lasts[1][k] + lasts[2][k]) / 3
            assert abs(mean[k] - w) <= 1e-12 * abs(w), (k, mean[k], w)
    after = ts.summaries(reset=False)                                          # ... and then it was reset
    assert (after["steps"], after["skipped"]) == (0, 0) and math.isnan(after["model/bits_per_dim"])
    assert ts.skipped == 0 and ts.graphed == graph and ts.graph_refused is None
    assert ts.captures == (1 if graph else 0)
    _compare_state(ts, plain, exact=not graph, what="graph" if graph else "eager")
    ts(*_inputs(c, 3))                                                         # the record goes on after a reset, in the same graph
    last = ts.last_summaries()
    one = ts.summaries()                                                       # (the reset zeroes the whole record, `last` included)
    assert (one["steps"], one["skipped"]) == (1, 0) and ts.captures == (1 if graph else 0)
    assert one == last and math.isfinite(one["model/bits_per_dim"]) and one["grad_norm"] > 0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_a_skipped_step_is_counted_and_kept_out_of_the_means(amd, case, graph):
    c = case
    ts = amd.TrainStep(_model(amd, c), LR, graph=graph, summaries=True)
    lasts = []
    for step in range(2):
        ts(*_inputs(c, step))
        lasts.append(ts.last_summaries())
    x, noise = _inputs(c, 2)
    noise[5][1, 3, 4, 5] = float("nan")                       # one posterior eps of the 16x16 level
    ts(x, noise)
    assert ts.skipped == 1
    last = ts.last_summaries()
    assert not math.isfinite(last["grad_norm"])
    assert (last["steps"], last["skipped"]) == (2, 1)
    assert math.isfinite(last["model/kl_obj_01_01"]) and last["model/kl_obj_01_01"] != lasts[1]["model/kl_obj_01_01"]   # its own numbers
    mean = ts.summaries()
    assert (mean["steps"], mean["skipped"]) == (2, 1)
    for k in lasts[0]:
        if k not in ("steps", "skipped"):
            w = (lasts[0][k] + lasts[1][k]) / 2
            assert math.isfinite(mean[k]) and abs(mean[k] - w) <= 1e-12 * abs(w), (k, mean[k], w)
