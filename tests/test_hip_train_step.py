"""GPU tests of the guarded training step (iaf_amd/train.py, include/iaf_hip.h: iaf_nonfinite_scan, iaf_adamax_ema_step_guarded,
iaf_skip_counter_*): the two kernels on their own and inside a replayed hipGraph, clean CVAE1 steps against the hand-composed step
(prepare_weights -> forward_backward(grads=flat.g) -> FlatParams.adamax_ema_step), a poisoned input, and a real overflow of the
fp16 planes that the fp32 oracle trains through."""
import ctypes

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


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def scan(amd, buf, extra, guard, check=True):
    amd._capi.check(amd._capi.lib().iaf_nonfinite_scan(ptr(buf), buf.numel(), ptr(extra) if extra is not None else None,
                                                       0 if extra is None else extra.numel(), ptr(guard), stream()))
    if check:
        torch.cuda.synchronize()
        assert guard[1:].tolist() == [0, 0, 0], guard.tolist()             # the arrival count is back to 0 after every scan


# -- the kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1000003])
def test_guard_scan_finds_every_non_finite_and_nothing_else(amd, n):
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    guard[0] = 7                                                            # (every scan writes its own verdict)
    rng = np.random.RandomState(n)
    base = rng.standard_normal(n).astype(np.float32)
    base[::7] = np.finfo(np.float32).max                                    # the largest finite float ...
    base[1::5] = -np.finfo(np.float32).max
    base[2::11] = np.float32(1e-40)                                         # ... and subnormals are finite
    base[3::13] = -np.float32(1e-45)
    buf = dev(base)
    extra = dev([1.0, -3.0e38])
    scan(amd, buf, extra, guard)
    assert int(guard[0].item()) == 0
    places = sorted({0, n - 1, max(0, n - 2), (n // 4) * 4 if (n // 4) * 4 < n else n - 1, n // 2})   # first, last, tail, middle
    for bad in (float("nan"), float("inf"), float("-inf")):
        for i in places:
            b = base.copy()
            b[i] = bad
            scan(amd, dev(b), extra, guard)
            assert int(guard[0].item()) == 1, (n, bad, i)
            scan(amd, buf, extra, guard)                                    # cleared again by the next scan
            assert int(guard[0].item()) == 0, (n, bad, i)
        for j in range(2):
            e = np.array([1.0, -3.0e38], np.float32)
            e[j] = bad
            scan(amd, buf, dev(e), guard)
            assert int(guard[0].item()) == 1, (n, bad, "extra", j)
    # unaligned (every element through the scalar path)
    big = dev(np.concatenate([[0.0], base]))
    un = big[1:]
    assert un.data_ptr() % 16
    scan(amd, un, None, guard)
    assert int(guard[0].item()) == 0
    big[-1] = float("nan")
    scan(amd, un, None, guard)
    assert int(guard[0].item()) == 1


def _buffers(n, seed):
    rng = np.random.RandomState(seed)
    return [dev(rng.standard_normal(n)), dev(rng.standard_normal(n)), dev(np.abs(rng.standard_normal(n))),
            dev(rng.standard_normal(n)), dev(rng.standard_normal(n))]         # var, grad, slot_m, slot_v, ema


def _adamax_args(bufs, n):
    var, grad, m, v, ema = bufs
    return [ptr(var), ptr(grad), ptr(m), ptr(v), ptr(ema), n, LR, 0.9, 0.999, 1e-8, 0.999, 0.5]


@pytest.mark.parametrize("n", [5, 1000003])
def test_gated_update_is_the_plain_update_when_clear_and_moves_nothing_when_raised(amd, n):
    from iaf_amd.train import _SkipCounter
    lib = amd._capi.lib()
    cnt = _SkipCounter()
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    a, b = _buffers(n, 1), _buffers(n, 1)
    extra = dev([0.0])
    for step in range(3):
        scan(amd, a[1], extra, guard)
        amd._capi.check(lib.iaf_adamax_ema_step_guarded(*(_adamax_args(a, n) + [ptr(guard), cnt._h, stream()])))
        amd._capi.check(lib.iaf_adamax_ema_step(*(_adamax_args(b, n) + [stream()])))
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(x, y), step                                  # bit-identical
    assert cnt.read() == 0
    before = [t.clone() for t in a]
    for k, bad_extra in enumerate((False, True)):
        if bad_extra:
            extra.fill_(float("inf"))
        else:
            a[1][n - 1] = float("nan")
        scan(amd, a[1], extra, guard)
        amd._capi.check(lib.iaf_adamax_ema_step_guarded(*(_adamax_args(a, n) + [ptr(guard), cnt._h, stream()])))
        torch.cuda.synchronize()
        for x, y in zip(a[:1] + a[2:], before[:1] + before[2:]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))   # byte-identical
        assert cnt.read() == k + 1


def test_guard_and_gated_update_in_a_replayed_graph(amd):
    from iaf_amd.train import _SkipCounter
    lib = amd._capi.lib()
    n = 1000003
    cnt = _SkipCounter()
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    a, b = _buffers(n, 2), _buffers(n, 2)
    extra = dev([0.0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            scan(amd, a[1], extra, guard, check=False)
            amd._capi.check(lib.iaf_adamax_ema_step_guarded(*(_adamax_args(a, n) + [ptr(guard), cnt._h, stream()])))
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    clean_grad = a[1].clone()
    # replays: clean, NaN at the first element, clean, -inf in the extra, clean -- the guard starts clear on every replay
    for r, poison in enumerate([None, "grad", None, "extra", None, "grad"]):
        a[1].copy_(clean_grad)
        extra.fill_(0.0)
        if poison == "grad":
            a[1][0] = float("nan")
        elif poison == "extra":
            extra.fill_(float("-inf"))
        before = [t.clone() for t in a]
        g.replay()
        torch.cuda.synchronize()
        assert guard.tolist() == [0 if poison is None else 1, 0, 0, 0], (r, guard.tolist())   # the verdict of THIS replay
        if poison is None:
            b[1].copy_(clean_grad)
            amd._capi.check(lib.iaf_adamax_ema_step(*(_adamax_args(b, n) + [stream()])))
            torch.cuda.synchronize()
            for x, y in zip(a, b):
                assert torch.equal(x, y), r
        else:
            for x, y in zip(a, before):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), r
    assert cnt.read() == 3
    del g


# -- the model step ----------------------------------------------------------------------------------------------------------------
def _model(amd, c, params):
    model = amd.CVAE1(z_size=c["z_size"], h_size=c["h_size"], kl_min=c["kl_min"], depth=c["depth"], num_blocks=c["num_blocks"], k=1,
                      image_size=c["image_size"])
    model.set_training(True)
    model.load({k: dev(v) if isinstance(v, np.ndarray) else v.clone() for k, v in params.items()})
    return model


class Hand(object):
    """the hand-composed step: prepare_weights -> forward_backward(grads=flat.g) -> FlatParams.adamax_ema_step"""

    def __init__(self, amd, c, params, state=None):
        import iaf_amd.parallel as par
        self.model = _model(amd, c, params)
        self.flat = par.FlatParams({k: self.model.params[k] for k in self.model.completion_order()})
        self.model.load(self.flat.p)
        if state is not None:
            for k in ("params", "slot_m", "slot_v", "ema"):
                getattr(self.flat, k).copy_(state[k])

    def __call__(self, x, noise):
        self.model.prepare_weights()
        _, obj, _ = self.model.forward_backward(x, noise, grads=self.flat.g)
        self.flat.adamax_ema_step(LR)
        return obj


def _state(flat):
    torch.cuda.synchronize()
    return {k: getattr(flat, k).clone() for k in ("params", "slot_m", "slot_v", "ema", "grads")}


def _compare(ts, hand, exact, what):
    for k in ("params", "slot_m", "slot_v", "ema", "grads"):
        a, b = getattr(ts.flat, k), getattr(hand.flat, k)
        assert a.shape == b.shape
        if exact:
            assert torch.equal(a, b), (what, k, float((a - b).abs().max()))
        else:
            rel = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
            assert rel <= 1e-6, (what, k, rel)


def _inputs(c, step):
    x = torch.from_numpy(c["x"]).cuda()
    noise = [dev(np.roll(e, step, axis=0) * (1.0 + 0.05 * step)) for e in c["noise"]]
    return x, noise


def _exchange_note(ts, B):
    st = [(i, j, layer.posterior.stack.step_exchanges(B, 16 >> i, 16 >> i)) for i, lv in enumerate(ts.model.layers) for j, layer in enumerate(lv)]
    return "stacks whose eager step hands halo rows over (a replay may recompute them instead): %s" % [s[:2] for s in st if s[2]]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_clean_steps_equal_the_hand_composed_step(amd, graph):
    c = gi.model_case_inputs("model_cfg")
    ts = amd.TrainStep(_model(amd, c, c["params"]), LR, graph=graph)
    hand = Hand(amd, c, c["params"])
    assert list(ts.flat.p) == list(hand.flat.p)
    for step in range(5):
        x, noise = _inputs(c, step)
        obj = ts(x, noise)
        want = hand(x, noise)
        torch.cuda.synchronize()
        if graph:
            assert abs(float(obj.item()) - float(want.item())) <= 1e-6 * abs(float(want.item())), step
        else:
            assert torch.equal(obj, want), step
    assert ts.skipped == 0
    assert ts.graphed == graph and ts.graph_refused is None
    if graph:
        print(_exchange_note(ts, c["B"]))
    _compare(ts, hand, exact=not graph, what="graph" if graph else "eager")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_a_nan_in_one_eps_skips_the_step_and_the_next_step_is_the_hand_composed_one(amd, graph):
    c = gi.model_case_inputs("model_cfg")
    ts = amd.TrainStep(_model(amd, c, c["params"]), LR, graph=graph)
    for step in range(2):
        ts(*_inputs(c, step))
    saved = _state(ts.flat)
    x, noise = _inputs(c, 2)
    noise[5][1, 3, 4, 5] = float("nan")                       # one posterior eps of the 16x16 level
    ts(x, noise)
    assert ts.skipped == 1
    # (the objective itself can stay finite: the free-bits max(mean KL, kl_min) drops a NaN, tf_train.py:79 -- the gradients do not)
    assert not bool(torch.isfinite(ts.flat.grads).all())
    for k in ("params", "slot_m", "slot_v", "ema"):
        assert torch.equal(getattr(ts.flat, k).view(torch.int32), saved[k].view(torch.int32)), k
    hand = Hand(amd, c, {k: v for k, v in ts.flat.p.items()}, state=saved)
    x, noise = _inputs(c, 3)
    ts(x, noise)
    hand(x, noise)
    assert ts.skipped == 1
    _compare(ts, hand, exact=not graph, what="after the skip")


def test_a_real_fp16_overflow_is_skipped_then_trained_through_on_bf16_planes(amd):
    """exp(g) + 15 on the first hidden layer of one IAF stack and -15 on its two output layers: its weights pass 65504, so the step on
    two fp16 planes is not finite while the fp32 model (the oracle) is.  The step is skipped; at the next call after the host has seen
    the counter rise the stack moves to bf16 planes, the graph is captured again and the update is applied with the oracle's gradients."""
    from oracle import iaf_grad_oracle as G
    from oracle import iaf_oracle as O
    c = gi.model_case_inputs("model_cfg")
    B = c["B"]
    ts = amd.TrainStep(_model(amd, c, c["params"]), LR, graph=True)
    x, noise = torch.from_numpy(c["x"]).cuda(), [dev(e) for e in c["noise"]]
    ts(x, noise)
    assert ts.skipped == 0 and ts.captures == 1
    st = ts.model.layers[0][0].posterior.stack
    assert st.step_is_f16(B, 16, 16), "the 16x16 stack must run its step on two fp16 planes at B = %d" % B
    pre = "IAF_0_0/ar_multiconv2d/"
    with torch.no_grad():
        ts.flat.p[pre + "layer_1/g"].add_(15.0)
        ts.flat.p[pre + "layer_out_0/g"].sub_(15.0)
        ts.flat.p[pre + "layer_out_1/g"].sub_(15.0)
    saved = _state(ts.flat)
    p64 = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in ts.flat.p.items()}
    noise64 = [f32(e) for e in c["noise"]]
    want, xo, want_obj = G.cvae1_grads(c["x"], p64, c["z_size"], c["h_size"], c["depth"], c["num_blocks"], c["kl_min"], noise64)
    assert np.isfinite(want_obj) and np.isfinite(xo).all() and all(np.isfinite(v).all() for v in want.values())
    fxo, fobj, _ = O.cvae1_forward(c["x"], p64, c["z_size"], c["h_size"], c["depth"], c["num_blocks"], c["kl_min"], 1, noise64)
    assert np.isfinite(fobj).all() and np.isfinite(fxo).all()                # the fp32 forward trains through these weights
    ts(x, noise)                                              # the graph as captured: the fp16-plane step overflows
    assert ts.skipped == 1, "the fp16-plane step was finite: the test's weights do not overflow it"
    assert not bool(torch.isfinite(ts.flat.grads).all())      # (what the guard saw; the objective may stay finite, see above)
    assert st.range_errors() != 0
    for k in ("params", "slot_m", "slot_v", "ema"):
        assert torch.equal(getattr(ts.flat, k).view(torch.int32), saved[k].view(torch.int32)), k
    obj = ts(x, noise)                                        # moves the stack, captures again, applies
    assert ts.skipped == 1 and ts.captures == 2 and ts.graphed
    assert not st.step_is_f16(B, 16, 16)
    assert np.isfinite(float(obj.item()))
    assert abs(float(obj.item()) - want_obj) <= 2e-5 * abs(want_obj)
    assert not torch.equal(ts.flat.params, saved["params"]) and bool(torch.isfinite(ts.flat.params).all())
    assert bool(torch.isfinite(ts.flat.ema).all())
    worst = (0.0, None)
    for k in sorted(want):
        got = ts.flat.g[k].detach().cpu().numpy().astype(np.float64)
        err = float(np.abs(got - want[k]).max() / (np.abs(want[k]).max() + 1e-3))
        worst = max(worst, (err, k))
        assert err < 2e-3, (k, err)
    print("after the overflow: worst relative gradient error %.2e (%s)" % worst)
