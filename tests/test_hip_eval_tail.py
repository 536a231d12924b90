"""GPU leaf test of iaf_eval_tail / iaf_eval_reset (include/iaf_hip.h; iaf_amd/csrc/iaf_kernels_objective.hpp: iaf_eval_tail_kernel) through
the raw C ABI: the one launch that closes an evaluation pass against the entry points it replaces, called on the same device
buffers -- iaf_discretized_logistic -> iaf_colsum -> iaf_lowerbound_stream_update(k_chunk = 1) per pass, iaf_lowerbound_stream_finalize
(and, for k = 1, iaf_compute_lowerbound) behind the k-th.  The criterion is BIT IDENTITY: the kernel's summation orders are those
kernels' (which have their own fp64 leaf tests, tests/test_hip_objective_kernels.py), so no tolerance is involved.  The record's
counts are exact; its fp64 loss_sum is held to n 2^-53 sum|bound|, the most a reordered fp64 sum of n terms can differ by.

Sizes: n (batch rows, one workgroup each) 1, 3, 64, 257; row lengths 1, 192, 193, 256, 257, 3072 around the 256-thread sweep, from the
logistic case generator of tests/objective_reference.py; 1, 2, 20 layers; k 1, 2, 3."""
import ctypes

import numpy as np
import pytest
import torch

import objective_reference as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
NS, ROWS, LAYERS, KS = (1, 3, 64, 257), (1, 192, 193, 256, 257, 3072), (1, 2, 20), (1, 2, 3)
# every n with every row length; the layer counts and k rotate so that each value meets each n and several row lengths
CASES = [(n, r, LAYERS[(i + j) % 3], KS[(i + 2 * j) % 3]) for i, n in enumerate(NS) for j, r in enumerate(ROWS)]


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()      # raises if the HIP extension is missing: no silent fallback
    return iaf_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def abi(amd):
    return amd._capi.lib(), amd.layers._ptr, amd.layers._stream, amd._capi.check


def bits(t):
    torch.cuda.synchronize()
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def read_record(rec):
    """(loss_sum, images, nonfinite, pass, arrivals) of the 32-byte record"""
    torch.cuda.synchronize()
    h = rec.cpu()
    c = h[1:3].view(torch.int64)
    w = h[3:4].view(torch.int32)
    return float(h[0]), int(c[0]), int(c[1]), int(w[0]), int(w[1])


def pass_inputs(n, row, nl, s):
    """the inputs of pass s on a batch of n rows: x (the scaled image, shared by the passes) and x_out from the logistic size-case
    generator, x_out moved a little per pass (so that the k weights of a row are of one size and the log-sum-exp mixes them), and
    layer_cost [nl, n] around 900 / nl"""
    c = R.dl_size_case(n, row)
    rng = np.random.RandomState(9000 + 131 * s + 7 * row + n + nl)
    mean = R.f32(np.clip(c["mean"] + 0.002 * rng.standard_normal((n, row)), -0.6, 0.6))
    cost = R.f32(900.0 / nl + rng.standard_normal((nl, n)))
    return dev(c["sample"]), dev(mean), dev(cost)


class State(object):
    """the device state of one side: the streaming pair, the bound, the record (fused side only)"""

    def __init__(self, n, per_image_n=0):
        self.n = n
        self.run_max, self.run_sum, self.bound = nans(n), nans(n), nans(n)
        self.rec = torch.full((4,), NAN, dtype=torch.float64, device="cuda")
        self.per_image = nans(per_image_n) if per_image_n else None


def fused_pass(amd, st, x, x_out, cost, logscale, k, indices=None):
    lib, P, stream, check = abi(amd)
    n, row = x_out.shape
    check(lib.iaf_eval_tail(P(x_out), P(logscale), P(x), row, R.BINSIZE, P(cost), int(cost.shape[0]), n, P(st.run_max), P(st.run_sum), k,
                            None if indices is None else ctypes.c_void_p(indices.data_ptr()),
                            None if st.per_image is None else P(st.per_image), P(st.bound), ctypes.c_void_p(st.rec.data_ptr()), stream()))


def composed_pass(amd, st, x, x_out, cost, logscale):
    """the launches the tail replaces, on the same device buffers -> (log_pxz, kl)"""
    lib, P, stream, check = abi(amd)
    n, row = x_out.shape
    lp, kl = nans(n), nans(n)
    check(lib.iaf_discretized_logistic(P(x_out), P(logscale), 1, P(x), P(lp), n, row, R.BINSIZE, stream()))
    check(lib.iaf_colsum(P(cost), P(kl), int(cost.shape[0]), n, stream()))
    check(lib.iaf_lowerbound_stream_update(P(st.run_max), P(st.run_sum), P(lp), P(kl), n, 1, stream()))
    return lp, kl


def reset(amd, st):
    lib, P, stream, check = abi(amd)
    check(lib.iaf_eval_reset(ctypes.c_void_p(st.rec.data_ptr()), P(st.run_max), P(st.run_sum), st.n, stream()))


def armed(st):
    torch.cuda.synchronize()
    return bool((st.run_max == float("-inf")).all()) and bool((st.run_sum == 0).all())


@pytest.mark.parametrize("n,row,nl,k", CASES, ids=lambda v: str(v))
def test_tail_equals_the_entry_points_it_replaces_bit_for_bit(amd, n, row, nl, k):
    """two batches in a row with no reset between them: after every pass the streaming pair, after the k-th the bound; the record's
    pass counter cycles 1, 2, ..., 0 and its sums accumulate over the batches"""
    lib, P, stream, check = abi(amd)
    logscale = dev(np.array([R.DL_TAIL]))
    fu, co = State(n), State(n)
    reset(amd, fu)
    assert armed(fu) and read_record(fu.rec) == (0.0, 0, 0, 0, 0)
    all_bounds = []
    for batch in range(2):
        check(lib.iaf_lowerbound_stream_init(P(co.run_max), P(co.run_sum), n, stream()))
        for s in range(k):
            x, x_out, cost = pass_inputs(n, row, nl, 10 * batch + s)
            fused_pass(amd, fu, x, x_out, cost, logscale, k)
            lp, kl = composed_pass(amd, co, x, x_out, cost, logscale)
            loss_sum, images, nonfinite, pas, arrivals = read_record(fu.rec)
            assert (pas, arrivals, nonfinite) == ((s + 1) % k, 0, 0)
            if s + 1 < k:
                assert same_bits(fu.run_max, co.run_max) and same_bits(fu.run_sum, co.run_sum), (batch, s)
                assert images == batch * n
        check(lib.iaf_lowerbound_stream_finalize(P(co.run_max), P(co.run_sum), P(co.bound), n, k, stream()))
        assert same_bits(fu.bound, co.bound), batch
        assert armed(fu), "the rows are armed again behind the closing pass"
        if k == 1:
            one = nans(n)
            check(lib.iaf_compute_lowerbound(P(lp), P(kl), P(one), n, 1, stream()))
            assert same_bits(fu.bound, one)
        torch.cuda.synchronize()
        bd = fu.bound.cpu().numpy().astype(np.float64)
        assert np.isfinite(bd).all()
        all_bounds.append(bd)
        want = np.concatenate(all_bounds)
        loss_sum, images, nonfinite, pas, _ = read_record(fu.rec)
        err, tol = abs(loss_sum - float(np.sum(want))), want.size * 2.0 ** -53 * float(np.abs(want).sum())
        print("n %d row %d nl %d k %d batch %d: loss_sum %.17g, |error| %.3g (bound %.3g)" % (n, row, nl, k, batch, loss_sum, err, tol))
        assert (images, nonfinite, pas) == ((batch + 1) * n, 0, 0)
        assert err <= tol
    reset(amd, fu)
    assert armed(fu) and read_record(fu.rec) == (0.0, 0, 0, 0, 0)


def test_a_nan_in_one_layer_cost_entry_is_one_nonfinite_bound(amd):
    """planted in the closing pass: the streaming update the tail restates (iaf_lb_update_kernel) starts a row's sum afresh while its
    running maximum is still -inf, so a NaN weight that comes FIRST is dropped by the pass behind it"""
    n, row, nl, k = 64, 193, 2, 2
    logscale = dev(np.array([R.DL_TAIL]))
    fu = State(n)
    reset(amd, fu)
    for s in range(k):
        x, x_out, cost = pass_inputs(n, row, nl, s)
        if s == k - 1:
            cost[1, 37] = NAN
        fused_pass(amd, fu, x, x_out, cost, logscale, k)
    torch.cuda.synchronize()
    bd = fu.bound.cpu().numpy()
    assert list(np.nonzero(~np.isfinite(bd))[0]) == [37]
    loss_sum, images, nonfinite, pas, _ = read_record(fu.rec)
    assert (images, nonfinite, pas) == (n, 1, 0) and not np.isfinite(loss_sum)
    reset(amd, fu)
    assert armed(fu) and read_record(fu.rec) == (0.0, 0, 0, 0, 0)


@pytest.mark.parametrize("n,k", [(3, 1), (257, 3)])
def test_per_image_goes_through_the_index_vector(amd, n, k):
    row, nl, total = 192, 2, 2 * n + 5
    logscale = dev(np.array([R.DL_TAIL]))
    idx = np.random.RandomState(n).permutation(total)[:n].astype(np.int64)
    indices = torch.from_numpy(idx).cuda()
    fu = State(n, per_image_n=total)
    reset(amd, fu)
    for s in range(k):
        x, x_out, cost = pass_inputs(n, row, nl, s)
        fused_pass(amd, fu, x, x_out, cost, logscale, k, indices)
        if s + 1 < k:
            torch.cuda.synchronize()
            assert bool(torch.isnan(fu.per_image).all()), "only the closing pass writes per_image"
    torch.cuda.synchronize()
    got, bd = fu.per_image.cpu().numpy(), fu.bound.cpu().numpy()
    assert np.isfinite(bd).all()
    assert np.array_equal(got[idx].view(np.int32), bd.view(np.int32))
    rest = np.ones(total, bool)
    rest[idx] = False
    assert np.isnan(got[rest]).all() and rest.sum() == total - n


def test_error_codes(amd):
    lib, P, stream, _ = abi(amd)
    C = amd._capi
    n, row, nl = 3, 4, 2
    x, x_out, cost = pass_inputs(n, row, nl, 0)
    logscale = dev(np.array([R.DL_TAIL]))
    st = State(n, per_image_n=n)
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    rec, ip = ctypes.c_void_p(st.rec.data_ptr()), ctypes.c_void_p(idx.data_ptr())
    good = [P(x_out), P(logscale), P(x), row, R.BINSIZE, P(cost), nl, n, P(st.run_max), P(st.run_sum), 1, ip, P(st.per_image), P(st.bound), rec,
            stream()]
    for i in (0, 1, 2, 5, 8, 9, 13, 14):                      # every pointer that may not be NULL
        a = list(good)
        a[i] = None
        assert lib.iaf_eval_tail(*a) == C.IAF_ERR_NULL, i
    a = list(good)
    a[11] = None                                               # indices may be NULL only together with per_image
    assert lib.iaf_eval_tail(*a) == C.IAF_ERR_NULL
    for i, bad in ((3, 0), (4, 0.0), (4, -1.0), (6, 0), (7, 0), (7, 65536), (10, 0)):
        a = list(good)
        a[i] = bad
        assert lib.iaf_eval_tail(*a) == C.IAF_ERR_SHAPE, (i, bad)
    a = list(good)
    a[14] = ctypes.c_void_p(st.rec.data_ptr() + 4)
    assert lib.iaf_eval_tail(*a) == C.IAF_ERR_WORKSPACE
    assert lib.iaf_eval_reset(None, P(st.run_max), P(st.run_sum), n, stream()) == C.IAF_ERR_NULL
    assert lib.iaf_eval_reset(rec, None, P(st.run_sum), n, stream()) == C.IAF_ERR_NULL
    assert lib.iaf_eval_reset(rec, P(st.run_max), None, n, stream()) == C.IAF_ERR_NULL
    assert lib.iaf_eval_reset(rec, P(st.run_max), P(st.run_sum), 0, stream()) == C.IAF_ERR_SHAPE
    assert lib.iaf_eval_reset(ctypes.c_void_p(st.rec.data_ptr() + 4), P(st.run_max), P(st.run_sum), n, stream()) == C.IAF_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(st.bound).all()) and bool(torch.isnan(st.rec).all()), "a refused call launches nothing"
    a = list(good)
    a[11], a[12] = None, None                                  # no per_image: no indices needed
    assert lib.iaf_eval_tail(*a) == C.IAF_OK


def test_captured_in_a_graph_and_replayed_k_times_equals_eager(amd):
    """the pass counter lives in the record: ONE captured launch, replayed k times on inputs refilled in place, closes the batch"""
    n, row, nl, k = 257, 257, 20, 3
    logscale = dev(np.array([R.DL_TAIL]))
    inputs = [pass_inputs(n, row, nl, s) for s in range(k)]
    eager = State(n)
    reset(amd, eager)
    for x, x_out, cost in inputs:
        fused_pass(amd, eager, x, x_out, cost, logscale, k)
    want = read_record(eager.rec)
    gr = State(n)
    sx, sxo, sc = (t.clone() for t in inputs[0])
    reset(amd, gr)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        fused_pass(amd, gr, sx, sxo, sc, logscale, k)
    reset(amd, gr)                                            # (a capture launches nothing)
    for x, x_out, cost in inputs:
        sx.copy_(x), sxo.copy_(x_out), sc.copy_(cost)
        g.replay()
    assert read_record(gr.rec) == want and want[1:] == (n, 0, 0, 0)
    assert same_bits(gr.bound, eager.bound) and armed(gr)
