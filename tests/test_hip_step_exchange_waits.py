"""The 16x16 exchange-form step kernel after its hand-over was reordered (iaf_amd/csrc/iaf_step_fused.hpp: xch_import -> xch_handover ->
xch_rearm; the ticket taken by the first helper thread).  No arithmetic changed, so every check here is about the protocol:

 * re-arming: an imported row is put back to the "not there yet" pattern BEHIND the barrier that hands it to the compute waves, later in
   the helper's phase.  A row left un-armed would be taken by the next launch on the stack as that launch's data: inputs A, B, A on one
   stack, eagerly and as three replays of a captured graph -- the third output equals the first and the second a fresh stack's, bit for bit;
 * tickets: who takes the ticket changed, not what it decides -- knobs 1 (lists ignore the placement), 2 (tickets out of dispatch order)
   and 3 give the bits of knob 0;
 * numbers: against the recomputing kernel (other summation order of the output pair: not bitwise);
 * posterior_block: the helper waves that re-arm also finish the free-bits sums.

Geometry of the headline: n_z = 32, n_h = 160, depth_ar = 2, 16x16, on both plane formats.  B = 1, 3, 9: fewer work lists than XCDs, a
batch that is no multiple of 8, more than one image per list.  No test here provokes a give-up (tests/test_hip_halo_exchange.py does)."""
import numpy as np
import pytest
import torch

import golden_inputs as gi

pytestmark = pytest.mark.gpu
N_Z, N_H, D, HW = 32, 160, 2, 16
BATCHES = [1, 3, 9]
PRECISIONS = ["f16x2", "bf16x3"]


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()
    return iaf_amd


@pytest.fixture(scope="module")
def weights():
    hp = gi.ar_multiconv2d_params(np.random.RandomState(61), N_Z, [N_H] * D, [N_Z, N_Z])
    return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda() for k, v in hp.items()}


def _stack(amd, weights, precision, B, exchange=True):
    st = amd.ARStack(N_Z, [N_H] * D)
    st.set_precision(precision)
    st.set_fuse_step("always")                                   # (one launch at every batch size, beyond the size rule too)
    if not exchange:
        st.set_halo_exchange(False)
    st.prepare(weights)
    assert st.step_is_fused(B, HW, HW) and st.step_exchanges(B, HW, HW) == exchange
    if exchange:
        assert st.step_is_f16(B, HW, HW) == (precision == "f16x2")
    return st


def _inputs(B, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(B, N_Z, HW, HW, device="cuda", generator=g), torch.randn(B, N_H, HW, HW, device="cuda", generator=g))


def _step(st, z, ctx):
    zn, ls = st.iaf_step(z, ctx)
    torch.cuda.synchronize()
    assert st.exchange_errors() == 0
    return zn.clone(), ls.clone()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("z", "logsd")):
        assert torch.isfinite(x).all(), (what, name)
        assert torch.equal(x, y), (what, name, float((x.double() - y.double()).abs().max()))


@pytest.mark.parametrize("B", BATCHES, ids=lambda b: "B%d" % b)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rows_are_rearmed_between_eager_launches(amd, weights, precision, B):
    st, fresh = _stack(amd, weights, precision, B), _stack(amd, weights, precision, B)
    a, b = _inputs(B, 100 + B), _inputs(B, 200 + B)
    first = _step(st, *a)
    second = _step(st, *b)
    third = _step(st, *a)
    _same(third, first, "A again")
    _same(second, _step(fresh, *b), "B behind A against B on a fresh stack")
    assert not torch.equal(first[0], second[0])


@pytest.mark.parametrize("B", BATCHES, ids=lambda b: "B%d" % b)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rows_are_rearmed_between_replays_of_a_graph(amd, weights, precision, B):
    st, fresh = _stack(amd, weights, precision, B), _stack(amd, weights, precision, B)
    a, b = _inputs(B, 300 + B), _inputs(B, 400 + B)
    z, ctx = a[0].clone(), a[1].clone()
    out = (torch.empty_like(z), torch.empty_like(z))
    st.iaf_step(z, ctx, out=out)                                 # (warm-up: the exchange set is allocated outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.iaf_step(z, ctx, out=out)
    got = []
    for src in (a, b, a):
        z.copy_(src[0])
        ctx.copy_(src[1])
        graph.replay()
        torch.cuda.synchronize()
        assert st.exchange_errors() == 0
        got.append((out[0].clone(), out[1].clone()))
    _same(got[2], got[0], "A again")
    _same(got[1], _step(fresh, *b), "B behind A against B on a fresh stack")
    _same(got[0], _step(fresh, *a), "the replay against an eager launch")


@pytest.mark.parametrize("B", BATCHES, ids=lambda b: "B%d" % b)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ticket_order_and_placement_do_not_change_a_bit(amd, weights, precision, B):
    st = _stack(amd, weights, precision, B)
    x = _inputs(B, 500 + B)
    ref = _step(st, *x)
    for knob in (1, 2, 3):
        st.set_halo_exchange_debug(knob)
        assert st.step_exchanges(B, HW, HW)
        _same(_step(st, *x), ref, "knob %d" % knob)
    st.set_halo_exchange_debug(0)
    _same(_step(st, *x), ref, "knob 0 again")


@pytest.mark.parametrize("B", BATCHES, ids=lambda b: "B%d" % b)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_against_the_recomputing_kernel(amd, weights, precision, B):
    """Measure and bound of tests/test_hip_pair_step.py (_close, tol = 2e-6) for this pair of kernels, exchange form against recomputing
    form at 16-pixel rows: max |a - r| <= 2e-6 max(1, max |r|).  Where it comes from: both kernels add the same fp32 part-products, the
    exchange form sums the output pair's taps of the row below apart from those of its own rows -- a different order of a few hundred
    fp32 additions, 2e-6 = 34 ulp of the largest output."""
    xs, rc = _stack(amd, weights, precision, B), _stack(amd, weights, precision, B, exchange=False)
    x = _inputs(B, 600 + B)
    got, ref = _step(xs, *x), rc.iaf_step(*x)
    for a, r, name in zip(got, ref, ("z", "logsd")):
        a, r = a.double(), r.double()
        assert torch.isfinite(a).all(), name
        err = float((a - r).abs().max())
        print("%s B=%d %s: max |exchange - recomputing| = %.3g, bound %.3g" % (precision, B, name, err, 2e-6 * max(1.0, float(r.abs().max()))))
        assert err <= 2e-6 * max(1.0, float(r.abs().max())), (name, err)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_posterior_block_rearms_and_finishes_the_free_bits_sums(amd, weights, precision):
    B = 3
    st, fresh = _stack(amd, weights, precision, B), _stack(amd, weights, precision, B)

    def args(seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        t = lambda c, s=1.0: s * torch.randn(B, c, HW, HW, device="cuda", generator=g)
        return dict(qz_mean=t(N_Z), qz_logsd=t(N_Z, .25), rz_mean=t(N_Z), rz_logsd=t(N_Z, .25), pz_mean=t(N_Z), pz_logsd=t(N_Z, .25),
                    eps=t(N_Z), up_context=t(N_H), down_context=t(N_H))

    def block(s, kw):
        o = s.posterior_block(kl_min=0.25, **kw)
        torch.cuda.synchronize()
        assert s.exchange_errors() == 0
        return {k: o[k].clone() for k in ("z", "kl_obj", "kl_cost")}

    a, b = args(700), args(701)
    first, second, third = block(st, a), block(st, b), block(st, a)
    ref = block(fresh, b)
    for k in ("z", "kl_obj", "kl_cost"):
        assert torch.isfinite(first[k]).all() and torch.isfinite(second[k]).all(), k
        assert torch.equal(third[k], first[k]), ("A again", k)
        assert torch.equal(second[k], ref[k]), ("B behind A against B on a fresh stack", k)
    assert not torch.equal(first["z"], second["z"])
