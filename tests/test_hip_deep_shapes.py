"""Every compiled launch shape of both conv families under the epilogues of the masked ResNet (iaf_stack_create_resnet): EPI_RES with NCHW
input (the input conv) and with pixel-major input (every block's conv2, in place on the residual stream), EPI_HIDDEN (conv1) and EPI_OUT
on the raw stream -- the forward counterpart, for iaf_amd.ResnetARStack, of test_every_launch_shape_agrees (test_hip_parity.py) and
test_every_bf16x3_launch_shape_agrees (test_hip_bf3.py).  The shape lists are iaf_amd.build.SHAPES / BF3_SHAPES, the parsed
csrc/iaf_variants.def.

Per shape, three configurations (tests/deep_plan_reference.py FORWARD_CONFIGS) and every tile count per wave: the shape is pinned on every
layer that accepts it (set_tuning / set_tuning_bf3), a layer that refuses keeps its default shape, and a combination where no layer took
the pin does not count.  (The third configuration, n_h = 48 for three co tiles, has n_z = 16: a resnet stack and the reference's mask
need n_z and n_h to divide one another, so 32 cannot go with 48.)  Values against the fp64 statement (tests/deep_reference.py) on the fp32-rounded inputs, 1e-4 absolute, the
bound of test_resnet_stack_vs_fp64; the training forward against the evaluation forward bit for bit (the last block's conv2 writes
h_last != raw there, with no activation output).  At the end a shape must have run in each of the five roles a layer of the stack has.
Weights: deep_plan_reference.rand_params (the _s scale at 0.2: the reference then moves by more than 100 x the bound when any one layer is
missing, tests/test_deep_plan_reference.py)."""
import functools

import numpy as np
import pytest
import torch

import deep_plan_reference as D
import deep_reference as DR
from iaf_amd import build

pytestmark = pytest.mark.gpu

ATOL = 1e-4
CONFIGS = D.FORWARD_CONFIGS
ROLES = ("input", "conv1", "conv2", "conv2_last", "out")          # (a) .. (e)
F32_ERR = {}          # configuration -> error of the exact-fp32 family against fp64 (test 1 fills it, lazily otherwise)


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import iaf_amd
    iaf_amd._capi.lib()      # raises if the HIP extension is missing: no silent fallback
    return iaf_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(cfg):
    """weights, inputs and the fp64 outputs of one configuration: computed once, shared by every test, never modified"""
    B, n_h, n_z, depth, H, W = cfg
    rng = np.random.RandomState(6000 + n_h + 7 * n_z + depth)
    w = D.rand_params(rng, "r", n_z, n_h, depth)
    z, ctx = rng.standard_normal((B, n_z, H, W)), rng.standard_normal((B, n_h, H, W))
    m, s = DR.resnet(f32(z), f32(ctx), {k: f32(v) for k, v in w.items()}, "r", n_z, n_h, depth)
    return w, z, ctx, m, s


def _rel(w):
    return {k[2:]: dev(v) for k, v in w.items()}


def _pin(amd, st, family, shape, nt):
    """the shape on every hidden layer at `nt` tiles per wave and on the output pair at the first even count it accepts; a layer that
    refuses (divisibility, fewer K chunks than slices, no split pack) keeps its default shape.  Returns the layers that took the pin
    with the tile count each took."""
    took = {}
    for layer in range(st.depth_ar + 1):
        for n in ((nt,) if layer < st.depth_ar else (2, 4)):
            try:
                if family == "f32":
                    pxt, wco, ks = shape
                    st.set_tuning(layer, n, pxt, wco, ks)
                else:
                    ppw, pxt, ks, wco = shape
                    st.set_tuning_bf3(layer, n, ppw, pxt, ks, wco)
            except amd.UnsupportedError:
                continue
            took[layer] = n
            break
    return took


def _lds_bytes(family, shape, c_in, W, nt):
    """the launch's LDS, restated: conv_lds_bytes / bf3_lds_bytes of iaf_engine.hip:432-454"""
    if family == "f32":
        pxt, wco, ks = shape
        return D.conv_lds_bytes(c_in, W, nt, pxt, wco, ks)
    ppw, pxt, ks, wco = shape
    return D.bf3_lds_bytes(c_in, W, nt, ppw, pxt, ks, wco)


def _forward(amd, family, shape, cfg, nt, training):
    """one pinned stack: (layers that took the pin, (m_raw, s_raw, z_new, logsd)), or (layers, None) where the launch refuses the shape
    for its LDS -- any other refusal fails"""
    B, n_h, n_z, depth, H, W = cfg
    w, z, ctx, _, _ = _case(cfg)
    st = amd.ResnetARStack(n_z, n_h, depth)
    if family == "f32":
        st.set_precision("f32")
    if training:
        st.set_training(True)
    st.prepare(_rel(w))
    took = _pin(amd, st, family, shape, nt)
    if not took:
        return took, None
    layers = D.resnet_layers(n_z, n_h, depth)
    lds = {l: _lds_bytes(family, shape, layers[l][0], W, n) for l, n in took.items()}
    if family == "bf3":       # bf3_select falls back to the exact-fp32 kernel silently: every pinned layer must answer "bf16x3" ...
        took = {l: n for l, n in took.items() if lds[l] <= D.LDS_MAX}          # ... but past the LDS bound, where it does not count
        for l in took:
            assert st.layer_precision(l, B, H, W) == "bf16x3", (l, shape, nt)
        if not took:
            return took, None
    zd, cd = dev(z), dev(ctx)
    try:
        if training:
            z_new, logsd = st.iaf_step_train(zd, cd)
            m_raw = s_raw = None
        else:
            m_raw, s_raw = st.ar_multiconv2d(zd, cd)
            z_new, logsd = st.iaf_step(zd, cd)
    except amd.UnsupportedError:
        assert max(lds.values()) > D.LDS_MAX, "%s %s nt %d refused at launch, and not for the 160 KiB of LDS: %s" % (family, shape, nt, lds)
        return took, None
    torch.cuda.synchronize()
    return took, (m_raw, s_raw, z_new, logsd)


def _sweep(amd, family, shape, nts, cfgs):
    """-> roles seen, {configuration: worst error of the raw outputs}"""
    seen, errs, ran = set(), {}, []
    for cfg in cfgs:
        B, n_h, n_z, depth, H, W = cfg
        _, z, _, em, es = _case(cfg)
        for nt in nts:
            took, ev = _forward(amd, family, shape, cfg, nt, False)
            if ev is None:
                continue
            took_t, tr = _forward(amd, family, shape, cfg, nt, True)
            assert took_t == took and tr is not None
            m_raw, s_raw, z_new, logsd = ev
            e = max(np.abs(host(m_raw) - em).max(), np.abs(host(s_raw) - es).max())
            errs[cfg] = max(errs.get(cfg, 0.0), e)
            print("%s %s nt %d  B%d_h%d_z%d_d%d_%dx%d  layers %s: max |raw - fp64| = %.3g (max |ref| %.3g)"
                  % ((family, shape, nt) + cfg + (sorted(took.items()), e, max(np.abs(em).max(), np.abs(es).max()))))
            np.testing.assert_allclose(host(m_raw), em, atol=ATOL, rtol=0)
            np.testing.assert_allclose(host(s_raw), es, atol=ATOL, rtol=0)
            np.testing.assert_allclose(host(z_new), (f32(z) - 0.1 * em) / np.exp(0.1 * es), atol=ATOL, rtol=0)
            np.testing.assert_allclose(host(logsd), 0.1 * es, atol=ATOL, rtol=0)
            # the training forward runs the same kernels on the same operands (tests/test_hip_backward_geometry.py:193-195 for the plain stack)
            assert torch.equal(tr[2], z_new) and torch.equal(tr[3], logsd), (shape, nt, cfg)
            seen |= {D.layer_role(l, depth) for l in took}
            ran.append((cfg, nt))
    print("%s %s ran at %s in the roles %s" % (family, shape, ran, sorted(seen)))
    return seen, errs


def _f32_error(amd, cfg):
    """the exact-fp32 family's error of a configuration at the launch shapes it chooses itself"""
    if cfg not in F32_ERR:
        B, n_h, n_z, depth, H, W = cfg
        w, z, ctx, em, es = _case(cfg)
        st = amd.ResnetARStack(n_z, n_h, depth)
        st.set_precision("f32")
        st.prepare(_rel(w))
        m_raw, s_raw = st.ar_multiconv2d(dev(z), dev(ctx))
        F32_ERR[cfg] = max(np.abs(host(m_raw) - em).max(), np.abs(host(s_raw) - es).max())
    return F32_ERR[cfg]


@pytest.mark.parametrize("shape", build.SHAPES, ids=lambda s: "pxt%d_wco%d_ks%d" % s)
def test_every_fp32_launch_shape_runs_the_resnet_epilogues(amd, shape):
    """A1.  Roles: (a) needs n_z / 16 >= ks chunks (ks = 4: the second configuration); wco = 2 needs n_h / 16 a multiple of 2 nt
    (160: nt 5, 1; 64: nt 2, 1); (c) needs two blocks (the first and third configuration); (e) takes even nt with 4 | 2 n_z / 16 at
    wco = 2.  Every shape of the list reaches all five."""
    seen, _ = _sweep(amd, "f32", shape, (5, 4, 3, 2, 1), CONFIGS)
    assert seen == set(ROLES), "never ran as %s" % sorted(set(ROLES) - seen)


@pytest.mark.parametrize("shape", build.BF3_SHAPES, ids=lambda s: "ppw%d_pxt%d_ks%d_wco%d" % s)
def test_every_bf16x3_launch_shape_runs_the_resnet_epilogues(amd, shape):
    """A2.  The first two configurations (the third has c_in = 16 and 48: no split pack).  Besides the bounds of A1: the split products
    are no worse than twice the exact-fp32 family's error on the same configuration + 1e-6 (the rule of tests/test_hip_bf3.py:98),
    the exact family at the launch shapes it chooses itself, as there -- the smallest of its errors (5.9e-6 / 5.4e-6; its ks = 1 pins
    reach 2.5e-5).  Measured on an MI355X: 4.7e-6 / 4.5e-6 at the K-sliced shapes, 1.26e-5 / 9.6e-6 at (1, 4, 1, 1), which sums all
    of K in one wave: inside the rule's 1.28e-5 / 1.18e-5, the kernels being deterministic."""
    seen, errs = _sweep(amd, "bf3", shape, (5, 4, 2), CONFIGS[:2])
    for cfg, e in sorted(errs.items()):
        exact = _f32_error(amd, cfg)
        print("bf16x3 %s  B%d_h%d_z%d_d%d_%dx%d: %.3g against exact fp32 %.3g" % ((shape,) + cfg + (e, exact)))
        assert e <= 2.0 * exact + 1e-6, "%s: bf16x3 %.3g against exact fp32 %.3g" % (cfg, e, exact)
    assert seen == set(ROLES), "never ran as %s" % sorted(set(ROLES) - seen)


@pytest.mark.parametrize("family,shape,nt", [("f32", (2, 1, 4), 5), ("bf3", (2, 1, 4, 2), 5)], ids=["f32_ks4", "bf16x3_wco2"])
def test_resnet_ar_structure_bit_exact(amd, family, shape, nt):
    """A3.  z changed at (pixel q, channel c) on every image: logsd at every position that precedes or equals (q, c) in the step's
    ordering -- the rows above q, the pixels left of it in its row, the channels up to c at q: the Theano statement's taps look up and
    left, the mirror of test_bf16x3_batch_independence_and_ar_structure_bit_exact -- is bit-identical, and so is z_new but AT (q, c),
    where z itself enters (z_new = (z - m) / exp(s)) and must differ; z_new changes at a later position.  Guards the resnet's own
    prepare path: its conv names, no zero-diagonal but on the output pair, exact zeros in every plane of a masked weight."""
    cfg = CONFIGS[0]
    B, n_h, n_z, depth, H, W = cfg
    w, z, ctx, _, _ = _case(cfg)
    st = amd.ResnetARStack(n_z, n_h, depth)
    if family == "f32":
        st.set_precision("f32")
    st.prepare(_rel(w))
    took = _pin(amd, st, family, shape, nt)
    assert sorted(took) == ([1, 2, 3, 4, 5] if family == "f32" else [0, 1, 2, 3, 4, 5]), took      # (ks = 4: the input conv has two chunks)
    if family == "bf3":
        assert all(st.layer_precision(l, B, H, W) == "bf16x3" for l in took)
    qh, qw, c = 2, 3, 11
    zd, cd = dev(z), dev(ctx)
    z2 = zd.clone()
    z2[:, c, qh, qw] += 0.5
    z_a, s_a = st.iaf_step(zd, cd)
    z_b, s_b = st.iaf_step(z2, cd)
    torch.cuda.synchronize()
    same_s, same_z = (torch.from_numpy(m).cuda() for m in D.unchanged_positions((B, n_z, H, W), qh, qw, c))
    assert int(((s_b != s_a) & same_s).sum()) == 0 and int(((z_b != z_a) & same_z).sum()) == 0
    assert bool((z_b[:, c, qh, qw] != z_a[:, c, qh, qw]).all())
    later = ~same_z
    later[:, c, qh, qw] = False
    assert bool(((z_b != z_a) & later).any()) and bool(((s_b != s_a) & ~same_s).any())
