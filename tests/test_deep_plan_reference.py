"""Coverage proof of the masked ResNet sweeps (tests/test_hip_deep_geometry.py, tests/test_hip_deep_shapes.py), without a GPU:
  * the case table RESNET_CASES, labelled by the plain-Python restatement of the host's launch plan (tests/deep_plan_reference.py),
    holds a case in every class the backward sweep was written for; a class that loses its last case fails here by name;
  * the fp64 reference the forward bound (1e-4 absolute) is held against moves by more than 100 x that bound when one conv of the
    network is taken out or the skip term is dropped, so a kernel that loses a layer cannot pass;
  * the positions the bit-exact autoregressive test of tests/test_hip_deep_shapes.py calls "earlier" are the ones the fp64 statement
    leaves unchanged."""
import numpy as np
import pytest

import deep_plan_reference as D
import deep_reference as DR
import backward_plan_reference as R

PLANS = D.all_resnet_plans()          # (case, plan)
RES = [(c, e) for c, pl in PLANS for e in pl["layers"] if e["epi"] == "EPI_DGRAD_RES"]
ROLES = {"input": "n_z->n_h", "conv1": "n_h->n_h", "conv2": "n_h->n_h", "conv2_last": "n_h->n_h", "out": "n_h->2n_z"}
# what the restated auto_shape returns for an EPI_DGRAD_RES launch over D.CHANNELS and every P <= 4400: (pxt, wco, ks), either mode
REACHABLE = [(1, 1, 4), (1, 2, 2), (2, 1, 2), (2, 2, 1), (4, 1, 1)]
UNREACHABLE = [(4, 1, 2), (2, 2, 2), (2, 1, 4)]
BF3_REACHABLE = [(1, 4, 1, 1), (2, 1, 4, 1)]          # (ppw, pxt, ks, wco)


def _any(seq):
    return any(True for _ in seq)


def test_reachable_dgrad_shapes_are_the_listed_ones():
    """the lists of the module docstring of deep_plan_reference.py, found by enumeration"""
    for mode in ("RAW", "SKIP"):
        shapes, full = D.reachable_dgrad_shapes(mode)
        assert shapes == REACHABLE, (mode, shapes)
        assert {s[0] for s in full} == {1, 2, 5}
    assert sorted(REACHABLE + UNREACHABLE) == sorted(D.SHAPES)
    assert {s[2] for s in REACHABLE} == {1, 2, 4} and {s[0] for s in REACHABLE} == {1, 2, 4}
    assert all(s in D.BF3_SHAPES for s in BF3_REACHABLE)


CLASSES = {}
for _mode in ("RAW", "SKIP"):
    for _s in REACHABLE:          # on the exact-fp32 kernel: at the default precision, or in the "f32" run of a case whose data gradient is split
        CLASSES["dgrad_res_%s_f32_pxt%d_wco%d_ks%d" % ((_mode,) + _s)] = (lambda m, s: lambda: _any(
            e for _, e in RES if e["mode"] == m and e["f32_shape"][1:] == s))(_mode, _s)
    for _nt in (1, 2, 5):
        CLASSES["dgrad_res_%s_f32_nt%d" % (_mode, _nt)] = (lambda m, n: lambda: _any(
            e for _, e in RES if e["mode"] == m and e["f32_shape"][0] == n))(_mode, _nt)
    for _s in BF3_REACHABLE:
        CLASSES["dgrad_res_%s_bf16x3_ppw%d_pxt%d_ks%d_wco%d" % ((_mode,) + _s)] = (lambda m, s: lambda: _any(
            e for _, e in RES if e["mode"] == m and e["split"] and e["shape"][1:] == s))(_mode, _s)
    CLASSES["dgrad_res_%s_bf16x3_nt5" % _mode] = (lambda m: lambda: _any(
        e for _, e in RES if e["mode"] == m and e["split"] and e["shape"][0] == 5))(_mode)
for _form in D.SKIP_FORMS_REACHABLE:
    CLASSES["dgrad_skip_with_%s" % _form] = (lambda f: lambda: _any(e for _, e in RES if e["mode"] == "SKIP" and e["form"] == f))(_form)
    CLASSES["dgrad_skip_with_%s_bf16x3" % _form] = (lambda f: lambda: _any(
        e for _, e in RES if e["mode"] == "SKIP" and e["form"] == f and e["split"]))(_form)
CLASSES["P_below_16"] = lambda: _any(pl for _, pl in PLANS if pl["P"] < 16)
CLASSES["P_above_16_not_a_multiple"] = lambda: _any(pl for _, pl in PLANS if pl["P"] > 16 and pl["P"] % 16)
CLASSES["P_multiple_of_16"] = lambda: _any(pl for _, pl in PLANS if pl["P"] % 16 == 0)
CLASSES["P_more_than_one_workgroup_ragged"] = lambda: _any(pl for _, pl in PLANS if pl["P"] > 64 and pl["P"] % 64)
for _nm, _pred in (("1x1", lambda H, W: H == 1 and W == 1), ("1xW", lambda H, W: H == 1 and W > 1), ("Hx1", lambda H, W: H > 1 and W == 1)):
    CLASSES["image_%s_batch_1" % _nm] = (lambda f: lambda: _any(1 for c, _ in PLANS if f(c[4], c[5]) and c[3] == 1))(_pred)
    CLASSES["image_%s_batch_above_1" % _nm] = (lambda f: lambda: _any(1 for c, _ in PLANS if f(c[4], c[5]) and c[3] > 1))(_pred)
    CLASSES["image_%s_depth_above_1" % _nm] = (lambda f: lambda: _any(1 for c, _ in PLANS if f(c[4], c[5]) and c[2] > 1))(_pred)
CLASSES["split_rule_last_below_4096"] = lambda: _any(
    pl for c, pl in PLANS if pl["P"] == R.STACK_DGRAD_BF3_MIN_P - 1 and not any(pl["dgrad_split"]) and
    all(D.resnet_plan(c[0], c[1], c[2], 4096, 1, 1)["dgrad_split"]))
CLASSES["split_rule_first_at_4096_every_layer"] = lambda: _any(pl for _, pl in PLANS if pl["P"] == 4096 and all(pl["dgrad_split"]))
CLASSES["split_rule_at_4096_input_conv_stays_f32"] = lambda: _any(
    pl for c, pl in PLANS if pl["P"] == 4096 and c[0] % 32 and not pl["dgrad_split"][0] and all(pl["dgrad_split"][1:]))
CLASSES["n_h_160_from_2048_pixels_leaves_ks4"] = lambda: _any(
    e for c, e in RES if c[1] == 160 and c[3] * c[4] * c[5] >= 2048 and e["f32_shape"][3] != 4)
for _d in D.DEPTHS:
    CLASSES["depth_%d" % _d] = (lambda d: lambda: _any(1 for c, _ in PLANS if c[2] == d))(_d)
for _ch in D.CHANNELS:
    CLASSES["channels_%d_%d" % _ch] = (lambda ch: lambda: _any(1 for c, _ in PLANS if c[:2] == ch))(_ch)


def _wgrad_classes_reachable():
    """(conv kind, kernel) over D.CHANNELS and every P <= 4400 at the default (split) precision"""
    out = set()
    for n_z, n_h in D.CHANNELS:
        for kind, (ci, co) in (("n_z->n_h", (n_z, n_h)), ("n_h->n_h", (n_h, n_h)), ("n_h->2n_z", (n_h, 2 * n_z))):
            for P in range(1, D.P_MAX_ENUMERATED + 1):
                out.add((kind, R.wgrad_plan(P, ci, co, R.NTAPS_STACK, True)["kernel"]))
    return out


WGRAD_REACHABLE = _wgrad_classes_reachable()
for _kind, _kernel in sorted(WGRAD_REACHABLE):
    CLASSES["wgrad_%s_%s" % (_kind.replace("->", "_to_"), _kernel)] = (lambda kd, kn: lambda: _any(
        e for _, e in [(c, e) for c, pl in PLANS for e in pl["layers"]] if ROLES[e["role"]] == kd and e["wgrad"]["kernel"] == kn))(_kind, _kernel)


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_the_table_has_a_case_in_every_class(name):
    assert CLASSES[name](), "no case of RESNET_CASES is in class %s" % name


def test_every_weight_gradient_class_is_reachable():
    """narrow, wide and bf3 for each of the three conv kinds, but for one"""
    want = {(k, n) for k in ("n_z->n_h", "n_h->n_h", "n_h->2n_z") for n in ("narrow", "wide", "bf3")}
    # the output pair never runs the narrow kernel: its 2 n_z packed channels are a multiple of 32, which wide_shape always covers
    assert all(R.wide_shape(2 * n_z) is not None for n_z, _ in D.CHANNELS)
    assert WGRAD_REACHABLE == want - {("n_h->2n_z", "narrow")}


def test_skip_forms_of_the_restated_walk():
    """MODE_DGRAD_SKIP is launched with y2 or with out0, never with neither: iaf_step_backward refuses a NULL dcontext (iaf_engine.hip:2381)
    and gives every conv1 past block 0 a y2 (:2491)"""
    for depth in D.DEPTHS:
        forms = [D.layer_dgrad(l, depth) for l in range(2 * depth + 2)]
        assert forms[0] == ("EPI_DGRAD", "Z", None) and forms[-1] == ("EPI_DGRAD_RES", "RAW", "y2")
        assert [f[2] for f in forms if f[1] == "SKIP"] == ["out0"] + ["y2"] * (depth - 1)
        assert all(f == ("EPI_DGRAD", "ELU", None) for l, f in enumerate(forms) if l and l % 2 == 0)
    assert D.SKIP_FORMS_REACHABLE == ("y2", "out0")


def test_restatement_on_shapes_worked_out_by_hand():
    """auto_shape as read off the C++ by hand.  16 -> 16 at P = 1 (one chunk, one tile): only ks = 1 shapes with nt = 1, wco = 1 pass:
    (4, 1, 1) with T = 1 (5 * 128 * 1 + 6000) + 0 - 0.01 = 6639.99.  160 -> 160 at P = 4096, 10 chunks and tiles: (4, 1, 1) at nt 5 is
    2 x 64 = 128 workgroups, one round: 5 * 10 * 5 * 128 + 6000 = 38000; (2, 1, 4) at nt 5: 256 workgroups, one round,
    (50 / 4) * 5 * 128 * 2 + 6000 + 1200 = 23200; (1, 1, 4) at nt 5: 512 workgroups, two rounds of 8000 + 6000: 29200;
    (2, 1, 2) at nt 5: 256 workgroups, 25 * 5 * 128 + 6000 + 400 = 22400; (4, 1, 2) at nt 5: 128 workgroups of 8 waves: 2 x 16000 +
    6400 = 38400; (2, 2, 2): 8 waves: 38400; (1, 2, 2) at nt 5: 256 workgroups, 16000 + 6400 = 22400.006, later in the list; (2, 2, 1) at
    nt 5: 128 workgroups, 32000 + 6000.  So (5, 2, 1, 2)."""
    assert D.auto_shape(16, 1, 1, False, 1, 1) == (1, 4, 1, 1)
    assert D.auto_shape(160, 10, 10, False, 4096, 16) == (5, 2, 1, 2)
    assert D.conv_lds_bytes(160, 7, 5, 2, 1, 4) == 4 * ((32 + 8 + 1) * 168 + 4 * 2 * 1 * 5 * 256)
    assert D.dgrad_problem(160, 64) == (64, 4, 10)
    assert D.bf3_dgrad_shape(64, 64, 4096) == (4, 2, 1, 4, 1) and D.bf3_dgrad_shape(64, 64, 4095) is None
    assert D.bf3_dgrad_shape(32, 32, 4096) == (2, 1, 4, 1, 1) and D.bf3_dgrad_shape(16, 32, 4096) is None
    assert D.bf3_dgrad_shape(160, 64, 4352) == (5, 2, 1, 4, 1)
    pl = D.resnet_plan(16, 32, 1, 16, 16, 16)
    assert pl["dgrad_split"] == [False, True, True, True]


def test_ids_are_unique_and_the_table_is_the_size_asked_for():
    ids = [D.resnet_id(c) for c in D.RESNET_CASES]
    assert len(set(ids)) == len(ids) == D.N_CASES == 40
    assert D.RESNET_CASES[:len(D.RESNET_FIXED)] == D.RESNET_FIXED and D.DEFERRED_CASE == R.DEFERRED_CASE
    for n_z, n_h, d, B, H, W in D.RESNET_CASES:
        assert (n_z, n_h) in D.CHANNELS and d in D.DEPTHS
        assert B * H * W <= D.P_MAX_ENUMERATED


# ---------------------------------------------------------------- sensitivity of the fp64 reference
ATOL = 1e-4
A_CONFIGS = D.FORWARD_CONFIGS          # B, n_h, n_z, depth, H, W: tests/test_hip_deep_shapes.py
_THREE = [(16, 16, 1, 1, 1, 1), (64, 64, 2, 5, 1, 7), (32, 160, 2, 5, 6, 11)]          # 1 x 1 at the smallest channels; 1 x W; ten tiles
assert all(c in D.RESNET_CASES for c in _THREE)
SENSITIVITY = list(A_CONFIGS) + [(c[3], c[1], c[0], c[2], c[4], c[5]) for c in _THREE]


def _mutated(z, ctx, w, n_z, n_h, depth, zero=None, drop_skip=None):
    """DR.resnet with conv `zero` giving zeros, or block `drop_skip` computing h = 0.1 conv2(.) without its skip term"""
    conv = lambda x, nm, ci, co, zd: (np.zeros((x.shape[0], co) + x.shape[2:]) if nm == zero else DR._conv(x, w, "r_" + nm, ci, co, zd))
    h = conv(z, "input", n_z, n_h, False) + ctx
    for i in range(depth):
        t = DR._elu(conv(DR._elu(h), "%d_conv1" % i, n_h, n_h, False))
        h = (0.0 if i == drop_skip else h) + 0.1 * conv(t, "%d_conv2" % i, n_h, n_h, False)
    return [conv(h, "out_%d" % j, n_h, n_z, True) for j in range(2)]


@pytest.mark.parametrize("cfg", SENSITIVITY, ids=lambda c: "B%d_h%d_z%d_d%d_%dx%d" % c)
def test_the_reference_moves_when_a_layer_is_missing(cfg):
    """with the weights of D.rand_params (the _s scale raised from deep_reference's 0.1 to 0.2: its docstring has the figures), zeroing
    any one conv of the network or dropping any block's skip term moves m_raw or s_raw by more than 100 x the forward bound"""
    B, n_h, n_z, depth, H, W = cfg
    rng = np.random.RandomState(5000 + n_h + depth + H)
    w = D.rand_params(rng, "r", n_z, n_h, depth)
    z, ctx = rng.standard_normal((B, n_z, H, W)), rng.standard_normal((B, n_h, H, W))
    m, s = DR.resnet(z, ctx, w, "r", n_z, n_h, depth)
    m0, s0 = _mutated(z, ctx, w, n_z, n_h, depth)
    assert np.array_equal(m, m0) and np.array_equal(s, s0)
    muts = [dict(zero=nm) for nm in DR.conv_names(depth)] + [dict(drop_skip=i) for i in range(depth)]
    for mut in muts:
        m1, s1 = _mutated(z, ctx, w, n_z, n_h, depth, **mut)
        moved = max(np.abs(m1 - m).max(), np.abs(s1 - s).max())
        print("%s: moves the outputs by %.3g" % (mut, moved))
        assert moved > 100 * ATOL, (mut, moved)


def test_what_precedes_a_position_in_the_steps_ordering():
    """Theano ordering (the taps look up and left): a change of z at (pixel q, channel c) leaves logsd unchanged at every pixel above q's
    row, left of q in its row, and at q for the channels up to c; z_new there too, except at (q, c) itself, where z enters directly"""
    B, n_h, n_z, depth, H, W = 1, 32, 16, 1, 3, 4
    rng = np.random.RandomState(5100)
    w = DR.rand_params(rng, "r", n_z, n_h, depth)
    z, ctx = rng.standard_normal((B, n_z, H, W)), rng.standard_normal((B, n_h, H, W))
    qh, qw, c = 1, 2, 5
    z2 = z.copy()
    z2[:, c, qh, qw] += 0.5
    zn, ls = DR.deep_step(z, ctx, w, "r", n_z, n_h, depth)
    zn2, ls2 = DR.deep_step(z2, ctx, w, "r", n_z, n_h, depth)
    same_s, same_z = D.unchanged_positions((B, n_z, H, W), qh, qw, c)
    assert np.array_equal(ls2[same_s], ls[same_s]) and np.array_equal(zn2[same_z], zn[same_z])
    assert not same_z[:, c, qh, qw].any() and same_s[:, c, qh, qw].all() and zn2[0, c, qh, qw] != zn[0, c, qh, qw]
    # later positions do move: the later channels of q, its right neighbour, the pixel below it
    assert (ls2 != ls)[:, c + 1:, qh, qw].all() and (zn2 != zn)[:, :, qh, qw + 1].all() and (zn2 != zn)[:, :, qh + 1, qw].all()
