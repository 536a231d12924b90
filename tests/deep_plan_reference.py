"""What the host code decides for the launches of a masked ResNet stack (iaf_stack_create_resnet / iaf_amd.ResnetARStack), restated in plain
Python, and the case table of tests/test_hip_deep_geometry.py.

THIS IS A RESTATEMENT.  It was written by reading the C++ and it can drift from it: nothing keeps the two equal.  Its only job is to LABEL
the cases of tests/test_hip_deep_geometry.py (which compiled launch shape each data gradient runs, in which mode and output form, which
weight-gradient kernel) and to let tests/test_deep_plan_reference.py PROVE that the table reaches every class the sweep was written for.  It
is never an oracle for values: every value the GPU tests compare comes from tests/deep_reference.py in fp64.

Launch shapes pinned by set_tuning / set_tuning_bf3 and the development knobs of the host code (tests/backward_plan_reference.py names
them) are assumed UNSET: the restatement follows the default branches only.  The lists of compiled shapes are iaf_amd.build.SHAPES /
BF3_SHAPES, the parsed csrc/iaf_variants.def, in its search order.

Source lines restated (iaf_amd/csrc/iaf_engine.hip):
  conv_lds_bytes     :444-454   (IAF_SHARED_W is not defined by the build: no weight buffers)
  auto_shape         :1025-1047 (the exact-fp32 family's launch-shape model; ties keep the earlier candidate)
  dgrad_problem      gemm_layer_set_training :356-365: T[l] reads L[l].c_out channels and writes L[l].c_in (nchunk and ncot swap)
  layer_dgrad        layer_dgrad_epi :785-787 and iaf_step_backward's walk :2475-2499 (mode, and what a MODE_DGRAD_SKIP launch writes)
  bf3_dgrad_shape    auto_shape_bf3 :1091-1107 on T[l] (through bf3_select :1110-1121), minus its LDS bound
  resnet_layers      iaf_stack_create_resnet :582-594, run_resnet :1581-1616
The weight gradients and the 4096-pixel rule of the split data gradient are backward_plan_reference.wgrad_plan / _stack_dgrad_split.

The three output forms of MODE_DGRAD_SKIP (iaf_conv_kernel.hpp:704-717): with y2 (conv1 of a block > 0: 0.1 d h_i is the dY of block i - 1's
conv2), with out0 (conv1 of block 0: d h_0 is d context, NCHW), with neither.  iaf_step_backward reaches the first two only: layer 1 gets
out0 = dcontext, which the entry point refuses as NULL (:2381), and every other odd layer gets y2 (:2491-2492).  "neither" is compiled
and unreachable; SKIP_FORMS_REACHABLE says so and the CPU test holds the restated walk to it.

Compiled and unreachable without a pin, for EPI_DGRAD_RES under the default plan (found by enumerating the restated auto_shape over the
channel sets below and every P <= 4400, test_deep_plan_reference.py::test_reachable_dgrad_shapes_are_the_listed_ones holds the lists):
  exact-fp32 family (pxt, wco, ks): (4, 1, 2), (2, 2, 2), (2, 1, 4), in RAW and in SKIP mode alike: the three shapes of eight waves per
      workgroup, which the model charges two passes over a CU's four SIMDs.  The two other wco = 2 shapes ARE reached, in narrow
      windows of P at n_h = 160 only: (1, 2, 2) at 801 <= P <= 816 and (2, 2, 1) at 1601 <= P <= 1632, both with nt = 1;
  bf16x3 family (ppw, pxt, ks, wco): (4, 1, 4, 1), (1, 1, 4, 1), (2, 1, 4, 2), (1, 1, 4, 2): auto_shape_bf3 returns (2, 1, 4, 1) or,
      for a single c_in pair, (1, 4, 1, 1), and ppw = 4 only for the output pair's FORWARD launch from 32768 pixels on.
Reached by default, either mode: (4, 1, 1), (2, 1, 2), (1, 1, 4), (2, 2, 1), (1, 2, 2) with nt in {1, 2, 5}; split: (2, 1, 4, 1), (1, 4, 1, 1).
Forward, every compiled shape of both families is reached for EPI_RES and EPI_HIDDEN by pinning: tests/test_hip_deep_shapes.py."""
import math

import numpy as np

import backward_plan_reference as R
from iaf_amd import build as BUILD

SHAPES = list(BUILD.SHAPES)              # exact-fp32 family: (pxt, wco, ks)
BF3_SHAPES = list(BUILD.BF3_SHAPES)      # bf16x3 family: (ppw, pxt, ks, wco)
LDS_MAX = 160 * 1024
SKIP_FORMS_REACHABLE = ("y2", "out0")    # of ("y2", "out0", "neither"): see the module docstring


def conv_lds_bytes(cin, W, nt, pxt, wco, ks, full3x3=False):
    nslot = 16 * pxt + (2 if full3x3 else 1) * (W + 1)
    fl = (nslot + 1) * (cin + 8)
    if ks > 1:
        fl += ks * pxt * wco * nt * 256
    return 4 * fl


def bf3_lds_bytes(cin, W, nt, ppw, pxt, ks, wco=1):
    """iaf_engine.hip:432-436"""
    tile = (16 * ppw * pxt + W + 1 + 1) * (3 * (cin // 8) + 2) * 16
    red = pxt * wco * ks * ppw * nt * 1024 if ks > 1 else 0
    return max(tile, red)


def auto_shape(cin, nchunk, ncot, is_out, P, W):
    """(nt, pxt, wco, ks) of the exact-fp32 kernel for a GEMM problem of `nchunk` 16-channel K chunks and `ncot` output tiles, or None:
    no candidate passes and the descriptor keeps what it had"""
    best, pick = 1e30, None
    for si, (pxt, wco, ks) in enumerate(SHAPES):
        if nchunk < ks:
            continue
        for nt in range(5, 0, -1):
            if is_out and nt % 2:
                continue
            if ncot % (nt * wco):
                continue
            if conv_lds_bytes(cin, W, nt, pxt, wco, ks) > LDS_MAX:
                continue
            wgs = float((P + 16 * pxt - 1) // (16 * pxt)) * (ncot // (nt * wco))
            rounds = math.ceil(wgs / 256.0)
            cyc_wave = (5.0 * nchunk / ks) * nt * 128.0
            cyc_wg = cyc_wave * math.ceil(pxt * wco * ks / 4.0)
            T = rounds * (cyc_wg + 6000.0) + 400.0 * (ks - 1) + 1e-3 * si - 1e-2 * nt
            if T < best:
                best, pick = T, (nt, pxt, wco, ks)
    return pick


def resnet_layers(n_z, n_h, depth):
    """(c_in, c_out) of the GEMM layers: the input conv, conv1 / conv2 of every block, the two output convs as ONE layer"""
    return [(n_z, n_h)] + [(n_h, n_h)] * (2 * depth) + [(n_h, 2 * n_z)]


def layer_role(l, depth):
    d = 2 * depth + 1
    return "out" if l == d else "input" if l == 0 else "conv1" if l % 2 else "conv2_last" if l == d - 1 else "conv2"


def dgrad_problem(c_in, c_out):
    """the transposed problem of a forward layer: (cin, nchunk, ncot)"""
    return c_out, c_out // 16, c_in // 16


def layer_dgrad(l, depth):
    """(epilogue, mode, output form) of layer l's data-gradient launch"""
    d = 2 * depth + 1
    if l == 0:
        return "EPI_DGRAD", "Z", None
    if l == d:
        return "EPI_DGRAD_RES", "RAW", "y2"               # y = da[0], y2 = da[d - 1] = 0.1 d h_D
    if l % 2:
        return "EPI_DGRAD_RES", "SKIP", "y2" if l > 1 else "out0"
    return "EPI_DGRAD", "ELU", None


def bf3_dgrad_shape(c_in, c_out, P):
    """(nt, ppw, pxt, ks, wco) of the split data gradient of a forward layer c_in -> c_out, or None: the exact-fp32 kernel runs"""
    if not R._stack_dgrad_split(c_in, c_out, P):
        return None
    n_tiles, short_k = c_in // 16, c_out // 32 == 1
    for nt in (5, 4, 2):
        if n_tiles % nt or (short_k and nt == 5 and n_tiles % 2 == 0):
            continue
        shape = (nt, 1, 4, 1, 1) if short_k else (nt, 2, 1, 4, 1)
        assert shape[1:] in BF3_SHAPES
        return shape if bf3_lds_bytes(c_out, 1, *shape) <= LDS_MAX else None        # (W adds slots; the GPU test asserts the outcome)
    return None


def resnet_plan(n_z, n_h, depth, B, H, W, split=True):
    """ResnetARStack.iaf_step_backward at the stack's default (split) precision or at "f32": per layer the data gradient's epilogue,
    mode, output form, kernel family and launch shape, and the weight gradient's plan"""
    P = B * H * W
    out = []
    for l, (ci, co) in enumerate(resnet_layers(n_z, n_h, depth)):
        epi, mode, form = layer_dgrad(l, depth)
        b3 = bf3_dgrad_shape(ci, co, P) if split else None
        cin, nchunk, ncot = dgrad_problem(ci, co)
        f32_shape = auto_shape(cin, nchunk, ncot, False, P, W) or (1, 4, 1, 1)       # (gemm_layer_set_training's initial shape)
        out.append(dict(layer=l, role=layer_role(l, depth), epi=epi, mode=mode, form=form, split=b3 is not None,
                        shape=b3 if b3 else f32_shape, f32_shape=f32_shape, wgrad=R.wgrad_plan(P, ci, co, R.NTAPS_STACK, split)))
    return dict(P=P, W=W, H=H, layers=out, dgrad_split=[e["split"] for e in out])


# --------------------------------------------------------------------------------------
# the case table of tests/test_hip_deep_geometry.py: (n_z, n_h, depth, B, H, W)
# --------------------------------------------------------------------------------------
CHANNELS = [(16, 16), (16, 32), (32, 64), (16, 80), (32, 160), (64, 64)]
DEPTHS = [1, 2, 3]
GEOMETRIES = [(1, 1), (1, 7), (9, 1), (2, 19), (3, 5), (7, 7), (6, 11)]
BATCHES = [1, 2, 3, 5]
P_MAX_ENUMERATED = 4400
RESNET_FIXED = [
    (32, 64, 1, 15, 13, 21),         # P 4095: last below the split rule
    (32, 64, 1, 16, 16, 16),         # P 4096: first at it, every layer on the split products
    (16, 32, 1, 16, 16, 16),         # P 4096: the input conv has no split pack (c_in 16), its data gradient no tile count (1)
    (32, 64, 2, 3, 37, 37),          # P 4107 (% 32 = 11), W 37, depth 2: the split MODE_DGRAD_SKIP with y2 and with out0
    (32, 160, 1, 9, 16, 16),         # P 2304 at n_h = 160: auto_shape leaves the ks = 4 shapes for (nt 2, pxt 4, wco 1, ks 1)
    (16, 16, 1, 1, 1, 1), (32, 64, 2, 3, 1, 1),              # 1 x 1
    (16, 80, 1, 1, 1, 7), (64, 64, 2, 5, 1, 7),              # 1 x W
    (32, 160, 1, 1, 9, 1), (16, 32, 3, 2, 9, 1),             # H x 1
    (16, 16, 2, 1, 4, 4),            # P 16 exactly
    (32, 160, 2, 5, 6, 11),          # P 330 at n_h = 160: SKIP at (1, 1, 1, 4), with y2 and with out0
    (32, 160, 1, 2, 27, 15),         # P 810 in 801 .. 816: the window of (nt 1, pxt 1, wco 2, ks 2), RAW and SKIP
    (32, 160, 1, 5, 14, 23),         # P 1610 in 1601 .. 1632: the window of (1, 2, 2, 1), RAW and SKIP
    (32, 160, 1, 4, 17, 25),         # P 1700: (5, 1, 1, 4), RAW and SKIP
    (16, 80, 1, 13, 16, 16),         # P 3328: RAW at (5, 2, 1, 2), SKIP at (5, 1, 1, 4)
    (32, 160, 1, 13, 16, 16),        # P 3328: SKIP at (5, 2, 1, 2)
    (32, 160, 1, 17, 16, 16),        # P 4352: the split data gradients at nt = 5; at "f32" RAW at (5, 4, 1, 1)
    (64, 64, 1, 4, 16, 16),          # P 1024 at n_z = n_h: RAW at (1, 1, 1, 4), the last before (1, 2, 1, 2)
    (32, 64, 1, 9, 13, 21),          # P 2457: (1, 4, 1, 1)
]
N_CASES = 40
DEFERRED_CASE = (32, 64, 2, 3, 6, 11)


def resnet_cases():
    rng = np.random.RandomState(2026)
    cases = list(RESNET_FIXED)
    while len(cases) < N_CASES:
        n_z, n_h = CHANNELS[rng.randint(len(CHANNELS))]
        d = int(DEPTHS[rng.randint(len(DEPTHS))])
        B = int(BATCHES[rng.randint(len(BATCHES))])
        H, W = GEOMETRIES[rng.randint(len(GEOMETRIES))]
        c = (n_z, n_h, d, B, H, W)
        if c not in cases:
            cases.append(c)
    return cases


RESNET_CASES = resnet_cases()


def _shape_label(shape):
    return "".join(str(v) for v in shape)


def resnet_id(case):
    n_z, n_h, d, B, H, W = case
    pl = resnet_plan(n_z, n_h, d, B, H, W)
    raw = pl["layers"][-1]
    skip = pl["layers"][1]
    lab = "raw%s%s_skip%s%s" % ("B" if raw["split"] else "F", _shape_label(raw["shape"]), "B" if skip["split"] else "F", _shape_label(skip["shape"]))
    return "z%d_h%d_d%d_B%d_%dx%d_%s" % (n_z, n_h, d, B, H, W, lab)


def all_resnet_plans():
    return [(c, resnet_plan(*c)) for c in RESNET_CASES + [DEFERRED_CASE]]


# the configurations of tests/test_hip_deep_shapes.py: (B, n_h, n_z, depth, H, W)
FORWARD_CONFIGS = [
    (3, 160, 32, 2, 5, 7),           # 10 co tiles; 105 pixels = 6 full 16-pixel tiles + 9: more than one workgroup even at pxt = 4
    (3, 64, 64, 1, 5, 7),            # n_z / 16 = 4 K chunks: the input conv accepts ks = 4; depth 1: the only block is the last one
    (2, 48, 16, 2, 3, 5),            # 3 co tiles: nt = 3 (n_z = 16: n_z and n_h must divide one another, iaf_stack_create_resnet :587)
]
S_SCALE = 0.2


def rand_params(rng, name, n_z, n_h, depth):
    """the inputs of the new sweeps: deep_reference.rand_params with the _s entries at twice its scale (0.2 for 0.1).  At 0.1 the fp64
    reference of the 1 x 1, 16-channel case moves by 0.0085 when block 0's conv1 is zeroed, below 100 x the forward bound; at 0.2 every
    single conv and every skip term moves it by 0.019 or more (tests/test_deep_plan_reference.py holds that)."""
    import deep_reference as DR
    w = DR.rand_params(rng, name, n_z, n_h, depth)
    for k in w:
        if k.endswith("_s"):
            w[k] = w[k] * (S_SCALE / 0.1)
    return w


def unchanged_positions(shape, qh, qw, c):
    """boolean [B, n_z, H, W] pair (logsd, z_new): the positions a change of z at (pixel (qh, qw), channel c) cannot reach in the step's
    ordering (Theano statement, tap_sign = -1: a conv reads the row above and the pixel to the left; at the pixel itself an output
    channel reads the input channels before it, ar.py:243-276).  logsd: the rows above, the pixels left of q in its row, and at q the
    channels up to and including c.  z_new = (z - m) / exp(s) the same, except (q, c) itself, where z enters directly."""
    same = np.zeros(shape, dtype=bool)
    same[:, :, :qh, :] = True
    same[:, :, qh, :qw] = True
    same[:, :c + 1, qh, qw] = True
    same_z = same.copy()
    same_z[:, c, qh, qw] = False
    return same, same_z


def reachable_dgrad_shapes(mode, p_max=P_MAX_ENUMERATED):
    """the exact-fp32 launch shapes (pxt, wco, ks) -- and with them the (nt, pxt, wco, ks) -- the restated auto_shape returns for the
    EPI_DGRAD_RES launch of `mode` ("RAW": the output pair's transposed problem, "SKIP": a conv1's) over CHANNELS and every P <= p_max"""
    shapes, full = set(), set()
    for n_z, n_h in CHANNELS:
        ci, co = (n_h, 2 * n_z) if mode == "RAW" else (n_h, n_h)
        cin, nchunk, ncot = dgrad_problem(ci, co)
        for P in range(1, p_max + 1):
            s = auto_shape(cin, nchunk, ncot, False, P, 7)
            shapes.add(s[1:])
            full.add(s)
    return sorted(shapes), sorted(full)
