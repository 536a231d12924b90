"""What the host code decides for ONE backward call, restated in plain Python, and the case tables of the backward geometry sweep.

THIS IS A RESTATEMENT.  It was written by reading the C++ and it can drift from it: nothing keeps the two equal.  Its only job is to LABEL the
cases of tests/test_hip_backward_geometry.py (which weight-gradient kernel, how many pixel ranges, which of them are empty, ...) and to let
tests/test_backward_plan_reference.py PROVE that the case tables reach every class of launch plan the sweep was written for.  It is never an
oracle for values: every value the GPU tests compare comes from torch-fp64 autograd (oracle/iaf_grad_oracle.py).

The development knobs of the host code -- the environment variables IAF_WGRAD_WIDE, IAF_WGRAD_BF3 and IAF_WGRAD_NRANGE -- are assumed UNSET,
as are launch shapes pinned by set_tuning / autotune: the restatement follows the default branches only.

Source lines restated (iaf_amd/csrc):
  wide_shape            iaf_engine.hip            wgrad_wide_shape                                          :1995-2011
  bf3_ncob              iaf_wgrad_bf3.hip         iaf_wgrad_bf3_ncob                                        :292-298
  wgrad_plan            iaf_engine.hip            wgrad_plan :2027-2072, px_per_range in launch_wgrad       :2234, :2245
                        iaf_kernels_backward.hpp  r0 / r1 of a range :75-76, :191-192; iaf_wgrad_bf3.hip    :90-91
  conv_plan             iaf_conv3x3_host.hpp      iaf_conv3x3_backward: fold_db :897, choice3 / dgrad16 :921-922, launch_wgrad :928,
                                                  nslab / px_per_slab :929-930; conv3x3_bf3_shape :288-314 (size rule and tile coverage);
                                                  conv3x3_create :86, :98 (tile counts, which convs have split packs)
                        iaf_engine.hip            gemm_layer_set_training :353-359 (the transposed problem and its split pack)
  stack_plan            iaf_engine.hip            iaf_step_backward: nslab / px_per_slab :2342-2343, launch_wgrad per layer :2397;
                                                  auto_shape_bf3 :1049-1065 and bf3_select :1068-1078 (size rule, tile-count divisibility)
NOT restated: the LDS bound of the split data-gradient kernels (bf3_plain_lds_bytes / bf3_lds_bytes <= 160 KiB) and the lists of compiled launch
shapes (iaf_variants.def).  `dgrad_split` therefore says "the size rule and the tile arithmetic pass", not "the split kernel certainly ran"."""
import numpy as np

NTAPS_STACK, NTAPS_PLAIN = 5, 9
WGRAD_MAX_RANGES = 32
DGRAD_BF3_MIN_P, DGRAD_F16_MIN_P, STACK_DGRAD_BF3_MIN_P = 4096, 2048, 4096
CONV_DB_FOLD_MAX_P = 256 * 64          # fold_db: ceil(P / 64) <= 256
STACK_SLAB_FULL_P = 256 * 32           # nslab = min(ceil(P / 32), 256): past this the slabs hold more than 32 pixels


def wide_shape(c_out):
    """(BW, NB) of iaf_wgrad_wide_kernel for c_out packed output channels, or None: the narrow kernel"""
    if c_out % 32 != 0:
        return None
    if c_out % 64 == 0:
        n = c_out // 64
        nb = 3 if n % 3 == 0 else 2 if n % 2 == 0 else 1
        if nb > 1 or n == 1:
            return (4, nb)
    n = c_out // 32
    for c in range(7, 0, -1):
        if n % c == 0:
            return (2, c)


def bf3_ncob(c_in, c_out):
    """output tiles per workgroup of iaf_wgrad_bf3_kernel, 0 = the conv is not covered"""
    if c_in <= 0 or c_out <= 0 or c_in % 32 != 0 or c_out % 16 != 0:
        return 0
    for c in (14, 12, 10, 4):
        if (c_out // 16) % c == 0:
            return c
    return 0


def wgrad_plan(P, c_in, c_out, ntaps, split):
    """the weight-gradient launch of one conv.  dict(kernel "bf3" | "wide" | "narrow", shape (ncob | (BW, NB) | NCOT), gx, gz, nrange,
    px_per_range, step (pixels per K step: 32 | 16), empty (ranges that start at or past P), ragged_last (the last non-empty range ends
    inside a K step))"""
    w = {}
    ncob = bf3_ncob(c_in, c_out) if (split and P % 8 == 0 and P >= 64) else 0
    if ncob > 0:
        rows = 3 if ntaps == NTAPS_PLAIN else 2
        gx, gz = rows * (c_in // 32), (c_out // 16) // ncob
        n = 512 // (gx * gz)
        if n > WGRAD_MAX_RANGES:
            n = 256 // (gx * gz)
        n = max(1, min(n, WGRAD_MAX_RANGES, P // 64))
        w.update(kernel="bf3", shape=ncob, step=32)
    else:
        gx = ntaps * ((c_in + 31) // 32)
        off32 = P * max(c_in, c_out) * 4 < (1 << 32)
        ws = wide_shape(c_out) if (off32 and c_in % 16 == 0) else None
        if ws:
            gz = c_out // (ws[0] * ws[1] * 16)
            w.update(kernel="wide", shape=ws, step=16)
        else:
            ncot = next(c for c in (14, 12, 10, 8, 7, 6, 5, 4, 3, 2, 1) if (c_out // 16) % c == 0)
            gz = (c_out // 16) // ncot
            w.update(kernel="narrow", shape=ncot, step=16)
        if P // 64 >= 16:
            n = 8 if gx * gz >= 40 else 16
        elif P // 64 >= 8:
            n = 8
        else:
            n = max(1, min(512 // gx, P // 64))
    step = w["step"]
    px = ((P + n - 1) // n + step - 1) // step * step
    nonempty = sum(1 for r in range(n) if r * px < P)
    w.update(gx=gx, gz=gz, nrange=n, px_per_range=px, empty=n - nonempty, ragged_last=(P % step) != 0)
    return w


def _plain_dgrad_shape(n_tiles, P):
    """conv3x3_bf3_shape's choice of (nt, wco) for `n_tiles` output tiles of the (transposed) problem, minus its LDS and compiled-shape
    tests; None = no candidate covers the tiles"""
    cand = ((4, 3), (5, 2), (4, 2), (2, 3), (5, 1), (4, 1), (2, 2), (2, 1))
    nblk = (P + 31) // 32
    best, best_wgs = None, 0
    for nt, wco in cand:
        per = nt * wco
        covered = (n_tiles + per - 1) // per * per
        if (covered - n_tiles) * 8 > n_tiles:
            continue
        wgs = nblk * (covered // per)
        if wgs >= 256:
            best = (nt, wco)
            break
        if wgs > best_wgs:
            best_wgs, best = wgs, (nt, wco)
    if best is None:
        return None
    per = best[0] * best[1]
    covered = (n_tiles + per - 1) // per * per
    return best if (covered - n_tiles) * 4 <= n_tiles else None         # bf3_ragged_ok


def conv_plan(B, H, W, c_in, c_out, precision="f32"):
    """WNConv2d.backward (channel counts on the MFMA path: multiples of 16) at one precision ("f32" | "bf16x3" | "f16x2")"""
    assert c_in % 16 == 0 and c_out % 16 == 0
    P = B * H * W
    split = precision != "f32"
    fold = (P + 63) // 64 <= 256
    nslab = (P + 63) // 64 if fold else 256
    px_per_slab = (P + nslab - 1) // nslab
    # the transposed problem T reads c_out channels and writes c_in: its split pack exists when c_out / 16 is even
    has_t3 = (c_out // 16) % 2 == 0
    f16 = precision == "f16x2" and has_t3
    thr = DGRAD_F16_MIN_P if f16 else DGRAD_BF3_MIN_P
    dgrad_split = split and has_t3 and P >= thr and _plain_dgrad_shape(c_in // 16, P) is not None
    return dict(P=P, W=W, wgrad=wgrad_plan(P, c_in, c_out, NTAPS_PLAIN, split), db_folded=fold, nslab=nslab, px_per_slab=px_per_slab,
                last_slab_partial=(P % px_per_slab) != 0, dgrad_split=dgrad_split, dgrad_kernel=("f16x2" if f16 else "bf16x3") if dgrad_split else "f32",
                dgrad_threshold=thr if (split and has_t3) else None)


def stack_layers(n_z, n_h, depth):
    """(c_in, c_out) of the GEMM layers of ARStack(n_z, [n_h] * depth): hidden convs, then the two output convs as ONE layer"""
    sizes = [n_z] + [n_h] * depth
    return [(sizes[i], sizes[i + 1]) for i in range(depth)] + [(sizes[-1], 2 * n_z)]


def _stack_dgrad_split(c_in, c_out, P):
    """auto_shape_bf3 on the transposed problem of a layer (reads c_out, writes c_in), minus the LDS and compiled-shape tests"""
    if P < STACK_DGRAD_BF3_MIN_P or (c_out // 16) % 2 != 0 or c_out % 32 != 0:
        return False
    n_tiles = c_in // 16
    short_k = c_out // 32 == 1
    for nt in (5, 4, 2):
        if n_tiles % nt != 0:
            continue
        if short_k and nt == 5 and n_tiles % 2 == 0:
            continue
        return True
    return False


def stack_plan(B, H, W, n_z, n_h, depth, split=True):
    """ARStack.iaf_step_backward (split: the stack's precision is not "f32"; the default precision is "bf16x3")"""
    P = B * H * W
    nslab = min((P + 31) // 32, 256)
    px_per_slab = (P + nslab - 1) // nslab
    layers = stack_layers(n_z, n_h, depth)
    return dict(P=P, W=W, wgrad=[wgrad_plan(P, ci, co, NTAPS_STACK, split) for ci, co in layers], nslab=nslab, px_per_slab=px_per_slab,
                last_slab_partial=(P % px_per_slab) != 0, dgrad_split=[split and _stack_dgrad_split(ci, co, P) for ci, co in layers])


# --------------------------------------------------------------------------------------
# case tables of tests/test_hip_backward_geometry.py
# --------------------------------------------------------------------------------------
# plain conv: (B, c_in, c_out, H, W, forms).  forms: e = elu_input, x = split input (x2), y = split dys, s = dy_scale 0.1,
# r = dx_residual, n = want_dx False.  Channels stay at the smallest values that reach a path; P grows through B and odd H x W.
CONV_CASES = [
    (5, 16, 80, 13, 16, "e"),        # P 1040 = 16.25 x 64: narrow 5, 16 ranges of 80, 3 empty
    (13, 16, 32, 8, 10, "xy"),       # P 1040: wide (2,1), 3 empty
    (2, 32, 160, 20, 13, "es"),      # P 520 = 8.1 x 64: wide (2,5), 8 ranges, 1 empty, ragged; split: bf16x3 ncob 10, 2 empty
    (3, 32, 64, 8, 11, "r"),         # P 264: split: bf16x3 ncob 4, 1 empty; fp32: wide (4,1), 4 ranges, ragged
    (2, 16, 96, 5, 13, "esr"),       # wide (2,3), 2 ranges, ragged
    (1, 32, 112, 9, 1, "y"),         # H x 1, B = 1: narrow 7
    (1, 16, 352, 3, 5, "n"),         # wide (2,1) at 11 x 32 channels
    (257, 16, 16, 8, 8, "e"),        # P 16448 > 16384: db not folded, 256 slabs of 65 (last one partial, two empty); narrow 1, 16 ranges
    (3, 32, 32, 37, 37, "er"),       # P 4107 (% 32 = 11, % 8 = 3), W 37: past the bf16x3 data-gradient threshold; split wgrad falls back
    (2, 16, 48, 7, 11, "xs"),        # P 154: narrow 3, c_in 16, 2 ranges, ragged
    (3, 16, 48, 12, 13, "ey"),       # P 468 = 7.3 x 64: 7 ranges of 80, 1 empty, ragged
    (5, 16, 32, 14, 14, ""),         # P 980 = 15.3 x 64: 8 ranges
    (13, 16, 176, 8, 10, "s"),       # P 1040, narrow 1 with gz 11: gx * gz = 99 >= 40 -> 8 ranges
    (1, 32, 64, 8, 8, "e"),          # split precision at P = 64 exactly: bf16x3 weight gradient, one range of two K blocks
    (1, 32, 64, 7, 8, "x"),          # split precision at P = 56: below the bf16x3 weight gradient's 64
    (3, 32, 64, 5, 7, "es"),         # split precision, P 105 (% 8 = 1): falls back to the fp32 kernels
    (5, 32, 32, 21, 39, "e"),        # P 4095: last below the bf16x3 data-gradient threshold, past the f16x2 one, W 39, % 32 = 31
    (4, 32, 32, 32, 32, "r"),        # P 4096: first at the bf16x3 data-gradient threshold, W 32
    (1, 32, 32, 89, 23, "es"),       # P 2047: last below the f16x2 data-gradient threshold
    (2, 32, 32, 32, 32, "y"),        # P 2048: first at the f16x2 data-gradient threshold
    (2, 16, 128, 3, 5, "e"),         # wide (4,2)
    (1, 16, 192, 5, 3, "x"),         # wide (4,3)
    (3, 32, 224, 2, 19, "s"),        # wide (2,7); split: ncob 14, P 114 (% 8 = 2) falls back
    (1, 16, 288, 1, 7, "e"),         # 1 x W, B = 1: wide (2,3) at 9 x 32 channels
    (1, 16, 704, 3, 5, ""),          # wide (2,2), reachable only at c_out = 704
    (1, 16, 16, 1, 1, "e"),          # 1 x 1, B = 1
    (5, 32, 64, 1, 1, "r"),          # 1 x 1, B = 5
    (3, 16, 80, 1, 7, "y"),          # 1 x W, B = 3
    (2, 16, 48, 9, 1, "es"),         # H x 1, B = 2
]
WIDE_SHAPES_LEFT_OUT = []            # (2,2) at c_out = 704 is in: at c_in 16 and 15 pixels it costs milliseconds


def conv_precisions(case):
    """the precisions a plain-conv case runs at: "f32" always; the split ones where a split kernel could take part of the backward
    (c_in % 32 == 0: the bf16x3 weight gradient; or the data gradient's size rule passes)"""
    B, ci, co, H, W = case[:5]
    if ci % 32 == 0 or any(conv_plan(B, H, W, ci, co, p)["dgrad_split"] for p in ("bf16x3", "f16x2")):
        return ("f32", "bf16x3", "f16x2")
    return ("f32",)


def conv_labels(case, precision):
    """short class label of a plain-conv case for the parametrised id"""
    B, ci, co, H, W = case[:5]
    pl = conv_plan(B, H, W, ci, co, precision)
    w = pl["wgrad"]
    shape = "x".join(str(v) for v in w["shape"]) if isinstance(w["shape"], tuple) else str(w["shape"])
    lab = "%s%s_r%d" % (w["kernel"], shape, w["nrange"])
    if w["empty"]:
        lab += "_empty%d" % w["empty"]
    if w["ragged_last"]:
        lab += "_ragged"
    if not pl["db_folded"]:
        lab += "_dbslabs"
    if pl["dgrad_split"]:
        lab += "_dx-" + pl["dgrad_kernel"]
    return lab


def conv_id(case):
    B, ci, co, H, W, forms = case
    return "B%d_%dto%d_%dx%d_%s_%s" % (B, ci, co, H, W, forms or "plain", conv_labels(case, "f32"))


# stack: (seed, n_z, n_h, depth, B, H, W).  The first block is fixed (thresholds and the images whose taps see only padding), the rest is
# drawn with a fixed seed from the channel pairs, depths, geometries and batch sizes of the sweep.
STACK_CHANNELS = [(16, 16), (16, 32), (32, 64), (16, 80), (32, 160)]
STACK_GEOMETRIES = [(1, 1), (1, 7), (9, 1), (2, 19), (3, 5), (7, 7), (6, 11)]
STACK_BATCHES = [1, 2, 3, 5]
STACK_FIXED = [
    (0, 16, 32, 1, 129, 8, 8),       # P 8256 = 8192 + one image: 256 slabs of 33, last one partial
    (1, 32, 64, 1, 5, 21, 39),       # P 4095: last below the data gradient's bf16x3 threshold, W 39
    (2, 32, 64, 1, 3, 37, 37),       # P 4107: past it, W 37, ragged 32-pixel block
    (3, 32, 64, 2, 4, 32, 32),       # P 4096: first at it, W 32
    (4, 16, 16, 0, 1, 1, 1), (5, 32, 64, 2, 3, 1, 1),
    (6, 16, 80, 1, 1, 1, 7), (7, 16, 32, 3, 5, 1, 7),
    (8, 32, 160, 1, 1, 9, 1), (9, 16, 16, 2, 2, 9, 1),
]


def stack_cases():
    rng = np.random.RandomState(2025)
    cases = list(STACK_FIXED)
    for i in range(len(STACK_FIXED), 24):
        n_z, n_h = STACK_CHANNELS[rng.randint(len(STACK_CHANNELS))]
        d = int(rng.randint(0, 4))
        B = int(STACK_BATCHES[rng.randint(len(STACK_BATCHES))])
        H, W = STACK_GEOMETRIES[rng.randint(len(STACK_GEOMETRIES))]
        cases.append((i, n_z, n_h, d, B, H, W))
    return cases


def stack_id(case):
    seed, n_z, n_h, d, B, H, W = case
    pl = stack_plan(B, H, W, n_z, n_h, d)
    kinds = "+".join("%s%s" % (w["kernel"], "x".join(str(v) for v in w["shape"]) if isinstance(w["shape"], tuple) else w["shape"])
                     for w in pl["wgrad"])
    lab = "%s_r%d" % (kinds, max(w["nrange"] for w in pl["wgrad"]))
    if any(pl["dgrad_split"]):
        lab += "_dx-bf16x3"
    if pl["P"] > STACK_SLAB_FULL_P:
        lab += "_slabs%d" % pl["px_per_slab"]
    return "s%d_z%d_h%d_d%d_B%d_%dx%d_%s" % (seed, n_z, n_h, d, B, H, W, lab)


# the other families of the sweep, (n_z, n_h, depth, B, H, W [, extra])
THEANO_CASES = [(16, 32, 1, 3, 3, 5, False), (32, 64, 2, 2, 2, 19, True), (16, 80, 1, 1, 9, 1, False)]      # extra: flipmask
POSTERIOR_CASES = [(16, 32, 1, 3, 7, 7, 0.25), (32, 64, 2, 2, 6, 11, 0.0), (16, 16, 1, 5, 1, 7, 0.25)]      # extra: kl_min
DEFERRED_CASE = (32, 64, 2, 3, 6, 11)
# border property: plain convs (B, c_in, c_out, H, W) and stacks (n_z, n_h, depth, B, H, W) on 1 x 1, 1 x W and H x 1 images
BORDER_CONV_CASES = [(3, 16, 48, 1, 1), (5, 32, 64, 1, 1), (3, 16, 32, 1, 7), (3, 32, 64, 9, 1)]
BORDER_STACK_CASES = [(16, 32, 2, 3, 1, 1), (32, 64, 1, 5, 1, 1), (16, 16, 1, 3, 1, 7), (16, 80, 1, 3, 9, 1)]


def all_conv_plans():
    """every (case, precision, plan) the plain-conv family runs"""
    return [(c, p, conv_plan(c[0], c[3], c[4], c[1], c[2], p)) for c in CONV_CASES for p in conv_precisions(c)]


def all_stack_plans():
    """every (case, plan) the stack families run at the stack's default (split) precision"""
    cs = [c[1:] for c in stack_cases()] + [c[:6] for c in THEANO_CASES] + [c[:6] for c in POSTERIOR_CASES] + [DEFERRED_CASE]
    return [(c, stack_plan(c[3], c[4], c[5], c[0], c[1], c[2])) for c in cs]
