"""Coverage proof of the backward geometry sweep (tests/test_hip_backward_geometry.py): its case tables, labelled by the plain-Python
restatement of the host's launch plan (tests/backward_plan_reference.py), contain at least one case in every class of plan the sweep was
written for.  Runs without a GPU.  A class that loses its last case fails here by name."""
import pytest

import backward_plan_reference as R

CONV = R.all_conv_plans()          # (case, precision, plan)
STACK = R.all_stack_plans()        # (case, plan)
WGRADS = [(pl["P"], c[1], pl["wgrad"], prec != "f32") for c, prec, pl in CONV] + \
         [(pl["P"], ci, w, True) for c, pl in STACK for (ci, _), w in zip(R.stack_layers(c[0], c[1], c[2]), pl["wgrad"])]
FP32_WGRADS = [t for t in WGRADS if t[2]["kernel"] != "bf3"]
IMAGES = [(c[0], c[3], c[4]) for c in R.CONV_CASES] + [(c[3], c[4], c[5]) for c, _ in STACK] + \
         [(c[0], c[3], c[4]) for c in R.BORDER_CONV_CASES] + [(c[3], c[4], c[5]) for c in R.BORDER_STACK_CASES]


def _reachable_wide_shapes(max_c_out):
    return sorted({R.wide_shape(co) for co in range(16, max_c_out + 1, 16)} - {None})


def _any(seq):
    return any(True for _ in seq)


CLASSES = {}          # class name -> does some case of the sweep fall into it?
for _ncot in (1, 3, 5, 7):
    CLASSES["narrow_ncot%d" % _ncot] = (lambda n: lambda: _any(w for _, _, w, _ in WGRADS if w["kernel"] == "narrow" and w["shape"] == n))(_ncot)
CLASSES["narrow_more_than_one_range"] = lambda: _any(w for _, _, w, _ in WGRADS if w["kernel"] == "narrow" and w["nrange"] > 1)
CLASSES["narrow_c_in_16"] = lambda: _any(w for _, ci, w, _ in WGRADS if w["kernel"] == "narrow" and ci == 16)
for _ws in _reachable_wide_shapes(448) + [(2, 2)]:
    if _ws not in R.WIDE_SHAPES_LEFT_OUT:
        CLASSES["wide_%dx%d" % _ws] = (lambda s: lambda: _any(w for _, _, w, _ in WGRADS if w["kernel"] == "wide" and w["shape"] == s))(_ws)
for _k in ("narrow", "wide", "bf3"):
    CLASSES["empty_ranges_%s" % _k] = (lambda k: lambda: _any(w for _, _, w, _ in WGRADS if w["kernel"] == k and w["empty"] >= 1))(_k)
CLASSES["more_than_one_empty_range"] = lambda: _any(w for _, _, w, _ in WGRADS if w["empty"] > 1)
for _k in ("narrow", "wide"):
    CLASSES["ragged_last_range_of_several_%s" % _k] = (lambda k: lambda: _any(
        w for P, _, w, _ in WGRADS if w["kernel"] == k and P % 16 != 0 and w["nrange"] - w["empty"] > 1))(_k)
for _q in (7, 8, 15, 16):
    CLASSES["P_div_64_is_%d" % _q] = (lambda q: lambda: _any(w for P, _, w, _ in FP32_WGRADS if P // 64 == q))(_q)
CLASSES["gx_gz_below_40_at_16_blocks"] = lambda: _any(w for P, _, w, _ in FP32_WGRADS if P // 64 >= 16 and w["gx"] * w["gz"] < 40 and w["nrange"] == 16)
CLASSES["gx_gz_from_40_at_16_blocks"] = lambda: _any(w for P, _, w, _ in FP32_WGRADS if P // 64 >= 16 and w["gx"] * w["gz"] >= 40 and w["nrange"] == 8)
CLASSES["split_falls_back_P_not_multiple_of_8"] = lambda: _any(
    w for P, ci, w, split in WGRADS if split and P % 8 != 0 and P >= 64 and ci % 32 == 0 and w["kernel"] != "bf3")
CLASSES["split_at_P_64"] = lambda: _any(w for P, _, w, split in WGRADS if split and P == 64 and w["kernel"] == "bf3")
CLASSES["split_at_P_56"] = lambda: _any(w for P, ci, w, split in WGRADS if split and P == 56 and ci % 32 == 0 and w["kernel"] != "bf3")


def _conv_dx(kernel):
    return [pl for _, prec, pl in CONV if pl["dgrad_kernel"] == kernel]


for _k, _thr in (("bf16x3", R.DGRAD_BF3_MIN_P), ("f16x2", R.DGRAD_F16_MIN_P)):
    CLASSES["conv_dx_%s_ragged_block" % _k] = (lambda k: lambda: _any(pl for pl in _conv_dx(k) if pl["P"] % 32 != 0))(_k)
    CLASSES["conv_dx_%s_other_width" % _k] = (lambda k: lambda: _any(pl for pl in _conv_dx(k) if pl["W"] not in (8, 16)))(_k)
    CLASSES["conv_dx_%s_first_at_threshold" % _k] = (lambda k, t: lambda: _any(pl for pl in _conv_dx(k) if pl["P"] == t))(_k, _thr)
    CLASSES["conv_dx_%s_last_below_threshold" % _k] = (lambda k, t: lambda: _any(
        pl for _, prec, pl in CONV if prec == k and pl["dgrad_threshold"] == t and pl["P"] == t - 1 and not pl["dgrad_split"]))(_k, _thr)
CLASSES["stack_dx_split_ragged_block"] = lambda: _any(pl for _, pl in STACK if any(pl["dgrad_split"]) and pl["P"] % 32 != 0)
CLASSES["stack_dx_split_other_width"] = lambda: _any(pl for _, pl in STACK if any(pl["dgrad_split"]) and pl["W"] not in (8, 16))
CLASSES["stack_dx_first_at_threshold"] = lambda: _any(pl for _, pl in STACK if any(pl["dgrad_split"]) and pl["P"] == R.STACK_DGRAD_BF3_MIN_P)
CLASSES["stack_dx_last_below_threshold"] = lambda: _any(
    pl for c, pl in STACK if pl["P"] == R.STACK_DGRAD_BF3_MIN_P - 1 and not any(pl["dgrad_split"]) and
    any(R._stack_dgrad_split(ci, co, R.STACK_DGRAD_BF3_MIN_P) for ci, co in R.stack_layers(c[0], c[1], c[2])))
CLASSES["conv_db_not_folded"] = lambda: _any(pl for _, _, pl in CONV if pl["P"] > R.CONV_DB_FOLD_MAX_P and not pl["db_folded"])
CLASSES["conv_db_not_folded_partial_last_slab"] = lambda: _any(pl for _, _, pl in CONV if not pl["db_folded"] and pl["last_slab_partial"])
CLASSES["conv_db_folded_partial_last_slab"] = lambda: _any(pl for _, _, pl in CONV if pl["db_folded"] and pl["P"] % 64 != 0)
CLASSES["stack_slabs_past_8192"] = lambda: _any(pl for _, pl in STACK if pl["P"] > R.STACK_SLAB_FULL_P and pl["px_per_slab"] > 32)
CLASSES["stack_slabs_past_8192_partial_last_slab"] = lambda: _any(pl for _, pl in STACK if pl["P"] > R.STACK_SLAB_FULL_P and pl["last_slab_partial"])
CLASSES["stack_partial_last_slab"] = lambda: _any(pl for _, pl in STACK if pl["P"] <= R.STACK_SLAB_FULL_P and pl["P"] % 32 != 0)
for _nm, _pred in (("1x1", lambda H, W: H == 1 and W == 1), ("1xW", lambda H, W: H == 1 and W > 1), ("Hx1", lambda H, W: H > 1 and W == 1)):
    CLASSES["image_%s_batch_1" % _nm] = (lambda f: lambda: _any(1 for B, H, W in IMAGES if f(H, W) and B == 1))(_pred)
    CLASSES["image_%s_batch_above_1" % _nm] = (lambda f: lambda: _any(1 for B, H, W in IMAGES if f(H, W) and B > 1))(_pred)


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_the_sweep_has_a_case_in_every_class(name):
    assert CLASSES[name](), "no case of the backward geometry sweep is in class %s" % name


def test_reachable_wide_shapes():
    """the shapes the restated rule can return: seven up to c_out = 448, and (2, 2) first at c_out = 704"""
    assert _reachable_wide_shapes(448) == [(2, 1), (2, 3), (2, 5), (2, 7), (4, 1), (4, 2), (4, 3)]
    assert (2, 2) not in _reachable_wide_shapes(703) and R.wide_shape(704) == (2, 2)
    assert R.WIDE_SHAPES_LEFT_OUT == []


def test_restatement_on_shapes_worked_out_by_hand():
    """the plans of a few shapes as read off the C++ by hand (9 taps; B, c_in, c_out, H, W)"""
    def w(B, ci, co, H, W, split=False):
        return R.wgrad_plan(B * H * W, ci, co, 9, split)
    p = w(5, 16, 80, 13, 16)
    assert (p["kernel"], p["shape"], p["nrange"], p["px_per_range"], p["empty"]) == ("narrow", 5, 16, 80, 3)
    p = w(13, 16, 32, 8, 10)
    assert (p["kernel"], p["shape"], p["nrange"], p["empty"]) == ("wide", (2, 1), 16, 3)
    p = w(2, 32, 160, 20, 13)
    assert (p["kernel"], p["shape"], p["nrange"], p["px_per_range"], p["empty"], p["ragged_last"]) == ("wide", (2, 5), 8, 80, 1, True)
    p = w(2, 32, 160, 20, 13, True)
    assert (p["kernel"], p["shape"], p["nrange"], p["px_per_range"], p["empty"]) == ("bf3", 10, 8, 96, 2)
    p = w(3, 32, 64, 8, 11, True)
    assert (p["kernel"], p["shape"], p["nrange"], p["empty"]) == ("bf3", 4, 4, 1)
    assert w(2, 16, 96, 5, 13)["shape"] == (2, 3) and w(1, 32, 112, 9, 1)["shape"] == 7 and w(1, 16, 352, 3, 5)["shape"] == (2, 1)
    assert w(1, 16, 176, 1, 1)["shape"] == 1 and w(1, 16, 208, 1, 1)["shape"] == 1
    # P 1040 and 520 in 80-pixel ranges
    assert w(1, 16, 16, 1040, 1)["empty"] == 3 and w(1, 16, 16, 520, 1)["empty"] == 1
    c = R.conv_plan(257, 8, 8, 16, 16)
    assert (c["P"], c["db_folded"], c["nslab"], c["px_per_slab"], c["last_slab_partial"]) == (16448, False, 256, 65, True)
    assert R.conv_plan(256, 8, 8, 16, 16)["db_folded"]
    c = R.conv_plan(3, 37, 37, 32, 32, "bf16x3")
    assert c["P"] == 4107 and c["dgrad_split"] and c["wgrad"]["kernel"] == "wide"
    assert not R.conv_plan(3, 37, 37, 32, 32, "f32")["dgrad_split"]
    s = R.stack_plan(129, 8, 8, 16, 32, 1)
    assert (s["P"], s["nslab"], s["px_per_slab"], s["last_slab_partial"]) == (8256, 256, 33, True)


def test_ids_are_unique_and_every_case_is_on_the_mfma_path():
    ids = [R.conv_id(c) for c in R.CONV_CASES]
    assert len(set(ids)) == len(ids)
    ids = [R.stack_id(c) for c in R.stack_cases()]
    assert len(set(ids)) == len(ids) and 20 <= len(ids) <= 30
    for c in R.CONV_CASES:
        assert c[1] % 16 == 0 and c[2] % 16 == 0
        if "x" in c[5]:
            assert "r" not in c[5]              # dx_residual goes with a single input
    for c, _ in STACK:
        assert (c[0], c[1]) in R.STACK_CHANNELS
