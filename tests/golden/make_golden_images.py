#!/usr/bin/env python3
"""Generate tests/golden/image_grids.npz by EXECUTING THE REFERENCE'S OWN img_stretch / img_tile (tf_utils/common.py:118-168, read-only,
imported behind tf_shim as the other generators do); the two sequences of run_eval (tf_train.py:346-353: every source stretched over
its own slice and interleaved; :363-373: the batch stretched, then the slice shown stretched again) are composed here from those
two functions.  Inputs and expected float grids only.  Build container only.  TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("IAF_REFERENCE", "/root/reference")
sys.path.insert(0, HERE)

H, W = 3, 5          # H != W: a transposition shows

# name: (sources [(key, dtype, rows, stretch_over, then_over)], n_imgs, C, border, border_color)
CASES = {
    "n1_c3":        ([("a", "u8", 1, 1, None)], 1, 3, 0, 0.0),
    "n4_c1_b1":     ([("a", "f32", 4, 4, None)], 4, 1, 1, 0.25),
    "n5_c3_b1":     ([("a", "u8", 5, 5, None)], 5, 3, 1, 0.25),            # empty tiles
    "n5_c1":        ([("a", "f32", 5, 5, None)], 5, 1, 0, 0.0),
    "n6_c3":        ([("a", "f32", 6, 6, None)], 6, 3, 0, 0.0),
    "pair_c3":      ([("a", "u8", 4, 3, None), ("b", "f32", 5, 3, None)], 6, 3, 0, 0.0),      # run_eval's reconstructions
    "pair_c1_b1":   ([("a", "u8", 3, 3, None), ("b", "f32", 3, 2, None)], 5, 1, 1, 0.25),
    "twice_c3":     ([("a", "f32", 7, 7, 4)], 4, 3, 0, 0.0),               # run_eval's samples: the slice's min / max are not the batch's
    "twice_c1_b1":  ([("a", "f32", 6, 5, 3)], 3, 1, 1, 0.25),
    "constant":     ([("a", "f32", 4, 4, None)], 4, 3, 0, 0.0),            # divisor 1e-12
    "constant_u8":  ([("a", "u8", 2, 2, 2)], 2, 1, 0, 0.0),
    "narrow":       ([("a", "f32", 4, 4, None)], 4, 3, 1, 0.25),           # a range of 1e-7
}


def make_input(rng, name, key, dtype, rows, C):
    shape = (rows, C, H, W)
    if name.startswith("constant"):
        return np.full(shape, 7, np.uint8) if dtype == "u8" else np.full(shape, -0.375, np.float32)
    if name == "narrow":
        return (1e-7 * rng.random_sample(shape)).astype(np.float32)
    if dtype == "u8":
        return rng.randint(3, 250, size=shape).astype(np.uint8)
    a = (rng.standard_normal(shape) * 0.3).astype(np.float32)
    if name.startswith("twice"):          # the extremes of the batch lie in the rows that are NOT shown
        a[-1, 0, 0, 0], a[-2, 0, 1, 1] = 4.0, -5.0
    return a


def main():
    import tf_shim
    tf_shim.install()
    sys.path.insert(0, REF)
    from tf_utils.common import img_stretch, img_tile          # the reference's functions, unmodified
    rng = np.random.RandomState(20261)
    out = {}
    for name, (sources, n_imgs, C, border, color) in CASES.items():
        shown = []
        for key, dtype, rows, over, then in sources:
            a = make_input(rng, name, key, dtype, rows, C)
            out["%s/%s" % (name, key)] = a
            bhwc = np.transpose(a, (0, 2, 3, 1))
            s = img_stretch(bhwc[:over])
            if then is not None:
                s = img_stretch(s[:then])
            shown.append(s)
        ns = len(sources)
        plot = np.zeros((n_imgs, H, W, C), np.float32)
        for k in range(ns):
            plot[k::ns] = shown[k][:len(plot[k::ns])]
        out["%s/grid" % name] = img_tile(plot, aspect_ratio=1.0, border=border, border_color=color).astype(np.float32)
    path = os.path.join(HERE, "image_grids.npz")
    np.savez_compressed(path, **out)
    print("wrote image_grids.npz %.1f KiB, numpy %s" % (os.path.getsize(path) / 1024.0, np.__version__))


if __name__ == "__main__":
    main()
