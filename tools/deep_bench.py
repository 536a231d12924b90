#!/usr/bin/env python
"""GPU dev tool: per-call cost of the posterior 'down_iaf2_deep' of iaf_amd.CVAELayerIAF (the masked ResNet inside the IAF step) at
B 32, n_z 32, n_h 160, 16x16 and 8x8, depth 1, 2 and 4: iaf_step of the resnet stack (2 depth + 2 conv launches), down_q, and the training
pair (down_q + backward); and, from the same process as the yardstick, the rows of 'down_iaf2_nl' at depth_ar 2 -- its step in one
launch (the default) and layer by layer (3 conv launches), down_q, the training pair.  Every row is warmed up, then timed between device
events over REPS calls, REPEATS times -- the median and the spread (min .. max) are printed.  --json PATH also writes the rows; --txt
PATH writes the printed lines (profiles/deep/deep_bench.txt; profiles/deep/README.md quotes them)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import iaf_amd  # noqa: E402

WARMUP, REPS, REPEATS = 20, 200, 7


def timed(fn, reps=REPS):
    """us per call: (median, min, max) over REPEATS windows of `reps` calls between two device events"""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)
    return float(np.median(out)), min(out), max(out)


def conv_params(rng, w, base, n_in, n_out):
    w[base + "_w"] = 0.05 * rng.standard_normal((n_out, n_in + 1, 3, 3))
    w[base + "_b"] = 0.1 * rng.standard_normal(n_out)
    w[base + "_s"] = 0.1 * rng.standard_normal(n_out)


def deep_params(rng, name, n_z, n_h, depth):
    w = {}
    conv_params(rng, w, name + "_deepiaf_input", n_z, n_h)
    for i in range(depth):
        conv_params(rng, w, name + "_deepiaf_%d_conv1" % i, n_h, n_h)
        conv_params(rng, w, name + "_deepiaf_%d_conv2" % i, n_h, n_h)
    for j in range(2):
        conv_params(rng, w, name + "_deepiaf_out_%d" % j, n_h, n_z)
    return w


def plain_params(rng, name, n_z, n_h, depth_ar):
    w = {}
    for i in range(depth_ar):
        conv_params(rng, w, name + "_posterior_conv1_%d" % i, n_z if i == 0 else n_h, n_h)
    for j in range(2):
        conv_params(rng, w, name + "_posterior_conv1_out_%d" % j, n_h, n_z)
    return w


def layer_rows(res, tag, make, w, h_up, h_dn, eps, d_h, d_up):
    layer = make()
    layer.load(w)
    layer.up(h_up)
    layer.down_q(h_dn, eps=eps)
    res[tag + "down_q"] = timed(lambda: layer.down_q(h_dn, eps=eps))
    train = make()
    train.set_training(True)
    train.load(w)
    train.up(h_up)

    def pair():
        train.down_q(h_dn, eps=eps)
        train.backward(d_h, d_obj=1.0, d_up=d_up)

    res[tag + "training pair (down_q + backward)"] = timed(pair)
    return layer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deep_bench needs a GPU: a CPU run says nothing about these times")
    B, n_z, n_h, kl_min = 32, 32, 160, 0.25
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    rows, lines = [], []
    for H in (16, 8):
        rng = np.random.RandomState(0)
        h_up, h_dn = rng.standard_normal((B, 2 * n_h + 2 * n_z, H, H)), rng.standard_normal((B, 2 * n_h + 4 * n_z, H, H))
        h_up[:, n_h + n_z:n_h + 2 * n_z] *= 0.25
        h_dn[:, n_h + n_z:n_h + 2 * n_z] *= 0.25
        h_dn[:, n_h + 3 * n_z:n_h + 4 * n_z] *= 0.25
        h_up, h_dn = dev(h_up), dev(h_dn)
        eps = dev(rng.standard_normal((B, n_z, H, H)))
        z, ctx = dev(rng.standard_normal((B, n_z, H, H))), dev(rng.standard_normal((B, n_h, H, H)))
        d_h, d_up = dev(rng.standard_normal((B, n_h + n_z, H, H))), dev(rng.standard_normal((B, n_h, H, H)))
        res, notes = {}, {}
        for depth in (1, 2, 4):
            tag = "down_iaf2_deep depth %d: " % depth
            w = {k: dev(v) for k, v in deep_params(rng, "1", n_z, n_h, depth).items()}
            layer = layer_rows(res, tag, lambda: iaf_amd.CVAELayerIAF("1", n_h, n_z, depth, posterior="down_iaf2_deep", kl_min=kl_min),
                               w, h_up, h_dn, eps, d_h, d_up)
            st = layer.stack
            res[tag + "iaf_step of the resnet stack (%d conv launches)" % (2 * depth + 2)] = timed(lambda: st.iaf_step(z, ctx))
            notes[tag + "forward layers on"] = ", ".join(st.layer_precision(l, B, H, H) for l in range(st.depth_ar + 1))
        tag = "down_iaf2_nl depth_ar 2: "
        w = {k: dev(v) for k, v in plain_params(rng, "1", n_z, n_h, 2).items()}
        layer = layer_rows(res, tag, lambda: iaf_amd.CVAELayerIAF("1", n_h, n_z, 2, posterior="down_iaf2_nl", kl_min=kl_min),
                           w, h_up, h_dn, eps, d_h, d_up)
        st = layer.stack
        res[tag + "iaf_step, one launch (%d rows per workgroup)" % st.step_is_fused(B, H, H)] = timed(lambda: st.iaf_step(z, ctx))
        st.set_fuse_step(0)
        assert st.step_is_fused(B, H, H) == 0
        res[tag + "iaf_step, layer by layer (3 conv launches)"] = timed(lambda: st.iaf_step(z, ctx))
        head = ("B=%d n_z=%d n_h=%d %dx%d, kl_min=%g  (us per call: median [min .. max] of %d windows)" % (B, n_z, n_h, H, H, kl_min, REPEATS))
        print(head)
        lines.append(head)
        for k, (med, lo, hi) in res.items():
            ln = "  %-72s %8.1f  [%7.1f .. %7.1f]" % (k, med, lo, hi)
            print(ln)
            lines.append(ln)
            rows.append(dict(H=H, W=H, row=k, median_us=med, min_us=lo, max_us=hi))
        for k, v in notes.items():
            ln = "  %s: %s" % (k, v)
            print(ln)
            lines.append(ln)
            rows.append(dict(H=H, W=H, row=k, note=v))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(dict(B=B, n_z=n_z, n_h=n_h, kl_min=kl_min, warmup=WARMUP, reps=REPS, repeats=REPEATS, rows=rows), f, indent=1)
    if args.txt:
        os.makedirs(os.path.dirname(os.path.abspath(args.txt)), exist_ok=True)
        with open(args.txt, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
