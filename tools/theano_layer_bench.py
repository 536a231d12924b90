#!/usr/bin/env python
"""GPU dev tool: cost of the plain Theano convs (iaf_conv3x3_create_theano) and of the whole iaf_amd.CVAELayer at n_h 160, n_z 32, B 32,
16x16 and 8x8.

  * Each of the layer's four convs (up_conv1_1 160 -> 384, up_conv2 160 -> 160, down_conv1 160 -> 448, down_conv2_1 192 -> 160, with the
    fused elu / residual the layer uses) in the Theano form against the TF form of the same shape pinned to the same precision (bf16x3:
    the Theano form has no fp16 planes), in the same process, ALTERNATING window by window so that drift hits both alike.  The K loops
    are identical; the Theano form reads its bias from the position-class table.
  * The whole CVAELayer forward (up + down_q) and forward + backward (up + down_q + backward_down + backward_up) per posterior, beside
    the inner CVAELayerIAF alone on the same conv outputs.

Every row is warmed up, then timed between device events over REPS calls, REPEATS times -- median and spread (min .. max).  --txt PATH
writes the printed lines (profiles/theano_layer/theano_layer_bench.txt), --json PATH the rows."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import iaf_amd  # noqa: E402

WARMUP, REPS, REPEATS = 20, 100, 7


def window(fn, reps=REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def stats(v):
    return float(np.median(v)), min(v), max(v)


def timed(fn, reps=REPS):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    return stats([window(fn, reps) for _ in range(REPEATS)])


def timed_pair(fa, fb, reps=REPS):
    """two rows alternating window by window"""
    for _ in range(WARMUP):
        fa()
        fb()
    torch.cuda.synchronize()
    va, vb = [], []
    for _ in range(REPEATS):
        va.append(window(fa, reps))
        vb.append(window(fb, reps))
    return stats(va), stats(vb)


def conv_params(rng, w, base, n_in, n_out):
    w[base + "_w"] = 0.05 * rng.standard_normal((n_out, n_in + 1, 3, 3))
    w[base + "_b"] = 0.1 * rng.standard_normal(n_out)
    w[base + "_s"] = 0.1 * rng.standard_normal(n_out)


def stack_params(rng, w, name, n_z, n_h, depth_ar):
    for i in range(depth_ar):
        conv_params(rng, w, name + "_%d" % i, n_z if i == 0 else n_h, n_h)
    for j in range(2):
        conv_params(rng, w, name + "_out_%d" % j, n_h, n_z)


def layer_params(rng, layer, posterior, prior, n_z, n_h, depth):
    w = {}
    for nm, (a, b) in layer.widths.items():
        conv_params(rng, w, "1" + nm, a, b)
    if posterior == "down_iaf2_deep":
        conv_params(rng, w, "1_deepiaf_input", n_z, n_h)
        for i in range(depth):
            conv_params(rng, w, "1_deepiaf_%d_conv1" % i, n_h, n_h)
            conv_params(rng, w, "1_deepiaf_%d_conv2" % i, n_h, n_h)
        for j in range(2):
            conv_params(rng, w, "1_deepiaf_out_%d" % j, n_h, n_z)
        return w
    stack_params(rng, w, "1_posterior_conv1", n_z, n_h, depth)
    if posterior == "down_iaf2_nl2":
        stack_params(rng, w, "1_posterior_conv2", n_z, n_h, depth)
    if prior == "made":
        stack_params(rng, w, "1_prior_conv1", n_z, n_h, depth)
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("theano_layer_bench needs a GPU: a CPU run says nothing about these times")
    B, n_z, n_h, kl_min = 32, 32, 160, 0.25
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    rows, lines = [], []

    def say(ln):
        print(ln, flush=True)
        lines.append(ln)

    for H in (16, 8):
        rng = np.random.RandomState(0)
        say("B=%d n_z=%d n_h=%d %dx%d  (us per call: median [min .. max] of %d windows of %d calls)" % (B, n_z, n_h, H, H, REPEATS, REPS))
        # ---- the four convs, Theano form against TF form
        convs = [("up_conv1_1", n_h, 2 * n_h + 2 * n_z, False), ("up_conv2", n_h, n_h, True), ("down_conv1", n_h, 2 * n_h + 4 * n_z, False),
                 ("down_conv2_1", n_h + n_z, n_h, True)]
        for name, n_in, n_out, residual in convs:
            x = dev(0.3 * rng.standard_normal((B, n_in, H, H)))
            res = dev(0.3 * rng.standard_normal((B, n_out, H, H))) if residual else None
            th, tf = iaf_amd.WNConv2d(n_in, n_out, theano=True), iaf_amd.WNConv2d(n_in, n_out)
            tf.set_precision("bf16x3")
            th.prepare(dev(0.05 * rng.standard_normal((n_out, n_in + 1, 3, 3))), dev(0.1 * rng.standard_normal(n_out)), dev(0.1 * rng.standard_normal(n_out)))
            tf.prepare(dev(0.05 * rng.standard_normal((3, 3, n_in, n_out))), dev(0.1 * rng.standard_normal(n_out)), dev(0.1 * rng.standard_normal(n_out)))
            fam = ["bf16x3" if c.runs_bf16x3(B, H, H) else "f32" for c in (th, tf)]
            assert fam[0] == fam[1] and not tf.runs_f16x2(B, H, H), fam
            out_th = [torch.empty(B, n_out, H, H, device="cuda")]
            out_tf = [torch.empty(B, n_out, H, H, device="cuda")]
            a, b = timed_pair(lambda: th(x, elu_input=True, residual=res, out=out_th), lambda: tf(x, elu_input=True, residual=res, out=out_tf))
            for form, (med, lo, hi) in (("Theano", a), ("TF", b)):
                say("  %-14s %3d -> %3d %-7s %-6s %8.2f  [%7.2f .. %7.2f]" % (name, n_in, n_out, form, fam[0], med, lo, hi))
                rows.append(dict(H=H, row="%s %s" % (name, form), family=fam[0], median_us=med, min_us=lo, max_us=hi))
            say("  %-14s Theano / TF = %.3f" % (name, a[0] / b[0]))
        # ---- the whole layer per posterior, beside the IAF part alone
        for posterior, prior, depth in (("down_iaf2_nl", "diag", 2), ("down_iaf2_nl2", "diag", 2), ("down_iaf2_deep", "diag", 2), ("down_iaf2_nl", "made", 2)):
            tag = "%s / %s depth %d: " % (posterior, prior, depth)
            up_in, dn_in = dev(0.3 * rng.standard_normal((B, n_h, H, H))), dev(0.3 * rng.standard_normal((B, n_h, H, H)))
            eps = dev(rng.standard_normal((B, n_z, H, H)))
            d_up, d_dn = dev(rng.standard_normal((B, n_h, H, H))), dev(rng.standard_normal((B, n_h, H, H)))
            res = {}
            for training in (False, True):
                layer = iaf_amd.CVAELayer("1", n_h, n_z, depth, posterior=posterior, prior=prior, kl_min=kl_min)
                layer.set_training(training)
                w = {k: dev(v) for k, v in layer_params(np.random.RandomState(1), layer, posterior, prior, n_z, n_h, depth).items()}
                layer.load(w)

                def fwd():
                    layer.up(up_in)
                    return layer.down_q(dn_in, eps=eps)

                def fwd_bwd():
                    fwd()
                    layer.backward_down(d_dn, d_obj=1.0)
                    layer.backward_up(d_up)

                h_up = layer.convs["_up_conv1_1"](up_in, elu_input=True)[0]
                h_dn = layer.convs["_down_conv1"](dn_in, elu_input=True)[0]
                d_h = dev(rng.standard_normal((B, n_h + n_z, H, H)))
                inner = layer.iaf

                def inner_fwd():
                    inner.up(h_up)
                    return inner.down_q(h_dn, eps=eps)

                def inner_fwd_bwd():
                    inner_fwd()
                    inner.backward(d_h, d_obj=1.0, d_up=d_up)

                if training:
                    res[tag + "CVAELayer forward + backward"] = timed(fwd_bwd, 50)
                    res[tag + "CVAELayerIAF alone, forward + backward"] = timed(inner_fwd_bwd, 50)
                else:
                    res[tag + "CVAELayer forward (up + down_q)"] = timed(fwd, 50)
                    res[tag + "CVAELayerIAF alone, forward"] = timed(inner_fwd, 50)
            for k, (med, lo, hi) in res.items():
                say("  %-72s %8.1f  [%7.1f .. %7.1f]" % (k, med, lo, hi))
                rows.append(dict(H=H, row=k, median_us=med, min_us=lo, max_us=hi))
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
