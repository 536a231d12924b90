#!/usr/bin/env python
"""GPU dev tool: per-call cost of prior 'made' of iaf_amd.CVAELayerIAF at BASELINE configs[1] sizes (B 32, n_h 160, n_z 32, depth_ar 2,
16x16 and 8x8), for both posteriors it is built with: down_q, the training pair (down_q + backward), down_p(exact=True) at tol 1e-6 with
the sweeps it ran and its last residual, down_p(exact=False) (the pack alone), and the prior's step alone.  All rows come from ONE
process; every row is warmed up, then timed between device events over REPS calls, REPEATS times -- the median and the spread
(min .. max) are printed.  --json PATH also writes the rows; --txt PATH writes the printed lines (profiles/made/made_bench.txt; profiles/made/README.md quotes them)."""
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


def params(rng, name, n_z, n_h_list):
    w = {}
    sizes = [n_z] + n_h_list
    for conv in ("_posterior_conv1", "_posterior_conv2", "_prior_conv1"):
        for i in range(len(n_h_list)):
            w["%s%s_%d_w" % (name, conv, i)] = 0.05 * rng.standard_normal((sizes[i + 1], sizes[i] + 1, 3, 3))
            w["%s%s_%d_b" % (name, conv, i)] = 0.1 * rng.standard_normal(sizes[i + 1])
            w["%s%s_%d_s" % (name, conv, i)] = 0.1 * rng.standard_normal(sizes[i + 1])
        for i in range(2):
            w["%s%s_out_%d_w" % (name, conv, i)] = 0.05 * rng.standard_normal((n_z, sizes[-1] + 1, 3, 3))
            w["%s%s_out_%d_b" % (name, conv, i)] = 0.1 * rng.standard_normal(n_z)
            w["%s%s_out_%d_s" % (name, conv, i)] = 0.1 * rng.standard_normal(n_z)
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("made_bench needs a GPU: a CPU run says nothing about these times")
    B, n_z, n_h, d, kl_min, tol = 32, 32, 160, 2, 0.25, 1e-6
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    rows, lines = [], []
    for H in (16, 8):
        rng = np.random.RandomState(0)
        w = {k: dev(v) for k, v in params(rng, "1", n_z, [n_h] * d).items()}
        h_up, h_dn = rng.standard_normal((B, 2 * n_h + 2 * n_z, H, H)), rng.standard_normal((B, 3 * n_h + 2 * n_z, H, H))
        h_up[:, n_h + n_z:n_h + 2 * n_z] *= 0.25
        h_dn[:, 2 * n_h + n_z:2 * n_h + 2 * n_z] *= 0.25
        h_up, h_dn = dev(h_up), dev(h_dn)
        eps = dev(rng.standard_normal((B, n_z, H, H)))
        d_h, d_up = dev(rng.standard_normal((B, n_h + n_z, H, H))), dev(rng.standard_normal((B, n_h, H, H)))
        res, notes = {}, {}
        for posterior in ("down_iaf2_nl", "down_iaf2_nl2"):
            tag = "%s + made: " % posterior
            layer = iaf_amd.CVAELayerIAF("1", n_h, n_z, d, posterior=posterior, kl_min=kl_min, prior="made")
            layer.load(w)
            layer.up(h_up)
            layer.down_q(h_dn, eps=eps)
            st = layer._st
            res[tag + "down_q"] = timed(lambda: layer.down_q(h_dn, eps=eps))
            if posterior == "down_iaf2_nl":
                res["the prior's iaf_step alone"] = timed(lambda: layer.prior_stack.iaf_step(st["z"], st["made_context"]))
                stats = torch.zeros(2, dtype=torch.int32, device="cuda")
                layer.down_p(h_dn, eps, tol=tol, stats=stats)
                torch.cuda.synchronize()
                sweeps, bits = (int(v) for v in stats.cpu().numpy())
                notes["down_p(exact=True)"] = "%d sweeps run of at most 64, last residual %.3g" % (
                    sweeps, float(np.array([bits], dtype=np.int32).view(np.float32)[0]))
                res["down_p(exact=True), tol 1e-6, max_sweeps 64, check_every 4"] = timed(lambda: layer.down_p(h_dn, eps, tol=tol), reps=50)
                res["down_p(exact=False): the pack alone"] = timed(lambda: layer.down_p(h_dn, eps, exact=False))
            train = iaf_amd.CVAELayerIAF("1", n_h, n_z, d, posterior=posterior, kl_min=kl_min, prior="made")
            train.set_training(True)
            train.load(w)
            train.up(h_up)

            def pair():
                train.down_q(h_dn, eps=eps)
                train.backward(d_h, d_obj=1.0, d_up=d_up)

            res[tag + "training pair (down_q + backward)"] = timed(pair)
        head = ("B=%d n_z=%d n_h=%d depth_ar=%d %dx%d, kl_min=%g  (us per call: median [min .. max] of %d windows)"
                % (B, n_z, n_h, d, H, H, kl_min, REPEATS))
        print(head)
        lines.append(head)
        for k, (med, lo, hi) in res.items():
            ln = "  %-62s %8.1f  [%7.1f .. %7.1f]" % (k, med, lo, hi)
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
            json.dump(dict(B=B, n_z=n_z, n_h=n_h, depth_ar=d, kl_min=kl_min, tol=tol, warmup=WARMUP, reps=REPS, repeats=REPEATS, rows=rows),
                      f, indent=1)
    if args.txt:
        os.makedirs(os.path.dirname(os.path.abspath(args.txt)), exist_ok=True)
        with open(args.txt, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
