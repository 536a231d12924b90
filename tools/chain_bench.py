#!/usr/bin/env python
"""GPU dev tool: per-call cost of the 'down_iaf2_nl2' posterior (a chain of two IAF steps) of iaf_amd.CVAELayerIAF at BASELINE configs[1]
sizes, next to what it is made of: the one-flow posterior block, one flipmask IAF step, the chain's head and tail launches alone, and the
training pair (down_q + backward).  All rows of both resolutions come from ONE process; every row is warmed up, then timed between device
events over REPS calls, REPEATS times -- the median and the spread (min .. max) are printed.  --json PATH also writes the rows."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import iaf_amd  # noqa: E402
from iaf_amd import _capi  # noqa: E402
from iaf_amd.layers import _ptr, _stream  # noqa: E402

WARMUP, REPS, REPEATS = 20, 200, 7


def timed(fn):
    """us per call: (median, min, max) over REPEATS windows of REPS calls between two device events"""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / REPS * 1e3)
    return float(np.median(out)), min(out), max(out)


def params(rng, name, n_z, n_h_list):
    w = {}
    sizes = [n_z] + n_h_list
    for conv in ("_posterior_conv1", "_posterior_conv2"):
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chain_bench needs a GPU: a CPU run says nothing about these times")
    B, n_z, n_h, d, kl_min = 32, 32, 160, 2, 0.25
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    rows = []
    for H in (16, 8):
        rng = np.random.RandomState(0)
        w = {k: dev(v) for k, v in params(rng, "1", n_z, [n_h] * d).items()}
        h_up, h_dn = rng.standard_normal((B, 2 * n_h + 2 * n_z, H, H)), rng.standard_normal((B, 2 * n_h + 4 * n_z, H, H))
        h_up[:, n_h + n_z:n_h + 2 * n_z] *= 0.25
        h_dn[:, n_h + n_z:n_h + 2 * n_z] *= 0.25
        h_dn[:, n_h + 3 * n_z:n_h + 4 * n_z] *= 0.25
        h_up, h_dn = dev(h_up), dev(h_dn)
        eps = dev(rng.standard_normal((B, n_z, H, H)))
        d_h, d_up = dev(rng.standard_normal((B, n_h + n_z, H, H))), dev(rng.standard_normal((B, n_h, H, H)))
        HW = H * H
        res = {}

        one = iaf_amd.CVAELayerIAF("1", n_h, n_z, d, posterior="down_iaf2_nl", kl_min=kl_min)      # the existing one-flow posterior
        one.load(w)
        one.up(h_up)
        st = one._st
        pieces = iaf_amd.layers.split(h_dn, 1, [n_h, n_z, n_z, n_z, n_z, n_h])
        res["one-flow posterior block (ARStack.posterior_block)"] = timed(lambda: one.stack.posterior_block(
            st["qz_mean"], st["qz_logsd"], pieces[3], pieces[4], pieces[1], pieces[2], st["context"], pieces[5], eps, kl_min, want_kl_elem=True))
        res["one-flow down_q (6 split copies + block + cat)"] = timed(lambda: one.down_q(h_dn, eps=eps))

        chain = iaf_amd.CVAELayerIAF("1", n_h, n_z, d, posterior="down_iaf2_nl2", kl_min=kl_min)
        chain.load(w)
        chain.up(h_up)
        out = chain.down_q(h_dn, eps=eps)
        cst = chain._st
        res["one flipmask iaf_step"] = timed(lambda: chain.stack2.iaf_step(cst["z1"], cst["context_sum"]))
        res["one plain iaf_step"] = timed(lambda: chain.stack.iaf_step(cst["z0"], cst["context_sum"]))
        res["chain down_q (head + 2 steps + tail + free bits)"] = timed(lambda: chain.down_q(h_dn, eps=eps))
        z0, lq, ctx = torch.empty_like(eps), torch.empty_like(eps), torch.empty_like(cst["context_sum"])
        lib = _capi.lib()
        res["iaf_chain_head alone"] = timed(lambda: _capi.check(lib.iaf_chain_head(
            _ptr(h_up), _ptr(h_dn), _ptr(eps), _ptr(z0), _ptr(lq), _ptr(ctx), B, n_h, n_z, HW, _stream())))
        kl, h_out = torch.empty_like(eps), torch.empty_like(out["h"])
        res["iaf_chain_tail alone"] = timed(lambda: _capi.check(lib.iaf_chain_tail(
            _ptr(h_dn), _ptr(lq), _ptr(cst["s1"]), _ptr(cst["s2"]), _ptr(cst["z"]), _ptr(kl), _ptr(h_out), B, n_h, n_z, HW, _stream())))

        train = iaf_amd.CVAELayerIAF("1", n_h, n_z, d, posterior="down_iaf2_nl2", kl_min=kl_min)
        train.set_training(True)
        train.load(w)
        train.up(h_up)

        def pair():
            train.down_q(h_dn, eps=eps)
            train.backward(d_h, d_obj=1.0, d_up=d_up)

        res["chain training pair (down_q + backward)"] = timed(pair)
        one_t = iaf_amd.CVAELayerIAF("1", n_h, n_z, d, posterior="down_iaf2_nl", kl_min=kl_min)
        one_t.set_training(True)
        one_t.load(w)
        one_t.up(h_up)

        def pair_one():
            one_t.down_q(h_dn, eps=eps)
            one_t.backward(d_h, d_obj=1.0, d_up=d_up)

        res["one-flow training pair (down_q + backward)"] = timed(pair_one)
        print("B=%d n_z=%d n_h=%d depth_ar=%d %dx%d, kl_min=%g  (us per call: median [min .. max] of %d windows of %d calls)"
              % (B, n_z, n_h, d, H, H, kl_min, REPEATS, REPS))
        for k, (med, lo, hi) in res.items():
            print("  %-52s %8.1f  [%7.1f .. %7.1f]" % (k, med, lo, hi))
            rows.append(dict(H=H, W=H, row=k, median_us=med, min_us=lo, max_us=hi))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(dict(B=B, n_z=n_z, n_h=n_h, depth_ar=d, kl_min=kl_min, warmup=WARMUP, reps=REPS, repeats=REPEATS, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
