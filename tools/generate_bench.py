#!/usr/bin/env python
"""GPU dev tool: CVAE1.generate (images from the prior: the tiled h_top, every layer's generate_down, x_dec) against forward() in mode
"sample" on the same weights and prior noise, at the bench workload's geometry (z 32, h 160, 32x32 images, depth 2 x num_blocks 10,
seeded init-scale weights, B = 32).  The two are timed in alternation in one process (median over rounds of back-to-back calls, events on
torch's current stream); prints one JSON line: ms of each, their ratio, images/s of generate, max |difference| of the two outputs.

  --convs              instead: 20 calls each of down_conv1 in full (iaf_conv3x3_forward) and in prior form
                       (iaf_conv3x3_forward_prior_sample) at 16x16 and 8x8, B = 32 -- the workload of a kernel-trace run:
                       rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/generate_bench.py --convs
  --summarize FILE     per (kernel, grid) of a rocprofv3 run (its rocpd run_results.db, or a kernel_trace.csv): calls and median duration (us) of the split-product conv
                       kernels, EPI 3 = the full conv, EPI 7 = the prior form"""
import argparse
import csv
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def timed(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def model_bench(args):
    import torch
    import golden_inputs as gi
    import iaf_amd
    B, zs, hs = args.batch, 32, 160
    gi.MODEL_CASES["generate_bench"] = (B, 1, zs, hs, 2, args.num_blocks, 32, 0.25)
    c = gi.model_case_inputs("generate_bench")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    model = iaf_amd.CVAE1(z_size=zs, h_size=hs, kl_min=0.25, depth=2, num_blocks=args.num_blocks, k=1, image_size=32, mode="sample")
    model.load({k: dev(v) for k, v in c["params"].items()})
    noise = [dev(e) for e in c["noise"]]
    x = torch.from_numpy(c["x"]).cuda()
    eps_prior = noise[0::2]
    gen = lambda: model.generate(eps_prior)
    fwd = lambda: model.forward(x, noise)
    out_g, out_f = gen(), fwd()[0]
    torch.cuda.synchronize()
    diff = float((out_g - out_f).abs().max().item())
    tg, tf = [], []
    for _ in range(args.rounds):                       # alternating: drift of clocks / neighbours hits both alike
        tg.append(timed(gen, args.reps))
        tf.append(timed(fwd, args.reps))
    mg, mf = float(np.median(tg)), float(np.median(tf))
    print(json.dumps({"tool": "generate_bench", "B": B, "z": zs, "h": hs, "depth": 2, "num_blocks": args.num_blocks,
                      "generate_ms": round(mg, 4), "forward_sample_ms": round(mf, 4), "ratio": round(mg / mf, 4),
                      "generate_images_per_s": round(B / (mg * 1e-3), 1), "max_abs_diff": diff,
                      "rounds": args.rounds, "reps": args.reps}), flush=True)


def conv_workload(args):
    import torch
    import golden_inputs as gi
    import iaf_amd
    B, zs, hs = args.batch, 32, 160
    rng = np.random.RandomState(7)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    for H in (16, 8):
        p = gi.conv_params(rng, hs, 4 * zs + 2 * hs)
        conv = iaf_amd.WNConv2d(hs, 4 * zs + 2 * hs)
        conv.prepare(dev(p["V"]), dev(p["g"]), dev(p["b"]))
        x, eps = dev(rng.standard_normal((B, hs, H, H))), dev(rng.standard_normal((B, zs, H, H)))
        for _ in range(20):
            conv(x, elu_input=True, split=[zs] * 4 + [hs] * 2)
        for _ in range(20):
            conv.prior_sample(x, eps, zs, elu_input=True)
        torch.cuda.synchronize()
        print("%dx%d B=%d: down_conv1 f16x2 %s" % (H, H, B, conv.runs_f16x2(B, H, H)), flush=True)


def summarize(path):
    """path: the rocpd database rocprofv3 writes (run_results.db: the `kernels` view) or a kernel_trace.csv"""
    rows = {}

    def add(name, grid, ns):
        m = re.search(r"iaf_conv_bf3_kernel<([^>]*)>", name)
        if m:
            targs = [t.strip() for t in m.group(1).split(",")]
            rows.setdefault((targs[5] if len(targs) > 5 else "?", m.group(1), grid), []).append(ns / 1e3)
    if path.endswith(".db"):
        import sqlite3
        for name, gx, gy, gz, ns in sqlite3.connect(path).execute("select name, grid_x, grid_y, grid_z, duration from kernels"):
            add(name, "%dx%dx%d" % (gx, gy, gz), ns)
    else:
        with open(path) as f:
            for r in csv.DictReader(f):
                add(r.get("Kernel_Name", ""), r.get("Grid_Size", "?"), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for (epi, targs, grid), us in sorted(rows.items()):
        print("EPI %s  <%s>  grid %s: %d calls, median %.2f us" % (epi, targs, grid, len(us), float(np.median(us))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--num-blocks", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--convs", action="store_true")
    ap.add_argument("--summarize", default=None)
    args = ap.parse_args()
    if args.summarize is not None:
        summarize(args.summarize)
    elif args.convs:
        conv_workload(args)
    else:
        model_bench(args)


if __name__ == "__main__":
    main()
