#!/usr/bin/env python
"""GPU dev tool: what the device-resident dataset costs inside the training step.  At the BASELINE geometry (B = 32, z 32, h 160, depths
[10, 10], 32x32 images, seeded weights, launch shapes autotuned as bench.py --train --model does) and a dataset of --images random
uint8 images it times, in alternation (median over rounds of back-to-back calls between HIP events on the current stream):
  data_ms     ts() of TrainStep(noise_source=, data=, batch_size=B): the replay alone, the gather is the graph's first launch
  fed_ms      ts(x) of TrainStep(noise_source=) fed a batch that already lies in a device tensor: a 98 KB device copy into the graph's
              static input, then the replay (the step without a dataset)
  gather_us   DeviceDataset.next_batch alone, advance=False (one launch) and advance=True (the gather and the one-thread counter launch),
              200 back-to-back calls -- enqueue-bound at this size
and reports how far the parameters of the two steps are apart after the same calls from the same weights, seeds and steps, the fed step
getting images[reference indices] (--no-autotune: the two models then run the same launch shapes and the difference must be 0; with the
timing-based shape search each model picks its own, and the difference is that of two summation orders).  tests/test_hip_data.py holds
the exact statement.  Two models live side by side.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--num-blocks", type=int, default=10)
    ap.add_argument("--images", type=int, default=50000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-autotune", action="store_true", help="default launch shapes for both models")
    args = ap.parse_args()
    import torch
    import data_reference as D
    import golden_inputs as gi
    import iaf_amd
    B, zs, hs, nb, n, seed = args.batch, 32, 160, args.num_blocks, args.images, 1234
    gi.MODEL_CASES["data_step_bench"] = (B, 1, zs, hs, 2, nb, 32, 0.25)
    c = gi.model_case_inputs("data_step_bench")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    images = torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, device="cuda", generator=g)
    lr = 1e-4

    def build(**kw):
        m = iaf_amd.CVAE1(z_size=zs, h_size=hs, kl_min=0.25, depth=2, num_blocks=nb, k=1, image_size=32)
        m.set_training(True)
        m.load({k: dev(v) for k, v in c["params"].items()})
        ts = iaf_amd.TrainStep(m, lr, graph=True, noise_source=iaf_amd.NoiseSource(seed), **kw)
        x0 = images[:B].contiguous()
        noise = m.draw_noise(B, iaf_amd.NoiseSource(seed + 1), which="posterior")
        for tune in (() if args.no_autotune else (True, False)):        # launch-shape search of the plain convs (bench.py --train --model does the same)
            m.prepare_weights()
            m.fb_begin(x0, noise, grads=ts.flat.g, autotune=tune)
            for i in range(ts.n_buckets):
                m.fb_segment(i)
        torch.cuda.synchronize()
        return ts

    ds = iaf_amd.DeviceDataset(images, seed)
    ts_data = build(data=ds, batch_size=B)
    ts_fed = build()
    # the same training from both: the fed step gets the batches of the reference indices
    calls = 3
    for t in range(calls):
        ts_data()
        ts_fed(images[torch.from_numpy(D.batch_indices(n, seed, t, B)).cuda()])
    torch.cuda.synchronize()
    apart = max(float((getattr(ts_data.flat, k) - getattr(ts_fed.flat, k)).abs().max()) for k in ("params", "slot_m", "slot_v", "ema"))
    if not (ts_data.graphed and ts_fed.graphed):
        raise SystemExit("data_step_bench: a step was not captured (%s / %s)" % (ts_data.graph_refused, ts_fed.graph_refused))
    x = images[B:2 * B].contiguous()
    data_call = lambda: ts_data()
    fed_call = lambda: ts_fed(x)
    for _ in range(3):
        data_call()
        fed_call()
    td, tf = [], []
    for _ in range(args.rounds):
        td.append(timed(data_call, args.reps))
        tf.append(timed(fed_call, args.reps))
    md, mf = float(np.median(td)), float(np.median(tf))
    out = torch.empty(B, 3, 32, 32, dtype=torch.uint8, device="cuda")
    probe = iaf_amd.DeviceDataset(images, seed)
    g0 = lambda: probe.next_batch(B, out=out, advance=False)
    g1 = lambda: probe.next_batch(B, out=out)
    g0()
    g1()
    u0 = [1e3 * timed(g0, 200) for _ in range(5)]
    u1 = [1e3 * timed(g1, 200) for _ in range(5)]
    print(json.dumps({
        "tool": "data_step_bench", "B": B, "z": zs, "h": hs, "depths": [nb, nb], "images": n, "batch_bytes": B * 3072,
        "data_ms": md, "fed_ms": mf, "data_over_fed": md / mf, "data_repeats_ms": td, "fed_repeats_ms": tf,
        "data_spread": (max(td) - min(td)) / md, "fed_spread": (max(tf) - min(tf)) / mf,
        "gather_us": float(np.median(u0)), "gather_and_advance_us": float(np.median(u1)), "gather_repeats_us": u0,
        "gather_and_advance_repeats_us": u1, "max_abs_difference_after_%d_calls" % calls: apart, "autotuned": not args.no_autotune,
        "captures": [ts_data.captures, ts_fed.captures], "skipped": [ts_data.skipped, ts_fed.skipped], "dataset_step": ds.tell(),
        "timing": "median of %d rounds of %d back-to-back calls between HIP events, the two steps in alternation" % (args.rounds, args.reps)}))


if __name__ == "__main__":
    main()
