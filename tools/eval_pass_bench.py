#!/usr/bin/env python
"""GPU dev tool: what a batch of the test-set evaluation costs.  At the BASELINE geometry (z 32, h 160, depth 2, --num-blocks 10,
32x32 images, seeded weights, default launch shapes), --batch 100, k = 1 and a dataset of --images random uint8 images it times, in
alternation (wall clock around a whole epoch, the device idle before and after; the median over --rounds epochs, divided by the
batches of an epoch):
  eval_pass_ms   EvalPass(graph=True).run(): 1 + k graph replays per batch, one host read at the end of the epoch
  eager_loop_ms  the loop the library could express before EvalPass: DeviceDataset.next_batch + CVAE1.draw_noise + CVAE1.forward as
                 eager launches, and one host read of the loss per batch
and reports both epochs' bits per dim (the same images, weights and noise steps: they agree to fp32 summation order).
Prints one JSON line."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--num-blocks", type=int, default=10)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    import golden_inputs as gi
    import iaf_amd
    B, zs, hs, nb, n, k, seed = args.batch, 32, 160, args.num_blocks, args.images, args.k, 1234
    gi.MODEL_CASES["eval_pass_bench"] = (2, 1, zs, hs, 2, nb, 32, 0.25)
    c = gi.model_case_inputs("eval_pass_bench")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    images = torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, device="cuda", generator=g)
    model = iaf_amd.CVAE1(z_size=zs, h_size=hs, kl_min=0.25, depth=2, num_blocks=nb, k=1, image_size=32)
    model.load({k_: dev(v) for k_, v in c["params"].items()})
    batches = n // B
    per_dim = math.log(2.0) * 3 * 32 * 32 * n

    src = iaf_amd.NoiseSource(seed)
    ev = iaf_amd.EvalPass(model, iaf_amd.DeviceDataset(images, seed, deterministic=True), B, src, k=k)

    def captured():
        src.seek(0)
        return ev.run()["eval_bits_per_dim"]

    ds, src2 = iaf_amd.DeviceDataset(images, seed, deterministic=True), iaf_amd.NoiseSource(seed)
    x, noise = ds.next_batch(B, advance=False), model.draw_noise(B, src2, which="posterior", advance=False)

    def eager():
        model.prepare_weights()
        ds.seek(0)
        src2.seek(0)
        total = 0.0
        for _ in range(batches):
            ds.next_batch(B, out=x)
            if k == 1:
                model.draw_noise(B, src2, which="posterior", out=noise)
                total += float(model.forward(x, noise)[2])            # the host reads every batch's loss
            else:
                total += float(model.iw_eval(x, k=k, noise_source=src2))
        return total / per_dim

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / batches, v

    for _ in range(2):
        wall(captured)
        wall(eager)
    if not ev.graphed:
        raise SystemExit("eval_pass_bench: the evaluation was not captured (%s)" % ev.graph_refused)
    tc, te = [], []
    for _ in range(args.rounds):
        t, bc = wall(captured)
        tc.append(t)
        t, be = wall(eager)
        te.append(t)
    mc, me = float(np.median(tc)), float(np.median(te))
    print(json.dumps({
        "tool": "eval_pass_bench", "B": B, "z": zs, "h": hs, "depths": [nb, nb], "images": n, "k": k, "batches": batches,
        "eval_pass_ms_per_batch": mc, "eager_loop_ms_per_batch": me, "eager_over_eval_pass": me / mc,
        "eval_pass_repeats_ms": tc, "eager_loop_repeats_ms": te, "eval_pass_spread": (max(tc) - min(tc)) / mc,
        "eager_loop_spread": (max(te) - min(te)) / me, "eval_bits_per_dim": bc, "eager_bits_per_dim": be, "captures": ev.captures,
        "timing": "wall clock around one epoch of %d batches, device idle before and after, median of %d epochs, the two loops in "
                  "alternation" % (batches, args.rounds)}))


if __name__ == "__main__":
    main()
