#!/usr/bin/env python
"""GPU dev tool: one NoiseSource.fill of the BASELINE model's posterior noise list (z 32, 32x32 images, depth 2 x num_blocks 10:
ten [B,32,8,8] and ten [B,32,16,16] tensors, B = 32) against the per-tensor torch normal_() calls on the same buffers that callers
of forward() / TrainStep make today.  The two are timed in alternation in one process: per round `reps` back-to-back calls between
two events on torch's current stream, after a warm-up of both; medians over the rounds.  Spread = the 10th-to-90th percentile width
of the torch path's rounds.  Also the rate of the fill (bytes written / time) on the list and on one 256 MiB tensor, next to the
6.29 TB/s copy rate measured on MI355X.  Prints one JSON line; exit status 1 if the single launch is slower than the torch path by
more than one spread."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

COPY_TBPS = 6.29


def timed(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--num-blocks", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    import iaf_amd
    model = iaf_amd.CVAE1(z_size=32, h_size=160, depth=2, num_blocks=args.num_blocks, k=1, image_size=32)
    src = iaf_amd.NoiseSource(1)
    bufs = [t for t in model.draw_noise(args.batch, src, which="posterior") if t is not None]
    nbytes = 4 * sum(t.numel() for t in bufs)
    fill = lambda: src.fill(bufs)
    def per_tensor():
        for t in bufs:
            t.normal_()
    for _ in range(3):                               # warm-up of both
        timed(fill, args.reps)
        timed(per_tensor, args.reps)
    tf, tt = [], []
    for _ in range(args.rounds):                     # alternating: drift of clocks / neighbours hits both alike
        tf.append(timed(fill, args.reps))
        tt.append(timed(per_tensor, args.reps))
    mf, mt = float(np.median(tf)), float(np.median(tt))
    spread = float(np.percentile(tt, 90) - np.percentile(tt, 10))
    big = torch.empty(1 << 26, dtype=torch.float32, device="cuda")
    big_fill = lambda: src.fill([big], advance=False)
    timed(big_fill, 5)
    tb = float(np.median([timed(big_fill, 5) for _ in range(9)]))
    ok = mf <= mt + spread
    print(json.dumps({"tool": "noise_bench", "B": args.batch, "tensors": len(bufs), "bytes": nbytes, "rounds": args.rounds, "reps": args.reps,
                      "fill_us": round(mf, 2), "fill_us_min_max": [round(min(tf), 2), round(max(tf), 2)],
                      "torch_normal_us": round(mt, 2), "torch_normal_us_min_max": [round(min(tt), 2), round(max(tt), 2)],
                      "torch_spread_us": round(spread, 2), "speedup": round(mt / mf, 2),
                      "fill_TBps": round(nbytes / mf * 1e-6, 3), "big_fill_bytes": 4 * big.numel(), "big_fill_us": round(tb, 1),
                      "big_fill_TBps": round(4 * big.numel() / tb * 1e-6, 3), "copy_TBps": COPY_TBPS,
                      "single_launch_not_slower": ok}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
