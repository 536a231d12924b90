#!/usr/bin/env python
"""GPU dev tool: what a checkpoint costs.  At the BASELINE config-2 geometry (z 32, h 160, depth 2, --num-blocks 10, 32x32 images, batch
32, seeded weights, default launch shapes; a captured TrainStep with a noise source and a device dataset) it measures, in one process
and after warm-up, in alternation:
  snapshot_ms / copies_ms   device time (events, behind an enqueued training step so that no host time is inside) of one ts.snapshot()
                            against the summed device time of four Tensor.copy_ of the same four flat buffers into the same staging
                            buffers (what exists without the feature: no digest, no counters); median over --reps repetitions each
  snapshot_tbps             bytes read + written by the snapshot per second, and its share of the 6.29 TB/s float4-copy figure
  step_ms / step_snap_ms    wall clock per ts() over --steps steps without a snapshot, and with one every 100
  save / load               wall clock of snap.save and load_checkpoint, with and without verify (a file under --dir)
Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

COPY_TBPS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--num-blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    import torch
    import golden_inputs as gi
    import iaf_amd
    B, zs, hs, nb, seed = args.batch, 32, 160, args.num_blocks, 1234
    gi.MODEL_CASES["checkpoint_bench"] = (2, 1, zs, hs, 2, nb, 32, 0.25)
    c = gi.model_case_inputs("checkpoint_bench")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    images = torch.randint(0, 256, (16 * B, 3, 32, 32), dtype=torch.uint8, device="cuda", generator=g)
    model = iaf_amd.CVAE1(z_size=zs, h_size=hs, kl_min=0.25, depth=2, num_blocks=nb, k=1, image_size=32)
    model.set_training(True)
    model.load({k: dev(v) for k, v in c["params"].items()})
    ts = iaf_amd.TrainStep(model, 2e-3, noise_source=iaf_amd.NoiseSource(seed), data=iaf_amd.DeviceDataset(images, seed), batch_size=B)
    for _ in range(5):
        ts()
    torch.cuda.synchronize()
    if not ts.graphed:
        raise SystemExit("checkpoint_bench: the step was not captured (%s)" % ts.graph_refused)
    flat = ts.flat
    srcs = (flat.params, flat.slot_m, flat.slot_v, flat.ema)
    words = flat.params.numel()
    snap = ts.snapshot()
    torch.cuda.synchronize()

    def timed(fn):
        """device time of fn's launches: a training step is enqueued in front, so that the host is a step ahead of the device and the
        interval between the two events holds device work only (with an idle device it would hold the host's time to launch as well)"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def copies():
        for d, s in zip(snap.bufs, srcs):
            d.copy_(s)
    for _ in range(5):
        timed(lambda: ts.snapshot(into=snap))
        timed(copies)
    t_snap, t_copy = [], []
    for _ in range(args.reps):
        t_snap.append(timed(lambda: ts.snapshot(into=snap)))
        t_copy.append(timed(copies))
    m_snap, m_copy = float(np.median(t_snap)), float(np.median(t_copy))
    moved = 2.0 * 4 * 4 * words                      # four buffers read and written
    tbps = moved / (m_snap * 1e-3) / 1e12

    def steps(every):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(args.steps):
            ts()
            if every and (t + 1) % every == 0:
                ts.snapshot(into=snap)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps
    steps(0)
    plain, with_snap = [], []
    for _ in range(3):
        plain.append(steps(0))
        with_snap.append(steps(100))
    skipped = ts.skipped

    def wall(fn):
        t0 = time.perf_counter()
        v = fn()
        return time.perf_counter() - t0, v
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        path = os.path.join(d, "bench.ckpt")
        ts.snapshot(into=snap)
        torch.cuda.synchronize()
        wall(lambda: snap.save(path, verify=False))
        save_plain = min(wall(lambda: snap.save(path, verify=False))[0] for _ in range(2))
        save_verify = min(wall(lambda: snap.save(path, verify=True))[0] for _ in range(2))
        size = os.path.getsize(path)
        load_plain = min(wall(lambda: iaf_amd.load_checkpoint(path, verify=False))[0] for _ in range(2))
        load_verify = min(wall(lambda: iaf_amd.load_checkpoint(path, verify=True))[0] for _ in range(2))
        restore_s = wall(lambda: ts.restore(path))[0]
    print(json.dumps({
        "tool": "checkpoint_bench", "B": B, "z": zs, "h": hs, "depths": [nb, nb], "words_per_buffer": words, "file_bytes": size,
        "snapshot_ms": m_snap, "four_copies_ms": m_copy, "snapshot_over_copies": m_snap / m_copy,
        "snapshot_min_max_ms": [min(t_snap), max(t_snap)], "copies_min_max_ms": [min(t_copy), max(t_copy)], "reps": args.reps,
        "snapshot_tbps": tbps, "share_of_float4_copy": tbps / COPY_TBPS,
        "step_ms": float(np.median(plain)), "step_with_snapshot_every_100_ms": float(np.median(with_snap)), "steps": args.steps,
        "step_ms_runs": plain, "step_with_snapshot_runs": with_snap, "skipped": skipped,
        "save_s": save_plain, "save_verify_s": save_verify, "load_s": load_plain, "load_verify_s": load_verify, "restore_s": restore_s,
        "timing": "device events around one call enqueued behind a training step, median of %d, snapshot and copies in alternation; steps: wall clock over %d calls, "
                  "device idle before and after, median of 3 runs in alternation; save / load: wall clock, best of 2" % (args.reps, args.steps)}))


if __name__ == "__main__":
    main()
