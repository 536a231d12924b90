#!/usr/bin/env python
"""GPU dev tool: what run_eval's pictures cost.  At B = 100, S = 32 (z 32, h 160, depth 2, --num-blocks blocks per level, seeded weights,
a device dataset of --batches * B random images, default launch shapes) it measures, in one process and after warm-up:
  range_*_us      device time per iaf_img_range launch (events around --launches launches back to back on one stream, so the figure
                  is the launch-to-launch period of a busy stream, not a kernel's duration alone): the whole batch of samples
                  (fp32 [100,3,32,32]), the 36 shown, 18 reconstructions (fp32) and 18 inputs (uint8)
  grid_*_us       the same for iaf_img_grid: the samples' grid (one source, outer + inner record) and the reconstructions' (two sources),
                  both outputs written, [192,192,3]
  images_ms       wall clock of one EvalPass.images(total=36) (it ends in its one synchronisation), median over --reps
  eval_batch_ms   wall clock of EvalPass.run(batches=1) (one captured head + pass and the record's copy), in alternation with it
Prints one JSON line."""
import argparse
import json
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
    ap.add_argument("--num-blocks", type=int, default=2)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch
    import golden_inputs as gi
    import iaf_amd
    from iaf_amd import _capi
    if not torch.cuda.is_available():
        raise SystemExit("image_grid_bench: needs a GPU")
    B, zs, hs, nb, S, total = args.batch, 32, 160, args.num_blocks, 32, 36
    gi.MODEL_CASES["image_grid_bench"] = (2, 1, zs, hs, 2, nb, S, 0.25)
    c = gi.model_case_inputs("image_grid_bench")
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    images = torch.randint(0, 256, (args.batches * B, 3, S, S), dtype=torch.uint8, device="cuda", generator=g)
    model = iaf_amd.CVAE1(z_size=zs, h_size=hs, kl_min=0.25, depth=2, num_blocks=nb, k=1, image_size=S)
    model.load({k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda() for k, v in c["params"].items()})
    src = iaf_amd.NoiseSource(1234)
    ev = iaf_amd.EvalPass(model, iaf_amd.DeviceDataset(images, 0, deterministic=True), B, src, k=1)
    for _ in range(3):
        ev.run(batches=1)
        r = ev.images(total=total)
    if not ev.graphed:
        raise SystemExit("image_grid_bench: the evaluation was not captured (%s)" % ev.graph_refused)

    lib, per = _capi.lib(), 3 * S * S
    x_gen, x_mean, inputs = r["x_gen"], r["x_mean"].contiguous(), r["inputs"].contiguous()
    recs = torch.zeros((4, 4), dtype=torch.int32, device="cuda")
    g8 = torch.empty((6 * S, 6 * S, 3), dtype=torch.uint8, device="cuda")
    gf = torch.empty((6 * S, 6 * S, 3), dtype=torch.float32, device="cuda")

    def rng_call(t, rows, rec):
        dt = _capi.IAF_IMG_U8 if t.dtype == torch.uint8 else _capi.IAF_IMG_F32
        return lambda: _capi.check(lib.iaf_img_range(_capi.ptr(t), dt, rows * per, _capi.ptr(rec), _capi.stream()))

    def grid_call(entries):
        table = (_capi.ImgSource * len(entries))()
        for s, (t, outer, inner) in enumerate(entries):
            table[s].ptr, table[s].dtype = t.data_ptr(), _capi.IAF_IMG_U8 if t.dtype == torch.uint8 else _capi.IAF_IMG_F32
            table[s].outer, table[s].inner = outer.data_ptr(), None if inner is None else inner.data_ptr()
        return lambda: _capi.check(lib.iaf_img_grid(table, len(entries), total, 3, S, S, 0, 0.0, _capi.ptr(gf), _capi.ptr(g8), _capi.stream()))
    calls = {
        "range_batch_f32_307200": rng_call(x_gen, B, recs[0]),
        "range_shown_f32_110592": rng_call(x_gen, total, recs[1]),
        "range_recs_f32_55296": rng_call(x_mean, total // 2, recs[2]),
        "range_inputs_u8_55296": rng_call(inputs, total // 2, recs[3]),
    }
    for fn in calls.values():
        fn()
    calls["grid_samples"] = grid_call([(x_gen, recs[0], recs[1])])
    calls["grid_reconstructions"] = grid_call([(inputs, recs[3], None), (x_mean, recs[2], None)])

    def period_us(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.launches):
            fn()
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / args.launches
    out = {}
    for name, fn in calls.items():
        period_us(fn)
    for name, fn in calls.items():
        runs = [period_us(fn) for _ in range(5)]
        out[name + "_us"] = float(np.median(runs))
        out[name + "_us_min_max"] = [min(runs), max(runs)]

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    t_img, t_eval = [], []
    for _ in range(args.reps):
        t_img.append(wall_ms(lambda: ev.images(total=total)))
        t_eval.append(wall_ms(lambda: ev.run(batches=1)))
    out.update({"tool": "image_grid_bench", "B": B, "S": S, "z": zs, "h": hs, "depths": [nb, nb], "total": total,
                "images_ms": float(np.median(t_img)), "images_ms_min_max": [min(t_img), max(t_img)],
                "eval_batch_ms": float(np.median(t_eval)), "eval_batch_ms_min_max": [min(t_eval), max(t_eval)],
                "launches": args.launches, "reps": args.reps,
                "timing": "kernels: device events around %d launches back to back, median of 5 windows (the period of a busy stream); "
                          "images / eval batch: wall clock around a call that ends in a synchronise, device idle before, median of %d, in "
                          "alternation" % (args.launches, args.reps)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
