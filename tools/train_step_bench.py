#!/usr/bin/env python
"""GPU dev tool: what the guard of iaf_amd.TrainStep costs.  At the BASELINE geometry (B = 32, z 32, h 160, depths [10, 10], 32x32
images, seeded weights, launch shapes autotuned as bench.py --train --model does) it times, in alternation (median over rounds of
back-to-back replays between HIP events on the current stream):
  guarded     the hipGraph of TrainStep(model, lr) replayed: prep, forward, backward, reduce, join, guard scan, gated Adamax / EMA
  unguarded   the same step captured on the same stream with FlatParams.adamax_ema_step in place of scan + gated update
  call        ts(x, noise): the guarded replay plus the copies of x and noise into the graph's static inputs
  scan_us     iaf_nonfinite_scan of the flat gradient alone (50 back-to-back launches)
then forces one re-capture of the guarded step (the path a skip takes after an object moved to bf16 planes) and times it again: a
re-captured step that is slower than the first capture by more than 2 % is reported as probably running the recomputing one-launch
step instead of the halo exchange (the exchange sets of a stream stay marked as captured: include/iaf_hip.h).
--summaries adds, before the re-capture: a second model and TrainStep(summaries=True) on a stream of its own, its replay timed in
alternation with the guarded replay (summaries_ms against guarded_alt_ms), and iaf_nonfinite_scan_sumsq in alternation with
iaf_nonfinite_scan on the same gradient buffer (fused_scan_us against scan_alt_us), then reads the record once.  The second model
and its flat state (parameters, gradients, slots, EMA) live next to the first in the same process: about 1.3 GB more device memory at
the default geometry.  It replays the TrainStep's private graph (ts._graph) to time the step without the input copies.
--towers N (N > 1; --batch is then the rows PER TOWER, the reference's 16) measures instead what CVAE1(towers=N) is for, three unguarded
steps (prep, forward, backward, Adamax / EMA with 1/N) captured as hipGraphs on one stream and replayed in alternation:
  towers      (a) ONE pass over N * batch rows with the free-bits mean per tower (towers = N)
  passes      (b) N passes of `batch` rows each on a towers = 1 model, their gradients accumulated with iaf_axpby
  one_batch   (c) one pass over N * batch rows with towers = 1 (a different objective: what grouping costs)
(a) / (b) is the feature's value, (a) / (c) its price.  Three models live side by side.
Prints one JSON line."""
import argparse
import ctypes
import json
import math
import os
import sys
import time

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


def towers_main(args):
    import torch
    import golden_inputs as gi
    import iaf_amd
    from iaf_amd import _capi
    from iaf_amd import parallel as par
    N, B, zs, hs, nb = args.towers, args.batch, 32, 160, args.num_blocks
    rows = N * B
    gi.MODEL_CASES["train_step_bench"] = (rows, 1, zs, hs, 2, nb, 32, 0.25)
    c = gi.model_case_inputs("train_step_bench")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    rng = np.random.RandomState(99)
    x = torch.from_numpy(rng.randint(0, 256, size=(rows, 3, 32, 32)).astype(np.uint8)).cuda()
    noise = [dev(rng.standard_normal(e.shape)) for e in c["noise"]]
    xs = [x[t * B:(t + 1) * B].contiguous() for t in range(N)]
    ns = [[e[t * B:(t + 1) * B].contiguous() for e in noise] for t in range(N)]
    lr = 1e-4
    lib = _capi.lib()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def build(towers):
        m = iaf_amd.CVAE1(z_size=zs, h_size=hs, kl_min=0.25, depth=2, num_blocks=nb, k=1, image_size=32, towers=towers)
        m.set_training(True)
        m.load({k: dev(v) for k, v in c["params"].items()})
        f = par.FlatParams({k: m.params[k] for k in m.completion_order()})
        m.load(f.p)
        nbk = len(m.set_grad_buckets(1))
        return m, f, nbk

    def fb(m, f, nbk, xx, nn, tune=False):
        out = m.fb_begin(xx, nn, grads=f.g, autotune=tune)
        for i in range(nbk):
            m.fb_segment(i)
        return out

    ma_, fa, ka = build(N)
    mb_, fb_, kb = build(1)
    mc_, fc, kc = build(1)
    acc = torch.zeros_like(fb_.grads)

    def step_a():
        ma_.prepare_weights()
        fb(ma_, fa, ka, x, noise)
        fa.adamax_ema_step(lr, world=N)

    def step_b():
        mb_.prepare_weights()
        for t in range(N):
            fb(mb_, fb_, kb, xs[t], ns[t])
            dst = fb_.grads if t == N - 1 else acc                  # acc = g (+ acc); the last sum lands where the update reads it
            _capi.check(lib.iaf_axpby(P(fb_.grads), 1.0, P(acc), 0.0 if t == 0 else 1.0, P(dst), acc.numel(), st()))
        fb_.adamax_ema_step(lr, world=N)

    def step_c():
        mc_.prepare_weights()
        fb(mc_, fc, kc, x, noise)
        fc.adamax_ema_step(lr, world=1)

    for tune in (True, False):                          # launch-shape search of the plain convs at both batch sizes
        for m, f, k, xx, nn in ((ma_, fa, ka, x, noise), (mb_, fb_, kb, xs[0], ns[0]), (mc_, fc, kc, x, noise)):
            m.prepare_weights()
            fb(m, f, k, xx, nn, tune)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graphs = []
    with torch.cuda.stream(s):
        for fn in (step_a, step_b, step_c):
            fn()                                        # warm up on the capture stream (the exchange sets are per stream)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                fn()
            graphs.append(g)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for _ in range(3):
        for g in graphs:
            g.replay()
    ta, tb, tc = [], [], []
    for _ in range(args.rounds):
        ta.append(timed(graphs[0].replay, args.reps))
        tb.append(timed(graphs[1].replay, args.reps))
        tc.append(timed(graphs[2].replay, args.reps))
    a, b, cc = float(np.median(ta)), float(np.median(tb)), float(np.median(tc))
    # the accumulated gradient of (b) is the one-pass gradient of (a), fp32 round-off of the sums apart (same weights only before the
    # first update: compared on a fresh eager pass of each with the parameters of (a))
    fb_.params.copy_(fa.params)
    mb_.prepare_weights()
    ma_.prepare_weights()
    step_grad = fb(ma_, fa, ka, x, noise)
    ga = fa.grads.clone()
    for t in range(N):
        fb(mb_, fb_, kb, xs[t], ns[t])
        if t == 0:
            acc.copy_(fb_.grads)
        else:
            acc.add_(fb_.grads)
    torch.cuda.synchronize()
    rel = float((ga - acc).abs().max() / ga.abs().max())
    print(json.dumps({
        "tool": "train_step_bench --towers", "towers": N, "rows_per_tower": B, "rows": rows, "z": zs, "h": hs, "depths": [nb, nb],
        "towers_ms": a, "passes_ms": b, "one_batch_ms": cc, "towers_over_passes": a / b, "towers_over_one_batch": a / cc,
        "towers_repeats_ms": ta, "passes_repeats_ms": tb, "one_batch_repeats_ms": tc,
        "towers_spread": (max(ta) - min(ta)) / a, "passes_spread": (max(tb) - min(tb)) / b, "one_batch_spread": (max(tc) - min(tc)) / cc,
        "grad_towers_vs_accumulated_rel": rel, "obj_towers": float(step_grad["obj"].item()),
        "timing": "median of %d rounds of %d back-to-back graph replays between HIP events, the three steps in alternation" % (args.rounds, args.reps)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--num-blocks", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--summaries", action="store_true", help="also time the step and the scan with training summaries")
    ap.add_argument("--towers", type=int, default=1, help="N > 1: time towers = N against N passes and against one batch (see above)")
    args = ap.parse_args()
    if args.towers > 1:
        return towers_main(args)
    import torch
    import golden_inputs as gi
    import iaf_amd
    from iaf_amd import _capi
    B, zs, hs, nb = args.batch, 32, 160, args.num_blocks
    gi.MODEL_CASES["train_step_bench"] = (B, 1, zs, hs, 2, nb, 32, 0.25)
    c = gi.model_case_inputs("train_step_bench")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    model = iaf_amd.CVAE1(z_size=zs, h_size=hs, kl_min=0.25, depth=2, num_blocks=nb, k=1, image_size=32)
    model.set_training(True)
    model.load({k: dev(v) for k, v in c["params"].items()})
    rng = np.random.RandomState(99)
    x = torch.from_numpy(rng.randint(0, 256, size=(B, 3, 32, 32)).astype(np.uint8)).cuda()
    noise = [dev(rng.standard_normal(e.shape)) for e in c["noise"]]
    lr = 1e-4
    ts = iaf_amd.TrainStep(model, lr, graph=True)
    flat, red = ts.flat, ts.red
    for tune in (True, False):                          # launch-shape search of the plain convs (bench.py --train --model does the same)
        model.prepare_weights()
        model.fb_begin(x, noise, grads=flat.g, autotune=tune)
        for i in range(ts.n_buckets):
            model.fb_segment(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ts(x, noise)
    torch.cuda.synchronize()
    first_call_s = time.perf_counter() - t0
    if not ts.graphed:
        raise SystemExit("train_step_bench: the step was not captured (%s)" % ts.graph_refused)

    def plain_step():
        model.prepare_weights()
        model.fb_begin(x, noise, grads=flat.g)
        for i in range(ts.n_buckets):
            model.fb_segment(i)
            red.reduce(i)
        red.wait()
        flat.adamax_ema_step(lr, world=ts.world)

    s = ts._stream                                      # the guarded step's capture stream: the two graphs share its exchange sets
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plain_step()
        torch.cuda.synchronize()
        g_plain = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_plain, stream=s, capture_error_mode="thread_local"):
            plain_step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    call = lambda: ts(x, noise)                          # the public call: also copies x and noise into the graph's static inputs
    guarded = lambda: ts._graph.replay()                 # the guarded step alone, like for like with the unguarded replay
    for _ in range(3):
        call()
        g_plain.replay()
    tg, tp, tc = [], [], []
    for _ in range(args.rounds):
        tg.append(timed(guarded, args.reps))
        tp.append(timed(g_plain.replay, args.reps))
        tc.append(timed(call, args.reps))
    mg, mp, mc = float(np.median(tg)), float(np.median(tp)), float(np.median(tc))
    lib = _capi.lib()
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    scan = lambda: _capi.check(lib.iaf_nonfinite_scan(P(flat.grads), flat.grads.numel(), P(ts._status), 1, P(guard), st()))
    scan()
    scan_us = 1e3 * float(np.median([timed(scan, 50) for _ in range(5)]))
    extra = {}
    if args.summaries:
        model2 = iaf_amd.CVAE1(z_size=zs, h_size=hs, kl_min=0.25, depth=2, num_blocks=nb, k=1, image_size=32)
        model2.set_training(True)
        model2.load({k: dev(v) for k, v in c["params"].items()})
        ts2 = iaf_amd.TrainStep(model2, lr, graph=True, summaries=True)
        for tune in (True, False):
            model2.prepare_weights()
            model2.fb_begin(x, noise, grads=ts2.flat.g, autotune=tune)
            for i in range(ts2.n_buckets):
                model2.fb_segment(i)
        torch.cuda.synchronize()
        ts2(x, noise)
        torch.cuda.synchronize()
        if not ts2.graphed:
            raise SystemExit("train_step_bench: the step with summaries was not captured (%s)" % ts2.graph_refused)
        with_s = lambda: ts2._graph.replay()
        for _ in range(3):
            guarded()
            with_s()
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(guarded, args.reps))
            tb.append(timed(with_s, args.reps))
        ma, mb = float(np.median(ta)), float(np.median(tb))
        partials = torch.zeros(2048, dtype=torch.float64, device="cuda")
        sumsq = torch.zeros(1, dtype=torch.float64, device="cuda")
        fused = lambda: _capi.check(lib.iaf_nonfinite_scan_sumsq(P(flat.grads), flat.grads.numel(), P(ts._status), 1, P(guard), P(partials),
                                                                 P(sumsq), st()))
        fused()
        sa, sb = [], []
        for _ in range(5):
            sa.append(1e3 * timed(scan, 50))
            sb.append(1e3 * timed(fused, 50))
        msa, msb = float(np.median(sa)), float(np.median(sb))
        norm = float(torch.sqrt((flat.grads.double() ** 2).sum()).item())
        rec = ts2.summaries(reset=False)
        extra = {"summaries_ms": mb, "guarded_alt_ms": ma, "summaries_overhead_ms": mb - ma, "summaries_overhead_frac": (mb - ma) / ma,
                 "summaries_repeats_ms": tb, "guarded_alt_repeats_ms": ta, "fused_scan_us": msb, "scan_alt_us": msa,
                 "fused_over_plain_scan": msb / msa, "fused_scan_repeats_us": sb, "scan_alt_repeats_us": sa,
                 "fused_scan_gbs": 4 * flat.grads.numel() / (msb * 1e-6) / 1e9,
                 "fused_scan_norm_rel_err": abs(math.sqrt(float(sumsq.item())) - norm) / norm,
                 "summaries_captures": ts2.captures, "summaries_record": {k: rec[k] for k in ("model/bits_per_dim", "model/dec_log_stdv", "model/log_pxz",
                                                                                                "model/kl_obj", "model/kl_cost", "grad_norm", "steps", "skipped")}}
        del ts2, model2
    # one re-capture of the guarded step, as after a skip that moved an object to bf16 planes
    t0 = time.perf_counter()
    ts._capture()
    torch.cuda.synchronize()
    recapture_s = time.perf_counter() - t0
    for _ in range(3):
        call()
    guarded = lambda: ts._graph.replay()
    tr = [timed(guarded, args.reps) for _ in range(args.rounds)]
    mr = float(np.median(tr))
    skipped = ts.skipped
    obj = float(ts._sobj.item())
    print(json.dumps({
        **extra, "tool": "train_step_bench", "B": B, "z": zs, "h": hs, "depths": [nb, nb], "params": int(flat.params.numel()),
        "flat_mb": 4e-6 * flat.params.numel(),
        "guarded_ms": mg, "unguarded_ms": mp, "guard_overhead_ms": mg - mp, "guard_overhead_frac": (mg - mp) / mp,
        "scan_us": scan_us, "scan_gbs": 4 * flat.grads.numel() / (scan_us * 1e-6) / 1e9,
        "call_ms": mc, "call_repeats_ms": tc, "guarded_repeats_ms": tg, "unguarded_repeats_ms": tp,
        "first_call_s": first_call_s, "recapture_s": recapture_s, "recaptured_ms": mr, "recaptured_repeats_ms": tr,
        "recaptured_over_first": mr / mg, "recaptured_probably_recomputes_halo_rows": bool(mr > 1.02 * mg),
        "captures": ts.captures, "skipped": skipped, "obj_last": obj,
        "timing": "median of %d rounds of %d back-to-back steps between HIP events, guarded and unguarded in alternation" % (args.rounds, args.reps)}))


if __name__ == "__main__":
    main()
