#!/usr/bin/env python
"""GPU dev tool: the latent entry points of CVAE1 at the bench workload's geometry (z 32, h 160, 32x32 images, depth 2 x num_blocks 10,
seeded init-scale weights, B = 32), the variants timed in alternation in one process (median over rounds of back-to-back calls, events on
torch's current stream; the spread of a variant = max - min over its rounds).  Prints one JSON line: ms of forward(), of decode() with every
latent given, of reconstruct() at 0, nl / 2 and nl posterior layers, and of generate().

  --convs              instead: down_conv1 in full (iaf_conv3x3_forward, the path decode() falls back to) against the h_det-only form
                       (iaf_conv3x3_forward_hdet) at 16x16 and 8x8, B = 32: each a captured graph of --reps launches, replayed in
                       alternation; one JSON line per size with the median us per launch, the spread of each, and the verdict (faster by
                       more than both spreads?).  --shapes "4,3;2,3;2,1": also the form under these launch shapes (IAF_HDET_SHAPE).
  --convs --eager      20 plain calls of each instead (no graph, no timing): the workload of a kernel-trace run,
                       rocprofv3 --kernel-trace -d DIR -o run -- python tools/latents_bench.py --convs --eager
  --summarize FILE     per (kernel, grid) of a rocprofv3 run (its rocpd run_results.db, or a kernel_trace.csv): calls and median duration
                       (us) of the split-product conv kernels, EPI 3 = the full conv, EPI 7 = the prior / h_det-only form"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from generate_bench import summarize, timed  # noqa: E402


def stats(ts):
    return dict(median=round(float(np.median(ts)), 4), spread=round(float(np.max(ts) - np.min(ts)), 4))


def model_bench(args):
    import torch
    import golden_inputs as gi
    import iaf_amd
    B, zs, hs = args.batch, 32, 160
    gi.MODEL_CASES["latents_bench"] = (B, 1, zs, hs, 2, args.num_blocks, 32, 0.25)
    c = gi.model_case_inputs("latents_bench")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    model = iaf_amd.CVAE1(z_size=zs, h_size=hs, kl_min=0.25, depth=2, num_blocks=args.num_blocks, k=1, image_size=32, mode="train")
    model.load({k: dev(v) for k, v in c["params"].items()})
    noise = [dev(e) for e in c["noise"]]
    x = torch.from_numpy(c["x"]).cuda()
    nl = 2 * args.num_blocks
    z = model.encode(x, noise)["z"]
    variants = [("forward", lambda: model.forward(x, noise)), ("decode_all_given", lambda: model.decode(z)),
                ("generate", lambda: model.generate(noise[0::2]))]
    for n in (0, nl // 2, nl):
        variants.append(("reconstruct_%d" % n, lambda n=n: model.reconstruct(x, noise, n)))
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    diff = float((model.decode(z) - model.forward(x, noise)[0]).abs().max().item())
    ts = {nm: [] for nm, _ in variants}
    for _ in range(args.rounds):                       # alternating: drift of clocks / neighbours hits all alike
        for nm, fn in variants:
            ts[nm].append(timed(fn, args.reps))
    out = {"tool": "latents_bench", "B": B, "z": zs, "h": hs, "depth": 2, "num_blocks": args.num_blocks, "rounds": args.rounds,
           "reps": args.reps, "decode_vs_forward_max_abs_diff": diff}
    for nm, _ in variants:
        out[nm + "_ms"] = stats(ts[nm])
    out["decode_over_forward"] = round(out["decode_all_given_ms"]["median"] / out["forward_ms"]["median"], 4)
    print(json.dumps(out), flush=True)


def conv_bench(args):
    import torch
    import golden_inputs as gi
    import iaf_amd
    B, zs, hs = args.batch, 32, 160
    rng = np.random.RandomState(7)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    shapes = [s for s in (args.shapes or "").split(";") if s]
    for H in (16, 8):
        p = gi.conv_params(rng, hs, 4 * zs + 2 * hs)
        conv = iaf_amd.WNConv2d(hs, 4 * zs + 2 * hs)
        conv.prepare(dev(p["V"]), dev(p["g"]), dev(p["b"]))
        x = dev(rng.standard_normal((B, hs, H, H)))
        outs = [torch.empty((B, ch, H, H), device="cuda") for ch in [zs] * 4 + [hs] * 2]
        full = lambda: conv(x, elu_input=True, split=[zs] * 4 + [hs] * 2, out=outs)
        form = lambda: conv.hdet(x, zs, elu_input=True)
        if args.eager:
            for fn in (full, form):
                for _ in range(20):
                    fn()
            torch.cuda.synchronize()
            print("%dx%d B=%d: down_conv1 f16x2 %s" % (H, H, B, conv.runs_f16x2(B, H, H)), flush=True)
            continue
        variants = [("full", None, full), ("hdet", None, form)] + [("hdet[%s]" % s, s, form) for s in shapes]
        graphs = []
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for nm, env, fn in variants:
                os.environ.pop("IAF_HDET_SHAPE", None)
                if env:
                    os.environ["IAF_HDET_SHAPE"] = env          # (read at every launch; a captured graph keeps the shape it was captured with)
                fn()
                side.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    for _ in range(args.reps):
                        fn()
                graphs.append((nm, g))
            os.environ.pop("IAF_HDET_SHAPE", None)
            side.synchronize()
            ts = {nm: [] for nm, _ in graphs}
            for _ in range(args.rounds):
                for nm, g in graphs:
                    ts[nm].append(1e3 * timed(g.replay, 1) / args.reps)
        res = {nm: stats(ts[nm]) for nm, _ in graphs}
        f, h = res["full"], res["hdet"]
        print(json.dumps({"tool": "latents_bench --convs", "B": B, "HxW": "%dx%d" % (H, H), "f16x2": conv.runs_f16x2(B, H, H), "us": res,
                          "hdet_over_full": round(h["median"] / f["median"], 4),
                          "faster_by_more_than_the_spreads": bool(f["median"] - h["median"] > max(f["spread"], h["spread"])),
                          "rounds": args.rounds, "reps": args.reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--num-blocks", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--convs", action="store_true")
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--summarize", default=None)
    args = ap.parse_args()
    if args.summarize is not None:
        summarize(args.summarize)
    elif args.convs:
        conv_bench(args)
    else:
        model_bench(args)


if __name__ == "__main__":
    main()
