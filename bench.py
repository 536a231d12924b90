#!/usr/bin/env python3
"""bench.py -- IAF-step throughput of the MI355X engine on BASELINE.json's configs[1].

  python bench.py --gpus N --steps K --warmup W
  N>1: one rank per GPU over RCCL.  Launched either by the driver as `python -m torch.distributed.run --nnodes=1
  --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...` (RANK/LOCAL_RANK/WORLD_SIZE in the
  env), or plainly as `python bench.py --gpus N`, in which case bench.py starts those N ranks itself.  It refuses to
  run when fewer than N GPUs are visible or when WORLD_SIZE disagrees with --gpus; `n_gpus` in the JSON line is the
  number of ranks that took part, read back from the communicator (`rccl_ranks`, one entry per rank in `devices`).

Workload (config.workload): "cifar10 n_z=32 n_h=160 depths=[10,10] depth_ar=2 down_iaf2_nl bs=32":
one STEP = one pass of the IAF hot path (weight prep + ar_multiconv2d + affine transform +
log-det term, tf_train.py:69-72) over one synthetic batch of 32 through the model's layer schedule:
10 IAF layers on [32,32,16,16] latents and 10 on [32,32,8,8], each layer with its own weights,
z and context (seeded N(0,1) data, random-init weights; inputs resident in HBM).
value = samples/s through the whole IAF stack = N_gpus * 32 / t_step  (weak scaling: each rank
runs its own batch of 32; the forward path has no collective).

The timed region replays a hipGraph of the step (1 batched weight prep + 60 conv launches); right after it
the dominant kernel (the 160->160 masked conv at 16x16) is timed with HIP events on the same stream
(50 back-to-back launches per event pair, and per-launch brackets inside eager steps) for the roofline.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 MFMA; a bf16x3 fp32-grade product costs 6 bf16 products
PEAK_BF16X3_TFLOPS = PEAK_BF16_MFMA_TFLOPS / 6.0
PEAK_HBM_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32, help="per-GPU batch (BASELINE config 2: 32)")
    ap.add_argument("--n-z", type=int, default=32)
    ap.add_argument("--n-h", type=int, default=160)
    ap.add_argument("--depth-ar", type=int, default=2)
    ap.add_argument("--depths", type=str, default="10,10")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--cached-weights", action="store_true",
                    help="prepare weights once outside the timed region (inference with frozen weights); "
                         "default re-derives mask*V / weight-norm every step like the reference graph does")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget of the cpu_baseline leg (rank 0, N=1)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--tune", type=str, default="", help="layer:nt,pxt,wco,ks;... launch-shape override")
    ap.add_argument("--layers", action="store_true",
                    help="widened workload (SURVEY 8f-4): whole IAFLayers (plain convs + posterior block), forward")
    ap.add_argument("--model", action="store_true",
                    help="with --layers: the whole model forward, CVAE1._forward (tf_train.py:150-218): uint8 images -> x_enc -> the "
                         "layer stack -> x_dec -> discretized_logistic -> obj / loss; with --train: one tower's whole training step "
                         "from that objective (all gradients, all-reduce, Adamax/EMA)")
    ap.add_argument("--train", action="store_true",
                    help="extra mode (not the headline metric): data-parallel TRAINING step of the IAF posterior stack -- "
                         "posterior block forward + backward for every layer, one RCCL all-reduce of the flat gradient "
                         "buffer, fused Adamax + EMA")
    ap.add_argument("--all-packs", action="store_true",
                    help="--layers (inference): keep every weight pack of every conv up to date instead of the one its launch reads")
    ap.add_argument("--precision", type=str, default="f16x2", choices=["f16x2", "bf16x3", "f32"],
                    help="arithmetic of the forward masked convs: f16x2 (the engine's default since round 6) = the one-launch step "
                         "kernels of the BASELINE geometries split every fp32 operand into two fp16 planes (hi, lo 2^11) and accumulate "
                         "three part-products in two fp32 accumulators on the fp16 matrix cores, everything else as bf16x3; bf16x3 = "
                         "three bf16 parts, six part-products (fp32-grade; round 5's default); f32 = the exact-fp32 MFMA everywhere")
    ap.add_argument("--no-fuse", action="store_true",
                    help="never run the first masked conv inside the second one's kernel (iaf_stack_set_fuse_first)")
    ap.add_argument("--no-fuse-step", action="store_true",
                    help="run every IAF step layer by layer instead of as one launch (iaf_stack_set_fuse_step)")
    ap.add_argument("--no-autotune", action="store_true",
                    help="skip the per-layer kernel/launch-shape search (iaf_stack_autotune) before the timed region")
    ap.add_argument("--ar-buckets", type=int, default=4,
                    help="--train: number of gradient all-reduce buckets overlapped with the backward pass")
    ap.add_argument("--iw-eval", action="store_true",
                    help="extra mode: BASELINE configs[4] -- importance-weighted ELBO evaluation, rows of --batch (256) "
                         "importance samples per pass through every layer's posterior block, k samples per image streamed "
                         "through the online log-sum-exp")
    ap.add_argument("--iw-k", type=int, default=10000, help="--iw-eval: importance samples per image")
    ap.add_argument("--keep-f32-pack", action="store_true",
                    help="keep the fp32 fragment pack up to date in the per-step weight prep even when every step runs on the "
                         "bf16 matrix cores (iaf_stack_set_packs; default: dropped when no launch of the workload reads it)")
    ap.add_argument("--no-modes", action="store_true",
                    help="default mode: skip the `modes` object (quick in-process runs of --train --model, --layers --model and "
                         "--iw-eval --model behind the headline measurement, ~20 s)")
    ap.add_argument("--repeats", type=int, default=5,
                    help="the timed region (--steps steps between barriers) is run this many times; the median is reported")
    ap.add_argument("--settle-seconds", type=float, default=0.4,
                    help="untimed replays after the --warmup steps until the GPU has been busy this long (clocks, graph upload)")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="default mode: after the timed region, write what its last step computed (every layer's z_new and logsd, "
                         "stacked per latent level) to DIR/<name>.npy in float32, at most 64 MB in all (a fixed seeded sample beyond)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and (args.train or args.layers or args.model or args.iw_eval):
        ap.error("--dump-outputs writes the default workload's outputs; it does not combine with --train, --layers, --model or --iw-eval")
    return args


DUMP_BYTES = 64 << 20


def dump_outputs(dirname, layers):
    """--dump-outputs: the arrays a caller of the timed step receives -- each layer's (z_new, logsd) of iaf_step -- as
    <name>_<H>x<W>.npy, [layers, B, n_z, H, W] float32.  Beyond DUMP_BYTES in all, every array is cut to the same share of its
    elements at fixed seeded positions (flat, ascending), so that two runs with the same arguments still compare element for element."""
    os.makedirs(dirname, exist_ok=True)
    arrays = {}
    for H in sorted({L["H"] for L in layers}, reverse=True):
        lv = [L for L in layers if L["H"] == H]
        for i, name in enumerate(("z_new", "logsd")):
            arrays["%s_%dx%d" % (name, H, H)] = torch.stack([L["out"][i] for L in lv]).float().cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > DUMP_BYTES:
            keep = a.size * DUMP_BYTES // total
            a = a.reshape(-1)[np.sort(np.random.RandomState(0).choice(a.size, keep, replace=False))]
        np.save(os.path.join(dirname, name + ".npy"), a)


RANK_INFO = {}
OUT_FD = [None]
CAPTURE = [None]      # a list: emit() appends to it instead of printing (the default mode's `modes` object runs the other modes in-process)


def emit(out):
    """rank 0's ONE JSON line; every mode reports who actually took part (read back from the communicator)"""
    out = dict(out)
    if CAPTURE[0] is not None:
        CAPTURE[0].append(out)
        return
    out["rccl_ranks"] = RANK_INFO.get("rccl_ranks")
    out["devices"] = RANK_INFO.get("devices")
    if "halo_exchange" in RANK_INFO:
        out["halo_exchange"] = RANK_INFO["halo_exchange"]
    line = json.dumps(out) + "\n"
    if OUT_FD[0] is not None:          # multi-rank runs: fd 1 points at stderr (RCCL banners), the JSON goes to the real stdout
        sys.stdout.flush()
        os.write(OUT_FD[0], line.encode())
    else:
        sys.stdout.write(line)
        sys.stdout.flush()


def force_dist(args):
    """The training modes run their gradient exchange through RCCL even on ONE GPU (a one-rank communicator: the call path, stream
    ordering and graph capture of the real thing; IAF_BENCH_FORCE_DIST=0 turns that off, =1 turns it on for the other modes)."""
    if getattr(args, "_no_dist", False):      # (the quick in-process runs behind the headline line: no process group)
        return False
    v = os.environ.get("IAF_BENCH_FORCE_DIST")
    return (v not in ("0", "")) if v is not None else bool(args.train)


def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves (torch.distributed.run, one process
    per GPU, rendezvous on 127.0.0.1) and hand their stdout through -- rank 0 prints the JSON line."""
    import subprocess
    ndev = torch.cuda.device_count()
    if ndev < args.gpus:
        sys.exit("bench.py: --gpus %d but only %d GPU(s) visible on this node" % (args.gpus, ndev))
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC only on this driver (RCCL / tensor sharing)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


def init_ranks(args):
    """-> (dist or None, rank, n_ranks, info).  n_ranks is what the communicator reports, not what --gpus asked for."""
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args)                                  # does not return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d: launch one rank per requested GPU" % (args.gpus, world))
    if not torch.cuda.is_available() or torch.cuda.device_count() <= local_rank:
        sys.exit("bench.py: rank %d needs GPU %d but %d GPU(s) are visible" % (rank, local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    info = {"rccl_ranks": None, "devices": ["rank0:cuda:%d %s" % (local_rank, torch.cuda.get_device_name(local_rank))]}
    if world == 1 and not force_dist(args):               # (training modes: the RCCL path runs on one GPU too)
        return None, 0, 1, info
    import torch.distributed as dist
    # RCCL prints a banner (ROCm version / hostname / library path) to STDOUT whenever a communicator comes up (the first
    # collective on a stream, possibly long after init); the contract is ONE JSON line on stdout, so for the rest of the
    # process fd 1 points at stderr and emit() writes the JSON line to the saved, real stdout
    sys.stdout.flush()
    OUT_FD[0] = os.dup(1)
    os.dup2(2, 1)
    if world == 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(free_port()))
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    try:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        dist.barrier()
    except Exception as e:          # noqa: BLE001
        if world > 1:
            raise
        # (the one-rank communicator of the single-GPU training modes is a convenience -- the same call path as N ranks --,
        #  not a requirement: without it the step runs with no exchange and the line says so)
        info["rccl_one_rank_init"] = "failed (%s): no communicator, the gradient exchange is skipped" % (str(e).splitlines() or [""])[0][:160]
        os.dup2(OUT_FD[0], 1)
        OUT_FD[0] = None
        return None, 0, 1, info
    # read the participants back from the communicator: every rank contributes 1 and its device identity
    ones = torch.ones(1, device="cuda")
    dist.all_reduce(ones)
    props = torch.cuda.get_device_properties(local_rank)
    ident = "rank%d:cuda:%d %s %s" % (rank, local_rank, props.name, getattr(props, "uuid", ""))
    idents = [None] * dist.get_world_size()
    dist.all_gather_object(idents, ident)
    torch.cuda.synchronize()
    info = {"rccl_ranks": int(ones.item()), "devices": idents}
    if info["rccl_ranks"] != dist.get_world_size() or len(set(idents)) != len(idents):
        sys.exit("bench.py: communicator reports %r ranks / devices %r" % (info["rccl_ranks"], idents))
    return dist, rank, dist.get_world_size(), info


def make_layer_inputs(rng, B, n_z, n_h, depth_ar, H):
    import golden_inputs as gi
    params = gi.ar_multiconv2d_params(rng, n_z, [n_h] * depth_ar, [n_z, n_z])
    # SURVEY 8d synthetic inputs: V~N(0,.05^2), g,b~N(0,.1^2), z,context~N(0,1)
    for k in params:
        if k.endswith("/g") or k.endswith("/b"):
            params[k] = 0.1 * rng.standard_normal(params[k].shape)
    z = rng.standard_normal((B, n_z, H, H))
    ctx = rng.standard_normal((B, n_h, H, H))
    return params, z, ctx


def cpu_baseline(args, depths):
    """torch-CPU fp32 port (oracle/iaf_cpu_port.py) on a bounded sample of the same workload."""
    from oracle import iaf_cpu_port as Pt
    ncpu = os.cpu_count() or 1
    # oneDNN convs of this size stop scaling (and collapse when oversubscribed) well before a 128+-core host is
    # full: probe a few thread counts on the 16x16 step and keep the fastest -- that is the baseline we report.
    prng = np.random.RandomState(7)
    params, z, ctx = make_layer_inputs(prng, args.batch, args.n_z, args.n_h, args.depth_ar, 16)
    tp = Pt.as_torch(params)
    w = Pt.prepare_weights(tp, args.n_z, [args.n_h] * args.depth_ar)
    zt, ct = torch.from_numpy(z.astype(np.float32)), torch.from_numpy(ctx.astype(np.float32))
    best = None
    for nt in sorted(set(min(c, ncpu) for c in (4, 8, 16, 32, 64, 128))):
        torch.set_num_threads(nt)
        with torch.no_grad():
            Pt.iaf_step(zt, ct, w, args.depth_ar)
            t0 = time.perf_counter()
            for _ in range(3):
                Pt.iaf_step(zt, ct, w, args.depth_ar)
            dt = (time.perf_counter() - t0) / 3
        if best is None or dt < best[0]:
            best = (dt, nt)
        if dt > 4 * best[0]:
            break
    nthreads = best[1]
    torch.set_num_threads(nthreads)
    rng = np.random.RandomState(1)
    per_level = []
    budget = args.cpu_seconds / max(len(depths), 1)
    for lvl, _ in enumerate(depths):
        H = 16 >> lvl
        params, z, ctx = make_layer_inputs(rng, args.batch, args.n_z, args.n_h, args.depth_ar, H)
        tp = Pt.as_torch(params)
        zt, ct = torch.from_numpy(z.astype(np.float32)), torch.from_numpy(ctx.astype(np.float32))

        def one():
            w = tp_w if args.cached_weights else Pt.prepare_weights(tp, args.n_z, [args.n_h] * args.depth_ar)
            return Pt.iaf_step(zt, ct, w, args.depth_ar)

        tp_w = Pt.prepare_weights(tp, args.n_z, [args.n_h] * args.depth_ar)
        with torch.no_grad():
            for _ in range(3):
                one()
            ts = []
            t_end = time.perf_counter() + budget
            while time.perf_counter() < t_end or len(ts) < 5:
                t0 = time.perf_counter()
                one()
                ts.append(time.perf_counter() - t0)
        per_level.append(float(np.median(ts)))
    t_model = sum(d * t for d, t in zip(depths, per_level))
    return {
        "value": args.batch / t_model, "unit": "samples/s", "cores": nthreads, "kind": "port",
        "sample": "torch-CPU fp32 port of the same IAF step (oracle/iaf_cpu_port.py), B=%d: median of repeated single "
                  "IAF steps per level (%s ms at %s), ~%.0f s total, scaled to the depths=%s schedule; the reference has "
                  "no CPU path (SURVEY D1); %d of %d host CPUs used (fastest of a thread-count probe)" % (args.batch, ",".join("%.2f" % (1e3 * t) for t in per_level),
                                              ",".join("%dx%d" % (16 >> i, 16 >> i) for i in range(len(depths))),
                                              args.cpu_seconds, depths, nthreads, ncpu),
        "ms_per_iaf_step": [1e3 * t for t in per_level],
    }


def _exchange_sweep(flat, red, dist, counts=(1, 2, 4, 8, 16), reps=3):
    """the same flat gradient buffer all-reduced ALONE as 1, 2, 4, ... equal contiguous messages back to back (ms per whole
    exchange): what bucket size costs on this node's links before any overlap -- read next to `exposed_ms` it says whether a
    different --ar-buckets would help (xGMI rings are per-link bound: few large messages)"""
    if not red.active:
        return None
    n = flat.grads.numel()
    one = (lambda t: red.comm.all_reduce_sum_(t)) if red.comm is not None else (lambda t: dist.all_reduce(t))
    out = {}
    for c in counts:
        cuts = [n * i // c for i in range(c + 1)]
        views = [flat.grads[cuts[i]:cuts[i + 1]] for i in range(c) if cuts[i + 1] > cuts[i]]
        for v in views:
            one(v)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            for v in views:
                one(v)
        b.record()
        b.synchronize()
        out[str(c)] = a.elapsed_time(b) / reps
    return out


def _exchange_expectation(n_floats, n_gpus):
    """what the all-reduce should take on one MI355X node, so that a first multi-GPU run can be judged at once: a ring all-reduce
    moves 2 (N-1)/N of the buffer through every GPU; xGMI is point to point, 7 links x ~153 GB/s per GPU (the task's hardware
    notes), and RCCL lays its rings over the links it finds"""
    if n_gpus < 2:
        return None
    mb = 4e-6 * n_floats
    per_gpu_mb = 2.0 * (n_gpus - 1) / n_gpus * mb
    return {"buffer_mb": mb, "moved_per_gpu_mb": per_gpu_mb,
            "ms_if_one_link_carries_it": per_gpu_mb / 153.0, "ms_if_seven_links_share_it": per_gpu_mb / (7 * 153.0),
            "note": "ring all-reduce, 153 GB/s per xGMI link and direction; anything above the one-link figure means the rings are "
                    "not using the fabric, anything near the seven-link figure is as good as this topology gets"}


def _chunks(lst, n):
    n = max(1, min(n, len(lst)))
    return [lst[i * len(lst) // n:(i + 1) * len(lst) // n] for i in range(n)]


def _time_exchange(flat, red, dist, reps=5):
    """the gradient exchange alone: `reps` all-reduces of the whole flat bucket between one event pair (ms each)"""
    if not red.active:
        return None
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # through the C ABI (iaf_allreduce_sum_f32 = ncclAllReduce) like the training step's own buckets
    one = (lambda: red.comm.all_reduce_sum_(flat.grads)) if red.comm is not None else (lambda: dist.all_reduce(flat.grads))
    one()
    a.record()
    for _ in range(reps):
        one()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _run_segmented(args, segments, red, flat, n_gpus, dist):
    """Shared driver of the two training modes.  `segments[i]()` enqueues the compute that completes gradient bucket i
    (segment 0 also holds weight prep and the forward pass); each segment replays as its own hipGraph and bucket i's
    all-reduce is issued right behind it, overlapping the remaining segments (parallel.OverlappedGradReduce)."""
    nb = len(segments)

    def step_eager():
        for i in range(nb):
            segments[i]()
            red.reduce(i)
        red.wait()
        flat.adamax_ema_step(1e-4, world=n_gpus)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    stream = torch.cuda.Stream()
    graphs, whole = None, None
    with torch.cuda.stream(stream):
        step_eager()
        stream.synchronize()
        step = step_eager
        if not args.no_graph:
            graphs = []
            for i in range(nb):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=stream):
                    segments[i]()
                graphs.append(g)

            def step():  # noqa: F811
                for i in range(nb):
                    graphs[i].replay()
                    red.reduce(i)
                red.wait()
                flat.adamax_ema_step(1e-4, world=n_gpus)

            # ... or the WHOLE step as one graph: the exchange stream forks off the compute stream behind every segment and joins in front of
            # the optimiser INSIDE the capture (ncclAllReduce is capturable), so a replay has no host in its loop at all -- between
            # per-segment graphs the host's launch + cross-stream waits cost ~0.14 ms per bucket (r04: exposed_ms 0.56 with ONE rank, whose
            # all-reduce is a 5 us no-op).  Falls back to the per-segment graphs if the runtime refuses the capture.
            whole = None
            if not os.environ.get("IAF_BENCH_SEGMENT_GRAPHS"):
                try:
                    g1 = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g1, stream=stream, capture_error_mode="thread_local"):
                        step_eager()
                    g1.replay()
                    stream.synchronize()
                    whole = g1
                except Exception as e:          # noqa: BLE001
                    sys.stderr.write("bench.py: one-graph capture of the training step refused (%s): per-segment graphs\n" % (str(e).splitlines() or [""])[0])
                    whole = None
                    torch.cuda.synchronize()
            if whole is not None:
                step = whole.replay
        for _ in range(args.warmup):
            step()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        elapsed = time.perf_counter() - t0
        # the same step without the exchange, and the exchange alone: how much of it the overlap hides
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = max(3, min(args.steps, 10))
        a.record()
        for _ in range(reps):
            for i in range(nb):
                (graphs[i].replay if graphs is not None else segments[i])()
            flat.adamax_ema_step(1e-4, world=n_gpus)
        b.record()
        b.synchronize()
        compute_ms = a.elapsed_time(b) / reps
        exch_ms = _time_exchange(flat, red, dist)
        sweep = _exchange_sweep(flat, red, dist)
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    step_ms = 1e3 * elapsed / args.steps
    exchange = {"collective": "all-reduce(sum) fp32, 1/N folded into the Adamax kernel (tf_utils/common.py:83-86)",
                "executed": bool(red.active), "buckets": nb,
                "via": ("C ABI iaf_allreduce_sum_f32 (ncclAllReduce of %s) on a dedicated exchange stream" % red.comm.library)
                       if red.comm is not None else "torch.distributed",
                "bucket_mb": [4e-6 * (hi - lo) for lo, hi in red.bounds],
                "alone_ms": exch_ms, "step_without_exchange_ms": compute_ms,
                "exposed_ms": (step_ms - compute_ms) if red.active else 0.0,
                "alone_ms_by_message_count": sweep, "expected_on_this_node": _exchange_expectation(flat.grads.numel(), n_gpus),
                "rccl_ranks": RANK_INFO.get("rccl_ranks"),
                "overlap": "bucket i is reduced while the backward segments i+1.. run (issued behind its segment's graph)"}
    exchange["launch"] = ("one hipGraph for the whole step: segments, forked all-reduces, join, optimiser" if (graphs is not None and whole is not None)
                          else "one hipGraph per segment, the all-reduces issued between the replays" if graphs is not None else "eager")
    return elapsed, graphs is not None, exchange


def _train_roofline(fwd_flops, ms_per_step, mode):
    """VERDICT r05 "next" #3b: the training lines' roofline.  Work = the forward's live FLOPs (mask-aware) three times over:
    forward, data gradients (dX = W^T dY: the same contraction), weight gradients (dW = X^T dY: the same again; the MADE mask on dV,
    graphy/nodes/ar.py:369-373, makes the same half of it live).  Peak = the pipe the forward and most of the backward run on (bf16x3:
    2500 / 6 TF; the round-6 fp16 planes of the step kernels are priced against the same denominator).  `kernels`: the six launches
    that take most of one steady-state step, from the committed rocprofv3 kernel trace of the same command (tools/step_breakdown.py
    --json), each family with the live FLOPs it carries and its own fraction of the pipe."""
    tf_ = 3.0 * fwd_flops / (ms_per_step * 1e-3) / 1e12
    r = {"bound": "mfma", "achieved": tf_, "peak": PEAK_BF16X3_TFLOPS, "unit": "TFLOP/s", "frac": tf_ / PEAK_BF16X3_TFLOPS, "traffic": None,
         "frac_of_f32_mfma_peak": tf_ / PEAK_F32_MFMA_TFLOPS,
         "live_gflop_per_step": {"forward": fwd_flops / 1e9, "data_gradients": fwd_flops / 1e9, "weight_gradients": fwd_flops / 1e9},
         "note": "whole training step (weight prep + forward + backward + weight-norm backward + all-reduce + Adamax/EMA) against the "
                 "bf16x3 pipe peak; live FLOPs = 3 x the forward's mask-aware count"}
    pth = os.path.join(ROOT, "profiles", "train_kernels_%s.json" % mode)
    if os.path.exists(pth):
        try:
            tj = json.load(open(pth))
            fam = {}
            for k in tj.get("families", []):
                # a family's live FLOPs: forward-shaped convs carry forward + data gradients (2 F), the weight-gradient kernels F
                share = {"conv": 2.0, "wgrad": 1.0}.get(k["family"])
                if share and k["us_per_step"] > 0:
                    k = dict(k)
                    k["live_gflop_per_step"] = share * fwd_flops / 1e9
                    k["frac"] = share * fwd_flops / (k["us_per_step"] * 1e-6) / 1e12 / PEAK_BF16X3_TFLOPS
                fam[k["family"]] = k
            r["kernels"] = tj.get("top", [])[:6]
            r["kernel_families"] = list(fam.values())
            r["kernels_source"] = tj.get("source")
        except Exception:
            pass
    return r


def train_bench(args, depths, dist, rank, n_gpus):
    """DP training step of the IAF posterior stack (SURVEY 8f-1,2): per step, for every layer, posterior block forward
    (tf_train.py:56-85) + backward (what opt.compute_gradients derives, tf_train.py:138), gradients written into ONE flat
    buffer laid out in completion order, bucketed all-reduce(sum) over ranks (RCCL) overlapped with the remaining
    backward, fused Adamax(1/N)+EMA (tf_utils/common.py:86, adamax.py:40-56, tf_train.py:157-158).  Synthetic upstream
    gradients (dz ~ N(0,1), dkl_obj = 1)."""
    import iaf_amd
    from iaf_amd import parallel as par
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    rng = np.random.RandomState(4321 + rank)
    wrng = np.random.RandomState(99)                      # identical initial weights on every rank
    layers, named = [], {}
    for lvl, nlayer in enumerate(depths):
        H = 16 >> lvl
        for j in range(nlayer):
            params, _, _ = make_layer_inputs(wrng, args.batch, args.n_z, args.n_h, args.depth_ar, H)
            f = lambda c: dev(rng.standard_normal((args.batch, c, H, H)))
            inp = dict(qm=f(args.n_z), ql=0.1 * f(args.n_z), rm=f(args.n_z), rl=0.1 * f(args.n_z), pm=f(args.n_z),
                       pl=0.1 * f(args.n_z), uc=f(args.n_h), dc=f(args.n_h), eps=f(args.n_z), dz=f(args.n_z),
                       dko=torch.ones(args.batch, device="cuda"))
            st = iaf_amd.ARStack(args.n_z, [args.n_h] * args.depth_ar)
            st.set_training(True)
            pre = "IAF_%d_%d/ar_multiconv2d/" % (lvl, j)
            for k, v in params.items():
                named[pre + k] = dev(v)
            layers.append(dict(stack=st, pre=pre, keys=list(params), inp=inp, H=H))
    flat = par.FlatParams(named)          # `named` is in layer order == the order this step completes the gradients
    for L in layers:
        L["params"] = {k: flat.p[L["pre"] + k] for k in L["keys"]}
        L["gradviews"] = {k: flat.g[L["pre"] + k] for k in L["keys"]}
    groups = _chunks(layers, args.ar_buckets)
    bounds = par.OverlappedGradReduce.bounds_from_groups(flat, [[L["pre"] + k for L in g for k in L["keys"]] for g in groups])
    red = par.OverlappedGradReduce(flat, bounds, force=force_dist(args))
    prep = iaf_amd.PrepBatch([L["stack"] for L in layers])
    plist = [L["params"] for L in layers]
    # mask + weight-norm backward: one launch per bucket (it finishes the bucket's dV / dg)
    wnbs = [iaf_amd.WnBwdBatch(stacks=[L["stack"] for L in g]) for g in groups]

    def make_segment(bi):
        def seg():
            if bi == 0:
                prep.run(plist)
            for L in groups[bi]:
                i, st = L["inp"], L["stack"]
                fw = st.posterior_block_train(i["qm"], i["ql"], i["rm"], i["rl"], i["pm"], i["pl"], i["uc"], i["dc"], i["eps"], 0.25)
                st.posterior_block_backward(i["qm"], i["ql"], i["rm"], i["rl"], i["pm"], i["pl"], i["eps"], 0.25, fw["z"], i["dz"],
                                            i["dko"], L["params"], grads_out=L["gradviews"])
            wnbs[bi].run(stack_params=[L["params"] for L in groups[bi]], stack_grads=[L["gradviews"] for L in groups[bi]])
        return seg

    elapsed, graphed, exchange = _run_segmented(args, [make_segment(i) for i in range(len(groups))], red, flat, n_gpus, dist)
    if rank == 0:
        emit({
            "metric": "IAF posterior-stack TRAIN-step samples/sec (forward + backward + grad all-reduce + Adamax/EMA)",
            "value": n_gpus * args.batch / (elapsed / args.steps), "unit": "samples/s", "n_gpus": n_gpus, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32" if args.precision == "f32" else "f32 (forward convs: operands split into 3 bf16 parts, 6 part-products on the bf16 MFMA, fp32 accumulate: fp32-grade error; backward: exact fp32 MFMA)", "data": "synthetic",
            "config": {"workload": "cifar10 n_z=%d n_h=%d depths=%s depth_ar=%d down_iaf2_nl bs=%d per GPU, kl_min=0.25; "
                                   "%d trainable fp32 parameters in one flat gradient buffer (%.1f MB)"
                                   % (args.n_z, args.n_h, depths, args.depth_ar, args.batch, flat.params.numel(),
                                      4e-6 * flat.params.numel()),
                       "global_batch": n_gpus * args.batch,
                       "launch": "hipGraph replay per gradient bucket, all-reduce behind each, then the update" if graphed else "eager",
                       "parallelism": "dp%d (RCCL all-reduce of %d gradient buckets, overlapped with backward)" % (n_gpus, len(groups))},
            "roofline": _train_roofline(sum(L["stack"].step_work(args.batch, L["H"], L["H"])["live_flops"] for L in layers),
                                        1e3 * elapsed / args.steps, "stacks"),
            "exchange": exchange})


def layers_bench(args, depths, dist, rank, n_gpus):
    """SURVEY 8f-4 widening: the whole IAFLayer stack of BASELINE configs[1] as ONE connected model (tf_train.py:188-200),
    forward, mode "train": the bottom-up pass through every layer -- the first layer of each coarser level downsamples
    (tf_train.py:196: stride-2 up_conv1, resize 0.5) -- then the top-down pass back (down_deconv2 + resize 2 in the
    downsampling layer); all weight-norm reparametrisations re-derived every step in batched launches."""
    import golden_inputs as gi
    import iaf_amd
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    rng = np.random.RandomState(777 + rank)
    wrng = np.random.RandomState(5)
    zs, hs, B = args.n_z, args.n_h, args.batch
    levels = []
    for lvl, nlayer in enumerate(depths):
        H = 16 >> lvl
        L = []
        for j in range(nlayer):
            ds = lvl > 0 and j == 0                                         # tf_train.py:196
            p = {}
            for nm, (ci, co) in (("up_conv1", (hs, 2 * zs + 2 * hs)), ("up_conv3", (hs, hs)),
                                 ("down_conv1", (hs, 4 * zs + 2 * hs))):
                for k, v in gi.conv_params(wrng, ci, co).items():
                    p[nm + "/" + k] = dev(v)
            last = gi.deconv_params(wrng, hs + zs, hs) if ds else gi.conv_params(wrng, hs + zs, hs)
            for k, v in last.items():
                p[("down_deconv2/" if ds else "down_conv2/") + k] = dev(v)
            for k, v in gi.ar_multiconv2d_params(wrng, zs, [hs] * args.depth_ar, [zs, zs]).items():
                p["ar_multiconv2d/" + k] = dev(v)
            layer = iaf_amd.IAFLayer(zs, hs, depth_ar=args.depth_ar, kl_min=0.25, downsample=ds)
            layer.posterior.stack.set_precision(args.precision)
            for cvx in layer.convs():
                cvx.set_precision(args.precision)
            layer.load(p)
            L.append(dict(layer=layer, params=p, eps=dev(rng.standard_normal((B, zs, H, H)))))
        levels.append(dict(H=H, layers=L))
    up_in = dev(0.5 * rng.standard_normal((B, hs, 16, 16)))
    Htop = 16 >> (len(depths) - 1)
    down_in = dev(0.5 * rng.standard_normal((B, hs, Htop, Htop)))
    all_layers = [L for lv in levels for L in lv["layers"]]
    prep_s = iaf_amd.PrepBatch([L["layer"].posterior.stack for L in all_layers])
    # plain convs in one batched prep launch; a downsampling layer's deconv has its own (two small launches)
    bconvs, cplist, deconvs = [], [], []
    for L in all_layers:
        lay, p = L["layer"], L["params"]
        for nm in ("up_conv1", "up_conv3", "down_conv1") + (() if lay.downsample else ("down_conv2",)):
            bconvs.append(getattr(lay, nm))
            cplist.append((p[nm + "/V"], p[nm + "/g"], p[nm + "/b"]))
        if lay.downsample:
            deconvs.append((lay.down_conv2, p["down_deconv2/V"], p["down_deconv2/g"], p["down_deconv2/b"]))
    prep_c = iaf_amd.ConvPrepBatch(bconvs)
    splist = [iaf_amd.IAFLayer.stack_params(L["params"]) for L in all_layers]
    # --model: the two ends of CVAE1._forward around the stack (tf_train.py:153-159, 183, 189-192, 206-218)
    edge = None
    if args.model:
        from iaf_amd.layers import _ptr, _stream
        lib, chk = iaf_amd._capi.lib(), iaf_amd._capi.check
        ep = {"x_enc/" + k: dev(v) for k, v in gi.conv_params(wrng, 3, hs, ksize=5).items()}
        ep.update({"x_dec/" + k: dev(v) for k, v in gi.deconv_params(wrng, hs, 3, k=5).items()})
        ep["h_top"] = dev(0.3 * wrng.standard_normal(hs))
        ep["dec_log_stdv"] = dev(np.array([-0.7]))
        nl = len(all_layers)
        edge = dict(p=ep, w_enc=torch.empty_like(ep["x_enc/V"]), w_dec=torch.empty_like(ep["x_dec/V"]),
                    img=torch.from_numpy(rng.randint(0, 256, size=(B, 3, 32, 32)).astype(np.uint8)).cuda(),
                    xf=torch.empty((B, 3, 32, 32), device="cuda"), h0=torch.empty((B, hs, 16, 16), device="cuda"),
                    x_out=torch.empty((B, 3, 32, 32), device="cuda"), kl_obj=torch.empty(B, device="cuda"), kl_cost=torch.empty(B, device="cuda"),
                    obj=torch.empty(1, device="cuda"), loss=torch.empty(1, device="cuda"))

    def step(autotune=False):
        if not args.cached_weights:
            prep_s.run(splist)
            prep_c.run(cplist)
            for cv, V, g, b in deconvs:
                cv.prepare_deconv(V, g, b, force=True)
        outs = []
        h = up_in
        if edge is not None:
            E, ep = edge, edge["p"]
            if not args.cached_weights:
                chk(lib.iaf_convk_weightnorm(_ptr(ep["x_enc/V"]), _ptr(ep["x_enc/g"]), _ptr(E["w_enc"]), 5, 5, 3, hs, 0, _stream()))
                chk(lib.iaf_convk_weightnorm(_ptr(ep["x_dec/V"]), _ptr(ep["x_dec/g"]), _ptr(E["w_dec"]), 5, 5, hs, 3, 1, _stream()))
            chk(lib.iaf_image_to_float(E["img"].data_ptr(), _ptr(E["xf"]), B, 3 * 32 * 32, 1, _stream()))
            chk(lib.iaf_convk_forward(_ptr(E["xf"]), _ptr(E["w_enc"]), _ptr(ep["x_enc/b"]), _ptr(E["h0"]), B, 3, 32, 32, hs, 5, 5, 2, 0,
                                      _stream()))
            h = E["h0"]
        for lv in levels:                         # bottom-up (tf_train.py:188-192), chained across levels
            for L in lv["layers"]:
                h = L["layer"].up(h, autotune=autotune)
        h = down_in
        if edge is not None:
            chk(lib.iaf_tile_channels(_ptr(ep["h_top"]), _ptr(down_in), B, hs, Htop * Htop, _stream()))
        li = 0
        for lv in reversed(levels):               # top-down (tf_train.py:195-200)
            for L in reversed(lv["layers"]):
                h, kl_obj, kl_cost = L["layer"].down(h, L["eps"], autotune=autotune)
                outs.append((kl_obj, kl_cost))
                li += 1
        outs.append(h)
        if edge is not None:
            objs, costs = torch.stack([o[0] for o in outs[:li]]), torch.stack([o[1] for o in outs[:li]])
            chk(lib.iaf_colsum(_ptr(objs), _ptr(E["kl_obj"]), li, B, _stream()))
            chk(lib.iaf_colsum(_ptr(costs), _ptr(E["kl_cost"]), li, B, _stream()))
            outs.append((objs, costs))
            chk(lib.iaf_deconvk_forward(_ptr(h), _ptr(E["w_dec"]), _ptr(ep["x_dec/b"]), _ptr(E["x_out"]), B, hs, 16, 16, 3, 5, 5, 2, 1,
                                        -0.5 + 1 / 512., 0.5 - 1 / 512., _stream()))
            log_pxz = iaf_amd.discretized_logistic(E["x_out"], ep["dec_log_stdv"], sample=E["xf"])
            chk(lib.iaf_sum_axpy(_ptr(E["kl_obj"]), _ptr(log_pxz), -1.0, _ptr(E["obj"]), B, _stream()))
            lb = iaf_amd.compute_lowerbound(log_pxz, E["kl_cost"], 1)
            chk(lib.iaf_sum_axpy(_ptr(lb), None, 0.0, _ptr(E["loss"]), B, _stream()))
            outs.append((log_pxz, lb))
        return outs

    if not args.no_autotune and args.depth_ar > 0:      # masked stacks: kernel family / launch shape per layer
        for lv in levels:
            for L in lv["layers"]:
                H = lv["H"]
                L["layer"].posterior.stack.autotune(torch.randn(B, zs, H, H, device="cuda"), torch.randn(B, hs, H, H, device="cuda"), reps=10)

    stream = torch.cuda.Stream()
    graph = None
    with torch.cuda.stream(stream):
        step()
        step(autotune=True)                       # launch-shape search of the plain convs (cuDNN's algorithm search)
        stream.synchronize()
        packs_kept = None
        if not args.all_packs:
            # inference at one size: every conv / stack keeps only the weight pack its launch reads (IAFLayer.trim_packs: the prep launches
            # then write 4-6 instead of 14 bytes per weight; a launch that needed another pack would fail loudly, not read stale weights)
            packs_kept = {}
            for lvl, lv in enumerate(levels):
                for L in lv["layers"]:
                    Hin = 2 * lv["H"] if L["layer"].downsample else lv["H"]
                    for nm, pk in L["layer"].trim_packs(B, Hin, Hin).items():
                        packs_kept[pk] = packs_kept.get(pk, 0) + 1
            step()
            stream.synchronize()
        if not args.no_graph:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                keep = step()
        run = graph.replay if graph is not None else step

        def barrier():
            torch.cuda.synchronize()
            if dist is not None:
                dist.barrier()
            torch.cuda.synchronize()

        for _ in range(args.warmup):
            run()
        barrier()
        # A fresh box starts with the GPU clocks down and the graph not yet resident: 5 warm-up replays of a 0.5 ms step
        # are 2.5 ms.  More untimed replays until the box has been busy for a while (the driver's
        # fresh box read 10 % under the builder's lease), then the timed region -- EXACTLY --steps steps between barrier +
        # synchronize on both sides -- is repeated and the MEDIAN repeat reported (all repeats listed in config.repeats_ms).
        t_settle = time.perf_counter()
        n_settle = 0
        while time.perf_counter() - t_settle < args.settle_seconds:
            for _ in range(max(args.steps, 1)):
                run()
            torch.cuda.synchronize()
            n_settle += max(args.steps, 1)
        repeats = []
        for _ in range(max(1, args.repeats)):
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run()
            barrier()
            repeats.append(time.perf_counter() - t0)
        elapsed = float(np.median(repeats))

        # dominant kernel of this mode: down_conv1 (n_h -> 4 n_z + 2 n_h) at 16x16; 50 back-to-back launches per layer
        # between one event pair on the launch stream
        kt = []
        for L in levels[0]["layers"]:
            cv = L["layer"].down_conv1
            x = up_in
            call = lambda: cv(x, elu_input=True, split=[zs] * 4 + [hs] * 2)
            call()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(50):
                call()
            b.record(stream)
            b.synchronize()
            kt.append(a.elapsed_time(b) / 50)
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank != 0:
        return
    cv = levels[0]["layers"][0]["layer"].down_conv1
    fl, by = cv.work(B, 16, 16)
    k_ms = float(np.mean(kt))
    achieved = fl / (k_ms * 1e-3) / 1e12
    total_fl = 0.0
    for lv in levels:
        for L in lv["layers"]:
            # useful FLOPs: a downsampling layer's strided convs at their minimal cost (what the strided kernels multiply since round 4)
            total_fl += sum(c.work(B, lv["H"], lv["H"])[0] for c in L["layer"].convs())
            total_fl += L["layer"].posterior.stack.step_work(B, lv["H"], lv["H"])["live_flops"]
    emit({
        "metric": ("CVAE1 forward samples/sec (tf_train.py:150-218: uint8 images -> x_enc -> up + down of every layer -> x_dec -> "
                   "discretized_logistic -> obj / loss)") if edge is not None else
                  "IAFLayer forward samples/sec (up + down of every layer: 4 plain weight-normed convs + IAF posterior block)",
        "value": n_gpus * B / (elapsed / args.steps), "unit": "samples/s", "n_gpus": n_gpus, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32" if args.precision == "f32" else "f32 (forward convs: operands split into 2 fp16 planes, 3 part-products on the fp16 MFMA in two fp32 accumulators: fp32-grade error, operands up to 65504)" if cv.runs_f16x2(B, 16, 16) else "f32 (forward convs: operands split into 3 bf16 parts, 6 part-products on the bf16 MFMA, fp32 accumulate: fp32-grade error; backward: exact fp32 MFMA)", "data": "synthetic",
        "config": {"workload": "cifar10 z_size=%d h_size=%d depths=%s depth_ar=%d bs=%d per GPU, kl_min=0.25: %d IAFLayers "
                               "(tf_train.py:23-95) as one connected model -- up pass 16x16 -> %dx%d through the downsampling "
                               "layer of each coarser level, then the down pass back"
                               % (zs, hs, depths, args.depth_ar, B, len(all_layers), Htop, Htop),
                   "global_batch": n_gpus * B, "launch": "hipGraph replay" if graph is not None else "eager",
                   "model_edges": None if edge is None else {"loss": float(edge["loss"].item()), "obj": float(edge["obj"].item()),
                                                             "bits_per_dim": float(edge["loss"].item()) / (np.log(2.) * 3072 * B)},
                   "weights": "re-derived every step (2 batched launches)" if not args.cached_weights else "prepared once",
                   "weight_packs_kept": packs_kept if packs_kept is not None else "all (--all-packs)",
                   "live_gflop_per_step": total_fl / 1e9,
                   "model_tflops": total_fl / (elapsed / args.steps) / 1e12,
                   "parallelism": "dp%d (batch-sharded replicas, no forward collective)" % n_gpus},
        # yardstick = the pipe the kernel runs on (see the headline line): 2500 / 6 TF for the bf16x3 kernels, 157.3 TF for exact fp32
        "roofline": {"bound": "mfma", "achieved": achieved, "unit": "TFLOP/s",
                     "peak": PEAK_BF16X3_TFLOPS if cv.runs_bf16x3(B, 16, 16) else PEAK_F32_MFMA_TFLOPS,
                     "frac": achieved / (PEAK_BF16X3_TFLOPS if cv.runs_bf16x3(B, 16, 16) else PEAK_F32_MFMA_TFLOPS), "traffic": None,
                     "frac_of_f32_mfma_peak": achieved / PEAK_F32_MFMA_TFLOPS,
                     "kernel": "%s<.., EPI_PLAIN, 9 taps> (down_conv1 %d->%d, B=%d 16x16)" % (
                         "iaf_conv_bf3_kernel" if cv.runs_bf16x3(B, 16, 16) else "iaf_conv_kernel", cv.n_in, cv.n_out, B),
                     "dominant_kernel_family": "f16x2" if cv.runs_f16x2(B, 16, 16) else "bf16x3" if cv.runs_bf16x3(B, 16, 16) else "f32",
                     "peak_note": "416.7 TF = 2500 / 6 (the bf16x3 yardstick) kept as the denominator for the two-plane fp16 launch too (3 part-products per fp32 product: own pipe 833.3 TF)",
                     "avg_launch_us": 1e3 * k_ms, "launches_timed": 50 * len(kt), "flops_per_launch": fl,
                     "bytes_per_launch": by, "hbm_frac_at_this_rate": (by / (k_ms * 1e-3) / 1e9) / PEAK_HBM_GBS,
                     "timing": "HIP events on the launch stream around 50 back-to-back launches per 16x16 layer"}})


def model_train_bench(args, depths, dist, rank, n_gpus):
    """One tower's training step of the WHOLE reference model (CVAE1, tf_train.py:114-218) from its own objective: every weight norm
    re-derived (batched launches), forward, obj = sum(kl_obj - log_pxz), backward of everything (iaf_amd.CVAE1.forward_backward:
    opt.compute_gradients(obj), tf_train.py:128) with the gradients written into ONE flat buffer laid out in the order the backward
    completes them (CVAE1.completion_order) and cut into --ar-buckets buckets (CVAE1.set_grad_buckets): each bucket's all-reduce(sum)
    over the ranks is issued right behind the backward segment that completes it and travels while the remaining segments run
    (tf_utils/common.py:83-86 on RCCL, parallel.OverlappedGradReduce), then the fused Adamax(1/N) + EMA on the flat parameter buffer
    (tf_utils/adamax.py:40-56, tf_train.py:146-159).  uint8 images and noise are synthetic, weights random-init."""
    import golden_inputs as gi
    import iaf_amd
    import iaf_amd.parallel as par
    if len(set(depths)) != 1:
        raise SystemExit("--train --model: the reference model has the same number of layers on every level (depth x num_blocks)")
    B, zs, hs, nb = args.batch, args.n_z, args.n_h, depths[0]
    gi.MODEL_CASES["bench"] = (B, 1, zs, hs, len(depths), nb, 32, 0.25)
    c = gi.model_case_inputs("bench")
    rng = np.random.RandomState(99 + rank)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    model = iaf_amd.CVAE1(z_size=zs, h_size=hs, kl_min=0.25, depth=len(depths), num_blocks=nb, k=1, image_size=32, depth_ar=args.depth_ar)
    for level in model.layers:
        for layer in level:
            layer.posterior.stack.set_precision(args.precision)
            for cvx in layer.convs():
                cvx.set_precision(args.precision)
    model.set_training(True)
    host = {k: dev(v) for k, v in c["params"].items()}
    model.load(host)                                       # (names only: the flat buffer is laid out in the model's completion order)
    flat = par.FlatParams({k: host[k] for k in model.completion_order()})
    model.load(flat.p)
    bucket_names = model.set_grad_buckets(args.ar_buckets)
    red = par.OverlappedGradReduce(flat, par.OverlappedGradReduce.bounds_from_groups(flat, bucket_names), force=force_dist(args))
    x = torch.from_numpy(rng.randint(0, 256, size=(B, 3, 32, 32)).astype(np.uint8)).cuda()
    noise = [dev(rng.standard_normal(e.shape)) for e in c["noise"]]
    keep, tune = {}, [False]

    def seg0():
        model.prepare_weights()
        keep["fb"] = model.fb_begin(x, noise, grads=flat.g, autotune=tune[0])
        model.fb_segment(0)

    segments = [seg0] + [(lambda i=i: model.fb_segment(i)) for i in range(1, len(bucket_names))]
    for sgm in segments:
        sgm()
    if not args.no_autotune:
        tune[0] = True                                     # launch-shape search of the plain convs and their data gradients (cuDNN's search)
        for sgm in segments:
            sgm()
        tune[0] = False
    for sgm in segments:
        sgm()
    torch.cuda.synchronize()
    obj0 = float(keep["fb"]["obj"].item())
    elapsed, graphed, exchange = _run_segmented(args, segments, red, flat, n_gpus, dist)
    obj1 = float(keep["fb"]["obj"].item())
    xerr = model.exchange_errors()                         # (a NaN objective with a non-zero count would be the hand-over, not the numerics)
    if rank != 0:
        return
    exchange["rccl"] = bool(red.comm is not None)
    exchange["halo_exchange_errors"] = xerr
    exchange["messages"] = len(bucket_names) if red.active else 0
    exchange["bytes"] = 4 * flat.params.numel()
    fwd_fl = 0.0
    for li, level in enumerate(model.layers):
        Hl = 16 >> li
        for layer in level:
            fwd_fl += sum(cv.work(B, Hl, Hl)[0] for cv in layer.convs())
            fwd_fl += layer.posterior.stack.step_work(B, Hl, Hl)["live_flops"]
    emit({
        "metric": "CVAE1 TRAIN-step samples/sec (whole model from its own objective: weight norms, forward, backward of every variable, "
                  "grad all-reduce, Adamax/EMA)",
        "value": n_gpus * B / (elapsed / args.steps), "unit": "samples/s", "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32" if args.precision == "f32" else "f32 (forward convs and most data gradients: operands split into 3 bf16 parts on the bf16 MFMA, fp32 accumulate; the rest exact fp32)",
        "data": "synthetic",
        "config": {"workload": "cifar10 z_size=%d h_size=%d depth=%d num_blocks=%d depth_ar=%d bs=%d per GPU, kl_min=0.25, k=1: CVAE1 "
                               "(tf_train.py:114-218), %d trainable fp32 parameters in %d tensors, one flat gradient buffer (%.1f MB)"
                               % (zs, hs, len(depths), nb, args.depth_ar, B, flat.params.numel(), len(flat.p), 4e-6 * flat.params.numel()),
                   "global_batch": n_gpus * B,
                   "launch": "hipGraph replay per gradient bucket, all-reduce behind each, then the update" if graphed else "eager",
                   "obj_first_step": obj0, "obj_last_step": obj1,
                   "bits_per_dim_last_step": obj1 / (np.log(2.) * 3072 * B),
                   "parallelism": "dp%d (RCCL all-reduce of %d gradient buckets, overlapped with backward)" % (n_gpus, len(bucket_names))},
        "roofline": _train_roofline(fwd_fl, 1e3 * elapsed / args.steps, "model"),
        "exchange": exchange})


def layers_train_bench(args, depths, dist, rank, n_gpus):
    """DP training step of whole IAFLayers (SURVEY 8f-4 + 8f-1,2): weight prep, up pass, down pass, backward of both
    passes (every plain conv and the posterior block), gradients written into ONE flat buffer laid out in the order the
    backward completes them (top-down-pass parameters layer by layer, then bottom-up-pass parameters in reverse), bucketed
    all-reduce(sum) over ranks overlapped with the remaining backward, fused Adamax(1/N)+EMA.  Synthetic upstream
    gradients (d output ~ N(0,1), d kl_obj = 1)."""
    import golden_inputs as gi
    import iaf_amd
    from iaf_amd import parallel as par
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    rng = np.random.RandomState(4321 + rank)
    wrng = np.random.RandomState(99)
    zs, hs, B = args.n_z, args.n_h, args.batch
    DOWN = (("down_conv1", (hs, 4 * zs + 2 * hs)), ("down_conv2", (hs + zs, hs)))
    UP = (("up_conv1", (hs, 2 * zs + 2 * hs)), ("up_conv3", (hs, hs)))
    host, levels = {}, []
    for lvl, nlayer in enumerate(depths):
        H = 16 >> lvl
        L = []
        for j in range(nlayer):
            pre = "IAF_%d_%d/" % (lvl, j)
            for nm, (ci, co) in UP + DOWN:
                for k, v in gi.conv_params(wrng, ci, co).items():
                    host[pre + nm + "/" + k] = v
            for k, v in gi.ar_multiconv2d_params(wrng, zs, [hs] * args.depth_ar, [zs, zs]).items():
                host[pre + "ar_multiconv2d/" + k] = v
            layer = iaf_amd.IAFLayer(zs, hs, depth_ar=args.depth_ar, kl_min=0.25)
            layer.posterior.stack.set_precision(args.precision)
            for cvx in layer.convs():
                cvx.set_precision(args.precision)
            layer.set_training(True)
            L.append(dict(layer=layer, pre=pre, eps=dev(rng.standard_normal((B, zs, H, H)))))
        f = lambda: dev(rng.standard_normal((B, hs, H, H)))
        levels.append(dict(H=H, layers=L, up_in=f(), down_in=f(), d_up=f(), d_down=f()))
    all_layers = [L for lv in levels for L in lv["layers"]]
    for lv in levels:
        for i, L in enumerate(lv["layers"]):
            L["lv"], L["first"], L["last"] = lv, i == 0, i == len(lv["layers"]) - 1
    # completion order of the gradients: down_backward visits levels / layers in forward order and finishes each
    # layer's down_conv1, down_conv2 and ar_multiconv2d; up_backward then runs in reverse and finishes up_conv1/3
    down_order = all_layers
    up_order = [L for lv in reversed(levels) for L in reversed(lv["layers"])]
    is_down = lambda k: ("/down_conv" in k) or ("/ar_multiconv2d/" in k)
    named = {}
    for L in down_order:
        for k, v in host.items():
            if k.startswith(L["pre"]) and is_down(k):
                named[k] = dev(v)
    for L in up_order:
        for k, v in host.items():
            if k.startswith(L["pre"]) and not is_down(k):
                named[k] = dev(v)
    flat = par.FlatParams(named)
    for L in all_layers:
        n = len(L["pre"])
        L["params"] = {k[n:]: v for k, v in flat.p.items() if k.startswith(L["pre"])}
        L["grads"] = {k[n:]: v for k, v in flat.g.items() if k.startswith(L["pre"])}
    nb = max(1, args.ar_buckets)
    dgroups = _chunks(down_order, (nb + 1) // 2)
    ugroups = _chunks(up_order, nb // 2) if nb >= 2 else []
    if not ugroups:                                       # a single bucket: everything completes at the very end
        names = [[k for k in named]]
    else:
        names = [[k for L in g for k in named if k.startswith(L["pre"]) and is_down(k)] for g in dgroups] + \
                [[k for L in g for k in named if k.startswith(L["pre"]) and not is_down(k)] for g in ugroups]
    red = par.OverlappedGradReduce(flat, par.OverlappedGradReduce.bounds_from_groups(flat, names),
                                   force=force_dist(args))
    prep_s = iaf_amd.PrepBatch([L["layer"].posterior.stack for L in all_layers])
    prep_c = iaf_amd.ConvPrepBatch([c for L in all_layers for c in L["layer"].convs()])
    splist = [iaf_amd.IAFLayer.stack_params(L["params"]) for L in all_layers]
    cplist = [t for L in all_layers for t in iaf_amd.IAFLayer.conv_params(L["params"])]
    dko = torch.ones(B, device="cuda")
    tup = lambda d, nm: (d[nm + "/V"], d[nm + "/g"], d[nm + "/b"])

    def wn_batch(group, down):
        """deferred mask + weight-norm backward of the parameters a segment completes"""
        convs = [getattr(L["layer"], nm) for L in group for nm, _ in (DOWN if down else UP)]
        stacks = [L["layer"].posterior.stack for L in group] if down else []
        w = iaf_amd.WnBwdBatch(stacks=stacks, convs=convs)
        cp = [tup(L["params"], nm) for L in group for nm, _ in (DOWN if down else UP)]
        cg = [tup(L["grads"], nm) for L in group for nm, _ in (DOWN if down else UP)]
        sp = [iaf_amd.IAFLayer.stack_params(L["params"]) for L in group] if down else []
        sg = [iaf_amd.IAFLayer.stack_params(L["grads"]) for L in group] if down else []
        return lambda: w.run(stack_params=sp, stack_grads=sg, conv_params=cp, conv_grads=cg)

    tune = [False]
    carry = {}

    def forward():
        prep_s.run(splist)
        prep_c.run(cplist)
        for lv in levels:
            h = lv["up_in"]
            for L in lv["layers"]:
                h = L["layer"].up_train(h, autotune=tune[0])
        for lv in reversed(levels):
            h = lv["down_in"]
            for L in reversed(lv["layers"]):
                h, _, _ = L["layer"].down_train(h, L["eps"], autotune=tune[0])

    def down_bwd(group):                                  # backward of the top-down pass, layer by layer
        for L in group:
            d = L["lv"]["d_down"] if L["first"] else carry["d"]
            carry["d"] = L["layer"].down_backward(d, dko, L["params"], L["grads"], autotune=tune[0])

    def up_bwd(group):                                    # backward of the bottom-up pass, in reverse
        for L in group:
            d = L["lv"]["d_up"] if L["last"] else carry["u"]
            carry["u"] = L["layer"].up_backward(d, L["params"], L["grads"], autotune=tune[0])

    segments = []
    if not ugroups:
        wd, wu = wn_batch(down_order, True), wn_batch(up_order, False)
        segments.append(lambda: (forward(), down_bwd(down_order), up_bwd(up_order), wd(), wu()))
    else:
        for gi_, g in enumerate(dgroups):
            w = wn_batch(g, True)
            segments.append((lambda g=g, w=w, first=(gi_ == 0): ((forward() if first else None), down_bwd(g), w())))
        for g in ugroups:
            w = wn_batch(g, False)
            segments.append((lambda g=g, w=w: (up_bwd(g), w())))

    # launch-shape search of the plain convs, forward and data gradient (cuDNN's autotune), before anything is captured
    for sgm in segments:
        sgm()
    tune[0] = True
    for sgm in segments:
        sgm()
    tune[0] = False
    torch.cuda.synchronize()
    elapsed, graphed, exchange = _run_segmented(args, segments, red, flat, n_gpus, dist)
    if rank == 0:
        fwd_fl = 0.0
        for lv in levels:
            for L in lv["layers"]:
                fwd_fl += sum(c.work(B, lv["H"], lv["H"])[0] for c in L["layer"].convs())
                fwd_fl += L["layer"].posterior.stack.step_work(B, lv["H"], lv["H"])["live_flops"]
        emit({
            "metric": "IAFLayer TRAIN-step samples/sec (forward + backward of every layer + grad all-reduce + Adamax/EMA)",
            "value": n_gpus * B / (elapsed / args.steps), "unit": "samples/s", "n_gpus": n_gpus, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32" if args.precision == "f32" else "f32 (forward convs: operands split into 3 bf16 parts, 6 part-products on the bf16 MFMA, fp32 accumulate: fp32-grade error; backward: exact fp32 MFMA)", "data": "synthetic",
            "config": {"workload": "cifar10 z_size=%d h_size=%d depths=%s depth_ar=%d bs=%d per GPU, kl_min=0.25: %d "
                                   "non-downsampling IAFLayers; %d trainable fp32 parameters in one flat gradient buffer (%.1f MB)"
                                   % (zs, hs, depths, args.depth_ar, B, len(all_layers), flat.params.numel(),
                                      4e-6 * flat.params.numel()),
                       "global_batch": n_gpus * B,
                       "launch": "hipGraph replay per gradient bucket, all-reduce behind each, then the update" if graphed else "eager",
                       "model_tflops_fwd_plus_bwd": 3.0 * fwd_fl / (elapsed / args.steps) / 1e12,
                       "parallelism": "dp%d (RCCL all-reduce of %d gradient buckets, overlapped with backward)" % (n_gpus, len(segments))},
            "roofline": _train_roofline(fwd_fl, 1e3 * elapsed / args.steps, "layers"),
            "exchange": exchange})


def iw_eval_bench(args, depths, dist, rank, n_gpus):
    """BASELINE configs[4]: importance-weighted ELBO evaluation, inference only.  One STEP = one pass of `--batch` (256)
    rows -- 256 images x 1 importance sample (the Theano driver's order, train.py:194-203) -- through the fused posterior
    block of every layer (10 at 16x16 + 10 at 8x8: sample, logqs, IAF step, log-det, logps, KL sums), the column sum of
    the per-layer KL costs (tf_train.py:198-200) and the update of the per-image running log-sum-exp
    (distributions.py:55-62 without ever materialising the [n, k] weights).  k = --iw-k passes complete one estimate;
    value = importance samples (rows) per second, config.images_per_s_at_k = value / k.  log p(x|z) comes from the
    decoder (out of scope): synthetic."""
    import iaf_amd
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    B = args.batch
    rng = np.random.RandomState(2468 + rank)
    wrng = np.random.RandomState(99)
    stacks, inputs = [], []
    for lvl, nlayer in enumerate(depths):
        H = 16 >> lvl
        for _ in range(nlayer):
            params, _, _ = make_layer_inputs(wrng, B, args.n_z, args.n_h, args.depth_ar, H)
            st = iaf_amd.ARStack(args.n_z, [args.n_h] * args.depth_ar)
            st.set_precision(args.precision)
            st.prepare({k: dev(v) for k, v in params.items()})
            f = lambda c, sc=1.0: dev(sc * rng.standard_normal((B, c, H, H)))
            inputs.append((f(args.n_z), f(args.n_z, 0.25), f(args.n_z), f(args.n_z, 0.25), f(args.n_z), f(args.n_z, 0.25),
                           f(args.n_h), f(args.n_h), f(args.n_z)))
            if not args.no_autotune and args.depth_ar > 0:
                st.autotune(inputs[-1][0], inputs[-1][6], reps=10)
            stacks.append(st)
    log_pxz = dev(-7000.0 + 30.0 * rng.standard_normal(B))
    ev = iaf_amd.IWEvaluator(stacks, kl_min=0.25)

    def one_pass():
        ev.run_pass(inputs, log_pxz)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    stream = torch.cuda.Stream()
    graph = None
    with torch.cuda.stream(stream):
        one_pass()
        stream.synchronize()
        if not args.no_graph:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                one_pass()
        run = graph.replay if graph is not None else one_pass
        for _ in range(args.warmup):
            run()
        barrier()
        # A fresh box starts with the GPU clocks down and the graph not yet resident: 5 warm-up replays of a 0.5 ms step
        # are 2.5 ms.  More untimed replays until the box has been busy for a while (the driver's
        # fresh box read 10 % under the builder's lease), then the timed region -- EXACTLY --steps steps between barrier +
        # synchronize on both sides -- is repeated and the MEDIAN repeat reported (all repeats listed in config.repeats_ms).
        t_settle = time.perf_counter()
        n_settle = 0
        while time.perf_counter() - t_settle < args.settle_seconds:
            for _ in range(max(args.steps, 1)):
                run()
            torch.cuda.synchronize()
            n_settle += max(args.steps, 1)
        repeats = []
        for _ in range(max(1, args.repeats)):
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run()
            barrier()
            repeats.append(time.perf_counter() - t0)
        elapsed = float(np.median(repeats))
        # dominant kernel: the n_h -> n_h masked conv at 16x16 with B rows
        dom = max(args.depth_ar - 1, 0)
        z16, c16 = inputs[0][0], inputs[0][6]
        k_ms = float(np.mean([stacks[i].time_layer(dom, z16, c16, reps=20) for i in range(min(3, depths[0]))]))
        if graph is not None:
            ev.state.k += args.warmup + args.steps      # replays folded passes into the device state behind Python's back
        bound = ev.result()
        torch.cuda.synchronize()
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank != 0:
        return
    lw = stacks[0].layer_work(dom, B, 16, 16)
    kern = stacks[0].layer_precision(dom, B, 16, 16)
    peak = PEAK_BF16X3_TFLOPS if kern == "bf16x3" else PEAK_F32_MFMA_TFLOPS      # the pipe the kernel runs on (see the headline line)
    ach = lw["live_flops"] / (k_ms * 1e-3) / 1e12
    step_fl = sum(d * stacks[0].step_work(B, 16 >> i, 16 >> i)["live_flops"] for i, d in enumerate(depths))
    rows_per_s = n_gpus * B / (elapsed / args.steps)
    emit({
        "metric": "IW-ELBO evaluation importance-samples/sec (posterior blocks of every layer + streaming log-sum-exp)",
        "value": rows_per_s, "unit": "samples/s", "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32" if args.precision == "f32" else "f32 (bf16x3 split-product MFMA where it wins, fp32 accumulate)",
        "data": "synthetic",
        "config": {"workload": "10000-sample importance-weighted ELBO eval, inference only (BASELINE configs[4]): cifar10 n_z=%d "
                               "n_h=%d depths=%s depth_ar=%d, %d rows per pass (= %d images x 1 sample), k = %d passes per estimate"
                               % (args.n_z, args.n_h, depths, args.depth_ar, B, B, args.iw_k),
                   "global_batch": n_gpus * B, "k": args.iw_k, "images_per_s_at_k": rows_per_s / args.iw_k,
                   "seconds_per_estimate_of_%d_images" % B: args.iw_k * elapsed / args.steps,
                   "launch": "hipGraph replay of one pass" if graph is not None else "eager",
                   "passes_folded_so_far": ev.k, "finite_bound": bool(torch.isfinite(bound).all().item()),
                   "model_tflops": step_fl / (elapsed / args.steps) / 1e12,
                   "parallelism": "dp%d (images sharded over ranks, no collective)" % n_gpus},
        "roofline": {"bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "traffic": None,
                     "frac_of_f32_mfma_peak": ach / PEAK_F32_MFMA_TFLOPS, "dominant_kernel_family": kern,
                     "kernel": "masked 3x3 conv %d->%d, B=%d 16x16" % (args.n_h, args.n_h, B), "avg_launch_us": 1e3 * k_ms,
                     "flops_per_launch_live": lw["live_flops"], "bytes_per_launch": lw["bytes"],
                     "step": {"live_flops_per_step": step_fl, "frac_of_f32_mfma_peak": step_fl / (elapsed / args.steps) / 1e12 / PEAK_F32_MFMA_TFLOPS}}})


def iw_eval_model_bench(args, depths, dist, rank, n_gpus):
    """BASELINE configs[4] at MODEL level: the k-sample importance-weighted bound of the whole CVAE1 (tf_train.py:168-170,218 with
    hps.k = --iw-k), streamed: the bottom-up pass (image scaling, x_enc, every layer's up_conv1 / up_conv3) depends on x only and runs
    ONCE per image block (CVAE1.iw_eval keeps its products across the passes); one STEP = one importance sample of every image of the
    block = one top-down pass (h_top, every layer's down_conv1 / posterior block / down_conv2, x_dec, likelihood) + the update of the
    running log-sum-exp.  Reported beside it: the same pass with the bottom-up pass recomputed (= k x forward, what round 4 ran)."""
    import golden_inputs as gi
    import iaf_amd
    from iaf_amd.distributions import StreamingLowerBound
    if len(set(depths)) != 1:
        raise SystemExit("--iw-eval --model: the reference model has the same number of layers on every level")
    B, zs, hs, nb = args.batch, args.n_z, args.n_h, depths[0]
    gi.MODEL_CASES["bench"] = (B, 1, zs, hs, len(depths), nb, 32, 0.25)
    c = gi.model_case_inputs("bench")
    rng = np.random.RandomState(2468 + rank)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    model = iaf_amd.CVAE1(z_size=zs, h_size=hs, kl_min=0.25, depth=len(depths), num_blocks=nb, k=1, image_size=32, depth_ar=args.depth_ar)
    for level in model.layers:
        for layer in level:
            layer.posterior.stack.set_precision(args.precision)
            for cvx in layer.convs():
                cvx.set_precision(args.precision)
    model.load({k: dev(v) for k, v in c["params"].items()})
    x = torch.from_numpy(rng.randint(0, 256, size=(B, 3, 32, 32)).astype(np.uint8)).cuda()
    noise = [dev(rng.standard_normal(e.shape)) for e in c["noise"]]
    acc = StreamingLowerBound(B, x.device)
    keep = {}

    def bottom_up():
        keep["xf"] = model._bottom_up(x, noise)

    def one_pass():
        log_pxz, kl_cost = model._top_down(keep["xf"], B, noise, terms=True)
        acc.update(log_pxz.reshape(B, 1), kl_cost.reshape(B, 1))

    passes_run = [0]

    def full_pass():                                       # round 4's form: the whole forward per sample
        bottom_up()
        one_pass()

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, updates=False):
        graph = None
        fn()
        n_run = 1                                          # passes that reached the device accumulators (a capture does not execute)
        torch.cuda.current_stream().synchronize()
        if not args.no_graph:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=torch.cuda.current_stream()):
                fn()
        run = graph.replay if graph is not None else fn
        for _ in range(args.warmup):
            run()
        n_run += args.warmup + max(1, args.repeats) * args.steps
        if updates:
            passes_run[0] += n_run
        reps = []
        for _ in range(max(1, args.repeats)):
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run()
            barrier()
            reps.append(time.perf_counter() - t0)
        return float(np.median(reps)), graph is not None

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        bottom_up()
        stream.synchronize()
        t_up, _ = timed(bottom_up)
        t_full, _ = timed(full_pass, updates=True)
        elapsed, graphed = timed(one_pass, updates=True)
        # (graph replays update the device accumulators, the host-side count only saw the eager call and the capture:
        #  the bound's log k comes from the passes that actually ran)
        acc.k = passes_run[0]
        bound = acc.result()
        torch.cuda.synchronize()
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank != 0:
        return
    rows_per_s = n_gpus * B / (elapsed / args.steps)
    emit({
        "metric": "CVAE1 IW-ELBO evaluation importance-samples/sec (whole model, bottom-up pass once per image block, streaming log-sum-exp)",
        "value": rows_per_s, "unit": "samples/s", "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32" if args.precision == "f32" else "f32 (bf16x3 split-product MFMA where it wins, fp32 accumulate)",
        "data": "synthetic",
        "config": {"workload": "10000-sample importance-weighted ELBO eval of the whole model, inference only (BASELINE configs[4]): cifar10 "
                               "z_size=%d h_size=%d depth=%d num_blocks=%d depth_ar=%d, %d images per block, one sample of each per pass, "
                               "k = %d passes per estimate" % (zs, hs, len(depths), nb, args.depth_ar, B, args.iw_k),
                   "global_batch": n_gpus * B, "k": args.iw_k, "images_per_s_at_k": rows_per_s / args.iw_k,
                   "ms_per_pass_top_down_only": 1e3 * elapsed / args.steps,
                   "ms_per_pass_with_the_bottom_up_pass_recomputed": 1e3 * t_full / args.steps,
                   "ms_bottom_up_pass_once_per_block": 1e3 * t_up / args.steps,
                   "speedup_vs_k_times_forward": t_full / elapsed,
                   "seconds_per_estimate_of_%d_images" % B: (args.iw_k * elapsed + t_up) / args.steps,
                   "launch": "hipGraph replay of one pass" if graphed else "eager",
                   "finite_bound": bool(torch.isfinite(bound).all().item()),
                   "parallelism": "dp%d (images sharded over ranks, no collective)" % n_gpus}})


def quick_modes(args, depths, xunit):
    """VERDICT r05 "next" #3a: the widened workloads measured in the SAME run as the headline, each a short in-process
    run of the mode's own code path (`bench.py --train --model`, `--layers --model`, `--iw-eval --model`; 3 timed steps behind 2 warm-up
    steps, no process group, no CPU baseline) -- so that the driver's default run sees them.  None of these is `value`."""
    import copy
    res = {"note": "quick in-process runs of the other modes (3 timed steps each); the full lines: python bench.py --train --model | "
                   "--layers --model | --iw-eval --model"}
    for pb in xunit:
        res["posterior_block_us_%s" % pb["latent"]] = pb["us"]

    def run(fn, **over):
        a2 = copy.copy(args)
        a2.steps, a2.warmup, a2.repeats, a2.settle_seconds, a2.no_cpu_baseline, a2._no_dist = 3, 2, 1, 0.0, True, True
        for k, v in over.items():
            setattr(a2, k, v)
        CAPTURE[0] = []
        t0 = time.perf_counter()
        try:
            fn(a2, depths, None, 0, 1)
            got = CAPTURE[0][0] if CAPTURE[0] else None
        except BaseException as e:          # noqa: BLE001  (SystemExit included: a mode that refuses this configuration)
            got = {"error": "%s: %s" % (type(e).__name__, (str(e).splitlines() or [""])[0][:200])}
        finally:
            CAPTURE[0] = None
        torch.cuda.synchronize()
        return got, time.perf_counter() - t0

    got, dt = run(model_train_bench, train=True, model=True)
    if got is not None:
        res["train_model_ms"] = got.get("ms_per_step", got.get("error"))
        if "roofline" in got:
            res["train_model_frac"] = got["roofline"].get("frac")
        res["train_model_wall_s"] = dt
    got, dt = run(layers_bench, layers=True, model=True)
    if got is not None:
        res["model_fwd_ms"] = got.get("ms_per_step", got.get("error"))
        if "config" in got:
            res["model_fwd_tflops"] = got["config"].get("model_tflops")
        res["model_fwd_wall_s"] = dt
    got, dt = run(iw_eval_model_bench, iw_eval=True, model=True, batch=256, iw_k=8)
    if got is not None:
        res["iw_eval_ms_per_pass"] = (got.get("config") or {}).get("ms_per_pass", got.get("ms_per_step", got.get("error")))
        res["iw_eval_wall_s"] = dt
    return res


def _halo_note(st, R, args):
    """how many MACs the one-launch step issues per live MAC: hidden layer l is computed on R + depth_ar - l rows per R
    output rows (iaf_step_fused.hpp) -- or on its R own rows where the row blocks exchange their halo rows; roofline figures
    count the live ones only"""
    d = args.depth_ar
    if st.step_exchanges(args.batch, 16, 16):
        return ("the row blocks of an image exchange their halo rows through device memory (agent-scope accesses): every hidden "
                "layer is computed on the %d rows its workgroup owns, none twice" % R)
    live = [st.layer_work(l, args.batch, 16, 16)["live_flops"] for l in range(d + 1)]
    issued = sum(live[l] * (R + d - l) / R for l in range(d)) + live[d]
    return "the launch multiplies %.2fx the live MACs (halo rows of the hidden layers recomputed per %d-row workgroup); only live MACs are counted" % (
        issued / sum(live), R)


def _tri_skipped(nht, npair):
    """(co tile, centre-tap step) units a channel-triangular hidden layer of the one-launch step neither loads nor multiplies
    (iaf_step_fused.hpp, tri_live): tile slot j of wave w holds tile 4j + w (odd j: 4(j+1) - 1 - w), the left-over tiles are never
    dead; a slot is skipped at input pair c when c > t // 2 for the tiles t of every wave of its group (waves {0,1}, {2,3} when
    two tiles are left over, else all four)"""
    nfull, nx = nht // 4, nht % 4
    gn = 4 // nx if nx and 4 % nx == 0 else 1
    skipped = 0
    for gi in range(gn):
        waves = range(gi * (4 // gn), (gi + 1) * (4 // gn))
        for j in range(nfull):
            tiles = [4 * (j + 1) - 1 - w if j & 1 else 4 * j + w for w in waves]
            for c in range(npair):
                if all(c > t // 2 for t in tiles):
                    skipped += len(tiles)
    return skipped


def _issued_over_live(args, R, W):
    """fp32-equivalent FLOPs the one-launch step's MFMAs multiply per live FLOP: per row block, hidden layer l on
    ceil((R + depth_ar - l) * W / 16) pixel tiles, the output pair on ceil(R * W / 16), every co tile x every (32-channel,
    tap) step of the 5 stored taps -- 16 x 16 x 32 MACs each (iaf_step_fused.hpp), less the dead centre-tap blocks the
    triangular hidden layers skip (_tri_skipped) -- against the mask-aware live count"""
    d, nz, nh = args.depth_ar, args.n_z, args.n_h
    H = W
    nrb = (H + R - 1) // R
    units = 0
    cin = nz
    import iaf_amd
    st = iaf_amd.ARStack(nz, [nh] * d)
    xch = st.step_exchanges(args.batch, H, W)          # halo rows imported from the block below instead of recomputed
    for l in range(d):
        per_tile = (nh // 16) * (cin // 32) * 5
        if l >= 1 and getattr(args, "variant", "tf") == "tf":
            per_tile -= _tri_skipped(nh // 16, cin // 32)
        units += -(-((R if xch else R + d - l) * W) // 16) * per_tile
        cin = nh
    units += -(-(R * W) // 16) * (2 * nz // 16) * (cin // 32) * 5
    issued = float(args.batch * nrb * units) * 16 * 16 * 32 * 2
    return issued / st.step_work(args.batch, H, W)["live_flops"]


def main():
    args = parse()
    depths = [int(d) for d in args.depths.split(",") if d]
    dist, rank, n_gpus, rank_info = init_ranks(args)
    RANK_INFO.update(rank_info)

    import iaf_amd
    iaf_amd._capi.lib()           # fail loudly if the HIP engine is not built
    if args.iw_eval:
        if args.batch == 32:
            args.batch = 256              # configs[4]: bs = 256
        (iw_eval_model_bench if args.model else iw_eval_bench)(args, depths, dist, rank, n_gpus)
        if dist is not None:
            dist.destroy_process_group()
        return
    if args.model and args.train:
        model_train_bench(args, depths, dist, rank, n_gpus)
        if dist is not None:
            dist.destroy_process_group()
        return
    if args.layers and args.train:
        layers_train_bench(args, depths, dist, rank, n_gpus)
        if dist is not None:
            dist.destroy_process_group()
        return
    if args.layers:
        layers_bench(args, depths, dist, rank, n_gpus)
        if dist is not None:
            dist.destroy_process_group()
        return
    if args.train:
        train_bench(args, depths, dist, rank, n_gpus)
        if dist is not None:
            dist.destroy_process_group()
        return
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    # ---------------- build the layer schedule (every rank its own data: seed + rank)
    rng = np.random.RandomState(1234 + rank)
    layers = []
    for lvl, nlayer in enumerate(depths):
        H = 16 >> lvl
        for _ in range(nlayer):
            params, z, ctx = make_layer_inputs(rng, args.batch, args.n_z, args.n_h, args.depth_ar, H)
            st = iaf_amd.ARStack(args.n_z, [args.n_h] * args.depth_ar)
            dp = {k: dev(v) for k, v in params.items()}
            zd, cd = dev(z), dev(ctx)
            out = (torch.empty_like(zd), torch.empty_like(zd))
            st.set_precision(args.precision)
            if args.no_fuse:
                st.set_fuse_first("never")
            if args.no_fuse_step:
                st.set_fuse_step("never")
            st.prepare(dp)
            layers.append(dict(stack=st, params=dp, z=zd, ctx=cd, out=out, H=H, one=st.step_is_fused(args.batch, H, H)))
    if args.tune:
        for item in args.tune.split(";"):
            lay, shp = item.split(":")
            nt, pxt, wco, ks = [int(v) for v in shp.split(",")]
            for L in layers:
                L["stack"].set_tuning(int(lay), nt, pxt, wco, ks)

    # every IAF step of this workload runs as ONE bf16x3 launch: the prep launch need not keep the fp32 fragment pack up to
    # date (iaf_stack_set_packs; a launch that needed it would fail loudly, not read stale weights)
    bf3_only = (not args.keep_f32_pack) and args.precision in ("bf16x3", "f16x2") and all(L["one"] for L in layers)
    # ... and where every one of them is a two-plane fp16 kernel, not the bf16x3 pack either (4 B per weight instead of 6 + 4)
    f16_all = args.precision == "f16x2" and all(L["stack"].step_is_f16(args.batch, L["H"], L["H"]) for L in layers)
    f16_only = bf3_only and f16_all
    if bf3_only:
        for L in layers:
            L["stack"].set_packs(f32=False, bf16x3=not f16_only, f16x2=f16_only)
            L["stack"].prepare(L["params"])
    prep = iaf_amd.PrepBatch([L["stack"] for L in layers])
    plist = [L["params"] for L in layers]
    tuned = {}
    if not args.no_autotune and not args.tune and args.depth_ar > 0:
        # kernel family + launch shape per layer, measured on this box for this size (the cuDNN algorithm search of the
        # reference's convs); outside the timed region, before the graph is captured
        for L in layers:
            if L["one"]:             # the step runs as ONE launch at this size: no per-layer kernels to choose between
                tuned.setdefault("%dx%d" % (L["H"], L["H"]), ["whole step in one launch (%d rows per workgroup)" % L["one"]])
                continue
            picks = L["stack"].autotune(L["z"], L["ctx"], reps=20)
            L["fused"] = picks[0][0] == "fused into next"
            tuned.setdefault("%dx%d" % (L["H"], L["H"]), [c for c, _ in picks])

    def step():
        if not args.cached_weights:
            prep.run(plist)      # mask*V, l2-normalise, exp(g), repack (layers.py:56-60): all 20 layers, one launch
        for L in layers:
            L["stack"].iaf_step(L["z"], L["ctx"] if args.depth_ar > 0 else None, out=L["out"])

    stream = torch.cuda.Stream()
    graph = None
    with torch.cuda.stream(stream):
        step()                                                   # allocate workspaces, warm caches
        stream.synchronize()
        # the halo exchange between the row blocks of the 16x16 step waits with a bound; should a wait ever give up on this box,
        # fall back to the recomputing kernel for the whole run (and say so) rather than time garbage
        for _ in range(3):
            step()
        stream.synchronize()
        if any(L["stack"].exchange_errors() for L in layers):
            for L in layers:
                L["stack"].set_halo_exchange(False)
            RANK_INFO["halo_exchange"] = "disabled: a bounded wait gave up during warm-up"
            step()
            stream.synchronize()
        if not args.no_graph:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                step()
        run = graph.replay if graph is not None else step

        def barrier():
            torch.cuda.synchronize()
            if dist is not None:
                dist.barrier()
            torch.cuda.synchronize()

        for _ in range(args.warmup):
            run()
        barrier()
        # A fresh box starts with the GPU clocks down and the graph not yet resident: 5 warm-up replays of a 0.5 ms step
        # are 2.5 ms.  More untimed replays until the box has been busy for a while (the driver's
        # fresh box read 10 % under the builder's lease), then the timed region -- EXACTLY --steps steps between barrier +
        # synchronize on both sides -- is repeated and the MEDIAN repeat reported (all repeats listed in config.repeats_ms).
        t_settle = time.perf_counter()
        n_settle = 0
        while time.perf_counter() - t_settle < args.settle_seconds:
            for _ in range(max(args.steps, 1)):
                run()
            torch.cuda.synchronize()
            n_settle += max(args.steps, 1)
        repeats = []
        for _ in range(max(1, args.repeats)):
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run()
            barrier()
            repeats.append(time.perf_counter() - t0)
        elapsed = float(np.median(repeats))
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, layers)      # before the kernel leg below launches these layers again

        # ---------------- kernel leg: eager steps, HIP events around every launch of the dominant kernel
        # IN SITU per launch (VERDICT r03 "next" #5: a relaunched layer meets its 0.8-1.2 MB of weight packs L2-hot and reads
        # 1-2 us short of the launch it is inside the step): the launches of ONE latent level -- its 10 layers, every one with its
        # own packs and inputs, in the step's order -- captured as a graph and replayed between ONE HIP event pair on the launch
        # stream; per launch = elapsed / launches (includes the ~1.2 us gap between two launches of a graph, like the step itself:
        # 10 x 16x16 + 10 x 8x8 + the prep launch add up to ms_per_step).  profiles/ holds the rocprofv3 average of the kernel alone.
        dom_layer = max(args.depth_ar - 1, 0)                    # the n_h -> n_h masked conv (layer 1 at depth_ar=2)
        prof = [L for L in layers if L["H"] == 16]
        one16 = bool(prof) and all(L["one"] for L in prof)       # the 16x16 steps run as ONE launch each: that is the kernel
        insitu_ms, insitu_n = {}, {}
        for H in sorted({L["H"] for L in layers if L["one"]}, reverse=True):
            lv = [L for L in layers if L["H"] == H]
            if not all(L["one"] for L in lv):
                continue

            def level(lv=lv):
                for L in lv:
                    L["stack"].iaf_step(L["z"], L["ctx"], out=L["out"])
            level()
            stream.synchronize()
            lrun = level
            if not args.no_graph:
                lg = torch.cuda.CUDAGraph()
                with torch.cuda.graph(lg, stream=stream):
                    level()
                lrun = lg.replay
            for _ in range(20):
                lrun()
            stream.synchronize()
            rounds = []
            for _ in range(5):
                ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ea.record(stream)
                for _ in range(30):
                    lrun()
                eb.record(stream)
                eb.synchronize()
                rounds.append(ea.elapsed_time(eb) / (30 * len(lv)))
            insitu_ms[H], insitu_n[H] = float(np.median(rounds)), 5 * 30 * len(lv)
        # primary figure: N back-to-back launches of the dominant kernel between ONE event pair (no per-launch
        # event/dispatch latency), averaged over the 16x16 layers
        fused16 = (not one16) and dom_layer == 1 and bool(prof) and all(L.get("fused") for L in prof)     # every 16x16 stack tuned to the fused launch
        tl_med = lambda st_, lay, z_, c_: float(np.median([st_.time_layer(lay, z_, c_, reps=50) for _ in range(5)]))
        if one16:
            kbatch = [tl_med(L["stack"], -2, L["z"], L["ctx"]) for L in prof]
        else:
            kbatch = [L["stack"].time_layer(-1 if fused16 else dom_layer, L["z"], L["ctx"] if args.depth_ar > 0 else None, reps=50)
                      for L in prof if fused16 or not L.get("fused")] or \
                     [L["stack"].time_layer(-1, L["z"], L["ctx"], reps=50) for L in prof]
        # every GEMM layer of the IAF step at every latent level, same method (first layer of each level), and the
        # extended unit of SURVEY 8d (posterior block: sample + logqs + IAF step + log-det + logps + KL / free bits)
        ktable, xunit = [], []
        for lvl, nlayer in enumerate(depths):
            if nlayer == 0:
                continue
            H = 16 >> lvl
            L = [x for x in layers if x["H"] == H][0]
            st = L["stack"]
            cin = args.n_z
            fused = bool(L.get("fused"))
            if L["one"]:
                hot_ms = tl_med(st, -2, L["z"], L["ctx"])
                ms = insitu_ms.get(H, hot_ms)
                w = st.step_work(args.batch, H, H)
                tf_ = w["live_flops"] / (ms * 1e-3) / 1e12
                ktable.append({"layer": "IAF step: masked convs %d->%d%s->%d (mean,logsd pair) + affine/log-det, ONE launch, %d rows per workgroup"
                                        % (args.n_z, args.n_h, "->%d" % args.n_h if args.depth_ar > 1 else "", 2 * args.n_z, L["one"]),
                               "latent": "%dx%d" % (H, H), "kernel": "f16x2" if st.step_is_f16(args.batch, H, H) else "bf16x3",
                               "us": 1e3 * ms, "live_gflop": w["live_flops"] / 1e9,
                               "live_tflops": tf_, "frac": tf_ / PEAK_BF16X3_TFLOPS, "frac_of_f32_mfma_peak": tf_ / PEAK_F32_MFMA_TFLOPS,
                               "us_method": ("in situ: the level's %d launches (every layer its own packs and inputs) replayed as a graph "
                                             "between one event pair, %d launches, gaps included" % (len([x for x in layers if x["H"] == H]), insitu_n[H]))
                                            if H in insitu_ms else "relaunched layer",
                               "us_relaunched_hot": 1e3 * hot_ms,
                               # MFMA work issued per live FLOP (half-filled 16-pixel tiles and recomputed halo rows at 8-pixel rows)
                               "issued_over_live": _issued_over_live(args, L["one"], H)})
            for gl in range(args.depth_ar + 1) if not L["one"] else ():
                cout = args.n_h if gl < args.depth_ar else 2 * args.n_z
                name = "masked conv %d->%d%s" % (cin, cout, " (mean,logsd pair + affine/log-det epilogue)" if gl == args.depth_ar else "")
                w = st.layer_work(gl, args.batch, H, H)
                cin = args.n_h
                if fused and gl == 0:
                    w0 = w
                    continue                      # computed inside the next launch
                if fused and gl == 1:
                    ms = st.time_layer(-1, L["z"], L["ctx"], reps=50)
                    w = {k: w[k] + w0[k] for k in w}
                    name = "masked conv %d->%d + %s, ONE launch (first layer fused into the prologue)" % (args.n_z, args.n_h, name)
                    kern = "bf16x3"
                else:
                    ms = st.time_layer(gl, L["z"], L["ctx"] if args.depth_ar > 0 else None, reps=50)
                    kern = st.layer_precision(gl, args.batch, H, H)
                tf_ = w["live_flops"] / (ms * 1e-3) / 1e12
                ktable.append({"layer": name, "latent": "%dx%d" % (H, H), "kernel": kern, "us": 1e3 * ms,
                               "live_gflop": w["live_flops"] / 1e9, "live_tflops": tf_,
                               "frac": tf_ / (PEAK_BF16X3_TFLOPS if kern == "bf16x3" else PEAK_F32_MFMA_TFLOPS),
                               "frac_of_f32_mfma_peak": tf_ / PEAK_F32_MFMA_TFLOPS, "us_method": "relaunched layer (50 back-to-back launches)"})
            if args.depth_ar > 0:
                # extended unit: the posterior block with pre-allocated outputs, XREP calls captured once
                # and replayed -- the way a model runs it -- so that the figure reads the kernels and not the host's launch
                # rate or the allocator (30 eager calls after 3 warm-ups read 1.3 ms on a fresh box)
                f = lambda c, sc=1.0: sc * torch.randn(args.batch, c, H, H, device="cuda")
                pin = [f(args.n_z), f(args.n_z, 0.25), f(args.n_z), f(args.n_z, 0.25), f(args.n_z), f(args.n_z, 0.25),
                       f(args.n_h), f(args.n_h), f(args.n_z)]
                pout = dict(z=torch.empty_like(pin[0]), kl_obj=torch.empty(args.batch, device="cuda"),
                            kl_cost=torch.empty(args.batch, device="cuda"))
                XREP = 30
                for _ in range(3):
                    st.posterior_block(*pin, 0.25, out=pout)
                stream.synchronize()
                xg = None
                if not args.no_graph:
                    xg = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(xg, stream=stream):
                        for _ in range(XREP):
                            st.posterior_block(*pin, 0.25, out=pout)

                def xrun():
                    if xg is not None:
                        xg.replay()
                    else:
                        for _ in range(XREP):
                            st.posterior_block(*pin, 0.25, out=pout)
                for _ in range(10):
                    xrun()
                stream.synchronize()
                xs = []
                for _ in range(5):
                    ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ea.record(stream)
                    xrun()
                    eb.record(stream)
                    eb.synchronize()
                    xs.append(1e3 * ea.elapsed_time(eb) / XREP)
                us = float(np.median(xs))
                sw = st.step_work(args.batch, H, H)
                xunit.append({"latent": "%dx%d" % (H, H), "us": us, "samples_per_s": args.batch / (us * 1e-6),
                              "live_tflops": sw["live_flops"] / (us * 1e-6) / 1e12,
                              "frac": sw["live_flops"] / (us * 1e-6) / 1e12 / (PEAK_BF16X3_TFLOPS if args.precision != "f32" else PEAK_F32_MFMA_TFLOPS),
                              "frac_of_f32_mfma_peak": sw["live_flops"] / (us * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS,
                              "repeats_us": xs,
                              "launches": st.posterior_block_launches(args.batch, H, H),
                              "timing": "%d calls with pre-allocated outputs %s, 10 warm-up rounds, median of 5 rounds between HIP events"
                                        % (XREP, "captured in one hipGraph and replayed" if xg is not None else "issued eagerly")})

    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    ms_per_step = 1e3 * elapsed / args.steps
    value = n_gpus * args.batch / (elapsed / args.steps)
    n_iaf = sum(depths)

    st0 = prof[0]["stack"]
    lw = st0.layer_work(dom_layer, args.batch, 16, 16)
    if one16:                        # the launch is the whole step: its live flops and the step's algorithmic bytes
        lw = st0.step_work(args.batch, 16, 16)
    if fused16:                      # the launch also computes the first masked conv (on tile + halo): count its useful work once
        lw0 = st0.layer_work(0, args.batch, 16, 16)
        lw = {"live_flops": lw["live_flops"] + lw0["live_flops"], "dense_flops": lw["dense_flops"] + lw0["dense_flops"],
              "bytes": lw["bytes"] + lw0["bytes"] - 2.0 * 4.0 * args.batch * args.n_h * 256}   # its output never reaches HBM
    k_hot_ms = float(np.mean(kbatch))                           # a layer relaunched 50 times: packs and inputs L2-hot
    k_avg_ms = insitu_ms[16] if (one16 and 16 in insitu_ms) else k_hot_ms       # in situ (see the kernel leg above)
    achieved = lw["live_flops"] / (k_avg_ms * 1e-3) / 1e12
    traffic = None
    pmc = os.path.join(ROOT, "profiles", "pmc_dominant_kernel.json")
    if os.path.exists(pmc):
        try:
            traffic = json.load(open(pmc)).get("hbm_bytes_per_launch")
        except Exception:
            traffic = None
    dom_f16 = one16 and st0.step_is_f16(args.batch, 16, 16)
    dom_kernel = ("f16x2" if dom_f16 else "bf16x3") if one16 else st0.layer_precision(dom_layer, args.batch, 16, 16)
    pipe_peak = PEAK_BF16X3_TFLOPS if dom_kernel in ("bf16x3", "f16x2") else PEAK_F32_MFMA_TFLOPS
    roofline = {
        # yardstick = the pipe the kernel's instruction stream runs on (VERDICT r03 "next" #5).  bf16x3 kernels issue
        # v_mfma_f32_16x16x32_bf16: dense bf16 peak 2500 TF / 6 part-products per fp32 product = 416.7 TF of fp32-grade live FLOPs.
        # The exact-fp32 kernels (--precision f32) issue v_mfma_f32_16x16x4_f32: 157.3 TF.  The fp32 figure SURVEY 8d names is
        # kept next to it (frac_of_f32_mfma_peak): config 3's n_h = 192 already exceeds it, so it can no longer rank kernels.
        "bound": "mfma", "achieved": achieved, "peak": pipe_peak, "unit": "TFLOP/s",
        "frac": achieved / pipe_peak, "traffic": traffic,
        "peak_note": ("dense bf16 MFMA peak 2500 TF / 6 bf16 part-products per fp32 product" if dom_kernel == "bf16x3" else
                      "416.7 TF = dense 16-bit MFMA peak 2500 TF / 6: the bf16x3 yardstick of rounds 4-5, KEPT as the denominator (VERDICT r05 "
                      "'next' #1) although this kernel issues 3 fp16 part-products per fp32 product -- against its own pipe "
                      "(2500 / 3 = 833.3 TF) see frac_of_own_pipe" if dom_kernel == "f16x2" else
                      "dense fp32 MFMA peak (v_mfma_f32_16x16x4_f32)"),
        "frac_of_f32_mfma_peak": achieved / PEAK_F32_MFMA_TFLOPS, "peak_f32_mfma": PEAK_F32_MFMA_TFLOPS,
        "dominant_kernel_family": dom_kernel,
        "frac_of_own_pipe": achieved / (PEAK_BF16_MFMA_TFLOPS / 3.0) if dom_kernel == "f16x2" else achieved / pipe_peak,
        # how many MACs the launch ISSUES per live MAC (halo rows of the hidden layers recomputed per row block where they are
        # not exchanged, partially filled pixel tiles, dead centre-tap blocks multiplied as stored zeros)
        "issued_over_live": _issued_over_live(args, prof[0]["one"], 16) if one16 else 1.0,
        "kernel": ("iaf_step_fused_kernel (one IAF step = masked 3x3 convs %d->%d%s->%d + affine/log-det in ONE launch, B=%d 16x16)"
                   % (args.n_z, args.n_h, "->%d" % args.n_h if args.depth_ar > 1 else "", 2 * args.n_z, args.batch)) if one16 else
                  ("iaf_conv_bf3_kernel<IN_FUSED0> (masked 3x3 convs %d->%d and %d->%d in ONE launch, B=%d 16x16)" % (args.n_z, args.n_h, args.n_h, args.n_h, args.batch)) if fused16 else
                  "%s (masked 3x3 conv %d->%d, B=%d 16x16, GEMM layer %d)" % ("iaf_conv_bf3_kernel" if dom_kernel == "bf16x3" else "iaf_conv_kernel", args.n_h, args.n_h, args.batch, dom_layer),
        "avg_launch_us": 1e3 * k_avg_ms, "launches_timed": insitu_n[16] if (one16 and 16 in insitu_ms) else 50 * len(kbatch),
        "timing": ("IN SITU: the ten 16x16 launches of the step (ten layers, each with its own weight packs and inputs, none of them "
                   "in any L2 when its launch starts) captured as one graph and replayed between one HIP event pair on the launch "
                   "stream, median of 5 rounds of 30 replays, per launch = elapsed / launches (the ~1.2 us gap between launches "
                   "included, as in ms_per_step); the same layer relaunched 50 times back to back (packs L2-hot) reads %.2f us"
                   % (1e3 * k_hot_ms)) if (one16 and 16 in insitu_ms) else
                  "HIP events on the launch stream around 50 back-to-back launches per 16x16 layer (includes the inter-launch gap)",
        "avg_launch_us_relaunched_hot": 1e3 * k_hot_ms,
        "flops_per_launch_live": lw["live_flops"], "flops_per_launch_dense9tap": lw["dense_flops"],
        "halo_recompute": _halo_note(st0, prof[0]["one"], args) if one16 else None,
        "bytes_per_launch": lw["bytes"],
        "hbm_frac_at_this_rate": (lw["bytes"] / (k_avg_ms * 1e-3) / 1e9) / PEAK_HBM_GBS,
    }
    work16 = st0.step_work(args.batch, 16, 16)
    step_flops = sum(d * st0.step_work(args.batch, 16 >> i, 16 >> i)["live_flops"] for i, d in enumerate(depths))
    step_tf = step_flops / (ms_per_step * 1e-3) / 1e12
    roofline["step"] = {"live_flops_per_step": step_flops, "ms_per_step": ms_per_step, "achieved": step_tf,
                        "frac": step_tf / pipe_peak, "frac_of_f32_mfma_peak": step_tf / PEAK_F32_MFMA_TFLOPS,
                        "note": "the whole timed step (weight prep + every conv launch + gaps) against the same peak"}
    roofline["kernels"] = ktable
    roofline["extended_unit"] = xunit
    # the halo exchange between the row blocks of the 16x16 step waits with a bound: a wait that gave up would have produced garbage
    xerrs = sum(L["stack"].exchange_errors() for L in layers)
    if xerrs:
        raise RuntimeError("one-launch IAF step: %d halo-exchange wait(s) gave up (iaf_stack_exchange_errors)" % xerrs)
    # ... and an operand beyond fp16's range in a two-plane fp16 kernel would have produced inf / NaN
    if any(L["stack"].range_errors() for L in layers):
        raise RuntimeError("one-launch IAF step (f16x2): an operand beyond fp16's range (iaf_stack_range_errors)")
    rp = os.path.join(ROOT, "profiles", "rocprof_dominant_kernel.json")
    if os.path.exists(rp):
        try:
            rj = json.load(open(rp))
            roofline["rocprof"] = {"avg_launch_us": rj.get("avg_launch_us"), "source": rj.get("source"),
                                   "frac": lw["live_flops"] / (rj["avg_launch_us"] * 1e-6) / 1e12 / pipe_peak,
                                   "frac_of_f32_mfma_peak": lw["live_flops"] / (rj["avg_launch_us"] * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS}
        except Exception:
            pass
    out = {
        "metric": "IAF-step samples/sec (down_iaf2_nl posterior stack, forward + log-det)",
        "value": value, "unit": "samples/s", "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32" if args.precision == "f32" else
                 "f32 (operands split into 2 fp16 planes hi + lo 2^-11, 3 part-products on the fp16 MFMA in two fp32 accumulators: fp32-grade error, "
                 "operands up to 65504)" if f16_all else
                 "f32 (operands split into 3 bf16 parts, 6 part-products on the bf16 MFMA, fp32 accumulate: fp32-grade error)",
        "data": "synthetic",
        "config": {
            "workload": "cifar10 n_z=%d n_h=%d depths=%s depth_ar=%d down_iaf2_nl bs=%d per GPU (BASELINE configs[1]); "
                        "one step = %d IAF steps: %s" % (args.n_z, args.n_h, depths, args.depth_ar, args.batch, n_iaf,
                                                        " + ".join("%d x [%d,%d,%d,%d]" % (d, args.batch, args.n_z, 16 >> i, 16 >> i)
                                                                   for i, d in enumerate(depths))),
            "global_batch": n_gpus * args.batch, "iaf_steps_per_step": n_iaf,
            "iaf_step_samples_per_s": value * n_iaf,
            "weights": ("re-derived every step (mask, l2-norm, exp(g)) for all layers in one batched launch" + (
                            "; two-plane fp16 packs only (no launch of this workload reads another)" if f16_only else
                            "; bf16x3 packs only (no launch of this workload reads the fp32 pack)" if bf3_only else "")) if not args.cached_weights else "prepared once",
            "launch": "hipGraph replay" if graph is not None else "eager",
            "parallelism": "dp%d (batch-sharded replicas, no forward collective)" % n_gpus,
            "live_gflop_per_iaf_step_16x16": work16["live_flops"] / 1e9,
            "precision": args.precision,
            "kernels_chosen": tuned if tuned else "static rule (no autotune)",
            "repeats_ms": [1e3 * r / args.steps for r in repeats],
            # which levels of the one-launch step hand their halo rows from row block to row block instead of recomputing them
            "halo_exchange": sorted({"%dx%d" % (L["H"], L["H"]) for L in layers if L["stack"].step_exchanges(args.batch, L["H"], L["H"])}),
            "timing": "median of %d repeats of the timed region (%d steps each, barrier + synchronize on both sides); %d untimed "
                      "settle replays after the %d warm-up steps" % (len(repeats), args.steps, n_settle, args.warmup),
            "settle_replays": n_settle,
        },
        "roofline": roofline,
    }
    if n_gpus == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args, depths)
        out["config"]["gpu_over_cpu"] = value / out["cpu_baseline"]["value"]
    if n_gpus == 1 and not args.no_modes and dist is None:
        out["modes"] = quick_modes(args, depths, xunit)
    emit(out)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
