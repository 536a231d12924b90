"""TrainStep -- one data-parallel training step of CVAE1 (tf_train.py:124-159) with a guard: the update is applied only if the
step's all-reduced gradients and objective are finite.

The step is the one bench.py --train --model times: every weight norm re-derived (CVAE1.prepare_weights), forward and backward
(CVAE1.fb_begin / fb_segment) into ONE flat gradient buffer laid out in completion order (parallel.FlatParams), bucket i's
all-reduce(sum) issued behind backward segment i (parallel.OverlappedGradReduce), the join, then
  - the guard scan (iaf_nonfinite_scan) of the reduced flat gradient and of a status word that went through the same reduce (the
    sum of the ranks' objectives: one rank's non-finite objective makes it non-finite on every rank), and
  - the gated Adamax / EMA (iaf_adamax_ema_step_guarded, grad_scale 1/world; 1/(world * towers) for a model with towers): bit-identical to FlatParams.adamax_ema_step when
    the guard is clear; when it is raised nothing moves and a counter in mapped host memory counts the skip.
Every rank scans the same reduced numbers, so every rank takes the same decision.  A skipped batch is dropped (as
torch.amp.GradScaler does), not recomputed.

Why a step goes non-finite on a model the fp32 reference trains through: an operand beyond 65504 in a launch on two fp16 planes
(the default arithmetic of the one-launch step and the forward convs) makes that launch's outputs inf / NaN; its stack or conv
raises a range word, and only its NEXT eager call reports IAF_ERR_RANGE and moves it to bf16 planes (include/iaf_hip.h).  A
replayed hipGraph runs no host code and would keep the fp16-plane launch forever.  So at the first call after the host has seen
the skip counter rise, every object whose range word is newly set is moved through that existing protocol (compute-only eager
passes on the call's inputs, no collective, no update) and the graph is captured again on the same stream; from then on the
step runs where it did not overflow."""
import ctypes
import inspect
import math

import torch
import torch.distributed as dist

from . import _capi, _recover
from ._recover import SWITCHED as _SWITCHED, range_objects as _range_objects      # (read from outside under these names)
from .layers import check_groups
from .parallel import FlatParams, OverlappedGradReduce


class _SkipCounter(object):
    """iaf_skip_counter_t: the number of updates the gated kernel skipped, in mapped host memory"""

    def __init__(self):
        self._own = _capi.Handle("iaf_skip_counter_create")
        self._h = self._own.h

    def read(self):
        """the count as far as the device has got (no synchronisation)"""
        c = ctypes.c_uint()
        _capi.check(_capi.lib().iaf_skip_counter_read(self._h, ctypes.byref(c)))
        return c.value

    def counter_ptr(self):
        """the count's device address (what a state snapshot copies)"""
        return _capi.counter_address("iaf_skip_counter_ptr", self._h)


class TrainStep(object):
    """ts = TrainStep(model, lr); obj = ts(x, noise) per batch (ts(x) with a noise_source, ts() with a dataset as well).

    model: a CVAE1 after set_training(True) and load(params).  The constructor lays its variables out in ONE flat buffer in
    model.completion_order() (ts.flat: params, grads, slots, EMA; the model is re-loaded with the views of ts.flat.p), cuts the
    backward into `n_buckets` gradient buckets (model.set_grad_buckets) and sets up their all-reduce (through `comm`, a
    parallel.RcclComm, when one is given; else torch.distributed's default group when it has more than one rank).
    lr, beta1, beta2, eps, ema_decay: Adamax and the EMA (tf_utils/adamax.py:40-56, tf_train.py:146-159).
    graph=True captures the whole step as one hipGraph on a stream of its own (segments, forked all-reduces, join, scan, gated
    update); if the runtime refuses the capture, the step runs as eager launches (ts.graph_refused says why).

    ts(x, noise) enqueues one step on the current stream and returns the device objective [1] (graph mode: x and noise are first
    copied into the graph's static inputs -- same shapes every call -- and the returned tensor is overwritten by the next step).
    It does not synchronise.  ts.flat.g holds the step's all-reduced gradients afterwards.  ts.skipped synchronises and returns the
    number of skipped updates so far.

    noise_source (a NoiseSource; device parameters only): ts(x) draws the step's posterior noise itself -- one launch into buffers the
    step owns, the FIRST launch of the step, in graph mode inside the captured graph (the source's step counter lives in device memory:
    every replay draws fresh noise and no launch or copy precedes the graph).  Call t (t = 0, 1, ...) uses step s0 + t of the source,
    s0 being where the source stood at the first call, whatever was skipped or captured again: the compute-only passes (warm-up,
    recovery) run on what the buffers hold and never advance the source.  ts(x, noise) with a list still works: that call runs as eager
    launches on the list and moves the source on by one like any other call.

    data (a DeviceDataset; device parameters only) with batch_size: ts() takes no batch -- the step gathers its own, one launch into a
    uint8 [batch_size,3,S,S] buffer the step owns, the FIRST launch of the step (in front of the noise draw), in graph mode inside the
    captured graph: nothing is copied into the graph's inputs before a replay, and a replay trains on the next shuffled batch.  The rules
    are the noise source's: the buffer is filled once WITHOUT advancing the dataset when it is created, the compute-only passes run on
    what it holds, and call t trains on step s0 + t of the dataset whatever was skipped or captured again.  ts(x) with an explicit batch
    still works: that call runs as eager launches on x and moves the dataset on by one.  Without a noise_source, ts(noise=list).  The
    dataset is built with this rank's rank and the step's world.

    summaries=True: the step also produces the numbers the reference loop fetches and logs (tf_train.py:142, 148-149, 203-204,
    214-216, 268-285) -- with launches of the step itself (in graph mode inside the captured graph) that accumulate in device memory,
    so no step waits for the host.  The model's fb_begin must take terms=True and return "terms" (CVAE1 does), and the model needs
    image_size.  The local loss travels in the status word's second slot through the all-reduce the objective already makes.
    ts.summaries(reset=True) synchronises and returns the means over the accepted steps since the last reset (NaN when there were
    none) under the reference's tags -- model/bits_per_dim, model/dec_log_stdv, model/log_pxz, model/kl_obj, model/kl_cost,
    model/kl_obj_%02d_%02d, model/kl_cost_%02d_%02d -- plus grad_norm (the norm of the averaged gradient), steps and skipped;
    ts.last_summaries() the same keys for the most recent step alone, accepted or not.

    A model with towers (model.towers = N > 1, CVAE1(towers=N)): this rank's batch holds N of the reference's towers, so the update and
    grad_norm use 1/(world * N) where they use 1/world otherwise (average_grads over all towers); model/bits_per_dim already counts every
    row (tf_train.py:142).  Deviation: the reference logs its KL and log_pxz summaries from the LAST tower only (tf_train.py:202, 213);
    here they are means over all rows."""

    _FIXED = ("model/bits_per_dim", "model/dec_log_stdv", "model/log_pxz", "model/kl_obj", "model/kl_cost", "grad_norm")

    def __init__(self, model, lr, n_buckets=1, comm=None, graph=True, beta1=0.9, beta2=0.999, eps=1e-8, ema_decay=0.999,
                 noise_source=None, summaries=False, data=None, batch_size=None):
        if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not math.isfinite(lr) or lr <= 0:
            raise ValueError("lr must be a positive finite number, got %r" % (lr,))
        if not _capi.int_in(n_buckets, 1):
            raise ValueError("n_buckets must be a positive int, got %r" % (n_buckets,))
        if not isinstance(graph, bool):
            raise ValueError("graph must be True or False, got %r" % (graph,))
        for nm, v in (("beta1", beta1), ("beta2", beta2), ("ema_decay", ema_decay)):
            if not (isinstance(v, (int, float)) and 0.0 <= v < 1.0):
                raise ValueError("%s must lie in [0, 1), got %r" % (nm, v))
        if not (isinstance(eps, (int, float)) and math.isfinite(eps) and eps >= 0):
            raise ValueError("eps must be a finite number >= 0, got %r" % (eps,))
        if not isinstance(summaries, bool):
            raise ValueError("summaries must be True or False, got %r" % (summaries,))
        if data is not None:
            from .data import DeviceDataset
            if not isinstance(data, DeviceDataset):
                raise ValueError("data must be a DeviceDataset, got %r" % (data,))
            if not _capi.int_in(batch_size, 1):
                raise ValueError("TrainStep(data=): batch_size must be a positive int, got %r" % (batch_size,))
            data.batches_per_epoch(batch_size)          # (ValueError: a global batch larger than the dataset)
        elif batch_size is not None:
            raise ValueError("TrainStep: batch_size goes with data=")
        if getattr(model, "params", None) is None:
            raise RuntimeError("TrainStep: model.set_training(True), then model.load(params), first")
        if summaries:
            try:
                takes = "terms" in inspect.signature(model.fb_begin).parameters
            except (TypeError, ValueError):
                takes = False
            if not takes:
                raise ValueError("TrainStep(summaries=True): the model's fb_begin takes no terms= (it cannot say what the summaries are made of)")
            if not isinstance(getattr(model, "image_size", None), int) or model.image_size < 1:
                raise ValueError("TrainStep(summaries=True): the model needs image_size (bits per dim are per pixel)")
            if "dec_log_stdv" not in model.params:
                raise ValueError("TrainStep(summaries=True): the model has no dec_log_stdv variable")
        self.model, self.lr = model, float(lr)
        self._hyper = (float(beta1), float(beta2), float(eps), float(ema_decay))
        self.flat = FlatParams({k: model.params[k] for k in model.completion_order()})
        self.on_device = self.flat.params.is_cuda
        if graph and not self.on_device:
            raise ValueError("TrainStep: graph=True needs device parameters")
        if noise_source is not None and not self.on_device:
            raise ValueError("TrainStep: noise_source needs device parameters (host replicas take their noise from the caller)")
        if data is not None and not self.on_device:
            raise ValueError("TrainStep: data needs device parameters (host replicas take their batches from the caller)")
        self.noise_source = noise_source
        self.data, self.batch_size = data, batch_size
        self._xb = None                   # the batch buffer a dataset fills
        self._drawn = None                # the posterior noise buffers a source fills (forward()'s layout, None in the prior slots)
        model.load(self.flat.p)
        names = model.set_grad_buckets(n_buckets)
        self.n_buckets = len(names)
        self.red = OverlappedGradReduce(self.flat, OverlappedGradReduce.bounds_from_groups(self.flat, names), force=comm is not None,
                                        comm=comm)
        self.world = 1
        if self.red.active:
            self.world = int(getattr(self.red.comm, "world", 0) or dist.get_world_size())
        if data is not None and data.world != self.world:
            raise ValueError("TrainStep: the dataset was built for a world of %d, the step has %d" % (data.world, self.world))
        # the reference's towers inside this rank's batch (CVAE1(towers=N), tf_train.py:124-147): the gradients are sums over world * towers
        # towers, which average_grads divides by their number
        self.towers = check_groups(getattr(model, "towers", 1), "model.towers")
        self._replicas = self.world * self.towers
        dev = self.flat.params.device
        # [0]: the step's objective, summed over the ranks by the same exchange as the gradients (the rest: 16-byte padding)
        self._status = torch.zeros(4, dtype=torch.float32, device=dev)
        if self.on_device:
            self._guard = torch.zeros(4, dtype=torch.int32, device=dev)
            self._skips = _SkipCounter()
        self._host_skips = 0
        self.steps = 0                    # __call__s so far (a restore sets it to the saved run's)
        self._skip_base = 0               # what a restore adds to the skip counter: the saved run's skips
        self._acted = 0                   # the count at the last recovery
        self._aborted = False             # an eager step could not finish on this rank (an object switched kernels in the middle)
        self._seen = set()                # range objects already moved to bf16 planes
        self._objects = _range_objects(model)
        self.use_graph = graph
        self.graph_refused = None
        self.captures = 0
        self._graph = None
        self._static = None
        self._static_gathers = False      # the captured step begins with the dataset's gather
        self._stale = False               # the captured graph must be captured again before its next replay
        self._stream = torch.cuda.Stream(device=dev) if graph else None
        self.with_summaries = summaries
        self._terms = None                # the step's terms (fb_begin(terms=True)["terms"]); the captured graph reads these very tensors
        self._rec = None                  # the record: device memory (iaf_train_summaries), or a dict of host fp64 arrays

    # -- the step's launches ------------------------------------------------------------------------------------------------------
    def _compute(self, x, noise):
        """forward and backward only: no collective, no update (the passes that move objects whose range word is set)"""
        self.model.prepare_weights()
        self._begin(x, noise)
        for i in range(self.n_buckets):
            self.model.fb_segment(i)

    def _begin(self, x, noise):
        """fb_begin; with summaries also the step's terms, the local loss into the status word's second slot and, the first time, the
        record (a compute-only pass precedes every capture, so the record is never allocated or zeroed inside one)"""
        if not self.with_summaries:
            return self.model.fb_begin(x, noise, grads=self.flat.g)
        fb = self.model.fb_begin(x, noise, grads=self.flat.g, terms=True)
        if "terms" not in fb:
            raise ValueError("TrainStep(summaries=True): the model's fb_begin returned no \"terms\"")
        self._set_terms(fb["terms"])
        self._status[1:2].copy_(self._terms["loss"].reshape(1))
        return fb

    def _enqueue(self, x, noise, draw=False, gather=False):
        """one whole step on the current stream; returns the objective.  gather: `x` is the step's own batch buffer, and the step's first
        launch fills it from the dataset (one step of the dataset).  draw: `noise` is the step's own buffer set, and the launch behind
        that fills it from the noise source (one step of the source)"""
        m, red, flat = self.model, self.red, self.flat
        sent, status_sent = 0, False
        if gather:
            self.data.next_batch(self.batch_size, out=x)
        if draw:
            m.draw_noise(int(x.shape[0]), self.noise_source, which="posterior", out=noise)
        try:
            m.prepare_weights()
            obj = self._begin(x, noise)["obj"]
            self._status[:1].copy_(obj.reshape(1))
            red.reduce_tensor(self._status)
            status_sent = True
            for i in range(self.n_buckets):
                m.fb_segment(i)
                red.reduce(i)
                sent = i + 1
        except _SWITCHED:
            if self.on_device and torch.cuda.is_current_stream_capturing():
                raise
            # An object reported a failed EARLIER launch and switched kernels: this rank cannot finish the step's compute.  Every rank
            # still issues the same collectives, and every rank must skip: the buckets not yet sent (and the status, if not yet sent)
            # go out as NaN.  The next call moves what else needs moving before it enqueues anything.
            self._aborted = True
            if not status_sent:
                self._status.fill_(float("nan"))
                red.reduce_tensor(self._status)
            flat.grads[red.bounds[sent][0]:].fill_(float("nan"))
            for i in range(sent, self.n_buckets):
                red.reduce(i)
            obj = torch.full((1,), float("nan"), dtype=torch.float32, device=flat.params.device)
        red.wait()
        self._update()
        return obj

    def _set_terms(self, terms):
        """keep the step's terms and, at the first step, make the record for their geometry (nl layers, n batch rows)"""
        lo, lc, lp = terms["layer_obj"], terms["layer_cost"], terms["log_pxz"]
        nl, n = int(lo.shape[0]), int(lo.shape[1])
        if tuple(lc.shape) != (nl, n) or lp.numel() != n or len(terms["layers"]) != nl or terms["loss"].numel() != 1:
            raise ValueError("TrainStep: terms must hold layer_obj / layer_cost [nl, n], log_pxz [n], loss [1] and nl (i, j) pairs")
        self._terms = terms
        if self._rec is not None:
            if (nl, n) != self._geom:
                raise ValueError("TrainStep(summaries=True): the batch size and the layers must stay those of the first step")
            return
        self._geom = (nl, n)
        self._tags = list(self._FIXED)
        for (i, j) in terms["layers"]:
            self._tags += ["model/kl_obj_%02d_%02d" % (i, j), "model/kl_cost_%02d_%02d" % (i, j)]
        F = 6 + 2 * nl
        if self.on_device:
            lib, dev = _capi.lib(), self.flat.params.device
            nbytes = int(lib.iaf_train_summaries_bytes(nl))
            if nbytes != (2 * F + 2) * 8:
                raise ValueError("TrainStep(summaries=True): %d layers are more than the record holds" % nl)
            # (allocated outside any capture's pool by the warm-up pass that precedes every capture; zeroed by torch, no launch of ours)
            self._rec = torch.zeros(2 * F + 2, dtype=torch.float64, device=dev)
            self._partials = torch.zeros(2048, dtype=torch.float64, device=dev)
            self._sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        else:
            self._rec = dict(acc=torch.zeros(F, dtype=torch.float64), last=torch.zeros(F, dtype=torch.float64), steps=0, skipped=0)

    def _host_fields(self):
        """the record's fields of this step with torch fp64 ops (host replicas)"""
        t, f64 = self._terms, torch.float64
        lo, lc = t["layer_obj"].to(f64).mean(dim=1), t["layer_cost"].to(f64).mean(dim=1)
        norm = (1.0 / self._replicas) * torch.sqrt((self.flat.grads.to(f64) ** 2).sum())
        head = [self._status[1].to(f64), self.model.params["dec_log_stdv"].reshape(-1)[0].to(f64), -t["log_pxz"].to(f64).mean(), lo.sum(),
                lc.sum(), norm]
        return torch.cat([torch.stack(head), torch.stack([lo, lc], dim=1).reshape(-1)])

    def _update(self):
        flat, (b1, b2, eps, decay) = self.flat, self._hyper
        summ = self.with_summaries and self._terms is not None      # (no terms: the very first step could not finish its compute)
        if self.on_device:
            lib, ptr, st = _capi.lib(), _capi.ptr, _capi.stream()
            if summ:
                t, (nl, n) = self._terms, self._geom
                _capi.check(lib.iaf_nonfinite_scan_sumsq(ptr(flat.grads), flat.grads.numel(), ptr(self._status), 1, ptr(self._guard),
                                                         ptr(self._partials), ptr(self._sumsq), st))
                _capi.check(lib.iaf_train_summaries(ptr(t["layer_obj"]), ptr(t["layer_cost"]), ptr(t["log_pxz"]),
                                                    ptr(self.model.params["dec_log_stdv"]), ctypes.c_void_p(self._status.data_ptr() + 4),
                                                    ptr(self._sumsq), 1.0 / self._replicas, ptr(self._guard), ptr(self._rec), nl, n, st))
            else:
                _capi.check(lib.iaf_nonfinite_scan(ptr(flat.grads), flat.grads.numel(), ptr(self._status), 1, ptr(self._guard), st))
            _capi.check(lib.iaf_adamax_ema_step_guarded(ptr(flat.params), ptr(flat.grads), ptr(flat.slot_m), ptr(flat.slot_v),
                                                        ptr(flat.ema), flat.params.numel(), self.lr, b1, b2, eps, decay,
                                                        1.0 / self._replicas, ptr(self._guard), self._skips._h, st))
            # (raw-pointer writes: tell torch, as FlatParams.adamax_ema_step does)
            torch.autograd.graph.increment_version((flat.params, flat.ema, flat.slot_m, flat.slot_v))
        else:        # host replicas: the same decision with torch ops
            ok = bool(torch.isfinite(flat.grads).all()) and bool(torch.isfinite(self._status[:1]).all())
            if summ:
                rec = self._rec
                rec["last"] = self._host_fields()
                if ok:
                    rec["acc"] = rec["acc"] + rec["last"]
                    rec["steps"] += 1
                else:
                    rec["skipped"] += 1
            if ok:
                flat.adamax_ema_step(self.lr, world=self._replicas, beta1=b1, beta2=b2, eps=eps, ema_decay=decay)
            else:
                self._host_skips += 1

    # -- recovery after a skip --------------------------------------------------------------------------------------------------
    def _count(self):
        return self._skips.read() if self.on_device else self._host_skips

    def _must_move(self):
        """True if objects must be moved to bf16 planes (and the graph captured again) before this call's step"""
        if not self._aborted and self._count() <= self._acted:
            return False
        if self.on_device:
            torch.cuda.synchronize()
        self._acted = self._count()
        new = _recover.newly_flagged(self._objects, self._seen)
        moved, self._aborted = self._aborted or bool(new), False
        return moved

    def _move(self, x, noise):
        """compute-only eager passes on (x, noise) until the objects that switch kernels have settled (_recover.settle)"""
        _recover.settle(lambda: self._compute(x, noise), len(self._objects), "TrainStep", self.on_device)

    def _capture(self):
        self._graph = None
        x, noise = self._static
        done = _recover.capture(self, self._stream, lambda: self._move(x, noise),
                                [lambda: self._enqueue(x, noise, draw=self.noise_source is not None, gather=self._static_gathers)],
                                "TrainStep", "the step", stacklevel=4)
        if done is not None:
            (self._graph,), (self._sobj,) = done
            self.captures += 1

    # -- public ---------------------------------------------------------------------------------------------------------------------
    def _own_noise(self, x):
        """the buffer set a noise source fills for batches like x; filled once WITHOUT advancing the source when it is created, so that a
        compute-only pass before the first step has noise to run on"""
        B = int(x.shape[0])
        if self._drawn is None or int(self._drawn[1].shape[0]) != B:
            self._drawn = self.model.draw_noise(B, self.noise_source, which="posterior", advance=False)
        return self._drawn

    def _own_batch(self):
        """the batch buffer the dataset fills; filled once WITHOUT advancing the dataset when it is created, so that a compute-only pass
        before the first step has a batch to run on"""
        if self._xb is None:
            self._xb = self.data.next_batch(self.batch_size, advance=False)
        return self._xb

    def __call__(self, x=None, noise=None):
        obj = self._step(x, noise)
        self.steps += 1
        return obj

    def _step(self, x, noise):
        src, data = self.noise_source, self.data
        if x is None and data is None:
            raise ValueError("TrainStep: pass the step's batch, or build the step with data=")
        if noise is None and src is None:
            raise ValueError("TrainStep: pass the step's noise list, or build the step with noise_source=")
        draw, gather = noise is None, x is None
        if gather:
            x = self._own_batch()
        moved = self._must_move() or self._stale
        self._stale = False
        # (a step built with a source captures the draw into its graph: a call that brings its own list runs as eager launches; so does
        #  a call that brings its own batch to a step built with a dataset)
        if self.use_graph and self.graph_refused is None and (draw or src is None) and (gather or data is None):
            if self._static is None:
                self._static = (x if gather else x.clone(),
                                self._own_noise(x) if draw else [None if e is None else e.clone() for e in noise])
                self._static_gathers = gather
                moved = True
            else:
                sx, sn = self._static
                if x.shape != sx.shape or x.dtype != sx.dtype:
                    raise ValueError("TrainStep(graph=True): x and noise must keep the shapes of the first call")
                if not draw and (len(noise) != len(sn) or any((a is None) != (b is None) or (a is not None and a.shape != b.shape) for a, b in zip(noise, sn))):
                    raise ValueError("TrainStep(graph=True): x and noise must keep the shapes of the first call")
                if not gather:
                    sx.copy_(x)
                if not draw:
                    for a, b in zip(sn, noise):
                        if a is not None:           # (a slot the model does not read may be None, as CVAE1.forward allows)
                            a.copy_(b)
            if moved:
                self._capture()
            if self._graph is not None:
                self._graph.replay()
                return self._sobj
        if draw:
            noise = self._own_noise(x)
        if moved:
            self._move(x, noise)
            self._stale = self._graph is not None        # objects switched kernels outside the graph: capture it again before its next replay
        obj = self._enqueue(x, noise, draw=draw, gather=gather)
        if src is not None and not draw:
            src.skip(1)
        if data is not None and not gather:
            data.skip(1)
        return obj

    @property
    def skipped(self):
        """the number of updates skipped so far (synchronises the device); after a restore, the saved run's count plus this step's own"""
        if self.on_device:
            torch.cuda.synchronize()
        return self._skip_base + self._count()

    @property
    def global_step(self):
        """steps - skipped: the updates applied so far, the reference's global_step (synchronises the device)"""
        return self.steps - self.skipped

    # -- checkpoints (iaf_amd/checkpoint.py) ---------------------------------------------------------------------------------------------
    def snapshot(self, into=None):
        """snap = ts.snapshot(): ONE launch on the current stream (iaf_state_snapshot) copies ts.flat's variables, slots and EMA into
        staging buffers the Snapshot owns, the noise source's and the dataset's step and the skip count into its header tensor, and leaves
        a digest of each; an event follows.  Reads only, does not synchronise, copies nothing to the host; not while the current stream
        captures (RuntimeError).  into=: an earlier Snapshot of the same size, reused.  Host replicas: tensor clones, the numpy digest.
        snap.save(path) writes the file."""
        from . import checkpoint
        return checkpoint.take_snapshot(self, into)

    def restore(self, ck_or_path):
        """Continue the run a checkpoint was saved from (a Checkpoint or a path), before the first step or between two steps: the
        variables' names, shapes and order, world, towers and -- with a dataset -- batch_size and the dataset's size must be this step's
        (ValueError names the first difference); lr, betas, eps and ema_decay stay this step's.  The arrays are checked by their digests
        ON THE DEVICE before ts.flat is touched (IafHipError), then copied into ts.flat in place; the noise source and the dataset are
        sought to the saved steps; ts.steps and ts.skipped continue the saved counts; the stacks and convs the saved run had moved to bf16
        planes are moved here.  The summaries record starts as after summaries(reset=True).  Synchronises."""
        from . import checkpoint
        return checkpoint.restore(self, ck_or_path)

    def _reset_record(self):
        """the summaries record as after summaries(reset=True) (nothing to do before the first step has made one)"""
        if not self.with_summaries or self._rec is None:
            return
        if self.on_device:
            _capi.check(_capi.lib().iaf_train_summaries_reset(_capi.ptr(self._rec), self._geom[0], _capi.stream()))
        else:
            self._rec.update(acc=torch.zeros_like(self._rec["acc"]), last=torch.zeros_like(self._rec["last"]), steps=0, skipped=0)

    # -- summaries ------------------------------------------------------------------------------------------------------------------
    def _read_record(self):
        """(acc, last, steps, skipped) on the host, after everything enqueued so far has run"""
        if not self.with_summaries:
            raise RuntimeError("TrainStep: built without summaries=True")
        if self._rec is None:
            return None
        if not self.on_device:
            r = self._rec
            return r["acc"].numpy().copy(), r["last"].numpy().copy(), r["steps"], r["skipped"]
        torch.cuda.current_stream().synchronize()
        if self._stream is not None:
            self._stream.synchronize()
        F = 6 + 2 * self._geom[0]
        host = self._rec.cpu()
        counts = host[2 * F:].view(torch.int64)
        return host[:F].numpy().copy(), host[F:2 * F].numpy().copy(), int(counts[0]), int(counts[1])

    def _as_dict(self, fields, steps, skipped):
        S, n = self.model.image_size, self._geom[1]
        vals = [float(v) for v in fields]
        vals[0] = vals[0] / (math.log(2.) * 3 * S * S * n * self.world)            # tf_train.py:142
        out = dict(zip(self._tags, vals))
        out["steps"], out["skipped"] = steps, skipped
        return out

    def summaries(self, reset=True):
        """the means over the accepted steps since the last reset (NaN with steps == 0), steps and skipped; synchronises.  reset=True
        then zeroes the record with a stream-ordered launch (outside any capture): the whole record, `last` included, so read
        last_summaries() before a resetting call if the most recent step's numbers are wanted."""
        rec = self._read_record()
        if rec is None:
            raise RuntimeError("TrainStep.summaries: no step has run yet")
        acc, _, steps, skipped = rec
        mean = acc / steps if steps else acc * float("nan")
        if reset:
            self._reset_record()
        return self._as_dict(mean, steps, skipped)

    def last_summaries(self):
        """the same keys for the most recent step alone, accepted or skipped (steps / skipped: the record's counts); synchronises.  After
        summaries(reset=True) and before the next step every value is 0: the reset zeroes the whole record."""
        rec = self._read_record()
        if rec is None:
            raise RuntimeError("TrainStep.last_summaries: no step has run yet")
        _, last, steps, skipped = rec
        return self._as_dict(last, steps, skipped)

    @property
    def graphed(self):
        """True if the steps replay a captured hipGraph"""
        return self._graph is not None

    def ema_params(self):
        """the EMA of the variables (tf_train.py:157-158) as name -> view into ts.flat.ema, the names and shapes of model.params: load a
        second CVAE1 of the same geometry from it ONCE (eval_model.load(ts.ema_params()); the reference's Saver(model.avg_dict),
        tf_train.py:297) and every later EvalPass.run() evaluates the average as it stands, without a copy"""
        return self.flat.e
