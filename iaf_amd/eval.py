"""EvalPass -- the reference's test-set evaluation (tf_train.py:293-327, run_eval) on the device: the whole set walked once in
batches of `batch_size`, every batch scored with the k-sample importance-weighted bound (hps.k; k = 1: the plain bound), and
eval_bits_per_dim = the mean over the batches.  The reference restores the EMA of the variables for it (Saver(model.avg_dict),
:297): load the model from TrainStep.ema_params().

A batch is one HEAD -- the dataset's gather, the image scaling, x_enc and every layer's up pass (CVAE1._bottom_up, which depends
on the images only) -- followed by k PASSES: one draw of posterior noise, the top-down pass up to x_dec, and iaf_eval_tail
(include/iaf_hip.h), the one launch that turns x_out and the layers' kl_cost into the row's importance weight, streams it into the
running log-sum-exp and, on the k-th pass, closes the batch into a 32-byte device record.  The dataset's and the source's step
counters and the record's pass counter live in device memory, so head and pass are captured ONCE each (two hipGraphs without
parallel branches) and a batch is 1 + k replays; the host reads nothing until the epoch's last launch has run."""
import math
import warnings

import torch

from . import _capi, _recover
from ._capi import ptr as _ptr, stream as _stream
from .data import MAX_BATCH, DeviceDataset
from .images import image_grid
from .model import CVAE1
from .noise import NoiseSource

BINSIZE = 1 / 256.0


class EvalPass(object):
    """ev = EvalPass(model, data, batch_size, noise_source, k=1); r = ev.run() evaluates one epoch and returns
    {"eval_bits_per_dim", "loss", "images", "batches", "k", "nonfinite", "noise_step"}.

    model: a loaded CVAE1 with k = 1, towers = 1, mode "train" (the reference's "eval" mode samples the posterior as "train" does,
    tf_train.py:57-66).  run() calls model.prepare_weights(), so variables that changed in place since the last run -- the views of
    TrainStep.ema_params() a training step writes -- are what it evaluates.
    data: a DeviceDataset with world = 1 (deterministic=True is the reference's order; a shuffled one works as well) whose size is a
    multiple of batch_size (tf_train.py:313).  noise_source: a NoiseSource; every pass draws one step of it.
    k: importance samples per image.  per_image=True: ev.per_image is an fp32 [data.n] tensor that holds -log p_k(x_i) in nats
    under every image's index after a run (NaN where the run did not come).
    graph=True: head and pass are captured once each on a stream of the object's own, behind a compute-only eager batch that
    advances neither the dataset nor the source; ev.graphed, ev.captures.  If the runtime refuses the capture, ev.graph_refused says
    why and the batches run as eager launches.  The numbers do not depend on `graph`.

    run(batches=None): one epoch (or the first `batches` batches) from the dataset's step 0; the noise source is left where the
    last pass put it, and r["noise_step"] is where it stood before the first.  loss = the sum over the images of the bound in nats
    (fp64, a fixed order: the same bits on every run), eval_bits_per_dim = loss / (ln 2 * 3 * S^2 * images), nonfinite = the
    number of images whose bound is NaN or inf (k > 1: the streaming update, StreamingLowerBound's, starts a row's sum afresh while
    its running maximum is -inf, so a NaN weight that is a row's first is dropped by the pass behind it; any later one
    counts).  One synchronisation, at the end.

    A run that ends with nonfinite > 0 while a stack or conv of the model has newly raised its range word (an operand beyond
    65504 in a launch on two fp16 planes, include/iaf_hip.h) moves those objects to bf16 planes through the existing protocol --
    compute-only eager passes, then a new capture --, seeks the source back to noise_step and repeats the run ONCE behind a
    RuntimeWarning; what the second run gives is returned as it is.

    images(total=36, temperature=1.0): run_eval's reconstruction and sample grids (k = 1 only); see the method."""

    def __init__(self, model, data, batch_size, noise_source, k=1, graph=True, per_image=False):
        if not isinstance(model, CVAE1) or model.params is None:
            raise ValueError("EvalPass: model must be a CVAE1 after load(params)")
        if model.k != 1 or model.towers != 1 or model.mode != "train":
            raise ValueError("EvalPass: a model with k = 1, towers = 1 and mode 'train' (the k samples are streamed; got k = %r, towers = %r, "
                             "mode %r)" % (model.k, model.towers, model.mode))
        if not isinstance(data, DeviceDataset):
            raise ValueError("EvalPass: data must be a DeviceDataset, got %r" % (data,))
        if data.world != 1:
            raise ValueError("EvalPass: the dataset was built for a world of %d (multi-rank evaluation is not covered)" % data.world)
        if not _capi.int_in(batch_size, 1, MAX_BATCH + 1):
            raise ValueError("EvalPass: batch_size must be an int in [1, %d], got %r" % (MAX_BATCH, batch_size))
        if data.n % batch_size:
            raise ValueError("EvalPass: the dataset's %d images are no multiple of batch_size %d (tf_train.py:313)" % (data.n, batch_size))
        if data.image_shape != (3, model.image_size, model.image_size):
            raise ValueError("EvalPass: images of shape %r, model built for %d" % (data.image_shape, model.image_size))
        if not isinstance(noise_source, NoiseSource):
            raise ValueError("EvalPass: noise_source must be a NoiseSource, got %r" % (noise_source,))
        if not _capi.int_in(k, 1):
            raise ValueError("EvalPass: k must be a positive int, got %r" % (k,))
        if not isinstance(graph, bool) or not isinstance(per_image, bool):
            raise ValueError("EvalPass: graph and per_image must be True or False")
        dev = data.device
        if noise_source.device != dev or any(v.device != dev for v in model.params.values()):
            raise ValueError("EvalPass: model, data and noise_source must live on one device")
        self.model, self.data, self.batch_size, self.noise_source, self.k = model, data, batch_size, noise_source, k
        self.device = dev
        self.use_graph = graph
        self.graph_refused = None
        self.captures = {"head": 0, "pass": 0}
        self.per_image = None
        self._want_per_image = per_image
        self._buf = None                  # the buffers head and pass work on (the captured graphs read these very tensors)
        self._graphs = None               # (head, pass)
        self._kept = None                 # what the captured head left for the captured pass
        self._stream = torch.cuda.Stream(device=dev) if graph else None
        self._objects = _recover.range_objects(model)
        self._seen = set()                # range objects already moved to bf16 planes

    # -- the launches -------------------------------------------------------------------------------------------------------------
    def _buffers(self):
        if self._buf is None:
            B, S, dev = self.batch_size, self.model.image_size, self.device
            f32 = dict(dtype=torch.float32, device=dev)
            b = dict(x=torch.empty((B, 3, S, S), dtype=torch.uint8, device=dev),
                     idx=torch.zeros(B, dtype=torch.int64, device=dev) if self._want_per_image else None,
                     rec=torch.zeros(4, dtype=torch.float64, device=dev),          # the 32-byte record
                     run_max=torch.empty(B, **f32), run_sum=torch.empty(B, **f32), bound=torch.empty(B, **f32),
                     noise=self.model.draw_noise(B, self.noise_source, which="posterior", advance=False), xf=None)
            if self._want_per_image:
                self.per_image = torch.full((self.data.n,), float("nan"), **f32)
            self._buf = b
        return self._buf

    def _head(self, advance=True):
        """the part of a batch that depends on the images only: gather, image scaling, x_enc, every layer's up pass"""
        b = self._buf
        self.data.next_batch(self.batch_size, out=b["x"], indices=b["idx"], advance=advance)
        b["xf"] = self.model._bottom_up(b["x"], b["noise"])

    def _pass(self, advance=True):
        """one importance sample of the batch: posterior noise, the top-down pass up to x_dec, the tail"""
        b, m, B = self._buf, self.model, self.batch_size
        m.draw_noise(B, self.noise_source, which="posterior", out=b["noise"], advance=advance)
        x_out, xf, costs = m._top_down(b["xf"], B, b["noise"], terms="raw")
        S = m.image_size
        _capi.check(_capi.lib().iaf_eval_tail(_ptr(x_out), _ptr(m.params["dec_log_stdv"]), _ptr(xf), 3 * S * S, BINSIZE, _ptr(costs),
                                              int(costs.shape[0]), B, _ptr(b["run_max"]), _ptr(b["run_sum"]), self.k,
                                              _ptr(b["idx"]), _ptr(self.per_image), _ptr(b["bound"]), _ptr(b["rec"]),
                                              _stream()))
        torch.autograd.graph.increment_version((b["run_max"], b["run_sum"], b["bound"], b["rec"]) +
                                               (() if self.per_image is None else (self.per_image,)))
        b["last"] = (x_out, costs)

    def _reset(self):
        b = self._buf
        _capi.check(_capi.lib().iaf_eval_reset(_ptr(b["rec"]), _ptr(b["run_max"]), _ptr(b["run_sum"]), self.batch_size, _stream()))

    def _move(self):
        """Compute-only eager batches (one head, one pass; neither the dataset nor the source advances) until two in a row report
        nothing (_recover.settle, as TrainStep._move).  Also the warm-up that precedes every capture."""
        def batch():
            self.model.prepare_weights()
            self._head(advance=False)
            self._pass(advance=False)
        _recover.settle(batch, len(self._objects), "EvalPass")

    def _state(self):
        return [(po.qz_mean, po.qz_logsd, po.up_context) for po in (layer.posterior for level in self.model.layers for layer in level)]

    def _capture(self):
        self._graphs = self._kept = None

        def head():
            self._head()
            return self._buf["xf"], self._state()       # (Python references: the pass is captured on exactly these tensors)
        done = _recover.capture(self, self._stream, self._move, [head, self._pass], "EvalPass", "the evaluation", stacklevel=5)
        if done is not None:
            self._graphs, self._kept = tuple(done[0]), done[1][0]
            self.captures["head"] += 1
            self.captures["pass"] += 1

    def _run_once(self, nb):
        b, k = self._buffers(), self.k
        try:
            self.model.prepare_weights()
        except _recover.SWITCHED:         # an object reports an EARLIER launch of somebody else's: move it before anything is enqueued
            self._move()
            self._graphs = self._kept = None
        if self.use_graph and self.graph_refused is None and self._graphs is None:
            self._capture()
        if self.per_image is not None:
            self.per_image.fill_(float("nan"))
        self.data.seek(0)
        self._reset()                     # (behind the capture and its compute-only batch: they leave a pass counted in the record)
        if self._graphs is not None:
            gh, gp = self._graphs
            for _ in range(nb):
                gh.replay()
                for _ in range(k):
                    gp.replay()
        else:
            for _ in range(nb):
                self._head()
                for _ in range(k):
                    self._pass()
        host = b["rec"].cpu()             # the run's one synchronisation
        counts = host[1:].view(torch.int64)
        return float(host[0]), int(counts[0]), int(counts[1])

    # -- public -------------------------------------------------------------------------------------------------------------------
    def run(self, batches=None):
        nb = self.data.n // self.batch_size
        if batches is not None:
            if not _capi.int_in(batches, 1, nb + 1):
                raise ValueError("EvalPass.run: batches must be an int in [1, %d], got %r" % (nb, batches))
            nb = batches
        noise_step = self.noise_source.tell()
        loss, images, nonfinite = self._run_once(nb)
        if nonfinite > 0:
            new = _recover.newly_flagged(self._objects, self._seen)
            if new:
                warnings.warn("EvalPass: %d of %d bounds were not finite and %d object(s) met an operand beyond fp16's range: they move to "
                              "bf16 planes and the run is repeated" % (nonfinite, images, len(new)), RuntimeWarning, stacklevel=2)
                self._move()
                self._graphs = self._kept = None          # captured again by the run below
                self.noise_source.seek(noise_step)
                loss, images, nonfinite = self._run_once(nb)
        S = self.model.image_size
        bpd = loss / (math.log(2.) * 3 * S * S * images) if images else float("nan")
        return {"eval_bits_per_dim": bpd, "loss": loss, "images": images, "batches": nb, "k": self.k, "nonfinite": nonfinite,
                "noise_step": noise_step}

    def images(self, total=36, temperature=1.0):
        """run_eval's two pictures (tf_train.py:329-376; hps.k = 1 only): "reconstructions" -- total/2 images of the dataset's next batch
        in the even slots, the model's reconstructions of them (the clipped x_dec output, m_trunc) in the odd ones, each stretched over
        its own total/2 rows -- and "samples" -- `total` images from the prior at `temperature`, stretched over the batch of
        batch_size rows they were drawn in and then over the `total` shown.  Both tiled with border 0 (iaf_amd/images.py).

        Returns the two grids as host uint8 ndarrays [Hg,Wg,3] under those names (write_png takes them), "reconstructions_f32" /
        "samples_f32" (the float grids in [0,1]), "inputs" (uint8 [total/2,3,S,S]), "x_mean" (fp32 [total/2,3,S,S]) and "x_gen" (fp32
        [batch_size,3,S,S]) as device tensors, and "data_step", "noise_step", "nonfinite": the dataset's step the batch was gathered
        at, the source's step of the posterior noise (the prior noise is the step behind it), and the number of non-finite elements
        the stretches met -- > 0: the source concerned shows NaN / 0 in its slots, behind a RuntimeWarning.
        The batch is the one at the dataset's current step, which advances by one: after run() on a deterministic dataset that is
        the wrap to batch 0, as in the reference.  The source advances by two steps.  Eager launches on the current stream, the ones
        CVAE1.forward and CVAE1.sample make: the epoch's record, per_image and the captured graphs are not touched.  One
        synchronisation, at the final copy."""
        if self.k != 1:
            raise ValueError("EvalPass.images: the reference draws its pictures with k = 1 only (tf_train.py:329), this pass has k = %r" % (self.k,))
        B = self.batch_size
        if not _capi.int_in(total, 2, B + 1) or total % 2:
            raise ValueError("EvalPass.images: total must be an even int in [2, batch_size = %d], got %r (a grid that spans several batches, "
                             "each of which the reference stretches on its own, is not covered)" % (B, total))
        if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature):
            raise ValueError("EvalPass.images: temperature must be a finite number, got %r" % (temperature,))
        m, half = self.model, total // 2
        lib = _capi.lib()
        steps = torch.empty((2, 2), dtype=torch.int64, device=self.device)          # [0]: the two counters as they stand, [1]: their digests
        parts = (_capi.StatePart * 2)()
        for i, owner in enumerate((self.data, self.noise_source)):
            parts[i].src, parts[i].dst, parts[i].bytes = owner.counter_ptr(), steps[0, i:].data_ptr(), 8
        _capi.check(lib.iaf_state_snapshot(parts, 2, _ptr(steps[1]), _stream()))     # (read in the stream: no tell(), which synchronises)
        try:
            m.prepare_weights()
        except _recover.SWITCHED:         # an object reports an EARLIER launch and has switched kernels: run() captures again
            self._graphs = self._kept = None
            m.prepare_weights()
        x = self.data.next_batch(B)
        x_mean = m.forward(x, m.draw_noise(B, self.noise_source, which="posterior"))[0]
        x_gen = m.sample(B, self.noise_source, temperature=temperature)
        rec8, recf, rr = image_grid([(x, half), (x_mean, half)], total)
        smp8, smpf, sr = image_grid([(x_gen, B, total)], total)
        host = torch.cat([rec8.reshape(-1), smp8.reshape(-1), steps[0].view(torch.uint8),
                          torch.cat([rr, sr])[:, 2].contiguous().view(torch.uint8)]).cpu()      # the one synchronisation
        n8 = rec8.numel()
        data_step, noise_step = (int(v) & (1 << 64) - 1 for v in host[2 * n8:2 * n8 + 16].clone().view(torch.int64))
        nonfinite = int(host[2 * n8 + 16:].clone().view(torch.int32).to(torch.int64).sum())
        if nonfinite > 0:
            warnings.warn("EvalPass.images: %d non-finite element(s) in what the pictures show: the slots concerned hold NaN / 0" % nonfinite,
                          RuntimeWarning, stacklevel=2)
        return {"reconstructions": host[:n8].reshape(rec8.shape).numpy(), "samples": host[n8:2 * n8].reshape(smp8.shape).numpy(),
                "reconstructions_f32": recf, "samples_f32": smpf, "inputs": x[:half], "x_mean": x_mean[:half], "x_gen": x_gen,
                "data_step": data_step, "noise_step": noise_step, "nonfinite": nonfinite}

    @property
    def graphed(self):
        """True if the batches replay captured hipGraphs"""
        return self._graphs is not None
