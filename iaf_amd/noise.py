"""NoiseSource -- the engine's own N(0,1) generator (include/iaf_hip.h: iaf_rng_*), the counterpart of the noise the
reference's DiagonalGaussian draws inside the graph (tf_utils/distributions.py:15-24).

Counter-based (Philox4x32-10 -> Box-Muller): element i of a tensor is a function of (seed, substream, step, i) alone.  The step
counter lives in device memory: a fill reads it and, with advance=True, a one-thread launch behind it adds one -- so a captured
graph that holds a fill draws fresh noise on every replay.  One launch fills up to 64 tensors."""
import ctypes

import torch

from . import _capi

MAX_TENSORS = 64
MAX_COUNT = 1 << 34


class NoiseSource(_capi.StepCounter):
    """src = NoiseSource(seed); src.fill([t0, t1, ...]) fills contiguous fp32 device tensors with N(0,1) noise at the current step
    and advances the step by one.

    seed: 0 <= seed < 2**64.  device: the device the counter lives on (default: the current one); tensors must be on it.
    substream_base: the substream of the first tensor of a list (the others follow); data-parallel ranks share the seed and use
    substream_base = rank << 16.  Drive one source from one stream at a time.
    seek / skip / tell (_capi.StepCounter): the step the next fill draws at."""
    _prefix = "iaf_rng"

    def __init__(self, seed, device=None, substream_base=0):
        if not _capi.int_in(seed, 0, 1 << 64):
            raise ValueError("seed must be an int in [0, 2**64), got %r" % (seed,))
        if not _capi.int_in(substream_base, 0, 1 << 32):
            raise ValueError("substream_base must be an int in [0, 2**32), got %r" % (substream_base,))
        self.seed, self.substream_base = seed, substream_base
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("NoiseSource lives on a GPU, got device %r" % (device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(self.device):
            self._own = _capi.Handle("iaf_rng_create", seed)
        self._h = self._own.h

    def fill(self, tensors, substreams=None, scales=None, advance=True):
        """tensors[i] <- scales[i] * N(0,1) at the current step, substream substreams[i] (default substream_base + i; scales default 1).
        Lists longer than 64 go out in several launches; the step advances once, behind the last.  Host-side checks only."""
        tensors = list(tensors)
        n = len(tensors)
        if n < 1:
            raise ValueError("fill: at least one tensor")
        if substreams is None:
            substreams = [self.substream_base + i for i in range(n)]
        if len(substreams) != n or (scales is not None and len(scales) != n):
            raise ValueError("fill: one substream (and one scale) per tensor")
        for i, t in enumerate(tensors):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) or t.device != self.device:
                raise ValueError("fill: tensors[%d] must be a contiguous fp32 tensor on %s" % (i, self.device))
            if not 1 <= t.numel() <= MAX_COUNT:
                raise ValueError("fill: tensors[%d] has %d elements (1 .. 2**34)" % (i, t.numel()))
            s = substreams[i]
            if not _capi.int_in(s, 0, 1 << 32):
                raise ValueError("fill: substreams[%d] must be an int in [0, 2**32), got %r" % (i, s))
        lib, st = _capi.lib(), _capi.stream()
        for lo in range(0, n, MAX_TENSORS):
            hi = min(n, lo + MAX_TENSORS)
            m = hi - lo
            outs = (ctypes.c_void_p * m)(*[t.data_ptr() for t in tensors[lo:hi]])
            counts = (ctypes.c_size_t * m)(*[t.numel() for t in tensors[lo:hi]])
            subs = (ctypes.c_uint * m)(*substreams[lo:hi])
            sc = None if scales is None else (ctypes.c_float * m)(*[float(v) for v in scales[lo:hi]])
            _capi.check(lib.iaf_rng_fill_normal(self._h, outs, counts, subs, sc, m, int(bool(advance) and hi == n), st))
        # (raw-pointer writes: tell torch)
        torch.autograd.graph.increment_version(tuple(tensors))
        return tensors
