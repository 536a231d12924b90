"""Training checkpoints: an in-stream snapshot of a TrainStep's state, one file, and the way back -- the reference's
saver.save every 100 steps (tf_train.py:286-287) and CheckpointLoader + Saver(model.avg_dict) in front of run_eval (tf_train.py:297-317).

    snap = ts.snapshot()              one launch on the current stream (include/iaf_hip.h: iaf_state_snapshot) copies the four flat buffers
                                      of ts.flat -- variables, both Adamax slots, the EMA -- into staging buffers the Snapshot owns and the
                                      step counters of the noise source and the dataset and the skip count into a small header tensor, and
                                      leaves a 64-bit digest of every part; an event behind it.  No synchronisation, nothing to the host:
                                      the run goes on, and the snapshot holds the state at ITS place in the stream.
    snap.save(path)                   waits for that event only, brings the staging buffers to the host, checks the digests, writes one file.
    ck = load_checkpoint(path)        header and arrays (memory-mapped); ck.params() / ck.ema_params() / ck.slots().
    ts.restore(ck)                    exact resume: the next steps are bit for bit the ones the saved run took.

The file, little endian: the 8 bytes IAFCKPT1, a u64 header length, a UTF-8 JSON header, then the four arrays raw (fp32, total_words
each) in the order params, slot_m, slot_v, ema, each starting at the next 64-byte boundary of the file.  No pickles, no code.

The digest of words w_0 .. w_{n-1} is sum_i (w_i + 1) * k_i mod 2^64, k_i = ((2 i + 1) * 0x9E3779B1) mod 2^32: a guard against
truncation, torn writes and stray bytes -- NOT a cryptographic hash.  `digest` below states it in numpy; the kernel's answer is the same
bits at every size.

Data-parallel runs: every rank holds the same variables, slots, EMA and counters; the ranks differ in the noise source's substream_base
and the dataset's rank only, and neither is restored (both belong to the objects the step was built with).  Rank 0's file therefore
restores every rank.

The summaries record of TrainStep(summaries=True) is not part of a checkpoint: a restored step starts its record as it does after
summaries(reset=True)."""
import json
import os

import numpy as np
import torch

from . import _capi, _recover

MAGIC = b"IAFCKPT1"
VERSION = 1
ARRAYS = ("params", "slot_m", "slot_v", "ema")
_ALIGN = 64
_CHUNK = 1 << 20
_MODEL = ("z_size", "h_size", "depth", "num_blocks", "k", "image_size", "kl_min", "depth_ar")
# the header tensor's 32-bit words: the noise source's step (2), the dataset's step (2), the skip count (1)
_H_NOISE, _H_DATA, _H_SKIP, _H_WORDS = 0, 2, 4, 8


def digest(a):
    """the 64-bit digest of the 32-bit words of `a` (a numpy array or a host tensor whose byte size is a multiple of 4), as an int"""
    if torch.is_tensor(a):
        a = a.detach().cpu().contiguous().numpy()
    w = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    if w.size % 4:
        raise ValueError("digest: %d bytes are no whole number of 32-bit words" % w.size)
    w = w.view("<u4")
    total = np.uint64(0)
    with np.errstate(over="ignore"):
        for lo in range(0, w.size, _CHUNK):
            c = w[lo:lo + _CHUNK].astype(np.uint64)
            i = np.arange(lo, lo + c.size, dtype=np.uint64)
            k = ((i * np.uint64(2) + np.uint64(1)) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
            total = total + ((c + np.uint64(1)) * k).sum(dtype=np.uint64)
    return int(total)


def _align(n):
    return (n + _ALIGN - 1) // _ALIGN * _ALIGN


def _layout(flat):
    """name, shape and word offset of every variable in FlatParams order, and the total number of words"""
    return dict(variables=[dict(name=k, shape=[int(v) for v in flat.p[k].shape], offset=int(flat.offset_of(k)[0])) for k in flat.p],
                total_words=int(flat.params.numel()))


def _views(arr, layout):
    out = {}
    for v in layout["variables"]:
        n = int(np.prod(v["shape"], dtype=np.int64)) if v["shape"] else 1
        out[v["name"]] = arr[v["offset"]:v["offset"] + n].reshape(v["shape"])
    return out


def _launch(parts, digests):
    """iaf_state_snapshot on the current stream; parts: (src pointer, dst pointer or None, bytes)"""
    table = (_capi.StatePart * len(parts))(*[_capi.StatePart(s, d, n) for s, d, n in parts])
    _capi.check(_capi.lib().iaf_state_snapshot(table, len(parts), _capi.ptr(digests), _capi.stream()))
    torch.autograd.graph.increment_version(digests)


class Snapshot(object):
    """What TrainStep.snapshot() returns: four staging buffers of the size of ts.flat's (snap.bufs, in ARRAYS order), a header tensor
    with the counters, the parts' digests and an event -- on the device for a device step, host clones for host replicas.
    snap.steps: ts.steps when the snapshot was enqueued."""

    def __init__(self, total, device):
        self.device = torch.device(device)
        self.on_device = self.device.type == "cuda"
        self.total = int(total)
        self.bufs = [torch.empty(self.total, dtype=torch.float32, device=self.device) for _ in ARRAYS]
        self.header = torch.zeros(_H_WORDS, dtype=torch.int32, device=self.device)
        self.digests = torch.zeros(_capi.IAF_STATE_MAX_PARTS, dtype=torch.int64, device=self.device)
        self.event = None
        self.steps = 0
        self._ts = None
        self._skip_base = 0
        self._has = (False, False)       # (the noise source's step, the dataset's step) are among the parts
        self._copy_stream = None

    # -- taking it ----------------------------------------------------------------------------------------------------------------
    def _take(self, ts):
        flat = ts.flat
        srcs = (flat.params, flat.slot_m, flat.slot_v, flat.ema)
        self._ts, self.steps, self._skip_base = ts, ts.steps, ts._skip_base
        self._has = (ts.noise_source is not None, ts.data is not None)
        if not self.on_device:
            for b, s in zip(self.bufs, srcs):
                b.copy_(s)
            self.header[_H_SKIP] = ts._host_skips
            self._host_digests = [digest(b) for b in self.bufs]
            return self
        nb = self.total * 4
        parts = [(s.data_ptr(), b.data_ptr(), nb) for s, b in zip(srcs, self.bufs)]
        hp = self.header.data_ptr()
        if ts.noise_source is not None:
            parts.append((ts.noise_source.counter_ptr(), hp + 4 * _H_NOISE, 8))
        if ts.data is not None:
            parts.append((ts.data.counter_ptr(), hp + 4 * _H_DATA, 8))
        parts.append((ts._skips.counter_ptr(), hp + 4 * _H_SKIP, 4))
        _launch(parts, self.digests)
        torch.autograd.graph.increment_version(tuple(self.bufs) + (self.header,))
        self.event = torch.cuda.Event()
        self.event.record()
        return self

    def _digest_only(self):
        """the digests of the four staging buffers as they stand (one launch without destinations; synchronises) -> four ints"""
        if not self.on_device:
            return [digest(b) for b in self.bufs]
        _launch([(b.data_ptr(), None, self.total * 4) for b in self.bufs], self.digests)
        return [int(v) & 0xFFFFFFFFFFFFFFFF for v in self.digests[:len(ARRAYS)].cpu().tolist()]

    # -- bringing it to the host ------------------------------------------------------------------------------------------------------
    def _fetch(self):
        """(four host arrays, their digests as the snapshot's launch left them, the header's words) after the snapshot's event -- and
        nothing else the stream holds"""
        if self._ts is None:
            raise RuntimeError("Snapshot: nothing has been taken into it yet")
        if not self.on_device:
            return [b.numpy() for b in self.bufs], list(self._host_digests), self.header.numpy().view(np.uint32)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        side = self._copy_stream
        side.wait_event(self.event)
        with torch.cuda.stream(side):
            arrays = [b.cpu().numpy() for b in self.bufs]
            digs = [int(v) & 0xFFFFFFFFFFFFFFFF for v in self.digests[:len(ARRAYS)].cpu().tolist()]
            words = self.header.cpu().numpy().view(np.uint32)
        side.synchronize()
        return arrays, digs, words

    def meta(self, digests, words):
        """the file's header for what _fetch returned (what does not live on the device is read from the step now: taking a snapshot
        stays a few host calls and one launch)"""
        ts = self._ts
        m = _static_meta(ts)
        raw_skips = int(words[_H_SKIP])
        m["digests"] = {k: "0x%016x" % d for k, d in zip(ARRAYS, digests)}
        m["steps"] = int(self.steps)
        m["skipped"] = int(self._skip_base + raw_skips)
        m["global_step"] = m["steps"] - m["skipped"]
        m["noise_step"] = int(words[_H_NOISE]) | int(words[_H_NOISE + 1]) << 32 if self._has[0] else None
        m["data_step"] = int(words[_H_DATA]) | int(words[_H_DATA + 1]) << 32 if self._has[1] else None
        moved = ts._seen | _recover.flagged(ts._objects)
        m["moved"] = sorted(int(i) for i in moved)
        m["range_objects"] = len(ts._objects)
        return m

    def save(self, path, verify=True):
        """write the snapshot to `path` (atomically: path + ".tmp", flush, fsync, rename).  Waits for the snapshot's event only.
        verify: the digests are recomputed on the host from the bytes about to be written; a mismatch raises IafHipError."""
        arrays, digs, words = self._fetch()
        if verify:
            for k, a, d in zip(ARRAYS, arrays, digs):
                got = digest(a)
                if got != d:
                    raise _capi.IafHipError("Snapshot.save: the digest of %s on the host is 0x%016x, the snapshot's launch left 0x%016x"
                                            % (k, got, d))
        write_file(path, self.meta(digs, words), arrays)
        return path


def _static_meta(ts):
    src, data, flat = ts.noise_source, ts.data, ts.flat
    b1, b2, eps, decay = ts._hyper
    m = dict(version=VERSION, layout=_layout(flat))
    m["noise"] = None if src is None else dict(seed=int(src.seed), substream_base=int(src.substream_base))
    m["data"] = None if data is None else dict(seed=int(data.seed), n=int(data.n), deterministic=bool(data.deterministic),
                                               world=int(data.world))
    m["batch_size"] = None if ts.batch_size is None else int(ts.batch_size)
    m["world"], m["towers"] = int(ts.world), int(ts.towers)
    m.update(lr=float(ts.lr), beta1=b1, beta2=b2, eps=eps, ema_decay=decay)
    m["model"] = {k: getattr(ts.model, k) for k in _MODEL if isinstance(getattr(ts.model, k, None), (int, float))}
    return m


def write_file(path, meta, arrays):
    """one checkpoint file from a header dict and the four arrays, atomically"""
    head = json.dumps(meta, sort_keys=True, allow_nan=False).encode("utf-8")
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(MAGIC)
            f.write(np.array([len(head)], dtype="<u8").tobytes())
            f.write(head)
            for a in arrays:
                f.write(b"\0" * (_align(f.tell()) - f.tell()))
                f.write(np.ascontiguousarray(a, dtype="<f4").reshape(-1).view(np.uint8))
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


class Checkpoint(object):
    """A loaded checkpoint: ck.meta (the header) and the four flat arrays (ck.arrays: name -> fp32 [total_words], memory-mapped
    copy-on-write: writing to them never touches the file)."""

    def __init__(self, meta, arrays, path=None):
        self.meta, self.arrays, self.path = meta, arrays, path

    def _named(self, which, device):
        if device is None:
            return _views(self.arrays[which], self.meta["layout"])
        t = torch.from_numpy(np.array(self.arrays[which], dtype=np.float32)).to(device)
        return _views(t, self.meta["layout"])

    def params(self, device=None):
        """the variables, name -> numpy view in the variable's shape (device=: fp32 tensors there, views into one flat upload)"""
        return self._named("params", device)

    def ema_params(self, device=None):
        """the EMA of the variables under the same names: eval_model.load(ck.ema_params(device="cuda")), then EvalPass(...).run(), is the
        reference's CheckpointLoader + Saver(model.avg_dict) path"""
        return self._named("ema", device)

    def slots(self, device=None):
        """(slot_m, slot_v): the two Adamax slots, each name -> view"""
        return self._named("slot_m", device), self._named("slot_v", device)


def _check_meta(meta):
    if not isinstance(meta, dict):
        raise ValueError("the header is no JSON object")
    if meta.get("version") != VERSION:
        raise ValueError("checkpoint format version %r, this package reads version %d" % (meta.get("version"), VERSION))
    lay = meta.get("layout")
    if not isinstance(lay, dict) or not isinstance(lay.get("variables"), list) or not isinstance(lay.get("total_words"), int) \
            or lay["total_words"] < 1:
        raise ValueError("the header holds no flat layout")
    for v in lay["variables"]:
        n = int(np.prod(v["shape"], dtype=np.int64)) if v["shape"] else 1
        if v["offset"] < 0 or v["offset"] + n > lay["total_words"]:
            raise ValueError("variable %r lies outside the flat buffer" % (v.get("name"),))
    if not isinstance(meta.get("digests"), dict) or any(k not in meta["digests"] for k in ARRAYS):
        raise ValueError("the header holds no digests")


def load_checkpoint(path, verify=True):
    """read a checkpoint file -> Checkpoint.  ValueError (with the reason) for a file that is not a checkpoint, is truncated or has
    another format version; with verify, IafHipError for an array whose digest is not the header's."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        fixed = f.read(16)
        if len(fixed) < 16 or fixed[:8] != MAGIC:
            raise ValueError("%s is not a checkpoint (it does not begin with %s)" % (path, MAGIC.decode()))
        hlen = int(np.frombuffer(fixed[8:], dtype="<u8")[0])
        if 16 + hlen > size:
            raise ValueError("%s is truncated: a header of %d bytes in a file of %d" % (path, hlen, size))
        try:
            meta = json.loads(f.read(hlen).decode("utf-8"))
        except (UnicodeDecodeError, ValueError) as e:
            raise ValueError("%s: the header is not JSON (%s)" % (path, e))
    try:
        _check_meta(meta)
    except (KeyError, TypeError) as e:
        raise ValueError("%s: the header is incomplete (%r)" % (path, e))
    except ValueError as e:
        raise ValueError("%s: %s" % (path, e))
    nb = 4 * meta["layout"]["total_words"]
    off, offs = 16 + hlen, []
    for _ in ARRAYS:
        off = _align(off)
        offs.append(off)
        off += nb
    if off > size:
        raise ValueError("%s is truncated: the declared layout needs %d bytes, the file has %d" % (path, off, size))
    arrays = {k: np.memmap(path, dtype="<f4", mode="c", offset=o, shape=(nb // 4,)) for k, o in zip(ARRAYS, offs)}
    if verify:
        for k in ARRAYS:
            got, want = digest(arrays[k]), int(meta["digests"][k], 16)
            if got != want:
                raise _capi.IafHipError("%s: the digest of %s is 0x%016x, the header says 0x%016x" % (path, k, got, want))
    return Checkpoint(meta, arrays, path)


def save_checkpoint(ts, path):
    """ts.snapshot().save(path)"""
    return ts.snapshot().save(path)


# -- the TrainStep side (TrainStep.snapshot / TrainStep.restore call these) -------------------------------------------------------------
def take_snapshot(ts, into=None):
    if ts.on_device and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("TrainStep.snapshot: the current stream is capturing (take the snapshot between two steps)")
    total, dev = ts.flat.params.numel(), ts.flat.params.device
    if into is None:
        into = Snapshot(total, dev)
    elif not isinstance(into, Snapshot) or into.total != total or into.device != dev:
        raise ValueError("TrainStep.snapshot(into=): a Snapshot of %d words on %s" % (total, dev))
    return into._take(ts)


def _first_difference(meta, ts):
    """None, or what makes the checkpoint another run's than this step's"""
    want, have = _layout(ts.flat), meta["layout"]
    if have["total_words"] != want["total_words"] or len(have["variables"]) != len(want["variables"]):
        return "%d variables in %d words, the step has %d in %d" % (len(have["variables"]), have["total_words"], len(want["variables"]),
                                                                    want["total_words"])
    for a, b in zip(have["variables"], want["variables"]):
        if a["name"] != b["name"] or list(a["shape"]) != b["shape"] or a["offset"] != b["offset"]:
            return "variable %r %r at word %d where the step has %r %r at word %d" % (a["name"], a["shape"], a["offset"], b["name"],
                                                                                      b["shape"], b["offset"])
    for k in ("world", "towers"):
        if meta.get(k) != getattr(ts, k):
            return "%s is %r, the step's is %r" % (k, meta.get(k), getattr(ts, k))
    if ts.data is not None and meta.get("data") is not None:
        if meta.get("batch_size") != ts.batch_size:
            return "batch_size is %r, the step's is %r" % (meta.get("batch_size"), ts.batch_size)
        if meta["data"].get("n") != ts.data.n:
            return "the dataset had %r images, the step's has %d" % (meta["data"].get("n"), ts.data.n)
    for k, obj, what in (("noise_step", ts.noise_source, "noise source"), ("data_step", ts.data, "dataset")):
        if (meta.get(k) is None) != (obj is None):
            return "%s is %r, and the step has %s %s" % (k, meta.get(k), "no" if obj is None else "a", what)
    moved = meta.get("moved", [])
    if not isinstance(moved, list) or not all(_capi.int_in(i, 0, len(ts._objects)) for i in moved):
        return "moved is %r, the step's model has %d stacks and convs" % (moved, len(ts._objects))
    if moved and meta.get("range_objects") != len(ts._objects):
        return "moved counts among %r stacks and convs, the step's model has %d" % (meta.get("range_objects"), len(ts._objects))
    for k in ("steps", "skipped"):
        if not _capi.int_in(meta.get(k), 0):
            return "%s is %r" % (k, meta.get(k))
    return None


def restore(ts, ck):
    if not isinstance(ck, Checkpoint):
        ck = load_checkpoint(ck)
    if ts.on_device and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("TrainStep.restore: the current stream is capturing")
    meta = ck.meta
    diff = _first_difference(meta, ts)
    if diff is not None:
        raise ValueError("TrainStep.restore: the checkpoint is not this step's: " + diff)
    flat = ts.flat
    total = flat.params.numel()
    for k in ARRAYS:
        if ck.arrays[k].shape != (total,):
            raise ValueError("TrainStep.restore: %s has shape %r, not (%d,)" % (k, ck.arrays[k].shape, total))
    # the arrays into a staging snapshot, and their digests as the DEVICE sees them, before anything of the step is touched
    stage = Snapshot(total, flat.params.device)
    for b, k in zip(stage.bufs, ARRAYS):
        b.copy_(torch.from_numpy(np.array(ck.arrays[k], dtype=np.float32)))
    for k, got in zip(ARRAYS, stage._digest_only()):
        want = int(meta["digests"][k], 16)
        if got != want:
            raise _capi.IafHipError("TrainStep.restore: the digest of %s after the upload is 0x%016x, the header says 0x%016x"
                                    % (k, got, want))
    # in place: the views the model (and any eval model) holds stay valid, a captured graph reads the buffers where they are, and
    # copy_ bumps the versions the prep caches key on
    for t, b in zip((flat.params, flat.slot_m, flat.slot_v, flat.ema), stage.bufs):
        t.copy_(b)
    if ts.noise_source is not None:
        ts.noise_source.seek(int(meta["noise_step"]))
    if ts.data is not None:
        ts.data.seek(int(meta["data_step"]))
    if ts.on_device:
        torch.cuda.synchronize()
    ts.steps = int(meta["steps"])
    ts._skip_base = int(meta["skipped"]) - ts._count()
    for i in meta.get("moved", []):
        ts._objects[i].set_precision("bf16x3")
    ts._seen.update(meta.get("moved", []))
    if meta.get("moved") and ts._graph is not None:
        ts._stale = True
    ts._reset_record()
    return ck
