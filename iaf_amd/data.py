"""DeviceDataset -- the training set in device memory, and one launch that gathers the next shuffled batch out of it (include/iaf_hip.h:
iaf_data_*): the counterpart of the reference's in-graph data source (tf_utils/cifar10_data.py:108-112 puts the whole set
into the graph, tf_utils/data_utils.py:29-36 shuffles per epoch and drops the remainder).

Stateless by definition: with G = B * world rows per global batch and bpe = n // G batches per epoch, row r of rank `rank` at step t is
image perm_e(j), e = t // bpe, j = (t % bpe) * G + rank * B + r (deterministic=True: image j).  perm_e is a keyed bijection of [0, n): a
4-round Feistel network on Philox4x32-10 with cycle walking (the header has the definition, tests/data_reference.py restates it in
numpy).  It is a keyed pseudo-random permutation, NOT a uniform draw from the n! orders: for tiny n the orders are visibly uneven (over
2400 epochs at n = 4, seed 99, all 24 orders occur, with counts from 63 to 130 around the even 100).

The step counter lives in device memory: a gather reads it and, with advance=True, a one-thread launch behind it adds one -- so a
captured graph that holds a gather trains on the next batch at every replay, and the host is out of the loop for whole epochs."""
import torch

from . import _capi

MAX_BATCH = 65535


class DeviceDataset(_capi.StepCounter):
    """ds = DeviceDataset(images, seed); x = ds.next_batch(B) gathers the batch of the current step and advances the step by one.

    images: a contiguous uint8 [n,3,S,S] device tensor, 1 <= n < 2**32; kept alive by the object and never copied (do not write to it
    while batches are drawn).  seed: 0 <= seed < 2**64 (a NoiseSource of the same seed shares no stream with it).
    deterministic=True (the reference's flag, used by its eval loop): the images in order, restarting at 0 after every epoch.
    rank, world: data-parallel ranks share images, seed and B and take disjoint rows of every global batch without talking.
    Drive one dataset from one stream at a time.
    seek / skip / tell (_capi.StepCounter): the step the next gather draws at."""
    _prefix = "iaf_data"

    def __init__(self, images, seed, deterministic=False, rank=0, world=1):
        if not _capi.int_in(seed, 0, 1 << 64):
            raise ValueError("seed must be an int in [0, 2**64), got %r" % (seed,))
        if not isinstance(deterministic, bool):
            raise ValueError("deterministic must be True or False, got %r" % (deterministic,))
        if not _capi.int_in(world, 1, 1 << 31):
            raise ValueError("world must be a positive int, got %r" % (world,))
        if not _capi.int_in(rank, 0, world):
            raise ValueError("rank must be an int in [0, world), got %r" % (rank,))
        if not (torch.is_tensor(images) and images.dtype == torch.uint8 and images.dim() == 4 and images.shape[1] == 3
                and images.shape[2] == images.shape[3] and images.is_contiguous()) or not images.is_cuda:
            raise ValueError("images must be a contiguous uint8 [n,3,S,S] device tensor")
        if not 1 <= images.shape[0] < 1 << 32 or images.shape[2] < 1:
            raise ValueError("images: 1 <= n < 2**32 images of at least one pixel, got shape %r" % (tuple(images.shape),))
        self.images, self.seed, self.deterministic, self.rank, self.world = images, seed, deterministic, rank, world
        self.device = images.device
        self.n = int(images.shape[0])
        self.image_shape = tuple(int(v) for v in images.shape[1:])
        self.bytes_per_image = 3 * self.image_shape[1] * self.image_shape[2]
        with torch.cuda.device(self.device):
            self._own = _capi.Handle("iaf_data_create", _capi.ptr(images), self.n, self.bytes_per_image, seed, int(deterministic))
        self._h = self._own.h

    def _check_batch(self, B):
        if not _capi.int_in(B, 1, MAX_BATCH + 1):
            raise ValueError("B must be an int in [1, %d], got %r" % (MAX_BATCH, B))
        if B * self.world > self.n:
            raise ValueError("a global batch of %d x %d rows is more than the dataset's %d images" % (B, self.world, self.n))

    def batches_per_epoch(self, B):
        """n // (B * world): the remainder is dropped and the next epoch reshuffles (host bookkeeping)"""
        self._check_batch(B)
        return self.n // (B * self.world)

    def next_batch(self, B, out=None, indices=None, advance=True):
        """the uint8 [B,3,S,S] batch of this rank at the current step (into `out` when given); `indices`: an int64 [B] device tensor
        that receives the image indices.  advance=False leaves the step alone.  One launch, host-side checks only, capturable."""
        self._check_batch(B)
        shape = (B,) + self.image_shape
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous()) \
                or out.device != self.device:
            raise ValueError("next_batch: out must be a contiguous uint8 %r tensor on %s" % (shape, self.device))
        written = (out,)
        ip = None
        if indices is not None:
            if not (torch.is_tensor(indices) and indices.dtype == torch.int64 and tuple(indices.shape) == (B,)
                    and indices.is_contiguous()) or indices.device != self.device:
                raise ValueError("next_batch: indices must be a contiguous int64 [%d] tensor on %s" % (B, self.device))
            ip = _capi.ptr(indices)
            written = (out, indices)
        _capi.check(_capi.lib().iaf_data_next_batch(self._h, _capi.ptr(out), ip, B, self.rank, self.world,
                                                    int(bool(advance)), _capi.stream()))
        # (raw-pointer writes: tell torch)
        torch.autograd.graph.increment_version(written)
        return out
