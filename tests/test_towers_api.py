"""CPU checks of the towers interface: TrainStep on a host stand-in model with .towers divides by world * towers (one process, and a
world-2 gloo run), and the argument checks of towers / groups."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_train_step_api import HostModel, _clean


class TowerModel(HostModel):
    def __init__(self, towers, seed=3):
        HostModel.__init__(self, seed)
        self.towers = towers


def test_a_model_with_towers_updates_as_that_many_replicas():
    import iaf_amd
    from iaf_amd import parallel as par
    ts = iaf_amd.TrainStep(TowerModel(4), 0.01, n_buckets=2, graph=False)
    assert ts.world == 1 and ts.towers == 4
    ref = par.FlatParams({k: v.clone() for k, v in ts.flat.p.items()})
    one = par.FlatParams({k: v.clone() for k, v in ts.flat.p.items()})
    for step in range(3):
        ts(*_clean(1.0 + step))
        for k in HostModel.NAMES:
            ref.g[k].copy_(ts.flat.g[k])
            one.g[k].copy_(ts.flat.g[k])
        ref.adamax_ema_step(0.01, world=4)
        one.adamax_ema_step(0.01, world=1)
        for a, b in ((ts.flat.params, ref.params), (ts.flat.ema, ref.ema), (ts.flat.slot_m, ref.slot_m), (ts.flat.slot_v, ref.slot_v)):
            assert torch.equal(a, b), step
    assert not torch.equal(ts.flat.slot_m, one.slot_m)                    # (the divisor matters on these gradients)
    # no towers attribute, or 1: as before
    plain = iaf_amd.TrainStep(HostModel(), 0.01, graph=False)
    assert plain.towers == 1


def test_towers_attribute_is_checked():
    import iaf_amd
    for bad in (0, -1, True, 2.0, "2", 65, None):
        with pytest.raises(ValueError):
            iaf_amd.TrainStep(TowerModel(bad), 0.01, graph=False)


def test_towers_and_groups_arguments_are_checked_before_anything_touches_the_device():
    import iaf_amd
    from iaf_amd import layers
    for bad in (0, -3, True, False, 1.0, "4", None, 65, 1 << 20):
        with pytest.raises(ValueError):
            layers.check_groups(bad)
        with pytest.raises(ValueError):
            iaf_amd.CVAE1(towers=bad)
        with pytest.raises(ValueError):
            layers.kl_free_bits(torch.zeros(4, 2, 2, 2), 0.25, groups=bad)
    assert [layers.check_groups(n) for n in (1, 2, 64)] == [1, 2, 64]
    assert layers.MAX_FREE_BITS_GROUPS == 64


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import iaf_amd
    from iaf_amd import parallel as par
    ts = iaf_amd.TrainStep(TowerModel(2), 0.01, n_buckets=2, graph=False)
    ref = par.FlatParams({k: v.clone() for k, v in ts.flat.p.items()})
    same = True
    for step in range(3):
        ts(*_clean(1.0 + rank + step))                                 # rank-specific batches
        for k in HostModel.NAMES:
            ref.g[k].copy_(ts.flat.g[k])                               # (the all-reduced sums)
        ref.adamax_ema_step(0.01, world=4)
        same = same and torch.equal(ts.flat.params, ref.params) and torch.equal(ts.flat.ema, ref.ema)
    out[rank] = dict(params=ts.flat.params.numpy().copy(), ema=ts.flat.ema.numpy().copy(), world=ts.world, towers=ts.towers, same=same)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_gloo_with_two_towers_divide_by_four():
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    for r in range(2):
        assert out[r]["world"] == 2 and out[r]["towers"] == 2
        assert out[r]["same"], r                                          # the update with 1 / (world * towers) = 1 / 4
    for k in ("params", "ema"):
        np.testing.assert_array_equal(out[0][k], out[1][k])               # replicas stay identical
