"""CPU checks of the EMA as loadable views (parallel.FlatParams.e, what TrainStep.ema_params() returns and an evaluation model is
loaded from): the names and shapes of p, storage shared with the flat EMA buffer at the offsets offset_of reports, and the values an
optimiser step leaves there.  Host tensors only: no GPU needed."""
import numpy as np
import torch

from iaf_amd.parallel import FlatParams


def _named():
    rng = np.random.RandomState(11)
    shapes = {"x_enc/V": (5, 5, 3, 8), "x_enc/g": (8,), "h_top": (7,), "dec_log_stdv": (), "IAF_0_0/up_conv1/b": (3,), "x_dec/V": (5, 5, 3, 8)}
    return {k: torch.from_numpy(np.asarray(rng.standard_normal(s), dtype=np.float32)) for k, s in shapes.items()}


def test_e_has_the_names_and_shapes_of_p_and_views_the_ema_buffer():
    named = _named()
    flat = FlatParams(named)
    assert list(flat.e) == list(flat.p) == list(named)
    for k, v in flat.e.items():
        assert v.shape == flat.p[k].shape == named[k].shape and v.dtype == torch.float32
        lo, hi = flat.offset_of(k)
        assert v.data_ptr() == flat.ema.data_ptr() + 4 * lo and hi - lo == v.numel()
        assert v.untyped_storage().data_ptr() == flat.ema.untyped_storage().data_ptr()
        assert torch.equal(v, named[k]), "the EMA starts at the parameters"
        assert v.data_ptr() % 16 == flat.ema.data_ptr() % 16, "every view keeps the buffer's 16-byte alignment"
    # a write through a view lands in the flat buffer, and the other way round
    lo, hi = flat.offset_of("h_top")
    flat.e["h_top"].fill_(3.0)
    assert bool((flat.ema[lo:hi] == 3.0).all())
    flat.ema[lo:hi] = -1.0
    assert bool((flat.e["h_top"] == -1.0).all())


def test_e_follows_the_optimiser_step():
    named = _named()
    flat = FlatParams(named)
    rng = np.random.RandomState(12)
    for step in range(3):
        flat.grads.copy_(torch.from_numpy(rng.standard_normal(flat.grads.numel()).astype(np.float32)))
        flat.adamax_ema_step(0.01, world=2, ema_decay=0.9)
        for k in named:
            lo, hi = flat.offset_of(k)
            assert torch.equal(flat.e[k].reshape(-1), flat.ema[lo:hi]), (step, k)
            assert not torch.equal(flat.e[k], flat.p[k]) or flat.p[k].numel() == 0, "the average lags the parameters"
    assert not torch.equal(flat.e["x_enc/V"], named["x_enc/V"])
