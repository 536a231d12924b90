#!/usr/bin/env python3
"""Generate tests/golden/cvae1_towers.npz by EXECUTING THE REFERENCE'S OWN CVAE1._forward(me, x_t, t) (tf_train.py:150-215) on tf_shim
for the towers t = 0, 1 of its training step (tf_train.py:124-147), like make_golden_model.py does for one tower:
    python tests/golden/make_golden_towers.py
Both towers run on the same variables (the reference's towers share them: reuse_variables, tf_train.py:130) with kl_min = 0.25, each on
its own rows of the batch -- tests/towers_reference.py: tower_inputs(t).  hps.num_gpus = 3, one more than the towers run, keeps the
summary branch (tf_train.py:202-208, 213-216: last tower only) out.  Stored per tower: x_out, obj, loss; and bits_per_dim of the step
as tf_train.py:142 forms it, sum of the towers' losses / (ln 2 * pixels * batch_size * towers).  TEST INFRASTRUCTURE ONLY."""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # tests/: towers_reference, objective_reference
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))      # the repository: oracle

import make_golden as MG          # installs the shim and imports the reference (its __main__ block does not run)
import golden_inputs as gi
import towers_reference as T

tf_shim, TT, P, STORE = MG.tf_shim, MG.TT, MG.P, MG.STORE


def gen_towers():
    c = gi.model_case_inputs(T.TOWERS_CASE)
    assert c["kl_min"] == 0.25 and c["k"] == 1 and c["mode"] == "train"
    hps = TT.HParams(batch_size=P(c["B"]), k=P(c["k"]), z_size=P(c["z_size"]), h_size=P(c["h_size"]), kl_min=c["kl_min"],
                     depth=P(c["depth"]), num_blocks=P(c["num_blocks"]), image_size=P(c["image_size"]), num_gpus=P(T.N_TOWERS + 1))
    out, losses = {}, []
    for t in range(T.N_TOWERS):
        x, noise = T.tower_inputs(t)
        MG.seed_store("", c["params"])                                   # the same variables for every tower
        STORE.noise_log[:] = []
        STORE.noise_queue[:] = list(noise)
        me = types.SimpleNamespace(hps=hps, mode="train", dec_log_stdv=tf_shim.T(np.float64(c["params"]["dec_log_stdv"])))
        x_out, obj, loss = TT.CVAE1._forward(me, tf_shim.T(x), t)
        assert not STORE.noise_queue and len(STORE.noise_log) == len(noise)
        out["tower%d/x_out" % t], out["tower%d/obj" % t], out["tower%d/loss" % t] = x_out, obj, loss
        losses.append(float(np.asarray(loss)))
        print("tower", t, "obj", float(np.asarray(obj)), "loss", losses[-1])
    num_pixels = 3 * c["image_size"] ** 2
    out["bits_per_dim"] = np.float64(sum(losses) / (np.log(2.) * num_pixels * c["B"] * T.N_TOWERS))      # tf_train.py:142
    print("bits/dim", float(out["bits_per_dim"]))
    MG.save("cvae1_towers", **out)


if __name__ == "__main__":
    gen_towers()
