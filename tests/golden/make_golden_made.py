#!/usr/bin/env python3
"""Generate tests/golden/theano_cvae_layer_made.npz by EXECUTING THE REFERENCE'S OWN models.cvae_layer with prior 'made' (models.py:36-38,
304-309: a multiconv2d stack '<name>_prior_conv1' with flipmask=False over z, on made_context, which down_conv1 emits in place of the
prior's mean and log standard deviation) -- up(), down_q() and down_p() -- through the loaders, the Theano shim and the noise queue of
make_golden_theano.py.  down_p of the reference does not sample this prior (models.py:338-340: it prints 'TODO: SAMPLES FROM MADE PRIOR'
and returns z = eps); the fixture holds what it does.  One case runs prior 'diag' for down_p.  Build container only:
    python tests/golden/make_golden_made.py
The case table and the inputs are here (golden_inputs.py holds the other fixtures' and stays as it is); importing this module needs
neither the reference nor the shim -- only main() does.  TEST INFRASTRUCTURE ONLY."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import golden_inputs as gi         # noqa: E402

# name: (B, n_h, n_z, depth_ar, H, W, kl_min, posterior, prior)
CASES = {
    "made_small": (3, 32, 16, 2, 6, 5, 0.25, "down_iaf2_nl", "made"),
    "made_64": (2, 64, 32, 2, 8, 8, 0.25, "down_iaf2_nl", "made"),
    "made_nl2_d1": (2, 32, 32, 1, 3, 7, 0.0, "down_iaf2_nl2", "made"),
    "diag_p": (2, 32, 16, 2, 4, 6, 0.0, "down_iaf2_nl", "diag"),
}
MADE_CASES = tuple(k for k in sorted(CASES) if CASES[k][8] == "made")
FIXTURE = "theano_cvae_layer_made.npz"


def case_inputs(cname, shapes):
    """weights (in sorted key order, shapes as the reference's constructors created them), inputs and noise of one case, regenerated
    from the case seed as make_golden_chain.case_inputs does; eps_p, the noise of down_p, is drawn last"""
    B, n_h, n_z, depth_ar, H, W = CASES[cname][:6]
    rng = np.random.RandomState(gi.case_seed(cname))
    w = {}
    for k in sorted(shapes):
        w[k] = (0.05 if k.endswith("_w") else 0.1) * rng.standard_normal(tuple(int(v) for v in shapes[k]))
    up_input, down_input = rng.standard_normal((B, n_h, H, W)), rng.standard_normal((B, n_h, H, W))
    eps_up, eps_down = rng.standard_normal((B, n_z, H, W)), rng.standard_normal((B, n_z, H, W))
    eps_p = rng.standard_normal((B, n_z, H, W))
    return dict(w=w, up_input=up_input, down_input=down_input, eps_up=eps_up, eps_down=eps_down, eps_p=eps_p)


def fixture_case(g, cname):
    """the inputs of `cname` with the weight shapes the fixture `g` (the loaded .npz) records"""
    pre = cname + "/w_shape/"
    return case_inputs(cname, {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)})


def main():
    import make_golden_theano as T          # loads the reference's graphy.nodes on the shim, installs the noise queue
    S, P = T.S, T.P
    with contextlib.redirect_stdout(io.StringIO()):
        models = T.load_py2("models", "models.py")
    out = {}
    for cname, (B, n_h, n_z, depth_ar, H, W, kl_min, posterior, prior) in CASES.items():
        w = {}
        with contextlib.redirect_stdout(io.StringIO()):
            layer = models.cvae_layer("1", prior, posterior, P(n_h), P(n_h), P(n_z), P(depth_ar), False, "elu", (P(3), P(3)),
                                      False, "nn", w)
        assert any(k.startswith("1_prior_conv1_") for k in w) == (prior == "made")
        n_down = (3 * n_h + 2 * n_z) if prior == "made" else (2 * n_h + 4 * n_z)
        assert w["1_down_conv1_w"].a.shape[0] == n_down, w["1_down_conv1_w"].a.shape
        shapes = {k: w[k].a.shape for k in w}
        c = case_inputs(cname, shapes)
        for k in sorted(w):
            w[k].set_value(c["w"][k])
            out["%s/w_shape/%s" % (cname, k)] = np.asarray(shapes[k], dtype=np.int64)
        T.NOISE.q[:] = [c["eps_up"], c["eps_down"]]          # the reference draws two noise tensors, the up pass's first
        said = io.StringIO()
        with contextlib.redirect_stdout(said):
            up_out = layer.up(S.TT(c["up_input"]), w)
            down_out, kl = layer.down_q(S.TT(c["down_input"]), True, w)
            assert not T.NOISE.q
            p_out = layer.down_p(S.TT(c["down_input"]), S.TT(c["eps_p"]), w)
        assert ("TODO: SAMPLES FROM MADE PRIOR" in said.getvalue()) == (prior == "made")
        kl = kl.a
        kl_sum = kl.sum(axis=(1, 2, 3))                                        # models.py:455
        if kl_min > 0:                                                         # :458-461
            obj_kl = np.maximum(np.asarray(kl_min), kl.sum(axis=(2, 3)).mean(axis=0)).sum()
        else:
            obj_kl = kl_sum                                                    # :466
        out.update({cname + "/up_out": up_out.a, cname + "/down_out": down_out.a, cname + "/down_p_out": p_out.a,
                    cname + "/kl": kl, cname + "/kl_sum": kl_sum, cname + "/obj_kl": np.asarray(obj_kl)})
    path = os.path.join(HERE, FIXTURE)
    np.savez_compressed(path, **out)
    print("wrote %s %.1f KiB, %d arrays" % (FIXTURE, os.path.getsize(path) / 1024.0, len(out)))


if __name__ == "__main__":
    main()
