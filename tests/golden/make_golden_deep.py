#!/usr/bin/env python3
"""Generate tests/golden/theano_cvae_layer_deep.npz by EXECUTING THE REFERENCE'S OWN models.cvae_layer with posterior 'down_iaf2_deep'
(models.py:104-108, 179-181, 272-285: the IAF step's autoregressive network is the masked ResNet N.ar.resnet, graphy/nodes/ar.py:428-448,
478-528, named '<name>_deepiaf') and prior 'diag' -- up(), down_q() and down_p() -- through the loaders, the Theano shim and the noise
queue of make_golden_theano.py.  Build container only:
    python tests/golden/make_golden_deep.py
resnet_layer_a passes the literal (3,3) to ar.conv2d (ar.py:434-435), whose Python-2 integer division of the kernel size then yields a
float under the shim; main() wraps the LOADED module's ar.conv2d so that size_kernel arrives as Py2Int (the shim itself stays as it is).
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

# name: (B, n_h, n_z, depth, H, W, kl_min)
CASES = {
    "deep_d1": (2, 32, 32, 1, 3, 7, 0.0),
    "deep_d2": (3, 64, 32, 2, 6, 5, 0.25),
    "deep_nz16": (2, 32, 16, 1, 4, 6, 0.25),
    "deep_d4": (1, 32, 32, 4, 4, 4, 0.0),
}
FIXTURE = "theano_cvae_layer_deep.npz"
INPUT_SCALE = 0.3       # up_input / down_input: at unit scale max|kl| is 2e3 .. 2e4 and the absolute tolerances of the GPU tests mean nothing
KL_BOUND = 100.0        # asserted per case below


def case_inputs(cname, shapes):
    """weights (in sorted key order, shapes as the reference's constructors created them: 0.05 for _w, 0.1 otherwise), inputs (0.3 of a
    standard normal) and noise of one case, regenerated from the case seed; eps_p, the noise of down_p, is drawn last"""
    B, n_h, n_z, depth, H, W = CASES[cname][:6]
    rng = np.random.RandomState(gi.case_seed(cname))
    w = {}
    for k in sorted(shapes):
        w[k] = (0.05 if k.endswith("_w") else 0.1) * rng.standard_normal(tuple(int(v) for v in shapes[k]))
    up_input, down_input = INPUT_SCALE * rng.standard_normal((B, n_h, H, W)), INPUT_SCALE * rng.standard_normal((B, n_h, H, W))
    eps_up, eps_down = rng.standard_normal((B, n_z, H, W)), rng.standard_normal((B, n_z, H, W))
    eps_p = rng.standard_normal((B, n_z, H, W))
    return dict(w=w, up_input=up_input, down_input=down_input, eps_up=eps_up, eps_down=eps_down, eps_p=eps_p)


def fixture_case(g, cname):
    """the inputs of `cname` with the weight shapes the fixture `g` (the loaded .npz) records"""
    pre = cname + "/w_shape/"
    return case_inputs(cname, {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)})


def deep_names(name, depth):
    """the variables of N.ar.resnet(name + '_deepiaf', depth, ...) without their _w / _s / _b (ar.py:483-498)"""
    pre = name + "_deepiaf_"
    return [pre + "input"] + [pre + "%d_conv%d" % (i, j) for i in range(depth) for j in (1, 2)] + [pre + "out_0", pre + "out_1"]


def main():
    import make_golden_theano as T          # loads the reference's graphy.nodes on the shim, installs the noise queue
    S, P = T.S, T.P
    with contextlib.redirect_stdout(io.StringIO()):
        models = T.load_py2("models", "models.py")
    ar_conv2d = T.N.ar.conv2d

    def conv2d_py2int(name, n_in, n_out, size_kernel=(3, 3), *a, **k):
        return ar_conv2d(name, n_in, n_out, tuple(P(int(v)) for v in size_kernel), *a, **k)

    T.N.ar.conv2d = conv2d_py2int
    out = {}
    try:
        for cname, (B, n_h, n_z, depth, H, W, kl_min) in CASES.items():
            w = {}
            with contextlib.redirect_stdout(io.StringIO()):
                layer = models.cvae_layer("1", "diag", "down_iaf2_deep", P(n_h), P(n_h), P(n_z), P(depth), False, "elu", (P(3), P(3)),
                                          False, "nn", w)
            for nm in deep_names("1", depth):
                assert nm + "_w" in w and nm + "_s" in w and nm + "_b" in w, nm
            assert not any("posterior_conv" in k for k in w)
            shapes = {k: w[k].a.shape for k in w}
            c = case_inputs(cname, shapes)
            for k in sorted(w):
                w[k].set_value(c["w"][k])
                out["%s/w_shape/%s" % (cname, k)] = np.asarray(shapes[k], dtype=np.int64)
            T.NOISE.q[:] = [c["eps_up"], c["eps_down"]]          # the reference draws two noise tensors, the up pass's first
            with contextlib.redirect_stdout(io.StringIO()):
                up_out = layer.up(S.TT(c["up_input"]), w)
                down_out, kl = layer.down_q(S.TT(c["down_input"]), True, w)
                assert not T.NOISE.q
                p_out = layer.down_p(S.TT(c["down_input"]), S.TT(c["eps_p"]), w)
            kl = kl.a
            for a in (up_out.a, down_out.a, p_out.a, kl):
                assert np.isfinite(a).all(), cname
            assert np.abs(kl).max() < KL_BOUND, (cname, np.abs(kl).max())
            print("%s: max|kl| = %.3g" % (cname, np.abs(kl).max()))
            kl_sum = kl.sum(axis=(1, 2, 3))                                        # models.py:455
            if kl_min > 0:                                                         # :458-461
                obj_kl = np.maximum(np.asarray(kl_min), kl.sum(axis=(2, 3)).mean(axis=0)).sum()
            else:
                obj_kl = kl_sum                                                    # :466
            out.update({cname + "/up_out": up_out.a, cname + "/down_out": down_out.a, cname + "/down_p_out": p_out.a,
                        cname + "/kl": kl, cname + "/kl_sum": kl_sum, cname + "/obj_kl": np.asarray(obj_kl)})
    finally:
        T.N.ar.conv2d = ar_conv2d
    path = os.path.join(HERE, FIXTURE)
    np.savez_compressed(path, **out)
    print("wrote %s %.1f KiB, %d arrays" % (FIXTURE, os.path.getsize(path) / 1024.0, len(out)))


if __name__ == "__main__":
    main()
