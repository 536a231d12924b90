"""fp64 restatement of CVAE1's mixed top-down pass (encode / decode / reconstruct), composed from the oracle's leaves: iaf_layer_up, and per
layer iaf_layer_down in mode "train" (latent from the posterior) or "sample" (from the prior), or -- for a GIVEN latent -- conv2d +
split_channels + conv2d / deconv2d (tf_train.py:52-54, 87-94).  tests/test_latents_reference.py holds it to O.cvae1_forward; the GPU tests
(tests/test_hip_latents.py) hold the engine to it."""
import numpy as np

from oracle import iaf_oracle as O


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def case_params(c):
    return {k: f32(v) for k, v in c["params"].items()}


def layer_order(depth, num_blocks):
    """(i, j, downsample) of every layer as the top-down pass runs them (tf_train.py:195-200)"""
    return [(i, j, i > 0 and j == 0) for i in reversed(range(depth)) for j in reversed(range(num_blocks))]


def bottom_up(x_uint8, p, c):
    """tf_train.py:153-187 at k = 1: {(i, j): (qz_mean, qz_logsd, up_context)}"""
    x = np.clip((x_uint8.astype(np.float64) + 0.5) / 256.0, 0.0, 1.0) - 0.5
    q = O._sub(p, "x_enc/")
    h = O.conv2d(x, q["V"], q["g"], q["b"], stride=(2, 2))
    ups = {}
    for i in range(c["depth"]):
        for j in range(c["num_blocks"]):
            h, qm, ql, uc = O.iaf_layer_up(h, O._sub(p, "IAF_%d_%d/" % (i, j)), c["z_size"], c["h_size"], downsample=(i > 0 and j == 0))
            ups[(i, j)] = (qm, ql, uc)
    return ups


def given_z_down(inp, lp, z, z_size, h_size, downsample):
    """one layer's down pass with its latent given: h_det = the sixth piece of down_conv1 (:52-54), then :87-94"""
    q = O._sub(lp, "down_conv1/")
    y = O.conv2d(O.elu(inp), q["V"], q["g"], q["b"])
    h_det = O.split_channels(y, [z_size] * 4 + [h_size] * 2)[5]
    h = O.elu(np.concatenate([z, h_det], axis=1))
    if downsample:
        q = O._sub(lp, "down_deconv2/")
        return O.resize_nearest_neighbor(inp, 2) + 0.1 * O.deconv2d(h, q["V"], q["g"], q["b"])
    q = O._sub(lp, "down_conv2/")
    return inp + 0.1 * O.conv2d(h, q["V"], q["g"], q["b"])


def top_down_mixed(p, c, sources, noise, ups=None, B=None):
    """sources[l]: "posterior" (noise[2l+1], needs ups), "prior" (noise[2l]) or the latent.  Returns (x_out, [z], [kl_cost or None])."""
    zs_, hs_ = c["z_size"], c["h_size"]
    order = layer_order(c["depth"], c["num_blocks"])
    assert len(sources) == len(order)
    if B is None:
        B = next(t for t in list(sources) + list(noise) if isinstance(t, np.ndarray)).shape[0]
    hw = c["image_size"] // 2 ** c["depth"]
    h = np.tile(np.asarray(p["h_top"]).reshape([1, -1, 1, 1]), [B, 1, hw, hw])
    z_all, costs = [], []
    for li, ((i, j, ds), s) in enumerate(zip(order, sources)):
        lp = O._sub(p, "IAF_%d_%d/" % (i, j))
        if isinstance(s, str) and s == "posterior":
            qm, ql, uc = ups[(i, j)]
            h, _, cost, blk = O.iaf_layer_down(h, lp, qm, ql, uc, f32(noise[2 * li + 1]), zs_, hs_, c["kl_min"], mode="train", downsample=ds)
            z_all.append(blk["z"])
            costs.append(cost)
        elif isinstance(s, str) and s == "prior":
            h, _, _, blk = O.iaf_layer_down(h, lp, None, None, None, None, zs_, hs_, c["kl_min"], mode="sample", downsample=ds,
                                            eps_prior=f32(noise[2 * li]))
            z_all.append(blk["z"])
            costs.append(None)
        else:
            h = given_z_down(h, lp, np.asarray(s, np.float64), zs_, hs_, ds)
            z_all.append(np.asarray(s, np.float64))
            costs.append(None)
    q = O._sub(p, "x_dec/")
    xo = O.deconv2d(O.elu(h), q["V"], q["g"], q["b"])
    return np.clip(xo, -0.5 + 1 / 512., 0.5 - 1 / 512.), z_all, costs


def reconstruct(p, c, x_uint8, noise, posterior_layers, ups=None):
    nl = c["depth"] * c["num_blocks"]
    ups = bottom_up(x_uint8, p, c) if ups is None else ups
    return top_down_mixed(p, c, ["posterior"] * posterior_layers + ["prior"] * (nl - posterior_layers), noise, ups, B=x_uint8.shape[0])


_CACHE = {}


def case_reference(name):
    """computed once per case and shared (read-only): params (fp32 values in fp64), ups, and for every n in 0 .. nl the x_out / z of
    reconstruct(n)"""
    if name not in _CACHE:
        import golden_inputs as gi
        c = gi.model_case_inputs(name)
        p = case_params(c)
        ups = bottom_up(c["x"], p, c)
        nl = c["depth"] * c["num_blocks"]
        recs = [reconstruct(p, c, c["x"], c["noise"], n, ups) for n in range(nl + 1)]
        for xo, zs, _ in recs:
            xo.setflags(write=False)
            for z in zs:
                z.setflags(write=False)
        _CACHE[name] = dict(c=c, p=p, ups=ups, nl=nl, recs=recs)
    return _CACHE[name]
