"""Reference statements for the 'down_iaf2_deep' posterior of models.cvae_layer (models.py:104-108, 179-181, 272-285): ONE IAF step whose
autoregressive network is the masked ResNet N.ar.resnet (graphy/nodes/ar.py:428-448, 478-528), prior 'diag'.  TEST INFRASTRUCTURE ONLY.

The network, with conv_X a masked 3x3 conv of the Theano statement (oracle.iaf_oracle.theano_ar_conv2d), D = depth, nl = elu:

    h_0     = conv_input(z) + context                 n_z -> n_h, not zero-diagonal; NO nonlinearity    ar.py:502-504
    t_i     = elu(conv1_i(elu(h_i)))                  n_h -> n_h, not zero-diagonal                     ar.py:437-439
    h_{i+1} = h_i + 0.1 * conv2_i(t_i)                n_h -> n_h, not zero-diagonal                     ar.py:440-441
    m_raw, s_raw = out_0(h_D), out_1(h_D)             n_h -> n_z, zero-diagonal, on the RAW stream      ar.py:511-514
    m, s = 0.1 m_raw, 0.1 s_raw;  z' = (z - m) / exp(s);  logqs += s                                    models.py:281-285

Three statements:
  * NumPy fp64, composed from oracle.iaf_oracle.theano_ar_conv2d: resnet, deep_step, deep_iaf (between the plain convs), deep_layer (the
    whole layer), down_p_layer, inverse_exact (the ancestral solution of the step's inverse);
  * torch fp64, composed from oracle.iaf_grad_oracle.theano_ar_conv2d, for gradients: resnet_torch, deep_step_torch, deep_iaf_torch,
    deep_iaf_grads (autograd of the WHOLE statement), deep_step_grads (one step alone);
  * deep_iaf_grads_by_steps: the decomposition CVAELayerIAF.backward runs -- iaf_chain_backward_pre, the step's backward, and
    iaf_chain_backward_post with a zero second context gradient -- from the NumPy contracts of tests/chain_reference.py.

Channel orders (models.py:141-143, 273-279, 296-297): as 'down_iaf2_nl'
    up_conv1 output    [h_det (n_h) | qz_mean (n_z) | qz_logsd (n_z) | up_context (n_h)]
    down_conv1 output  [h_det (n_h) | pz_mean | pz_logsd | rz_mean | rz_logsd (n_z each) | down_context (n_h)]"""
import numpy as np
import torch
import torch.nn.functional as F

import chain_reference as C
from oracle import iaf_grad_oracle as G
from oracle import iaf_oracle as O

LOG2PI = C.LOG2PI
_cut = C._cut


def conv_names(depth):
    """the convs of the network in the engine's order, relative to the network's name"""
    return ["input"] + ["%d_conv%d" % (i, j) for i in range(depth) for j in (1, 2)] + ["out_0", "out_1"]


def rand_params(rng, name, n_z, n_h, depth):
    """the weights of N.ar.resnet(name, depth, n_z, n_h, [n_z, n_z]) in the reference's layout (ar.py:288-296), at the fixtures' scales"""
    w = {}
    for nm in conv_names(depth):
        n_in = n_z if nm == "input" else n_h
        n_out = n_z if nm.startswith("out_") else n_h
        w["%s_%s_w" % (name, nm)] = 0.05 * rng.standard_normal((n_out, n_in + 1, 3, 3))
        w["%s_%s_b" % (name, nm)] = 0.1 * rng.standard_normal(n_out)
        w["%s_%s_s" % (name, nm)] = 0.1 * rng.standard_normal(n_out)
    return w


def _elu(t):
    return np.where(t < 0, np.exp(np.minimum(t, 0)) - 1, t)


# ---------------------------------------------------------------- NumPy fp64
def _conv(h, w, p, n_in, n_out, zerodiagonal):
    return O.theano_ar_conv2d(h, w[p + "_w"], w[p + "_b"], w[p + "_s"], n_in, n_out, zerodiagonal, False)


def resnet(z, context, w, name, n_z, n_h, depth, return_hiddens=False):
    """N.ar.resnet(name, depth, n_z, n_h, [n_z, n_z]) with layertype 'a', nl 'elu' -> [m_raw, s_raw] (and the raw streams h_0 .. h_D)"""
    h = _conv(z, w, name + "_input", n_z, n_h, False)                                          # ar.py:502
    if context is not None:
        h = h + context                                                                        # :503-504
    hs = [h]
    for i in range(depth):
        t = _elu(_conv(_elu(h), w, "%s_%d_conv1" % (name, i), n_h, n_h, False))                 # :438-439
        h = h + 0.1 * _conv(t, w, "%s_%d_conv2" % (name, i), n_h, n_h, False)                   # :440-441
        hs.append(h)
    out = [_conv(h, w, "%s_out_%d" % (name, j), n_h, n_z, True) for j in range(2)]             # :511-514: the RAW stream
    return (hs, out) if return_hiddens else out


def deep_step(z, context, w, name, n_z, n_h, depth):
    """models.py:281-285 -> (z_new, logsd)"""
    m, s = resnet(z, context, w, name, n_z, n_h, depth)
    m, s = 0.1 * m, 0.1 * s
    return (z - m) / np.exp(s), s


def inverse_exact(z_new, context, w, name, n_z, n_h, depth, sweeps=None):
    """z0 with deep_step(z0)[0] == z_new by H W n_z Jacobi sweeps z0 <- z_new exp(s(z0)) + m(z0) from z0 = z_new: (m, s) at a position
    read only strictly earlier positions of the autoregressive order, so every sweep finalises at least one more position, whatever the
    weights (tests/made_reference.py has the induction)"""
    _, _, H, W = z_new.shape
    z0 = z_new.copy()
    for _ in range(H * W * n_z if sweeps is None else sweeps):
        m, s = resnet(z0, context, w, name, n_z, n_h, depth)
        nxt = z_new * np.exp(0.1 * s) + 0.1 * m
        if np.array_equal(nxt, z0):
            break
        z0 = nxt
    return z0


def deep_iaf(h_up, h_dn, eps, w, name, n_h, n_z, depth):
    """models.py:272-285, 295-298, 317-318 between the plain convs.  Returns dict(z0, logq0, context, z, s1, kl, h)."""
    _, qm, ql, uctx = _cut(h_up, [n_h, n_z, n_z, n_h])
    h_det, pm, pl, rm, rl, dctx = _cut(h_dn, [n_h, n_z, n_z, n_z, n_z, n_h])
    mean, logvar = qm + rm, 2 * ql + 2 * rl                                                    # :275
    z0 = mean + np.exp(0.5 * logvar) * eps
    logq0 = O.gaussian_diag_logps(mean, logvar, z0)
    context = uctx + dctx                                                                      # :280
    z, s1 = deep_step(z0, context, w, name + "_deepiaf", n_z, n_h, depth)                      # :281-285
    kl = logq0 + s1 - O.gaussian_diag_logps(pm, 2 * pl, z)                                      # :298, 328
    return dict(z0=z0, logq0=logq0, context=context, z=z, s1=s1, kl=kl, h=np.concatenate([h_det, z], axis=1))


def _cw(w, name, nm):
    return w[name + nm + "_w"], w[name + nm + "_b"], w[name + nm + "_s"]


def deep_layer(name, w, n_h, n_z, depth, up_input, down_input, eps_down):
    """the whole cvae_layer with posterior 'down_iaf2_deep', prior 'diag', nl 'elu', no downsampling (eps_up is drawn by the reference
    but reaches no output: the up pass of this posterior returns h_det only, models.py:179-181)"""
    up_conv1 = O.theano_conv2d(_elu(up_input), *_cw(w, name, "_up_conv1_1"))                    # :139
    up_out = up_input + 0.1 * O.theano_conv2d(_elu(up_conv1[:, :n_h]), *_cw(w, name, "_up_conv2"))   # :181, 191
    down_conv1 = O.theano_conv2d(_elu(down_input), *_cw(w, name, "_down_conv1"))                # :207-209
    c = deep_iaf(up_conv1, down_conv1, eps_down, w, name, n_h, n_z, depth)
    down_out = down_input + 0.1 * O.theano_conv2d(_elu(c["h"]), *_cw(w, name, "_down_conv2_1"))  # :325
    c.update(up_out=up_out, down_out=down_out, up_conv1=up_conv1, down_conv1=down_conv1)
    return c


def down_p_layer(name, w, n_h, n_z, down_input, eps):
    """models.py:330-359, prior 'diag' -> (down_conv1 output, concat([h_det, z]), the layer's output)"""
    down_conv1 = O.theano_conv2d(_elu(down_input), *_cw(w, name, "_down_conv1"))
    h = np.concatenate([down_conv1[:, :n_h], down_conv1[:, n_h:n_h + n_z] + eps * np.exp(down_conv1[:, n_h + n_z:n_h + 2 * n_z])], axis=1)
    return down_conv1, h, down_input + 0.1 * O.theano_conv2d(_elu(h), *_cw(w, name, "_down_conv2_1"))


free_bits = C.free_bits


# ---------------------------------------------------------------- torch fp64 (gradients)
def _conv_t(h, w, p, n_in, n_out, zerodiagonal):
    return G.theano_ar_conv2d(h, w[p + "_w"], w[p + "_b"], w[p + "_s"], n_in, n_out, zerodiagonal, False)


def resnet_torch(z, context, w, name, n_z, n_h, depth):
    h = _conv_t(z, w, name + "_input", n_z, n_h, False) + context
    for i in range(depth):
        t = F.elu(_conv_t(F.elu(h), w, "%s_%d_conv1" % (name, i), n_h, n_h, False))
        h = h + 0.1 * _conv_t(t, w, "%s_%d_conv2" % (name, i), n_h, n_h, False)
    return [_conv_t(h, w, "%s_out_%d" % (name, j), n_h, n_z, True) for j in range(2)]


def deep_step_torch(z, context, w, name, n_z, n_h, depth):
    m_raw, s_raw = resnet_torch(z, context, w, name, n_z, n_h, depth)
    m, s = 0.1 * m_raw, 0.1 * s_raw
    return (z - m) / torch.exp(s), s


def deep_step_grads(z, context, w, name, n_z, n_h, depth, dz_new, dlogsd):
    """Gradients of  L = <dz_new, z_new> + <dlogsd, logsd>  w.r.t. z, context and every _w/_s/_b of the network"""
    zt, ct = G._t(z, True), G._t(context, True)
    wt = {k: G._t(v, True) for k, v in w.items()}
    z_new, logsd = deep_step_torch(zt, ct, wt, name, n_z, n_h, depth)
    ((z_new * G._t(dz_new)).sum() + (logsd * G._t(dlogsd)).sum()).backward()
    out = {"z": zt.grad.numpy(), "context": ct.grad.numpy()}
    out.update({k: v.grad.numpy() for k, v in wt.items()})
    return out, z_new.detach().numpy(), logsd.detach().numpy()


def deep_iaf_torch(h_up, h_dn, eps, w, name, n_h, n_z, depth, kl_min):
    """-> (what up_conv2 reads, concat([h_det, z]), kl, obj_kl)"""
    h_det_u, qm, ql, uctx = torch.split(h_up, [n_h, n_z, n_z, n_h], dim=1)
    h_det, pm, pl, rm, rl, dctx = torch.split(h_dn, [n_h, n_z, n_z, n_z, n_z, n_h], dim=1)
    mean, logvar = qm + rm, 2 * ql + 2 * rl
    z0 = mean + torch.exp(0.5 * logvar) * eps
    logqs = C._logps(mean, logvar, z0)
    z, s1 = deep_step_torch(z0, uctx + dctx, w, name + "_deepiaf", n_z, n_h, depth)
    kl = logqs + s1 - C._logps(pm, 2 * pl, z)
    kl_sum = kl.sum(dim=(1, 2, 3))
    obj = torch.clamp(kl.sum(dim=(2, 3)).mean(dim=0), min=kl_min).sum() if kl_min > 0 else kl_sum
    return h_det_u, torch.cat([h_det, z], dim=1), kl, obj


def deep_iaf_grads(h_up, h_dn, eps, w, name, n_h, n_z, depth, kl_min, d_up, d_h, d_obj):
    """L = <d_up, up_out> + <d_h, h_out> + <d_obj, obj_kl>; gradients w.r.t. both conv outputs and every weight of the network"""
    ut, dt = G._t(h_up, True), G._t(h_dn, True)
    wt = {k: G._t(v, True) for k, v in w.items()}
    up_out, h_out, kl, obj = deep_iaf_torch(ut, dt, G._t(eps), wt, name, n_h, n_z, depth, kl_min)
    loss = (h_out * G._t(d_h)).sum() + (obj * G._t(d_obj)).sum()
    if d_up is not None:
        loss = loss + (up_out * G._t(d_up)).sum()
    loss.backward()
    fw = dict(up_out=up_out.detach().numpy(), h=h_out.detach().numpy(), kl=kl.detach().numpy(), obj_kl=obj.detach().numpy())
    return dict(h_up=ut.grad.numpy(), h_dn=dt.grad.numpy(), w={k: v.grad.numpy() for k, v in wt.items()}), fw


def deep_iaf_grads_by_steps(h_up, h_dn, eps, w, name, n_h, n_z, depth, kl_min, d_up, d_h, d_obj):
    """the same gradients by the decomposition CVAELayerIAF.backward runs: iaf_chain_backward_pre's contract with one log-determinant, the
    step's backward as autograd of THAT STEP ALONE with (dz_new, dlogsd) = (dz, G), iaf_chain_backward_post's with dctx2 = 0"""
    f = deep_iaf(h_up, h_dn, eps, w, name, n_h, n_z, depth)
    B = eps.shape[0]
    if kl_min > 0:
        gate = (f["kl"].sum(axis=(2, 3)).mean(axis=0) > kl_min).astype(np.float64)
        dz, Gf, d_first = C.pre_np(h_dn, f["z"], d_h, n_h, n_z, gate=gate, gscale=float(d_obj) / B)
    else:
        dz, Gf, d_first = C.pre_np(h_dn, f["z"], d_h, n_h, n_z, dko=d_obj)
    pre = name + "_deepiaf"
    sub = {k: v for k, v in w.items() if k.startswith(pre + "_")}
    g1, _, _ = deep_step_grads(f["z0"], f["context"], sub, pre, n_z, n_h, depth, dz, Gf)
    d_uc1, rest = C.post_np(h_up, h_dn, f["z0"], g1["z"], Gf, g1["context"], np.zeros_like(g1["context"]), d_up, n_h, n_z)
    return dict(h_up=d_uc1, h_dn=np.concatenate([d_first, rest], axis=1), w={k: g1[k] for k in sub})
