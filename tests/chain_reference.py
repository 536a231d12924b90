"""Reference statements for the 'down_iaf2_nl2' posterior of models.cvae_layer (models.py:93-98, 272-291): a chain of two IAF steps on one
context, posterior_conv1 with the plain ordering, posterior_conv2 with the flipped one, both log-determinants added to logqs.
TEST INFRASTRUCTURE ONLY.  Three statements:

  * NumPy fp64, composed from oracle.iaf_oracle (gaussian_diag_logps, theano_iaf2_nl(flipmask=False), theano_iaf2_nl(flipmask=True)):
    chain_iaf (between the plain convs) and chain_layer (the whole layer, as oracle.iaf_oracle.theano_cvae_layer states the others);
  * torch fp64, composed from oracle.iaf_grad_oracle.theano_iaf2_nl, for gradients: chain_iaf_torch / chain_iaf_grads;
  * the contracts of the four elementwise entry points (iaf_chain_head / _tail / _backward_pre / _backward_post, include/iaf_hip.h) in
    plain NumPy: head_np, tail_np, pre_np, post_np.

Channel orders (models.py:141-143, 273-279, 296-297):
    up_conv1 output    [h_det (n_h) | qz_mean (n_z) | qz_logsd (n_z) | up_context (n_h)]
    down_conv1 output  [h_det (n_h) | pz_mean | pz_logsd | rz_mean | rz_logsd (n_z each) | down_context (n_h)]"""
import numpy as np
import torch

from oracle import iaf_grad_oracle as G
from oracle import iaf_oracle as O

LOG2PI = float(np.log(2 * np.pi))


def _cut(a, sizes):
    out, at = [], 0
    for s in sizes:
        out.append(a[:, at:at + s])
        at += s
    assert at == a.shape[1], (at, a.shape)
    return out


# ---------------------------------------------------------------- NumPy fp64 chain
def chain_iaf(h_up, h_dn, eps, w, name, n_h, n_z, depth_ar):
    """models.py:272-291, 295-298, 317-318 between the plain convs.  Returns dict(z0, logq0, context, z1, s1, z (= z2), s2, kl, h)."""
    _, qm, ql, uctx = _cut(h_up, [n_h, n_z, n_z, n_h])
    h_det, pm, pl, rm, rl, dctx = _cut(h_dn, [n_h, n_z, n_z, n_z, n_z, n_h])
    mean, logvar = qm + rm, 2 * ql + 2 * rl                                                    # :275
    z0 = mean + np.exp(0.5 * logvar) * eps
    logq0 = O.gaussian_diag_logps(mean, logvar, z0)
    context = uctx + dctx                                                                      # :280
    z1, s1 = O.theano_iaf2_nl(z0, context, w, name + "_posterior_conv1", n_z, [n_h] * depth_ar, flipmask=False)   # :281-285
    z2, s2 = O.theano_iaf2_nl(z1, context, w, name + "_posterior_conv2", n_z, [n_h] * depth_ar, flipmask=True)    # :286-291
    kl = logq0 + s1 + s2 - O.gaussian_diag_logps(pm, 2 * pl, z2)                                # :298, 328
    return dict(z0=z0, logq0=logq0, context=context, z1=z1, s1=s1, z=z2, s2=s2, kl=kl, h=np.concatenate([h_det, z2], axis=1))


def chain_layer(name, w, n_h, n_z, depth_ar, up_input, down_input, eps_down):
    """the whole cvae_layer with posterior 'down_iaf2_nl2', prior 'diag', nl 'elu', no downsampling (eps_up is drawn by the reference
    but does not reach any output: the up pass of this posterior returns h_det only, models.py:179-181)"""
    cw = lambda nm: (w[name + nm + "_w"], w[name + nm + "_b"], w[name + nm + "_s"])
    elu = lambda t: np.where(t < 0, np.exp(np.minimum(t, 0)) - 1, t)
    up_conv1 = O.theano_conv2d(elu(up_input), *cw("_up_conv1_1"))                               # :139
    up_out = up_input + 0.1 * O.theano_conv2d(elu(up_conv1[:, :n_h]), *cw("_up_conv2"))        # :181, 191
    down_conv1 = O.theano_conv2d(elu(down_input), *cw("_down_conv1"))                           # :207-209
    c = chain_iaf(up_conv1, down_conv1, eps_down, w, name, n_h, n_z, depth_ar)
    down_out = down_input + 0.1 * O.theano_conv2d(elu(c["h"]), *cw("_down_conv2_1"))            # :325
    c.update(up_out=up_out, down_out=down_out, up_conv1=up_conv1, down_conv1=down_conv1)
    return c


def free_bits(kl, kl_min):
    """models.py:455-466 -> (kl_sum [B], obj_kl: a scalar with free bits, else kl_sum)"""
    obj, kl_sum = O.theano_free_bits(kl, kl_min)
    return kl_sum, obj


# ---------------------------------------------------------------- torch fp64 chain (gradients)
def _logps(mean, logvar, x):
    return -0.5 * (LOG2PI + logvar + (x - mean) ** 2 / torch.exp(logvar))                      # rand.py:85-86


def chain_iaf_torch(h_up, h_dn, eps, w, name, n_h, n_z, depth_ar, kl_min):
    """-> (what up_conv2 reads, concat([h_det, z2]), kl, obj_kl)"""
    h_det_u, qm, ql, uctx = torch.split(h_up, [n_h, n_z, n_z, n_h], dim=1)
    h_det, pm, pl, rm, rl, dctx = torch.split(h_dn, [n_h, n_z, n_z, n_z, n_z, n_h], dim=1)
    mean, logvar = qm + rm, 2 * ql + 2 * rl
    z0 = mean + torch.exp(0.5 * logvar) * eps
    logqs = _logps(mean, logvar, z0)
    context = uctx + dctx
    z1, s1 = G.theano_iaf2_nl(z0, context, w, name + "_posterior_conv1", n_z, [n_h] * depth_ar, False)
    z2, s2 = G.theano_iaf2_nl(z1, context, w, name + "_posterior_conv2", n_z, [n_h] * depth_ar, True)
    kl = logqs + s1 + s2 - _logps(pm, 2 * pl, z2)
    kl_sum = kl.sum(dim=(1, 2, 3))
    obj = torch.clamp(kl.sum(dim=(2, 3)).mean(dim=0), min=kl_min).sum() if kl_min > 0 else kl_sum
    return h_det_u, torch.cat([h_det, z2], dim=1), kl, obj


def chain_iaf_grads(h_up, h_dn, eps, w, name, n_h, n_z, depth_ar, kl_min, d_up, d_h, d_obj):
    """L = <d_up, up_out> + <d_h, h_out> + <d_obj, obj_kl>; gradients w.r.t. both conv outputs and every weight of both stacks."""
    ut, dt = G._t(h_up, True), G._t(h_dn, True)
    wt = {k: G._t(v, True) for k, v in w.items()}
    up_out, h_out, kl, obj = chain_iaf_torch(ut, dt, G._t(eps), wt, name, n_h, n_z, depth_ar, kl_min)
    loss = (h_out * G._t(d_h)).sum() + (obj * G._t(d_obj)).sum()
    if d_up is not None:
        loss = loss + (up_out * G._t(d_up)).sum()
    loss.backward()
    fw = dict(up_out=up_out.detach().numpy(), h=h_out.detach().numpy(), kl=kl.detach().numpy(), obj_kl=obj.detach().numpy())
    return dict(h_up=ut.grad.numpy(), h_dn=dt.grad.numpy(), w={k: v.grad.numpy() for k, v in wt.items()}), fw


# ---------------------------------------------------------------- the four entry points' contracts, NumPy
def head_np(up, down, eps, n_h, n_z):
    """-> (z0, logq0, context)"""
    _, qm, ql, uctx = _cut(up, [n_h, n_z, n_z, n_h])
    _, _, _, rm, rl, dctx = _cut(down, [n_h, n_z, n_z, n_z, n_z, n_h])
    lsd = ql + rl
    return (qm + rm) + np.exp(lsd) * eps, -0.5 * (LOG2PI + 2 * lsd + eps * eps), uctx + dctx


def tail_np(down, logq0, s1, s2, z2, n_h, n_z):
    """-> (kl_elem, h_out)"""
    h_det, pm, pl = _cut(down, [n_h, n_z, n_z, n_z, n_z, n_h])[:3]
    logp = -0.5 * (LOG2PI + 2 * pl + (z2 - pm) ** 2 * np.exp(-2 * pl))
    return logq0 + s1 + s2 - logp, np.concatenate([h_det, z2], axis=1)


def expand_G(shape, gate=None, gscale=0.0, dko=None):
    """G = d obj / d kl on [B, n_z, ...]: gate[c] * gscale (free bits) or dko[b]"""
    tail = (1,) * (len(shape) - 2)
    if gate is not None:
        return np.broadcast_to((np.asarray(gate) * gscale).reshape((1, -1) + tail), shape).copy()
    return np.broadcast_to(np.asarray(dko).reshape((-1, 1) + tail), shape).copy()


def pre_np(down, z2, d_h, n_h, n_z, gate=None, gscale=0.0, dko=None):
    """-> (dz2, G, the first n_h + 2 n_z channels of d_down_conv1)"""
    pm, pl = _cut(down, [n_h, n_z, n_z, n_z, n_z, n_h])[1:3]
    Gf = expand_G(z2.shape, gate, gscale, dko)
    e2, dlt = np.exp(-2 * pl), z2 - pm
    return d_h[:, n_h:] + Gf * dlt * e2, Gf, np.concatenate([d_h[:, :n_h], -Gf * dlt * e2, Gf * (1 - dlt * dlt * e2)], axis=1)


def post_np(up, down, z0, dz0, Gf, dctx1, dctx2, d_up, n_h, n_z):
    """-> (d_up_conv1 whole, the last 2 n_z + n_h channels of d_down_conv1)"""
    qm = _cut(up, [n_h, n_z, n_z, n_h])[1]
    rm = _cut(down, [n_h, n_z, n_z, n_z, n_z, n_h])[3]
    rest = np.concatenate([dz0, dz0 * (z0 - (qm + rm)) - Gf, dctx1 + dctx2], axis=1)
    first = d_up if d_up is not None else np.zeros_like(up[:, :n_h])
    return np.concatenate([first, rest], axis=1), rest
