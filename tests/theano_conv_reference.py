"""fp64 restatement of the plain conv of the Theano path, N.conv.conv2d(name, n_in, n_out, (3,3), w=w) with pad_channel=True, border
'valid', l2norm=True, logscale=True and no down- / upsampling (graphy/nodes/conv.py:122-260), in torch so that autograd gives its
gradients; pinned to oracle.iaf_oracle.theano_conv2d and to central finite differences by tests/test_theano_conv_reference.py.

    K[o]     = w[o] / sqrt(sum_{c <= n_in, a, b} w[o,c,a,b]^2) * exp(3 s[o])                 (no epsilon, conv.py:162-164)
    y[o,i,j] = b[o] + sum_{c < n_in, dh, dw, inside} x[c,i+dh,j+dw] K[o,c,1-dh,1-dw]          (true convolution: kernel flipped)
                    + sum_{(dh,dw) != (0,0), (i+dh,j+dw) outside} K[o,n_in,1-dh,1-dw]         (border-indicator channel, conv.py:71-83)

The border addend of a pixel depends only on which of its neighbours leave the image: 16 position classes,
class = row above out | row below out << 1 | column left out << 2 | column right out << 3 (all four at H = W = 1).

Also here: the whole models.cvae_layer (downsample=False) in torch fp64 -- the plain convs around the IAF part that
tests/chain_reference.py, deep_reference.py and made_reference.py restate -- for the gradients of iaf_amd.CVAELayer."""
import numpy as np
import torch
import torch.nn.functional as F

# the geometry table of the GPU tests: reaches all 16 position classes (test_theano_conv_reference.py proves it)
GEOMETRIES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (6, 5)]


def effective_kernel(w, s):
    """K of the statement above, OIHW [n_out, n_in + 1, 3, 3]"""
    n = torch.sqrt((w * w).sum(dim=(1, 2, 3), keepdim=True))
    return w / n * torch.exp(3.0 * s).reshape(-1, 1, 1, 1)


def border_indicator(H, W, dtype=torch.float64):
    """the padded border channel [1, 1, H+2, W+2]: 1 on the padding ring, 0 inside"""
    ind = torch.ones(1, 1, H + 2, W + 2, dtype=dtype)
    ind[:, :, 1:-1, 1:-1] = 0.0
    return ind


def conv2d(x, w, s, b, border=True, flip=True):
    """x [B, n_in, H, W], w OIHW [n_out, n_in + 1, 3, 3], s, b [n_out] (torch, any float dtype) -> [B, n_out, H, W].
    border=False drops the border addend with the norm KEPT over n_in + 1 channels; flip=False runs a cross-correlation:
    the two terms a tolerance must not hide."""
    n_in = w.shape[1] - 1
    K = effective_kernel(w, s)
    kd, kb = K[:, :n_in], K[:, n_in:]
    if flip:                                 # F.conv2d is a cross-correlation
        kd, kb = kd.flip(2, 3), kb.flip(2, 3)
    y = F.conv2d(x, kd, padding=1) + b.reshape(1, -1, 1, 1)
    if border:
        y = y + F.conv2d(border_indicator(x.shape[2], x.shape[3], x.dtype), kb)
    return y


def elu(t):
    return torch.where(t < 0, torch.exp(torch.clamp(t, max=0.0)) - 1.0, t)


def position_classes(H, W):
    """[H, W] int array of the class of every pixel"""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return ((i == 0) * 1 + (i == H - 1) * 2 + (j == 0) * 4 + (j == W - 1) * 8).astype(np.int64)


def class_addend(K, cls):
    """the border addend [n_out] of position class `cls` from the effective kernel K (numpy or torch)"""
    tot = 0.0
    for dh in (-1, 0, 1):
        for dw in (-1, 0, 1):
            if (dh, dw) == (0, 0):
                continue
            out = (dh < 0 and cls & 1) or (dh > 0 and cls & 2) or (dw < 0 and cls & 4) or (dw > 0 and cls & 8)
            if out:
                tot = tot + K[:, -1, 1 - dh, 1 - dw]
    return tot


def rand_conv(rng, n_in, n_out):
    """(w, s, b) at the fixtures' scales: 0.05 N(0,1), 0.1 N(0,1), 0.1 N(0,1)"""
    return (0.05 * rng.standard_normal((n_out, n_in + 1, 3, 3)), 0.1 * rng.standard_normal(n_out), 0.1 * rng.standard_normal(n_out))


def t64(a, grad=False):
    """fp32-rounded values as an fp64 torch tensor"""
    t = torch.from_numpy(np.asarray(a, dtype=np.float32).astype(np.float64))
    return t.requires_grad_(True) if grad else t


def conv_grads(x, w, s, b, dy, x2=None, elu_input=False, residual=False):
    """autograd of  L = <dy, out>  with out = [x +] [0.1] conv2d([elu](concat(x, x2)), w, s, b)  (residual: the `input + 0.1 h` form with
    x as the residual, x2 None) -> dict(y, dx, dx2, dw, ds, db), numpy fp64"""
    xt, wt, st, bt = t64(x, True), t64(w, True), t64(s, True), t64(b, True)
    x2t = t64(x2, True) if x2 is not None else None
    a = xt if x2t is None else torch.cat([xt, x2t], dim=1)
    y = conv2d(elu(a) if elu_input else a, wt, st, bt)
    out = xt + 0.1 * y if residual else y
    (out * t64(dy)).sum().backward()
    g = lambda t: None if t is None else t.grad.numpy()
    return dict(y=out.detach().numpy(), dx=g(xt), dx2=g(x2t), dw=g(wt), ds=g(st), db=g(bt))


# ---------------------------------------------------------------- the whole layer
def conv_widths(n_h, n_z, posterior, prior):
    """(n_in, n_out) of the four plain convs of models.cvae_layer, downsample=False (models.py:25-29, 59-108)"""
    n_up1 = 2 * n_h + 2 * n_z
    n_up2_in = n_h + n_z if posterior == "up_iaf2_nl" else n_h
    if prior == "made":
        n_down1 = 3 * n_h + 2 * n_z
    else:
        n_down1 = n_h + 2 * n_z if posterior == "up_iaf2_nl" else 2 * n_h + 4 * n_z
    return {"_up_conv1_1": (n_h, n_up1), "_up_conv2": (n_up2_in, n_h), "_down_conv1": (n_h, n_down1), "_down_conv2_1": (n_h + n_z, n_h)}


def rand_layer_convs(rng, name, n_h, n_z, posterior, prior):
    w = {}
    for nm, (n_in, n_out) in conv_widths(n_h, n_z, posterior, prior).items():
        w[name + nm + "_w"], w[name + nm + "_s"], w[name + nm + "_b"] = rand_conv(rng, n_in, n_out)
    return w


def layer_torch(name, w, up_input, down_input, iaf):
    """models.py:138-194, 201-328 around the IAF part: iaf(up_conv1 output, down_conv1 output) -> (what up_conv2 reads, concat([h_det, z]),
    kl, obj_kl), torch.  Returns (up_out, down_out, kl, obj_kl)."""
    cw = lambda nm: (w[name + nm + "_w"], w[name + nm + "_s"], w[name + nm + "_b"])
    h_up = conv2d(elu(up_input), *cw("_up_conv1_1"))
    h_dn = conv2d(elu(down_input), *cw("_down_conv1"))
    hu, hd, kl, obj = iaf(h_up, h_dn)
    up_out = up_input + 0.1 * conv2d(elu(hu), *cw("_up_conv2"))
    down_out = down_input + 0.1 * conv2d(elu(hd), *cw("_down_conv2_1"))
    return up_out, down_out, kl, obj
