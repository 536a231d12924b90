"""The IAF part of the reference's Theano layer, models.cvae_layer (models.py:14-345), priors 'diag' and 'made', for the two posteriors
BASELINE names -- 'down_iaf2_nl' (configs 0-2, 4) and 'up_iaf2_nl' (config 3) -- and for 'down_iaf2_nl2' (models.py:93-98, 272-291): a CHAIN
of two IAF steps on one context, posterior_conv1 with the plain ordering and posterior_conv2 with the flipped one, both log-determinants
added to logqs -- the construction of the IAF paper, in which no latent stays first in every ordering.

Two classes.  CVAELayerIAF is the IAF part BETWEEN the plain Theano convs (up_conv1/2, down_conv1/2: graphy/nodes/conv.py:122-260):
it takes THEIR OUTPUTS in the reference's channel order and returns what the next conv consumes.  CVAELayer (at the end of this
file) is the whole models.cvae_layer with downsample=False: it owns a CVAELayerIAF and the four convs (layers.WNConv2d(theano=True),
iaf_conv3x3_create_theano), loads a Theano weight dict and runs up / down_q / down_p and the two-phase backward on the device.
The channel layouts between the convs and the IAF part:

    up_conv1 output    [h_det (n_h) | qz_mean (n_z) | qz_logsd (n_z) | context (n_h)]            models.py:139-143, 164/181
    down_conv1 output  [h_det (n_h) | pz_mean (n_z) | pz_logsd (n_z) || rz_mean | rz_logsd | down_context (n_h)]  :273-279, 296-297
    next conv's input  concat([h_det, z])  (the TF path concatenates [z, h_det])                  :180, 318

'down_iaf2_nl2' has the channel layouts of 'down_iaf2_nl'.  Its two steps are two launches of the existing step kernels (ARStack.iaf_step
/ iaf_step_train / iaf_step_backward); what lies between and around them -- the reparametrised sample and its density, the summed
context, the KL, concat([h_det, z]), and the two elementwise halves of the backward pass -- is four launches (iaf_chain_head / _tail /
_backward_pre / _backward_post) that read their operands at channel offsets INSIDE the two conv outputs and write the gradients of the
conv outputs whole: no split() copies, no torch.cat.

'down_iaf2_deep' (models.py:104-108, 272-285) also has the channel layouts of 'down_iaf2_nl' and prior 'diag': ONE IAF step whose
autoregressive network is the masked ResNet N.ar.resnet(name + '_deepiaf', depth_ar, n_z, n_h, [n_z, n_z]) (graphy/nodes/ar.py:428-448, 478-528)
-- h_0 = conv_input(z) + context, depth_ar blocks h <- h + 0.1 conv2(elu(conv1(elu(h)))), the (mean, logsd) pair on the raw h -- on a
layers.ResnetARStack; load() reads w[name + '_deepiaf_input_w|_s|_b'], '..._<i>_conv1_...', '..._<i>_conv2_...', '..._out_<j>_...'.  The
step is 2 depth_ar + 2 launches of the conv kernels; around it are the chain's four elementwise launches with a second log-determinant
(and, backwards, a second context gradient) of cached zeros, so down_q is capturable after a warm-up as the chain is.  depth_ar is 1 to 4,
the ordering the plain one (flipmask=True: UnsupportedError), and prior 'made' with it raises ValueError.

prior='made' (models.py:36-38, 304-309; with 'down_iaf2_nl' and 'down_iaf2_nl2') is the autoregressive prior: a further stack,
<name>_prior_conv1 with the plain ordering, reads z and a context of its own, and down_conv1 emits that context in place of the prior's
mean and log standard deviation:

    up_conv1 output    [h_det (n_h) | qz_mean (n_z) | qz_logsd (n_z) | up_context (n_h)]                         unchanged
    down_conv1 output  [h_det (n_h) | made_context (n_h) | rz_mean (n_z) | rz_logsd (n_z) | down_context (n_h)]   :38, 273-279, 305

With (u, s_p) = prior_stack.iaf_step(z, made_context) the prior's density is logps = -(log 2pi)/2 - s_p - u^2/2, so the density is one
more launch of the step kernels and its gradient one more iaf_step_backward; iaf_made_head / _tail / _backward_pre / _backward_join /
_backward_post are the elementwise launches around the steps.  down_p() (models.py:330-359) samples the prior: the reference leaves
z = eps for 'made' (:338-340); exact=True solves z = 0.1 m(z) + exp(0.1 s(z)) eps with the stack's inverse step, the ancestral sample.
The engine states the Theano operator for channel counts that are multiples of 16; with prior 'made' the plain-ordering stacks (the
prior's, and the posterior's first unless flipmask) of a layer with smaller counts and n_z | n_h run embedded in wider ones
(layers.EmbeddedTheanoStack): the same values and gradients, at the price of torch pad and slice copies around every step.  The flipped
ordering does not embed, so flipmask=True and 'down_iaf2_nl2' stay UnsupportedError at such sizes.

The masked-AR convs run on the GPU through the Theano statement of the operator (IAF_VARIANT_THEANO[_FLIPMASK]); the free
bits follow models.py:454-466 (a SCALAR per layer: sum over channels of max(kl_min, batch-mean of the per-channel KL))."""
import ctypes

import torch

from . import _capi
from .distributions import gaussian_diag_logps_logsd
from .iaf_layer import gaussian_sample
from .layers import (ARStack, ConvPrepBatch, PrepBatch, ResnetARStack, WNConv2d, kl_free_bits, split, theano_stack, _check_act, _ptr,
                     _stream)

POSTERIORS = ("down_iaf2_nl", "up_iaf2_nl", "down_iaf2_nl2", "down_iaf2_deep")
PRIORS = ("diag", "made")


class CVAELayerIAF(object):
    def __init__(self, name, n_h, n_z, depth_ar, posterior="down_iaf2_nl", flipmask=False, kl_min=0.0, prior="diag"):
        if prior not in PRIORS:
            raise Exception("Unknown prior")                                      # models.py:43
        if posterior not in POSTERIORS:
            raise Exception("Unknown posterior " + posterior)                     # models.py:115
        if prior == "made" and posterior == "up_iaf2_nl":
            raise ValueError("prior 'made' with posterior 'up_iaf2_nl' is not built: use 'down_iaf2_nl' or 'down_iaf2_nl2'")
        if prior == "made" and posterior == "down_iaf2_deep":
            raise ValueError("prior 'made' with posterior 'down_iaf2_deep' is not built: use prior 'diag'")
        self.name, self.n_h, self.n_z, self.depth_ar = name, int(n_h), int(n_z), int(depth_ar)
        self.posterior, self.kl_min, self.prior = posterior, float(kl_min), prior
        self._st, self._rel, self._rel2, self._rel_p, self._zeros = None, None, None, None, {}
        self.training = False
        self.stack2, self._prep, self.prior_stack = None, None, None
        if posterior == "down_iaf2_deep":
            # models.py:104-108: N.ar.resnet(name + '_deepiaf', depth_ar, n_z, n_h, [n_z, n_z], kernel, False): depth_ar counts residual
            # blocks here, and the ordering is always the plain one
            if flipmask:
                raise _capi.UnsupportedError("'down_iaf2_deep' has the plain ordering only (resnet_layer_a passes no flipmask, ar.py:434-435)")
            self.stack = ResnetARStack(self.n_z, self.n_h, self.depth_ar)
            return
        # With prior 'made', BOTH plain-ordering stacks (this one unless flipmask, and the prior's) may have channel counts that are not
        # multiples of 16 (n_z | n_h): theano_stack then returns an EmbeddedTheanoStack, which pads and slices with torch around
        # every step.  The flipped ordering does not embed: flipmask=True and 'down_iaf2_nl2' raise UnsupportedError at such sizes.
        self.stack = theano_stack(self.n_z, [self.n_h] * self.depth_ar,
                                  _capi.IAF_VARIANT_THEANO_FLIPMASK if flipmask else _capi.IAF_VARIANT_THEANO, embed=(prior == "made"))
        # the second flow of the chain is ALWAYS flipped (models.py:98 hard-codes True); `flipmask` is the first flow's
        if posterior == "down_iaf2_nl2":
            if self.depth_ar < 1:
                raise ValueError("'down_iaf2_nl2' needs depth_ar >= 1: both flows take the context through their first conv")
            self.stack2 = ARStack(self.n_z, [self.n_h] * self.depth_ar, variant=_capi.IAF_VARIANT_THEANO_FLIPMASK)
        # the MADE prior's stack always has the plain ordering (models.py:37 hard-codes False)
        if prior == "made":
            if self.depth_ar < 1:
                raise ValueError("prior 'made' needs depth_ar >= 1: the prior's stack takes made_context through its first conv")
            self.prior_stack = theano_stack(self.n_z, [self.n_h] * self.depth_ar, _capi.IAF_VARIANT_THEANO, embed=True)

    def set_training(self, on=True):
        """keep what backward() needs in up() / down_q() (call load() again afterwards: the data-gradient weight packs are
        written by the next prepare)"""
        self.stack.set_training(on)
        if self.stack2 is not None:
            self.stack2.set_training(on)
        if self.prior_stack is not None:
            self.prior_stack.set_training(on)
        self.training = bool(on)

    def load(self, w):
        """w: the reference's parameter dict; reads w[name + '_posterior_conv1_<i>_w|_b|_s'] and '..._out_<i>_...', for
        'down_iaf2_nl2' also w[name + '_posterior_conv2_...'], for prior 'made' also w[name + '_prior_conv1_...'] (all stacks
        prepared in ONE launch)"""
        pre = self.name + ("_deepiaf_" if self.posterior == "down_iaf2_deep" else "_posterior_conv1_")
        self._rel = {k[len(pre):]: v for k, v in w.items() if k.startswith(pre)}
        if self.stack2 is None and self.prior_stack is None:
            self.stack.prepare(self._rel)
            return
        stacks, rels = [self.stack], [self._rel]
        if self.stack2 is not None:
            pre2 = self.name + "_posterior_conv2_"
            self._rel2 = {k[len(pre2):]: v for k, v in w.items() if k.startswith(pre2)}
            stacks.append(self.stack2)
            rels.append(self._rel2)
        if self.prior_stack is not None:
            prep = self.name + "_prior_conv1_"
            self._rel_p = {k[len(prep):]: v for k, v in w.items() if k.startswith(prep)}
            stacks.append(self.prior_stack)
            rels.append(self._rel_p)
        if self._prep is None:
            self._prep = PrepBatch(stacks)
        self._prep.run(rels)

    def up(self, h, eps=None):
        """h: output of up_conv1 [B, 2 n_h + 2 n_z, H, W].  Returns the input of up_conv2 (before its nonlinearity):
        h_det for 'down_iaf2_nl' (models.py:180-182), concat([h_det, z]) for 'up_iaf2_nl' (:168-176; needs eps)."""
        n_h, n_z = self.n_h, self.n_z
        if self.posterior in ("down_iaf2_nl2", "down_iaf2_deep") or self.prior == "made":
            # as 'down_iaf2_nl' (models.py:179-181); the chain's kernels read the conv output itself, so what is kept of it are views
            _check_act(h, "h (up_conv1 output)")
            if h.dim() != 4 or h.shape[1] != 2 * n_h + 2 * n_z:
                raise ValueError("h must be [B, %d, H, W], got %s" % (2 * n_h + 2 * n_z, tuple(h.shape)))
            self._st = dict(up_conv1=h, qz_mean=h.narrow(1, n_h, n_z), qz_logsd=h.narrow(1, n_h + n_z, n_z),
                            context=h.narrow(1, n_h + 2 * n_z, n_h))
            return h.narrow(1, 0, n_h).contiguous()
        h_det, qz_mean, qz_logsd, context = split(h, 1, [n_h, n_z, n_z, n_h])
        st = dict(qz_mean=qz_mean, qz_logsd=qz_logsd, context=context)
        if self.posterior == "up_iaf2_nl":
            if eps is None:
                raise ValueError("'up_iaf2_nl' samples the posterior in the up pass: pass eps")
            z0 = gaussian_sample(qz_mean, qz_logsd, eps)                                          # rand.py:81-83
            logq0 = gaussian_diag_logps_logsd(qz_mean, qz_logsd, z0)                              # rand.py:85-86
            z, logdet = (self.stack.iaf_step_train if self.training else self.stack.iaf_step)(z0, context)   # models.py:170-173
            st.update(z=z, logq0=logq0, logdet=logdet, z0=z0, eps=eps)
            out = torch.cat([h_det, z], dim=1)                                                    # :176
        else:
            out = h_det
        self._st = st
        return out

    def down_q(self, h, eps=None):
        """h: output of down_conv1 [B, 2 n_h + 4 n_z, H, W] ('down_iaf2_nl', 'down_iaf2_nl2') or [B, n_h + 2 n_z, H, W] ('up_iaf2_nl').
        Returns dict(h = concat([h_det, z]) for down_conv2, kl [B, n_z, H, W] = logqs - logps (:328), kl_sum [B] (:455),
        obj_kl (:458-466: scalar tensor when kl_min > 0, else kl_sum)).  With prior 'made' h is [B, 3 n_h + 2 n_z, H, W]."""
        n_h, n_z, st = self.n_h, self.n_z, self._st
        if self.prior == "made":
            return self._down_q_made(h, eps)
        if self.posterior in ("down_iaf2_nl2", "down_iaf2_deep"):
            return self._down_q_chain(h, eps)
        if self.posterior == "down_iaf2_nl":
            h_det, pz_mean, pz_logsd, rz_mean, rz_logsd, down_context = split(h, 1, [n_h, n_z, n_z, n_z, n_z, n_h])
            if self.training:
                blk = self.stack.posterior_block_train(st["qz_mean"], st["qz_logsd"], rz_mean, rz_logsd, pz_mean, pz_logsd,
                                                       st["context"], down_context, eps, self.kl_min)
                st.update(rz_mean=rz_mean, rz_logsd=rz_logsd, pz_mean=pz_mean, pz_logsd=pz_logsd, eps=eps, z=blk["z"])
                obj_kl = blk["kl_obj"][0] if self.kl_min > 0 else blk["kl_cost"]
                return dict(h=torch.cat([h_det, blk["z"]], dim=1), z=blk["z"], kl=None, kl_sum=blk["kl_cost"], obj_kl=obj_kl)
            blk = self.stack.posterior_block(st["qz_mean"], st["qz_logsd"], rz_mean, rz_logsd, pz_mean, pz_logsd, st["context"],
                                             down_context, eps, self.kl_min, want_kl_elem=True)   # :272-285, 296-298
            z, kl, kl_sum, kl_obj = blk["z"], blk["kl_elem"], blk["kl_cost"], blk["kl_obj"]
        else:
            h_det, pz_mean, pz_logsd = split(h, 1, [n_h, n_z, n_z])
            z = st["z"]                                                                           # :216-217
            logp = gaussian_diag_logps_logsd(pz_mean, pz_logsd, z)                                # :298
            kl = torch.empty_like(z)
            _capi.check(_capi.lib().iaf_kl_combine(_ptr(st["logq0"]), _ptr(st["logdet"]), _ptr(logp), _ptr(kl), kl.numel(),
                                                   _stream()))
            if self.training and self.kl_min > 0:        # the gate of the free bits is what backward() multiplies with
                kl_sum, kl_obj, gate = kl_free_bits(kl, self.kl_min, want_gate=True)
                st["gate"] = gate
            else:
                kl_sum, kl_obj = kl_free_bits(kl, self.kl_min)
            st.update(pz_mean=pz_mean, pz_logsd=pz_logsd, kl=kl)
        # TF: kl_obj[b] = sum_c max(mean_b sum_hw kl, kl_min) for every b (tf_train.py:79-82); Theano adds that SCALAR
        # once per layer (models.py:460-461)
        obj_kl = kl_obj[0] if self.kl_min > 0 else kl_sum
        return dict(h=torch.cat([h_det, z], dim=1), z=z, kl=kl, kl_sum=kl_sum, obj_kl=obj_kl)

    def _down_q_chain(self, h, eps):
        """'down_iaf2_nl2' (models.py:272-291, 295-298, 317-318): iaf_chain_head, the two steps, iaf_chain_tail, the free bits -- launches
        on the current stream only (no torch arithmetic, no host synchronisation: capturable after a warm-up on the capturing stream)"""
        n_h, n_z, st = self.n_h, self.n_z, self._st
        if st is None or "up_conv1" not in st:
            raise RuntimeError("down_q() follows up()")
        if eps is None:
            raise ValueError("'%s' samples the posterior in the down pass: pass eps" % self.posterior)
        up = st["up_conv1"]
        B, H, W = int(up.shape[0]), int(up.shape[2]), int(up.shape[3])
        _check_act(h, "h (down_conv1 output)", (B, 2 * n_h + 4 * n_z, H, W))
        _check_act(eps, "eps", (B, n_z, H, W))
        z0, logq0 = torch.empty_like(eps), torch.empty_like(eps)
        context = torch.empty(B, n_h, H, W, dtype=torch.float32, device=h.device)
        _capi.check(_capi.lib().iaf_chain_head(_ptr(up), _ptr(h), _ptr(eps), _ptr(z0), _ptr(logq0), _ptr(context), B, n_h, n_z, H * W,
                                               _stream()))
        z1, s1 = (self.stack.iaf_step_train if self.training else self.stack.iaf_step)(z0, context)       # :281-285
        if self.stack2 is not None:
            z2, s2 = (self.stack2.iaf_step_train if self.training else self.stack2.iaf_step)(z1, context)     # :286-291
        else:       # 'down_iaf2_deep': ONE flow; the chain's tail adds a second log-determinant of zeros (x + 0 is x, bit for bit)
            z2, s2 = z1, self._zero(z1)
        kl = torch.empty_like(eps)
        h_out = torch.empty(B, n_h + n_z, H, W, dtype=torch.float32, device=h.device)
        _capi.check(_capi.lib().iaf_chain_tail(_ptr(h), _ptr(logq0), _ptr(s1), _ptr(s2), _ptr(z2), _ptr(kl), _ptr(h_out), B, n_h, n_z,
                                               H * W, _stream()))
        st.pop("gate", None)
        if self.training and self.kl_min > 0:            # the gate of the free bits is what backward() multiplies with
            kl_sum, kl_obj, st["gate"] = kl_free_bits(kl, self.kl_min, want_gate=True)
        else:
            kl_sum, kl_obj = kl_free_bits(kl, self.kl_min)
        st.update(down_conv1=h, z0=z0, context_sum=context, z1=z1, s1=s1, z=z2, s2=s2)
        obj_kl = kl_obj[0] if self.kl_min > 0 else kl_sum                                                  # :458-466
        return dict(h=h_out, z=z2, kl=kl, kl_sum=kl_sum, obj_kl=obj_kl)

    def _backward_chain(self, d_h, d_obj, d_up):
        """T.grad through the chain: iaf_chain_backward_pre, the two steps' backward in reverse order, iaf_chain_backward_post.  Both
        steps see the same G = d obj / d kl as the gradient of their log-determinant, and their context gradients add up.  A d_obj given
        as a host number (free bits) keeps the stream free of host synchronisation."""
        n_h, n_z, st = self.n_h, self.n_z, self._st
        z2, up, down = st["z"], st["up_conv1"], st["down_conv1"]
        B, H, W = int(z2.shape[0]), int(z2.shape[2]), int(z2.shape[3])
        _check_act(d_h, "d_h", (B, n_h + n_z, H, W))
        if d_up is not None:
            _check_act(d_up, "d_up", (B, n_h, H, W))
        free_bits = self.kl_min > 0
        if free_bits:
            if "gate" not in st:
                raise RuntimeError("backward() with free bits follows down_q() in training mode")
            gate, dko = st["gate"], None
            gscale = (1.0 if d_obj is None else float(d_obj)) / B    # obj_kl is ONE scalar per layer (models.py:460-461)
        else:
            gate, gscale = None, 0.0
            dko = torch.ones(B, dtype=torch.float32, device=z2.device) if d_obj is None else d_obj
            _check_act(dko, "d_obj", (B,))
        dz2, G = torch.empty_like(z2), torch.empty_like(z2)
        d_dc1 = torch.empty_like(down)
        d_uc1 = torch.empty_like(up)
        _capi.check(_capi.lib().iaf_chain_backward_pre(_ptr(down), _ptr(z2), _ptr(d_h), _ptr(gate), gscale, _ptr(dko), _ptr(dz2), _ptr(G),
                                                       _ptr(d_dc1), B, n_h, n_z, H * W, _stream()))
        ctx = st["context_sum"]
        if self.stack2 is not None:
            dz1, dctx2, grads2 = self.stack2.iaf_step_backward(st["z1"], ctx, z2, st["s2"], dz2, G, self._rel2)
        else:       # 'down_iaf2_deep': one flow; the second context gradient of iaf_chain_backward_post is zeros
            dz1, dctx2, grads2 = dz2, self._zero(ctx), None
        dz0, dctx1, grads1 = self.stack.iaf_step_backward(st["z0"], ctx, st["z1"], st["s1"], dz1, G, self._rel)
        _capi.check(_capi.lib().iaf_chain_backward_post(_ptr(up), _ptr(down), _ptr(st["z0"]), _ptr(dz0), _ptr(G), _ptr(dctx1), _ptr(dctx2),
                                                        _ptr(d_up), _ptr(d_uc1), _ptr(d_dc1), B, n_h, n_z, H * W, _stream()))
        if grads2 is None:
            return dict(d_up_conv1=d_uc1, d_down_conv1=d_dc1, grads={self.name + "_deepiaf_" + k: v for k, v in grads1.items()})
        grads = {self.name + "_posterior_conv1_" + k: v for k, v in grads1.items()}
        grads.update({self.name + "_posterior_conv2_" + k: v for k, v in grads2.items()})
        return dict(d_up_conv1=d_uc1, d_down_conv1=d_dc1, grads=grads)

    def _zero(self, like):
        """a cached tensor of zeros with the shape of `like` (made on first use: warm up before a capture)"""
        key = (tuple(like.shape), like.device)
        if key not in self._zeros:
            self._zeros[key] = torch.zeros_like(like)
        return self._zeros[key]

    def _down_q_made(self, h, eps):
        """prior 'made' (models.py:272-291, 304-309, 317-318): iaf_made_head, the posterior's one or two steps, the prior's step on
        (z, made_context), iaf_made_tail, the free bits.  Everything is ordered on the current stream and nothing synchronises with the
        host, so the call is capturable after a warm-up on the capturing stream.  With channel counts that are multiples of 16 these are
        the library's launches alone, with no torch arithmetic; embedded stacks (smaller counts) add torch's zero fills and strided
        copies around every step."""
        n_h, n_z, st = self.n_h, self.n_z, self._st
        if st is None or "up_conv1" not in st:
            raise RuntimeError("down_q() follows up()")
        if eps is None:
            raise ValueError("'%s' samples the posterior in the down pass: pass eps" % self.posterior)
        up = st["up_conv1"]
        B, H, W = int(up.shape[0]), int(up.shape[2]), int(up.shape[3])
        _check_act(h, "h (down_conv1 output)", (B, 3 * n_h + 2 * n_z, H, W))
        _check_act(eps, "eps", (B, n_z, H, W))
        lib = _capi.lib()
        z0, logq0 = torch.empty_like(eps), torch.empty_like(eps)
        context = torch.empty(B, n_h, H, W, dtype=torch.float32, device=h.device)
        made_context = torch.empty_like(context)
        _capi.check(lib.iaf_made_head(_ptr(up), _ptr(h), _ptr(eps), _ptr(z0), _ptr(logq0), _ptr(context), _ptr(made_context), B, n_h, n_z,
                                      H * W, _stream()))
        step = lambda s: s.iaf_step_train if self.training else s.iaf_step
        z1, s1 = step(self.stack)(z0, context)                                                            # :281-285
        z, s2 = step(self.stack2)(z1, context) if self.stack2 is not None else (z1, None)                 # :286-291
        u, s_p = step(self.prior_stack)(z, made_context)                                                  # :305-308
        kl = torch.empty_like(eps)
        h_out = torch.empty(B, n_h + n_z, H, W, dtype=torch.float32, device=h.device)
        _capi.check(lib.iaf_made_tail(_ptr(h), _ptr(logq0), _ptr(s1), _ptr(s2), _ptr(z), _ptr(u), _ptr(s_p), _ptr(kl), _ptr(h_out), B, n_h,
                                      n_z, H * W, _stream()))
        st.pop("gate", None)
        if self.training and self.kl_min > 0:            # the gate of the free bits is what backward() multiplies with
            kl_sum, kl_obj, st["gate"] = kl_free_bits(kl, self.kl_min, want_gate=True)
        else:
            kl_sum, kl_obj = kl_free_bits(kl, self.kl_min)
        st.update(down_conv1=h, z0=z0, context_sum=context, made_context=made_context, z1=z1, s1=s1, z=z, s2=s2, u=u, s_p=s_p)
        obj_kl = kl_obj[0] if self.kl_min > 0 else kl_sum                                                  # :458-466
        return dict(h=h_out, z=z, kl=kl, kl_sum=kl_sum, obj_kl=obj_kl)

    def _backward_made(self, d_h, d_obj, d_up):
        """T.grad with prior 'made': kl holds s_p + u^2/2 of the prior's step, so that step's backward runs first with (dz_new, dlogsd) =
        (G u, G) (iaf_made_backward_pre); its dz joins the z part of d_h (iaf_made_backward_join); then the posterior's steps in reverse
        order, each with dlogsd = G, and iaf_made_backward_post.  d_obj as in _backward_chain."""
        n_h, n_z, st = self.n_h, self.n_z, self._st
        z, up, down = st["z"], st["up_conv1"], st["down_conv1"]
        B, H, W = int(z.shape[0]), int(z.shape[2]), int(z.shape[3])
        _check_act(d_h, "d_h", (B, n_h + n_z, H, W))
        if d_up is not None:
            _check_act(d_up, "d_up", (B, n_h, H, W))
        free_bits = self.kl_min > 0
        if free_bits:
            if "gate" not in st:
                raise RuntimeError("backward() with free bits follows down_q() in training mode")
            gate, dko = st["gate"], None
            gscale = (1.0 if d_obj is None else float(d_obj)) / B    # obj_kl is ONE scalar per layer (models.py:460-461)
        else:
            gate, gscale = None, 0.0
            dko = torch.ones(B, dtype=torch.float32, device=z.device) if d_obj is None else d_obj
            _check_act(dko, "d_obj", (B,))
        lib = _capi.lib()
        du, G, dz = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
        d_dc1 = torch.empty_like(down)
        d_uc1 = torch.empty_like(up)
        _capi.check(lib.iaf_made_backward_pre(_ptr(st["u"]), _ptr(d_h), _ptr(gate), gscale, _ptr(dko), _ptr(du), _ptr(G), _ptr(d_dc1), B,
                                              n_h, n_z, H * W, _stream()))
        dz_p, d_mctx, grads_p = self.prior_stack.iaf_step_backward(z, st["made_context"], st["u"], st["s_p"], du, G, self._rel_p)
        _capi.check(lib.iaf_made_backward_join(_ptr(d_h), _ptr(dz_p), _ptr(d_mctx), _ptr(dz), _ptr(d_dc1), B, n_h, n_z, H * W, _stream()))
        ctx = st["context_sum"]
        grads = {self.name + "_prior_conv1_" + k: v for k, v in grads_p.items()}
        dctx2 = None
        if self.stack2 is not None:
            dz, dctx2, grads2 = self.stack2.iaf_step_backward(st["z1"], ctx, z, st["s2"], dz, G, self._rel2)
            grads.update({self.name + "_posterior_conv2_" + k: v for k, v in grads2.items()})
        dz0, dctx1, grads1 = self.stack.iaf_step_backward(st["z0"], ctx, st["z1"], st["s1"], dz, G, self._rel)
        grads.update({self.name + "_posterior_conv1_" + k: v for k, v in grads1.items()})
        _capi.check(lib.iaf_made_backward_post(_ptr(up), _ptr(down), _ptr(st["z0"]), _ptr(dz0), _ptr(G), _ptr(dctx1), _ptr(dctx2),
                                               _ptr(d_up), _ptr(d_uc1), _ptr(d_dc1), B, n_h, n_z, H * W, _stream()))
        return dict(d_up_conv1=d_uc1, d_down_conv1=d_dc1, grads=grads)

    def down_p(self, h, eps, exact=True, max_sweeps=64, tol=1e-6, check_every=4, stats=None):
        """models.py:330-359 between the plain convs: h is the output of down_conv1 (in this layer's layout), eps [B, n_z, H, W] the
        noise; returns concat([h_det, z]) for down_conv2.  prior 'diag': z = pz_mean + eps exp(pz_logsd) (:334-337).  prior 'made':
        exact=False is the reference, z = eps (:338-340, 'TODO: SAMPLES FROM MADE PRIOR'); exact=True is the ancestral sample
        z_i ~ N(0.1 m_i(z_<i), exp(2 * 0.1 s_i(z_<i))), the solution of z = 0.1 m(z) + exp(0.1 s(z)) eps, by the prior stack's queued
        inverse step (Jacobi sweeps; max_sweeps, tol, check_every and stats as ARStack.iaf_step_inverse_queued: exact after H W n_z
        sweeps for any weights).  Ordered on the current stream with no host synchronisation: capturable after a warm-up.  Beside the
        library's launches, exact=True makes one torch copy (the contiguous made_context), and an embedded prior stack pads and slices
        with torch."""
        n_h, n_z = self.n_h, self.n_z
        _check_act(h, "h (down_conv1 output)")
        if self.prior == "made":
            n_down = 3 * n_h + 2 * n_z
        else:
            n_down = n_h + 2 * n_z if self.posterior == "up_iaf2_nl" else 2 * n_h + 4 * n_z
        if h.dim() != 4 or h.shape[1] != n_down:
            raise ValueError("h must be [B, %d, H, W], got %s" % (n_down, tuple(h.shape)))
        B, H, W = int(h.shape[0]), int(h.shape[2]), int(h.shape[3])
        _check_act(eps, "eps", (B, n_z, H, W))
        lib = _capi.lib()
        h_out = torch.empty(B, n_h + n_z, H, W, dtype=torch.float32, device=h.device)
        if self.prior == "diag":
            _capi.check(lib.iaf_diag_prior_sample(_ptr(h), _ptr(eps), _ptr(h_out), B, n_down, n_h, n_z, H * W, _stream()))
            return h_out
        z = eps
        if exact:
            made_context = h.narrow(1, n_h, n_h).contiguous()
            z, _ = self.prior_stack.iaf_step_inverse_queued(eps, made_context, max_sweeps=max_sweeps, tol=tol, check_every=check_every,
                                                            stats=stats)
        _capi.check(lib.iaf_made_tail(_ptr(h), None, None, None, _ptr(z), None, None, None, _ptr(h_out), B, n_h, n_z, H * W, _stream()))
        return h_out

    def backward(self, d_h, d_obj=None, d_up=None):
        """T.grad (graphy/misc/optim.py:102) of  <d_up, up()> + <d_h, down_q()['h']> + <d_obj, obj_kl>  through the lines
        models.py:139-146,168-176,272-298,454-466.  Must follow up() and down_q() in training mode on the same inputs.
        d_h: gradient of concat([h_det, z]) [B, n_h + n_z, H, W];  d_up: gradient of what up() returned (None = zeros);
        d_obj: gradient of obj_kl (a scalar with free bits, [B] without; None = ones).  Returns dict(d_up_conv1, d_down_conv1
        -- gradients of the two conv outputs in the reference's channel order -- and grads keyed like the reference's w)."""
        if not self.training or self._st is None or "z" not in self._st:
            raise RuntimeError("backward() follows up() and down_q() in training mode")
        if self.prior == "made":
            return self._backward_made(d_h, d_obj, d_up)
        if self.posterior in ("down_iaf2_nl2", "down_iaf2_deep"):
            return self._backward_chain(d_h, d_obj, d_up)
        n_h, n_z, st = self.n_h, self.n_z, self._st
        z = st["z"]
        B = z.shape[0]
        d_hdet, dz = d_h[:, :n_h], d_h[:, n_h:].contiguous()
        if self.kl_min > 0:      # obj_kl is ONE scalar per layer (models.py:460-461): d obj / d kl[b,c,:,:] = gate[c] / B
            dko = torch.zeros(B, dtype=torch.float32, device=z.device)
            dko[0] = 1.0 if d_obj is None else float(d_obj)
        else:
            dko = torch.ones(B, dtype=torch.float32, device=z.device) if d_obj is None else d_obj.contiguous()
        pre = self.name + "_posterior_conv1_"
        if self.posterior == "down_iaf2_nl":
            bw = self.stack.posterior_block_backward(st["qz_mean"], st["qz_logsd"], st["rz_mean"], st["rz_logsd"], st["pz_mean"],
                                                     st["pz_logsd"], st["eps"], self.kl_min, z, dz, dko, self._rel)
            d_up_hdet = d_up if d_up is not None else torch.zeros_like(d_hdet)
            d_uc1 = torch.cat([d_up_hdet, bw["dmean"], bw["dlogsd"], bw["dcontext"]], dim=1)                     # :141-143
            d_dc1 = torch.cat([d_hdet, bw["dpz_mean"], bw["dpz_logsd"], bw["dmean"], bw["dlogsd"], bw["dcontext"]], dim=1)
            grads = bw["grads"]
        else:
            # kl = logq0 + logdet - logp(z): gate the per-element gradient G as the free bits prescribe, push it through
            # logp (prior side and z), the IAF step, and the reparametrised sample z0 = qz_mean + exp(qz_logsd) eps -- two
            # elementwise launches around iaf_step_backward (iaf_up_iaf2_backward_pre / _post); tensors are storage only
            H, W = int(z.shape[2]), int(z.shape[3])
            d_h = d_h.contiguous()
            d_up_c = d_up.contiguous() if d_up is not None else None
            dz_tot, G = torch.empty_like(z), torch.empty_like(z)
            d_dc1 = torch.empty(B, n_h + 2 * n_z, H, W, dtype=torch.float32, device=z.device)
            free_bits = self.kl_min > 0
            if free_bits and "gate" not in st:
                raise RuntimeError("backward() with free bits follows down_q() in training mode")
            gscale = ((1.0 if d_obj is None else float(d_obj)) / B) if free_bits else 0.0
            _capi.check(_capi.lib().iaf_up_iaf2_backward_pre(
                _ptr(z), _ptr(st["pz_mean"]), _ptr(st["pz_logsd"]), _ptr(d_h), _ptr(d_up_c), _ptr(st["gate"]) if free_bits else None,
                gscale, None if free_bits else _ptr(dko), _ptr(dz_tot), _ptr(G), _ptr(d_dc1), B, n_h, n_z, H * W, _stream()))
            dz0, dctx, grads = self.stack.iaf_step_backward(st["z0"], st["context"], z, st["logdet"], dz_tot, G, self._rel)
            d_uc1 = torch.empty(B, 2 * n_h + 2 * n_z, H, W, dtype=torch.float32, device=z.device)
            _capi.check(_capi.lib().iaf_up_iaf2_backward_post(
                _ptr(dz0), _ptr(st["z0"]), _ptr(st["qz_mean"]), _ptr(G), _ptr(dctx), _ptr(d_up_c), _ptr(d_uc1), B, n_h, n_z, H * W,
                _stream()))
        return dict(d_up_conv1=d_uc1, d_down_conv1=d_dc1, grads={pre + k: v for k, v in grads.items()})


class CVAELayer(object):
    """models.cvae_layer(name, prior, posterior, n_h1 = n_h2 = n_h, n_z, depth_ar, downsample=False, nl='elu', ..., w) (models.py:14-345)
    on the device: the four plain Theano convs (graphy/nodes/conv.py:122-260; layers.WNConv2d(theano=True)) around a CVAELayerIAF,
    which stays what it is.  Conv widths (models.py:25-29, 59-108):

        <name>_up_conv1_1    n_h -> 2 n_h + 2 n_z
        <name>_up_conv2      n_h -> n_h                      ('up_iaf2_nl': n_h + n_z -> n_h)
        <name>_down_conv1    n_h -> 2 n_h + 4 n_z            ('up_iaf2_nl': n_h + 2 n_z;  prior 'made': 3 n_h + 2 n_z)
        <name>_down_conv2_1  n_h + n_z -> n_h

    The elu in front of every conv and the `input + 0.1 *` behind up_conv2 / down_conv2_1 are fused into the conv launches.  Launches
    of up() + down_q(): four convs + the IAF part's own (see CVAELayerIAF) + ONE copy: the IAF part hands h_det to up_conv2 as a
    contiguous copy of the first n_h channels of up_conv1's output ('down_*' posteriors; 'up_iaf2_nl': torch.cat([h_det, z])), a conv
    input being a whole tensor.  Nothing synchronises with the host, so after a warm-up up() + down_q() capture into one graph.
    Channel counts must be multiples of 16 (n_h at most 240 so that n_h + n_z <= 256)."""
    CONVS = ("_up_conv1_1", "_up_conv2", "_down_conv1", "_down_conv2_1")

    def __init__(self, name, n_h, n_z, depth_ar, posterior="down_iaf2_nl", prior="diag", flipmask=False, kl_min=0.0, downsample=False):
        if downsample:
            raise _capi.UnsupportedError("downsample=True is not built: the two strided convs (up_conv1_2 / up_conv3 with downsample 2, "
                                         "down_conv2_2 / down_conv3 with upsample 2 through depool2d_split) and the 'nn' resampling of "
                                         "the residual are missing for the Theano statement")
        self.iaf = CVAELayerIAF(name, n_h, n_z, depth_ar, posterior=posterior, flipmask=flipmask, kl_min=kl_min, prior=prior)
        self.name, self.n_h, self.n_z, self.posterior, self.prior = name, int(n_h), int(n_z), posterior, prior
        n_h, n_z = self.n_h, self.n_z
        if prior == "made":
            n_down1 = 3 * n_h + 2 * n_z                                               # models.py:38
        else:
            n_down1 = n_h + 2 * n_z if posterior == "up_iaf2_nl" else 2 * n_h + 4 * n_z
        self.widths = {"_up_conv1_1": (n_h, 2 * n_h + 2 * n_z), "_up_conv2": (n_h + n_z if posterior == "up_iaf2_nl" else n_h, n_h),
                       "_down_conv1": (n_h, n_down1), "_down_conv2_1": (n_h + n_z, n_h)}
        self.convs = {nm: WNConv2d(a, b, theano=True) for nm, (a, b) in self.widths.items()}
        self._prep = ConvPrepBatch([self.convs[nm] for nm in self.CONVS])
        self._w, self._st, self._grads, self.training = None, {}, {}, False

    def set_training(self, on=True):
        """keep what the backward needs (call load() again afterwards: the data-gradient packs are written by the next prepare)"""
        self.iaf.set_training(on)
        for c in self.convs.values():
            c.set_training(on)
        self.training = bool(on)

    def load(self, w):
        """w: the reference's parameter dict.  Reads <name>_up_conv1_1_*, <name>_up_conv2_*, <name>_down_conv1_*, <name>_down_conv2_1_*
        (w OIHW [n_out, n_in + 1, 3, 3], s, b; the four convs prepare in ONE launch) and hands the rest to the IAF part."""
        self._w = {nm: (w[self.name + nm + "_w"], w[self.name + nm + "_s"], w[self.name + nm + "_b"]) for nm in self.CONVS}
        self._prep.run([self._w[nm] for nm in self.CONVS])
        self.iaf.load(w)

    def up(self, input, eps=None):
        """models.py:138-194: input [B, n_h, H, W] -> output [B, n_h, H, W] (eps [B, n_z, H, W]: 'up_iaf2_nl' only)"""
        _check_act(input, "input")
        h = self.convs["_up_conv1_1"](input, elu_input=True)[0]
        hu = self.iaf.up(h, eps=eps)
        out = self.convs["_up_conv2"](hu, elu_input=True, residual=input)[0]
        self._st.update(up_input=input, up_conv2_in=hu)
        return out

    def down_q(self, input, eps=None):
        """models.py:201-328: input [B, n_h, H, W], eps [B, n_z, H, W] -> dict(output [B, n_h, H, W], kl, kl_sum, obj_kl, z) (kl is None
        on the training path of 'down_iaf2_nl', as in CVAELayerIAF.down_q)"""
        _check_act(input, "input")
        h = self.convs["_down_conv1"](input, elu_input=True)[0]
        d = self.iaf.down_q(h, eps=eps)
        out = self.convs["_down_conv2_1"](d["h"], elu_input=True, residual=input)[0]
        self._st.update(down_input=input, down_conv2_in=d["h"])
        return dict(output=out, kl=d["kl"], kl_sum=d["kl_sum"], obj_kl=d["obj_kl"], z=d["z"])

    def down_p(self, input, eps, **inverse_options):
        """models.py:330-359: a sample of the prior pushed down.  inverse_options: CVAELayerIAF.down_p's (exact, max_sweeps, ...)"""
        _check_act(input, "input")
        h = self.convs["_down_conv1"](input, elu_input=True)[0]
        hp = self.iaf.down_p(h, eps, **inverse_options)
        return self.convs["_down_conv2_1"](hp, elu_input=True, residual=input)[0]

    def _conv_backward(self, nm, x, dy, dy_scale, dx_residual):
        V, s, _ = self._w[nm]
        dxs, dV, ds, db = self.convs[nm].backward(x, [dy], V, s, elu_input=True, dy_scale=dy_scale, dx_residual=dx_residual)
        self._grads.update({self.name + nm + "_w": dV, self.name + nm + "_s": ds, self.name + nm + "_b": db})
        return dxs[0]

    def backward_down(self, d_down_out, d_obj=None):
        """First phase of T.grad of  <d_up_out, up()> + <d_down_out, down_q()['output']> + <d_obj, obj_kl>: everything that does not
        need d_up_out -- down_conv2_1, the IAF part, down_conv1.  Returns d_down_input.  (The cotangent of up()'s output exists only
        once the layers above have run THEIR backward: backward_up comes second.)  d_obj as CVAELayerIAF.backward: a number with free
        bits, [B] without, None = ones."""
        if self.posterior == "up_iaf2_nl":
            raise _capi.UnsupportedError("the whole-layer backward of 'up_iaf2_nl' is not built: its IAF step sits in the up pass, so the "
                                         "step's gradient needs d_up_out (use CVAELayerIAF.backward between the convs)")
        if not self.training or "down_conv2_in" not in self._st:
            raise RuntimeError("backward_down() follows up() and down_q() in training mode")
        _check_act(d_down_out, "d_down_out", tuple(self._st["down_input"].shape))
        d_h = self._conv_backward("_down_conv2_1", self._st["down_conv2_in"], d_down_out, 0.1, None)
        bw = self.iaf.backward(d_h, d_obj=d_obj, d_up=None)
        self._grads.update(bw["grads"])
        self._st["d_up_conv1"] = bw["d_up_conv1"]           # its h_det channels (zero so far) are filled by backward_up
        return self._conv_backward("_down_conv1", self._st["down_input"], bw["d_down_conv1"], 1.0, d_down_out)

    def backward_up(self, d_up_out):
        """Second phase: up_conv2, then up_conv1 on [d h_det | what backward_down left for qz_mean, qz_logsd, context].  Returns
        d_up_input.  One strided torch copy puts d h_det into the first n_h channels of d_up_conv1."""
        if "d_up_conv1" not in self._st:
            raise RuntimeError("backward_up() follows backward_down()")
        _check_act(d_up_out, "d_up_out", tuple(self._st["up_input"].shape))
        d_hu = self._conv_backward("_up_conv2", self._st["up_conv2_in"], d_up_out, 0.1, None)
        d_uc1 = self._st.pop("d_up_conv1")
        d_uc1.narrow(1, 0, self.n_h).copy_(d_hu)
        return self._conv_backward("_up_conv1_1", self._st["up_input"], d_uc1, 1.0, d_up_out)

    def grads(self):
        """every gradient of the last backward_down + backward_up, keyed like the reference's w (the IAF part's included)"""
        return dict(self._grads)
