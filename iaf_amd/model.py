"""CVAE1 -- the caller of the hot path: the reference's whole model forward, CVAE1._forward (tf_train.py:150-218), for one tower:
image scaling, conv2d("x_enc", 5x5, stride 2), the bottom-up pass through depth x num_blocks IAFLayers, the tiled h_top, the
top-down pass accumulating kl_obj / kl_cost, deconv2d("x_dec", 5x5) + clip, discretized_logistic, obj and the (k-sample) loss.
Every number is computed by HIP launches behind the C ABI (include/iaf_hip.h); torch tensors are storage.  The two edge convs
have 3 channels on one side and run as direct convolutions (csrc/iaf_kernels_edge.hpp); the layers are iaf_amd.IAFLayer.
forward() for every mode; forward_backward() = one tower's training objective and its gradient w.r.t. every variable (mode "train",
k = 1): the layers' backward (IAFLayer.down_backward / .up_backward) chained through the model + the backward of the two ends."""
import math

import torch

from . import _capi
from .distributions import StreamingLowerBound, compute_lowerbound, discretized_logistic
from .iaf_layer import IAFLayer
from .layers import (check_groups, ConvPrepBatch, PrepBatch, VariableStore, WnBwdBatch, ar_multiconv2d, resample2, variable_scope, _check_act, _ptr,
                     _stream)


def lerp_latents(za, zb, alpha, out=None):
    """(1 - alpha) za + alpha zb, layer by layer: interpolation between two sets of codes (CVAE1.encode()'s z lists; the result goes to
    CVAE1.decode).  One iaf_axpby launch per layer, no torch op; alpha 0 / 1 return the endpoints' values exactly.  out: a list from an
    earlier call -- its tensors are refilled (a captured graph's static buffers)."""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha):
        raise ValueError("alpha must be a finite number, got %r" % (alpha,))
    if not isinstance(za, (list, tuple)) or not isinstance(zb, (list, tuple)) or len(za) != len(zb) or len(za) < 1:
        raise ValueError("za, zb: two lists of latents of the same length")
    if out is not None and (not isinstance(out, (list, tuple)) or len(out) != len(za)):
        raise ValueError("out: a list of %d tensors" % len(za))
    for li, (a, b) in enumerate(zip(za, zb)):
        _check_act(a, "za[%d]" % li)
        _check_act(b, "zb[%d]" % li, tuple(a.shape))
        if out is not None:
            _check_act(out[li], "out[%d]" % li, tuple(a.shape))
    res = [torch.empty_like(a) for a in za] if out is None else list(out)
    for a, b, o in zip(za, zb, res):
        _capi.check(_capi.lib().iaf_axpby(_ptr(a), 1.0 - float(alpha), _ptr(b), float(alpha), _ptr(o), a.numel(), _stream()))
    return res


class CVAE1(object):
    """Same hyper-parameters as the reference's HParams (tf_train.py:98-112) that _forward reads: z_size, h_size, kl_min, depth
    (number of resolution levels), num_blocks (layers per level), k (importance samples), image_size.  `mode` as in the
    reference: "train" (posterior samples), "init" (prior samples through the posterior block), "sample".

    towers=N (1 .. 64, attribute model.towers): the N towers of the reference's training step (tf_train.py:124-147, num_gpus) in ONE batch.
    Rows t B/N .. (t+1) B/N of x and of every noise tensor are tower t (tf.split(0, num_gpus, x), :126); every layer takes its free-bits
    mean per tower (:79-82, the only place where rows of a batch meet), so obj and loss are the sums over the towers of what the
    reference's _forward returns for each, and the gradients the sums over the towers (average_grads' sum; TrainStep divides by
    world * towers).  forward, forward_backward, fb_begin / fb_segment and TrainStep need nothing else; B must be a multiple of N.
    generate, sample, iw_eval (it reads kl_cost only; its B too is a multiple of N) and init_pass (the reference initialises on one
    tower's batch: any B) are unaffected.
    1 (the default): one free-bits mean over the whole batch, as before."""

    def __init__(self, z_size=32, h_size=160, kl_min=0.25, depth=2, num_blocks=2, k=1, image_size=32, depth_ar=2, mode="train", towers=1):
        self.towers = check_groups(towers, "towers")
        self.z_size, self.h_size, self.kl_min = int(z_size), int(h_size), float(kl_min)
        self.depth, self.num_blocks, self.k, self.image_size, self.mode = int(depth), int(num_blocks), int(k), int(image_size), mode
        self.depth_ar = int(depth_ar)
        if self.image_size % (2 ** self.depth):
            raise ValueError("image_size must be divisible by 2**depth (tf_train.py:183,192)")
        # tf_train.py:176-181: the first layer of every level but the first downsamples
        self.layers = [[IAFLayer(z_size, h_size, depth_ar=depth_ar, kl_min=kl_min, downsample=(i > 0 and j == 0), mode=mode)
                        for j in range(self.num_blocks)] for i in range(self.depth)]
        if self.towers != 1:
            for level in self.layers:
                for layer in level:
                    layer.set_towers(self.towers)
        self._w_enc = self._w_dec = None
        self.params = None

    def load(self, params):
        """params: device fp32 tensors under the reference's variable names (tf_train.py:175-215): x_enc/{V [5,5,3,h],g,b},
        IAF_<i>_<j>/<IAFLayer names>, h_top [h], x_dec/{V [5,5,3,h],g,b}, dec_log_stdv []."""
        lib, hs = _capi.lib(), self.h_size
        for nm, shape in (("x_enc/V", (5, 5, 3, hs)), ("x_enc/g", (hs,)), ("x_enc/b", (hs,)), ("x_dec/V", (5, 5, 3, hs)),
                          ("x_dec/g", (3,)), ("x_dec/b", (3,)), ("h_top", (hs,))):
            _check_act(params[nm], nm, shape)
        self._w_enc = torch.empty_like(params["x_enc/V"])
        self._w_dec = torch.empty_like(params["x_dec/V"])
        _capi.check(lib.iaf_convk_weightnorm(_ptr(params["x_enc/V"]), _ptr(params["x_enc/g"]), _ptr(self._w_enc), 5, 5, 3, hs, 0,
                                             _stream()))                                                    # layers.py:56-60
        _capi.check(lib.iaf_convk_weightnorm(_ptr(params["x_dec/V"]), _ptr(params["x_dec/g"]), _ptr(self._w_dec), 5, 5, hs, 3, 1,
                                             _stream()))                                                    # layers.py:104-106
        self._lparams = {}
        for i, level in enumerate(self.layers):
            for j, layer in enumerate(level):
                pre = "IAF_%d_%d/" % (i, j)
                self._lparams[(i, j)] = {k[len(pre):]: v for k, v in params.items() if k.startswith(pre)}
                layer.load(self._lparams[(i, j)])
        self.params = params

    def trim_packs(self, B):
        """inference with batch B: every plain conv of every layer keeps only the weight pack its launch reads (IAFLayer.trim_packs); the
        prep launches of prepare_weights() then write 4-6 instead of 14 bytes per weight.  After load(); not for training."""
        kept = {}
        for i, level in enumerate(self.layers):
            for j, layer in enumerate(level):
                # input resolution of layer (i, j): level i runs at image_size / 2^(i+1); its first layer (downsample) is fed the finer level
                H = self.image_size // (2 ** (i + 1))
                Hin = 2 * H if layer.downsample else H
                kept[(i, j)] = layer.trim_packs(B, Hin, Hin)
        self.prepare_weights()
        return kept

    def prepare_weights(self):
        """Re-derive every weight norm from the loaded variables (what the reference's graph does inside every step, layers.py:56-60) in
        batched launches: all masked stacks in one, all plain convs in one, a downsampling layer's deconv and the two ends on their own.
        For a training loop that updates the variables in place (parallel.FlatParams): load(params) once, then prepare_weights() per step."""
        if self.params is None:
            raise RuntimeError("CVAE1.load(params) first")
        lib, p, hs = _capi.lib(), self.params, self.h_size
        if getattr(self, "_prep", None) is None:
            order = [(i, j) for i in range(self.depth) for j in range(self.num_blocks)]
            convs = [(ij, nm) for ij in order
                     for nm in ("up_conv1", "up_conv3", "down_conv1") + (() if self.layers[ij[0]][ij[1]].downsample else ("down_conv2",))]
            try:
                self._prep = dict(order=order, convs=convs, s=PrepBatch([self.layers[i][j].posterior.stack for i, j in order]),
                                  c=ConvPrepBatch([getattr(self.layers[ij[0]][ij[1]], nm) for ij, nm in convs]))
            except _capi.UnsupportedError:
                # channel counts the batched prep launches do not cover (the generic stacks): every object's own prep launch, as load()
                # runs them -- each re-derives its weights when a variable's (pointer, version) has changed since its last prep
                self._prep = dict(order=order, per_object=True)
        P = self._prep
        if P.get("per_object"):
            for i, j in P["order"]:
                self.layers[i][j].load(self._lparams[(i, j)])
        else:
            P["s"].run([IAFLayer.stack_params(self._lparams[ij]) for ij in P["order"]])
            P["c"].run([(self._lparams[ij][nm + "/V"], self._lparams[ij][nm + "/g"], self._lparams[ij][nm + "/b"]) for ij, nm in P["convs"]])
            for i, j in P["order"]:
                layer = self.layers[i][j]
                if layer.downsample:
                    lp = self._lparams[(i, j)]
                    layer.down_conv2.prepare_deconv(lp["down_deconv2/V"], lp["down_deconv2/g"], lp["down_deconv2/b"], force=True)
        _capi.check(lib.iaf_convk_weightnorm(_ptr(p["x_enc/V"]), _ptr(p["x_enc/g"]), _ptr(self._w_enc), 5, 5, 3, hs, 0, _stream()))
        _capi.check(lib.iaf_convk_weightnorm(_ptr(p["x_dec/V"]), _ptr(p["x_dec/g"]), _ptr(self._w_dec), 5, 5, hs, 3, 1, _stream()))

    def init_pass(self, x, params, noise):
        """The data-dependent initialisation pass: the reference builds CVAE1(hps, "init") first, i.e. _forward under
        arg_scope([conv2d, deconv2d], init=True) (tf_train.py:175) with every IAFLayer in mode "init" (z from the prior, :60-61).  Every conv
        -- x_enc, the plain and strided convs, the masked convs of ar_multiconv2d (conv2d is in the scope), the deconvs, x_dec -- takes its g
        and b from the moments of its own un-gained output on this batch (layers.py:38-51, 87-100) and hands the NORMALISED output on.
        params: the V of every conv (g / b entries are ignored), h_top, dec_log_stdv; noise as in forward() (the priors' draws are used).
        Returns (x_out, params_out) with params_out = params + every g and b; the model is left loaded with params_out."""
        lib, hs, zs = _capi.lib(), self.h_size, self.z_size
        B, S, n = self._check_inputs(x, noise, None)
        dev, st = x.device, _stream
        f32 = dict(dtype=torch.float32, device=dev)
        out = {k: v for k, v in params.items() if not (k.endswith("/g") or k.endswith("/b"))}

        def norm(raw, init_scale):                        # layers.py:46-51: moments over (N,H,W), g = log(scale)/3, b = -mean scale
            B_, C_, H_, W_ = (int(v) for v in raw.shape)
            y, g, b = torch.empty_like(raw), torch.empty(C_, **f32), torch.empty(C_, **f32)
            _capi.check(lib.iaf_datainit_normalize(_ptr(raw), None, _ptr(y), _ptr(g), _ptr(b), B_, C_, H_ * W_, float(init_scale), st()))
            return y, g, b

        def axpby(a, sa, b, sb):
            o = torch.empty_like(a)
            _capi.check(lib.iaf_axpby(_ptr(a), float(sa), _ptr(b), float(sb), _ptr(o), a.numel(), st()))
            return o

        def conv_init(conv, name, inp, kind="plain", x2=None):
            V = params[name + "/V"]
            z0, z1 = torch.zeros(conv.n_out, **f32), torch.zeros(conv.n_out, **f32)
            if kind == "deconv":
                conv.prepare_deconv(V, z0, z1, force=True)
                raw = conv.deconv(inp, x2=x2, elu_input=True)
            elif kind == "stride2":
                conv.prepare(V, z0, z1, force=True)
                raw = conv.stride2(inp, elu_input=True)[0]
            else:
                conv.prepare(V, z0, z1, force=True)
                raw = conv(inp, x2=x2, elu_input=True)[0]
            y, out[name + "/g"], out[name + "/b"] = norm(raw, 0.1)
            return y

        def pieces(t, sizes):
            r, off = [], 0
            for c in sizes:
                r.append(t.narrow(1, off, c).contiguous())
                off += c
            return r

        xf = torch.empty((n, 3, S, S), **f32)
        _capi.check(lib.iaf_image_to_float(x.data_ptr(), _ptr(xf), B, 3 * S * S, self.k, st()))
        w = torch.empty_like(params["x_enc/V"])
        zg, zb = torch.zeros(hs, **f32), torch.zeros(hs, **f32)
        _capi.check(lib.iaf_convk_weightnorm(_ptr(params["x_enc/V"]), _ptr(zg), _ptr(w), 5, 5, 3, hs, 0, st()))
        raw = torch.empty((n, hs, S // 2, S // 2), **f32)
        _capi.check(lib.iaf_convk_forward(_ptr(xf), _ptr(w), _ptr(zb), _ptr(raw), n, 3, S, S, hs, 5, 5, 2, 0, st()))
        h, out["x_enc/g"], out["x_enc/b"] = norm(raw, 0.1)
        ups = {}
        for i in range(self.depth):                                                                        # tf_train.py:29-44
            for j in range(self.num_blocks):
                layer, pre = self.layers[i][j], "IAF_%d_%d/" % (i, j)
                y1 = conv_init(layer.up_conv1, pre + "up_conv1", h, "stride2" if layer.downsample else "plain")
                qm, ql, uc, hh = pieces(y1, [zs, zs, hs, hs])
                y3 = conv_init(layer.up_conv3, pre + "up_conv3", hh)
                h = axpby(resample2(h, "down_even") if layer.downsample else h, 1.0, y3, 0.1)
                ups[(i, j)] = (qm, ql, uc)
        St = S // 2 ** self.depth
        h = torch.empty((n, hs, St, St), **f32)
        _capi.check(lib.iaf_tile_channels(_ptr(params["h_top"]), _ptr(h), n, hs, St * St, st()))
        li = 0
        for i in reversed(range(self.depth)):                                                              # tf_train.py:46-95, mode "init"
            for j in reversed(range(self.num_blocks)):
                layer, pre = self.layers[i][j], "IAF_%d_%d/" % (i, j)
                y = conv_init(layer.down_conv1, pre + "down_conv1", h)
                pz_mean, pz_logsd, rz_mean, rz_logsd, down_context, h_det = pieces(y, [zs] * 4 + [hs] * 2)
                z = torch.empty_like(pz_mean)
                _capi.check(lib.iaf_gaussian_sample_logsd(_ptr(pz_mean), _ptr(pz_logsd), _ptr(noise[2 * li]), _ptr(z), z.numel(), st()))   # :60-61
                qm, ql, uc = ups[(i, j)]
                context = axpby(uc, 1.0, down_context, 1.0)                                                # :58
                store = VariableStore()
                ar = pre + "ar_multiconv2d/"
                for k_, v in params.items():
                    if k_.startswith(ar) and k_.endswith("/V"):
                        store.set(k_, v)
                with variable_scope("IAF_%d_%d" % (i, j), store):
                    m_raw, s_raw = ar_multiconv2d("ar_multiconv2d", z, context, [hs] * self.depth_ar, [zs, zs], store=store, init=True)   # :69
                for k_, v in store.vars.items():
                    if k_.endswith("/g") or k_.endswith("/b"):
                        out[k_] = v
                z2 = torch.empty_like(z)
                _capi.check(lib.iaf_affine_transform(_ptr(z), _ptr(m_raw), _ptr(s_raw), 0.1, _ptr(z2), z.numel(), st()))                # :70-71
                if layer.downsample:
                    y = conv_init(layer.down_conv2, pre + "down_deconv2", z2, "deconv", x2=h_det)
                    h = axpby(resample2(h, "up_nearest"), 1.0, y, 0.1)
                else:
                    y = conv_init(layer.down_conv2, pre + "down_conv2", z2, x2=h_det)
                    h = axpby(h, 1.0, y, 0.1)                                                              # :94
                li += 1
        w = torch.empty_like(params["x_dec/V"])
        zg3, zb3 = torch.zeros(3, **f32), torch.zeros(3, **f32)
        _capi.check(lib.iaf_convk_weightnorm(_ptr(params["x_dec/V"]), _ptr(zg3), _ptr(w), 5, 5, hs, 3, 1, st()))
        raw = torch.empty((n, 3, S, S), **f32)
        _capi.check(lib.iaf_deconvk_forward(_ptr(h), _ptr(w), _ptr(zb3), _ptr(raw), n, hs, S // 2, S // 2, 3, 5, 5, 2, 1, 0.0, 0.0, st()))
        y, out["x_dec/g"], out["x_dec/b"] = norm(raw, 0.1)
        x_out = torch.empty_like(y)
        _capi.check(lib.iaf_clip(_ptr(y), -0.5 + 1 / 512., 0.5 - 1 / 512., _ptr(x_out), y.numel(), st()))                               # :208
        self.load(out)
        return x_out, out

    # -- noise from the engine's own generator (iaf_amd.NoiseSource) instead of the caller ---------------------------------------------
    def noise_shapes(self, B):
        """Host bookkeeping: the shapes of forward()'s noise list for a batch of B images -- per layer in top-down order (eps_prior,
        eps_post), B * k rows each."""
        if not _capi.int_in(B, 1):
            raise ValueError("B must be a positive int, got %r" % (B,))
        return self._noise_shapes(B * self.k)

    @staticmethod
    def noise_shapes_for(rows, z_size, depth, num_blocks, image_size):
        """Pure bookkeeping (no device, no instance): the shapes of the noise list of a depth x num_blocks model, `rows` rows each"""
        out = []
        for i in reversed(range(depth)):
            Sl = image_size // 2 ** (i + 1)
            out += [(rows, z_size, Sl, Sl)] * (2 * num_blocks)
        return out

    def _noise_shapes(self, rows):
        return CVAE1.noise_shapes_for(rows, self.z_size, self.depth, self.num_blocks, self.image_size)

    def draw_noise(self, B, source, which="both", out=None, temperature=1.0, advance=True, _rows=None):
        """forward()'s noise list drawn by `source` (a NoiseSource) in ONE launch at its current step: which = "both", "posterior" (the
        eps_post slots; what modes "train" and iw_eval read) or "prior" (the eps_prior slots; modes "init" / "sample", generate()) --
        the slots not drawn are None.  A tensor's substream is source.substream_base + its index in the FULL list, so the posterior
        noise does not depend on whether the prior noise is drawn with it.  temperature scales the prior entries (z = mean +
        temperature * sd * eps).  out: a list from an earlier call with the same B and `which` -- its tensors are refilled.  No host
        synchronisation: capturable."""
        if which not in ("both", "posterior", "prior"):
            raise ValueError("which must be 'both', 'posterior' or 'prior', got %r" % (which,))
        if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature):
            raise ValueError("temperature must be a finite number, got %r" % (temperature,))
        shapes = self.noise_shapes(B) if _rows is None else self._noise_shapes(_rows)      # (_rows: generate() does not apply k)
        take = [i for i in range(len(shapes)) if which == "both" or (i % 2 == 1) == (which == "posterior")]
        if out is None:
            out = [None] * len(shapes)
            for i in take:
                out[i] = torch.empty(shapes[i], dtype=torch.float32, device=source.device)
        elif (not isinstance(out, list) or len(out) != len(shapes)
              or any((out[i] is None) != (i not in take) or (out[i] is not None and tuple(out[i].shape) != shapes[i]) for i in range(len(shapes)))):
            raise ValueError("out: the list an earlier draw_noise(B=%d, which=%r) returned" % (B, which))
        source.fill([out[i] for i in take], substreams=[source.substream_base + i for i in take],
                    scales=[float(temperature) if i % 2 == 0 else 1.0 for i in take], advance=advance)
        return out

    def sample(self, B, source, temperature=1.0):
        """B images from the prior with noise from `source` (one step of it): draw_noise(which="prior") + generate().  No host
        synchronisation: capturable, and a replay draws fresh noise."""
        if not _capi.int_in(B, 1):
            raise ValueError("B must be a positive int, got %r" % (B,))
        return self.generate(self.draw_noise(B, source, which="prior", temperature=temperature, _rows=B)[0::2])

    def iw_eval(self, x, noise_passes=None, k=None, noise_source=None):
        """With noise_source (a NoiseSource) and k: the k noise lists are drawn by the source, one step per pass, into ONE set of
        buffers that every pass refills (memory does not grow with k) -- equal to passing the k lists draw_noise(which="posterior")
        returns at those steps.  Otherwise noise_passes as below.
        The k-sample importance-weighted bound of the whole model without materialising k samples at once (tf_train.py:168-170,218 with
        hps.k = len(noise_passes); BASELINE config 5 evaluates k = 10^4): one top-down pass with k = 1 per sample, the per-image terms
        log_pxz and sum-of-KL streamed into the running log-sum-exp (StreamingLowerBound).  The bottom-up pass -- image scaling, x_enc,
        every layer's up_conv1 / up_conv3 (tf_train.py:183-187) -- depends on x only: it runs ONCE and its products (qz_mean, qz_logsd,
        up_context of every layer, tf_train.py:38) are kept across the k passes.  noise_passes: one noise list (as for forward) per sample.
        Returns the loss [1] = sum over images of -log (1/k) sum_s exp(log_pxz_s - kl_s); bits_per_dim(loss, B) as usual."""
        if self.k != 1:
            raise ValueError("iw_eval streams the samples: build the model with k = 1")
        if (noise_passes is None) == (noise_source is None):
            raise ValueError("iw_eval: either noise_passes or noise_source (with k)")
        if noise_source is None:
            if k is not None:
                raise ValueError("iw_eval: k goes with noise_source (noise_passes carries its own length)")
        elif not _capi.int_in(k, 1):
            raise ValueError("iw_eval: k must be a positive int with noise_source, got %r" % (k,))
        if not torch.is_tensor(x) or x.dim() != 4:
            raise ValueError("x must be a contiguous uint8 [B,3,S,S] device tensor")
        B = int(x.shape[0])
        if noise_source is not None:
            def drawn():                  # one buffer set, refilled (one step of the source) per pass
                buf = None
                for _ in range(k):
                    buf = self.draw_noise(B, noise_source, which="posterior", out=buf)
                    yield buf
            noise_passes = drawn()
        acc = StreamingLowerBound(B, x.device)
        xf = None
        for noise in noise_passes:
            self._check_inputs(x, noise, self.k)      # every pass's noise list (host-only checks: the kernels take raw pointers)
            if xf is None:
                xf = self._bottom_up(x, noise)
            log_pxz, kl_cost = self._top_down(xf, B, noise, terms=True)
            acc.update(log_pxz.reshape(B, 1), kl_cost.reshape(B, 1))
        lb = acc.result()
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        _capi.check(_capi.lib().iaf_sum_axpy(_ptr(lb), None, 0.0, _ptr(loss), B, _stream()))
        return loss

    def _check_inputs(self, x, noise, k):
        """what forward(), forward_backward() and init_pass() require of (x, noise): the kernels behind them take raw pointers"""
        if self.params is None and k is not None:
            raise RuntimeError("CVAE1.load(params) first")
        if not torch.is_tensor(x) or x.dtype != torch.uint8 or not x.is_cuda or not x.is_contiguous() or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("x must be a contiguous uint8 [B,3,S,S] device tensor")
        B, _, S, S2 = (int(v) for v in x.shape)
        if S != self.image_size or S2 != S:
            raise ValueError("image size %r, model built for %d" % (tuple(x.shape), self.image_size))
        if k is not None and B % self.towers:            # (init_pass, k None: one tower's batch, no free bits)
            raise ValueError("batch of %d rows, model built for %d towers: B must be a multiple of towers" % (B, self.towers))
        if len(noise) != 2 * self.depth * self.num_blocks:
            raise ValueError("noise: %d tensors expected (prior, posterior per layer, top-down)" % (2 * self.depth * self.num_blocks))
        n = B * (self.k if k is None else k)
        li = 0
        for i in reversed(range(self.depth)):
            for _ in range(self.num_blocks):
                Sl = S // 2 ** (i + 1)
                for e in noise[2 * li:2 * li + 2]:
                    if e is None:
                        continue
                    if (not torch.is_tensor(e) or e.dtype != torch.float32 or not e.is_cuda or not e.is_contiguous()
                            or tuple(e.shape) != (n, self.z_size, Sl, Sl)):
                        raise ValueError("noise[%d..%d]: contiguous fp32 device tensors [%d,%d,%d,%d] (batch x k rows)"
                                         % (2 * li, 2 * li + 1, n, self.z_size, Sl, Sl))
                li += 1
        return B, S, n

    def forward(self, x, noise, _terms=False):
        """x: uint8 [B,3,S,S] on the device.  noise: per layer in top-down order the pair (eps_prior, eps_post) the reference's two
        DiagonalGaussians draw (distributions.py:15-24), flattened into one list -- eps_post is used in mode "train", eps_prior in
        "init" / "sample".  Returns (x_out [B k,3,S,S], obj [1], loss [1]) as tf_train.py:218."""
        xf = self._bottom_up(x, noise)
        return self._top_down(xf, int(x.shape[0]), noise, terms=_terms)

    def generate(self, eps_prior):
        """Images from the prior: the reference's m_trunc[0] of CVAE1(hps, "sample") with no image fed (tf_train.py:300, 358-362) -- TF runs
        only the top-down pass: the tiled h_top (:189-192), every layer's down() in mode "sample" (IAFLayer.generate_down: down_conv1 in
        prior form, no IAF step, no KL), x_dec + clip (:206-208).  eps_prior: per layer in top-down order the prior noise, i.e. the
        eps_prior half of forward()'s noise list, fp32 device tensors [B,z_size,S_l,S_l]; B comes from them (k is not applied).
        Returns x_out [B,3,S,S].  Works whatever `mode` the model was built with (the variables are the same); after load(params).
        No host synchronisation: capturable with torch.cuda.graph."""
        B = self._check_prior_noise(eps_prior)
        lib, p, hs, S = _capi.lib(), self.params, self.h_size, self.image_size
        dev = eps_prior[0].device
        St = S // 2 ** self.depth
        h = torch.empty((B, hs, St, St), dtype=torch.float32, device=dev)
        _capi.check(lib.iaf_tile_channels(_ptr(p["h_top"]), _ptr(h), B, hs, St * St, _stream()))          # :189-192
        li = 0
        for level in reversed(self.layers):                                                                # :195-200
            for layer in reversed(level):
                h = layer.generate_down(h, eps_prior[li])
                li += 1
        x_out = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
        _capi.check(lib.iaf_deconvk_forward(_ptr(h), _ptr(self._w_dec), _ptr(p["x_dec/b"]), _ptr(x_out), B, hs, S // 2, S // 2, 3, 5, 5,
                                            2, 1, -0.5 + 1 / 512., 0.5 - 1 / 512., _stream()))             # :206-208
        return x_out

    def _check_prior_noise(self, eps_prior):
        """what generate() requires of its noise list (host-only checks, before any launch); returns B"""
        if self.params is None:
            raise RuntimeError("CVAE1.load(params) first")
        nl = self.depth * self.num_blocks
        if not isinstance(eps_prior, (list, tuple)) or len(eps_prior) != nl:
            raise ValueError("eps_prior: %d tensors expected (the prior noise of every layer, top-down)" % nl)
        e0 = eps_prior[0]
        if not torch.is_tensor(e0) or e0.dim() != 4 or int(e0.shape[0]) < 1:
            raise ValueError("eps_prior[0]: a [B,%d,S_l,S_l] tensor" % self.z_size)
        B, li = int(e0.shape[0]), 0
        for i in reversed(range(self.depth)):
            Sl = self.image_size // 2 ** (i + 1)
            for _ in range(self.num_blocks):
                e = eps_prior[li]
                if (not torch.is_tensor(e) or e.dtype != torch.float32 or not e.is_cuda or not e.is_contiguous() or e.device != e0.device
                        or tuple(e.shape) != (B, self.z_size, Sl, Sl)):
                    raise ValueError("eps_prior[%d]: a contiguous fp32 device tensor [%d,%d,%d,%d]" % (li, B, self.z_size, Sl, Sl))
                li += 1
        return B

    # -- the latents: one top-down pass in which every layer takes its z from the posterior, from the prior, or from the caller ------------
    def _layers_top_down(self):
        """[(layer, resolution of its latent)] in the order the down pass runs (tf_train.py:195-200)"""
        return [(layer, self.image_size // 2 ** (i + 1)) for i in reversed(range(self.depth)) for layer in reversed(self.layers[i])]

    def _check_latent_call(self, what):
        if self.params is None:
            raise RuntimeError("CVAE1.load(params) first")
        if self.k != 1:
            raise ValueError("%s works on one sample per image: build the model with k = 1" % what)

    def _check_sources(self, sources, noise):
        """what _top_down_mixed requires (host-only checks, before any launch); returns (B, device)"""
        nl = self.depth * self.num_blocks
        if not isinstance(sources, (list, tuple)) or len(sources) != nl:
            raise ValueError("sources: %d entries expected ('posterior', 'prior' or a latent per layer, top-down)" % nl)
        if not isinstance(noise, (list, tuple)) or len(noise) != 2 * nl:
            raise ValueError("noise: %d entries expected (prior, posterior per layer, top-down; None where not read)" % (2 * nl))
        read = [s if torch.is_tensor(s) else noise[2 * li + (1 if s == "posterior" else 0)] if isinstance(s, str) and s in ("posterior", "prior")
                else None for li, s in enumerate(sources)]
        t0 = read[0]
        if not torch.is_tensor(t0) or t0.dim() != 4 or int(t0.shape[0]) < 1:
            raise ValueError("layer 0: 'posterior' / 'prior' with its noise tensor, or a latent [B,%d,S_l,S_l]" % self.z_size)
        B, dev = int(t0.shape[0]), t0.device
        for li, ((layer, Sl), s, t) in enumerate(zip(self._layers_top_down(), sources, read)):
            if (not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.device != dev
                    or tuple(t.shape) != (B, self.z_size, Sl, Sl)):
                raise ValueError("layer %d (%s): a contiguous fp32 device tensor [%d,%d,%d,%d]"
                                 % (li, s if isinstance(s, str) else "latent", B, self.z_size, Sl, Sl))
            if isinstance(s, str) and s == "posterior":
                q = layer.posterior.qz_mean
                if q is None or int(q.shape[0]) != B:
                    raise RuntimeError("layer %d: 'posterior' reads what the bottom-up pass of these %d images leaves in the layer" % (li, B))
        return B, dev

    def _top_down_mixed(self, sources, noise, out=None, cost_rows=None):
        """tf_train.py:189-208 with the latent of every layer taken from sources[l] (top-down): "posterior" (IAFLayer.down in mode "train" on
        the state _bottom_up left, noise[2l+1]), "prior" (generate_down, noise[2l]) or the latent itself (IAFLayer.down_from).  noise:
        forward()'s list; slots not read may be None.  out: a contiguous [B,3,S,S] tensor (or slice) x_out is written into.  cost_rows: a
        [nl, B] matrix whose row l a "posterior" layer writes its kl_cost into.  Returns (x_out, [z of every layer]).  No host
        synchronisation: capturable with torch.cuda.graph."""
        B, dev = self._check_sources(sources, noise)
        lib, p, hs, S = _capi.lib(), self.params, self.h_size, self.image_size
        if out is None:
            out = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
        else:
            _check_act(out, "out", (B, 3, S, S))
        St = S // 2 ** self.depth
        h = torch.empty((B, hs, St, St), dtype=torch.float32, device=dev)
        _capi.check(lib.iaf_tile_channels(_ptr(p["h_top"]), _ptr(h), B, hs, St * St, _stream()))          # :189-192
        zs = []
        for li, ((layer, _), s) in enumerate(zip(self._layers_top_down(), sources)):                       # :195-200
            eps = None if torch.is_tensor(s) else noise[2 * li + (1 if s == "posterior" else 0)]
            h, z, _ = layer.down_from(h, s, eps, kl_cost_out=None if cost_rows is None or torch.is_tensor(s) or s != "posterior" else cost_rows[li])
            zs.append(z)
        _capi.check(lib.iaf_deconvk_forward(_ptr(h), _ptr(self._w_dec), _ptr(p["x_dec/b"]), _ptr(out), B, hs, S // 2, S // 2, 3, 5, 5,
                                            2, 1, -0.5 + 1 / 512., 0.5 - 1 / 512., _stream()))             # :206-208
        return out, zs

    def _check_read_slots(self, noise, posterior_layers):
        """reconstruct's noise: the posterior slots of the first posterior_layers layers and the prior slots of the rest must be there"""
        nl = self.depth * self.num_blocks
        for li in range(nl):
            slot = 2 * li + (1 if li < posterior_layers else 0)
            if noise[slot] is None:
                raise ValueError("noise[%d] is None: layer %d reads its %s noise" % (slot, li, "posterior" if li < posterior_layers else "prior"))

    def encode(self, x, noise):
        """The codes of a batch of images: the bottom-up pass, then the top-down pass with every latent drawn from the posterior (what
        forward() computes in mode "train", whatever mode the model was built with).  x uint8 [B,3,S,S]; noise: forward()'s list (the
        posterior slots are read, the prior ones may be None).  Returns dict(z = [the post-flow latent of every layer (tf_train.py:71),
        top-down, B x z_size x S_l x S_l], x_out [B,3,S,S], kl_cost [nl, B] (:85, row l = layer l))."""
        self._check_latent_call("encode")
        B, _, _ = self._check_inputs(x, noise, 1)
        nl = self.depth * self.num_blocks
        self._check_read_slots(noise, nl)
        self._bottom_up(x, noise)
        cost_rows = torch.empty((nl, B), dtype=torch.float32, device=x.device)
        x_out, zs = self._top_down_mixed(["posterior"] * nl, noise, cost_rows=cost_rows)
        return dict(z=zs, x_out=x_out, kl_cost=cost_rows)

    def decode(self, z, eps_prior=None):
        """Images from codes: the top-down pass alone (no image, no bottom-up pass).  z: per layer in top-down order the latent
        [B,z_size,S_l,S_l] (encode()'s, edited or interpolated: iaf_amd.lerp_latents), or None = sample that layer from the prior with
        eps_prior[l] (generate()'s list; entries of given layers may be None).  All None is generate(eps_prior).  Returns x_out [B,3,S,S]."""
        self._check_latent_call("decode")
        nl = self.depth * self.num_blocks
        if not isinstance(z, (list, tuple)) or len(z) != nl:
            raise ValueError("z: %d entries expected (a latent or None per layer, top-down)" % nl)
        if eps_prior is None:
            eps_prior = [None] * nl
        if not isinstance(eps_prior, (list, tuple)) or len(eps_prior) != nl:
            raise ValueError("eps_prior: %d entries expected (the prior noise of every layer not given, top-down)" % nl)
        noise = []
        for li in range(nl):
            if z[li] is None and eps_prior[li] is None:
                raise ValueError("layer %d: neither a latent nor prior noise" % li)
            noise += [eps_prior[li], None]
        return self._top_down_mixed(["prior" if t is None else t for t in z], noise)[0]

    def reconstruct(self, x, noise, posterior_layers):
        """x_out with the first `posterior_layers` layers of the top-down pass drawn from the posterior of x and the rest from the prior:
        what the top levels of the hierarchy carry.  nl (= depth * num_blocks) is forward()'s x_out in mode "train", 0 is
        generate(noise[0::2]).  noise: forward()'s list (posterior slots of the first layers, prior slots of the rest)."""
        return self.reconstruct_ladder(x, noise, [posterior_layers])

    def reconstruct_ladder(self, x, noise, steps):
        """reconstruct() for every entry of `steps` in one contiguous [len(steps) B,3,S,S] tensor, step s in rows s B .. (s+1) B (what
        image_grid takes): the bottom-up pass runs once for all steps."""
        self._check_latent_call("reconstruct")
        B, S, _ = self._check_inputs(x, noise, 1)
        nl = self.depth * self.num_blocks
        if not isinstance(steps, (list, tuple)) or len(steps) < 1 or not all(_capi.int_in(n, 0, nl + 1) for n in steps):
            raise ValueError("posterior_layers: ints in 0 .. %d, got %r" % (nl, steps))
        for n in steps:
            self._check_read_slots(noise, n)
        if max(steps) > 0:
            self._bottom_up(x, noise)
        out = torch.empty((len(steps) * B, 3, S, S), dtype=torch.float32, device=x.device)
        for s, n in enumerate(steps):
            self._top_down_mixed(["posterior"] * n + ["prior"] * (nl - n), noise, out=out[s * B:(s + 1) * B])
        return out

    def _bottom_up(self, x, noise):
        """tf_train.py:153-187: image scaling (+ repeat k), x_enc, the up pass of every layer (which leaves qz_mean, qz_logsd, up_context in
        the layers, :38).  Returns the scaled image the likelihood compares with."""
        B, S, n = self._check_inputs(x, noise, self.k)
        lib, p, hs, k = _capi.lib(), self.params, self.h_size, self.k
        dev = x.device
        xf = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
        _capi.check(lib.iaf_image_to_float(x.data_ptr(), _ptr(xf), B, 3 * S * S, k, _stream()))           # tf_train.py:153-159
        h = torch.empty((n, hs, S // 2, S // 2), dtype=torch.float32, device=dev)
        _capi.check(lib.iaf_convk_forward(_ptr(xf), _ptr(self._w_enc), _ptr(p["x_enc/b"]), _ptr(h), n, 3, S, S, hs, 5, 5, 2, 0,
                                          _stream()))                                                       # :183
        for level in self.layers:                                                                          # :184-187
            for layer in level:
                h = layer.up(h)
        return xf

    def _top_down(self, xf, B, noise, terms=False):
        """tf_train.py:189-218 on the state _bottom_up left: h_top, the down pass, x_dec, the likelihood, obj and loss.
        terms=True: (log_pxz [n], kl_cost [n]) instead.  terms="raw": the pass stops behind x_dec and returns what the likelihood and the
        bound are made of -- (x_out, xf, layer_cost [nl, n]: every layer's kl_cost, top-down, written by the layers into the rows of one
        matrix) -- with no discretized_logistic, iaf_colsum or lower-bound launch and no gathering copy (EvalPass: iaf_eval_tail)."""
        lib, p, hs, k = _capi.lib(), self.params, self.h_size, self.k
        n, S, dev = int(xf.shape[0]), int(xf.shape[2]), xf.device
        St = S // 2 ** self.depth
        h = torch.empty((n, hs, St, St), dtype=torch.float32, device=dev)
        _capi.check(lib.iaf_tile_channels(_ptr(p["h_top"]), _ptr(h), n, hs, St * St, _stream()))           # :189-192
        nl = self.depth * self.num_blocks
        objs, costs = [], []
        raw = isinstance(terms, str) and terms == "raw"
        cost_rows = torch.empty((nl, n), dtype=torch.float32, device=dev) if raw else None
        li = 0
        for level in reversed(self.layers):                                                                # :195-200
            for layer in reversed(level):
                eps_prior, eps_post = noise[2 * li], noise[2 * li + 1]
                if raw:
                    h, cur_obj, cur_cost = layer.down(h, eps_post, eps_prior=eps_prior, kl_cost_out=cost_rows[li])
                    if cur_cost.data_ptr() != cost_rows[li].data_ptr():       # (a mode whose down() has no posterior block to write it)
                        cost_rows[li].copy_(cur_cost)
                else:
                    h, cur_obj, cur_cost = layer.down(h, eps_post, eps_prior=eps_prior)
                objs.append(cur_obj)
                costs.append(cur_cost)
                li += 1
        if raw:
            x_out = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
            _capi.check(lib.iaf_deconvk_forward(_ptr(h), _ptr(self._w_dec), _ptr(p["x_dec/b"]), _ptr(x_out), n, hs, S // 2, S // 2, 3, 5, 5,
                                                2, 1, -0.5 + 1 / 512., 0.5 - 1 / 512., _stream()))         # :206-208
            return x_out, xf, cost_rows
        objs, costs = torch.stack(objs), torch.stack(costs)          # [nl, n] (one gathering copy each; the sums are iaf_colsum's)
        kl_obj = torch.empty(n, dtype=torch.float32, device=dev)
        kl_cost = torch.empty(n, dtype=torch.float32, device=dev)
        _capi.check(lib.iaf_colsum(_ptr(objs), _ptr(kl_obj), nl, n, _stream()))
        _capi.check(lib.iaf_colsum(_ptr(costs), _ptr(kl_cost), nl, n, _stream()))
        x_out = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
        _capi.check(lib.iaf_deconvk_forward(_ptr(h), _ptr(self._w_dec), _ptr(p["x_dec/b"]), _ptr(x_out), n, hs, S // 2, S // 2, 3, 5, 5,
                                            2, 1, -0.5 + 1 / 512., 0.5 - 1 / 512., _stream()))             # :206-208
        log_pxz = discretized_logistic(x_out, p["dec_log_stdv"], sample=xf)                                # :210
        if terms:
            return log_pxz, kl_cost
        obj = torch.empty(1, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        _capi.check(lib.iaf_sum_axpy(_ptr(kl_obj), _ptr(log_pxz), -1.0, _ptr(obj), n, _stream()))          # :211
        lb = compute_lowerbound(log_pxz, kl_cost, k)                                                       # :218
        _capi.check(lib.iaf_sum_axpy(_ptr(lb), None, 0.0, _ptr(loss), B, _stream()))
        return x_out, obj, loss

    # -- training: d obj / d every variable, what opt.compute_gradients(obj) hands the optimizer (tf_train.py:128, 211) -----------------
    def set_training(self, on=True):
        """allocate what the backward needs in every layer (transposed packs); call load(params) afterwards"""
        for level in self.layers:
            for layer in level:
                layer.set_training(on)
        for sg in (getattr(self, "_segs", None) or []):              # back to per-op weight-norm backward for anyone using the layers directly
            lib = _capi.lib()
            for st in sg["wn"].stacks:
                _capi.check(lib.iaf_stack_set_defer_weightnorm(st._h, 0))
            for cv in sg["wn"].convs:
                _capi.check(lib.iaf_conv3x3_set_defer_weightnorm(cv._h, 0))
        self._training = bool(on)
        self.params = None
        self._prep = None
        # mask + weight-norm backward of the stacks and plain convs of a gradient bucket in ONE launch per kind at the end of the bucket's
        # backward segment (a conv's own pass is 10-28 workgroups on a 256-CU chip; set_grad_buckets, default: one bucket = the whole model);
        # a downsampling layer's deconv differentiates its own norm inside its backward
        self._segs = None

    # The gradient exchange of data-parallel training (tf_train.py:124-147, tf_utils/common.py:83-86) overlaps the backward when the
    # flat gradient buffer is laid out in the order the backward COMPLETES the gradients and cut into contiguous buckets
    # (parallel.OverlappedGradReduce).  That order, for this model: the top end (dec_log_stdv, x_dec), then the top-down pass backwards
    # = layer by layer in up-pass order (each layer's last conv, its ar_multiconv2d stack, down_conv1), h_top, then the bottom-up pass
    # backwards (up_conv3, up_conv1 of every layer in reverse), x_enc.
    _DOWN_KEYS = ("down_conv2/", "down_deconv2/", "ar_multiconv2d/", "down_conv1/")

    @staticmethod
    def _names_of_layer(all_names, ij, down):
        pre = "IAF_%d_%d/" % ij
        return [k for k in all_names if k.startswith(pre) and (k[len(pre):].startswith(CVAE1._DOWN_KEYS) == down)]

    def _layer_names(self, ij, down):
        return CVAE1._names_of_layer(self.params if self.params is not None else {}, ij, down)

    @staticmethod
    def grad_bucket_names(all_names, depth, num_blocks, n_buckets=1):
        """Pure bookkeeping (no device): the variable names of a depth x num_blocks model, bucket by bucket, in the order forward_backward
        completes their gradients -- ceil(n/2) groups of layers for the top-down pass's backward (bucket 0 also holds the top end), floor(n/2)
        for the bottom-up pass's (the first with h_top, the last with x_enc).  Concatenated = completion_order()."""
        order = [(i, j) for i in range(depth) for j in range(num_blocks)]
        nb = max(1, min(int(n_buckets), 2 * len(order)))
        chunks = lambda lst, n: [lst[q * len(lst) // n:(q + 1) * len(lst) // n] for q in range(n)]
        top, bottom = ["dec_log_stdv", "x_dec/V", "x_dec/g", "x_dec/b"], ["x_enc/V", "x_enc/g", "x_enc/b"]
        names_of = lambda g, down: [k for ij in g for k in CVAE1._names_of_layer(all_names, ij, down)]
        if nb < 2:
            out = [top + names_of(order, True) + ["h_top"] + names_of(list(reversed(order)), False) + bottom]
        else:
            dgroups, ugroups = chunks(order, (nb + 1) // 2), chunks(list(reversed(order)), nb // 2)
            out = [(top if gi == 0 else []) + names_of(g, True) for gi, g in enumerate(dgroups)]
            out += [(["h_top"] if gi == 0 else []) + names_of(g, False) + (bottom if gi == len(ugroups) - 1 else []) for gi, g in enumerate(ugroups)]
        flat = [k for b in out for k in b]
        if sorted(flat) != sorted(all_names):
            raise ValueError("not the variables of a %d x %d CVAE1: %s" % (depth, num_blocks, sorted(set(flat) ^ set(all_names))[:6]))
        return out

    def completion_order(self):
        """every variable name in the order forward_backward completes its gradient (lay parallel.FlatParams out in this order)"""
        if self.params is None:
            raise RuntimeError("CVAE1.load(params) first")
        return [k for b in CVAE1.grad_bucket_names(list(self.params), self.depth, self.num_blocks, 1) for k in b]

    def set_grad_buckets(self, n_buckets=1):
        """Cut the backward into `n_buckets` segments, each completing one contiguous run of completion_order(): ceil(n/2) groups of layers
        for the top-down pass's backward, floor(n/2) for the bottom-up pass's; every segment ends with the deferred mask + weight-norm
        backward of exactly its own convs (one launch per kind).  Returns the variable names per bucket (for
        OverlappedGradReduce.bounds_from_groups).  forward_backward(on_bucket=) then reports each bucket the moment it is complete."""
        if not getattr(self, "_training", False) or self.params is None:
            raise RuntimeError("CVAE1.set_training(True), then load(params), before set_grad_buckets")
        order = [(i, j) for i in range(self.depth) for j in range(self.num_blocks)]
        nb = max(1, min(int(n_buckets), 2 * len(order)))
        chunks = lambda lst, n: [lst[q * len(lst) // n:(q + 1) * len(lst) // n] for q in range(n)]
        dgroups = chunks(order, (nb + 1) // 2) if nb >= 2 else [order]
        ugroups = chunks(list(reversed(order)), nb // 2) if nb >= 2 else []
        L = lambda ij: self.layers[ij[0]][ij[1]]
        dconvs = lambda ij: [(ij, "down_conv1")] + ([] if L(ij).downsample else [(ij, "down_conv2")])
        uconvs = lambda ij: [(ij, "up_conv3"), (ij, "up_conv1")]
        segs = []
        for gi, g in enumerate(dgroups):
            convs = [c for ij in g for c in dconvs(ij)]
            up_too = nb < 2                                          # a single bucket: everything completes at the very end
            if up_too:
                convs += [c for ij in reversed(order) for c in uconvs(ij)]
            names = (["dec_log_stdv", "x_dec/V", "x_dec/g", "x_dec/b"] if gi == 0 else []) + [k for ij in g for k in self._layer_names(ij, True)]
            if up_too:
                names += ["h_top"] + [k for ij in reversed(order) for k in self._layer_names(ij, False)] + ["x_enc/V", "x_enc/g", "x_enc/b"]
            segs.append(dict(down=g, up=list(reversed(order)) if up_too else [], h_top=up_too, x_enc=up_too, names=names, conv_ids=convs,
                             stack_ids=list(g),
                             wn=WnBwdBatch(stacks=[L(ij).posterior.stack for ij in g], convs=[getattr(L(ij), nm) for ij, nm in convs])))
        for gi, g in enumerate(ugroups):
            convs = [c for ij in g for c in uconvs(ij)]
            last = gi == len(ugroups) - 1
            names = (["h_top"] if gi == 0 else []) + [k for ij in g for k in self._layer_names(ij, False)] + \
                    (["x_enc/V", "x_enc/g", "x_enc/b"] if last else [])
            segs.append(dict(down=[], up=g, h_top=(gi == 0), x_enc=last, names=names, conv_ids=convs, stack_ids=[],
                             wn=WnBwdBatch(stacks=[], convs=[getattr(L(ij), nm) for ij, nm in convs])))
        names = CVAE1.grad_bucket_names(list(self.params), self.depth, self.num_blocks, nb)
        assert len(names) == len(segs) and all(sorted(sg["names"]) == sorted(nm) for sg, nm in zip(segs, names))
        for sg, nm in zip(segs, names):
            sg["names"] = nm
        self._segs = segs
        return names

    def fb_begin(self, x, noise, grads=None, autotune=False, terms=False):
        """forward_backward, first part: the forward pass (keeping what the backward reads) and the backward of the top end --
        obj = sum(kl_obj - log_pxz), likelihood, clip, x_dec (tf_train.py:206-211).  Then fb_segment(0 .. n_buckets-1).
        terms=True also keeps what the reference's summaries are made of (tf_train.py:203-204, 214-218), under "terms" in the returned
        dict: layer_obj / layer_cost [nl, n] (every layer's kl_obj / kl_cost, top-down as the down pass runs), layers (the (i, j) of
        each table row), log_pxz [n] and loss [1] = sum(kl_cost - log_pxz) (what compute_lowerbound sums to at k = 1; two launches more: one iaf_colsum, one iaf_sum_axpy).  terms=False: not one launch
        more."""
        if not getattr(self, "_training", False) or self.params is None:
            raise RuntimeError("CVAE1.set_training(True), then load(params), before forward_backward")
        if self.k != 1 or self.mode != "train":
            raise ValueError("forward_backward: mode 'train', k = 1 (the training objective, tf_train.py:211)")
        if getattr(self, "_segs", None) is None:
            self.set_grad_buckets(1)
        B, S, n = self._check_inputs(x, noise, 1)
        lib, p, hs = _capi.lib(), self.params, self.h_size
        dev, st = x.device, _stream
        f32 = dict(dtype=torch.float32, device=dev)
        # ---- forward, keeping what the backward reads
        xf = torch.empty((n, 3, S, S), **f32)
        _capi.check(lib.iaf_image_to_float(x.data_ptr(), _ptr(xf), B, 3 * S * S, 1, st()))
        h = torch.empty((n, hs, S // 2, S // 2), **f32)
        _capi.check(lib.iaf_convk_forward(_ptr(xf), _ptr(self._w_enc), _ptr(p["x_enc/b"]), _ptr(h), n, 3, S, S, hs, 5, 5, 2, 0, st()))
        for level in self.layers:
            for layer in level:
                h = layer.up_train(h, autotune=autotune)
        St = S // 2 ** self.depth
        h = torch.empty((n, hs, St, St), **f32)
        _capi.check(lib.iaf_tile_channels(_ptr(p["h_top"]), _ptr(h), n, hs, St * St, st()))
        objs, costs, li = [], [], 0
        for level in reversed(self.layers):
            for layer in reversed(level):
                h, cur_obj, cur_cost = layer.down_train(h, noise[2 * li + 1], autotune=autotune)
                objs.append(cur_obj)
                costs.append(cur_cost)
                li += 1
        h_last = h
        objs = torch.stack(objs)
        kl_obj = torch.empty(n, **f32)
        _capi.check(lib.iaf_colsum(_ptr(objs), _ptr(kl_obj), li, n, st()))
        lo, hi = -0.5 + 1 / 512., 0.5 - 1 / 512.
        x_out = torch.empty((n, 3, S, S), **f32)
        _capi.check(lib.iaf_deconvk_forward(_ptr(h_last), _ptr(self._w_dec), _ptr(p["x_dec/b"]), _ptr(x_out), n, hs, S // 2, S // 2, 3, 5, 5,
                                            2, 1, lo, hi, st()))
        log_pxz = discretized_logistic(x_out, p["dec_log_stdv"], sample=xf)
        obj = torch.empty(1, **f32)
        _capi.check(lib.iaf_sum_axpy(_ptr(kl_obj), _ptr(log_pxz), -1.0, _ptr(obj), n, st()))
        kept = None
        if terms:                                                    # loss = sum(kl_cost - log_pxz), as obj above (tf_train.py:218, k = 1)
            costs = torch.stack(costs)
            kl_cost = torch.empty(n, **f32)
            _capi.check(lib.iaf_colsum(_ptr(costs), _ptr(kl_cost), li, n, st()))
            loss = torch.empty(1, **f32)
            _capi.check(lib.iaf_sum_axpy(_ptr(kl_cost), _ptr(log_pxz), -1.0, _ptr(loss), n, st()))
            kept = dict(layer_obj=objs, layer_cost=costs, log_pxz=log_pxz, loss=loss, kl_cost=kl_cost,
                        layers=[(i, j) for i in reversed(range(self.depth)) for j in reversed(range(self.num_blocks))])
        # ---- backward of the top end: obj = sum(kl_obj - log_pxz)  (tf_train.py:206-211)
        grads = {} if grads is None else grads
        gs = lambda nm: grads.setdefault(nm, torch.empty_like(p[nm]))
        d_xout = torch.empty_like(x_out)
        dls_rows = torch.empty(n, **f32)
        logscale = p["dec_log_stdv"].reshape(1).contiguous()
        _capi.check(lib.iaf_discretized_logistic_backward(_ptr(x_out), _ptr(logscale), _ptr(xf), -1.0, lo, hi, _ptr(d_xout), _ptr(dls_rows), n,
                                                          3 * S * S, 1 / 256.0, st()))
        _capi.check(lib.iaf_sum_axpy(_ptr(dls_rows), None, 0.0, _ptr(gs("dec_log_stdv")), n, st()))
        dW = torch.empty_like(p["x_dec/V"])
        _capi.check(lib.iaf_convk_wgrad(_ptr(d_xout), _ptr(h_last), _ptr(dW), n, 3, S, S, hs, 5, 5, 2, 0, 1, st()))
        gs("x_dec/V"), gs("x_dec/g"), gs("x_dec/b")
        scratch = torch.empty(hs * 3, **f32)
        _capi.check(lib.iaf_convk_weightnorm_backward(_ptr(p["x_dec/V"]), _ptr(p["x_dec/g"]), _ptr(dW), _ptr(grads["x_dec/V"]),
                                                      _ptr(grads["x_dec/g"]), _ptr(scratch), 5, 5, hs, 3, 1, st()))
        _capi.check(lib.iaf_channel_sum(_ptr(d_xout), _ptr(grads["x_dec/b"]), n, 3, S * S, st()))
        # d h_last = elu'(h_last) * (the strided conv of d x_out with x_dec's filter: the adjoint of the transposed conv)
        zero_b = torch.zeros(hs, **f32)
        t = torch.empty_like(h_last)
        _capi.check(lib.iaf_convk_forward(_ptr(d_xout), _ptr(self._w_dec), _ptr(zero_b), _ptr(t), n, 3, S, S, hs, 5, 5, 2, 0, st()))
        d = torch.empty_like(h_last)
        _capi.check(lib.iaf_mul_elu_grad(_ptr(t), _ptr(h_last), _ptr(d), t.numel(), st()))
        lgrads = {}
        for i, level in enumerate(self.layers):
            for j, layer in enumerate(level):
                pre = "IAF_%d_%d/" % (i, j)
                lgrads[(i, j)] = {k[len(pre):]: v for k, v in grads.items() if k.startswith(pre)}
        self._fb = dict(x_out=x_out, obj=obj, grads=grads, lgrads=lgrads, d=d, xf=xf, n=n, S=S, St=St, autotune=autotune,
                        dko=torch.ones(n, **f32), keep=(dW, scratch, zero_b, t, d_xout, dls_rows, logscale, log_pxz, kl_obj, objs))
        if kept is not None:
            self._fb["terms"] = kept
        return self._fb

    def fb_segment(self, si):
        """forward_backward, segment si (in order, after fb_begin): the backward of its layers and the deferred mask + weight-norm backward
        of its convs -- on return every gradient of bucket si is complete (enqueued on the current stream)."""
        lib, p, hs, F, sg = _capi.lib(), self.params, self.h_size, self._fb, self._segs[si]
        grads, lgrads, n, S, St, autotune, st = F["grads"], F["lgrads"], F["n"], F["S"], F["St"], F["autotune"], _stream
        gs = lambda nm: grads.setdefault(nm, torch.empty_like(p[nm]))
        # ---- the layer stack: the top-down pass backwards (= in up-pass order), then the bottom-up pass backwards
        for (i, j) in sg["down"]:
            F["d"] = self.layers[i][j].down_backward(F["d"], F["dko"], self._lparams[(i, j)], lgrads[(i, j)], autotune=autotune)
        if sg["h_top"]:
            _capi.check(lib.iaf_channel_sum(_ptr(F["d"]), _ptr(gs("h_top")), n, hs, St * St, st()))        # adjoint of the tile (:190-192)
            F["d"] = torch.zeros((n, hs, St, St), dtype=torch.float32, device=F["d"].device)   # the up pass's last output is not used (h_top replaces it)
        for (i, j) in sg["up"]:
            F["d"] = self.layers[i][j].up_backward(F["d"], self._lparams[(i, j)], lgrads[(i, j)], autotune=autotune)
        tup = lambda dct, nm: (dct[nm + "/V"], dct[nm + "/g"], dct[nm + "/b"])
        sg["wn"].run(stack_params=[IAFLayer.stack_params(self._lparams[ij]) for ij in sg["stack_ids"]],
                     stack_grads=[IAFLayer.stack_params(lgrads[ij]) for ij in sg["stack_ids"]],
                     conv_params=[tup(self._lparams[ij], nm) for ij, nm in sg["conv_ids"]],
                     conv_grads=[tup(lgrads[ij], nm) for ij, nm in sg["conv_ids"]])
        for (i, j) in set(sg["down"]) | set(sg["up"]):
            for k, v in lgrads[(i, j)].items():
                grads["IAF_%d_%d/%s" % (i, j, k)] = v
        if sg["x_enc"]:                                                                                    # :183
            d = F["d"]
            dW = torch.empty_like(p["x_enc/V"])
            _capi.check(lib.iaf_convk_wgrad(_ptr(F["xf"]), _ptr(d), _ptr(dW), n, 3, S, S, hs, 5, 5, 2, 0, 0, st()))
            gs("x_enc/V"), gs("x_enc/g"), gs("x_enc/b")
            _capi.check(lib.iaf_convk_weightnorm_backward(_ptr(p["x_enc/V"]), _ptr(p["x_enc/g"]), _ptr(dW), _ptr(grads["x_enc/V"]),
                                                          _ptr(grads["x_enc/g"]), None, 5, 5, 3, hs, 0, st()))
            _capi.check(lib.iaf_channel_sum(_ptr(d), _ptr(grads["x_enc/b"]), n, hs, (S // 2) ** 2, st()))
            F["keep"] = F["keep"] + (dW,)

    def forward_backward(self, x, noise, grads=None, autotune=False, on_bucket=None):
        """One tower's forward and backward in mode "train", k = 1: returns (x_out, obj [1], grads) with grads[name] = d obj / d params[name]
        for every variable (written into the tensors of `grads` where it has them -- e.g. the views of parallel.FlatParams.g).
        autotune=True: the first call at a new batch size searches the launch shapes of the plain convs and their data gradients (what
        cuDNN's algorithm search does for the reference).  The layer stack's backward is IAFLayer.down_backward / .up_backward chained through the model (the down pass
        in up-pass order, then the up pass in reverse); the two ends -- likelihood, clip, x_dec, h_top, x_enc -- are the launches of
        csrc/iaf_model_ops.hip.  noise as in forward().  on_bucket(i): called as soon as the gradients of bucket i (set_grad_buckets) are
        complete on the current stream -- where a data-parallel step issues that bucket's all-reduce (OverlappedGradReduce.reduce)."""
        F = self.fb_begin(x, noise, grads, autotune)
        for si in range(len(self._segs)):
            self.fb_segment(si)
            if on_bucket is not None:
                on_bucket(si)
        return F["x_out"], F["obj"], F["grads"]

    def exchange_errors(self):
        """bounded waits of the hand-overs inside the one-launch IAF steps that gave up, over all layers (0 = never; it synchronises the
        device).  A NaN loss with a non-zero count means the exchange, not the numerics: re-arm with ARStack.set_halo_exchange(True) and,
        if the step is replayed from a hipGraph, capture it again (include/iaf_hip.h)."""
        return sum(layer.posterior.stack.exchange_errors() for level in self.layers for layer in level)

    def bits_per_dim(self, loss, batch_size):
        """tf_train.py:133 for one tower: loss / (log 2 * num_pixels * batch_size)"""
        return float(loss) / (math.log(2.) * 3 * self.image_size ** 2 * batch_size)
