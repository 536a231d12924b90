// iaf_conv3x3_host.hpp -- host side + C ABI of the plain / single masked 3x3 convs (iaf_conv3x3_*): functions of an iaf_conv3x3_t or a batch of them.
// A section of iaf_engine.hip (included there last: it uses the stack's launch logic; not a standalone header).
#pragma once

// ---------------------------------------------------------------------------------------------
// plain weight-normed 3x3 convs around the IAF step: up_conv1 / up_conv3 / down_conv1 / down_conv2
// (tf_train.py:36-44, 52-54, 87-94; operator tf_utils/layers.py:31-64 with mask=None, stride 1, pad SAME).
// Same implicit-GEMM kernel as the masked stack with all 9 taps live (template NTP = 9) and the EPI_PLAIN epilogue:
// ELU / channel concat fused into the input staging, channel split / residual fused into the store.
// ---------------------------------------------------------------------------------------------
struct iaf_conv3x3 : PackState {   // precision, packs (iaf_conv3x3_set_packs), f16_off, prepared: iaf_pack_state.hpp
    int n_in, n_out;
    int mask_mode;     // 0 plain conv2d, 1 ar_conv2d(zerodiagonal=False), 2 ar_conv2d(zerodiagonal=True)
    int variant = IAF_VARIANT_TF;   // masked convs only: the Theano statements of ar.conv2d (graphy/nodes/ar.py:200-375)
    bool generic;
    GemmLayer L;
    PrepLayer* h_desc = nullptr;   // pinned staging of the prep descriptor
    PrepLayer* d_desc = nullptr;
    bool training = false;
    bool deconv = false;           // weights prepared by iaf_conv3x3_prepare_deconv (deconv2d's norm + rotated filter)
    // the plain conv of the Theano statement (iaf_conv3x3_create_theano; graphy/nodes/conv.py:122-260): weights w OIHW [n_out][n_in+1][3][3],
    // s, b; the pack is flipped at prep time (prep_tile_plain_theano), so launches keep the TF tap tables and `variant` stays
    // IAF_VARIANT_TF; L.bias is the position-class table [16][ncot*16], L.border the eight border weights [8][ncot*16]
    bool theano_plain = false;
    bool dgrad_pinned = false;     // iaf_conv3x3_set_dgrad_tuning: the data gradient runs the split products in the shape T.b_* at every size
    // forward on the bf16 matrix cores (bf16x3 split products, iaf_conv_bf3.hpp with 9 taps): plain convs with c_in % 32 == 0
    // IAF_PRECISION_F16X2 (round 6): as BF16X3, the stride-1 forward launches on TWO fp16 planes (iaf_conv_bf3.hpp F16) from the pack L.wp2;
    // an operand beyond 65504 raises rng_err (mapped host memory): the next forward returns IAF_ERR_RANGE once and the conv runs bf16x3
    // from then on (f16_off) until iaf_conv3x3_set_precision(F16X2) re-arms
    RangeWord rng;
    int bf3_choice = 1;            // 1 size rule, 2 the shape in L.b_* (pinned by iaf_conv3x3_autotune), 3 fp32 kernel (measured faster)
    GemmLayer T;                   // transposed problem dX = W^T dY (valid when training)
    // deferred weight-norm backward (iaf_conv3x3_wn_bwd_batch_run): the reduced dW / db partials live here, not in the
    // (shared) workspace
    bool defer_wn = false;
    float* own_dW = nullptr; float* own_dbp = nullptr;
    int pend_nslab = 0; bool pending = false;
};

extern "C" int iaf_conv3x3_destroy(iaf_conv3x3_t* c) {
    if (!c) return IAF_ERR_NULL;
    gemm_layer_free(c->L);
    c->rng.free();
    if (c->own_dW) (void)hipFree(c->own_dW);
    if (c->own_dbp) (void)hipFree(c->own_dbp);
    if (c->h_desc) (void)hipHostFree(c->h_desc);
    if (c->d_desc) (void)hipFree(c->d_desc);
    delete c;
    return IAF_OK;
}

static inline bool conv_split(const iaf_conv3x3* c) { return c->precision != IAF_PRECISION_F32; }
// the forward launches of this conv run the two-plane fp16 kernels now
static inline bool conv_f16_active(const iaf_conv3x3* c) {
    return pack_f16_wanted(*c) && c->L.wp2 && !c->generic && !c->mask_mode;
}
// which packs a prep launch writes for a plain conv (iaf_conv3x3_set_packs; training keeps all of them)
static inline void conv_prep_packs(const iaf_conv3x3* c, PrepLayer& P) {
    prep_layer_packs(P, c->L, pack_prep_writes(*c, PACK_CONV, conv_f16_active(c), c->L.wp3 != nullptr, c->training), c->rng.dev);
}
static int conv3x3_create(iaf_conv3x3_t** out, int n_in, int n_out, int mask_mode, bool theano_plain = false);
extern "C" int iaf_conv3x3_create(iaf_conv3x3_t** out, int n_in, int n_out) { return conv3x3_create(out, n_in, n_out, 0); }
extern "C" int iaf_conv3x3_create_masked(iaf_conv3x3_t** out, int n_in, int n_out, int zerodiagonal) {
    if (n_in > 0 && n_out > 0 && !(n_in % n_out == 0 || n_out % n_in == 0)) return IAF_ERR_NOT_MULTIPLE;   // layers.py:116
    return conv3x3_create(out, n_in, n_out, zerodiagonal ? 2 : 1);
}

// N.ar.conv2d(name, n_in, n_out, (3,3), zerodiagonal, flipmask, w=w) of the Theano path (graphy/nodes/ar.py:200-375; e.g.
// posteriors 'up_iaf1' / 'down_iaf2', models.py:53-55,73-79): weights w OIHW [n_out][n_in+1][3][3], s, b.  Forward only.
extern "C" int iaf_conv3x3_create_masked_theano(iaf_conv3x3_t** out, int n_in, int n_out, int zerodiagonal, int flipmask) {
    if (n_in > 0 && n_out > 0 && !(n_in % n_out == 0 || n_out % n_in == 0)) return IAF_ERR_NOT_MULTIPLE;   // ar.py:250,257
    int rc = conv3x3_create(out, n_in, n_out, zerodiagonal ? 2 : 1);
    if (rc) return rc;
    iaf_conv3x3* c = *out;
    if (c->generic) { iaf_conv3x3_destroy(c); *out = nullptr; return IAF_ERR_UNSUPPORTED; }
    c->variant = flipmask ? IAF_VARIANT_THEANO_FLIPMASK : IAF_VARIANT_THEANO;
    if ((rc = (int)hipMalloc(&c->L.border, (size_t)4 * c->L.ncot * 16 * sizeof(float))) != 0) { iaf_conv3x3_destroy(c); *out = nullptr; return rc; }
    return IAF_OK;
}

// N.conv.conv2d(name, n_in, n_out, (3,3), w=w) of the Theano path (graphy/nodes/conv.py:122-260; up_conv1/2, down_conv1/2 of
// models.cvae_layer, models.py:59-108): include/iaf_hip.h has the contract
extern "C" int iaf_conv3x3_create_theano(iaf_conv3x3_t** out, int n_in, int n_out) {
    if (!out) return IAF_ERR_NULL;
    *out = nullptr;
    if (n_in > 0 && n_out > 0 && (n_in % 16 != 0 || n_out % 16 != 0 || n_in > 16 * PREP_MAXI)) return IAF_ERR_UNSUPPORTED;    // (no generic form)
    return conv3x3_create(out, n_in, n_out, 0, true);
}

static int conv3x3_create(iaf_conv3x3_t** out, int n_in, int n_out, int mask_mode, bool theano_plain) {
    if (!out) return IAF_ERR_NULL;
    *out = nullptr;
    if (n_in <= 0 || n_out <= 0) return IAF_ERR_SHAPE;
    iaf_conv3x3* c = new (std::nothrow) iaf_conv3x3();
    if (!c) return (int)hipErrorOutOfMemory;
    c->n_in = n_in; c->n_out = n_out; c->prepared = false; c->mask_mode = mask_mode; c->theano_plain = theano_plain;
    c->generic = (n_in % 16 != 0 || n_out % 16 != 0 || n_in > 16 * PREP_MAXI);
    GemmLayer& L = c->L;
    L.cin = n_in; L.cout = n_out; L.npair = 1; L.zerodiag = (mask_mode == 2) ? 1 : 0; L.full3x3 = (mask_mode == 0);
    L.nchunk = (n_in + 15) / 16; L.ncot = (n_out + 15) / 16;
    default_tuning(L, false);
    L.live_macs_per_px = L.dense_macs_per_px = 9.0 * n_in * n_out;
    if (mask_mode) count_macs(L, n_in, n_out, L.zerodiag, 1);
    int rc;
    if ((rc = (int)hipMalloc(&L.wp, c->generic ? (size_t)MAXTAPS * n_in * n_out * sizeof(float) : pack_bytes_f32(L, MAXTAPS))) != 0 ||
        (rc = (int)hipMalloc(&L.bias, ((size_t)L.ncot * 16 * (theano_plain ? 16 : 1) + (size_t)n_in) * sizeof(float))) != 0 ||   // + deconv norms
        (theano_plain && (rc = (int)hipMalloc(&L.border, (size_t)(MAXTAPS - 1) * L.ncot * 16 * sizeof(float))) != 0) ||
        (rc = (int)hipHostMalloc((void**)&c->h_desc, sizeof(PrepLayer))) != 0 ||
        (rc = (int)hipMalloc((void**)&c->d_desc, sizeof(PrepLayer))) != 0) {
        iaf_conv3x3_destroy(c);
        return rc;
    }
    if (!c->generic && mask_mode == 0 && n_in % 32 == 0 && (rc = (int)hipMalloc(&L.wp3, pack_bytes_split(L, MAXTAPS, 3))) != 0) {
        iaf_conv3x3_destroy(c);
        return rc;
    }
    // default arithmetic of a plain conv with a split pack: the two-plane fp16 forward (IAF_DEFAULT_PRECISION=bf16x3: round 5's)
    if (L.wp3 && !theano_plain) {     // (the Theano plain conv has no fp16-plane form: bf16x3, the PackState default)
        static const bool f16_default = !(getenv("IAF_DEFAULT_PRECISION") && !strcmp(getenv("IAF_DEFAULT_PRECISION"), "bf16x3"));
        if (f16_default) {
            rc = iaf_conv3x3_set_precision(c, IAF_PRECISION_F16X2);
            if (rc != IAF_OK && rc != IAF_ERR_UNSUPPORTED) { iaf_conv3x3_destroy(c); return rc; }
        }
    }
    *out = c;
    return IAF_OK;
}

extern "C" int iaf_conv3x3_prepare(iaf_conv3x3_t* c, const float* V, const float* g, const float* b, void* stream) {
    if (!c || !V || !g || !b) return IAF_ERR_NULL;
    const GemmLayer& L = c->L;
    c->deconv = false;
    if (c->generic) {
        GenPrepArgs ga;
        memset(&ga, 0, sizeof(ga));
        ga.nlayers = 1;
        GenPrepLayer& P = ga.L[0];
        P.V[0] = V; P.g[0] = g; P.b[0] = b; P.w = L.wp; P.bias = L.bias;
        P.cin = L.cin; P.cout_each = L.cout; P.npair = 1; P.zerodiag = L.zerodiag; P.ch_begin = 0; P.ntaps = MAXTAPS;
        P.mask9 = c->mask_mode ? 1 : 0;
        hipLaunchKernelGGL(iaf_generic_prep_kernel, dim3(L.cout), dim3(256), 0, (hipStream_t)stream, ga);
    } else if (c->mask_mode) {    // the masked prep of the stack, one layer
        PrepArgs a;
        memset(&a, 0, sizeof(a));
        a.nlayers = 1;
        PrepLayer& P = a.L[0];
        P.V[0] = V; P.g[0] = g; P.b[0] = b; P.wp = L.wp; P.variant = c->variant;
        prep_layer_geometry(P, L, 0);
        hipLaunchKernelGGL(iaf_prep_kernel, dim3(L.ncot), dim3(256), 0, (hipStream_t)stream, a, 0u);
    } else {
        PrepLayer& P = *c->h_desc;
        memset(&P, 0, sizeof(P));
        P.V[0] = V; P.g[0] = g; P.b[0] = b; P.variant = c->theano_plain ? PREP_PLAIN9_THEANO : PREP_PLAIN9;
        conv_prep_packs(c, P);
        prep_layer_geometry(P, L, 0);
        HIP_TRY(hipMemcpyAsync(c->d_desc, c->h_desc, sizeof(PrepLayer), hipMemcpyHostToDevice, (hipStream_t)stream));
        hipLaunchKernelGGL(iaf_prep_plain_kernel, dim3(L.ncot), dim3(256), 0, (hipStream_t)stream, c->d_desc, (const int*)nullptr);
        if (c->training) {
            PackT3Batch tb((hipStream_t)stream);
            int rc = tb.add(L, MAXTAPS);
            if (!rc) rc = tb.flush();
            if (rc) return rc;
        }
    }
    HIP_TRY(hipGetLastError());
    c->prepared = true;
    return IAF_OK;
}

// deconv2d("down_deconv2") of a downsampling IAFLayer (tf_train.py:91; tf_utils/layers.py:67-112): V is [3,3,n_out,n_in].
// The object is an ordinary iaf_conv3x3 (n_in, n_out) afterwards: run it with iaf_conv3x3_forward on the zero-inserted
// input (iaf_resample2 mode IAF_RESAMPLE_UP_ZERO_ODD) at the OUTPUT resolution.  Forward only.
extern "C" int iaf_conv3x3_prepare_deconv(iaf_conv3x3_t* c, const float* V, const float* g, const float* b, void* stream) {
    if (c && c->theano_plain) return IAF_ERR_UNSUPPORTED;
    if (!c || !V || !g || !b) return IAF_ERR_NULL;
    if (c->mask_mode) return IAF_ERR_UNSUPPORTED;
    if (c->packs != IAF_PACK_ALL) return IAF_ERR_UNSUPPORTED;    // (the deconv packs derive from the fp32 one)
    GemmLayer& L = c->L;
    hipStream_t st = (hipStream_t)stream;
    float* inv_norm = L.bias + (size_t)L.ncot * 16;    // n_in floats behind the packed bias (conv3x3_create)
    hipLaunchKernelGGL(iaf_deconv_norm_kernel, dim3(L.cin), dim3(256), 0, st, V, inv_norm, L.cin, L.cout);
    const size_t total = (size_t)9 * L.cin * L.cout;
    unsigned blocks = (unsigned)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(iaf_deconv_pack_kernel, dim3(blocks), dim3(256), 0, st, V, g, b, (const float*)inv_norm, L.wp, L.bias,
                       L.cin, L.cout, L.ncot, c->generic ? 1 : 0, (c->training && !c->generic) ? L.wpt : nullptr);
    HIP_TRY(hipGetLastError());
    if (L.wp3 && !c->generic && L.nchunk % 2 == 0) {   // the same pack as three bf16 planes (iaf_conv3x3_forward_deconv): wp has the layout
        PackT3Args a;                                  // iaf_pack_t3_kernel reads ([K chunk][tap][N tile][lane][4])
        memset(&a, 0, sizeof(a));
        a.L[0].src = L.wp; a.L[0].dst = L.wp3; a.L[0].ntp = MAXTAPS; a.L[0].nct = L.ncot; a.L[0].begin = 0;
        a.n = 1; a.total = (L.nchunk / 2) * MAXTAPS * L.ncot * 64;
        hipLaunchKernelGGL(iaf_pack_t3_kernel, dim3((a.total + 255) / 256), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    if (c->training && !c->generic) {           // ... and its bf16x3 form for the data gradient
        PackT3Batch tb(st);
        int rc = tb.add(L, MAXTAPS);
        if (!rc) rc = tb.flush();
        if (rc) return rc;
    }
    c->prepared = true;
    c->deconv = true;
    return IAF_OK;
}

// weight prep of many plain convs in one launch (the four convs of every IAFLayer of a model): descriptors in device
// memory, refreshed per run like iaf_prep_batch_run
struct iaf_conv3x3_prep_batch {
    std::vector<iaf_conv3x3*> convs;
    BatchTable<PrepLayer> t;       // one descriptor per conv (BatchTable in iaf_engine.hip)
};

extern "C" int iaf_conv3x3_prep_batch_destroy(iaf_conv3x3_prep_batch_t* b) {
    if (!b) return IAF_ERR_NULL;
    b->t.destroy();
    delete b;
    return IAF_OK;
}

// the convs a batch object takes (plain, on the MFMA path) and their tiles: one per 16 output channels
static int conv_batch_tiles(iaf_conv3x3_t* const* convs, int n, std::vector<int>* tiles) {
    for (int i = 0; i < n; ++i) {
        if (!convs[i]) return IAF_ERR_NULL;
        if (convs[i]->generic || convs[i]->mask_mode) return IAF_ERR_UNSUPPORTED;
        tiles->push_back(convs[i]->L.ncot);
    }
    return IAF_OK;
}

extern "C" int iaf_conv3x3_prep_batch_create(iaf_conv3x3_prep_batch_t** out, iaf_conv3x3_t* const* convs, int n) {
    if (!out || !convs) return IAF_ERR_NULL;
    *out = nullptr;
    if (n <= 0) return IAF_ERR_SHAPE;
    std::vector<int> tiles;
    if (int rc = conv_batch_tiles(convs, n, &tiles)) return rc;
    iaf_conv3x3_prep_batch* b = new (std::nothrow) iaf_conv3x3_prep_batch();
    if (!b) return (int)hipErrorOutOfMemory;
    b->convs.assign(convs, convs + n);
    if (int rc = b->t.create(tiles, false)) { iaf_conv3x3_prep_batch_destroy(b); return rc; }
    for (int i = 0; i < n; ++i) {
        PrepLayer& P = b->t.h[i];
        P.variant = convs[i]->theano_plain ? PREP_PLAIN9_THEANO : PREP_PLAIN9;
        conv_prep_packs(convs[i], P);
        prep_layer_geometry(P, convs[i]->L, b->t.begin[i]);
    }
    *out = b;
    return IAF_OK;
}

extern "C" int iaf_conv3x3_prep_batch_run(iaf_conv3x3_prep_batch_t* b, const float* const* V, const float* const* g,
                                          const float* const* bias, void* stream) {
    if (!b || !V || !g || !bias) return IAF_ERR_NULL;
    for (int i = 0; i < b->t.n; ++i) {
        if (!V[i] || !g[i] || !bias[i]) return IAF_ERR_NULL;
        b->t.set(i, [&](PrepLayer& P) {
            P.V[0] = V[i]; P.g[0] = g[i]; P.b[0] = bias[i];
            conv_prep_packs(b->convs[i], P);     // iaf_conv3x3_set_precision / _set_packs / _set_training / a range failure since the last run
        });
    }
    hipStream_t st = (hipStream_t)stream;
    const PrepLayer* d_layers = nullptr;
    if (int rc = b->t.upload(st, &d_layers)) return rc;
    hipLaunchKernelGGL(iaf_prep_plain_kernel, dim3(b->t.ntiles), dim3(256), 0, st, d_layers, b->t.d_tile2layer);
    HIP_TRY(hipGetLastError());
    {
        PackT3Batch tb(st);
        for (const iaf_conv3x3* c : b->convs)
            if (c->training) { int rc = tb.add(c->L, MAXTAPS); if (rc) return rc; }
        int rc = tb.flush();
        if (rc) return rc;
    }
    for (iaf_conv3x3* c : b->convs) { c->prepared = true; c->deconv = false; }   // (packs of a conv2d now, as iaf_conv3x3_prepare leaves them)
    return IAF_OK;
}

// co tiles per workgroup (NT x WCO) of a 9-tap split-product launch need not divide the layer's tile count: the last workgroup's surplus
// tiles are computed on clamped fragments and dropped (iaf_conv_bf3.hpp, toff) -- accepted up to a quarter of the layer's tiles
static inline bool bf3_ragged_ok(int ncot, int per_wg) {
    if (per_wg <= 0) return false;
    const int covered = (ncot + per_wg - 1) / per_wg * per_wg;
    return (covered - ncot) * 4 <= ncot;
}
extern "C" int iaf_conv3x3_set_tuning(iaf_conv3x3_t* c, int nt, int pxt, int wco, int ks) {
    if (!c) return IAF_ERR_NULL;
    GemmLayer& L = c->L;
    if (nt == 0) { L.user_tuned = false; c->bf3_choice = 1; return IAF_OK; }     // back to the automatic choice
    if (nt < 0) {           // a bf16x3 launch shape, as iaf_conv3x3_autotune reports it: (-nt, ppw, wco, ks), pxt = 1
        if (c->generic || c->mask_mode || !L.wp3 || !bf3_ragged_ok(L.ncot, -nt * wco) ||
            !pick_bf3p(-nt, pxt, 1, ks, wco, c->theano_plain ? BF3P_PLAIN_TH : BF3P_PLAIN)) return IAF_ERR_UNSUPPORTED;
        L.b_nt = -nt; L.b_ppw = pxt; L.b_pxt = 1; L.b_ks = ks; L.b_wco = wco;
        c->bf3_choice = 2;
        return IAF_OK;
    }
    if (c->generic || !pick_kernel(nt, pxt, wco, ks, IN_NCHW, c->mask_mode ? EPI_PLAIN5 : c->theano_plain ? EPI_PLAIN_TH : EPI_PLAIN)) return IAF_ERR_UNSUPPORTED;
    if (L.ncot % (nt * wco) != 0 || L.nchunk < ks) return IAF_ERR_UNSUPPORTED;
    L.nt = nt; L.pxt = pxt; L.wco = wco; L.ks = ks; L.user_tuned = true;
    c->bf3_choice = 3;      // a pinned fp32 shape means the fp32 kernel
    return IAF_OK;
}

// launch of the conv kernel for a plain / single masked conv descriptor (forward, or its transposed problem with the
// taps mirrored for the data gradient)
// the plain conv on the bf16 matrix cores: which shape, if any, for this size (choice: see iaf_conv3x3.bf3_choice)
static bool conv3x3_bf3_shape(GemmLayer& L, int choice, long long P, int W, bool f16 = false) {
    if (!L.wp3 || choice == 3) return false;
    if (choice != 2) {
        // size rule: worth it from ~4096 pixels on (as for the masked stack); on the fp16 planes (half the MFMAs) from 2048
        if (P < (f16 ? 2048 : 4096)) return false;
        // (nt, wco) at ppw 2, ks 4 -- what iaf_conv3x3_autotune finds at the BASELINE sizes (round 6): every workgroup of a 32-pixel block
        // stages the block's tile again, so the FEWEST workgroups per block that still give the chip a workgroup per CU, at most an
        // eighth of the co tiles wasted on a ragged last group; else whatever gives the most workgroups
        static const int cand[8][2] = {{4, 3}, {5, 2}, {4, 2}, {2, 3}, {5, 1}, {4, 1}, {2, 2}, {2, 1}};
        const long long nblk = (P + 31) / 32;
        int best = -1;
        long long best_wgs = 0;
        for (int i = 0; i < 8; ++i) {
            const int nt = cand[i][0], wco = cand[i][1], per = nt * wco;
            const int covered = (L.ncot + per - 1) / per * per;
            if ((covered - L.ncot) * 8 > L.ncot || !pick_bf3p(nt, 2, 1, 4, wco, BF3P_PLAIN)) continue;
            if (bf3_plain_lds_bytes(L.cin, W, nt, 2, 1, 4, wco, f16 ? 2 : 3) > 160 * 1024) continue;
            const long long wgs = nblk * (covered / per);
            if (wgs >= 256) { best = i; break; }
            if (wgs > best_wgs) { best_wgs = wgs; best = i; }
        }
        if (best < 0) return false;
        L.b_nt = cand[best][0]; L.b_ppw = 2; L.b_pxt = 1; L.b_ks = 4; L.b_wco = cand[best][1];
    }
    if (!bf3_ragged_ok(L.ncot, L.b_nt * L.b_wco) || !pick_bf3p(L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, L.b_wco, BF3P_PLAIN)) return false;
    return bf3_plain_lds_bytes(L.cin, W, L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, L.b_wco, f16 ? 2 : 3) <= 160 * 1024;
}

// dev tool (tools/conv_stamps.py): per-workgroup cycle stamps of THIS conv's bf16x3 plain-conv launches, [grid][8] u64 in a caller
// buffer of `bytes` bytes (NULL: off).  Per object and size-checked at every launch (it was one process-global pointer
// that every conv's launches on every stream wrote through without a bound); declared here, defined behind the object's definition.

// dgrad16: the data gradient (bwd3) of a conv whose arithmetic is IAF_PRECISION_F16X2 -- two fp16 planes with a tile-local scale
static int conv3x3_launch(GemmLayer& L, ConvP& p, int epi_sel, int inmode, bool masked, bool mirror, hipStream_t st,
                          int variant = IAF_VARIANT_TF, int bf3_choice = 3, unsigned* f16_rng = nullptr, bool dgrad16 = false) {
    // the plain conv on the bf16 matrix cores: forward (NCHW input, EPI_PLAIN), or its data gradient (L = the transposed
    // problem with wp3 = the transposed bf16x3 pack: dY pixel-major, mirrored taps, EPI_DGRAD)
    const bool th = epi_sel == EPI_PLAIN_TH;        // the Theano plain conv: the same launch, the forms with the position-class bias table
    const bool fwd3 = !masked && !mirror && (epi_sel == EPI_PLAIN || th) && inmode == IN_NCHW;
    const bool bwd3 = !masked && mirror && epi_sel == EPI_DGRAD9 && inmode == IN_PIXMAJOR && variant == IAF_VARIANT_TF;
    const bool f16l = (fwd3 && f16_rng != nullptr) || (bwd3 && dgrad16 && L.wp2 != nullptr);
    if ((fwd3 || bwd3) && conv3x3_bf3_shape(L, bf3_choice, p.P, p.W, f16l) &&
        pick_bf3p(L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, L.b_wco, bwd3 ? BF3P_DGRAD : th ? BF3P_PLAIN_TH : BF3P_PLAIN)) {
        conv_fn_t fn = pick_bf3p(L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, L.b_wco, bwd3 ? BF3P_DGRAD : th ? BF3P_PLAIN_TH : BF3P_PLAIN);
        const int tm = 16 * L.b_ppw * L.b_pxt, W = p.W, sg = bwd3 ? -1 : 1;
        p.border = nullptr; p.wp = (const float*)L.wp3; p.bias = L.bias; p.lim = nullptr;
        // f16_rng (the caller's conv runs IAF_PRECISION_F16X2): the forward on two fp16 planes, the same launch shape and LDS bound
        bool npl2 = false;
        if (conv_fn_t fn16 = (fwd3 && f16_rng && L.wp2) ? pick_bf3p(L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, L.b_wco, BF3P_F16) : nullptr) {
            fn = fn16; p.wp = (const float*)L.wp2; p.rng_err = f16_rng; npl2 = true;
        } else if (conv_fn_t fd16 = (bwd3 && dgrad16 && L.wp2) ? pick_bf3p(L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, L.b_wco, BF3P_F16_DGRAD) : nullptr) {
            fn = fd16; p.wp = (const float*)L.wp2; p.rng_err = nullptr; npl2 = true;
        } else if (f16l) {
            return IAF_ERR_UNSUPPORTED;         // (the shape was sized for two planes and no two-plane kernel exists for it: not reached by the compiled shape lists)
        }
        for (int t = 0; t < MAXTAPS; ++t) { p.tap_dh[t] = sg * (t / 3 - 1); p.tap_dw[t] = sg * (t % 3 - 1); }   // cross-correlation, SAME (mirrored: dX)
        p.halo_before = W + 1;
        p.nslot = tm + 2 * (W + 1);
        p.cin = L.cin; p.cout = L.cout; p.nchunk = L.nchunk; p.ncot = L.ncot; p.cp = L.cin + 8;
        const size_t lds = bf3_plain_lds_bytes(L.cin, W, L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, L.b_wco, npl2 ? 2 : 3);
        int rc = raise_lds_cap((const void*)fn, lds);
        if (rc) return rc;
        dim3 grid((p.P + tm - 1) / tm, (L.ncot + L.b_nt * L.b_wco - 1) / (L.b_nt * L.b_wco));
        p.gx = (int)grid.x;
        p.lds_bytes = (int)lds;
        p.dbg = (L.dbg && (size_t)grid.x * grid.y * 8 * sizeof(unsigned long long) <= L.dbg_bytes) ? L.dbg : nullptr;
        hipLaunchKernelGGL(fn, grid, dim3(64 * L.b_pxt * L.b_ks * L.b_wco), lds, st, p);
        return (int)hipGetLastError();
    }
    if (!L.user_tuned) {
        GemmLayer t = L;
        t.nt = L.t_nt; t.pxt = L.t_ppw; t.wco = L.t_pxt; t.ks = L.t_ks;
        if (L.tuned_P == p.P && L.tuned_W == p.W && L.t_nt > 0 && conv_lds_bytes(t, p.W) <= 160 * 1024) {
            L.nt = t.nt; L.pxt = t.pxt; L.wco = t.wco; L.ks = t.ks;     // measured for this size (iaf_conv3x3_autotune_backward)
        } else {
            auto_shape(L, false, p.P, p.W);
        }
    }
    conv_fn_t fn = pick_kernel(L.nt, L.pxt, L.wco, L.ks, inmode, epi_sel);
    if (!fn) return IAF_ERR_UNSUPPORTED;
    // Theano's true convolution looks left/above (taps negated); flipmask turns it back (see launch_gemm)
    const int tm = 16 * L.pxt, W = p.W, sgn = ((variant == IAF_VARIANT_THEANO) != mirror) ? -1 : 1;
    p.border = (masked && !mirror) ? L.border : nullptr;
    p.wp = L.wp; p.bias = L.bias; p.lim = nullptr;
    if (masked) {     // the 5 live taps of the MADE-masked filter: look right / below only
        static const int tf_dh[NTAPS] = {0, 0, 1, 1, 1}, tf_dw[NTAPS] = {0, 1, -1, 0, 1};
        for (int t = 0; t < NTAPS; ++t) { p.tap_dh[t] = sgn * tf_dh[t]; p.tap_dw[t] = sgn * tf_dw[t]; }
        p.halo_before = (sgn < 0) ? W + 1 : 0;
        p.nslot = tm + W + 1;
    } else {
        for (int t = 0; t < MAXTAPS; ++t) { p.tap_dh[t] = sgn * (t / 3 - 1); p.tap_dw[t] = sgn * (t % 3 - 1); }   // cross-correlation, SAME
        p.halo_before = W + 1;
        p.nslot = tm + 2 * (W + 1);
    }
    p.cin = L.cin; p.cout = L.cout; p.nchunk = L.nchunk; p.ncot = L.ncot;
    p.cp = L.cin + 8;
    const size_t lds = conv_lds_bytes(L, W);
    if (lds > 160 * 1024) return IAF_ERR_UNSUPPORTED;
    int rc = raise_lds_cap((const void*)fn, lds);
    if (rc) return rc;
    dim3 grid((p.P + tm - 1) / tm, L.ncot / (L.nt * L.wco));
    p.gx = (int)grid.x;
    p.lds_bytes = (int)lds;
    hipLaunchKernelGGL(fn, grid, dim3(64 * L.pxt * L.wco * L.ks), lds, st, p);
    return (int)hipGetLastError();
}

extern "C" int iaf_conv3x3_forward(iaf_conv3x3_t* c, const float* x, const float* x2, int c_split, int elu_input,
                                   const float* residual, float* const* outs, const int* out_channels, int n_outs, int B,
                                   int H, int W, void* stream) {
    if (!c || !x || !outs || !out_channels) return IAF_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || n_outs < 1 || n_outs > MAXSPLIT) return IAF_ERR_SHAPE;
    if ((long long)B * H * W > (1LL << 30) / 64) return IAF_ERR_SHAPE;
    if (!c->prepared) return IAF_ERR_NOT_PREPARED;
    if (x2 && (c_split <= 0 || c_split >= c->n_in)) return IAF_ERR_SHAPE;
    if (residual && n_outs != 1) return IAF_ERR_SHAPE;
    int tot = 0, ends[MAXSPLIT];
    for (int k = 0; k < n_outs; ++k) {
        if (!outs[k]) return IAF_ERR_NULL;
        if (out_channels[k] <= 0) return IAF_ERR_SHAPE;
        tot += out_channels[k];
        ends[k] = tot;
    }
    if (tot != c->n_out) return IAF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    GemmLayer& L = c->L;
    if (c->generic) {
        GenPlainP p;
        memset(&p, 0, sizeof(p));
        p.x = x; p.x2 = x2; p.w = L.wp; p.bias = L.bias; p.res = residual;
        p.B = B; p.H = H; p.W = W; p.cin = L.cin; p.cout = L.cout; p.c_split = c_split; p.in_elu = elu_input ? 1 : 0;
        p.nsplit = n_outs;
        for (int k = 0; k < n_outs; ++k) { p.split_end[k] = ends[k]; p.split_ptr[k] = outs[k]; }
        hipLaunchKernelGGL(iaf_generic_conv3x3_kernel, ew_grid((size_t)B * L.cout * H * W), dim3(256), 0, st, p);
        return (int)hipGetLastError();
    }
    // MFMA path: a lane owns 4 consecutive channels, so the concat point and the split points must be multiples of 4
    if (x2 && (c_split & 3)) return IAF_ERR_UNSUPPORTED;
    for (int k = 0; k < n_outs; ++k)
        if (ends[k] & 3) return IAF_ERR_UNSUPPORTED;
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.B = B; p.H = H; p.W = W; p.HW = H * W; p.P = B * H * W;
    p.x = x; p.x2 = x2; p.c_split = c_split; p.in_elu = elu_input ? 1 : 0; p.res = residual;
    p.nsplit = n_outs;
    for (int k = 0; k < MAXSPLIT; ++k) {
        p.split_end[k] = ends[k < n_outs ? k : n_outs - 1];
        p.split_ptr[k] = outs[k < n_outs ? k : n_outs - 1];
    }
    // an F16 launch of this conv (or the prep of its pack) met an operand beyond fp16's range: said once; bf16x3 from here on
    if (pack_range_report(*c, PACK_CONV, c->rng.peek())) return IAF_ERR_RANGE;
    if (!c->mask_mode && c->packs != IAF_PACK_ALL) {
        // iaf_conv3x3_set_packs: the pack this launch reads must be one the prep launches write
        GemmLayer t = L;
        const bool split = conv_split(c) && !c->deconv && conv3x3_bf3_shape(t, c->bf3_choice, p.P, W, conv_f16_active(c));
        const bool f16 = split && conv_f16_active(c) && pick_bf3p(t.b_nt, t.b_ppw, t.b_pxt, t.b_ks, t.b_wco, BF3P_F16);
        const int need = f16 ? IAF_PACK_F16X2 : split ? IAF_PACK_BF16X3 : IAF_PACK_F32;
        if (!(c->packs & need)) return IAF_ERR_NOT_PREPARED;
    }
    return conv3x3_launch(L, p, c->mask_mode ? EPI_PLAIN5 : c->theano_plain ? EPI_PLAIN_TH : EPI_PLAIN, IN_NCHW, c->mask_mode != 0, false, st, c->variant,
                          (conv_split(c) && !c->deconv) ? c->bf3_choice : 3, conv_f16_active(c) ? c->rng.dev : nullptr);
}

// ---- down_conv1 in prior form: the sample-mode top-down pass (tf_train.py:52-54, 56, 60-61; iaf_conv_bf3.hpp EPI_PRIOR) -------------
// Only the co tiles mode "sample" reads -- pz_mean, pz_logsd, h_det: (2 n_z + n_h) / 16 of down_conv1's (4 n_z + 2 n_h) / 16 -- stream from the
// conv's own pack (launch tile -> pack tile map, prior_pack_tile), and the prior sample is drawn in the epilogue.  Launch shape: the plain
// conv's size rule (fewest workgroups per 32-pixel block that still fill the chip, at most an eighth of the tiles ragged) on the LAUNCHED
// tiles, with NT in {2, 4} (two-tile units).  Arithmetic: two fp16 planes where the forward at this size runs them
// (iaf_conv3x3_runs_f16x2, same range word and protocol), else the bf16x3 planes at any size (fp32-grade; there is no fp32-kernel form).
// ragged_den: at most 1 / ragged_den of the tiles may be ragged (8: the plain conv's bound, and the prior form's).  The h_det-only form's is
// a fifth -- 12 launched tiles for the 10 of h 160, NT 4 x WCO 3: ONE workgroup per 32-pixel block where it fills the chip (the tile is
// staged once instead of five times; measured, DESIGN.md 4.3: 20.2 against 28.4 us at 32 x 16 x 16)
#ifndef IAF_HDET_RAGGED_DEN
#define IAF_HDET_RAGGED_DEN 5
#endif
static conv_fn_t conv3x3_prior_shape(const GemmLayer& L, int nlt, long long P, int W, bool f16, int* nt_out, int* wco_out, size_t* lds_out,
                                     int ragged_den = 8, const char* env_name = nullptr) {
    static const int cand[6][2] = {{4, 3}, {4, 2}, {2, 3}, {4, 1}, {2, 2}, {2, 1}};
    const long long nblk = (P + 31) / 32;
    int best = -1;
    long long best_wgs = 0;
    // env_name (dev override, as IAF_S2_SHAPE): "nt,wco" of a compiled shape, taken if it fits the LDS
    int env[2] = {0, 0};
    const char* e = env_name ? getenv(env_name) : nullptr;
    if (e && sscanf(e, "%d,%d", &env[0], &env[1]) == 2 && env[0] > 0 && env[1] > 0 &&
        pick_bf3p(env[0], 2, 1, 4, env[1], f16 ? BF3P_PRIOR_F16 : BF3P_PRIOR) &&
        bf3_plain_lds_bytes(L.cin, W, env[0], 2, 1, 4, env[1], f16 ? 2 : 3) <= 160 * 1024) {
        *nt_out = env[0]; *wco_out = env[1];
        *lds_out = bf3_plain_lds_bytes(L.cin, W, env[0], 2, 1, 4, env[1], f16 ? 2 : 3);
        return pick_bf3p(env[0], 2, 1, 4, env[1], f16 ? BF3P_PRIOR_F16 : BF3P_PRIOR);
    }
    for (int i = 0; i < 6; ++i) {
        const int nt = cand[i][0], wco = cand[i][1], per = nt * wco;
        const int covered = (nlt + per - 1) / per * per;
        if ((covered - nlt) * ragged_den > nlt || !pick_bf3p(nt, 2, 1, 4, wco, f16 ? BF3P_PRIOR_F16 : BF3P_PRIOR)) continue;
        if (bf3_plain_lds_bytes(L.cin, W, nt, 2, 1, 4, wco, f16 ? 2 : 3) > 160 * 1024) continue;
        const long long wgs = nblk * (covered / per);
        if (wgs >= 256) { best = i; break; }
        if (wgs > best_wgs) { best_wgs = wgs; best = i; }
    }
    if (best < 0) return nullptr;
    *nt_out = cand[best][0]; *wco_out = cand[best][1];
    *lds_out = bf3_plain_lds_bytes(L.cin, W, *nt_out, 2, 1, 4, *wco_out, f16 ? 2 : 3);
    return pick_bf3p(*nt_out, 2, 1, 4, *wco_out, f16 ? BF3P_PRIOR_F16 : BF3P_PRIOR);
}

// the launch behind both entry points.  n_zu: the (pz_mean, pz_logsd) units launched -- n_z / 16 (prior form), or 0 (h_det only: eps, z NULL)
static int conv3x3_prior_launch(iaf_conv3x3_t* c, const float* x, int elu_input, int n_z, int n_h, int n_zu, const float* eps, float* z,
                                float* h_det, int B, int H, int W, void* stream) {
    GemmLayer& L = c->L;
    if (c->generic || c->mask_mode || c->deconv || !L.wp3 || !conv_split(c) || (n_z & 15) || (n_h & 15)) return IAF_ERR_UNSUPPORTED;
    if (!c->prepared) return IAF_ERR_NOT_PREPARED;
    // an F16 launch of this conv (or the prep of its pack) met an operand beyond fp16's range: said once; bf16x3 from here on
    if (pack_range_report(*c, PACK_CONV, c->rng.peek())) return IAF_ERR_RANGE;
    const bool f16 = iaf_conv3x3_runs_f16x2(c, B, H, W) != 0;
    if (!(c->packs & (f16 ? IAF_PACK_F16X2 : IAF_PACK_BF16X3))) return IAF_ERR_NOT_PREPARED;    // (iaf_conv3x3_set_packs)
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.pr_nzt = n_zu; p.pr_nht = n_h / 16; p.pr_nlt = 2 * p.pr_nzt + 2 * ((p.pr_nht + 1) / 2);
    int nt = 0, wco = 0;
    size_t lds = 0;
    conv_fn_t fn = n_zu ? conv3x3_prior_shape(L, p.pr_nlt, (long long)B * H * W, W, f16, &nt, &wco, &lds)
                        : conv3x3_prior_shape(L, p.pr_nlt, (long long)B * H * W, W, f16, &nt, &wco, &lds, IAF_HDET_RAGGED_DEN, "IAF_HDET_SHAPE");
    if (!fn) return IAF_ERR_UNSUPPORTED;
    p.B = B; p.H = H; p.W = W; p.HW = H * W; p.P = B * H * W;
    p.x = x; p.in_elu = elu_input ? 1 : 0;
    p.eps = eps; p.out0 = z; p.out1 = h_det;
    // the tiles the z units skip, when none is launched: prior_pack_tile counts pack tiles from (4 pr_nzt) on, so with pr_nzt = 0 the pack and
    // the bias are handed over from down_conv1's tile 4 n_z / 16 on (a tile = npl KiB of every step; the step stride stays the whole pack's,
    // p.ncot).  The last tile read is pr_nht + pr_nht - 1 behind that = the pack's last.
    const int skip = 4 * (n_z / 16 - n_zu);
    const char* pack = f16 ? (const char*)L.wp2 : (const char*)L.wp3;
    p.wp = (const float*)(pack + (size_t)skip * (f16 ? 2 : 3) * 1024); p.bias = L.bias + (size_t)skip * 16;
    p.rng_err = f16 ? c->rng.dev : nullptr;
    for (int t = 0; t < MAXTAPS; ++t) { p.tap_dh[t] = t / 3 - 1; p.tap_dw[t] = t % 3 - 1; }     // cross-correlation, SAME
    const int tm = 32;                                                                             // ppw 2, pxt 1
    p.halo_before = W + 1;
    p.nslot = tm + 2 * (W + 1);
    p.cin = L.cin; p.cout = L.cout; p.nchunk = L.nchunk; p.ncot = L.ncot; p.cp = L.cin + 8;
    int rc = raise_lds_cap((const void*)fn, lds);
    if (rc) return rc;
    dim3 grid((p.P + tm - 1) / tm, (p.pr_nlt + nt * wco - 1) / (nt * wco));
    p.gx = (int)grid.x;
    p.lds_bytes = (int)lds;
    hipLaunchKernelGGL(fn, grid, dim3(64 * 4 * wco), lds, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

extern "C" int iaf_conv3x3_forward_prior_sample(iaf_conv3x3_t* c, const float* x, int elu_input, int n_z, int n_h, const float* eps, float* z,
                                                float* h_det, int B, int H, int W, void* stream) {
    if (c && c->theano_plain) return IAF_ERR_UNSUPPORTED;
    if (!c || !x || !eps || !z || !h_det) return IAF_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || n_z <= 0 || n_h <= 0) return IAF_ERR_SHAPE;
    if ((long long)B * H * W > (1LL << 30) / 64) return IAF_ERR_SHAPE;
    if (c->n_out != 4 * n_z + 2 * n_h) return IAF_ERR_SHAPE;
    return conv3x3_prior_launch(c, x, elu_input, n_z, n_h, n_z / 16, eps, z, h_det, B, H, W, stream);
}

// ---- down_conv1 in h_det-only form: a layer whose z is GIVEN (CVAE1.decode; tf_train.py:52-54, 87-88) ------------------------------------
// Of down_conv1's six outputs a given z leaves only h_det to compute: n_h / 16 of the (4 n_z + 2 n_h) / 16 co tiles (10 of 28 at z 32 /
// h 160).  It is the prior form with no z unit (EPI_PRIOR, pr_nzt = 0: every launched unit is a pair of h_det tiles; eps / out0 are never
// dereferenced -- epi_load / epi_apply touch them for u < pr_nzt only), on the pack handed over from its first skipped tile (above): no
// kernel of its own.  Arithmetic, range word, fallbacks: the prior form's.
extern "C" int iaf_conv3x3_forward_hdet(iaf_conv3x3_t* c, const float* x, int elu_input, int n_z, int n_h, float* h_det, int B, int H, int W,
                                        void* stream) {
    if (c && c->theano_plain) return IAF_ERR_UNSUPPORTED;
    if (!c || !x || !h_det) return IAF_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || n_z <= 0 || n_h <= 0) return IAF_ERR_SHAPE;
    if ((long long)B * H * W > (1LL << 30) / 64) return IAF_ERR_SHAPE;
    if (c->n_out != 4 * n_z + 2 * n_h) return IAF_ERR_SHAPE;
    return conv3x3_prior_launch(c, x, elu_input, n_z, n_h, 0, nullptr, nullptr, h_det, B, H, W, stream);
}

// ---- the downsampling IAFLayer's two strided convs at their minimal work (iaf_conv_bf3.hpp, template parameter S2) ------------
// launch shape (nt, ppw, ks, wco; pxt = 1) of a strided conv: the first compiled one that divides the co tiles and fits LDS.
// IAF_S2_SHAPE / IAF_DECONV_SHAPE="nt,ppw,ks,wco": dev override.
static conv_fn_t s2_shape(const GemmLayer& L, int s2, int W, int* sh, size_t* lds_out) {
    static const int cand[2][6][4] = {
        {{4, 2, 4, 2}, {5, 2, 4, 2}, {2, 2, 4, 2}, {4, 2, 4, 1}, {5, 2, 4, 1}, {2, 2, 4, 1}},       // stride 2: 32 output pixels (4 x 32 staged)
        {{5, 4, 4, 1}, {4, 4, 4, 1}, {2, 4, 4, 1}, {5, 2, 4, 2}, {4, 2, 4, 2}, {2, 2, 4, 2}}};      // deconv: 64 input pixels
    int env[4] = {0, 0, 0, 0};
    const char* e = getenv(s2 == 1 ? "IAF_S2_SHAPE" : "IAF_DECONV_SHAPE");
    const bool has_env = e && sscanf(e, "%d,%d,%d,%d", &env[0], &env[1], &env[2], &env[3]) == 4;
    for (int i = has_env ? -1 : 0; i < 6; ++i) {
        const int* q = i < 0 ? env : cand[s2 - 1][i];
        const int nt = q[0], ppw = q[1], ks = q[2], wco = q[3];
        if (nt <= 0 || wco <= 0 || L.ncot % (nt * wco) != 0) continue;
        conv_fn_t fn = pick_bf3p(nt, ppw, 1, ks, wco, s2 == 1 ? BF3P_S2 : BF3P_DECONV);
        if (!fn) continue;
        const int tm = 16 * ppw;
        const size_t slots = s2 == 1 ? (size_t)4 * tm + 2 * W + 2 + 1 : (size_t)tm + W + 1 + 1;
        const size_t tile = slots * (3 * (L.cin / 8) + 2) * 16;
        const size_t red = (size_t)wco * ks * ppw * nt * 1024;
        const size_t lds = tile > red ? tile : red;
        if (lds > 160 * 1024) continue;
        sh[0] = nt; sh[1] = ppw; sh[2] = ks; sh[3] = wco;
        *lds_out = lds;
        return fn;
    }
    return nullptr;
}

// y = conv2d(name, [elu](x), n_out, stride=[2,2]) (tf_train.py:33,36; layers.py:31-64: SAME, so window (i,j) covers input rows 2i..2i+2)
// split into n_outs tensors like iaf_conv3x3_forward.  x [B,n_in,2H,2W]; H, W = the OUTPUT size.  Nine taps per c_in on H x W pixels --
// a quarter of the stride-1 conv + subsampling it replaces.  IAF_ERR_UNSUPPORTED when the four staged phase tiles do not fit LDS
// (then: iaf_conv3x3_forward at [2H,2W] + iaf_resample2 DOWN_ODD, the same numbers).
extern "C" int iaf_conv3x3_forward_stride2(iaf_conv3x3_t* c, const float* x, int elu_input, float* const* outs, const int* out_channels,
                                           int n_outs, int B, int H, int W, void* stream) {
    if (c && c->theano_plain) return IAF_ERR_UNSUPPORTED;
    if (!c || !x || !outs || !out_channels) return IAF_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || n_outs < 1 || n_outs > MAXSPLIT) return IAF_ERR_SHAPE;
    if ((long long)B * H * W > (1LL << 30) / 64) return IAF_ERR_SHAPE;
    if (!c->prepared) return IAF_ERR_NOT_PREPARED;
    int tot = 0, ends[MAXSPLIT];
    for (int k = 0; k < n_outs; ++k) {
        if (!outs[k]) return IAF_ERR_NULL;
        if (out_channels[k] <= 0) return IAF_ERR_SHAPE;
        tot += out_channels[k];
        ends[k] = tot;
    }
    if (tot != c->n_out) return IAF_ERR_SHAPE;
    GemmLayer& L = c->L;
    if (c->generic || c->mask_mode || c->deconv || !L.wp3 || !conv_split(c)) return IAF_ERR_UNSUPPORTED;
    if (!(c->packs & IAF_PACK_BF16X3)) return IAF_ERR_NOT_PREPARED;     // (iaf_conv3x3_set_packs: the strided form reads the bf16 planes)
    for (int k = 0; k < n_outs; ++k)
        if (ends[k] & 3) return IAF_ERR_UNSUPPORTED;
    int sh[4]; size_t lds = 0;
    conv_fn_t fn = s2_shape(L, 1, W, sh, &lds);
    if (!fn) return IAF_ERR_UNSUPPORTED;
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.B = B; p.H = H; p.W = W; p.HW = H * W; p.P = B * H * W;
    p.x = x; p.in_elu = elu_input ? 1 : 0;
    p.nsplit = n_outs;
    for (int k = 0; k < MAXSPLIT; ++k) {
        p.split_end[k] = ends[k < n_outs ? k : n_outs - 1];
        p.split_ptr[k] = outs[k < n_outs ? k : n_outs - 1];
    }
    const int tm = 16 * sh[1];
    p.wp = (const float*)L.wp3; p.bias = L.bias;
    p.s2_pb[0] = 0; p.s2_pb[1] = tm + W + 1; p.s2_pb[2] = p.s2_pb[1] + tm + W; p.s2_pb[3] = p.s2_pb[2] + tm + 1;
    p.nslot = p.s2_pb[3] + tm;
    p.halo_before = 0;
    for (int t = 0; t < MAXTAPS; ++t) {
        const int di = t / 3, dj = t % 3;
        p.tap_dh[t] = di >> 1; p.tap_dw[t] = dj >> 1;
        p.tap_off[t] = p.s2_pb[(di & 1) * 2 + (dj & 1)] + (di >> 1) * W + (dj >> 1);
    }
    p.cin = L.cin; p.cout = L.cout; p.nchunk = L.nchunk; p.ncot = L.ncot; p.cp = L.cin + 8;
    int rc = raise_lds_cap((const void*)fn, lds);
    if (rc) return rc;
    dim3 grid((p.P + tm - 1) / tm, L.ncot / (sh[0] * sh[3]));
    p.gx = (int)grid.x;
    p.lds_bytes = (int)lds;
    hipLaunchKernelGGL(fn, grid, dim3(64 * sh[2] * sh[3]), lds, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

// out = [residual upsampled +] 0.1 x deconv2d(name, [elu](concat(x[:, :c_split], x2)), n_out) (tf_train.py:87-94; layers.py:83-112) for a
// conv prepared by iaf_conv3x3_prepare_deconv.  x (, x2) [B,.,H,W] -- H, W = the INPUT size --, out [B,n_out,2H,2W], residual
// [B,n_out,H,W] or NULL (without it: out = the deconv itself).  Each of the four output phases (2i+a, 2j+b) is a conv of the
// low-resolution input with the 4 / 2 / 2 / 1 filter taps that meet non-zero rows of the zero-inserted image: nine taps per input pixel
// instead of 36.  IAF_ERR_UNSUPPORTED: run iaf_conv3x3_forward on the zero-inserted inputs (same numbers up to fp32 rounding).
extern "C" int iaf_conv3x3_forward_deconv(iaf_conv3x3_t* c, const float* x, const float* x2, int c_split, int elu_input,
                                          const float* residual, float* out, int B, int H, int W, void* stream) {
    if (c && c->theano_plain) return IAF_ERR_UNSUPPORTED;
    if (!c || !x || !out) return IAF_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0) return IAF_ERR_SHAPE;
    if ((long long)B * H * W > (1LL << 30) / 256) return IAF_ERR_SHAPE;
    if (!c->prepared) return IAF_ERR_NOT_PREPARED;
    if (x2 && (c_split <= 0 || c_split >= c->n_in)) return IAF_ERR_SHAPE;
    GemmLayer& L = c->L;
    if (!c->deconv) return IAF_ERR_NOT_PREPARED;
    if (c->generic || c->mask_mode || !L.wp3 || L.nchunk % 2 != 0 || !conv_split(c)) return IAF_ERR_UNSUPPORTED;
    if ((x2 && (c_split & 3)) || (L.cout & 3)) return IAF_ERR_UNSUPPORTED;
    int sh[4]; size_t lds = 0;
    conv_fn_t fn = s2_shape(L, 2, W, sh, &lds);
    if (!fn) return IAF_ERR_UNSUPPORTED;
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.B = B; p.H = H; p.W = W; p.HW = H * W; p.P = B * H * W;
    p.x = x; p.x2 = x2; p.c_split = c_split; p.in_elu = elu_input ? 1 : 0; p.res = residual;
    p.nsplit = 1;
    for (int k = 0; k < MAXSPLIT; ++k) { p.split_end[k] = c->n_out; p.split_ptr[k] = out; }
    const int tm = 16 * sh[1];
    p.wp = (const float*)L.wp3; p.bias = L.bias;
    // tap (di,dj) of the rotated filter on the zero-inserted image = rows i-1 (di = 0) or i (di = 1, 2) of the input
    for (int t = 0; t < MAXTAPS; ++t) { p.tap_dh[t] = (t / 3 == 0) ? -1 : 0; p.tap_dw[t] = (t % 3 == 0) ? -1 : 0; }
    p.halo_before = W + 1;
    p.nslot = tm + W + 1;
    p.cin = L.cin; p.cout = L.cout; p.nchunk = L.nchunk; p.ncot = L.ncot; p.cp = L.cin + 8;
    int rc = raise_lds_cap((const void*)fn, lds);
    if (rc) return rc;
    dim3 grid((p.P + tm - 1) / tm, L.ncot / (sh[0] * sh[3]), 4);
    p.gx = (int)grid.x;
    p.lds_bytes = (int)lds;
    hipLaunchKernelGGL(fn, grid, dim3(64 * sh[2] * sh[3]), lds, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

// arithmetic of the forward conv: IAF_PRECISION_BF16X3 (default: split products on the bf16 matrix cores where a launch
// shape covers the problem, fp32-grade) or IAF_PRECISION_F32 (the exact-fp32 MFMA kernel always)
// which packs the prep launches of a plain conv keep up to date (as iaf_stack_set_packs): a conv that runs at ONE size needs one
extern "C" int iaf_conv3x3_set_packs(iaf_conv3x3_t* c, int packs) {
    if (!c) return IAF_ERR_NULL;
    if (c->theano_plain && packs == IAF_PACK_F16X2) return IAF_ERR_UNSUPPORTED;
    PackFacts f;
    f.generic = c->generic; f.masked = c->mask_mode != 0; f.training = c->training; f.deconv = c->deconv;
    f.all_split = c->L.wp3 != nullptr; f.f16_active = conv_f16_active(c);
    return pack_conv_set_packs(*c, packs, f);
}
extern "C" int iaf_conv3x3_set_precision(iaf_conv3x3_t* c, int precision) {
    if (!c) return IAF_ERR_NULL;
    if (c->theano_plain && precision == IAF_PRECISION_F16X2) return IAF_ERR_UNSUPPORTED;
    if (precision != IAF_PRECISION_F32 && precision != IAF_PRECISION_BF16X3 && precision != IAF_PRECISION_F16X2) return IAF_ERR_SHAPE;
    bool new_pack = false;
    if (precision == IAF_PRECISION_F16X2) {
        GemmLayer& L = c->L;
        if (c->generic || c->mask_mode || !L.wp3 || c->theano_plain) return IAF_ERR_UNSUPPORTED;       // (plain convs with c_in % 32 == 0: the same fragments, two planes)
        if (int rc = c->rng.alloc()) return rc;
        if (!L.wp2) {
            HIP_TRY(hipMalloc(&L.wp2, pack_bytes_split(L, MAXTAPS, 2)));
            new_pack = true;
        }
    }
    return pack_set_precision(*c, PACK_CONV, precision, new_pack, c->rng.peek()) ? c->rng.rearm() : IAF_OK;
}
extern "C" int iaf_conv3x3_range_errors(const iaf_conv3x3_t* c, unsigned* errors) {
    if (!c || !errors) return IAF_ERR_NULL;
    return c->rng.read(errors);
}
// 1 if a forward call at this size would run the bf16x3 kernel
extern "C" int iaf_conv3x3_runs_bf16x3(iaf_conv3x3_t* c, int B, int H, int W) {
    if (!c || c->generic || c->mask_mode || c->deconv || !conv_split(c)) return 0;
    GemmLayer t = c->L;
    return conv3x3_bf3_shape(t, c->bf3_choice, (long long)B * H * W, W, conv_f16_active(c)) ? 1 : 0;
}
// ... and on two fp16 planes (the split-product launch of this size is an F16 instantiation)
extern "C" int iaf_conv3x3_runs_f16x2(iaf_conv3x3_t* c, int B, int H, int W) {
    if (!iaf_conv3x3_runs_bf16x3(c, B, H, W) || !conv_f16_active(c)) return 0;
    GemmLayer t = c->L;
    if (!conv3x3_bf3_shape(t, c->bf3_choice, (long long)B * H * W, W, true)) return 0;
    return pick_bf3p(t.b_nt, t.b_ppw, t.b_pxt, t.b_ks, t.b_wco, BF3P_F16) ? 1 : 0;
}

extern "C" int iaf_conv3x3_autotune(iaf_conv3x3_t* c, const float* x, const float* x2, int c_split, int elu_input,
                                    const float* residual, float* const* outs, const int* out_channels, int n_outs, int B,
                                    int H, int W, int reps, void* stream, int* best_shape, float* best_us) {
    if (!c) return IAF_ERR_NULL;
    if (c->theano_plain) return IAF_ERR_UNSUPPORTED;
    if (c->generic) return IAF_OK;
    if (reps <= 0) reps = 20;
    hipStream_t st = (hipStream_t)stream;
    GemmLayer& L = c->L;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    float best = 1e30f;
    int bsh[4] = {L.nt, L.pxt, L.wco, L.ks};
    int rc = IAF_OK;
    c->bf3_choice = 3;                  // first the exact-fp32 kernel in every shape ...
    for (int si = 0; si < (int)std::size(k_conv_shapes) && rc == IAF_OK; ++si)
        for (int nt = 5; nt >= 1 && rc == IAF_OK; --nt) {
            const int pxt = k_conv_shapes[si].pxt, wco = k_conv_shapes[si].wco, ks = k_conv_shapes[si].ks;
            if (L.ncot % (nt * wco) != 0 || L.nchunk < ks) continue;
            GemmLayer t = L;
            t.nt = nt; t.pxt = pxt; t.wco = wco; t.ks = ks;
            if (conv_lds_bytes(t, W) > 160 * 1024) continue;
            L.nt = nt; L.pxt = pxt; L.wco = wco; L.ks = ks; L.user_tuned = true;
            for (int r = 0; r < 3 && rc == IAF_OK; ++r)
                rc = iaf_conv3x3_forward(c, x, x2, c_split, elu_input, residual, outs, out_channels, n_outs, B, H, W, stream);
            if (rc == IAF_ERR_UNSUPPORTED) { rc = IAF_OK; continue; }
            if (rc) break;
            (void)hipEventRecord(e0, st);
            for (int r = 0; r < reps && rc == IAF_OK; ++r)
                rc = iaf_conv3x3_forward(c, x, x2, c_split, elu_input, residual, outs, out_channels, n_outs, B, H, W, stream);
            (void)hipEventRecord(e1, st);
            if (rc) break;
            if ((rc = (int)hipEventSynchronize(e1)) != 0) break;
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            if (ms < best) { best = ms; bsh[0] = nt; bsh[1] = pxt; bsh[2] = wco; bsh[3] = ks; }
        }
    L.nt = bsh[0]; L.pxt = bsh[1]; L.wco = bsh[2]; L.ks = bsh[3]; L.user_tuned = true;
    // ... and the same conv on the bf16 matrix cores, every compiled 9-tap shape
    int bz[5] = {0, 0, 0, 0, 1};
    if (rc == IAF_OK && L.wp3 && conv_split(c) && !c->mask_mode && !c->deconv) {
        static const int nts[3] = {5, 4, 2};
        for (int si = 0; si < (int)std::size(k_bf3p_shapes) && rc == IAF_OK; ++si)
            for (int nt : nts) {
                const auto& sh = k_bf3p_shapes[si];
                if (!bf3_ragged_ok(L.ncot, nt * sh.wco)) continue;
                L.b_nt = nt; L.b_ppw = sh.ppw; L.b_pxt = sh.pxt; L.b_ks = sh.ks; L.b_wco = sh.wco;
                c->bf3_choice = 2;
                GemmLayer t = L;
                if (!conv3x3_bf3_shape(t, 2, (long long)B * H * W, W)) continue;
                for (int r = 0; r < 3 && rc == IAF_OK; ++r)
                    rc = iaf_conv3x3_forward(c, x, x2, c_split, elu_input, residual, outs, out_channels, n_outs, B, H, W, stream);
                if (rc) break;
                (void)hipEventRecord(e0, st);
                for (int r = 0; r < reps && rc == IAF_OK; ++r)
                    rc = iaf_conv3x3_forward(c, x, x2, c_split, elu_input, residual, outs, out_channels, n_outs, B, H, W, stream);
                (void)hipEventRecord(e1, st);
                if (rc) break;
                if ((rc = (int)hipEventSynchronize(e1)) != 0) break;
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, e0, e1);
                if (ms < best) { best = ms; bz[0] = nt; bz[1] = sh.ppw; bz[2] = sh.pxt; bz[3] = sh.ks; bz[4] = sh.wco; }
            }
        if (bz[0]) { L.b_nt = bz[0]; L.b_ppw = bz[1]; L.b_pxt = bz[2]; L.b_ks = bz[3]; L.b_wco = bz[4]; c->bf3_choice = 2; }
        else c->bf3_choice = 3;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (best_shape) {
        if (bz[0]) { best_shape[0] = -bz[0]; best_shape[1] = bz[1]; best_shape[2] = bz[4]; best_shape[3] = bz[3]; }   // (-nt, ppw, wco, ks)
        else for (int i = 0; i < 4; ++i) best_shape[i] = bsh[i];
    }
    if (best_us) *best_us = best * 1e3f / reps;
    return rc;
}

extern "C" int iaf_conv3x3_work(const iaf_conv3x3_t* c, int B, int H, int W, double* flops, double* bytes) {
    if (!c) return IAF_ERR_NULL;
    const double P = (double)B * H * W;
    if (flops) *flops = 2.0 * c->L.live_macs_per_px * P;
    // input + output activations once, raw V/g/b once
    if (bytes) *bytes = 4.0 * (P * (c->n_in + c->n_out) + 9.0 * c->n_in * c->n_out + 2.0 * c->n_out);
    return IAF_OK;
}

// ---------------------------------------------------------------------------------------------
// backward of a plain conv (what TF's autodiff derives for layers.py:52-64 inside IAFLayer, tf_train.py:138):
//   forward   y = conv(a, w) + b,  a = act(concat(x, x2)),  w = exp(g) V / ||V||_o
//   given     dY (as up to 6 NCHW tensors -- the gradients of the split outputs -- times dy_scale)
//   computes  dX = [dx_residual +] act'(.) * (W^T dY)   -> NCHW, split like the forward concat
//             dV, dg (through the weight norm), db
// Passes: (1) pack dY and a pixel-major, (2) data gradient = the SAME conv kernel on the transposed packs with mirrored
// taps (EPI_DGRAD, 9 taps), (3) MFMA weight gradient over pixel ranges + reduce, (4) weight-norm backward.
// ---------------------------------------------------------------------------------------------
extern "C" int iaf_conv3x3_set_debug(iaf_conv3x3_t* c, void* buf, size_t bytes) {
    if (!c) return IAF_ERR_NULL;
    c->L.dbg = (unsigned long long*)buf; c->L.dbg_bytes = buf ? bytes : 0;
    c->T.dbg = c->L.dbg; c->T.dbg_bytes = c->L.dbg_bytes;      // (the data gradient runs the transposed problem T)
    return IAF_OK;
}

extern "C" int iaf_conv3x3_set_training(iaf_conv3x3_t* c, int on) {
    if (!c) return IAF_ERR_NULL;
    if (c->mask_mode) return IAF_ERR_UNSUPPORTED;
    if (!on) { c->training = false; return IAF_OK; }
    if (c->generic) {         // channel counts outside the MFMA path: the direct backward kernels (iaf_kernels_generic.hpp), no extra packs
        c->training = true;
        return IAF_OK;
    }
    GemmLayer& L = c->L;
    // the transposed pack, also as bf16x3 (iaf_pack_t3_kernel: the data gradient on the bf16 matrix cores, even K tile counts) and as two
    // fp16 planes: the data gradient of a conv whose arithmetic is IAF_PRECISION_F16X2 (iaf_conv_bf3.hpp DG16; IAF_DGRAD_F16=0: dev knob)
    static const bool dg16_env = !(getenv("IAF_DGRAD_F16") && getenv("IAF_DGRAD_F16")[0] == '0');
    if (int rc = gemm_layer_set_training(L, c->T, MAXTAPS, dg16_env)) return rc;
    c->training = true; c->dgrad_pinned = false;
    pack_set_training(*c);    // (training keeps every pack)
    return IAF_OK;
}

#define CONV_BRD_SLABS 64      // pixel slabs of the Theano plain conv's border-tap sums (iaf_border9_sum_kernel)
// which family the data gradient runs (conv3x3_bf3_shape's `choice`): bf16x3 unless the conv's precision is fp32 or a backward search
// measured the fp32 kernel faster at this size; 2 = the pinned shape (iaf_conv3x3_set_dgrad_tuning)
static int conv3x3_dgrad_choice(const iaf_conv3x3* c, long long P, int W) {
    if (!conv_split(c) || c->bf3_choice == 3 || !c->T.wp3) return 3;
    if (c->dgrad_pinned) return 2;
    return (c->T.tuned_P == P && c->T.tuned_W == W && !c->T.tuned_bf3) ? 3 : 1;
}
struct ConvTrainWs { float* xe; float* dyc; float* part; float* dW; float* dbp; unsigned short* tapmask; float* dbrd; };
static size_t conv3x3_train_ws_floats(const iaf_conv3x3* c, long long P, ConvTrainWs* o, float* base) {
    size_t off = 0;
    auto take = [&](size_t n) { float* q = base ? base + off : nullptr; off += (n + 63) / 64 * 64; return q; };
    ConvTrainWs t;
    t.xe = take((size_t)P * c->n_in);
    t.dyc = take((size_t)P * c->n_out);
    t.part = take((size_t)WGRAD_MAX_RANGES * MAXTAPS * c->n_in * c->n_out);
    t.dW = take((size_t)MAXTAPS * c->n_in * c->n_out);
    t.dbp = take((size_t)256 * c->n_out);
    t.tapmask = (unsigned short*)take(((size_t)P + 1) / 2);
    t.dbrd = c->theano_plain ? take((size_t)CONV_BRD_SLABS * (MAXTAPS - 1) * c->n_out) : nullptr;
    if (o) *o = t;
    return off;
}

extern "C" size_t iaf_conv3x3_train_workspace_bytes(const iaf_conv3x3_t* c, int B, int H, int W) {
    if (!c || B <= 0 || H <= 0 || W <= 0) return 0;
    return conv3x3_train_ws_floats(c, (long long)B * H * W, nullptr, nullptr) * sizeof(float);
}

static void pack_fill(PackP& p, const float* const* src, const int* chans, int n, float* dst, int C, int HW, int P, float scale, int elu) {
    memset(&p, 0, sizeof(p));
    int tot = 0;
    for (int k = 0; k < n; ++k) { tot += chans[k]; p.src[k] = src[k]; p.end[k] = tot; }
    p.nsrc = n; p.dst = dst; p.C = C; p.HW = HW; p.P = P; p.scale = scale; p.elu = elu;
}
// the two backward operands of a conv in one launch (blockIdx.z): dY (scaled) and [elu](concat(x, x2))
static int pack_pixmajor2(const PackP& a, const PackP& b, hipStream_t st) {
    PackP2 pp;
    pp.t[0] = a; pp.t[1] = b;
    const int C = a.C > b.C ? a.C : b.C;
    hipLaunchKernelGGL(iaf_pack_pixmajor_kernel, dim3((a.P + 63) / 64, (C + 63) / 64, 2), dim3(256), 0, st, pp);
    return (int)hipGetLastError();
}

extern "C" int iaf_conv3x3_backward(iaf_conv3x3_t* c, const float* x, const float* x2, int c_split, int elu_input,
                                    const float* const* dys, const int* dy_channels, int n_dys, float dy_scale,
                                    float* const* dxs, const int* dx_channels, int n_dxs, const float* dx_residual,
                                    const float* V, const float* g, float* dV, float* dg, float* db, int B, int H, int W,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!c || !x || !dys || !dy_channels || !V || !g || !dV || !dg || !db || !workspace) return IAF_ERR_NULL;
    if (!c->training || !c->prepared) return IAF_ERR_NOT_PREPARED;
    if (B <= 0 || H <= 0 || W <= 0 || n_dys < 1 || n_dys > MAXSPLIT || n_dxs < 0 || n_dxs > MAXSPLIT) return IAF_ERR_SHAPE;
    if ((long long)B * H * W > (1LL << 30) / 64) return IAF_ERR_SHAPE;
    if (x2 && (c_split <= 0 || c_split >= c->n_in || (c_split & 3))) return IAF_ERR_SHAPE;
    if (n_dxs && (!dxs || !dx_channels)) return IAF_ERR_NULL;
    if (dx_residual && n_dxs != 1) return IAF_ERR_SHAPE;
    int tot = 0;
    for (int k = 0; k < n_dys; ++k) {
        if (!dys[k]) return IAF_ERR_NULL;
        if (dy_channels[k] <= 0 || (dy_channels[k] & 3)) return IAF_ERR_SHAPE;
        tot += dy_channels[k];
    }
    if (tot != c->n_out) return IAF_ERR_SHAPE;
    int dends[MAXSPLIT];
    tot = 0;
    for (int k = 0; k < n_dxs; ++k) {
        if (!dxs[k]) return IAF_ERR_NULL;
        if (dx_channels[k] <= 0 || (dx_channels[k] & 3)) return IAF_ERR_SHAPE;
        tot += dx_channels[k];
        dends[k] = tot;
    }
    if (n_dxs && tot != c->n_in) return IAF_ERR_SHAPE;
    if (((uintptr_t)workspace & 15) != 0 || workspace_bytes < iaf_conv3x3_train_workspace_bytes(c, B, H, W)) return IAF_ERR_WORKSPACE;
    const int P = B * H * W, HW = H * W;
    ConvTrainWs tw;
    conv3x3_train_ws_floats(c, P, &tw, (float*)workspace);
    hipStream_t st = (hipStream_t)stream;
    GemmLayer& L = c->L;
    int rc;
    if (c->generic) {
        // channel counts outside the MFMA path: direct loops over the NCHW tensors as they are (iaf_kernels_generic.hpp)
        if (c->deconv) return IAF_ERR_UNSUPPORTED;
        GenGradP p;
        memset(&p, 0, sizeof(p));
        int e = 0;
        for (int k = 0; k < n_dys; ++k) { e += dy_channels[k]; p.dy[k] = dys[k]; p.dy_end[k] = e; }
        p.ndy = n_dys; p.dy_scale = dy_scale;
        p.x = x; p.x2 = x2; p.c_split = c_split; p.in_elu = elu_input ? 1 : 0;
        p.w = L.wp; p.ntaps = MAXTAPS; p.B = B; p.H = H; p.W = W; p.cin = L.cin; p.cout = L.cout;
        for (int k = 0; k < n_dxs; ++k) { p.dx[k] = dxs[k]; p.dx_end[k] = dends[k]; }
        p.ndx = n_dxs; p.res = dx_residual;
        p.dW = tw.dW; p.db = tw.dbp;
        if (n_dxs) hipLaunchKernelGGL(iaf_generic_dgrad_kernel, ew_grid((size_t)P * L.cin), dim3(256), 0, st, p);
        hipLaunchKernelGGL(iaf_generic_wgrad_kernel, dim3((unsigned)((size_t)MAXTAPS * L.cin * L.cout + L.cout)), dim3(256), 0, st, p);
        GenWnBwdP wn;
        memset(&wn, 0, sizeof(wn));
        wn.V[0] = V; wn.g[0] = g; wn.dV[0] = dV; wn.dg[0] = dg; wn.db[0] = db;
        wn.dW = tw.dW; wn.dbsum = tw.dbp; wn.cin = L.cin; wn.cout_each = L.cout; wn.npair = 1; wn.ntaps = MAXTAPS;
        hipLaunchKernelGGL(iaf_generic_wn_bwd_kernel, dim3(L.cout), dim3(256), 0, st, wn);
        c->pending = false;
        return (int)hipGetLastError();
    }
    // (1) operands, pixel-major.  The column sums of dY (db's partials, one row per 64 pixels) come out of the same launch while they
    // fit the 256 rows the buffers hold (P <= 16384); beyond that the reduce launch below sums them over larger slabs, as before.
    const bool fold_db = (P + 63) / 64 <= 256;
    {
        const float* xs[2] = {x, x2};
        const int xc[2] = {x2 ? c_split : c->n_in, c->n_in - c_split};
        PackP pa, pb;
        pack_fill(pa, dys, dy_channels, n_dys, tw.dyc, c->n_out, HW, P, dy_scale, 0);
        if (fold_db) pa.colsum = c->defer_wn ? c->own_dbp : tw.dbp;      // the bias gradient's partials, while the tile is in LDS
        pack_fill(pb, xs, xc, x2 ? 2 : 1, tw.xe, c->n_in, HW, P, 1.0f, elu_input ? 1 : 0);
        if ((rc = pack_pixmajor2(pa, pb, st))) return rc;
    }
    // (2) data gradient
    if (n_dxs) {
        ConvP p;
        memset(&p, 0, sizeof(p));
        p.B = B; p.H = H; p.W = W; p.HW = HW; p.P = P;
        p.x = tw.dyc; p.mode = MODE_DGRAD_PLAIN;
        p.zin = elu_input ? tw.xe : nullptr;
        p.res = dx_residual;
        p.nsplit = n_dxs;
        for (int k = 0; k < MAXSPLIT; ++k) {
            p.split_end[k] = dends[k < n_dxs ? k : n_dxs - 1];
            p.split_ptr[k] = dxs[k < n_dxs ? k : n_dxs - 1];
        }
        // bf16x3 unless the conv's precision is fp32 or a backward search measured the fp32 kernel faster at this size
        const int choice3 = conv3x3_dgrad_choice(c, P, W);
        const bool dgrad16 = pack_f16_wanted(*c) && c->T.wp2 != nullptr && !c->deconv;
        if ((rc = conv3x3_launch(c->T, p, EPI_DGRAD9, IN_PIXMAJOR, false, true, st, IAF_VARIANT_TF, choice3, nullptr, dgrad16))) return rc;
    }
    // (3) weight gradient: partials over pixel ranges, then reduce (+ column sums of dY for db)
    const unsigned short* tapmask = nullptr;
    if ((rc = tapmask_for(B, H, W, st, tw.tapmask, &tapmask))) return rc;
    if ((rc = launch_wgrad(nullptr, L, tw.xe, tw.dyc, tw.part, tapmask, B, H, W, st, 1, conv_split(c)))) return rc;
    const int nslab = fold_db ? (P + 63) / 64 : 256;
    const int px_per_slab = (P + nslab - 1) / nslab;
    float* dWbuf = c->defer_wn ? c->own_dW : tw.dW;
    float* dbpbuf = c->defer_wn ? c->own_dbp : tw.dbp;
    {
        const size_t n4 = (size_t)MAXTAPS * L.cin * L.cout / 4;
        int nblk = (int)((n4 + 255) / 256);
        if (nblk > 1024) nblk = 1024;
        hipLaunchKernelGGL(iaf_wgrad_reduce_kernel, dim3(nblk + (fold_db ? 0 : nslab)), dim3(256), 0, st, tw.part, dWbuf,
                           wgrad_nrange(P, L.cin, MAXTAPS, L.cout, conv_split(c)), n4, nblk, (const float*)tw.dyc, dbpbuf, P, L.cout, px_per_slab);
    }
    // (4) through the weight norm -- now, or in iaf_conv3x3_wn_bwd_batch_run with every other conv of the model
    if (c->deconv) {      // deconv2d's norm runs per INPUT channel over the rotated filter (layers.py:104): its own two launches
        float* inv_norm = L.bias + (size_t)L.ncot * 16;       // (scratch behind the packed bias, as in prepare_deconv)
        float* S = tw.part;                                    // the range partials are reduced by now
        hipLaunchKernelGGL(iaf_deconv_bwd_channel_kernel, dim3(L.cin), dim3(256), 0, st, V, g, (const float*)dWbuf, inv_norm, S, L.cin,
                           L.cout);
        hipLaunchKernelGGL(iaf_deconv_bwd_apply_kernel, dim3(L.cout), dim3(256), 0, st, V, g, (const float*)dWbuf,
                           (const float*)inv_norm, (const float*)S, (const float*)dbpbuf, nslab, dV, dg, db, L.cin, L.cout);
        c->pending = false;
        return (int)hipGetLastError();
    }
    if (c->defer_wn) {
        c->pend_nslab = nslab; c->pending = true;
        return (int)hipGetLastError();
    }
    WnBwdLayer w;
    memset(&w, 0, sizeof(w));
    w.V = V; w.g = g; w.dW = dWbuf; w.dbp = dbpbuf; w.dV = dV; w.dg = dg; w.db = db;
    w.cin = L.cin; w.cout = L.cout; w.cout_packed = L.cout; w.nslab = nslab; w.pack_stride = 1;
    if (c->theano_plain) {
        // the border channel's eight taps: sums of dY over the pixels whose tap leaves the image, from the tap table (the `dbrd` of the
        // stack's Theano backward, eight taps), then the Theano statement's norm (all n_in + 1 channels, exp(3 s), OIHW)
        const int nb = P < CONV_BRD_SLABS * 64 ? (P + 63) / 64 : CONV_BRD_SLABS;
        const int per = (P + nb - 1) / nb;
        hipLaunchKernelGGL(iaf_border9_sum_kernel, dim3((L.cout + 63) / 64, nb), dim3(256), 0, st, (const float*)tw.dyc, tapmask, tw.dbrd, P, L.cout, per);
        w.dbrd = tw.dbrd; w.nbrd = nb; w.variant = PREP_PLAIN9_THEANO;
        hipLaunchKernelGGL(iaf_wn_bwd_plain_theano_kernel, dim3(L.cout / 16), dim3(256), 0, st, w);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(iaf_wn_bwd_plain_kernel, dim3(L.cout / 16), dim3(256), 0, st, w);
    return (int)hipGetLastError();
}

// 1 if the data gradient of a backward call at this size would run the split products (bf16x3, or two fp16 planes where the conv's
// precision asks for them)
extern "C" int iaf_conv3x3_dgrad_runs_bf16x3(iaf_conv3x3_t* c, int B, int H, int W) {
    if (!c || c->generic || !c->training || B <= 0 || H <= 0 || W <= 0) return 0;
    const long long P = (long long)B * H * W;
    GemmLayer t = c->T;
    const bool dgrad16 = pack_f16_wanted(*c) && c->T.wp2 != nullptr && !c->deconv;
    return conv3x3_bf3_shape(t, conv3x3_dgrad_choice(c, P, W), P, W, dgrad16) && pick_bf3p(t.b_nt, t.b_ppw, t.b_pxt, t.b_ks, t.b_wco, BF3P_DGRAD) ? 1 : 0;
}
// pin the data gradient's split-product launch shape (nt, ppw, wco, ks; pxt = 1), as iaf_conv3x3_set_tuning(-nt, ...) pins the forward's;
// nt = 0: back to the size rule.  After iaf_conv3x3_set_training (which rebuilds the transposed problem).
extern "C" int iaf_conv3x3_set_dgrad_tuning(iaf_conv3x3_t* c, int nt, int ppw, int wco, int ks) {
    if (!c) return IAF_ERR_NULL;
    if (nt == 0) { c->dgrad_pinned = false; return IAF_OK; }
    if (!c->training) return IAF_ERR_NOT_PREPARED;
    GemmLayer& T = c->T;
    if (c->generic || nt < 0 || !T.wp3 || !bf3_ragged_ok(T.ncot, nt * wco) || !pick_bf3p(nt, ppw, 1, ks, wco, BF3P_DGRAD)) return IAF_ERR_UNSUPPORTED;
    T.b_nt = nt; T.b_ppw = ppw; T.b_pxt = 1; T.b_ks = ks; T.b_wco = wco;
    c->dgrad_pinned = true;
    return IAF_OK;
}

// Launch-shape search for the data gradient (the transposed problem has its own best shape): times whole
// iaf_conv3x3_backward calls -- everything but the dgrad launch is the same for every candidate -- and pins the fastest.
extern "C" int iaf_conv3x3_autotune_backward(iaf_conv3x3_t* c, const float* x, const float* x2, int c_split, int elu_input,
                                             const float* const* dys, const int* dy_channels, int n_dys, float dy_scale,
                                             float* const* dxs, const int* dx_channels, int n_dxs, const float* dx_residual,
                                             const float* V, const float* g, float* dV, float* dg, float* db, int B, int H,
                                             int W, void* workspace, size_t workspace_bytes, int reps, void* stream,
                                             int* best_shape, float* best_us) {
    if (!c) return IAF_ERR_NULL;
    if (c->theano_plain) return IAF_ERR_UNSUPPORTED;
    if (!c->training) return IAF_ERR_NOT_PREPARED;
    if (reps <= 0) reps = 10;
    hipStream_t st = (hipStream_t)stream;
    GemmLayer& T = c->T;
    if (n_dxs == 0) return IAF_OK;          // no data gradient requested: nothing to tune
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    const bool was_pending = c->pending;
    float best = 1e30f;
    int bsh[4] = {T.nt, T.pxt, T.wco, T.ks};
    int rc = IAF_OK;
    auto run = [&]() {
        return iaf_conv3x3_backward(c, x, x2, c_split, elu_input, dys, dy_channels, n_dys, dy_scale, dxs, dx_channels, n_dxs,
                                    dx_residual, V, g, dV, dg, db, B, H, W, workspace, workspace_bytes, stream);
    };
    // (the fp32 candidates run with the bf16x3 data gradient switched off: tuned_bf3 = false for this size)
    T.tuned_P = (long long)B * H * W; T.tuned_W = W; T.tuned_bf3 = false;
    for (int si = 0; si < (int)std::size(k_conv_shapes) && rc == IAF_OK; ++si)
        for (int nt = 5; nt >= 1 && rc == IAF_OK; --nt) {
            const int pxt = k_conv_shapes[si].pxt, wco = k_conv_shapes[si].wco, ks = k_conv_shapes[si].ks;
            if (T.ncot % (nt * wco) != 0 || T.nchunk < ks) continue;
            GemmLayer t = T;
            t.nt = nt; t.pxt = pxt; t.wco = wco; t.ks = ks;
            if (conv_lds_bytes(t, W) > 160 * 1024) continue;
            if (!pick_kernel(nt, pxt, wco, ks, IN_PIXMAJOR, EPI_DGRAD9)) continue;
            T.nt = nt; T.pxt = pxt; T.wco = wco; T.ks = ks; T.user_tuned = true;
            for (int r = 0; r < 2 && rc == IAF_OK; ++r) rc = run();
            if (rc == IAF_ERR_UNSUPPORTED) { rc = IAF_OK; continue; }
            if (rc) break;
            (void)hipEventRecord(e0, st);
            for (int r = 0; r < reps && rc == IAF_OK; ++r) rc = run();
            (void)hipEventRecord(e1, st);
            if (rc) break;
            if ((rc = (int)hipEventSynchronize(e1)) != 0) break;
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            if (ms < best) { best = ms; bsh[0] = nt; bsh[1] = pxt; bsh[2] = wco; bsh[3] = ks; }
        }
    // ... and the bf16x3 data gradient in its rule shape (conv3x3_bf3_shape), if this conv has the transposed bf16x3 pack
    bool bf3_wins = false;
    if (rc == IAF_OK && T.wp3 && c->bf3_choice != 3 && conv_split(c)) {
        T.user_tuned = false;
        T.tuned_bf3 = true;
        for (int r = 0; r < 2 && rc == IAF_OK; ++r) rc = run();
        if (rc == IAF_OK) {
            (void)hipEventRecord(e0, st);
            for (int r = 0; r < reps && rc == IAF_OK; ++r) rc = run();
            (void)hipEventRecord(e1, st);
            float ms = 0.f;
            if (rc == IAF_OK && (rc = (int)hipEventSynchronize(e1)) == 0) {
                (void)hipEventElapsedTime(&ms, e0, e1);
                if (ms < best) { best = ms; bf3_wins = true; }
            }
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    T.tuned_bf3 = bf3_wins;
    if (bf3_wins) { bsh[0] = -T.b_nt; bsh[1] = T.b_ppw; bsh[2] = T.b_wco; bsh[3] = T.b_ks; }       // reported like the forward's bf16x3 shapes
    // remember the winner for THIS problem size only (t_* hold (nt, pxt, wco, ks) here): a backward at another size goes
    // back to the automatic shape instead of inheriting a shape tuned -- and LDS-sized -- for this one
    T.user_tuned = false;
    T.tuned_P = (long long)B * H * W; T.tuned_W = W;
    if (!bf3_wins) { T.t_nt = bsh[0]; T.t_ppw = bsh[1]; T.t_pxt = bsh[2]; T.t_ks = bsh[3]; }
    if (rc == IAF_OK) rc = run();           // leave the outputs as computed with the chosen shape
    (void)was_pending;
    if (best_shape) for (int i = 0; i < 4; ++i) best_shape[i] = bsh[i];
    if (best_us) *best_us = best * 1e3f / reps;
    return rc;
}

// ---- deferred weight-norm backward of many plain convs in one launch ----------------------------------------------
extern "C" int iaf_conv3x3_set_defer_weightnorm(iaf_conv3x3_t* c, int on) {
    if (!c) return IAF_ERR_NULL;
    if (on && c->theano_plain) return IAF_ERR_UNSUPPORTED;
    if (on && !c->training) return IAF_ERR_NOT_PREPARED;
    if (on) {
        if (!c->own_dW) HIP_TRY(hipMalloc(&c->own_dW, (size_t)MAXTAPS * c->n_in * c->n_out * sizeof(float)));
        if (!c->own_dbp) HIP_TRY(hipMalloc(&c->own_dbp, (size_t)256 * c->n_out * sizeof(float)));
    }
    c->defer_wn = on != 0;
    c->pending = false;
    return IAF_OK;
}

struct iaf_conv3x3_wn_bwd_batch {
    std::vector<iaf_conv3x3*> convs;
    BatchTable<WnBwdLayer> t;      // one descriptor per conv
};

extern "C" int iaf_conv3x3_wn_bwd_batch_destroy(iaf_conv3x3_wn_bwd_batch_t* b) {
    if (!b) return IAF_ERR_NULL;
    b->t.destroy();
    delete b;
    return IAF_OK;
}

extern "C" int iaf_conv3x3_wn_bwd_batch_create(iaf_conv3x3_wn_bwd_batch_t** out, iaf_conv3x3_t* const* convs, int n) {
    if (!out || !convs) return IAF_ERR_NULL;
    *out = nullptr;
    if (n <= 0) return IAF_ERR_SHAPE;
    for (int i = 0; i < n; ++i)
        if (convs[i] && convs[i]->theano_plain) return IAF_ERR_UNSUPPORTED;
    std::vector<int> tiles;
    if (int rc = conv_batch_tiles(convs, n, &tiles)) return rc;
    iaf_conv3x3_wn_bwd_batch* b = new (std::nothrow) iaf_conv3x3_wn_bwd_batch();
    if (!b) return (int)hipErrorOutOfMemory;
    b->convs.assign(convs, convs + n);
    if (int rc = b->t.create(tiles, true)) { iaf_conv3x3_wn_bwd_batch_destroy(b); return rc; }
    for (int i = 0; i < n; ++i) {
        const GemmLayer& L = convs[i]->L;
        WnBwdLayer& w = b->t.h[i];
        w.cin = L.cin; w.cout = L.cout; w.cout_packed = L.cout; w.pack_stride = 1;
    }
    *out = b;
    return IAF_OK;
}

extern "C" int iaf_conv3x3_wn_bwd_batch_run(iaf_conv3x3_wn_bwd_batch_t* b, const float* const* V, const float* const* g,
                                            float* const* dV, float* const* dg, float* const* db, void* stream) {
    if (!b || !V || !g || !dV || !dg || !db) return IAF_ERR_NULL;
    for (int i = 0; i < b->t.n; ++i) {
        const iaf_conv3x3* c = b->convs[i];
        if (!c->defer_wn || (!c->pending && !c->deconv)) return IAF_ERR_NOT_PREPARED;
        if (!V[i] || !g[i] || !dV[i] || !dg[i] || !db[i]) return IAF_ERR_NULL;
        b->t.set(i, [&](WnBwdLayer& w) {
            w.skip = c->deconv ? 1 : 0;        // a deconv2d pushes its gradient through its own norm inside iaf_conv3x3_backward
            w.V = V[i]; w.g = g[i]; w.dV = dV[i]; w.dg = dg[i]; w.db = db[i];
            w.dW = c->own_dW; w.dbp = c->own_dbp; w.nslab = c->pend_nslab;
        });
    }
    hipStream_t st = (hipStream_t)stream;
    const WnBwdLayer* d_layers = nullptr;
    if (int rc = b->t.upload(st, &d_layers)) return rc;
    hipLaunchKernelGGL(iaf_wn_bwd_plain_batch_kernel, dim3(b->t.ntiles), dim3(256), 0, st, d_layers, b->t.d_tile2layer, b->t.d_tile_begin);
    return (int)hipGetLastError();
}
