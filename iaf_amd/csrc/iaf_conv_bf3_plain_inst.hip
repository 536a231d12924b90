// iaf_conv_bf3_plain_inst.hip -- instantiates iaf_conv_bf3_kernel with all 9 taps for the plain weight-normed conv2d around
// the IAF step (up_conv1/3, down_conv1/2, tf_train.py:36,41,53,93): NCHW input with the graph's elu / concat, EPI_PLAIN
// epilogue (bias, split store, residual), and down_conv1 in prior form (EPI_PRIOR), ONE launch shape per translation unit.
// Built by iaf_amd/build.py (iaf_variants.def).
#include "iaf_conv_bf3.hpp"

#ifndef IAF_WCO
#define IAF_WCO 1
#endif
#ifndef IAF_PPW
#error "compile with -DIAF_PPW=.. -DIAF_PXT=.. -DIAF_KS=.. -DIAF_S2=.."
#endif

#define IAF_CAT_(a, b, c, d, e) a##b##_##c##_##d##_##e
#define IAF_CAT(a, b, c, d, e) IAF_CAT_(a, b, c, d, e)

// NT = 2, 4, 5.  (WCO = 3: 768 threads, three waves per SIMD, 170 registers -- NT = 5 does not fit and is not instantiated;
// the prior form works in two-tile units: NT = 2, 4)
template <int INMODE, int EPI, int S2 = 0, int F16 = 0, int BCLS = 0>
static conv_fn_t pick_nt(int nt) {
    switch (nt) {
        case 2: return iaf_conv_bf3_kernel<2, IAF_PPW, IAF_PXT, IAF_KS, INMODE, EPI, IAF_WCO, MAXTAPS, S2, F16, BCLS>;
        case 4: return iaf_conv_bf3_kernel<4, IAF_PPW, IAF_PXT, IAF_KS, INMODE, EPI, IAF_WCO, MAXTAPS, S2, F16, BCLS>;
    }
    if constexpr (IAF_WCO < 3 && EPI != EPI_PRIOR)
        if (nt == 5) return iaf_conv_bf3_kernel<5, IAF_PPW, IAF_PXT, IAF_KS, INMODE, EPI, IAF_WCO, MAXTAPS, S2, F16, BCLS>;
    return nullptr;
}

extern "C" conv_fn_t IAF_CAT(iaf_pick_bf3p_, IAF_PPW, IAF_PXT, IAF_KS, IAF_WCO)(int nt, int form) {
    switch (form) {
        // the data gradient of the conv: dY pixel-major, transposed bf16x3 pack, mirrored taps (iaf_conv3x3_backward)
        case BF3P_DGRAD: return pick_nt<IN_PIXMAJOR, EPI_DGRAD>(nt);
        case BF3P_PLAIN: return pick_nt<IN_NCHW, EPI_PLAIN>(nt);
        // the plain conv of the Theano statement (graphy/nodes/conv.py:122-260): the same K loop on the flipped pack, bias from the
        // position-class table
        case BF3P_PLAIN_TH: return pick_nt<IN_NCHW, EPI_PLAIN, 0, 0, 1>(nt);
#if IAF_S2
        // the downsampling layer's strided convs at their minimal work (iaf_conv_bf3.hpp, S2): conv2d stride 2, deconv2d by phases
        case BF3P_S2: return pick_nt<IN_NCHW, EPI_PLAIN, 1>(nt);
        case BF3P_DECONV: return pick_nt<IN_NCHW, EPI_PLAIN, 2>(nt);
#endif
        // the forward on two fp16 planes (iaf_conv_bf3.hpp F16; IAF_PRECISION_F16X2): p.wp = the two-plane pack
        case BF3P_F16: return pick_nt<IN_NCHW, EPI_PLAIN, 0, 1>(nt);
        // ... and its data gradient with a tile-local scale (iaf_conv_bf3.hpp DG16): dY pixel-major, the transposed two-plane pack
        case BF3P_F16_DGRAD: return pick_nt<IN_PIXMAJOR, EPI_DGRAD, 0, 1>(nt);
        // down_conv1 in prior form (iaf_conv_bf3.hpp, EPI_PRIOR; iaf_conv3x3_forward_prior_sample), on two fp16 planes or bf16x3
        case BF3P_PRIOR_F16: return pick_nt<IN_NCHW, EPI_PRIOR, 0, 1>(nt);
        case BF3P_PRIOR: return pick_nt<IN_NCHW, EPI_PRIOR>(nt);
    }
    return nullptr;
}
