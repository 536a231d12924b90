// iaf_model_ops.hip -- the operations of the model that take no stack and no conv (C ABI: include/iaf_hip.h): the two ends of the model
// around the IAFLayer stack (image scaling, x_enc / x_dec and their backward, h_top, obj / loss), the elementwise pieces of the init
// pass, and the objective side (Gaussian sample / logps, the 'up_iaf2_nl' backward halves, the elementwise path of the
// 'down_iaf2_nl2' chain and of the 'made' prior, the importance-weighted bound, the evaluation tail, data-dependent init, the likelihood, 2x resampling).
// A translation unit of its own beside iaf_engine.hip; its kernel headers are included here and nowhere else.
// Not here: iaf_kl_free_bits / _gate / _grouped.  They launch iaf_kl_rowsum_kernel and iaf_kl_finish_kernel, which the posterior block
// of the stack launches too (iaf_kernels_misc.hpp), and a kernel is defined in one unit and launched from that unit only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>

#include "iaf_hip.h"

#include "iaf_common.hpp"
#include "iaf_kernels_edge.hpp"
#include "iaf_kernels_objective.hpp"

// ---- the two ends of the model, forward (iaf_kernels_edge.hpp) -------------------------------------------------------------------
extern "C" int iaf_image_to_float(const unsigned char* x, float* out, int B, size_t n_per_image, int k, void* stream) {
    if (!x || !out) return IAF_ERR_NULL;
    if (B <= 0 || k <= 0 || n_per_image == 0) return IAF_ERR_SHAPE;
    const size_t total = (size_t)B * k * n_per_image;
    hipLaunchKernelGGL(iaf_image_to_float_kernel, ew_grid(total), dim3(256), 0, (hipStream_t)stream, x, out, n_per_image, total, k);
    return (int)hipGetLastError();
}

extern "C" int iaf_convk_weightnorm(const float* V, const float* g, float* w, int kh, int kw, int n_in, int n_out, int deconv,
                                    void* stream) {
    if (!V || !g || !w) return IAF_ERR_NULL;
    if (kh <= 0 || kw <= 0 || n_in <= 0 || n_out <= 0) return IAF_ERR_SHAPE;
    // conv: V [kh,kw,n_in,n_out] -> one workgroup per n_out; deconv: V [kh,kw,n_out,n_in] -> one per n_in
    hipLaunchKernelGGL(iaf_convk_weightnorm_kernel, dim3(deconv ? n_in : n_out), dim3(256), 0, (hipStream_t)stream, V, g, w, kh * kw,
                       deconv ? n_out : n_in, deconv ? n_in : n_out, deconv ? 1 : 0);
    return (int)hipGetLastError();
}

// TF "SAME": out = ceil(n / s), total padding max((out - 1) s + k - n, 0), the smaller half first
static void same_pad(int n, int k, int s, int* out, int* before) {
    *out = (n + s - 1) / s;
    int tot = (*out - 1) * s + k - n;
    if (tot < 0) tot = 0;
    *before = tot / 2;
}

extern "C" int iaf_convk_forward(const float* x, const float* w, const float* b, float* y, int B, int n_in, int H, int W, int n_out,
                                 int kh, int kw, int stride, int elu_input, void* stream) {
    if (!x || !w || !b || !y) return IAF_ERR_NULL;
    if (B <= 0 || n_in <= 0 || n_out <= 0 || H <= 0 || W <= 0 || kh <= 0 || kw <= 0 || stride <= 0) return IAF_ERR_SHAPE;
    ConvKP p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.w = w; p.b = b; p.y = y; p.B = B; p.n_in = n_in; p.H = H; p.W = W; p.n_out = n_out; p.kh = kh; p.kw = kw;
    p.stride = stride; p.elu = elu_input ? 1 : 0;
    same_pad(H, kh, stride, &p.OH, &p.pad_t);
    same_pad(W, kw, stride, &p.OW, &p.pad_l);
    const size_t npx = (size_t)B * p.OH * p.OW;
    if (npx > (1u << 30)) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_convk_forward_kernel, dim3((unsigned)((npx + 255) / 256), (n_out + CK_NO - 1) / CK_NO), dim3(256), 0,
                       (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

extern "C" int iaf_deconvk_forward(const float* x, const float* w, const float* b, float* y, int B, int n_in, int H, int W, int n_out,
                                   int kh, int kw, int stride, int elu_input, float clip_lo, float clip_hi, void* stream) {
    if (!x || !w || !b || !y) return IAF_ERR_NULL;
    if (B <= 0 || n_in <= 0 || n_out <= 0 || H <= 0 || W <= 0 || kh <= 0 || kw <= 0 || stride <= 0) return IAF_ERR_SHAPE;
    ConvKP p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.w = w; p.b = b; p.y = y; p.B = B; p.n_in = n_in; p.H = H; p.W = W; p.n_out = n_out; p.kh = kh; p.kw = kw;
    p.stride = stride; p.elu = elu_input ? 1 : 0; p.clip_lo = clip_lo; p.clip_hi = clip_hi;
    p.OH = H * stride; p.OW = W * stride;
    int o;
    same_pad(p.OH, kh, stride, &o, &p.pad_t);       // the forward conv this transposes maps [OH, OW] -> [H, W]
    same_pad(p.OW, kw, stride, &o, &p.pad_l);
    const size_t npx = (size_t)B * H * W;
    if (npx > (1u << 30) || stride > 8) return IAF_ERR_SHAPE;
    // dynamic LDS: the weights of one output phase, at most ceil(kh/s) ceil(kw/s) taps x DK_NO channels x n_in
    const size_t wl_bytes = (size_t)((kh + stride - 1) / stride) * ((kw + stride - 1) / stride) * DK_NO * n_in * sizeof(float);
    if (wl_bytes > 60 * 1024) return IAF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(iaf_deconvk_forward_kernel, dim3((unsigned)((npx + 15) / 16), stride * stride, (n_out + DK_NO - 1) / DK_NO),
                       dim3(256), wl_bytes, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

extern "C" int iaf_tile_channels(const float* v, float* out, int B, int C, int HW, void* stream) {
    if (!v || !out) return IAF_ERR_NULL;
    if (B <= 0 || C <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    const size_t total = (size_t)B * C * HW;
    hipLaunchKernelGGL(iaf_tile_channels_kernel, ew_grid(total), dim3(256), 0, (hipStream_t)stream, v, out, total, C, HW);
    return (int)hipGetLastError();
}

extern "C" int iaf_sum_axpy(const float* a, const float* b, float sb, float* out, int n, void* stream) {
    if (!a || !out) return IAF_ERR_NULL;
    if (n <= 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_sum_axpy_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a, b, sb, out, n);
    return (int)hipGetLastError();
}

// ---- the two ends of the model, backward -------------------------------------------------------------------------------------------
extern "C" int iaf_discretized_logistic_backward(const float* mean, const float* logscale, const float* sample, float up, float clip_lo,
                                                 float clip_hi, float* d_mean, float* d_logscale_rows, int B, size_t n_per_row,
                                                 float binsize, void* stream) {
    if (!mean || !logscale || !sample || !d_mean || !d_logscale_rows) return IAF_ERR_NULL;
    if (B <= 0 || n_per_row == 0 || !(binsize > 0.f)) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_discretized_logistic_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, mean, logscale, sample, up, clip_lo,
                       clip_hi, d_mean, d_logscale_rows, n_per_row, binsize);
    return (int)hipGetLastError();
}

extern "C" int iaf_convk_wgrad(const float* x, const float* dy, float* dW, int B, int n_small, int H, int W, int n_big, int kh, int kw,
                               int stride, int elu_x, int elu_dy, void* stream) {
    if (!x || !dy || !dW) return IAF_ERR_NULL;
    if (B <= 0 || n_small <= 0 || n_big <= 0 || H <= 0 || W <= 0 || kh <= 0 || kw <= 0 || stride <= 0) return IAF_ERR_SHAPE;
    ConvKWP p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.dy = dy; p.dW = dW; p.B = B; p.n_small = n_small; p.H = H; p.W = W; p.n_big = n_big; p.kh = kh; p.kw = kw;
    p.stride = stride; p.elu_x = elu_x ? 1 : 0; p.elu_dy = elu_dy ? 1 : 0;
    same_pad(H, kh, stride, &p.OH, &p.pad_t);
    same_pad(W, kw, stride, &p.OW, &p.pad_l);
    if ((long long)B * p.OH * p.OW > (1LL << 24)) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_convk_wgrad_kernel, dim3(kh * kw * n_small, (n_big + 15) / 16), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

// dV (V's layout), dg [n_out]; deconv: scratch = n_in * n_out floats
extern "C" int iaf_convk_weightnorm_backward(const float* V, const float* g, const float* dW, float* dV, float* dg, float* scratch,
                                             int kh, int kw, int n_in, int n_out, int deconv, void* stream) {
    if (!V || !g || !dW || !dV || !dg || (deconv && !scratch)) return IAF_ERR_NULL;
    if (kh <= 0 || kw <= 0 || n_in <= 0 || n_out <= 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_convk_weightnorm_bwd_kernel, dim3(deconv ? n_in : n_out), dim3(256), 0, (hipStream_t)stream, V, g, dW, dV,
                       deconv ? scratch : dg, kh * kw, deconv ? n_out : n_in, deconv ? n_in : n_out, deconv ? 1 : 0);
    HIP_TRY(hipGetLastError());
    if (deconv) return iaf_colsum(scratch, dg, n_in, n_out, stream);
    return IAF_OK;
}

extern "C" int iaf_channel_sum(const float* x, float* out, int B, int C, int HW, void* stream) {
    if (!x || !out) return IAF_ERR_NULL;
    if (B <= 0 || C <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_channel_sum_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, x, out, B, C, HW);
    return (int)hipGetLastError();
}

extern "C" int iaf_mul_elu_grad(const float* g, const float* h, float* out, size_t n, void* stream) {
    if (!g || !h || !out) return IAF_ERR_NULL;
    if (n == 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_mul_elu_grad_kernel, ew_grid(n), dim3(256), 0, (hipStream_t)stream, g, h, out, n);
    return (int)hipGetLastError();
}

// ---- elementwise pieces of the data-dependent init pass (mode "init", tf_train.py:60-61, 70-71, 94, 208) -----------------------------
extern "C" int iaf_axpby(const float* a, float sa, const float* b, float sb, float* out, size_t n, void* stream) {
    if (!a || !b || !out) return IAF_ERR_NULL;
    if (n == 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_axpby_kernel, ew_grid(n), dim3(256), 0, (hipStream_t)stream, a, sa, b, sb, out, n);
    return (int)hipGetLastError();
}
extern "C" int iaf_affine_transform(const float* z, const float* m, const float* s, float scale, float* out, size_t n, void* stream) {
    if (!z || !m || !s || !out) return IAF_ERR_NULL;
    if (n == 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_affine_kernel, ew_grid(n), dim3(256), 0, (hipStream_t)stream, z, m, s, scale, out, n);
    return (int)hipGetLastError();
}
extern "C" int iaf_clip(const float* x, float lo, float hi, float* out, size_t n, void* stream) {
    if (!x || !out) return IAF_ERR_NULL;
    if (n == 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_clip_kernel, ew_grid(n), dim3(256), 0, (hipStream_t)stream, x, lo, hi, out, n);
    return (int)hipGetLastError();
}

// eps' with (qm+rm) + exp(ql+rl) * eps' == z: the posterior noise that reproduces a given sample z (iaf_kernels_objective.hpp)
extern "C" int iaf_noise_from_sample(const float* z, const float* qz_mean, const float* qz_logsd, const float* rz_mean,
                                     const float* rz_logsd, float* eps_out, size_t n, void* stream) {
    if (!z || !qz_mean || !qz_logsd || !rz_mean || !rz_logsd || !eps_out) return IAF_ERR_NULL;
    if (n == 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_noise_from_sample_kernel, ew_grid(n), dim3(256), 0, (hipStream_t)stream, z, qz_mean, qz_logsd, rz_mean,
                       rz_logsd, eps_out, n);
    return (int)hipGetLastError();
}

extern "C" int iaf_datainit_normalize(const float* x_init, const float* add, float* y, float* g, float* b, int B, int C,
                                      int HW, float init_scale, void* stream) {
    if (!x_init || !g || !b) return IAF_ERR_NULL;
    if (B <= 0 || C <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_datainit_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, x_init, add, y, g, b, B, C, HW, init_scale);
    return (int)hipGetLastError();
}

// 2x resampling of an NCHW tensor (modes: IAF_RESAMPLE_* in include/iaf_hip.h); H, W = size of the SMALLER tensor
extern "C" int iaf_resample2(const float* src, float* dst, int B, int C, int H, int W, int mode, void* stream) {
    if (!src || !dst) return IAF_ERR_NULL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || mode < 0 || mode > 5) return IAF_ERR_SHAPE;
    const bool down = (mode == IAF_RESAMPLE_DOWN_EVEN || mode == IAF_RESAMPLE_DOWN_ODD || mode == IAF_RESAMPLE_DOWN_SUM4);
    const size_t n_dst = (size_t)B * C * H * W * (down ? 1 : 4);
    hipLaunchKernelGGL(iaf_resample2_kernel, ew_grid(n_dst), dim3(256), 0, (hipStream_t)stream, src, dst, n_dst, H, W, mode);
    return (int)hipGetLastError();
}

// ---- the objective side (iaf_kernels_objective.hpp) --------------------------------------------------------------------------------
extern "C" int iaf_gaussian_sample(const float* mean, const float* logvar, const float* noise, float* out, size_t n,
                                   void* stream) {
    if (!mean || !logvar || !noise || !out) return IAF_ERR_NULL;
    if (n == 0) return IAF_OK;
    hipLaunchKernelGGL(iaf_gauss_sample_kernel, ew_grid(n), dim3(256), 0, (hipStream_t)stream, mean, logvar, noise, out, n, 1.0f);
    return (int)hipGetLastError();
}

extern "C" int iaf_gaussian_sample_logsd(const float* mean, const float* logsd, const float* noise, float* out, size_t n,
                                         void* stream) {
    if (!mean || !logsd || !noise || !out) return IAF_ERR_NULL;
    if (n == 0) return IAF_OK;
    hipLaunchKernelGGL(iaf_gauss_sample_kernel, ew_grid(n), dim3(256), 0, (hipStream_t)stream, mean, logsd, noise, out, n, 2.0f);
    return (int)hipGetLastError();
}

extern "C" int iaf_gaussian_logps(const float* mean, const float* logvar, const float* sample, float* out, size_t n,
                                  void* stream) {
    if (!mean || !logvar || !sample || !out) return IAF_ERR_NULL;
    if (n == 0) return IAF_OK;
    hipLaunchKernelGGL(iaf_gauss_logps_kernel, ew_grid(n), dim3(256), 0, (hipStream_t)stream, mean, logvar, sample, out, n, 1.0f);
    return (int)hipGetLastError();
}

extern "C" int iaf_gaussian_logps_logsd(const float* mean, const float* logsd, const float* sample, float* out, size_t n,
                                        void* stream) {
    if (!mean || !logsd || !sample || !out) return IAF_ERR_NULL;
    if (n == 0) return IAF_OK;
    hipLaunchKernelGGL(iaf_gauss_logps_kernel, ew_grid(n), dim3(256), 0, (hipStream_t)stream, mean, logsd, sample, out, n, 2.0f);
    return (int)hipGetLastError();
}

// kl = logq0 + logdet - logp: models.py:175,298,328 when the three terms come from separate launches (posterior
// 'up_iaf2_nl': the IAF step runs in the up pass, the prior is only known in the down pass)
extern "C" int iaf_kl_combine(const float* logq0, const float* logdet, const float* logp, float* kl, size_t n, void* stream) {
    if (!logq0 || !logdet || !logp || !kl) return IAF_ERR_NULL;
    if (n == 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_kl_combine_kernel, ew_grid(n), dim3(256), 0, (hipStream_t)stream, logq0, logdet, logp, kl, n);
    return (int)hipGetLastError();
}

// out[j] = sum_i mat[i][j]: the per-row KL costs of all layers of a model -> sum_kl_costs (tf_train.py:198-200:
// `kl_cost += cur_cost` over the layer loop), the second argument of compute_lowerbound
extern "C" int iaf_colsum(const float* mat, float* out, int m, int n, void* stream) {
    if (!mat || !out) return IAF_ERR_NULL;
    if (m <= 0 || n <= 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_colsum_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, mat, out, m, n);
    return (int)hipGetLastError();
}

// The elementwise halves of the backward of models.cvae_layer 'up_iaf2_nl' around iaf_step_backward (iaf_kernels_objective.hpp:
// UpIafBwdP).  gate [n_z] non-NULL: free bits, G = gate[c] * gscale; else G = dko[b].
extern "C" int iaf_up_iaf2_backward_pre(const float* z, const float* pz_mean, const float* pz_logsd, const float* d_h, const float* d_up,
                                        const float* gate, float gscale, const float* dko, float* dz_tot, float* G, float* d_down_conv1,
                                        int B, int n_h, int n_z, int HW, void* stream) {
    if (!z || !pz_mean || !pz_logsd || !d_h || !dz_tot || !G || !d_down_conv1 || (!gate && !dko)) return IAF_ERR_NULL;
    if (B <= 0 || n_h <= 0 || n_z <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    UpIafBwdP p;
    memset(&p, 0, sizeof(p));
    p.z = z; p.pz_mean = pz_mean; p.pz_logsd = pz_logsd; p.d_h = d_h; p.d_up = d_up; p.gate = gate; p.dko = dko; p.gscale = gscale;
    p.dz_tot = dz_tot; p.Gf = G; p.d_dc1 = d_down_conv1; p.B = B; p.n_h = n_h; p.n_z = n_z; p.HW = HW;
    hipLaunchKernelGGL(iaf_up_iaf2_bwd_pre_kernel, ew_grid((size_t)B * (n_h + 2 * n_z) * HW), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

extern "C" int iaf_up_iaf2_backward_post(const float* dz0, const float* z0, const float* qz_mean, const float* G, const float* dctx,
                                         const float* d_up, float* d_up_conv1, int B, int n_h, int n_z, int HW, void* stream) {
    if (!dz0 || !z0 || !qz_mean || !G || !dctx || !d_up_conv1) return IAF_ERR_NULL;
    if (B <= 0 || n_h <= 0 || n_z <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    UpIafBwdP p;
    memset(&p, 0, sizeof(p));
    p.dz0 = dz0; p.z0 = z0; p.qz_mean = qz_mean; p.Gf = const_cast<float*>(G); p.dctx = dctx; p.d_up = d_up; p.d_uc1 = d_up_conv1;
    p.B = B; p.n_h = n_h; p.n_z = n_z; p.HW = HW;
    hipLaunchKernelGGL(iaf_up_iaf2_bwd_post_kernel, ew_grid((size_t)B * (2 * n_h + 2 * n_z) * HW), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

// The elementwise path of models.cvae_layer 'down_iaf2_nl2' around its two IAF steps (iaf_kernels_objective.hpp: ChainP), in place on
// the two conv outputs.  The 16-byte form runs only where every plane of every tensor starts on a 16-byte boundary.
static bool chain_vec4(int HW, std::initializer_list<const void*> ptrs) {
    if (HW % 4) return false;
    for (const void* q : ptrs)
        if ((uintptr_t)q & 15) return false;          // (NULL, an absent optional tensor, passes)
    return true;
}
#define CHAIN_LAUNCH(kernel, vec, n, st, p)                                                                         \
    do {                                                                                                            \
        if (vec) hipLaunchKernelGGL(kernel<4>, ew_grid((n) / 4), dim3(256), 0, (hipStream_t)(st), p);               \
        else hipLaunchKernelGGL(kernel<1>, ew_grid(n), dim3(256), 0, (hipStream_t)(st), p);                         \
    } while (0)

extern "C" int iaf_chain_head(const float* up_conv1_out, const float* down_conv1_out, const float* eps, float* z0, float* logq0,
                              float* context, int B, int n_h, int n_z, int HW, void* stream) {
    if (!up_conv1_out || !down_conv1_out || !eps || !z0 || !logq0 || !context) return IAF_ERR_NULL;
    if (B <= 0 || n_h <= 0 || n_z <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    ChainP p;
    memset(&p, 0, sizeof(p));
    p.up = up_conv1_out; p.down = down_conv1_out; p.eps = eps; p.o_z0 = z0; p.o_logq0 = logq0; p.o_context = context;
    p.B = B; p.n_h = n_h; p.n_z = n_z; p.HW = HW;
    const bool vec = chain_vec4(HW, {up_conv1_out, down_conv1_out, eps, z0, logq0, context});
    CHAIN_LAUNCH(iaf_chain_head_kernel, vec, (size_t)B * ((size_t)n_h + n_z) * HW, stream, p);
    return (int)hipGetLastError();
}

extern "C" int iaf_chain_tail(const float* down_conv1_out, const float* logq0, const float* logdet1, const float* logdet2,
                              const float* z2, float* kl_elem, float* h_out, int B, int n_h, int n_z, int HW, void* stream) {
    if (!down_conv1_out || !logq0 || !logdet1 || !logdet2 || !z2 || !kl_elem || !h_out) return IAF_ERR_NULL;
    if (B <= 0 || n_h <= 0 || n_z <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    ChainP p;
    memset(&p, 0, sizeof(p));
    p.down = down_conv1_out; p.logq0 = logq0; p.s1 = logdet1; p.s2 = logdet2; p.z2 = z2; p.o_kl = kl_elem; p.o_h = h_out;
    p.B = B; p.n_h = n_h; p.n_z = n_z; p.HW = HW;
    const bool vec = chain_vec4(HW, {down_conv1_out, logq0, logdet1, logdet2, z2, kl_elem, h_out});
    CHAIN_LAUNCH(iaf_chain_tail_kernel, vec, (size_t)B * ((size_t)n_h + n_z) * HW, stream, p);
    return (int)hipGetLastError();
}

// gate [n_z] non-NULL: free bits, G = gate[c] * gscale; else G = dko[b] (the convention of iaf_up_iaf2_backward_pre)
extern "C" int iaf_chain_backward_pre(const float* down_conv1_out, const float* z2, const float* d_h, const float* gate, float gscale,
                                      const float* dko, float* dz2, float* G, float* d_down_conv1, int B, int n_h, int n_z, int HW,
                                      void* stream) {
    if (!down_conv1_out || !z2 || !d_h || !dz2 || !G || !d_down_conv1 || (!gate && !dko)) return IAF_ERR_NULL;
    if (B <= 0 || n_h <= 0 || n_z <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    ChainP p;
    memset(&p, 0, sizeof(p));
    p.down = down_conv1_out; p.z2 = z2; p.d_h = d_h; p.gate = gate; p.gscale = gscale; p.dko = dko; p.o_dz2 = dz2; p.o_G = G;
    p.o_ddc1 = d_down_conv1; p.B = B; p.n_h = n_h; p.n_z = n_z; p.HW = HW;
    const bool vec = chain_vec4(HW, {down_conv1_out, z2, d_h, dz2, G, d_down_conv1});
    CHAIN_LAUNCH(iaf_chain_bwd_pre_kernel, vec, (size_t)B * ((size_t)n_h + 2 * (size_t)n_z) * HW, stream, p);
    return (int)hipGetLastError();
}

extern "C" int iaf_chain_backward_post(const float* up_conv1_out, const float* down_conv1_out, const float* z0, const float* dz0,
                                       const float* G, const float* dctx1, const float* dctx2, const float* d_up, float* d_up_conv1,
                                       float* d_down_conv1, int B, int n_h, int n_z, int HW, void* stream) {
    if (!up_conv1_out || !down_conv1_out || !z0 || !dz0 || !G || !dctx1 || !dctx2 || !d_up_conv1 || !d_down_conv1) return IAF_ERR_NULL;
    if (B <= 0 || n_h <= 0 || n_z <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    ChainP p;
    memset(&p, 0, sizeof(p));
    p.up = up_conv1_out; p.down = down_conv1_out; p.z0 = z0; p.dz0 = dz0; p.G = G; p.dctx1 = dctx1; p.dctx2 = dctx2; p.d_up = d_up;
    p.o_duc1 = d_up_conv1; p.o_ddc1 = d_down_conv1; p.B = B; p.n_h = n_h; p.n_z = n_z; p.HW = HW;
    const bool vec = chain_vec4(HW, {up_conv1_out, down_conv1_out, z0, dz0, G, dctx1, dctx2, d_up, d_up_conv1, d_down_conv1});
    CHAIN_LAUNCH(iaf_chain_bwd_post_kernel, vec, (size_t)B * (2 * (size_t)n_h + 2 * (size_t)n_z) * HW, stream, p);
    return (int)hipGetLastError();
}
// The elementwise path of models.cvae_layer with prior 'made' around the posterior's steps and the prior's step (iaf_kernels_objective.hpp:
// MadeP), in place on the two conv outputs; down_conv1_out has 3 n_h + 2 n_z channels here.
extern "C" int iaf_made_head(const float* up_conv1_out, const float* down_conv1_out, const float* eps, float* z0, float* logq0,
                             float* context, float* made_context, int B, int n_h, int n_z, int HW, void* stream) {
    if (!up_conv1_out || !down_conv1_out || !eps || !z0 || !logq0 || !context || !made_context) return IAF_ERR_NULL;
    if (B <= 0 || n_h <= 0 || n_z <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    MadeP p;
    memset(&p, 0, sizeof(p));
    p.up = up_conv1_out; p.down = down_conv1_out; p.eps = eps; p.o_z0 = z0; p.o_logq0 = logq0; p.o_context = context;
    p.o_mctx = made_context; p.B = B; p.n_h = n_h; p.n_z = n_z; p.HW = HW;
    const bool vec = chain_vec4(HW, {up_conv1_out, down_conv1_out, eps, z0, logq0, context, made_context});
    CHAIN_LAUNCH(iaf_made_head_kernel, vec, (size_t)B * (2 * (size_t)n_h + n_z) * HW, stream, p);
    return (int)hipGetLastError();
}

// kl_elem NULL: only h_out = [h_det | z] is written, and logq0, logdet1, u, s_p may be NULL; logdet2 NULL: one posterior flow
extern "C" int iaf_made_tail(const float* down_conv1_out, const float* logq0, const float* logdet1, const float* logdet2, const float* z,
                             const float* u, const float* s_p, float* kl_elem, float* h_out, int B, int n_h, int n_z, int HW,
                             void* stream) {
    if (!down_conv1_out || !z || !h_out || (kl_elem && (!logq0 || !logdet1 || !u || !s_p))) return IAF_ERR_NULL;
    if (B <= 0 || n_h <= 0 || n_z <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    MadeP p;
    memset(&p, 0, sizeof(p));
    p.down = down_conv1_out; p.z = z; p.o_h = h_out; p.B = B; p.n_h = n_h; p.n_z = n_z; p.HW = HW;
    bool vec = chain_vec4(HW, {down_conv1_out, z, h_out});
    if (kl_elem) {
        p.logq0 = logq0; p.s1 = logdet1; p.s2 = logdet2; p.u = u; p.s_p = s_p; p.o_kl = kl_elem;
        vec = vec && chain_vec4(HW, {logq0, logdet1, logdet2, u, s_p, kl_elem});
    }
    CHAIN_LAUNCH(iaf_made_tail_kernel, vec, (size_t)B * ((size_t)n_h + n_z) * HW, stream, p);
    return (int)hipGetLastError();
}

// gate [n_z] non-NULL: free bits, G = gate[c] * gscale; else G = dko[b] (the convention of iaf_chain_backward_pre)
extern "C" int iaf_made_backward_pre(const float* u, const float* d_h, const float* gate, float gscale, const float* dko, float* du,
                                     float* G, float* d_down_conv1, int B, int n_h, int n_z, int HW, void* stream) {
    if (!u || !d_h || !du || !G || !d_down_conv1 || (!gate && !dko)) return IAF_ERR_NULL;
    if (B <= 0 || n_h <= 0 || n_z <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    MadeP p;
    memset(&p, 0, sizeof(p));
    p.u = u; p.d_h = d_h; p.gate = gate; p.gscale = gscale; p.dko = dko; p.o_du = du; p.o_G = G; p.o_ddc1 = d_down_conv1;
    p.B = B; p.n_h = n_h; p.n_z = n_z; p.HW = HW;
    const bool vec = chain_vec4(HW, {u, d_h, du, G, d_down_conv1});
    CHAIN_LAUNCH(iaf_made_bwd_pre_kernel, vec, (size_t)B * ((size_t)n_h + n_z) * HW, stream, p);
    return (int)hipGetLastError();
}

extern "C" int iaf_made_backward_join(const float* d_h, const float* dz_p, const float* d_made_context, float* dz, float* d_down_conv1,
                                      int B, int n_h, int n_z, int HW, void* stream) {
    if (!d_h || !dz_p || !d_made_context || !dz || !d_down_conv1) return IAF_ERR_NULL;
    if (B <= 0 || n_h <= 0 || n_z <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    MadeP p;
    memset(&p, 0, sizeof(p));
    p.d_h = d_h; p.dz_p = dz_p; p.d_mctx = d_made_context; p.o_dz = dz; p.o_ddc1 = d_down_conv1;
    p.B = B; p.n_h = n_h; p.n_z = n_z; p.HW = HW;
    const bool vec = chain_vec4(HW, {d_h, dz_p, d_made_context, dz, d_down_conv1});
    CHAIN_LAUNCH(iaf_made_bwd_join_kernel, vec, (size_t)B * ((size_t)n_h + n_z) * HW, stream, p);
    return (int)hipGetLastError();
}

extern "C" int iaf_made_backward_post(const float* up_conv1_out, const float* down_conv1_out, const float* z0, const float* dz0,
                                      const float* G, const float* dctx1, const float* dctx2, const float* d_up, float* d_up_conv1,
                                      float* d_down_conv1, int B, int n_h, int n_z, int HW, void* stream) {
    if (!up_conv1_out || !down_conv1_out || !z0 || !dz0 || !G || !dctx1 || !d_up_conv1 || !d_down_conv1) return IAF_ERR_NULL;
    if (B <= 0 || n_h <= 0 || n_z <= 0 || HW <= 0) return IAF_ERR_SHAPE;
    MadeP p;
    memset(&p, 0, sizeof(p));
    p.up = up_conv1_out; p.down = down_conv1_out; p.z0 = z0; p.dz0 = dz0; p.G = G; p.dctx1 = dctx1; p.dctx2 = dctx2; p.d_up = d_up;
    p.o_duc1 = d_up_conv1; p.o_ddc1 = d_down_conv1; p.B = B; p.n_h = n_h; p.n_z = n_z; p.HW = HW;
    const bool vec = chain_vec4(HW, {up_conv1_out, down_conv1_out, z0, dz0, G, dctx1, dctx2, d_up, d_up_conv1, d_down_conv1});
    CHAIN_LAUNCH(iaf_made_bwd_post_kernel, vec, (size_t)B * (2 * (size_t)n_h + 2 * (size_t)n_z) * HW, stream, p);
    return (int)hipGetLastError();
}

// down_p with the diag prior: down_conv1_out [B, n_down, HW] in any diag layout, n_down >= n_h + 2 n_z
extern "C" int iaf_diag_prior_sample(const float* down_conv1_out, const float* eps, float* h_out, int B, int n_down, int n_h, int n_z,
                                     int HW, void* stream) {
    if (!down_conv1_out || !eps || !h_out) return IAF_ERR_NULL;
    if (B <= 0 || n_h <= 0 || n_z <= 0 || HW <= 0 || (long long)n_down < (long long)n_h + 2LL * n_z) return IAF_ERR_SHAPE;
    MadeP p;
    memset(&p, 0, sizeof(p));
    p.down = down_conv1_out; p.eps = eps; p.o_h = h_out; p.B = B; p.n_h = n_h; p.n_z = n_z; p.HW = HW; p.n_down = n_down;
    const bool vec = chain_vec4(HW, {down_conv1_out, eps, h_out});
    CHAIN_LAUNCH(iaf_diag_prior_sample_kernel, vec, (size_t)B * ((size_t)n_h + n_z) * HW, stream, p);
    return (int)hipGetLastError();
}
#undef CHAIN_LAUNCH

extern "C" int iaf_discretized_logistic(const float* mean, const float* logscale, int logscale_is_scalar, const float* sample,
                                        float* out, int B, size_t n_per_row, float binsize, void* stream) {
    if (!mean || !logscale || !sample || !out) return IAF_ERR_NULL;
    if (B <= 0 || n_per_row == 0 || !(binsize > 0.f)) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_disc_logistic_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, mean, logscale,
                       logscale_is_scalar ? 1 : 0, sample, out, n_per_row, binsize);
    return (int)hipGetLastError();
}

extern "C" int iaf_lowerbound_stream_init(float* run_max, float* run_sum, int n, void* stream) {
    if (!run_max || !run_sum) return IAF_ERR_NULL;
    if (n <= 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_lb_init_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, run_max, run_sum, n);
    return (int)hipGetLastError();
}

extern "C" int iaf_lowerbound_stream_update(float* run_max, float* run_sum, const float* log_pxz, const float* sum_kl,
                                            int n, int k_chunk, void* stream) {
    if (!run_max || !run_sum || !log_pxz || !sum_kl) return IAF_ERR_NULL;
    if (n <= 0 || k_chunk <= 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_lb_update_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, run_max, run_sum,
                       log_pxz, sum_kl, n, k_chunk);
    return (int)hipGetLastError();
}

extern "C" int iaf_lowerbound_stream_finalize(const float* run_max, const float* run_sum, float* out, int n,
                                              int k_total, void* stream) {
    if (!run_max || !run_sum || !out) return IAF_ERR_NULL;
    if (n <= 0 || k_total <= 0) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_lb_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, run_max, run_sum,
                       out, n, k_total);
    return (int)hipGetLastError();
}

// the tail of an evaluation pass and the epoch's record (iaf_kernels_objective.hpp: iaf_eval_tail_kernel): one workgroup per batch row
static_assert(sizeof(EvalRec) == 32, "the evaluation record is 32 bytes (include/iaf_hip.h)");
extern "C" int iaf_eval_reset(void* record, float* run_max, float* run_sum, int n, void* stream) {
    if (!record || !run_max || !run_sum) return IAF_ERR_NULL;
    if (n < 1 || n > 65535) return IAF_ERR_SHAPE;
    if (((uintptr_t)record & 7) != 0) return IAF_ERR_WORKSPACE;
    hipLaunchKernelGGL(iaf_eval_reset_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (EvalRec*)record, run_max,
                       run_sum, n);
    return (int)hipGetLastError();
}

extern "C" int iaf_eval_tail(const float* x_out, const float* dec_log_stdv, const float* x, size_t n_per_row, float binsize,
                             const float* layer_cost, int n_layers, int n, float* run_max, float* run_sum, int k,
                             const long long* indices, float* per_image, float* bound, void* record, void* stream) {
    if (!x_out || !dec_log_stdv || !x || !layer_cost || !run_max || !run_sum || !bound || !record) return IAF_ERR_NULL;
    if (per_image && !indices) return IAF_ERR_NULL;
    if (n < 1 || n > 65535 || n_layers < 1 || k < 1 || n_per_row == 0 || !(binsize > 0.f)) return IAF_ERR_SHAPE;
    if (((uintptr_t)record & 7) != 0) return IAF_ERR_WORKSPACE;
    hipLaunchKernelGGL(iaf_eval_tail_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, x_out, dec_log_stdv, x, n_per_row, binsize,
                       layer_cost, n_layers, n, run_max, run_sum, k, indices, per_image, bound, (EvalRec*)record);
    return (int)hipGetLastError();
}

extern "C" int iaf_compute_lowerbound(const float* log_pxz, const float* sum_kl, float* out, int n, int k, void* stream) {
    if (!log_pxz || !sum_kl || !out) return IAF_ERR_NULL;
    if (n <= 0 || k <= 0) return IAF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (k == 1) {
        hipLaunchKernelGGL(iaf_lb_k1_kernel, dim3((n + 255) / 256), dim3(256), 0, st, log_pxz, sum_kl, out, n);
        return (int)hipGetLastError();
    }
    // single-chunk streaming pass with the state kept in `out` itself is not possible (two words
    // per image); k>1 callers provide state through the stream API.  For convenience allocate on
    // the stream-ordered pool.
    float* state = nullptr;
    HIP_TRY(hipMallocAsync((void**)&state, 2 * (size_t)n * sizeof(float), st));
    hipLaunchKernelGGL(iaf_lb_init_kernel, dim3((n + 255) / 256), dim3(256), 0, st, state, state + n, n);
    hipLaunchKernelGGL(iaf_lb_update_kernel, dim3((n + 3) / 4), dim3(256), 0, st, state, state + n, log_pxz, sum_kl, n, k);
    hipLaunchKernelGGL(iaf_lb_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, st, state, state + n, out, n, k);
    int rc = (int)hipGetLastError();
    HIP_TRY(hipFreeAsync(state, st));
    return rc;
}
