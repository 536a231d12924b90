// iaf_kernels_objective.hpp -- kernels of the objective side of the model: Gaussian sample / logps, the elementwise halves of the
// 'up_iaf2_nl' backward, the elementwise path of the 'down_iaf2_nl2' chain and of the 'made' prior, the streaming lower bound, data-dependent init, the discretized logistic, the evaluation tail, and the small
// elementwise ops around them (posterior noise of a sample, KL from its terms, column sums, 2x resampling).
// Included by iaf_model_ops.hip and by no other unit; the C ABI over these kernels is there.
#pragma once
#include "iaf_common.hpp"   // iaf_nonfinite, iaf_block_sum_f64 (the evaluation tail)

// ---------------------------------------------------------------------------------------------
// elementwise distributions (tf_utils/distributions.py)
// ---------------------------------------------------------------------------------------------
// lvs: 1 when the second tensor holds log-variances (distributions.py), 2 when it holds log standard deviations (the callers'
// `2 * logsd`: tf_train.py:56-57, rand.py:81-86 -- exact in fp32, so the bits are those of a separate doubling)
__global__ void iaf_gauss_sample_kernel(const float* mean, const float* logvar, const float* noise, float* out, size_t n, float lvs) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = mean[i] + expf(0.5f * (lvs * logvar[i])) * noise[i];
}
__global__ void iaf_gauss_logps_kernel(const float* mean, const float* logvar, const float* sample, float* out, size_t n, float lvs) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float d = sample[i] - mean[i], lv = lvs * logvar[i];
        out[i] = -0.5f * (1.8378770664093453f + lv + d * d / expf(lv));
    }
}

// ---------------------------------------------------------------------------------------------
// Backward of models.cvae_layer with posterior 'up_iaf2_nl' (models.py:168-176, 201-210, 295-298, 454-466), the elementwise
// parts on either side of iaf_step_backward.  kl = logq0 + logdet - logp(z);  G = d obj / d kl (free bits: gate[c] * gscale,
// else dko[b]).
//   pre:  dz_tot = dz + G (z - pz_mean) exp(-2 pz_logsd) [+ d_up_z]      (the gradient that enters the IAF step: -G dlogp/dz)
//         Gf = G                                                           (contiguous, the step's d logdet)
//         d_down_conv1 = [d_hdet | -G dlt e2 | G (1 - dlt^2 e2)]            (models.py:296-297 channel order)
//   post: d_up_conv1 = [d_up_hdet | dz0 | dz0 (z0 - qz_mean) - G | dctx]    (models.py:141-143; logq0 = -(log 2pi + 2 qz_logsd + eps^2)/2)
// d_h / d_up are [B, n_h + n_z, HW] (concat([h_det, z]) order, models.py:176,318), d_up may be NULL (zeros).
// ---------------------------------------------------------------------------------------------
struct UpIafBwdP {
    const float *z, *pz_mean, *pz_logsd, *d_h, *d_up, *gate, *dko;
    float *dz_tot, *Gf, *d_dc1;
    const float *dz0, *z0, *qz_mean, *dctx;
    float* d_uc1;
    float gscale;
    int B, n_h, n_z, HW;
};
__global__ __launch_bounds__(256) void iaf_up_iaf2_bwd_pre_kernel(UpIafBwdP p) {
    const size_t nh = (size_t)p.n_h * p.HW, nz = (size_t)p.n_z * p.HW, per_in = nh + nz, per_out = nh + 2 * nz;
    const size_t total = (size_t)p.B * per_out;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / per_out, r = i - b * per_out;
        if (r < nh) { p.d_dc1[i] = p.d_h[b * per_in + r]; continue; }                    // d h_det passes through
        const bool second = r >= nh + nz;
        const size_t e = r - nh - (second ? nz : 0), zi = b * nz + e;                     // element of a [B, n_z, HW] tensor
        const int c = (int)(e / p.HW);
        const float G = p.gate ? p.gate[c] * p.gscale : p.dko[b];
        const float e2 = expf(-2.0f * p.pz_logsd[zi]), dlt = p.z[zi] - p.pz_mean[zi];
        if (!second) {
            float t = p.d_h[b * per_in + nh + e] + G * dlt * e2;
            if (p.d_up) t += p.d_up[b * per_in + nh + e];
            p.dz_tot[zi] = t;
            p.Gf[zi] = G;
            p.d_dc1[i] = -G * dlt * e2;
        } else {
            p.d_dc1[i] = G * (1.0f - dlt * dlt * e2);
        }
    }
}
__global__ __launch_bounds__(256) void iaf_up_iaf2_bwd_post_kernel(UpIafBwdP p) {
    const size_t nh = (size_t)p.n_h * p.HW, nz = (size_t)p.n_z * p.HW, per_in = nh + nz, per_out = 2 * nh + 2 * nz;
    const size_t total = (size_t)p.B * per_out;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / per_out, r = i - b * per_out;
        if (r < nh) p.d_uc1[i] = p.d_up ? p.d_up[b * per_in + r] : 0.f;
        else if (r < nh + nz) p.d_uc1[i] = p.dz0[b * nz + (r - nh)];
        else if (r < nh + 2 * nz) {
            const size_t zi = b * nz + (r - nh - nz);
            p.d_uc1[i] = p.dz0[zi] * (p.z0[zi] - p.qz_mean[zi]) - p.Gf[zi];
        } else p.d_uc1[i] = p.dctx[b * nh + (r - nh - 2 * nz)];
    }
}

// ---------------------------------------------------------------------------------------------
// models.cvae_layer with posterior 'down_iaf2_nl2' (models.py:93-98, 272-291, 295-298, 317-318, 454-466): the elementwise path
// around the chain of two IAF steps, read and written IN PLACE at channel offsets of the two conv outputs
//   up   [B, 2 n_h + 2 n_z, HW] = [h_det | qz_mean | qz_logsd | up_context]                              (:141-143, 180)
//   down [B, 2 n_h + 4 n_z, HW] = [h_det | pz_mean | pz_logsd | rz_mean | rz_logsd | down_context]       (:273-279, 296-297)
// and their gradients in the same layouts.  With mean = qz_mean + rz_mean, lsd = qz_logsd + rz_logsd:
//   head: z0 = mean + exp(lsd) eps;  logq0 = -(log 2pi + 2 lsd + eps^2) / 2;  context = up_context + down_context
//   tail: kl = logq0 + s1 + s2 - logp(z2; pz_mean, 2 pz_logsd);  h_out [B, n_h + n_z, HW] = [h_det (down) | z2]
//   pre:  G = gate[c] * gscale (free bits) or dko[b];  dlt = z2 - pz_mean, e2 = exp(-2 pz_logsd);
//         dz2 = d_h[z part] + G dlt e2;  d_down[0 : n_h + 2 n_z) = [d_h[h_det part] | -G dlt e2 | G (1 - dlt^2 e2)]
//   post: dmean = dz0, dlogsd = dz0 (z0 - mean) - G, dcontext = dctx1 + dctx2;
//         d_up = [d_up_hdet or 0 | dmean | dlogsd | dcontext];  d_down[n_h + 2 n_z : ) = [dmean | dlogsd | dcontext]
// V = 4: HW % 4 == 0 and every base pointer 16-byte aligned (the entry point checks), so every channel plane starts on a 16-byte
// boundary and a thread moves four consecutive elements of one plane with one 16-byte access; V = 1: any size, any alignment.
// Consecutive threads take consecutive units of the output's own index space, so loads and stores of a wave are contiguous except
// where it straddles a channel-group boundary.
// ---------------------------------------------------------------------------------------------
template <int V> struct alignas(4 * V) ChainVec { float v[V]; };
template <int V> __device__ __forceinline__ ChainVec<V> chain_ld(const float* p) { return *reinterpret_cast<const ChainVec<V>*>(p); }
template <int V> __device__ __forceinline__ void chain_st(float* p, const ChainVec<V>& x) { *reinterpret_cast<ChainVec<V>*>(p) = x; }

struct ChainP {
    const float *up, *down, *eps, *logq0, *s1, *s2, *z2, *d_h, *gate, *dko, *z0, *dz0, *G, *dctx1, *dctx2, *d_up;
    float *o_z0, *o_logq0, *o_context, *o_kl, *o_h, *o_dz2, *o_G, *o_duc1, *o_ddc1;
    float gscale;
    int B, n_h, n_z, HW;
};

template <int V> __global__ __launch_bounds__(256) void iaf_chain_head_kernel(ChainP p) {
    const size_t nh = (size_t)p.n_h * p.HW, nz = (size_t)p.n_z * p.HW, per = nz + nh, pu = 2 * nh + 2 * nz, pd = 2 * nh + 4 * nz;
    const size_t units = (size_t)p.B * per / V;
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
        const size_t i = u * V, b = i / per, r = i - b * per;
        const float *U = p.up + b * pu, *D = p.down + b * pd;
        if (r < nz) {
            const ChainVec<V> qm = chain_ld<V>(U + nh + r), ql = chain_ld<V>(U + nh + nz + r);
            const ChainVec<V> rm = chain_ld<V>(D + nh + 2 * nz + r), rl = chain_ld<V>(D + nh + 3 * nz + r);
            const ChainVec<V> e = chain_ld<V>(p.eps + b * nz + r);
            ChainVec<V> z0, lq;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float lsd = ql.v[k] + rl.v[k];
                z0.v[k] = (qm.v[k] + rm.v[k]) + expf(lsd) * e.v[k];
                lq.v[k] = -0.5f * (1.8378770664093453f + 2.0f * lsd + e.v[k] * e.v[k]);
            }
            chain_st<V>(p.o_z0 + b * nz + r, z0);
            chain_st<V>(p.o_logq0 + b * nz + r, lq);
        } else {
            const size_t e = r - nz;
            const ChainVec<V> a = chain_ld<V>(U + nh + 2 * nz + e), c = chain_ld<V>(D + nh + 4 * nz + e);
            ChainVec<V> o;
#pragma unroll
            for (int k = 0; k < V; ++k) o.v[k] = a.v[k] + c.v[k];
            chain_st<V>(p.o_context + b * nh + e, o);
        }
    }
}

template <int V> __global__ __launch_bounds__(256) void iaf_chain_tail_kernel(ChainP p) {
    const size_t nh = (size_t)p.n_h * p.HW, nz = (size_t)p.n_z * p.HW, per = nh + nz, pd = 2 * nh + 4 * nz;
    const size_t units = (size_t)p.B * per / V;
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
        const size_t i = u * V, b = i / per, r = i - b * per;
        const float* D = p.down + b * pd;
        if (r < nh) { chain_st<V>(p.o_h + i, chain_ld<V>(D + r)); continue; }             // h_det passes through
        const size_t e = r - nh, zi = b * nz + e;
        const ChainVec<V> z = chain_ld<V>(p.z2 + zi), pm = chain_ld<V>(D + nh + e), pl = chain_ld<V>(D + nh + nz + e);
        const ChainVec<V> lq = chain_ld<V>(p.logq0 + zi), s1 = chain_ld<V>(p.s1 + zi), s2 = chain_ld<V>(p.s2 + zi);
        ChainVec<V> kl;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float dlt = z.v[k] - pm.v[k], lv = 2.0f * pl.v[k];
            const float logp = -0.5f * (1.8378770664093453f + lv + dlt * dlt * expf(-lv));
            kl.v[k] = ((lq.v[k] + s1.v[k]) + s2.v[k]) - logp;
        }
        chain_st<V>(p.o_kl + zi, kl);
        chain_st<V>(p.o_h + i, z);
    }
}

template <int V> __global__ __launch_bounds__(256) void iaf_chain_bwd_pre_kernel(ChainP p) {
    const size_t nh = (size_t)p.n_h * p.HW, nz = (size_t)p.n_z * p.HW, per_in = nh + nz, per = nh + 2 * nz, pd = 2 * nh + 4 * nz;
    const size_t units = (size_t)p.B * per / V;
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
        const size_t i = u * V, b = i / per, r = i - b * per;
        const float* D = p.down + b * pd;
        float* O = p.o_ddc1 + b * pd;
        if (r < nh) { chain_st<V>(O + r, chain_ld<V>(p.d_h + b * per_in + r)); continue; }   // d h_det passes through
        const bool second = r >= nh + nz;
        const size_t e = r - nh - (second ? nz : 0), zi = b * nz + e;
        const float G = p.gate ? p.gate[e / p.HW] * p.gscale : p.dko[b];                   // (a unit never leaves its plane)
        const ChainVec<V> z = chain_ld<V>(p.z2 + zi), pm = chain_ld<V>(D + nh + e), pl = chain_ld<V>(D + nh + nz + e);
        ChainVec<V> o;
        if (!second) {
            const ChainVec<V> dh = chain_ld<V>(p.d_h + b * per_in + nh + e);
            ChainVec<V> dz, Gv;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float e2 = expf(-2.0f * pl.v[k]), dlt = z.v[k] - pm.v[k];
                dz.v[k] = dh.v[k] + G * dlt * e2;
                Gv.v[k] = G;
                o.v[k] = -G * dlt * e2;
            }
            chain_st<V>(p.o_dz2 + zi, dz);
            chain_st<V>(p.o_G + zi, Gv);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float e2 = expf(-2.0f * pl.v[k]), dlt = z.v[k] - pm.v[k];
                o.v[k] = G * (1.0f - dlt * dlt * e2);
            }
        }
        chain_st<V>(O + r, o);
    }
}

template <int V> __global__ __launch_bounds__(256) void iaf_chain_bwd_post_kernel(ChainP p) {
    const size_t nh = (size_t)p.n_h * p.HW, nz = (size_t)p.n_z * p.HW, pu = 2 * nh + 2 * nz, pd = 2 * nh + 4 * nz;
    const size_t units = (size_t)p.B * pu / V;                       // the index space of d_up_conv1 itself
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
        const size_t i = u * V, b = i / pu, r = i - b * pu;
        ChainVec<V> o;
        if (r < nh) {
            if (p.d_up) o = chain_ld<V>(p.d_up + b * nh + r);
            else {
#pragma unroll
                for (int k = 0; k < V; ++k) o.v[k] = 0.f;
            }
            chain_st<V>(p.o_duc1 + i, o);
            continue;
        }
        if (r < nh + nz) o = chain_ld<V>(p.dz0 + b * nz + (r - nh));
        else if (r < nh + 2 * nz) {
            const size_t e = r - nh - nz, zi = b * nz + e;
            const ChainVec<V> dz0 = chain_ld<V>(p.dz0 + zi), z0 = chain_ld<V>(p.z0 + zi), G = chain_ld<V>(p.G + zi);
            const ChainVec<V> qm = chain_ld<V>(p.up + b * pu + nh + e), rm = chain_ld<V>(p.down + b * pd + nh + 2 * nz + e);
#pragma unroll
            for (int k = 0; k < V; ++k) o.v[k] = dz0.v[k] * (z0.v[k] - (qm.v[k] + rm.v[k])) - G.v[k];
        } else {
            const size_t ci = b * nh + (r - nh - 2 * nz);
            const ChainVec<V> a = chain_ld<V>(p.dctx1 + ci), c = chain_ld<V>(p.dctx2 + ci);
#pragma unroll
            for (int k = 0; k < V; ++k) o.v[k] = a.v[k] + c.v[k];
        }
        chain_st<V>(p.o_duc1 + i, o);
        chain_st<V>(p.o_ddc1 + b * pd + (nh + 2 * nz) + (r - nh), o);   // the q and the r channels get the same gradient
    }
}

// ---------------------------------------------------------------------------------------------
// models.cvae_layer with prior 'made' (models.py:36-38, 304-309) and posterior 'down_iaf2_nl' / 'down_iaf2_nl2': the elementwise path
// around the posterior's one or two IAF steps AND the prior's step, in place on the two conv outputs
//   up   [B, 2 n_h + 2 n_z, HW] = [h_det | qz_mean | qz_logsd | up_context]
//   down [B, 3 n_h + 2 n_z, HW] = [h_det | made_context | rz_mean | rz_logsd | down_context]               (:38, 273-279, 305)
// With (u, s_p) = the prior stack's step on (z, made_context), i.e. u = (z - 0.1 m) / exp(0.1 s), s_p = 0.1 s:
//   logps = -(log 2pi) / 2 - s_p - u^2 / 2                                                                 (:306-309)
//   head: z0, logq0, context as iaf_chain_head_kernel;  made_context [B, n_h, HW] = the contiguous copy the prior stack reads
//   tail: kl = ((logq0 + s1) [+ s2]) + ((log 2pi) / 2 + s_p + u^2 / 2);  h_out = [h_det | z];  kl == NULL: only h_out
//   pre:  G = gate[c] * gscale (free bits) or dko[b];  du = G u;  d_down[h_det part] = d_h[h_det part]
//   join: dz = d_h[z part] + dz_p;  d_down[made_context part] = d_made_context
//   post: as iaf_chain_bwd_post_kernel at this layout's offsets, dctx2 optional (one flow)
// diag prior, any diag layout (n_down channels, [h_det | pz_mean | pz_logsd | ...]):  h_out = [h_det | pz_mean + eps exp(pz_logsd)]
// V as for the chain; a unit never leaves its channel plane.
// ---------------------------------------------------------------------------------------------
struct MadeP {
    const float *up, *down, *eps, *logq0, *s1, *s2, *z, *u, *s_p, *d_h, *gate, *dko, *dz_p, *d_mctx, *z0, *dz0, *G, *dctx1, *dctx2, *d_up;
    float *o_z0, *o_logq0, *o_context, *o_mctx, *o_kl, *o_h, *o_du, *o_G, *o_dz, *o_duc1, *o_ddc1;
    float gscale;
    int B, n_h, n_z, HW, n_down;
};

template <int V> __global__ __launch_bounds__(256) void iaf_made_head_kernel(MadeP p) {
    const size_t nh = (size_t)p.n_h * p.HW, nz = (size_t)p.n_z * p.HW, per = nz + 2 * nh, pu = 2 * nh + 2 * nz, pd = 3 * nh + 2 * nz;
    const size_t units = (size_t)p.B * per / V;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < units; t += (size_t)gridDim.x * blockDim.x) {
        const size_t i = t * V, b = i / per, r = i - b * per;
        const float *U = p.up + b * pu, *D = p.down + b * pd;
        if (r < nz) {
            const ChainVec<V> qm = chain_ld<V>(U + nh + r), ql = chain_ld<V>(U + nh + nz + r);
            const ChainVec<V> rm = chain_ld<V>(D + 2 * nh + r), rl = chain_ld<V>(D + 2 * nh + nz + r);
            const ChainVec<V> e = chain_ld<V>(p.eps + b * nz + r);
            ChainVec<V> z0, lq;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float lsd = ql.v[k] + rl.v[k];
                z0.v[k] = (qm.v[k] + rm.v[k]) + expf(lsd) * e.v[k];
                lq.v[k] = -0.5f * (1.8378770664093453f + 2.0f * lsd + e.v[k] * e.v[k]);
            }
            chain_st<V>(p.o_z0 + b * nz + r, z0);
            chain_st<V>(p.o_logq0 + b * nz + r, lq);
        } else if (r < nz + nh) {
            const size_t e = r - nz;
            const ChainVec<V> a = chain_ld<V>(U + nh + 2 * nz + e), c = chain_ld<V>(D + 2 * nh + 2 * nz + e);
            ChainVec<V> o;
#pragma unroll
            for (int k = 0; k < V; ++k) o.v[k] = a.v[k] + c.v[k];
            chain_st<V>(p.o_context + b * nh + e, o);
        } else {
            const size_t e = r - nz - nh;
            chain_st<V>(p.o_mctx + b * nh + e, chain_ld<V>(D + nh + e));
        }
    }
}

template <int V> __global__ __launch_bounds__(256) void iaf_made_tail_kernel(MadeP p) {
    const size_t nh = (size_t)p.n_h * p.HW, nz = (size_t)p.n_z * p.HW, per = nh + nz, pd = 3 * nh + 2 * nz;
    const size_t units = (size_t)p.B * per / V;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < units; t += (size_t)gridDim.x * blockDim.x) {
        const size_t i = t * V, b = i / per, r = i - b * per;
        if (r < nh) { chain_st<V>(p.o_h + i, chain_ld<V>(p.down + b * pd + r)); continue; }   // h_det passes through
        const size_t zi = b * nz + (r - nh);
        chain_st<V>(p.o_h + i, chain_ld<V>(p.z + zi));
        if (!p.o_kl) continue;                                                               // the pack alone (down_p)
        const ChainVec<V> lq = chain_ld<V>(p.logq0 + zi), s1 = chain_ld<V>(p.s1 + zi), u = chain_ld<V>(p.u + zi), sp = chain_ld<V>(p.s_p + zi);
        ChainVec<V> kl;
        if (p.s2) {
            const ChainVec<V> s2 = chain_ld<V>(p.s2 + zi);
#pragma unroll
            for (int k = 0; k < V; ++k) kl.v[k] = (lq.v[k] + s1.v[k]) + s2.v[k];
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) kl.v[k] = lq.v[k] + s1.v[k];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) kl.v[k] += (0.9189385332046727f + sp.v[k]) + 0.5f * u.v[k] * u.v[k];
        chain_st<V>(p.o_kl + zi, kl);
    }
}

template <int V> __global__ __launch_bounds__(256) void iaf_made_bwd_pre_kernel(MadeP p) {
    const size_t nh = (size_t)p.n_h * p.HW, nz = (size_t)p.n_z * p.HW, per = nh + nz, pd = 3 * nh + 2 * nz;
    const size_t units = (size_t)p.B * per / V;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < units; t += (size_t)gridDim.x * blockDim.x) {
        const size_t i = t * V, b = i / per, r = i - b * per;
        if (r < nh) { chain_st<V>(p.o_ddc1 + b * pd + r, chain_ld<V>(p.d_h + i)); continue; }   // d h_det passes through
        const size_t e = r - nh, zi = b * nz + e;
        const float G = p.gate ? p.gate[e / p.HW] * p.gscale : p.dko[b];                      // (a unit never leaves its plane)
        const ChainVec<V> u = chain_ld<V>(p.u + zi);
        ChainVec<V> du, Gv;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            du.v[k] = G * u.v[k];
            Gv.v[k] = G;
        }
        chain_st<V>(p.o_du + zi, du);
        chain_st<V>(p.o_G + zi, Gv);
    }
}

template <int V> __global__ __launch_bounds__(256) void iaf_made_bwd_join_kernel(MadeP p) {
    const size_t nh = (size_t)p.n_h * p.HW, nz = (size_t)p.n_z * p.HW, per = nz + nh, pd = 3 * nh + 2 * nz;
    const size_t units = (size_t)p.B * per / V;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < units; t += (size_t)gridDim.x * blockDim.x) {
        const size_t i = t * V, b = i / per, r = i - b * per;
        if (r < nz) {
            const ChainVec<V> a = chain_ld<V>(p.d_h + b * per + nh + r), c = chain_ld<V>(p.dz_p + b * nz + r);
            ChainVec<V> o;
#pragma unroll
            for (int k = 0; k < V; ++k) o.v[k] = a.v[k] + c.v[k];
            chain_st<V>(p.o_dz + b * nz + r, o);
        } else {
            const size_t e = r - nz;
            chain_st<V>(p.o_ddc1 + b * pd + nh + e, chain_ld<V>(p.d_mctx + b * nh + e));
        }
    }
}

template <int V> __global__ __launch_bounds__(256) void iaf_made_bwd_post_kernel(MadeP p) {
    const size_t nh = (size_t)p.n_h * p.HW, nz = (size_t)p.n_z * p.HW, pu = 2 * nh + 2 * nz, pd = 3 * nh + 2 * nz;
    const size_t units = (size_t)p.B * pu / V;                       // the index space of d_up_conv1 itself
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < units; t += (size_t)gridDim.x * blockDim.x) {
        const size_t i = t * V, b = i / pu, r = i - b * pu;
        ChainVec<V> o;
        if (r < nh) {
            if (p.d_up) o = chain_ld<V>(p.d_up + b * nh + r);
            else {
#pragma unroll
                for (int k = 0; k < V; ++k) o.v[k] = 0.f;
            }
            chain_st<V>(p.o_duc1 + i, o);
            continue;
        }
        if (r < nh + nz) o = chain_ld<V>(p.dz0 + b * nz + (r - nh));
        else if (r < nh + 2 * nz) {
            const size_t e = r - nh - nz, zi = b * nz + e;
            const ChainVec<V> dz0 = chain_ld<V>(p.dz0 + zi), z0 = chain_ld<V>(p.z0 + zi), G = chain_ld<V>(p.G + zi);
            const ChainVec<V> qm = chain_ld<V>(p.up + b * pu + nh + e), rm = chain_ld<V>(p.down + b * pd + 2 * nh + e);
#pragma unroll
            for (int k = 0; k < V; ++k) o.v[k] = dz0.v[k] * (z0.v[k] - (qm.v[k] + rm.v[k])) - G.v[k];
        } else {
            const size_t ci = b * nh + (r - nh - 2 * nz);
            o = chain_ld<V>(p.dctx1 + ci);
            if (p.dctx2) {
                const ChainVec<V> c = chain_ld<V>(p.dctx2 + ci);
#pragma unroll
                for (int k = 0; k < V; ++k) o.v[k] += c.v[k];
            }
        }
        chain_st<V>(p.o_duc1 + i, o);
        chain_st<V>(p.o_ddc1 + b * pd + 2 * nh + (r - nh), o);          // the q and the r channels get the same gradient
    }
}

template <int V> __global__ __launch_bounds__(256) void iaf_diag_prior_sample_kernel(MadeP p) {
    const size_t nh = (size_t)p.n_h * p.HW, nz = (size_t)p.n_z * p.HW, per = nh + nz, pd = (size_t)p.n_down * p.HW;
    const size_t units = (size_t)p.B * per / V;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < units; t += (size_t)gridDim.x * blockDim.x) {
        const size_t i = t * V, b = i / per, r = i - b * per;
        const float* D = p.down + b * pd;
        if (r < nh) { chain_st<V>(p.o_h + i, chain_ld<V>(D + r)); continue; }                // h_det passes through
        const size_t e = r - nh;
        const ChainVec<V> pm = chain_ld<V>(D + nh + e), pl = chain_ld<V>(D + nh + nz + e), ep = chain_ld<V>(p.eps + b * nz + e);
        ChainVec<V> o;
#pragma unroll
        for (int k = 0; k < V; ++k) o.v[k] = pm.v[k] + ep.v[k] * expf(pl.v[k]);
        chain_st<V>(p.o_h + i, o);
    }
}

// the pieces of the streaming log-sum-exp that iaf_eval_tail_kernel (below) shares with the three kernels here: the running sum
// rescaled to the new maximum plus a chunk's sum, and the bound the state stands for after k weights (distributions.py:62)
__device__ __forceinline__ float iaf_lb_rescaled_sum(float old_m, float old_s, float new_m, float s) {
    return (old_m == -INFINITY ? 0.f : old_s * expf(old_m - new_m)) + s;
}
__device__ __forceinline__ float iaf_lb_bound(float run_max, float run_sum, int k) {
    return -(-logf((float)k) + run_max + logf(run_sum));
}

// streaming logsumexp over k importance weights per image: one wave per image
__global__ __launch_bounds__(256) void iaf_lb_update_kernel(float* run_max, float* run_sum, const float* log_pxz,
                                                           const float* sum_kl, int n, int kc) {
    const int img = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (img >= n) return;
    const float* a = log_pxz + (size_t)img * kc;
    const float* b = sum_kl + (size_t)img * kc;
    float m = -INFINITY;
    for (int i = lane; i < kc; i += 64) m = fmaxf(m, a[i] - b[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    const float old_m = run_max[img];
    const float new_m = fmaxf(old_m, m);
    float s = 0.f;
    for (int i = lane; i < kc; i += 64) s += expf((a[i] - b[i]) - new_m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
        const float old_s = run_sum[img];
        run_sum[img] = iaf_lb_rescaled_sum(old_m, old_s, new_m, s);
        run_max[img] = new_m;
    }
}
__global__ void iaf_lb_init_kernel(float* run_max, float* run_sum, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { run_max[i] = -INFINITY; run_sum[i] = 0.f; }
}
__global__ void iaf_lb_finalize_kernel(const float* run_max, const float* run_sum, float* out, int n, int k) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = iaf_lb_bound(run_max[i], run_sum[i], k);   // distributions.py:62
}
__global__ void iaf_lb_k1_kernel(const float* log_pxz, const float* sum_kl, float* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sum_kl[i] - log_pxz[i];                                 // distributions.py:57
}

// ---------------------------------------------------------------------------------------------
// data-dependent init, tf_utils/layers.py:45-51: per-channel moments of x_init = conv(x, l2norm(mask*V)) over (N,H,W),
//   scale = init_scale / sqrt(var + 1e-10);  g = log(scale)/3;  b = -mean*scale;  y = scale*(x_init - mean)
// One workgroup per channel; two passes (mean, then centred variance) in a fixed tree order.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void iaf_datainit_kernel(const float* x, const float* __restrict__ add, float* y,
                                                          float* __restrict__ g, float* __restrict__ b, int B, int C, int HW,
                                                          float init_scale) {
    __shared__ float red[4];
    const int c = blockIdx.x;
    const int n = B * HW;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { const int bb = i / HW; s += x[((size_t)bb * C + c) * HW + (i - bb * HW)]; }
    const float mean = block_sum_256(s, red) / (float)n;
    float q = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int bb = i / HW;
        const float d = x[((size_t)bb * C + c) * HW + (i - bb * HW)] - mean;
        q += d * d;
    }
    const float var = block_sum_256(q, red) / (float)n;          // tf.nn.moments: biased
    const float scale = init_scale / sqrtf(var + 1e-10f);
    if (threadIdx.x == 0) { g[c] = logf(scale) / 3.0f; b[c] = -mean * scale; }
    if (y)
        for (int i = threadIdx.x; i < n; i += 256) {
            const int bb = i / HW;
            const size_t o = ((size_t)bb * C + c) * HW + (i - bb * HW);
            y[o] = scale * (x[o] - mean) + (add ? add[o] : 0.f);
        }
}

// discretized logistic log-likelihood, tf_utils/distributions.py:28-32 (call site tf_train.py:210): one workgroup per
// batch row, out[b] = sum log(sigmoid(s + binsize/scale) - sigmoid(s) + 1e-7), s = (floor(x/binsize)*binsize - mean)/scale
// (the row sum is a helper of its own: iaf_eval_tail_kernel below takes log_pxz from it too, bit for bit)
__device__ __forceinline__ float iaf_disc_logistic_row(const float* __restrict__ mean, const float* __restrict__ logscale,
                                                       int scalar_scale, const float* __restrict__ sample, size_t base, size_t n,
                                                       float binsize, float* red) {
    float acc = 0.f;
    for (size_t i = threadIdx.x; i < n; i += 256) {
        const float scale = expf(scalar_scale ? logscale[0] : logscale[base + i]);
        const float s = (floorf(sample[base + i] / binsize) * binsize - mean[base + i]) / scale;
        // sigmoid(s+d) - sigmoid(s), evaluated on the side where both terms are small (sigmoid(t) = 1 - sigmoid(-t)):
        // the literal fp32 form cancels to ~1e-7 absolute in the upper tail, the size of the +1e-7 floor itself
        const float d = binsize / scale;
        float diff;
        if (s > 0.f) {
            const float e0 = expf(-s), e1 = expf(-(s + d));
            diff = e0 / (1.0f + e0) - e1 / (1.0f + e1);
        } else {
            diff = 1.0f / (1.0f + expf(-(s + d))) - 1.0f / (1.0f + expf(-s));
        }
        acc += logf(diff + 1e-7f);
    }
    return block_sum_256(acc, red);
}
__global__ __launch_bounds__(256) void iaf_disc_logistic_kernel(const float* __restrict__ mean, const float* __restrict__ logscale,
                                                               int scalar_scale, const float* __restrict__ sample,
                                                               float* __restrict__ out, size_t n, float binsize) {
    __shared__ float red[4];
    const float tot = iaf_disc_logistic_row(mean, logscale, scalar_scale, sample, (size_t)blockIdx.x * n, n, binsize, red);
    if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// out[j] of iaf_colsum_kernel (below): ((0 + mat[0][j]) + mat[1][j]) + ..., row order
__device__ __forceinline__ float iaf_col_sum(const float* __restrict__ mat, int m, int n, int j) {
    float s = 0.f;
    for (int i = 0; i < m; ++i) s += mat[(size_t)i * n + j];
    return s;
}

// ---------------------------------------------------------------------------------------------
// The tail of one evaluation pass (tf_train.py:210, 198-200, 218 and run_eval's accumulation, :313-325) as ONE launch: what
// iaf_disc_logistic_kernel, iaf_colsum_kernel, iaf_lb_update_kernel (kc = 1), iaf_lb_finalize_kernel and a sum over the batch do,
// with the same helpers in the same order -- one workgroup per batch row.  The record counts the passes of the current batch, so a
// replayed graph needs no host to say which pass closes the batch; the last workgroup to arrive (an agent-scope counter, as in
// iaf_guard_sumsq_scan_kernel, iaf_kernels_train.hpp) adds the closed batch to the epoch's sums and moves the pass counter.  Only thread 0 of a
// workgroup reads the counter, before it arrives: the last workgroup's write cannot race a read of the same launch.
// ---------------------------------------------------------------------------------------------
struct EvalRec { double loss_sum; unsigned long long images, nonfinite; unsigned pass, arrivals; };
__global__ __launch_bounds__(256) void iaf_eval_tail_kernel(const float* __restrict__ x_out, const float* __restrict__ dec_log_stdv,
                                                           const float* __restrict__ x, size_t n_per_row, float binsize,
                                                           const float* __restrict__ layer_cost, int n_layers, int n, float* run_max,
                                                           float* run_sum, int k, const long long* __restrict__ indices,
                                                           float* per_image, float* bound, EvalRec* rec) {
    __shared__ float red[4];
    __shared__ double red64[4];
    __shared__ unsigned s_pass, s_last;
    const int b = blockIdx.x;
    unsigned p = 0u;
    float kl = 0.f;
    if (threadIdx.x == 0) {
        p = __hip_atomic_load(&rec->pass, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_pass = p;
        kl = iaf_col_sum(layer_cost, n_layers, n, b);
    }
    const float log_pxz = iaf_disc_logistic_row(x_out, dec_log_stdv, 1, x, (size_t)b * n_per_row, n_per_row, binsize, red);
    if (threadIdx.x == 0) {
        const bool closing = p + 1u >= (unsigned)k;
        const float w = log_pxz - kl;
        const float old_m = run_max[b], old_s = run_sum[b];
        const float new_m = fmaxf(old_m, fmaxf(-INFINITY, w));                        // iaf_lb_update_kernel, one weight
        float s = 0.f;
        s += expf(w - new_m);
        float rs = iaf_lb_rescaled_sum(old_m, old_s, new_m, s), rm = new_m;
        if (closing) {
            const float bd = iaf_lb_bound(rm, rs, k);
            // (agent scope: the workgroup that sums the bounds may sit on another XCD)
            __hip_atomic_store((unsigned*)bound + b, __float_as_uint(bd), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (per_image) per_image[indices[b]] = bd;
            rm = -INFINITY; rs = 0.f;                                                  // armed for the next batch
        }
        run_max[b] = rm;
        run_sum[b] = rs;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                               // the bound is in memory before this workgroup arrives
        s_last = __hip_atomic_fetch_add(&rec->arrivals, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    const unsigned pass = s_pass;
    const bool closing = pass + 1u >= (unsigned)k;
    if (closing) {
        // fixed order: thread t adds rows t, t + 256, ... in index order, then the shuffle / LDS tree; no float atomics
        double sum = 0.0, bad = 0.0;
        for (int i = threadIdx.x; i < n; i += 256) {
            const float v = __uint_as_float(__hip_atomic_load((unsigned*)bound + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            sum += (double)v;
            bad += iaf_nonfinite(v) ? 1.0 : 0.0;                                       // (a count below 2^53: exact)
        }
        sum = iaf_block_sum_f64(sum, red64);
        bad = iaf_block_sum_f64(bad, red64);
        if (threadIdx.x == 0) {
            rec->loss_sum += sum;
            rec->images += (unsigned long long)n;
            rec->nonfinite += (unsigned long long)bad;
        }
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&rec->pass, closing ? 0u : pass + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&rec->arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// zeroes the record and arms the streaming state of n rows
__global__ __launch_bounds__(256) void iaf_eval_reset_kernel(EvalRec* rec, float* run_max, float* run_sum, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { run_max[i] = -INFINITY; run_sum[i] = 0.f; }
    if (i == 0) { rec->loss_sum = 0.0; rec->images = 0ull; rec->nonfinite = 0ull; rec->pass = 0u; rec->arrivals = 0u; }
}

// eps' with (qm+rm) + exp(ql+rl) * eps' == z: the posterior noise that reproduces a given sample z (mode "init" of
// IAFLayer.down runs the posterior block on a PRIOR sample, tf_train.py:60-61,67-85)
__global__ __launch_bounds__(256) void iaf_noise_from_sample_kernel(const float* __restrict__ z, const float* __restrict__ qm,
                                                                   const float* __restrict__ ql, const float* __restrict__ rm,
                                                                   const float* __restrict__ rl, float* __restrict__ eps, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        eps[i] = (z[i] - (qm[i] + rm[i])) * __expf(-(ql[i] + rl[i]));
}

// kl = logq0 + logdet - logp (iaf_kl_combine)
__global__ __launch_bounds__(256) void iaf_kl_combine_kernel(const float* __restrict__ logq0, const float* __restrict__ logdet,
                                                            const float* __restrict__ logp, float* __restrict__ kl, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) kl[i] = (logq0[i] + logdet[i]) - logp[i];
}

// out[j] = sum_i mat[i][j] (iaf_colsum)
__global__ __launch_bounds__(256) void iaf_colsum_kernel(const float* __restrict__ mat, float* __restrict__ out, int m, int n) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    out[j] = iaf_col_sum(mat, m, n, j);            // (shared with iaf_eval_tail_kernel)
}

// ---- 2x resampling of an NCHW tensor (iaf_resample2; the downsampling IAFLayer, tf_train.py:33,42-43, 89-91) ----------------------
// The modes (IAF_RESAMPLE_* of include/iaf_hip.h):
//   DOWN_EVEN     dst[i,j] = src[2i, 2j]       == resize_nearest_neighbor(x, 0.5) (layers.py:169-175)
//   DOWN_ODD      dst[i,j] = src[2i+1, 2j+1]   the outputs a stride-2 SAME 3x3 conv keeps
//   UP_NEAREST    dst[y,x] = src[y/2, x/2]     == resize_nearest_neighbor(x, 2)
//   UP_ZERO_ODD   dst[2i+1,2j+1] = src[i,j], 0 elsewhere: the zero-inserted input of conv2d_transpose
// ... and the adjoints the backward pass needs (UP_ZERO_ODD is DOWN_ODD's, and the other way round):
//   UP_ZERO_EVEN  dst[2i,2j] = src[i,j], 0 elsewhere: adjoint of DOWN_EVEN
//   DOWN_SUM4     dst[i,j] = sum of src[2i..2i+1, 2j..2j+1]: adjoint of UP_NEAREST

// H, W: size of the SMALLER of the two tensors
__global__ __launch_bounds__(256) void iaf_resample2_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t n_dst,
                                                           int H, int W, int mode) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_dst; i += stride) {
        if (mode == IAF_RESAMPLE_DOWN_EVEN || mode == IAF_RESAMPLE_DOWN_ODD || mode == IAF_RESAMPLE_DOWN_SUM4) {
            const int x = (int)(i % W), y = (int)((i / W) % H);
            const size_t plane = i / ((size_t)W * H);
            const int o = (mode == IAF_RESAMPLE_DOWN_ODD) ? 1 : 0;
            const float* q = src + (plane * 2 * H + 2 * y + o) * 2 * W + 2 * x + o;
            dst[i] = (mode == IAF_RESAMPLE_DOWN_SUM4) ? (q[0] + q[1]) + (q[2 * W] + q[2 * W + 1]) : q[0];
        } else {
            const int W2 = 2 * W, H2 = 2 * H;
            const int x = (int)(i % W2), y = (int)((i / W2) % H2);
            const size_t plane = i / ((size_t)W2 * H2);
            const float v = src[(plane * H + (y >> 1)) * W + (x >> 1)];
            const bool keep = mode == IAF_RESAMPLE_UP_NEAREST || (mode == IAF_RESAMPLE_UP_ZERO_ODD && (y & 1) && (x & 1)) ||
                              (mode == IAF_RESAMPLE_UP_ZERO_EVEN && !(y & 1) && !(x & 1));
            dst[i] = keep ? v : 0.f;
        }
    }
}
