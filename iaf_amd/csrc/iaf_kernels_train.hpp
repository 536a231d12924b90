// iaf_kernels_train.hpp -- the kernels of the training loop's services that touch no stack and no conv: Adamax + EMA (plain and behind the
// guard), the guard scans of a step's gradient, the step's summaries.  Included by iaf_train_services.hip alone.
#pragma once
#include "iaf_common.hpp"
#include "iaf_conv_kernel.hpp"   // f32x4

// Adamax (tf_utils/adamax.py:40-56; NB the reference's slot naming: "v" = first moment, "m" = infinity norm) fused
// with the 1/N gradient averaging of average_grads (tf_utils/common.py:86) and the EMA of the parameters
// (tf_train.py:157-158, decay 0.999).  One pass over flat fp32 buffers: 5 reads + 4 writes per element, HBM-bound.
__global__ __launch_bounds__(256) void iaf_adamax_ema_kernel(float* __restrict__ var, const float* __restrict__ grad,
                                                            float* __restrict__ slot_m, float* __restrict__ slot_v,
                                                            float* __restrict__ ema, size_t n4, size_t n, float lr, float beta1,
                                                            float beta2, float eps, float ema_decay, float grad_scale) {
    auto upd = [&](float& w, float g, float& m, float& v, float& e) {
        g *= grad_scale;
        v = beta1 * v + (1.f - beta1) * g;                    // adamax.py:50
        m = fmaxf(beta2 * m + eps, fabsf(g));                 // adamax.py:52
        w -= lr * (v / m);                                    // adamax.py:53-55
        e -= (1.f - ema_decay) * (e - w);                     // ExponentialMovingAverage.apply
    };
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 w = ((f32x4*)var)[i], g = ((const f32x4*)grad)[i], m = ((f32x4*)slot_m)[i], v = ((f32x4*)slot_v)[i];
        f32x4 e = ema ? ((f32x4*)ema)[i] : w;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float wr_ = w[r], mr = m[r], vr = v[r], er = e[r];
            upd(wr_, g[r], mr, vr, er);
            w[r] = wr_; m[r] = mr; v[r] = vr; e[r] = er;
        }
        ((f32x4*)var)[i] = w; ((f32x4*)slot_m)[i] = m; ((f32x4*)slot_v)[i] = v;
        if (ema) ((f32x4*)ema)[i] = e;
    }
    for (size_t i = 4 * n4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {   // tail
        float e = ema ? ema[i] : var[i];
        upd(var[i], grad[i], slot_m[i], slot_v[i], e);
        if (ema) ema[i] = e;
    }
}

// The guard of a training step: guard[0] = 1 if NaN or +-inf is anywhere in the (all-reduced) flat gradient or in `extra` (the
// step's objective), else 0.  One HBM-bound read of the buffer; non-finite = exponent field all ones, tested on the bits so that
// no fast-math setting can fold it away.  Per workgroup one combine (the waves' ballots) and ONE device-scope atomic on guard[1]:
// the low 16 bits count the workgroups that have arrived, the high bits the ones that saw a non-finite value.  The last workgroup
// to arrive writes the verdict to guard[0] and puts guard[1] back to 0 -- every scan writes its own verdict and leaves the word
// as it found it, so nothing has to clear the guard between calls or graph replays (grids <= 2048 workgroups: ew_grid).
__global__ __launch_bounds__(256) void iaf_nonfinite_scan_kernel(const float* __restrict__ buf, size_t n4, size_t n,
                                                                const float* __restrict__ extra, int n_extra, unsigned* guard) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    bool bad = false;
    for (size_t i = t; i < n4; i += stride) {
        const f32x4 v = ((const f32x4*)buf)[i];
        bad |= iaf_nonfinite(v[0]) | iaf_nonfinite(v[1]) | iaf_nonfinite(v[2]) | iaf_nonfinite(v[3]);
    }
    for (size_t i = 4 * n4 + t; i < n; i += stride) bad |= iaf_nonfinite(buf[i]);      // tail
    if (t < (size_t)n_extra) bad |= iaf_nonfinite(extra[t]);
    bad = __syncthreads_or(bad) != 0;                                                    // the workgroup's verdict
    if (threadIdx.x == 0) {
        const unsigned mine = 1u + (bad ? 0x10000u : 0u);
        const unsigned total = __hip_atomic_fetch_add(guard + 1, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + mine;
        if ((total & 0xffffu) == gridDim.x) {                                               // the last workgroup
            __hip_atomic_store(guard, (total >> 16) ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(guard + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The same scan fused with sum(buf[i]^2) in fp64 (the square of the step's gradient norm): still ONE read of the buffer.  The verdict
// and the arrival word are the scan's above, bit for bit.  Every lane squares and accumulates in fp64 (the square of an fp32 value is
// exact there: only the additions round, and 1e25^2 is far inside the range) on four independent chains combined in a fixed order;
// the workgroup's lanes are combined by fixed-order shuffles and one LDS round, and lane 0 stores the workgroup's partial into ITS
// slot of `partials` ([gridDim.x] <= 2048) -- an agent-scope store, drained (vmcnt(0)) before the arrival add, because the reader
// sits on another XCD.  The last workgroup to arrive reads the slots with agent-scope loads and adds them in a fixed order (lane t
// slots 8t .. 8t+7 in index order, then the same shuffle / LDS tree): no float atomics anywhere, so sumsq is the same bits on every
// run and every replay of a captured graph for a given n and alignment of buf.
__global__ __launch_bounds__(256) void iaf_guard_sumsq_scan_kernel(const float* __restrict__ buf, size_t n4, size_t n,
                                                                      const float* __restrict__ extra, int n_extra, unsigned* guard,
                                                                      double* partials, double* sumsq) {
    __shared__ double red[4];
    __shared__ unsigned last;
    const size_t stride = (size_t)gridDim.x * blockDim.x, t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    bool bad = false;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (size_t i = t; i < n4; i += stride) {
        const f32x4 v = ((const f32x4*)buf)[i];
        bad |= iaf_nonfinite(v[0]) | iaf_nonfinite(v[1]) | iaf_nonfinite(v[2]) | iaf_nonfinite(v[3]);
        a0 = fma((double)v[0], (double)v[0], a0);
        a1 = fma((double)v[1], (double)v[1], a1);
        a2 = fma((double)v[2], (double)v[2], a2);
        a3 = fma((double)v[3], (double)v[3], a3);
    }
    for (size_t i = 4 * n4 + t; i < n; i += stride) {                                     // tail
        const float v = buf[i];
        bad |= iaf_nonfinite(v);
        a0 = fma((double)v, (double)v, a0);
    }
    if (t < (size_t)n_extra) bad |= iaf_nonfinite(extra[t]);
    bad = __syncthreads_or(bad) != 0;                                                    // the workgroup's verdict
    const double part = iaf_block_sum_f64((a0 + a1) + (a2 + a3), red);
    if (threadIdx.x == 0) {
        __hip_atomic_store((unsigned long long*)partials + blockIdx.x, (unsigned long long)__double_as_longlong(part), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                  // the partial is in memory before this workgroup arrives
        const unsigned mine = 1u + (bad ? 0x10000u : 0u);
        const unsigned total = __hip_atomic_fetch_add(guard + 1, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + mine;
        const bool is_last = (total & 0xffffu) == gridDim.x;
        if (is_last) {
            __hip_atomic_store(guard, (total >> 16) ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(guard + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        last = is_last ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;
    unsigned long long raw[8];                                                            // eight loads in flight, then the adds in index order
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned slot = threadIdx.x * 8u + k;
        raw[k] = __hip_atomic_load((unsigned long long*)partials + (slot < gridDim.x ? slot : gridDim.x - 1u), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (threadIdx.x * 8u + k < gridDim.x) s += __longlong_as_double((long long)raw[k]);
    s = iaf_block_sum_f64(s, red);
    if (threadIdx.x == 0) *sumsq = s;
}

// The summaries of one training step into a device record (tf_train.py:142, 148-149, 203-204, 214-216): one workgroup, one wave per
// reduced row (the 2 nl rows of layer_obj / layer_cost [nl][n], top-down as the model stacks them, then log_pxz [n]), lanes stride
// over the n batch rows, fp64 sums combined by fixed-order shuffles.  rec: double acc[F], double last[F], then two 64-bit counts
// (accumulated steps, skipped steps), F = 6 + 2 nl:
//   [0] loss_all (the all-reduced loss word)   [1] dec_log_stdv   [2] -mean(log_pxz)   [3] mean(kl_obj) = sum_l mean_b layer_obj[l]
//   [4] mean(kl_cost)   [5] grad_scale sqrt(sumsq)   [6 + 2l] mean_b layer_obj[l]   [7 + 2l] mean_b layer_cost[l]
// `last` is always written; guard[0] == 0: acc += fields and steps += 1; guard[0] != 0: acc is not touched and skipped += 1.
#define IAF_SUMMARY_MAX_LAYERS 256
__global__ __launch_bounds__(256) void iaf_train_summaries_kernel(const float* __restrict__ layer_obj, const float* __restrict__ layer_cost,
                                                                 const float* __restrict__ log_pxz, const float* __restrict__ dec_log_stdv,
                                                                 const float* __restrict__ loss_all, const double* __restrict__ sumsq,
                                                                 float grad_scale, const unsigned* guard, double* rec, int nl, int n) {
    __shared__ double rows[2 * IAF_SUMMARY_MAX_LAYERS + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nrows = 2 * nl + 1, F = 6 + 2 * nl;
    for (int r = wave; r < nrows; r += 4) {
        const float* src = r < nl ? layer_obj + (size_t)r * n : (r < 2 * nl ? layer_cost + (size_t)(r - nl) * n : log_pxz);
        double a = 0.0;
        for (int i = lane; i < n; i += 64) a += (double)src[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
        if (lane == 0) rows[r] = a / (double)n;
    }
    __syncthreads();
    const bool skip = __hip_atomic_load(guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
    for (int f = threadIdx.x; f < F; f += 256) {
        double v;
        if (f == 0) v = (double)loss_all[0];
        else if (f == 1) v = (double)dec_log_stdv[0];
        else if (f == 2) v = -rows[2 * nl];
        else if (f == 3 || f == 4) {
            v = 0.0;
            for (int l = 0; l < nl; ++l) v += rows[(f == 3 ? 0 : nl) + l];
        } else if (f == 5) v = (double)grad_scale * sqrt(sumsq[0]);
        else v = rows[((f - 6) & 1) * nl + ((f - 6) >> 1)];
        rec[F + f] = v;
        if (!skip) rec[f] += v;
    }
    if (threadIdx.x == 0) {
        unsigned long long* cnt = (unsigned long long*)(rec + 2 * F);
        cnt[skip ? 1 : 0] += 1ull;
    }
}
__global__ void iaf_train_summaries_reset_kernel(unsigned long long* rec, int words) {
    for (int i = threadIdx.x; i < words; i += blockDim.x) rec[i] = 0ull;
}

// iaf_adamax_ema_kernel behind the guard: *guard == 0 -> the same arithmetic, statement for statement (bit-identical results);
// *guard != 0 -> no store to var, the slots or ema, and one lane adds 1 to the skip counter (mapped host memory)
__global__ __launch_bounds__(256) void iaf_adamax_ema_guarded_kernel(float* __restrict__ var, const float* __restrict__ grad,
                                                                    float* __restrict__ slot_m, float* __restrict__ slot_v,
                                                                    float* __restrict__ ema, size_t n4, size_t n, float lr, float beta1,
                                                                    float beta2, float eps, float ema_decay, float grad_scale,
                                                                    const unsigned* guard, unsigned* skips) {
    if (__hip_atomic_load(guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_fetch_add(skips, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    auto upd = [&](float& w, float g, float& m, float& v, float& e) {
        g *= grad_scale;
        v = beta1 * v + (1.f - beta1) * g;                    // adamax.py:50
        m = fmaxf(beta2 * m + eps, fabsf(g));                 // adamax.py:52
        w -= lr * (v / m);                                    // adamax.py:53-55
        e -= (1.f - ema_decay) * (e - w);                     // ExponentialMovingAverage.apply
    };
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 w = ((f32x4*)var)[i], g = ((const f32x4*)grad)[i], m = ((f32x4*)slot_m)[i], v = ((f32x4*)slot_v)[i];
        f32x4 e = ema ? ((f32x4*)ema)[i] : w;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float wr_ = w[r], mr = m[r], vr = v[r], er = e[r];
            upd(wr_, g[r], mr, vr, er);
            w[r] = wr_; m[r] = mr; v[r] = vr; e[r] = er;
        }
        ((f32x4*)var)[i] = w; ((f32x4*)slot_m)[i] = m; ((f32x4*)slot_v)[i] = v;
        if (ema) ((f32x4*)ema)[i] = e;
    }
    for (size_t i = 4 * n4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {   // tail
        float e = ema ? ema[i] : var[i];
        upd(var[i], grad[i], slot_m[i], slot_v[i], e);
        if (ema) ema[i] = e;
    }
}
