// iaf_kernels_misc.hpp -- the small kernels the stack's own entry points launch: KL / free-bits reductions, max-diff, the control kernels of the inverse step.
// Included by iaf_engine.hip and by no other unit (the objective-side kernels: iaf_kernels_objective.hpp, in iaf_model_ops.hip).
#pragma once

// ---------------------------------------------------------------------------------------------
// KL / free-bits reduction, tf_train.py:77-85.  kl_elem [B,Z,H,W] -> kl_cost[B], kl_obj[B].
// One workgroup: deterministic tree order.  S[b,c] = sum_{H,W} kl.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void iaf_kl_rowsum_kernel(const float* kl, float* S, int rows, int HW) {
    // one wave per (b,c) row
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float a = 0.f;
    for (int i = lane; i < HW; i += 64) a += kl[(size_t)row * HW + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
    if (lane == 0) S[row] = a;
}

// gate (optional, [Z]): 1 where the free-bits max() passes the gradient (mean_b S[b,c] > kl_min), else 0 -- what the
// backward of tf_train.py:79-80 needs; written here because the batch mean is already on hand.
// nrb > 0: S holds per-row-block partial sums [B][nrb][Z] (the one-launch step's StepP::kl_part) and the sum over the row
// blocks -- in row order, eight loads in flight -- is the first thing this launch does; nrb = 0: S is [B][Z].
// scratch ([B*Z] floats) is only touched when B*Z does not fit the LDS staging.
// groups (1 .. 64, B % groups == 0): the free-bits mean is taken per contiguous run of G = B / groups rows (one tower of the
// reference's multi-tower step each, tf_train.py:126) -- a group's numbers are what a stand-alone G-row batch gives, its rows
// summed in row order, so groups = 1 is the one-batch arithmetic bit for bit; gate is then [groups][Z].
__global__ __launch_bounds__(256) void iaf_kl_finish_kernel(const float* S, float* kl_obj, float* kl_cost, int B, int Z,
                                                           float kl_min, float* gate, int nrb, float* scratch, int groups) {
    // S is tiny ([B, Z]); stage it through LDS in one coalesced sweep instead of B*Z dependent global loads
    __shared__ float sh[8192];
    __shared__ float part[256];
    __shared__ float s_fb[64];
    const int tid = threadIdx.x, n = B * Z, G = B / groups;
    const bool in_lds = n <= 8192;
    if (nrb > 0) {
        // item = four consecutive channels of one image: its nrb partial sums are nrb independent 16-byte loads, eight in
        // flight per round (the whole table in ONE round trip at B = 32, 16x16: 256 items x 8 row blocks)
        float* dst = in_lds ? sh : scratch;
        typedef float kf4 __attribute__((ext_vector_type(4)));
        if ((Z & 3) == 0) {
            const int Z4 = Z >> 2;
            for (int i = tid; i < B * Z4; i += 256) {
                const int b = i / Z4, c4 = i - b * Z4;
                kf4 a = kf4{0.f, 0.f, 0.f, 0.f};
                for (int r0 = 0; r0 < nrb; r0 += 8) {
                    kf4 v8[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int r = r0 + k < nrb ? r0 + k : nrb - 1;
                        v8[k] = *(const kf4*)(S + ((size_t)b * nrb + r) * Z + 4 * c4);
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (r0 + k < nrb) a += v8[k];
                }
                *(kf4*)(dst + (size_t)b * Z + 4 * c4) = a;
            }
        } else {
            for (int i = tid; i < n; i += 256) {
                const int b = i / Z, c = i - b * Z;
                float a = 0.f;
                for (int r = 0; r < nrb; ++r) a += S[((size_t)b * nrb + r) * Z + c];
                dst[i] = a;
            }
        }
        __syncthreads();
    } else if (in_lds) {
        for (int i = tid; i < n; i += 256) sh[i] = S[i];
        __syncthreads();
    }
    const float* src = in_lds ? sh : (nrb > 0 ? scratch : S);
    if (kl_min > 0.f) {
        // kl_ave[c] = max(mean_b S[b,c], kl_min); kl_obj[b] = sum_c kl_ave[c]   (tf_train.py:79-82)
        for (int r = 0; r < groups; ++r) {
            const float* sg = src + (size_t)r * G * Z;
            float a = 0.f;
            for (int c = tid; c < Z; c += 256) {
                float m = 0.f;
                for (int b = 0; b < G; ++b) m += sg[(size_t)b * Z + c];
                a += fmaxf(m / (float)G, kl_min);
                if (gate) gate[(size_t)r * Z + c] = (m / (float)G > kl_min) ? 1.f : 0.f;
            }
            part[tid] = a;
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) {
                if (tid < o) part[tid] += part[tid + o];
                __syncthreads();
            }
            if (tid == 0) s_fb[r] = part[0];
            __syncthreads();
        }
    }
    for (int b = tid; b < B; b += 256) {
        float a = 0.f;
        for (int c = 0; c < Z; ++c) a += src[(size_t)b * Z + c];
        kl_cost[b] = a;                                        // tf_train.py:85
        kl_obj[b] = (kl_min > 0.f) ? s_fb[b / G] : a;          // tf_train.py:82 / 84
    }
}

// S[b][c] = sum over the row blocks of the partial sums [B][nrb][Z], in row order: the first phase of the kernel above as
// its own many-workgroup launch, for batches whose partial sums are too many for ONE workgroup to walk (config 5: B = 256)
__global__ __launch_bounds__(256) void iaf_kl_partsum_kernel(const float* part, float* S, int n, int Z, int nrb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = i / Z, c = i - b * Z;
    float a = 0.f;
    for (int r0 = 0; r0 < nrb; r0 += 8) {
        float v8[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int r = r0 + k < nrb ? r0 + k : nrb - 1;
            v8[k] = part[((size_t)b * nrb + r) * Z + c];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) a += (r0 + k < nrb) ? v8[k] : 0.f;
    }
    S[i] = a;
}

// max |a - b| over n elements -> *out (float bits; non-negative floats order like unsigned ints).  NaN counts as +inf.
__global__ __launch_bounds__(256) void iaf_maxdiff_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n,
                                                         unsigned* out) {
    float m = 0.f;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float d = fabsf(a[i] - b[i]);
        m = (d > m || d != d) ? (d != d ? __builtin_inff() : d) : m;
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));
}

// ---- iaf_step_inverse without the host in its loop (round 6) -------------------------------------------------------------------
// The inverse of the IAF step -- z0 with z = (z0 - m(z0)) / exp(s(z0)) (tf_train.py:69-72 read backwards; the reference never inverts:
// it only evaluates densities of its own samples, tf_train.py:60-66, models.py:330-359) -- as JACOBI sweeps z0 <- z exp(s(z0)) + m(z0)
// on the forward kernels.  Why not the anti-diagonal wavefront north_star names: m, s at (pixel p, channel c) depend on z0 at the pixels
// right of / below p and on the lower channels at p (the MADE order), a DAG of depth H W n_z -- a true scan is H W n_z dependent steps of
// one channel of one pixel each (8192 launches-worth of latency at 16x16), while a Jacobi sweep is one full-rate forward launch that moves
// EVERY element one step down the DAG at once: exact after at most H W n_z sweeps (the DAG's depth), and -- the 0.1 on m and s makes the
// map a contraction in practice -- at fp32 resolution after ~8.  The control words live in device memory:
struct InvCtl { unsigned res_bits, done, sweeps, arrivals; float last_res; unsigned pad[3]; };
// max |a - b| of one sweep pair; the LAST workgroup to arrive compares it with tol, records (sweeps so far, residual), raises `done` (which the
// queued sweep launches read: StepP::skip) and re-arms the two scratch words.  Does nothing once done.  NaN counts as +inf (never converged).
__global__ __launch_bounds__(256) void iaf_inverse_check_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, InvCtl* c,
                                                               float tol, unsigned sweeps_so_far) {
    if (*(volatile unsigned*)&c->done) return;
    float m = 0.f;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float d = fabsf(a[i] - b[i]);
        m = (d > m || d != d) ? (d != d ? __builtin_inff() : d) : m;
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o, 64));
    __shared__ float wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
        __hip_atomic_fetch_max(&c->res_bits, __float_as_uint(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_fetch_add(&c->arrivals, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u) {
            const float res = __uint_as_float(__hip_atomic_load(&c->res_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            c->last_res = res;
            c->sweeps = sweeps_so_far;
            c->res_bits = 0u; c->arrivals = 0u;
            if (res <= tol) __hip_atomic_store(&c->done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
// the result into z0: where the sweep launches return early once converged (skipping), the converged estimate sits in the buffer sweep
// number c->sweeps wrote, buf[(max_sweeps - sweeps) & 1] with buf[0] = z0; otherwise the last sweep has written z0 itself.  Also the two
// numbers the caller may ask for: out[0] = sweeps run (as an int), out[1] = the last residual (as a float; -1: never checked)
__global__ __launch_bounds__(256) void iaf_inverse_finish_kernel(const float* __restrict__ other, float* __restrict__ z0, size_t n, const InvCtl* c,
                                                                int max_sweeps, int skipping, int checked, unsigned* out) {
    const unsigned done = c->done, sw = c->sweeps;
    if (blockIdx.x == 0 && threadIdx.x == 0 && out) {
        out[0] = done ? sw : (unsigned)max_sweeps;
        out[1] = __float_as_uint(checked ? c->last_res : -1.f);
    }
    if (!(skipping && done && ((max_sweeps - (int)sw) & 1))) return;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) z0[i] = other[i];
}
