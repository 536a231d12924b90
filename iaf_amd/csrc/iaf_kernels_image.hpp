// iaf_kernels_image.hpp -- run_eval's image summaries (tf_train.py:329-376; tf_utils/common.py:118-168, img_stretch / img_tile) on the
// device: the range of a slice (min, max, count of non-finite elements) and the one launch that stretches and tiles up to two NCHW
// sources into an HWC grid.  The C ABI and the arithmetic are stated in include/iaf_hip.h; included by iaf_train_services.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "iaf_common.hpp"

// ---------------------------------------------------------------------------------------------
// The range of src[0..n): 16-byte loads over the aligned body (workgroup w takes pieces w * 256 + t, + G * 256, ...), the scalar head
// (up to src's first 16-byte boundary) and tail on workgroup 0's first lanes; fmin / fmax / count down the wave's 64 lanes by shuffles,
// then one LDS round across the workgroup's four waves.  Non-finite elements are counted and left out of lo / hi; +-0 leaves as +0, so
// that the record does not depend on which of two equal zeros a reduction met first.
//
// One workgroup (G = 1) writes the record with plain stores and touches no counter.  G > 1: `arrivals` holds the workgroups that have
// ENTERED in its low half and, in its high half, one mark for the reset plus one per workgroup that is DONE.  The workgroup that
// enters first (it draws 0) sets lo = +inf, hi = -inf, nonfinite = 0 and then adds the reset's mark with release; it does so before
// it reads a single element.  Every workgroup combines behind that mark -- a 64-bit compare-and-swap on (lo, hi), an add on
// nonfinite; min, max and an integer sum do not depend on the order -- and the one that finds G marks before its own is the last: it
// sets `arrivals` back to 0, so a replayed graph needs no memset.  The wait for the mark is a wait for a workgroup that is resident
// and has nothing to do before it but three stores; it is bounded all the same (IAF_IMG_RANGE_POLLS), so that a record handed in
// with a stale `arrivals` (the header asks for zero before the first call) costs a wrong answer, never a hung queue.
// ---------------------------------------------------------------------------------------------
#define IAF_IMG_RANGE_MAX_BLOCKS 256
#define IAF_IMG_RANGE_SHARE 16384          // bytes of the body per workgroup before another one is added
#define IAF_IMG_RANGE_POLLS 65536
struct ImgRangeRec { float lo, hi; unsigned nonfinite, arrivals; };

__device__ __forceinline__ void iaf_img_take(float v, float& lo, float& hi, unsigned& nf) {
    if (iaf_nonfinite(v)) { ++nf; return; }
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
}
__device__ __forceinline__ void iaf_img_take_word(unsigned w, float& lo, float& hi) {      // four uint8 elements
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float v = (float)((w >> (8 * k)) & 0xffu);
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
}
__device__ __forceinline__ float iaf_img_plus_zero(float v) { return (__float_as_uint(v) & 0x7fffffffu) == 0u ? 0.f : v; }

__global__ __launch_bounds__(256) void iaf_img_range_kernel(const void* __restrict__ src, int dtype, unsigned long long n,
                                                            unsigned head, unsigned long long pieces, ImgRangeRec* rec) {
    __shared__ float s_lo[4], s_hi[4];
    __shared__ unsigned s_nf[4];
    const unsigned t = threadIdx.x, G = gridDim.x;
    if (G > 1 && t == 0) {
        const unsigned entered = __hip_atomic_fetch_add(&rec->arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0xffffu;
        if (entered == 0u) {
            __hip_atomic_store((unsigned*)&rec->lo, __float_as_uint(INFINITY), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store((unsigned*)&rec->hi, __float_as_uint(-INFINITY), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&rec->nonfinite, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                         // the reset is in memory before its mark
            (void)__hip_atomic_fetch_add(&rec->arrivals, 0x10000u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    float lo = INFINITY, hi = -INFINITY;
    unsigned nf = 0u;
    const unsigned long long first = (unsigned long long)blockIdx.x * 256ull + t, stride = (unsigned long long)G * 256ull;
    if (dtype == 0) {
        const unsigned char* p = (const unsigned char*)src;
        const uint4* body = (const uint4*)(p + head);
        for (unsigned long long i = first; i < pieces; i += stride) {
            const uint4 q = body[i];
            iaf_img_take_word(q.x, lo, hi);
            iaf_img_take_word(q.y, lo, hi);
            iaf_img_take_word(q.z, lo, hi);
            iaf_img_take_word(q.w, lo, hi);
        }
        if (blockIdx.x == 0) {
            const unsigned long long done = (unsigned long long)head + pieces * 16ull;
            if (t < head) iaf_img_take((float)p[t], lo, hi, nf);
            if (done + t < n) iaf_img_take((float)p[done + t], lo, hi, nf);       // (fewer than 16 elements are left)
        }
    } else {
        const float* p = (const float*)src;
        const float4* body = (const float4*)(p + head);
        for (unsigned long long i = first; i < pieces; i += stride) {
            const float4 q = body[i];
            iaf_img_take(q.x, lo, hi, nf);
            iaf_img_take(q.y, lo, hi, nf);
            iaf_img_take(q.z, lo, hi, nf);
            iaf_img_take(q.w, lo, hi, nf);
        }
        if (blockIdx.x == 0) {
            const unsigned long long done = (unsigned long long)head + pieces * 4ull;
            if (t < head) iaf_img_take(p[t], lo, hi, nf);
            if (done + t < n) iaf_img_take(p[done + t], lo, hi, nf);              // (fewer than 4 elements are left)
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_down(lo, o, 64));
        hi = fmaxf(hi, __shfl_down(hi, o, 64));
        nf += __shfl_down(nf, o, 64);
    }
    if ((t & 63u) == 0u) { s_lo[t >> 6] = lo; s_hi[t >> 6] = hi; s_nf[t >> 6] = nf; }
    __syncthreads();
    if (t != 0) return;
    lo = iaf_img_plus_zero(fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3])));
    hi = iaf_img_plus_zero(fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3])));
    nf = (s_nf[0] + s_nf[1]) + (s_nf[2] + s_nf[3]);
    if (G == 1) {
        rec->lo = lo; rec->hi = hi; rec->nonfinite = nf; rec->arrivals = 0u;
        return;
    }
    for (int polls = 0; polls < IAF_IMG_RANGE_POLLS; ++polls) {                      // the reset's mark (see above: bounded)
        if (__hip_atomic_load(&rec->arrivals, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >> 16) break;
        __builtin_amdgcn_s_sleep(1);
    }
    unsigned long long* pair = (unsigned long long*)rec;                             // (lo, hi): the record is 8-byte aligned
    unsigned long long seen = __hip_atomic_load(pair, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const float nlo = fminf(__uint_as_float((unsigned)seen), lo), nhi = fmaxf(__uint_as_float((unsigned)(seen >> 32)), hi);
        const unsigned long long want = (unsigned long long)__float_as_uint(nlo) | ((unsigned long long)__float_as_uint(nhi) << 32);
        if (want == seen) break;
        if (__hip_atomic_compare_exchange_strong(pair, &seen, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    }
    if (nf) (void)__hip_atomic_fetch_add(&rec->nonfinite, nf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                 // this workgroup's part is in memory before it is done
    const unsigned marks = __hip_atomic_fetch_add(&rec->arrivals, 0x10000u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) >> 16;
    if (marks == G) __hip_atomic_store(&rec->arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------
// The grid: one thread per pixel of the [Hg, Wg, C] grid (lanes along x: a wave reads a run of every plane's row and writes one run of
// the HWC row), every element written by this launch -- image pixels, borders, empty tiles.  The stretch constants of the (at most
// two) sources are worked out once per workgroup from the records, in the order include/iaf_hip.h states.
// ---------------------------------------------------------------------------------------------
struct ImgGridTable {
    const void* ptr[2];
    const ImgRangeRec* outer[2];
    const ImgRangeRec* inner[2];      // may be null
    int dtype[2];
};

__device__ __forceinline__ unsigned char iaf_img_quantise(float v) {
    const double q = floor((double)v * 255.0 + 0.5);      // (exact in fp64 for an fp32 v: no contraction can change the byte)
    return (unsigned char)(q >= 255.0 ? 255.0 : (q > 0.0 ? q : 0.0));               // (NaN: both tests fail -> 0)
}

__global__ __launch_bounds__(256) void iaf_img_grid_kernel(ImgGridTable T, int n_src, int n_imgs, int C, int H, int W, int border, float border_color,
                                                           int th, int tw, int Hg, int Wg, float* __restrict__ grid_f32,
                                                           unsigned char* __restrict__ grid_u8) {
    __shared__ float s_lo[2], s_d[2], s_a[2], s_di[2];
    __shared__ int s_two[2], s_bad[2];
    if ((int)threadIdx.x < n_src) {
        const int s = threadIdx.x;
        const ImgRangeRec* o = T.outer[s];
        const ImgRangeRec* in = T.inner[s];
        const float lo = o->lo, d = (float)((double)(o->hi - lo) + 1e-12);
        unsigned bad = o->nonfinite;
        float a = 0.f, di = 1.f;
        if (in) {
            a = (in->lo - lo) / d;
            const float b = (in->hi - lo) / d - a;
            di = (float)((double)b + 1e-12);
            bad |= in->nonfinite;
        }
        s_lo[s] = lo; s_d[s] = d; s_a[s] = a; s_di[s] = di; s_two[s] = in != nullptr; s_bad[s] = bad != 0u;
    }
    __syncthreads();
    const long long px = (long long)blockIdx.x * 256 + threadIdx.x;
    if (px >= (long long)Hg * Wg) return;
    const int gy = (int)(px / Wg), gx = (int)(px % Wg);
    const int ty = gy / (H + border), y = gy % (H + border), tx = gx / (W + border), x = gx % (W + border);
    const int slot = ty * tw + tx;
    const bool shown = y < H && x < W && ty < th && slot < n_imgs;
    const int s = shown ? slot % n_src : 0;
    const size_t plane = (size_t)H * W, at = ((size_t)(shown ? slot / n_src : 0) * C) * plane + (size_t)(shown ? y : 0) * W + (shown ? x : 0);
    const float lo = s_lo[s], d = s_d[s], a = s_a[s], di = s_di[s];
    const bool two = s_two[s] != 0, bad = s_bad[s] != 0;
    for (int c = 0; c < C; ++c) {
        float v = border_color;
        if (shown) {
            const size_t i = at + (size_t)c * plane;
            v = T.dtype[s] == 0 ? (float)((const unsigned char*)T.ptr[s])[i] : ((const float*)T.ptr[s])[i];
            v = (v - lo) / d;
            if (two) v = (v - a) / di;
            if (bad) v = __uint_as_float(0x7fc00000u);
        }
        const size_t o = (size_t)px * C + c;
        if (grid_f32) grid_f32[o] = v;
        if (grid_u8) grid_u8[o] = iaf_img_quantise(v);
    }
}
