// Which form of the state snapshot's kernel (csrc/iaf_kernels_data.hpp: iaf_state_snapshot_kernel) runs at copy speed?  Four buffers of the
// BASELINE config-2 size (41557932 words each) copied and digested by: four hipMemcpyAsync (the yardstick); the FIRST form of the kernel
// (every workgroup of 256 lanes walks every part, two loads in flight, one atomic per workgroup and part) with and without its atomics
// and its digest arithmetic, at 2048 and 1024 workgroups; the product kernel at its own budget of workgroups and at twice that.  Device
// events, median of 20 after 5 warm-up launches; the digests are checked against the host's.  Results: profiles/checkpoint/README.md.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "iaf_hip.h"
#include "iaf_kernels_rng.hpp"
#include "iaf_kernels_data.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

struct V1Table { const unsigned* src[8]; unsigned* dst[8]; unsigned long long words[8]; int n; };

__device__ __forceinline__ unsigned long long v1_term(unsigned w, unsigned long long i) {
    const unsigned k = (unsigned)(2ull * i + 1ull) * 0x9E3779B1u;
    return (unsigned long long)w * k + k;
}
__device__ __forceinline__ unsigned long long v1_piece(const data_u4 v, unsigned long long i, unsigned* d) {
    *(data_u4*)(d + i) = v;
    return (v1_term(v.x, i) + v1_term(v.y, i + 1)) + (v1_term(v.z, i + 2) + v1_term(v.w, i + 3));
}
// all workgroups walk all parts (aligned parts, words % 4 == 0 only); ATOM: the atomic per workgroup and part; DIG: the digest arithmetic
template <int ATOM, int DIG>
__global__ __launch_bounds__(256) void v1_kernel(const V1Table T, unsigned long long* __restrict__ digests) {
    __shared__ unsigned long long red[4];
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull, t = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    for (int p = 0; p < T.n; ++p) {
        const unsigned* const s = T.src[p];
        unsigned* const d = T.dst[p];
        const unsigned long long n4 = T.words[p] >> 2;
        const data_u4* const sv = (const data_u4*)s;
        unsigned long long acc = 0;
        unsigned long long j = t;
        for (; j + stride < n4; j += 2ull * stride) {
            const data_u4 v0 = sv[j], v1 = sv[j + stride];
            if (DIG) { acc += v1_piece(v0, 4ull * j, d); acc += v1_piece(v1, 4ull * (j + stride), d); }
            else { *(data_u4*)(d + 4ull * j) = v0; *(data_u4*)(d + 4ull * (j + stride)) = v1; }
        }
        if (j < n4) { const data_u4 v0 = sv[j]; if (DIG) acc += v1_piece(v0, 4ull * j, d); else *(data_u4*)(d + 4ull * j) = v0; }
        if (DIG) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
            __syncthreads();
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
            __syncthreads();
            if (threadIdx.x == 0) {
                const unsigned long long sum = (red[0] + red[1]) + (red[2] + red[3]);
                if (ATOM) { if (sum) (void)__hip_atomic_fetch_add(digests + p, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
                else if (sum == 0x1234567ull) digests[p] = sum;
            }
        }
    }
}

static unsigned long long host_digest(const std::vector<unsigned>& w) {
    unsigned long long d = 0;
    for (size_t i = 0; i < w.size(); ++i) {
        const unsigned k = (unsigned)(2ull * i + 1ull) * 0x9E3779B1u;
        d += ((unsigned long long)w[i] + 1ull) * k;
    }
    return d;
}

int main() {
    const size_t W = 41557932;                       // words per buffer (a multiple of 4)
    unsigned *src[4], *dst[4];
    unsigned long long* dig;
    for (int i = 0; i < 4; ++i) { CK(hipMalloc(&src[i], W * 4)); CK(hipMalloc(&dst[i], W * 4)); }
    CK(hipMalloc(&dig, 64));
    std::vector<unsigned> h(W);
    unsigned x = 12345u;
    for (size_t i = 0; i < W; ++i) { x = x * 1664525u + 1013904223u; h[i] = x; }
    const unsigned long long want = host_digest(h);
    for (int i = 0; i < 4; ++i) { CK(hipMemcpy(src[i], h.data(), W * 4, hipMemcpyHostToDevice)); CK(hipMemset(dst[i], 0, W * 4)); }
    hipStream_t st;
    CK(hipStreamCreate(&st));
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    V1Table T1;
    memset(&T1, 0, sizeof(T1));
    IafStateTable T3;
    memset(&T3, 0, sizeof(T3));
    for (int i = 0; i < 4; ++i) { T1.src[i] = src[i]; T1.dst[i] = dst[i]; T1.words[i] = W; T3.src[i] = src[i]; T3.dst[i] = dst[i]; T3.words[i] = W; }
    T1.n = T3.n = 4;
    const unsigned grid3 = iaf_state_assign(T3, IAF_STATE_MAX_BLOCKS);
    IafStateTable T3b = T3;
    const unsigned grid3b = iaf_state_assign(T3b, 512);
    printf("grid v3 %u (budget %d), %u (budget 512)\n", grid3, IAF_STATE_MAX_BLOCKS, grid3b);
    const char* names[] = {"memcpyD2D x4", "v1 2048x256 atomics+digest", "v1 no atomics", "v1 copy only", "v1 1024x256 atomics+digest",
                           "v3 budget 256", "v3 budget 512"};
    for (int v = 0; v < 7; ++v) {
        std::vector<float> ms;
        for (int rep = 0; rep < 25; ++rep) {
            CK(hipMemsetAsync(dig, 0, 64, st));
            CK(hipEventRecord(a, st));
            switch (v) {
                case 0: for (int i = 0; i < 4; ++i) CK(hipMemcpyAsync(dst[i], src[i], W * 4, hipMemcpyDeviceToDevice, st)); break;
                case 1: hipLaunchKernelGGL((v1_kernel<1, 1>), dim3(2048), dim3(256), 0, st, T1, dig); break;
                case 2: hipLaunchKernelGGL((v1_kernel<0, 1>), dim3(2048), dim3(256), 0, st, T1, dig); break;
                case 3: hipLaunchKernelGGL((v1_kernel<0, 0>), dim3(2048), dim3(256), 0, st, T1, dig); break;
                case 4: hipLaunchKernelGGL((v1_kernel<1, 1>), dim3(1024), dim3(256), 0, st, T1, dig); break;
                case 5: hipLaunchKernelGGL(iaf_state_snapshot_kernel, dim3(grid3), dim3(IAF_STATE_THREADS), 0, st, T3, dig); break;
                case 6: hipLaunchKernelGGL(iaf_state_snapshot_kernel, dim3(grid3b), dim3(IAF_STATE_THREADS), 0, st, T3b, dig); break;
            }
            CK(hipGetLastError());
            CK(hipEventRecord(b, st));
            CK(hipEventSynchronize(b));
            float t = 0;
            CK(hipEventElapsedTime(&t, a, b));
            if (rep >= 5) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        unsigned long long got[4] = {0, 0, 0, 0};
        CK(hipMemcpy(got, dig, 32, hipMemcpyDeviceToHost));
        const bool digest_ok = got[0] == want && got[1] == want && got[2] == want && got[3] == want;
        printf("%-30s median %.4f ms (min %.4f max %.4f)  %.2f TB/s moved  digest %s\n", names[v], ms[ms.size() / 2], ms.front(), ms.back(),
               2.0 * 4 * 4 * W / (ms[ms.size() / 2] * 1e-3) / 1e12, (v == 1 || v >= 4) ? (digest_ok ? "ok" : "WRONG") : "-");
        fflush(stdout);
    }
    std::vector<unsigned> back(W);
    CK(hipMemcpy(back.data(), dst[3], W * 4, hipMemcpyDeviceToHost));
    printf("copy %s\n", memcmp(back.data(), h.data(), W * 4) == 0 ? "ok" : "WRONG");
    return 0;
}
