// iaf_kernels_rng.hpp -- the device noise source: Philox4x32-10 counters -> Box-Muller normals, one launch per LIST of tensors
// (include/iaf_hip.h: iaf_rng_fill_normal).  The reference draws its noise inside the graph
// (tf_utils/distributions.py:15-24); this is the engine's counterpart, reproducible from (seed, substream, step, element index).
// Part of the translation unit iaf_train_services.hip (included there and nowhere else, behind iaf_hip.h; not a standalone header).
#pragma once

// (IAF_RNG_MAX_TENSORS: include/iaf_hip.h)
#define IAF_RNG_MAX_BLOCKS 4096         // workgroups per tensor; beyond 4096 * 256 16-byte pieces a thread takes several

// The list travels BY VALUE in the kernel arguments (1.8 KB of the 4 KB segment): nothing to upload, nothing a stream capture
// could find changed under it.  blk_end[t]: one past the last workgroup of tensor t (ascending).
struct IafRngTable {
    float* out[IAF_RNG_MAX_TENSORS];
    unsigned long long count[IAF_RNG_MAX_TENSORS];
    unsigned sub[IAF_RNG_MAX_TENSORS];
    float scale[IAF_RNG_MAX_TENSORS];
    unsigned blk_end[IAF_RNG_MAX_TENSORS];
    int n;
};

typedef float rng_f4 __attribute__((ext_vector_type(4)));
struct RngU4 { unsigned x, y, z, w; };

// Philox4x32-10 (Salmon et al., SC'11): known answers in include/iaf_hip.h, checked by tests/test_noise_reference.py
__device__ __forceinline__ RngU4 iaf_philox4x32_10(RngU4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, c.x), l0 = 0xD2511F53u * c.x;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c.z), l1 = 0xCD9E8D57u * c.z;
        c = RngU4{h1 ^ c.y ^ k0, l1, h0 ^ c.w ^ k1, l0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// The four normals of counter (q, sub, step): elements 4q .. 4q+3 of the tensor.  Both uniforms are exact in fp32: u1 in (0, 1],
// u2 in [0, 1); the angle is handed over in half turns (2 u2, exact), so no rounded 2 pi enters.  |z| <= sqrt(48 ln 2).
__device__ __forceinline__ rng_f4 iaf_rng_quad(unsigned q, unsigned sub, unsigned s_lo, unsigned s_hi, unsigned k0, unsigned k1) {
    const RngU4 x = iaf_philox4x32_10(RngU4{q, sub, s_lo, s_hi}, k0, k1);
    const float r0 = sqrtf(-2.f * logf((float)((x.x >> 8) + 1u) * 0x1p-24f));
    const float r1 = sqrtf(-2.f * logf((float)((x.z >> 8) + 1u) * 0x1p-24f));
    float s0, c0, s1, c1;
    sincospif((float)(x.y >> 8) * 0x1p-23f, &s0, &c0);
    sincospif((float)(x.w >> 8) * 0x1p-23f, &s1, &c1);
    return rng_f4{r0 * c0, r0 * s0, r1 * c1, r1 * s1};
}

// Workgroups [blk_end[t-1], blk_end[t]) fill tensor t.  An element's value depends on its index alone, so neither the grid, nor the
// other tensors of the list, nor the pointer's alignment change it:
//   head  the a <= 3 elements in front of the first 16-byte boundary, and
//   tail  the < 4 elements behind the last whole 16-byte piece: one 4-byte store each, by the first threads of the tensor's first workgroup;
//   body  16-byte stores.  A tensor that starts ON a boundary (every torch allocation) has piece v = counter v; one that starts a
//         elements before a boundary has piece v = the last 4 - a normals of counter v and the first a of counter v + 1 (two counters per
//         piece: the rare case pays double rather than trade registers between lanes).
__global__ __launch_bounds__(256) void iaf_rng_fill_kernel(const IafRngTable T, const unsigned long long* step_p, unsigned k0,
                                                           unsigned k1) {
    int t = 0;
    while (t < T.n - 1 && blockIdx.x >= T.blk_end[t]) ++t;
    const unsigned b0 = t ? T.blk_end[t - 1] : 0u, nb = T.blk_end[t] - b0, lb = blockIdx.x - b0;
    float* const out = T.out[t];
    const unsigned long long count = T.count[t];
    const unsigned sub = T.sub[t];
    const float scale = T.scale[t];
    const unsigned long long step = *step_p;
    const unsigned s_lo = (unsigned)step, s_hi = (unsigned)(step >> 32);
    unsigned long long a = ((16u - (unsigned)((uintptr_t)out & 15u)) & 15u) >> 2;
    if (a > count) a = count;
    const unsigned long long nv = (count - a) >> 2, e0 = a + 4 * nv;        // 16-byte pieces; first element of the tail
    rng_f4* const body = (rng_f4*)(out + a);
    const unsigned long long stride = (unsigned long long)nb * 256;
    if (a == 0) {
        for (unsigned long long v = (unsigned long long)lb * 256 + threadIdx.x; v < nv; v += stride)
            body[v] = scale * iaf_rng_quad((unsigned)v, sub, s_lo, s_hi, k0, k1);
    } else {
        for (unsigned long long v = (unsigned long long)lb * 256 + threadIdx.x; v < nv; v += stride) {
            const rng_f4 p = iaf_rng_quad((unsigned)v, sub, s_lo, s_hi, k0, k1);
            const rng_f4 n = iaf_rng_quad((unsigned)v + 1u, sub, s_lo, s_hi, k0, k1);
            const rng_f4 o = a == 1 ? rng_f4{p.y, p.z, p.w, n.x} : a == 2 ? rng_f4{p.z, p.w, n.x, n.y} : rng_f4{p.w, n.x, n.y, n.z};
            body[v] = scale * o;
        }
    }
    if (lb == 0 && threadIdx.x < (unsigned)(a + (count - e0))) {             // at most 3 + 3 elements
        const unsigned long long i = threadIdx.x < a ? (unsigned long long)threadIdx.x : e0 + (threadIdx.x - a);
        const rng_f4 p = iaf_rng_quad((unsigned)(i >> 2), sub, s_lo, s_hi, k0, k1);
        const unsigned m = (unsigned)i & 3u;
        out[i] = scale * (m == 0 ? p.x : m == 1 ? p.y : m == 2 ? p.z : p.w);
    }
}

// the step counter: one thread, a plain 8-byte store, stream-ordered behind the fill that read it (add) or wherever it is enqueued (set)
__global__ void iaf_rng_step_kernel(unsigned long long* step_p, unsigned long long value, int add) {
    *step_p = add ? *step_p + value : value;
}
