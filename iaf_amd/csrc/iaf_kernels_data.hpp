// iaf_kernels_data.hpp -- the device-resident dataset: one launch gathers the next shuffled batch out of an image array in device memory
// (include/iaf_hip.h: iaf_data_next_batch).  The reference keeps its training set in the graph and pulls a shuffled batch
// out of it per step (tf_utils/cifar10_data.py:108-112, tf_utils/data_utils.py:29-36); this is the engine's counterpart, reproducible
// from (seed, step, row).  Part of the single translation unit iaf_engine.hip (included there behind iaf_kernels_rng.hpp, whose
// Philox4x32-10 is the round function here; not a standalone header).
#pragma once

#define IAF_DATA_SLICE 4096u            // bytes of one image a workgroup copies: 256 threads x 16 bytes

typedef unsigned data_u4 __attribute__((ext_vector_type(4)));

// What a draw needs besides the pointers (by value in the kernel arguments; all of it fixed per call, so a captured launch stays valid):
// n images of bpi bytes, G = B * world rows per global batch, bpe = n / G batches per epoch, first = rank * B, w = half the bit width
// of the Feistel domain, (k0, k1) the permutation's key.
struct IafDataDraw {
    unsigned long long bpi;
    unsigned n, G, bpe, first, w, k0, k1;
    int deterministic, vec16;
};

// perm_e(j): 4-round balanced Feistel network on 2w bits, walked along its cycle until it lands inside [0, n).  j < n lies on a cycle of
// the permutation of [0, 4^w) that returns to j itself, so the walk ends without a cap (a cap would break the bijection).
__device__ __forceinline__ unsigned iaf_data_perm(unsigned j, unsigned n, unsigned w, unsigned e_lo, unsigned e_hi, unsigned k0, unsigned k1) {
    if (n == 1u) return 0u;
    const unsigned mask = (1u << w) - 1u;
    unsigned y = j;
    do {
        unsigned L = y >> w, R = y & mask;
#pragma unroll
        for (unsigned r = 0; r < 4; ++r) {
            const unsigned f = iaf_philox4x32_10(RngU4{R, r, e_lo, e_hi}, k0, k1).x & mask;
            const unsigned t = L ^ f;
            L = R;
            R = t;
        }
        y = (L << w) | R;
    } while (y >= n);
    return y;
}

// grid (ceil(bpi / 4096), B): workgroup (s, r) copies slice s of the image of row r.  The step, and with it the image index, is the same
// for every lane: it is worked out once, on values made wave-uniform, and only the copy is per lane.
//   vec16   bpi % 16 == 0 and both bases on a 16-byte boundary (the host checked): every image starts on one, one 16-byte piece per lane;
//   else    bytes, lane-consecutive, which also covers a tail.
__global__ __launch_bounds__(256) void iaf_data_gather_kernel(const unsigned char* __restrict__ images, unsigned char* __restrict__ out,
                                                              long long* __restrict__ idx_out, const unsigned long long* __restrict__ step_p,
                                                              const IafDataDraw D) {
    const unsigned long long step = *step_p;
    const unsigned t_lo = __builtin_amdgcn_readfirstlane((unsigned)step), t_hi = __builtin_amdgcn_readfirstlane((unsigned)(step >> 32));
    const unsigned long long t = ((unsigned long long)t_hi << 32) | t_lo;
    const unsigned long long e = t / D.bpe;
    const unsigned r = blockIdx.y;
    const unsigned j = (unsigned)(t - e * D.bpe) * D.G + D.first + r;            // < bpe * G <= n
    const unsigned idx = D.deterministic ? j : iaf_data_perm(j, D.n, D.w, (unsigned)e, (unsigned)(e >> 32), D.k0, D.k1);
    const unsigned char* const src = images + (unsigned long long)idx * D.bpi;
    unsigned char* const dst = out + (unsigned long long)r * D.bpi;
    const unsigned long long lo = (unsigned long long)blockIdx.x * IAF_DATA_SLICE;
    if (D.vec16) {
        const unsigned long long o = lo + 16ull * threadIdx.x;
        if (o < D.bpi) *(data_u4*)(dst + o) = *(const data_u4*)(src + o);       // (bpi % 16 == 0: a piece that starts inside ends inside)
    } else {
        const unsigned long long hi = lo + IAF_DATA_SLICE < D.bpi ? lo + IAF_DATA_SLICE : D.bpi;
        for (unsigned long long o = lo + threadIdx.x; o < hi; o += 256) dst[o] = src[o];
    }
    if (idx_out && blockIdx.x == 0 && threadIdx.x == 0) idx_out[r] = (long long)idx;
}
