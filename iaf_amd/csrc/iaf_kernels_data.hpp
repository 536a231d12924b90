// iaf_kernels_data.hpp -- the device-resident dataset: one launch gathers the next shuffled batch out of an image array in device memory
// (include/iaf_hip.h: iaf_data_next_batch).  The reference keeps its training set in the graph and pulls a shuffled batch
// out of it per step (tf_utils/cifar10_data.py:108-112, tf_utils/data_utils.py:29-36); this is the engine's counterpart, reproducible
// from (seed, step, row).  Part of the translation unit iaf_train_services.hip (included there and nowhere else, behind iaf_kernels_rng.hpp, whose
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

// The state snapshot (include/iaf_hip.h: iaf_state_snapshot): ONE launch reads up to 8 parts once, writes the same bytes to
// each part's destination (if it has one) and leaves a 64-bit digest of each part's 32-bit words,
//     digest = sum_i (w_i + 1) * k_i  mod 2^64,   k_i = ((2 i + 1) * 0x9E3779B1) mod 2^32,   (w_i + 1) taken in 64 bits,
// a sum mod 2^64: any reduction order and any grid give the same bits.  Per word one 32x32->64 multiply-add ((w + 1) k = w k + k).  A guard
// against truncation, torn writes and stray bytes -- not a cryptographic hash.  The table travels by value in the kernel arguments, so a
// captured launch stays valid.
//   the grid is sized to the chip (at most IAF_STATE_MAX_BLOCKS workgroups of 1024 lanes: one per CU) and shared out among the parts in
//   proportion to their sizes, at least one workgroup each (iaf_state_assign; blk_end[p] = one past part p's last workgroup);
//   a part's workgroups walk it grid-stride: a scalar head up to the source's first 16-byte boundary, 16-byte loads over the body -- four in
//   flight per lane, the next four issued before the current four are stored --, a scalar tail; the stores are 16 bytes wide where the
//   destination is congruent to the source mod 16 and dwords where it is not;
//   lanes accumulate in 64 bits, a wave combines by shuffles, the workgroup's sixteen waves through 128 bytes of LDS, and lane 0 adds the
//   workgroup's sum to digests[p] with ONE agent-scope 64-bit atomic (skipped when the sum is 0: it would add nothing).  The host zeroes
//   digests[] in front of the launch (a memset node in a captured graph), so a replay leaves the digest of what THAT replay read.
#define IAF_STATE_THREADS 1024
#define IAF_STATE_MAX_BLOCKS 256

struct IafStateTable {                  // (IAF_STATE_MAX_PARTS: include/iaf_hip.h)
    const unsigned* src[IAF_STATE_MAX_PARTS];
    unsigned* dst[IAF_STATE_MAX_PARTS];
    unsigned long long words[IAF_STATE_MAX_PARTS];
    unsigned blk_end[IAF_STATE_MAX_PARTS];
    int n;
};

// the workgroups of a launch over T.words[0 .. T.n): part p gets 1 + its share of the rest of `budget` (>= T.n), and never more than it
// has rounds of 16 words per lane for; returns the grid
static inline unsigned iaf_state_assign(IafStateTable& T, unsigned budget) {
    unsigned long long total = 0;
    for (int p = 0; p < T.n; ++p) total += T.words[p];
    const unsigned long long spare = budget > (unsigned)T.n ? budget - (unsigned)T.n : 0;
    unsigned end = 0;
    for (int p = 0; p < T.n; ++p) {
        const unsigned long long per = 16ull * IAF_STATE_THREADS, want = (T.words[p] + per - 1) / per;
        unsigned long long nb = 1 + (unsigned long long)((long double)spare * (long double)T.words[p] / (long double)(total ? total : 1));
        if (nb > want) nb = want;
        if (nb < 1) nb = 1;
        end += (unsigned)nb;
        T.blk_end[p] = end;
    }
    return end;
}

// (w + 1) k = w k + k: the products into `acc` (one multiply-add each), the k's into `ks`; the digest is their sum
__device__ __forceinline__ void iaf_state_term(unsigned w, unsigned i, unsigned long long& acc, unsigned long long& ks) {
    const unsigned k = (2u * i + 1u) * 0x9E3779B1u;
    acc += (unsigned long long)w * k;
    ks += k;
}

__device__ __forceinline__ void iaf_state_piece(const data_u4 v, unsigned long long i, unsigned* d, bool vst, unsigned long long& acc,
                                                unsigned long long& ks) {
    if (vst) {
        *(data_u4*)(d + i) = v;
    } else if (d) {
        d[i] = v.x;
        d[i + 1] = v.y;
        d[i + 2] = v.z;
        d[i + 3] = v.w;
    }
    const unsigned i32 = (unsigned)i;                  // (k_i depends on i mod 2^31 only)
    iaf_state_term(v.x, i32, acc, ks);
    iaf_state_term(v.y, i32 + 1u, acc, ks);
    iaf_state_term(v.z, i32 + 2u, acc, ks);
    iaf_state_term(v.w, i32 + 3u, acc, ks);
}

__global__ __launch_bounds__(IAF_STATE_THREADS) void iaf_state_snapshot_kernel(const IafStateTable T, unsigned long long* __restrict__ digests) {
    __shared__ unsigned long long red[IAF_STATE_THREADS / 64];
    int p = 0;
    unsigned first = 0;
    while (p < T.n - 1 && blockIdx.x >= T.blk_end[p]) first = T.blk_end[p++];               // (uniform: this workgroup's part)
    const unsigned long long stride = (unsigned long long)(T.blk_end[p] - first) * IAF_STATE_THREADS,
                             t = (unsigned long long)(blockIdx.x - first) * IAF_STATE_THREADS + threadIdx.x;
    const unsigned* const s = T.src[p];
    unsigned* const d = T.dst[p];
    const unsigned long long n = T.words[p];
    unsigned long long head = ((16u - (unsigned)((uintptr_t)s & 15u)) & 15u) >> 2;          // words in front of the source's 16-byte boundary
    if (head > n) head = n;
    const unsigned long long n4 = (n - head) >> 2, rest = n - 4ull * n4;                     // rest = head + tail <= 6
    const bool vst = d && (((uintptr_t)s ^ (uintptr_t)d) & 15u) == 0;
    const data_u4* const sv = (const data_u4*)(s + head);
    unsigned long long acc = 0, ks = 0;
    unsigned long long j = t;
    // rounds of four pieces per lane on two register sets in turn: set B's loads go out before set A's stores and the other way round, so
    // that loads and stores of neighbouring rounds are in flight together and no round waits for its own stores
    const unsigned long long s1 = stride, s2 = 2ull * stride, s3 = 3ull * stride, s4 = 4ull * stride;
    data_u4 a0, a1, a2, a3, b0, b1, b2, b3;
    bool have = j + s3 < n4;                                                                 // a whole round for this lane
    if (have) {
        a0 = sv[j];
        a1 = sv[j + s1];
        a2 = sv[j + s2];
        a3 = sv[j + s3];
    }
    while (have) {
        const unsigned long long jb = j + s4;
        const bool have_b = jb + s3 < n4;
        if (have_b) {
            b0 = sv[jb];
            b1 = sv[jb + s1];
            b2 = sv[jb + s2];
            b3 = sv[jb + s3];
        }
        iaf_state_piece(a0, head + 4ull * j, d, vst, acc, ks);
        iaf_state_piece(a1, head + 4ull * (j + s1), d, vst, acc, ks);
        iaf_state_piece(a2, head + 4ull * (j + s2), d, vst, acc, ks);
        iaf_state_piece(a3, head + 4ull * (j + s3), d, vst, acc, ks);
        j = jb;
        if (!have_b) break;
        const unsigned long long ja = j + s4;
        have = ja + s3 < n4;
        if (have) {
            a0 = sv[ja];
            a1 = sv[ja + s1];
            a2 = sv[ja + s2];
            a3 = sv[ja + s3];
        }
        iaf_state_piece(b0, head + 4ull * j, d, vst, acc, ks);
        iaf_state_piece(b1, head + 4ull * (j + s1), d, vst, acc, ks);
        iaf_state_piece(b2, head + 4ull * (j + s2), d, vst, acc, ks);
        iaf_state_piece(b3, head + 4ull * (j + s3), d, vst, acc, ks);
        j = ja;
    }
    for (; j < n4; j += stride) iaf_state_piece(sv[j], head + 4ull * j, d, vst, acc, ks);      // fewer than four pieces left for this lane
    if (t < rest) {                                                                          // the head's words, then the tail's
        const unsigned long long i = t < head ? t : t + 4ull * n4;
        const unsigned w = s[i];
        if (d) d[i] = w;
        iaf_state_term(w, (unsigned)i, acc, ks);
    }
    acc += ks;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
#pragma unroll
        for (int w = 0; w < IAF_STATE_THREADS / 64; ++w) sum += red[w];
        if (sum) (void)__hip_atomic_fetch_add(digests + p, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
