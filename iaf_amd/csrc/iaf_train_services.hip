// iaf_train_services.hip -- the services of the training loop that take no stack and no conv (C ABI: include/iaf_hip.h): Adamax + EMA,
// the skip counter, the guard scans, the step's summaries, the device noise source, the device-resident dataset, the state snapshot
// and run_eval's image grids.
// A translation unit of its own beside iaf_engine.hip; its kernel headers are included here and nowhere else.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "iaf_hip.h"

#include "iaf_common.hpp"
#include "iaf_kernels_train.hpp"
#include "iaf_kernels_rng.hpp"
#include "iaf_kernels_data.hpp"
#include "iaf_kernels_image.hpp"

extern "C" int iaf_adamax_ema_step(float* var, const float* grad, float* slot_m, float* slot_v, float* ema, size_t n, float lr,
                                   float beta1, float beta2, float eps, float ema_decay, float grad_scale, void* stream) {
    if (!var || !grad || !slot_m || !slot_v) return IAF_ERR_NULL;
    if (n == 0) return IAF_OK;
    const bool al = (((uintptr_t)var | (uintptr_t)grad | (uintptr_t)slot_m | (uintptr_t)slot_v | (uintptr_t)ema) & 15) == 0;
    const size_t n4 = al ? n / 4 : 0;
    hipLaunchKernelGGL(iaf_adamax_ema_kernel, ew_grid(n4 ? n4 : n), dim3(256), 0, (hipStream_t)stream, var, grad, slot_m, slot_v,
                       ema, n4, n, lr, beta1, beta2, eps, ema_decay, grad_scale);
    return (int)hipGetLastError();
}

// the guarded step: a skip counter in mapped host memory (read without synchronising), the scan, the gated update
struct iaf_skip_counter {
    unsigned* host = nullptr;
    unsigned* dev = nullptr;
};

extern "C" int iaf_skip_counter_create(iaf_skip_counter_t** out) {
    if (!out) return IAF_ERR_NULL;
    *out = nullptr;
    iaf_skip_counter_t* c = new iaf_skip_counter_t();
    if (hipHostMalloc((void**)&c->host, 64, hipHostMallocMapped) != hipSuccess) { delete c; return (int)hipErrorOutOfMemory; }
    *(volatile unsigned*)c->host = 0u;
    if (hipHostGetDevicePointer((void**)&c->dev, c->host, 0) != hipSuccess) {
        (void)hipHostFree(c->host);
        delete c;
        return (int)hipErrorOutOfMemory;
    }
    *out = c;
    return IAF_OK;
}

extern "C" int iaf_skip_counter_read(const iaf_skip_counter_t* c, unsigned* count) {
    if (!c || !count) return IAF_ERR_NULL;
    *count = *(volatile const unsigned*)c->host;
    return IAF_OK;
}

extern "C" int iaf_skip_counter_ptr(const iaf_skip_counter_t* c, const unsigned** count) {
    if (!c || !count) return IAF_ERR_NULL;
    *count = c->dev;
    return IAF_OK;
}

extern "C" int iaf_skip_counter_destroy(iaf_skip_counter_t* c) {
    if (!c) return IAF_OK;
    if (c->host) (void)hipHostFree(c->host);
    delete c;
    return IAF_OK;
}

extern "C" int iaf_nonfinite_scan(const float* buf, size_t n, const float* extra, int n_extra, unsigned* guard, void* stream) {
    if (!guard || (n && !buf) || n_extra < 0 || (n_extra && !extra)) return IAF_ERR_NULL;
    if (n_extra > 256) return IAF_ERR_SHAPE;                 // (the extras are read by the first workgroup's lanes)
    if (((uintptr_t)guard & 7) != 0) return IAF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t n4 = ((uintptr_t)buf & 15) == 0 ? n / 4 : 0;
    hipLaunchKernelGGL(iaf_nonfinite_scan_kernel, ew_grid((n4 ? n4 : n) > (size_t)n_extra ? (n4 ? n4 : n) : (size_t)n_extra), dim3(256), 0, st, buf,
                       n4, n, extra, n_extra, guard);
    return (int)hipGetLastError();
}

extern "C" int iaf_nonfinite_scan_sumsq(const float* buf, size_t n, const float* extra, int n_extra, unsigned* guard, double* partials,
                                        double* sumsq, void* stream) {
    if (!guard || !partials || !sumsq || (n && !buf) || n_extra < 0 || (n_extra && !extra)) return IAF_ERR_NULL;
    if (n_extra > 256) return IAF_ERR_SHAPE;                 // (the extras are read by the first workgroup's lanes)
    if ((((uintptr_t)guard | (uintptr_t)partials | (uintptr_t)sumsq) & 7) != 0) return IAF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t n4 = ((uintptr_t)buf & 15) == 0 ? n / 4 : 0;
    // (the scan's grid: at most 2048 workgroups, one slot of `partials` each)
    hipLaunchKernelGGL(iaf_guard_sumsq_scan_kernel, ew_grid((n4 ? n4 : n) > (size_t)n_extra ? (n4 ? n4 : n) : (size_t)n_extra), dim3(256), 0,
                       st, buf, n4, n, extra, n_extra, guard, partials, sumsq);
    return (int)hipGetLastError();
}

extern "C" size_t iaf_train_summaries_bytes(int n_layers) {
    if (n_layers < 1 || n_layers > IAF_SUMMARY_MAX_LAYERS) return 0;
    return (size_t)(2 * (6 + 2 * n_layers) + 2) * 8;
}

extern "C" int iaf_train_summaries_reset(void* record, int n_layers, void* stream) {
    if (!record) return IAF_ERR_NULL;
    if (n_layers < 1 || n_layers > IAF_SUMMARY_MAX_LAYERS) return IAF_ERR_SHAPE;
    if (((uintptr_t)record & 7) != 0) return IAF_ERR_WORKSPACE;
    hipLaunchKernelGGL(iaf_train_summaries_reset_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)record,
                       (int)(iaf_train_summaries_bytes(n_layers) / 8));
    return (int)hipGetLastError();
}

extern "C" int iaf_train_summaries(const float* layer_obj, const float* layer_cost, const float* log_pxz, const float* dec_log_stdv,
                                   const float* loss_all, const double* sumsq, float grad_scale, const unsigned* guard, void* record,
                                   int n_layers, int n, void* stream) {
    if (!layer_obj || !layer_cost || !log_pxz || !dec_log_stdv || !loss_all || !sumsq || !guard || !record) return IAF_ERR_NULL;
    if (n_layers < 1 || n_layers > IAF_SUMMARY_MAX_LAYERS || n < 1) return IAF_ERR_SHAPE;
    if ((((uintptr_t)record | (uintptr_t)sumsq) & 7) != 0) return IAF_ERR_WORKSPACE;
    hipLaunchKernelGGL(iaf_train_summaries_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, layer_obj, layer_cost, log_pxz, dec_log_stdv,
                       loss_all, sumsq, grad_scale, guard, (double*)record, n_layers, n);
    return (int)hipGetLastError();
}

extern "C" int iaf_adamax_ema_step_guarded(float* var, const float* grad, float* slot_m, float* slot_v, float* ema, size_t n,
                                           float lr, float beta1, float beta2, float eps, float ema_decay, float grad_scale,
                                           const unsigned* guard, iaf_skip_counter_t* skips, void* stream) {
    if (!var || !grad || !slot_m || !slot_v || !guard || !skips) return IAF_ERR_NULL;
    const bool al = (((uintptr_t)var | (uintptr_t)grad | (uintptr_t)slot_m | (uintptr_t)slot_v | (uintptr_t)ema) & 15) == 0;
    const size_t n4 = al ? n / 4 : 0;
    hipLaunchKernelGGL(iaf_adamax_ema_guarded_kernel, ew_grid(n4 ? n4 : n), dim3(256), 0, (hipStream_t)stream, var, grad, slot_m,
                       slot_v, ema, n4, n, lr, beta1, beta2, eps, ema_decay, grad_scale, guard, skips->dev);
    return (int)hipGetLastError();
}

// One 64-bit step counter in device memory (the noise source's, the dataset's): a launch of its owner reads it and a one-thread launch
// behind that sets or advances it -- a replayed hipGraph moves on with no host code in between.
struct StepCounter {
    unsigned long long* d = nullptr;
    hipError_t create() {
        hipError_t e = hipMalloc((void**)&d, 64);
        if (e == hipSuccess) e = hipMemset(d, 0, 64);
        if (e != hipSuccess) destroy();
        return e;
    }
    void destroy() { if (d) (void)hipFree(d), d = nullptr; }
    // *d = add ? *d + value : value, enqueued on st
    int set(hipStream_t st, unsigned long long value, int add) {
        hipLaunchKernelGGL(iaf_rng_step_kernel, dim3(1), dim3(1), 0, st, d, value, add);
        return (int)hipGetLastError();
    }
    // the value behind everything st holds (synchronises st; refused while st captures)
    int tell(hipStream_t st, uint64_t* out) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (st) (void)hipStreamIsCapturing(st, &cs);
        if (cs == hipStreamCaptureStatusActive) return (int)hipErrorStreamCaptureUnsupported;
        unsigned long long v = 0;
        hipError_t e = hipMemcpyAsync(&v, d, sizeof(v), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return (int)e;
        *out = v;
        return IAF_OK;
    }
    const uint64_t* ptr() const { return (const uint64_t*)d; }
};

// the device noise source (iaf_kernels_rng.hpp): the seed lives here, the step counter in device memory, where the fill launch reads it
struct iaf_rng {
    unsigned long long seed = 0;
    StepCounter step;
};

extern "C" int iaf_rng_create(iaf_rng_t** out, uint64_t seed) {
    if (!out) return IAF_ERR_NULL;
    *out = nullptr;
    iaf_rng_t* r = new (std::nothrow) iaf_rng_t();
    if (!r) return (int)hipErrorOutOfMemory;
    r->seed = seed;
    const hipError_t e = r->step.create();
    if (e != hipSuccess) {
        delete r;
        return (int)e;
    }
    *out = r;
    return IAF_OK;
}

extern "C" int iaf_rng_destroy(iaf_rng_t* r) {
    if (!r) return IAF_OK;
    r->step.destroy();
    delete r;
    return IAF_OK;
}

extern "C" int iaf_rng_fill_normal(iaf_rng_t* r, float* const* outs, const size_t* counts, const unsigned* substreams,
                                   const float* scales, int n, int advance, void* stream) {
    if (!r) return IAF_ERR_NULL;
    if (n < 1 || n > IAF_RNG_MAX_TENSORS) return IAF_ERR_SHAPE;
    if (!outs || !counts || !substreams) return IAF_ERR_NULL;
    IafRngTable T;
    memset(&T, 0, sizeof(T));
    unsigned blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (!outs[i]) return IAF_ERR_NULL;
        if (counts[i] == 0 || (unsigned long long)counts[i] > (1ull << 34)) return IAF_ERR_SHAPE;
        if ((uintptr_t)outs[i] & 3) return IAF_ERR_WORKSPACE;
        const unsigned long long pieces = ((unsigned long long)counts[i] + 3) / 4, nb = (pieces + 255) / 256;
        blocks += (unsigned)(nb < IAF_RNG_MAX_BLOCKS ? nb : IAF_RNG_MAX_BLOCKS);
        T.out[i] = outs[i];
        T.count[i] = counts[i];
        T.sub[i] = substreams[i];
        T.scale[i] = scales ? scales[i] : 1.f;
        T.blk_end[i] = blocks;
    }
    T.n = n;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(iaf_rng_fill_kernel, dim3(blocks), dim3(256), 0, st, T, (const unsigned long long*)r->step.d,
                       (unsigned)(r->seed & 0xffffffffull), (unsigned)(r->seed >> 32));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !advance) return (int)e;
    return r->step.set(st, 1ull, 1);
}

extern "C" int iaf_rng_seek(iaf_rng_t* r, uint64_t step, void* stream) { return r ? r->step.set((hipStream_t)stream, step, 0) : IAF_ERR_NULL; }
extern "C" int iaf_rng_skip(iaf_rng_t* r, uint64_t steps, void* stream) { return r ? r->step.set((hipStream_t)stream, steps, 1) : IAF_ERR_NULL; }
extern "C" int iaf_rng_tell(iaf_rng_t* r, uint64_t* step, void* stream) { return r && step ? r->step.tell((hipStream_t)stream, step) : IAF_ERR_NULL; }
extern "C" int iaf_rng_step_ptr(iaf_rng_t* r, const uint64_t** step) { return r && step ? (*step = r->step.ptr(), IAF_OK) : IAF_ERR_NULL; }

// the device-resident dataset (iaf_kernels_data.hpp): images borrowed from the caller, seed and flag here, the step counter in device
// memory like the noise source's, where the gather reads it
struct iaf_data {
    const unsigned char* images = nullptr;
    unsigned long long n = 0, bpi = 0, seed = 0;
    int deterministic = 0;
    StepCounter step;
};

extern "C" int iaf_data_create(iaf_data_t** out, const unsigned char* images, uint64_t n, size_t bytes_per_image, uint64_t seed,
                               int deterministic) {
    if (!out) return IAF_ERR_NULL;
    *out = nullptr;
    if (!images) return IAF_ERR_NULL;
    if (n == 0 || n >= (1ull << 32) || bytes_per_image == 0) return IAF_ERR_SHAPE;
    iaf_data_t* d = new (std::nothrow) iaf_data_t();
    if (!d) return (int)hipErrorOutOfMemory;
    d->images = images;
    d->n = n;
    d->bpi = bytes_per_image;
    d->seed = seed;
    d->deterministic = deterministic != 0;
    const hipError_t e = d->step.create();
    if (e != hipSuccess) {
        delete d;
        return (int)e;
    }
    *out = d;
    return IAF_OK;
}

extern "C" int iaf_data_destroy(iaf_data_t* d) {
    if (!d) return IAF_OK;
    d->step.destroy();
    delete d;
    return IAF_OK;
}

extern "C" int iaf_data_next_batch(iaf_data_t* d, unsigned char* out, long long* idx_out, int B, int rank, int world, int advance,
                                   void* stream) {
    if (!d || !out) return IAF_ERR_NULL;
    if (B < 1 || B > IAF_DATA_MAX_BATCH || world < 1 || rank < 0 || rank >= world) return IAF_ERR_SHAPE;
    const unsigned long long G = (unsigned long long)B * (unsigned long long)world;
    if (G > d->n) return IAF_ERR_SHAPE;
    const unsigned long long slices = (d->bpi + IAF_DATA_SLICE - 1) / IAF_DATA_SLICE;
    if (slices > 0x7fffffffull) return IAF_ERR_SHAPE;
    IafDataDraw D;
    memset(&D, 0, sizeof(D));
    D.bpi = d->bpi;
    D.n = (unsigned)d->n;
    D.G = (unsigned)G;
    D.bpe = (unsigned)(d->n / G);
    D.first = (unsigned)rank * (unsigned)B;
    unsigned bits = 0;                                                  // bitlength(n - 1)
    for (unsigned long long v = d->n - 1; v; v >>= 1) ++bits;
    D.w = bits < 2 ? 1u : (bits + 1) / 2;
    D.k0 = (unsigned)(d->seed & 0xffffffffull) ^ 0x61746164u;
    D.k1 = (unsigned)(d->seed >> 32) ^ 0x5F666169u;
    D.deterministic = d->deterministic;
    D.vec16 = d->bpi % 16 == 0 && (((uintptr_t)d->images | (uintptr_t)out) & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(iaf_data_gather_kernel, dim3((unsigned)slices, (unsigned)B), dim3(256), 0, st, d->images, out, idx_out,
                       (const unsigned long long*)d->step.d, D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !advance) return (int)e;
    return d->step.set(st, 1ull, 1);
}

extern "C" int iaf_data_seek(iaf_data_t* d, uint64_t step, void* stream) { return d ? d->step.set((hipStream_t)stream, step, 0) : IAF_ERR_NULL; }
extern "C" int iaf_data_skip(iaf_data_t* d, uint64_t steps, void* stream) { return d ? d->step.set((hipStream_t)stream, steps, 1) : IAF_ERR_NULL; }
extern "C" int iaf_data_tell(iaf_data_t* d, uint64_t* step, void* stream) { return d && step ? d->step.tell((hipStream_t)stream, step) : IAF_ERR_NULL; }
extern "C" int iaf_data_step_ptr(iaf_data_t* d, const uint64_t** step) { return d && step ? (*step = d->step.ptr(), IAF_OK) : IAF_ERR_NULL; }

// the state snapshot (iaf_kernels_data.hpp): a memset of the digests and ONE launch; the table travels in the kernel arguments.  The
// *_ptr getters hand out the device's view of counters their objects already own, so that a snapshot can take them in the same launch.
extern "C" int iaf_state_snapshot(const iaf_state_part_t* parts, int n_parts, uint64_t* digests, void* stream) {
    if (!parts || !digests) return IAF_ERR_NULL;
    if (n_parts < 1 || n_parts > IAF_STATE_MAX_PARTS) return IAF_ERR_SHAPE;
    IafStateTable T;
    memset(&T, 0, sizeof(T));
    for (int i = 0; i < n_parts; ++i) {
        if (!parts[i].src) return IAF_ERR_NULL;
        if (parts[i].bytes == 0 || (parts[i].bytes & 3) != 0) return IAF_ERR_SHAPE;
        if ((((uintptr_t)parts[i].src | (uintptr_t)parts[i].dst) & 3) != 0) return IAF_ERR_WORKSPACE;
        T.src[i] = (const unsigned*)parts[i].src;
        T.dst[i] = (unsigned*)parts[i].dst;
        T.words[i] = (unsigned long long)parts[i].bytes / 4;
    }
    if (((uintptr_t)digests & 7) != 0) return IAF_ERR_WORKSPACE;
    T.n = n_parts;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(digests, 0, sizeof(uint64_t) * (size_t)n_parts, st);
    if (e != hipSuccess) return (int)e;
    const unsigned grid = iaf_state_assign(T, IAF_STATE_MAX_BLOCKS);      // (the chip's share of workgroups, in proportion to the parts' sizes)
    hipLaunchKernelGGL(iaf_state_snapshot_kernel, dim3(grid), dim3(IAF_STATE_THREADS), 0, st, T, (unsigned long long*)digests);
    return (int)hipGetLastError();
}

// run_eval's image summaries (iaf_kernels_image.hpp): the range of a slice into a 16-byte record, and the one launch that stretches and
// tiles.  The source table travels in the kernel arguments, as the snapshot's part table does.
extern "C" int iaf_img_range(const void* src, int dtype, size_t n_elems, void* record, void* stream) {
    if (!src || !record) return IAF_ERR_NULL;
    if ((dtype != IAF_IMG_U8 && dtype != IAF_IMG_F32) || n_elems == 0) return IAF_ERR_SHAPE;
    if (((uintptr_t)record & 7) != 0 || (dtype == IAF_IMG_F32 && ((uintptr_t)src & 3) != 0)) return IAF_ERR_WORKSPACE;
    const size_t per = dtype == IAF_IMG_U8 ? 16 : 4, esz = dtype == IAF_IMG_U8 ? 1 : 4;       // elements per 16-byte piece, bytes per element
    size_t head = ((16 - ((uintptr_t)src & 15)) & 15) / esz;                                   // elements before src's first 16-byte boundary
    if (head > n_elems) head = n_elems;
    const size_t pieces = (n_elems - head) / per;
    size_t grid = (pieces * 16 + IAF_IMG_RANGE_SHARE - 1) / IAF_IMG_RANGE_SHARE;
    if (grid > IAF_IMG_RANGE_MAX_BLOCKS) grid = IAF_IMG_RANGE_MAX_BLOCKS;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(iaf_img_range_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, src, dtype, (unsigned long long)n_elems,
                       (unsigned)head, (unsigned long long)pieces, (ImgRangeRec*)record);
    return (int)hipGetLastError();
}

// the reference's grid of n tiles of H x W pixels at aspect_ratio 1.0 (include/iaf_hip.h states it; iaf_amd/images.py: grid_shape)
static void img_grid_tiles(int n, int H, int W, int* th, int* tw) {
    const double ar = 1.0 * ((double)W / (double)H);
    *th = (int)ceil(sqrt((double)n * ar));
    *tw = (int)ceil(sqrt((double)n / ar));
}

extern "C" int iaf_img_grid(const iaf_img_source_t* sources, int n_src, int n_imgs, int C, int H, int W, int border, float border_color,
                            float* grid_f32, unsigned char* grid_u8, void* stream) {
    if (!sources || (!grid_f32 && !grid_u8)) return IAF_ERR_NULL;
    if (n_src < 1 || n_src > 2 || n_imgs < 1 || (C != 1 && C != 3) || H < 1 || W < 1 || border < 0) return IAF_ERR_SHAPE;
    ImgGridTable T;
    memset(&T, 0, sizeof(T));
    for (int s = 0; s < n_src; ++s) {
        if (!sources[s].ptr || !sources[s].outer) return IAF_ERR_NULL;
        if (sources[s].dtype != IAF_IMG_U8 && sources[s].dtype != IAF_IMG_F32) return IAF_ERR_SHAPE;
        if ((((uintptr_t)sources[s].outer | (uintptr_t)sources[s].inner) & 7) != 0) return IAF_ERR_WORKSPACE;
        if (sources[s].dtype == IAF_IMG_F32 && ((uintptr_t)sources[s].ptr & 3) != 0) return IAF_ERR_WORKSPACE;
        T.ptr[s] = sources[s].ptr;
        T.dtype[s] = sources[s].dtype;
        T.outer[s] = (const ImgRangeRec*)sources[s].outer;
        T.inner[s] = (const ImgRangeRec*)sources[s].inner;
    }
    if (((uintptr_t)grid_f32 & 3) != 0) return IAF_ERR_WORKSPACE;
    int th = 0, tw = 0;
    img_grid_tiles(n_imgs, H, W, &th, &tw);
    const long long Hg = ((long long)H + border) * th - border, Wg = ((long long)W + border) * tw - border;
    if (Hg < 1 || Wg < 1 || Hg * Wg >= (1ll << 31) || (long long)th * tw < n_imgs) return IAF_ERR_SHAPE;
    hipLaunchKernelGGL(iaf_img_grid_kernel, dim3((unsigned)((Hg * Wg + 255) / 256)), dim3(256), 0, (hipStream_t)stream, T, n_src, n_imgs, C, H, W,
                       border, border_color, th, tw, (int)Hg, (int)Wg, grid_f32, grid_u8);
    return (int)hipGetLastError();
}
