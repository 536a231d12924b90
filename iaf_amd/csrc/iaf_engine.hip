// iaf_engine.hip -- MI355X (gfx950 / CDNA4) IAF posterior engine: kernels + C ABI (include/iaf_hip.h).
//
// What is computed (reference file:line, relative to the reference tree):
//   weight prep   get_conv_ar_mask + weight-norm          tf_utils/layers.py:134-141, 56-60
//   masked conv   ar_conv2d / ar_multiconv2d               tf_utils/layers.py:144-166, 63-64
//   IAF step      m,s=0.1*out; z=(z-m)/exp(s); logqs+=s    tf_train.py:69-72
//   posterior     sample/logqs/logps/KL/free bits          tf_train.py:56-85, tf_utils/distributions.py:5-25
//   IW bound      logsumexp / compute_lowerbound           tf_utils/distributions.py:35-62
//
// Design (DESIGN.md has the long form).  The MADE mask is exploited as structured sparsity, not
// as a scan: 4 of the 9 taps are dead and are never touched (the centre tap is block-triangular; its dead
// 16x16 blocks are stored as zeros and still multiplied by the layer-by-layer kernels; the one-launch step skips them).
// Each masked conv is an implicit GEMM on the exact-fp32 MFMA
// (v_mfma_f32_16x16x4_f32):  D[co][pixel] += W[co][k] * X[k][pixel],  k = (tap, c_in).
//   * X tile: pixel-major [slot][c_in (+8 pad)] in LDS, staged once per workgroup with a one-sided
//     halo (live taps only look right/below); tap shifts are per-lane LDS addresses, image borders
//     are a dedicated all-zero slot -- no predication in the main loop.
//   * W: repacked by the prep kernel into MFMA fragment order [chunk][tap][co_tile][lane][4] so a
//     wave fetches one contiguous 1 KiB global_load_dwordx4 per 4 MFMAs; waves never synchronise
//     inside the K loop.
//   * K order inside a 16-channel chunk is permuted (lane k-slot kk owns channels 4kk..4kk+3) so both
//     operands are 16-byte loads.
//   * epilogues fuse bias, context add, ELU, the 0.1 scaling, the affine transform and the
//     log-det term; hidden activations live in a pixel-major scratch that the next conv stages
//     with straight 16-byte copies.
//
// Source layout (this translation unit; the .hpp files below are sections of it, included in order -- a kernel header belongs to ONE
// unit: its __global__ functions are not static):
//   iaf_conv_kernel.hpp       the implicit-GEMM conv kernel template (instantiated per launch shape in iaf_conv_inst.hip)
//   iaf_kernels_prep.hpp      mask / weight-norm / repack kernels
//   iaf_common.hpp            shared with the two units below: the elementwise launch grid, HIP_TRY, two device helpers of the reductions
//   iaf_kernels_misc.hpp      what the stack itself launches: KL + free bits, max-diff, the inverse step's control kernels
//   iaf_kernels_backward.hpp  weight gradient, weight-norm backward, staging, posterior-block backward pieces
//   iaf_kernels_generic.hpp   direct-conv fallback for channel counts outside the MFMA path
//   iaf_kernels_resample.hpp  the deconv2d weight prep and its backward (downsampling IAFLayer)
//   (this file)               stack object, launch logic, C ABI of the masked stack, forward / inverse / training, free bits
//   iaf_conv3x3_host.hpp      C ABI of the plain and single masked 3x3 convs
// Units of their own, with the entry points that take no stack and no conv:
//   iaf_model_ops.hip         the model's own operations: its two ends around the layer stack (CVAE1._forward: x_enc, h_top, x_dec,
//                             obj / loss) and their backward (iaf_kernels_edge.hpp); Gaussian sample / logps, 'up_iaf2_nl' backward halves,
//                             lower bound, evaluation tail, data-dependent init, likelihood, 2x resampling (iaf_kernels_objective.hpp)
//   iaf_train_services.hip    Adamax + EMA, skip counter, guard scans, summaries (iaf_kernels_train.hpp), the device noise source
//                             (iaf_kernels_rng.hpp), the device-resident dataset and the state snapshot (iaf_kernels_data.hpp)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iterator>
#include <map>
#include <mutex>
#include <new>
#include <unordered_set>
#include <vector>

#include "iaf_hip.h"

#include "iaf_conv_kernel.hpp"

#define IAF_ABI_VERSION 8   // 8: the plain convs on two fp16 planes (iaf_conv3x3_range_errors, iaf_conv3x3_runs_f16x2); 7: IAF_PRECISION_F16X2 / IAF_PACK_F16X2 / IAF_ERR_RANGE / iaf_stack_range_errors (the two-plane fp16 step kernels); 6: iaf_stack_step_pairs, iaf_conv3x3_set_debug(conv, buf, bytes), generic backward behind the training entry points; 5: per-stream halo-exchange sets, IAF_ERR_EXCHANGE, iaf_stack_set_halo_exchange_debug; 4: stack-owned halo-exchange buffers (iaf_stack_set_halo_exchange / _exchange_errors / _step_exchanges): a stack's
                          //    one-launch steps must not overlap on different streams; 2: + iaf_conv3x3_*; 3: bf16x3 default precision, THEANO_FLIPMASK, negative nt in autotune reports,
                          //    iaf_stack_set_packs, iaf_comm_* (include/iaf_hip.h)
#define MAX_GEMM_LAYERS 10   // depth_ar <= 9 hidden + 1 output pair

#include "iaf_common.hpp"
#include "iaf_step_fused_types.hpp"
#include "iaf_kernels_prep.hpp"
#include "iaf_kernels_misc.hpp"
#include "iaf_kernels_backward.hpp"
#include "iaf_kernels_generic.hpp"
#include "iaf_kernels_resample.hpp"

#include "iaf_pack_state.hpp"   // the pack / precision / range protocol of iaf_stack and iaf_conv3x3 (no HIP in it: walked on a CPU by tests/test_pack_state.py)

// ---------------------------------------------------------------------------------------------
// host side: stack object
// ---------------------------------------------------------------------------------------------
struct GemmLayer {
    int cin, cout;        // cout = GEMM N (output pair: 2*n_z)
    int nchunk, ncot;
    int zerodiag, npair;
    float* wp = nullptr;
    float* bias = nullptr;
    float* border = nullptr;   // Theano variant only
    float* wpt = nullptr;      // transposed pack for dgrad (allocated by iaf_stack_set_training)
    void* wpt3 = nullptr;      // its bf16x3 form (iaf_pack_t3_kernel; even tile counts only): the data gradient on the bf16 matrix cores
    void* wp3 = nullptr;       // bf16x3 pack for iaf_conv_bf3_kernel (c_in % 32 == 0 only)
    void* wp2 = nullptr;       // two-plane fp16 pack of the F16 step kernels (allocated by iaf_stack_set_precision(F16X2))
    void* wpt2 = nullptr;      // ... of the TRANSPOSED problem (plain convs in training: the data gradient on two fp16 planes, iaf_conv_bf3.hpp DG16)
    int b_nt = 0, b_ppw = 0, b_pxt = 0, b_ks = 0, b_wco = 1;   // bf16x3 launch shape (auto or iaf_stack_set_tuning_bf3)
    bool b_user_tuned = false;
    // result of iaf_stack_autotune for one problem size: which kernel family and which bf16x3 shape won the timing
    long long tuned_P = -1; int tuned_W = -1; bool tuned_bf3 = false; int t_nt = 0, t_ppw = 0, t_pxt = 0, t_ks = 0, t_wco = 1;
    // layer 1 only: the first layer fused into this layer's kernel (IN_FUSED0): result of iaf_stack_autotune for one size
    long long fz_P = -1; int fz_W = -1; bool fz_on = false; int fz[5] = {0, 0, 0, 0, 1};
    float tuned_us = 0.f;      // time of the winner of the last iaf_stack_autotune
    int* lim = nullptr;
    // launch shape: fixed by iaf_stack_set_tuning (user_tuned) or chosen per problem size by auto_shape()
    int nt, pxt, wco, ks;
    bool user_tuned = false;
    bool full3x3 = false;      // plain 9-tap conv (iaf_conv3x3): halo on both sides of the pixel tile
    unsigned long long* dbg = nullptr; size_t dbg_bytes = 0;   // dev tool (iaf_conv3x3_set_debug): cycle stamps of THIS conv's bf16x3 launches
    double live_macs_per_px, dense_macs_per_px;
};

// the HIP half of the range word (iaf_pack_state.hpp has the protocol): mapped pinned memory an fp16 launch raises, read by the host
// without synchronising
struct RangeWord {
    unsigned* host = nullptr;
    unsigned* dev = nullptr;       // its device-side alias
    int alloc() {
        if (host) return IAF_OK;
        if (hipHostMalloc((void**)&host, 64, hipHostMallocMapped) != hipSuccess) { host = nullptr; return (int)hipErrorOutOfMemory; }
        *(volatile unsigned*)host = 0u;
        if (hipHostGetDevicePointer((void**)&dev, host, 0) != hipSuccess) { free(); return (int)hipErrorOutOfMemory; }
        return IAF_OK;
    }
    unsigned peek() const { return host ? *(volatile unsigned*)host : 0u; }
    // every launch so far has had its say
    int read(unsigned* errors) const {
        *errors = 0;
        if (!host) return IAF_OK;
        if (hipError_t e = hipDeviceSynchronize()) return (int)e;
        *errors = peek();
        return IAF_OK;
    }
    int rearm() {
        if (hipError_t e = hipDeviceSynchronize()) return (int)e;
        *(volatile unsigned*)host = 0u;
        return IAF_OK;
    }
    void free() {
        if (host) (void)hipHostFree(host);
        host = dev = nullptr;
    }
};

struct iaf_stack : PackState {     // precision (forward convs: F32 = the exact fp32 MFMA, else split products), packs, f16_off, prepared
    int n_z, n_h, depth_ar, variant;
    int nlayers;          // depth_ar + 1
    int resnet = 0;       // iaf_stack_create_resnet: residual blocks of the masked ResNet (ar.py:478-528), 0 = the plain conv stack.  Such a
                          // stack has depth_ar = 2 resnet + 1 hidden convs -- L[0] the input conv, L[2i+1] / L[2i+2] conv1 / conv2 of block i --
                          // so everything that walks L[] (prepare, packs, weight gradients, weight norm, work counts) serves it unchanged
    GemmLayer L[MAX_GEMM_LAYERS];
    GemmLayer T[MAX_GEMM_LAYERS];   // transposed problems (dX = W^T dY) of the same layers; valid when training
    bool training = false;
    bool defer_wn = false;    // backward leaves the weight-norm pass to iaf_wn_bwd_batch_run (one launch per model)
    float* pend_ws = nullptr; int pend_B = 0, pend_H = 0, pend_W = 0;   // ... which finds dWeff / dbp through these
    bool generic = false;     // channel counts outside the MFMA path: direct-conv fallback kernels
    // one-launch step with halo exchange (iaf_step_fused.hpp, XCH): the rows the row blocks hand each other, their flag lines, the
    // work-list heads -- one SET per stream the stack has launched such a step on (a set is used by one
    // launch at a time; launches of one stream are ordered), so calls on different streams do not share state (SURVEY 8b:
    // re-entrant per stream).  Allocated on a stream's first such launch outside a capture; nothing in a set is cleared between
    // launches (a consumer puts the "not there yet" pattern back into what it has taken, the last arrival zeroes the counters).  Outgrown buffers live as long as the stack: a captured graph
    // may still name them.
    struct XchSet {
        hipStream_t st = nullptr;
        char* buf = nullptr; size_t bytes = 0;                 // rows: every dword `pattern` between launches
        unsigned pattern = IAF_XSENT;                          // IAF_XSENT (bf16 planes) or IAF_XSENT_F16 (fp16 planes): a set serves kernels of ONE plane type
        bool captured = false;                                 // a hipGraph names this set's rows and counters: no OTHER capture stream may take it over
        unsigned long long* ctl = nullptr;                     // heads, arrivals, sticky error (StepP::xctl), arrivals of the in-launch KL finish (StepP::fin_ctl = xctl + IAF_XCTL_FIN): zero between launches
    };
    std::deque<XchSet> xch_sets;           // (stable addresses: a launch holds a pointer to its set outside the lock)
    std::mutex xch_mu;
    struct XchRetired { char* first; size_t second; unsigned pattern; };
    std::vector<XchRetired> xch_retired_rows;
    unsigned* xch_err_host = nullptr;     // mapped pinned word the kernels raise when a bounded wait gives up: read at every launch,
    unsigned* xch_err_dev = nullptr;      // ... without synchronising; its device-side alias
    bool xch_on = true;                   // iaf_stack_set_halo_exchange
    unsigned xch_knob = 0;                // iaf_stack_set_halo_exchange_debug
    int fb_groups = 1;                    // iaf_stack_set_free_bits_groups: the posterior block's free-bits mean per contiguous run of B / fb_groups rows
    int fuse_first = 2;       // first masked conv fused into the second one's kernel: 0 never, 1 whenever possible, 2 only where
                              // iaf_stack_autotune measured it faster (on MI355X at the BASELINE sizes it is not: docs/LAB_NOTEBOOK_r01-r03.md 4.8)
    int fuse_step = 1;        // the whole step as ONE launch (iaf_step_fused.hpp): 0 never, 1 where a compiled geometry covers it and
                              // the size rule / autotune's measurement favours it, 2 wherever a compiled geometry covers it
    long long fs_P = -1; int fs_W = 0; bool fs_on = false;   // ... unless iaf_stack_autotune measured this size: then what it found
    int fs_force = -1;        // (autotune's own measurements: -1 off, 0 / 1 = take this path regardless)
    // IAF_PRECISION_F16X2: the word the F16 kernels (and the prep of their packs) raise when an operand lies beyond fp16's largest finite
    // number -- mapped pinned memory, read without synchronising at the stack's next launch, which then returns IAF_ERR_RANGE once and
    // the stack goes on with the bf16x3 kernels (f16_off) until iaf_stack_set_precision(F16X2) is called again
    RangeWord rng;
    size_t weight_bytes;  // raw V/g/b bytes of the stack (for the algorithmic byte count)
    // optional per-launch event timing of one layer
    unsigned long long* dbg = nullptr; int dbg_layer = -1;
    int prof_layer = -1, prof_cap = 0, prof_n = 0;
    hipEvent_t* prof_start = nullptr;
    hipEvent_t* prof_stop = nullptr;
};

// ---- descriptor table of a batched prep launch: host-built PrepLayer array -> device ---------------------------------
// (the ring of pinned snapshots had no completion tracking.)  An async upload reads its pinned source when the
// copy EXECUTES, so the source must stay untouched until then:
//  * eager streams: PREP_RING pinned snapshots, an event recorded behind each upload; a slot is rewritten only after its
//    event has completed (the host waits if it ever runs PREP_RING pointer-changing prep runs ahead of the GPU);
//  * stream capture: every captured run gets its OWN device table (PREP_CAPTURE_SLOTS of them, allocated up front: no
//    allocation inside a capture), frozen for the life of the batch object like the kernel arguments of the captured launches
//    themselves.  It is filled synchronously AT CAPTURE TIME on a private stream (capture mode relaxed around the copy), so
//    the graph carries no copy node (round 3 first recorded one: 4.9 us per replay of a 475 us step); if the runtime refuses
//    that, the copy is captured from the slot's own pinned snapshot instead.  Either way a replay neither reads a recycled
//    snapshot nor overwrites the table the eager runs keep equal to their host copy.
#define PREP_RING 4
#define PREP_CAPTURE_SLOTS 16
struct DescTable {
    size_t bytes;
    char* h_ring;                  // pinned: PREP_RING eager snapshots, then PREP_CAPTURE_SLOTS capture snapshots
    char* d_tabs;                  // device: table 0 = the eager one, then one per capture slot
    hipEvent_t ev[PREP_RING];
    bool pending[PREP_RING];
    hipStream_t up;                // private stream of the capture-time uploads
    int ring_i, ncap;
    bool cap_done[PREP_CAPTURE_SLOTS];   // the slot's device table was written OUTSIDE any graph (else: only by a copy node of the graph that took it)
    bool uploaded;                 // the eager device table holds the caller's current host copy
};
static size_t desc_stride(const DescTable* t) { return (t->bytes + 255) / 256 * 256; }
static int desc_init(DescTable* t, size_t bytes) {
    memset(t, 0, sizeof(*t));
    t->bytes = bytes;
    const size_t st = desc_stride(t);
    HIP_TRY(hipHostMalloc((void**)&t->h_ring, st * (PREP_RING + PREP_CAPTURE_SLOTS)));
    HIP_TRY(hipMalloc((void**)&t->d_tabs, st * (1 + PREP_CAPTURE_SLOTS)));
    for (int i = 0; i < PREP_RING; ++i) HIP_TRY(hipEventCreateWithFlags(&t->ev[i], hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&t->up, hipStreamNonBlocking));
    return IAF_OK;
}
static void desc_destroy(DescTable* t) {
    for (int i = 0; i < PREP_RING; ++i)
        if (t->ev[i]) (void)hipEventDestroy(t->ev[i]);
    if (t->up) (void)hipStreamDestroy(t->up);
    if (t->h_ring) (void)hipHostFree(t->h_ring);
    if (t->d_tabs) (void)hipFree(t->d_tabs);
    memset(t, 0, sizeof(*t));
}
// Makes `host` (t->bytes of descriptors) visible to a kernel launched on `st` behind this call; *d_out = the table to pass.
// changed: the host copy differs from what the last eager upload carried.
static int desc_upload(DescTable* t, const void* host, bool changed, hipStream_t st, const void** d_out) {
    const size_t stride = desc_stride(t);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (st) (void)hipStreamIsCapturing(st, &cs);
    if (cs == hipStreamCaptureStatusActive) {
        //  the caller's host copy now holds THIS run's pointers while the eager device table keeps the previous
        // ones: the next eager run must upload even if it finds its host copy unchanged
        if (changed) t->uploaded = false;
        //  a capture of descriptors that an earlier capture already froze -- the usual re-capture of the same
        // tensors -- shares that slot's table; only captures of NEW pointer sets take a slot, PREP_CAPTURE_SLOTS per object
        // (include/iaf_hip.h: IAF_ERR_CAPTURE_SLOTS)
        for (int i = 0; i < t->ncap; ++i)
            if (!memcmp(t->h_ring + stride * (PREP_RING + i), host, t->bytes)) {
                //  a slot whose table was only ever filled by a copy NODE of the graph that took it is unwritten if that
                // graph was never launched (or is gone): this capture then carries the copy too
                if (!t->cap_done[i])
                    HIP_TRY(hipMemcpyAsync(t->d_tabs + stride * (1 + i), t->h_ring + stride * (PREP_RING + i), t->bytes, hipMemcpyHostToDevice, st));
                *d_out = t->d_tabs + stride * (1 + i);
                return IAF_OK;
            }
        if (t->ncap >= PREP_CAPTURE_SLOTS) return IAF_ERR_CAPTURE_SLOTS;
        char* snap = t->h_ring + stride * (PREP_RING + t->ncap);
        char* dtab = t->d_tabs + stride * (1 + t->ncap);
        const int slot_i = t->ncap;
        t->ncap++;
        memcpy(snap, host, t->bytes);
        hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
        bool done = false;
        if (hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess) {
            done = hipMemcpyAsync(dtab, snap, t->bytes, hipMemcpyHostToDevice, t->up) == hipSuccess &&
                   hipStreamSynchronize(t->up) == hipSuccess;
            (void)hipThreadExchangeStreamCaptureMode(&mode);
        }
        t->cap_done[slot_i] = done;
        if (!done) {
            (void)hipGetLastError();
            HIP_TRY(hipMemcpyAsync(dtab, snap, t->bytes, hipMemcpyHostToDevice, st));      // a copy node in the graph
        }
        *d_out = dtab;
        return IAF_OK;
    }
    if (changed || !t->uploaded) {
        const int slot = t->ring_i;
        t->ring_i = (t->ring_i + 1) % PREP_RING;
        if (t->pending[slot]) { HIP_TRY(hipEventSynchronize(t->ev[slot])); t->pending[slot] = false; }
        char* snap = t->h_ring + stride * slot;
        memcpy(snap, host, t->bytes);
        HIP_TRY(hipMemcpyAsync(t->d_tabs, snap, t->bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(t->ev[slot], st));
        t->pending[slot] = true;
        t->uploaded = true;
    }
    *d_out = t->d_tabs;
    return IAF_OK;
}

// ---- the tables of a batched launch (iaf_prep_batch, iaf_wn_bwd_batch and their iaf_conv3x3_* twins): one descriptor of type D per
// object, the launch's tile -> descriptor map and, for the weight-norm batches, every descriptor's first tile on the device too.
template <class D> struct BatchTable {
    int n = 0, ntiles = 0;
    D* h = nullptr;                // the current descriptors (host; a run changes them through set())
    std::vector<int> begin;        // [n + 1]: first tile of descriptor i
    bool dirty = false;            // h differs from what upload() last carried
    DescTable tab{};               // its way to the device
    int* d_tile2layer = nullptr;
    int* d_tile_begin = nullptr;   // begin[] on the device (with_begin)
    // tiles[i]: workgroups of descriptor i.  On an error the owner's destroy() frees what was made.
    int create(const std::vector<int>& tiles, bool with_begin) {
        n = (int)tiles.size();
        begin.assign(n + 1, 0);
        std::vector<int> t2l;
        for (int i = 0; i < n; ++i) { begin[i + 1] = begin[i] + tiles[i]; t2l.insert(t2l.end(), tiles[i], i); }
        ntiles = begin[n];
        if (!(h = (D*)calloc(n, sizeof(D)))) return (int)hipErrorOutOfMemory;
        if (int rc = desc_init(&tab, sizeof(D) * n)) return rc;
        HIP_TRY(hipMalloc((void**)&d_tile2layer, sizeof(int) * ntiles));
        HIP_TRY(hipMemcpy(d_tile2layer, t2l.data(), sizeof(int) * ntiles, hipMemcpyHostToDevice));
        if (!with_begin) return IAF_OK;
        HIP_TRY(hipMalloc((void**)&d_tile_begin, sizeof(int) * (n + 1)));
        return (int)hipMemcpy(d_tile_begin, begin.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice);
    }
    void destroy() {
        free(h);
        desc_destroy(&tab);
        if (d_tile2layer) (void)hipFree(d_tile2layer);
        if (d_tile_begin) (void)hipFree(d_tile_begin);
    }
    // this run's descriptor i: build the new one from the old (fill sets what a run decides), compare, assign
    template <class F> void set(int i, F fill) {
        D nw;
        memcpy(&nw, &h[i], sizeof(D));
        fill(nw);
        if (!memcmp(&nw, &h[i], sizeof(D))) return;
        memcpy(&h[i], &nw, sizeof(D));
        dirty = true;
    }
    // the table only travels when a descriptor changed (a training loop passes the same buffers every step)
    int upload(hipStream_t st, const D** d_out) {
        const void* d = nullptr;
        if (int rc = desc_upload(&tab, h, dirty, st, &d)) return rc;
        dirty = false;
        *d_out = (const D*)d;
        return IAF_OK;
    }
};

// ---- what a GemmLayer owns ----------------------------------------------------------------------------------------------------------
// bytes of its packs (taps: NTAPS masked, MAXTAPS plain): the fp32 fragments (forward and transposed: the same count); `planes` bf16 (3) or
// fp16 (2) planes of the forward problem (c_in % 32 == 0) and of the transposed one (even co tile counts)
static size_t pack_bytes_f32(const GemmLayer& L, int taps) { return (size_t)L.nchunk * taps * L.ncot * 256 * sizeof(float); }
static size_t pack_bytes_split(const GemmLayer& L, int taps, int planes) { return (size_t)(L.cin / 32) * taps * L.ncot * planes * 1024; }
static size_t pack_bytes_split_t(const GemmLayer& L, int taps, int planes) { return (size_t)(L.ncot / 2) * taps * L.nchunk * planes * 1024; }
static void gemm_layer_free(GemmLayer& L) {
    void* const own[] = {L.wp, L.bias, L.border, L.wpt, L.wpt3, L.wp3, L.wp2, L.wpt2, L.lim};
    for (void* q : own)
        if (q) (void)hipFree(q);
}
// training: the transposed packs of forward layer L (the next prepare writes them; f16: also as two fp16 planes, iaf_conv_bf3.hpp DG16)
// and T, the transposed problem dX = W^T dY, which runs the bf16x3 kernel where its launch-shape rule takes it
static int gemm_layer_set_training(GemmLayer& L, GemmLayer& T, int taps, bool f16) {
    if (!L.wpt) HIP_TRY(hipMalloc(&L.wpt, pack_bytes_f32(L, taps)));
    if (!L.wpt3 && L.ncot % 2 == 0) HIP_TRY(hipMalloc(&L.wpt3, pack_bytes_split_t(L, taps, 3)));
    if (f16 && L.wpt3 && !L.wpt2) HIP_TRY(hipMalloc(&L.wpt2, pack_bytes_split_t(L, taps, 2)));
    T = GemmLayer();
    T.cin = L.cout; T.cout = L.cin; T.nchunk = L.ncot; T.ncot = L.nchunk; T.zerodiag = L.zerodiag; T.npair = 1; T.full3x3 = L.full3x3;
    T.wp = L.wpt; T.wp3 = L.wpt3; T.wp2 = L.wpt2; T.nt = 1; T.pxt = 4; T.wco = 1; T.ks = 1;
    T.dbg = L.dbg; T.dbg_bytes = L.dbg_bytes;
    return IAF_OK;
}
// a prep descriptor's geometry, and the packs the launch writes (which: pack_prep_writes, iaf_pack_state.hpp)
static void prep_layer_geometry(PrepLayer& P, const GemmLayer& L, int tile_begin) {
    P.bias = L.bias; P.border = L.border;
    P.cin = L.cin; P.cout_each = L.cout / L.npair; P.ncot = L.ncot; P.nchunk = L.nchunk;
    P.zerodiag = L.zerodiag; P.npair = L.npair; P.tile_begin = tile_begin;
}
static void prep_layer_packs(PrepLayer& P, const GemmLayer& L, PackWrites w, unsigned* rng) {
    P.wp = w.wp ? L.wp : nullptr; P.wp3 = w.wp3 ? L.wp3 : nullptr; P.wpt = w.wpt ? L.wpt : nullptr;
    P.wp2 = w.wp2 ? L.wp2 : nullptr; P.rng_err = w.wp2 ? rng : nullptr;
}

// The compiled launch shapes (iaf_variants.def), one translation unit each: a table per family of {shape, picker}, in search order.
// exact-fp32 masked / plain conv (iaf_conv_inst.hip)
#define IAF_CONV(P, W, K) extern "C" conv_fn_t iaf_pick_conv_##P##_##W##_##K(int nt, int inmode, int epi);
// bf16x3 masked conv (iaf_conv_bf3_inst.hip)
#define IAF_BF3(P, X, K, C) extern "C" conv_fn_t iaf_pick_bf3_##P##_##X##_##K##_##C(int nt, int inmode, int epi);
// 9-tap plain conv on the matrix cores (iaf_conv_bf3_plain_inst.hip): form = BF3P_*
#define IAF_BF3P(P, X, K, C, S2) extern "C" conv_fn_t iaf_pick_bf3p_##P##_##X##_##K##_##C(int nt, int form);
#include "iaf_variants.def"

static const struct { int pxt, wco, ks; conv_fn_t (*pick)(int, int, int); } k_conv_shapes[] = {
#define IAF_CONV(P, W, K) {P, W, K, iaf_pick_conv_##P##_##W##_##K},
#include "iaf_variants.def"
};
static const struct { int ppw, pxt, ks, wco; conv_fn_t (*pick)(int, int, int); } k_bf3_shapes[] = {
#define IAF_BF3(P, X, K, C) {P, X, K, C, iaf_pick_bf3_##P##_##X##_##K##_##C},
#include "iaf_variants.def"
};
static const struct { int ppw, pxt, ks, wco; conv_fn_t (*pick)(int, int); } k_bf3p_shapes[] = {
#define IAF_BF3P(P, X, K, C, S2) {P, X, K, C, iaf_pick_bf3p_##P##_##X##_##K##_##C},
#include "iaf_variants.def"
};

static conv_fn_t pick_kernel(int nt, int pxt, int wco, int ks, int inmode, int epi) {
    if (nt < 1 || nt > 5) return nullptr;
    for (const auto& sh : k_conv_shapes)
        if (sh.pxt == pxt && sh.wco == wco && sh.ks == ks) return sh.pick(nt, inmode, epi);
    return nullptr;
}
static conv_fn_t pick_bf3(int nt, int ppw, int pxt, int ks, int inmode, int epi, int wco = 1) {
    for (const auto& sh : k_bf3_shapes)
        if (sh.ppw == ppw && sh.pxt == pxt && sh.ks == ks && sh.wco == wco) return sh.pick(nt, inmode, epi);
    return nullptr;
}
static conv_fn_t pick_bf3p(int nt, int ppw, int pxt, int ks, int wco, int form) {
    for (const auto& sh : k_bf3p_shapes)
        if (sh.ppw == ppw && sh.pxt == pxt && sh.ks == ks && sh.wco == wco) return sh.pick(nt, form);
    return nullptr;
}

// The one-launch step kernel for a key (iaf_step_fused_types.hpp): every part of iaf_variants.def is asked; at most one answers.
static step_fn_t (*const k_step_parts[])(const StepKey&, size_t*, size_t*) = {
#define IAF_STEP_PART(part) iaf_pick_step_part_##part,
#include "iaf_variants.def"
};
static step_fn_t pick_step(const StepKey& k, size_t* lds, size_t* row) {
    for (auto part : k_step_parts)
        if (step_fn_t f = part(k, lds, row)) return f;
    return nullptr;
}
// the statement of the operator as the step kernels' var
static int step_var(const iaf_stack_t* s) { return s->variant == IAF_VARIANT_TF ? 0 : s->variant == IAF_VARIANT_THEANO ? 1 : 2; }
static StepKey step_key(const iaf_stack_t* s, int W, int R, int form, int planes = STEP_BF16X3) {
    return StepKey{s->n_h / 16, s->n_z / 16, s->depth_ar, W, R, step_var(s), form, planes};
}

static size_t bf3_lds_bytes(int cin, int W, int nt, int ppw, int pxt, int ks, int wco = 1) {
    const size_t tile = (size_t)(16 * ppw * pxt + W + 1 + 1) * (3 * (cin / 8) + 2) * 16;
    const size_t red = ks > 1 ? (size_t)pxt * wco * ks * ppw * nt * 1024 : 0;     // split-K exchange aliases the (dead) tile
    return tile > red ? tile : red;
}
// LDS of a 9-tap bf16x3 launch: the pixel tile with a halo of W + 1 slots on BOTH sides (+ the zero slot)
static size_t bf3_plain_lds_bytes(int cin, int W, int nt, int ppw, int pxt, int ks, int wco, int npl = 3) {
    const size_t tile = (size_t)(16 * ppw * pxt + 2 * (W + 1) + 1) * (npl * (cin / 8) + 2) * 16;
    const size_t red = ks > 1 ? (size_t)pxt * wco * ks * ppw * nt * 1024 : 0;
    return tile > red ? tile : red;
}

static size_t conv_lds_bytes(const GemmLayer& L, int W) {
    const int tm = 16 * L.pxt, nslot = tm + (L.full3x3 ? 2 : 1) * (W + 1), cp = L.cin + 8;
    size_t fl = (size_t)(nslot + 1) * cp;
    size_t wbuf = 0, red = 0;
#if defined(IAF_SHARED_W) && IAF_SHARED_W
    if (L.pxt > 1) wbuf = (size_t)L.wco * L.ks * 2 * NTAPS * L.nt * 256;   // shared weights: 2 chunk buffers per wave group
#endif
    if (L.ks > 1) red = (size_t)L.ks * L.pxt * L.wco * L.nt * 256;          // split-K exchange (aliases the weight buffers)
    fl += wbuf > red ? wbuf : red;
    return fl * sizeof(float);
}

static void default_tuning(GemmLayer& L, bool is_out) {
    if (is_out) {
        L.nt = 2; L.pxt = 2; L.wco = (L.ncot >= 4 && (L.ncot / 2) % 2 == 0) ? 2 : 1; L.ks = (L.wco == 2) ? 1 : 2;
        return;
    }
    int nt = 1;
    for (int c = 5; c >= 1; --c)
        if (L.ncot % c == 0) { nt = c; break; }
    L.nt = nt; L.pxt = 4; L.wco = 1; L.ks = 1;
}

extern "C" int iaf_abi_version(void) { return IAF_ABI_VERSION; }
extern "C" const char* iaf_comm_error_string_(int code);       // iaf_comm.cpp

extern "C" const char* iaf_error_string(int code) {
    switch (code) {
        case IAF_OK: return "ok";
        case IAF_ERR_NULL: return "null pointer argument";
        case IAF_ERR_SHAPE: return "bad shape";
        case IAF_ERR_NOT_MULTIPLE: return "n_h must be a multiple of n_z or vice versa";
        case IAF_ERR_NOT_PREPARED: return "iaf_stack_prepare has not been called";
        case IAF_ERR_WORKSPACE: return "workspace too small or misaligned";
        case IAF_ERR_RANGE: return "an operand beyond fp16's largest finite number (65504) went into the two-plane fp16 kernels in an earlier launch of this stack (its outputs carry inf / NaN); the stack now runs the bf16x3 kernels -- prepare again if asked to, and repeat the call";
        case IAF_ERR_EXCHANGE: return "a bounded wait of the halo exchange gave up in an earlier launch of this stack (its outputs carry NaN); the stack now recomputes its halo rows -- repeat the call";
        case IAF_ERR_CAPTURE_SLOTS: return "this prep / weight-norm batch object has been captured into hipGraphs with more than 16 distinct sets of tensor pointers: create another batch object (include/iaf_hip.h)";
        case IAF_ERR_UNSUPPORTED: return "not covered by the gfx950 kernels (channels must be multiples of 16 and <= 256; launch shape must fit 160 KiB of LDS)";
    }
    if (code >= 10000) {                                  // 10000 + ncclResult_t (iaf_comm.cpp)
        const char* m = iaf_comm_error_string_(code);
        return m ? m : "RCCL error";
    }
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "unknown error";
}

extern "C" int iaf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

static void count_macs(GemmLayer& L, int n_in, int n_out_each, int zerodiag, int npair) {
    double centre = 0;
    for (int i = 0; i < n_in; ++i)
        for (int o = 0; o < n_out_each; ++o) centre += made_live(i, o, n_in, n_out_each, zerodiag) ? 1 : 0;
    L.live_macs_per_px = npair * (4.0 * n_in * n_out_each + centre);
    L.dense_macs_per_px = npair * 9.0 * n_in * n_out_each;
}

extern "C" int iaf_stack_create(iaf_stack_t** out, int n_z, int n_h, int depth_ar, int variant) {
    if (!out) return IAF_ERR_NULL;
    *out = nullptr;
    if (n_z <= 0 || n_h <= 0 || depth_ar < 0 || depth_ar > MAX_GEMM_LAYERS - 1) return IAF_ERR_SHAPE;
    if (variant != IAF_VARIANT_TF && variant != IAF_VARIANT_THEANO && variant != IAF_VARIANT_THEANO_FLIPMASK) return IAF_ERR_UNSUPPORTED;
    if (depth_ar > 0 && !(n_z % n_h == 0 || n_h % n_z == 0)) return IAF_ERR_NOT_MULTIPLE;   // layers.py:116
    const bool generic = (n_z % 16 != 0 || (depth_ar > 0 && n_h % 16 != 0) || n_z > 16 * PREP_MAXI ||
                          (depth_ar > 0 && n_h > 16 * PREP_MAXI));
    if (generic && variant != IAF_VARIANT_TF) return IAF_ERR_UNSUPPORTED;
    iaf_stack* s = new (std::nothrow) iaf_stack();
    if (!s) return (int)hipErrorOutOfMemory;
    s->generic = generic;
    // IAF_XCH_DEBUG=<bits>: every stack starts with these iaf_stack_set_halo_exchange_debug bits (1 = scrambled work lists, 2 = random
    // delays, 16 = free-bits finish as its own launch) -- how the whole GPU suite is run under a scrambled hand-over order
    // (32 = the pair form at 8-pixel rows: the whole suite through it)
    if (const char* e = getenv("IAF_XCH_DEBUG")) s->xch_knob = (unsigned)atoi(e) & (1u | 2u | 16u | 32u);
    s->n_z = n_z; s->n_h = n_h; s->depth_ar = depth_ar; s->variant = variant;
    s->nlayers = depth_ar + 1;
    s->prepared = false;
    s->weight_bytes = 0;
    int cin = n_z;
    for (int l = 0; l < s->nlayers; ++l) {
        GemmLayer& L = s->L[l];
        const bool is_out = (l == depth_ar);
        const int each = is_out ? n_z : n_h;
        L.cin = cin;
        L.npair = is_out ? 2 : 1;
        L.cout = each * L.npair;
        L.zerodiag = is_out ? 1 : 0;          // layers.py:162 (False) / 166 (True)
        L.nchunk = (cin + 15) / 16;
        L.ncot = (L.cout + 15) / 16;
        default_tuning(L, is_out);
        count_macs(L, cin, each, L.zerodiag, L.npair);
        s->weight_bytes += (size_t)L.npair * (9 * (size_t)(cin + (variant != IAF_VARIANT_TF ? 1 : 0)) * each + 2 * (size_t)each) * sizeof(float);
        int rc;
        if ((rc = (int)hipMalloc(&L.wp, generic ? (size_t)NTAPS * cin * L.cout * sizeof(float) : pack_bytes_f32(L, NTAPS))) != 0 ||
            (rc = (int)hipMalloc(&L.bias, (size_t)L.cout * sizeof(float))) != 0 ||
            (variant != IAF_VARIANT_TF && (rc = (int)hipMalloc(&L.border, (size_t)4 * L.cout * sizeof(float))) != 0) ||
            (rc = (int)hipMalloc(&L.lim, (size_t)L.ncot * sizeof(int))) != 0 ||
            (!generic && cin % 32 == 0 && (rc = (int)hipMalloc(&L.wp3, pack_bytes_split(L, NTAPS, 3))) != 0)) {
            iaf_stack_destroy(s);
            return rc;
        }
        // live-chunk limit of the centre tap per packed co-tile (the mask is monotone in c_in)
        int limh[1024];
        for (int gt = 0; gt < L.ncot && !generic; ++gt) {
            const int src = is_out ? (gt >> 1) : gt;
            int maxci = -1;
            for (int oo = 0; oo < 16; ++oo)
                for (int i = 0; i < cin; ++i)
                    if (made_live(i, src * 16 + oo, cin, each, L.zerodiag) && i > maxci) maxci = i;
            limh[gt] = (maxci + 16) / 16;    // ceil((maxci+1)/16); 0 if nothing live
        }
        if (!generic && (rc = (int)hipMemcpy(L.lim, limh, L.ncot * sizeof(int), hipMemcpyHostToDevice)) != 0) {
            iaf_stack_destroy(s);
            return rc;
        }
        cin = each;
    }
    // Default arithmetic (round 6): where the two-plane fp16 step kernels are compiled for the stack -- TF statement, (n_z, n_h, depth_ar) =
    // (32, 160, 2): the BASELINE run -- a new stack asks for them (IAF_PRECISION_F16X2: bf16x3 everywhere else, and after a range
    // failure); IAF_DEFAULT_PRECISION=bf16x3 keeps round 5's default.
    if (!generic && variant == IAF_VARIANT_TF) {
        static const bool f16_default = !(getenv("IAF_DEFAULT_PRECISION") && !strcmp(getenv("IAF_DEFAULT_PRECISION"), "bf16x3"));
        size_t l16 = 0, x16 = 0;
        if (f16_default && (pick_step(step_key(s, 16, 2, STEP_XCH, STEP_F16X2), &l16, &x16) ||
                            pick_step(step_key(s, 8, 1, STEP_HELPERS, STEP_F16X2), &l16, &x16))) {
            int rc = iaf_stack_set_precision(s, IAF_PRECISION_F16X2);
            if (rc != IAF_OK && rc != IAF_ERR_UNSUPPORTED) { iaf_stack_destroy(s); return rc; }
        }
    }
    *out = s;
    return IAF_OK;
}

// The masked ResNet of the reference's deep IAF (graphy/nodes/ar.py:428-448, 478-528; models.py 'down_iaf2_deep'): the same object with
// 2 depth + 1 hidden convs and the residual launch sequence (run_resnet, iaf_step_forward_train, iaf_step_backward).
extern "C" int iaf_stack_create_resnet(iaf_stack_t** out, int n_z, int n_h, int depth, int variant) {
    if (!out) return IAF_ERR_NULL;
    *out = nullptr;
    if (n_z <= 0 || n_h <= 0 || depth < 1 || 2 * depth + 2 > MAX_GEMM_LAYERS) return IAF_ERR_SHAPE;
    if (variant != IAF_VARIANT_THEANO) return IAF_ERR_UNSUPPORTED;     // (resnet_layer_a passes no flipmask, ar.py:434-435: only the plain ordering exists)
    if (!(n_z % n_h == 0 || n_h % n_z == 0)) return IAF_ERR_NOT_MULTIPLE;
    if (n_z % 16 != 0 || n_h % 16 != 0 || n_z > 16 * PREP_MAXI || n_h > 16 * PREP_MAXI) return IAF_ERR_UNSUPPORTED;
    iaf_stack_t* s = nullptr;
    if (int rc = iaf_stack_create(&s, n_z, n_h, 2 * depth + 1, variant)) return rc;
    s->resnet = depth;
    *out = s;
    return IAF_OK;
}

static void prof_free(iaf_stack* s) {
    for (int i = 0; i < s->prof_cap; ++i) {
        if (s->prof_start) (void)hipEventDestroy(s->prof_start[i]);
        if (s->prof_stop) (void)hipEventDestroy(s->prof_stop[i]);
    }
    free(s->prof_start); free(s->prof_stop);
    s->prof_start = s->prof_stop = nullptr;
    s->prof_cap = s->prof_n = 0; s->prof_layer = -1;
}

extern "C" int iaf_stack_set_debug(iaf_stack_t* s, int layer, void* buf) {
    if (!s) return IAF_ERR_NULL;
    s->dbg_layer = layer; s->dbg = (unsigned long long*)buf;
    return IAF_OK;
}

extern "C" int iaf_stack_profile_enable(iaf_stack_t* s, int layer, int max_samples) {
    if (!s) return IAF_ERR_NULL;
    prof_free(s);
    if (layer < 0 && layer != -2) return IAF_OK;       // -2: the one-launch step (iaf_step_fused.hpp)
    if (layer >= s->nlayers || max_samples <= 0 || max_samples > (1 << 20)) return IAF_ERR_SHAPE;
    s->prof_start = (hipEvent_t*)calloc(max_samples, sizeof(hipEvent_t));
    s->prof_stop = (hipEvent_t*)calloc(max_samples, sizeof(hipEvent_t));
    if (!s->prof_start || !s->prof_stop) { prof_free(s); return (int)hipErrorOutOfMemory; }
    for (int i = 0; i < max_samples; ++i) {
        HIP_TRY(hipEventCreate(&s->prof_start[i]));
        HIP_TRY(hipEventCreate(&s->prof_stop[i]));
        s->prof_cap = i + 1;
    }
    s->prof_layer = layer;
    return IAF_OK;
}

extern "C" int iaf_stack_profile_read(iaf_stack_t* s, float* ms_out, int capacity, int* n_out) {
    if (!s || !ms_out || !n_out) return IAF_ERR_NULL;
    int n = s->prof_n < capacity ? s->prof_n : capacity;
    for (int i = 0; i < n; ++i) {
        HIP_TRY(hipEventSynchronize(s->prof_stop[i]));
        HIP_TRY(hipEventElapsedTime(&ms_out[i], s->prof_start[i], s->prof_stop[i]));
    }
    *n_out = n;
    s->prof_n = 0;
    return IAF_OK;
}

static void xch_free_sets(iaf_stack_t* s) {
    for (auto& x : s->xch_sets) {
        if (x.buf) (void)hipFree(x.buf);
        if (x.ctl) (void)hipFree(x.ctl);
    }
    s->xch_sets.clear();
    for (auto& r : s->xch_retired_rows) (void)hipFree(r.first);
    s->xch_retired_rows.clear();
}

extern "C" int iaf_stack_destroy(iaf_stack_t* s) {
    if (!s) return IAF_ERR_NULL;
    prof_free(s);
    for (int l = 0; l < s->nlayers; ++l) gemm_layer_free(s->L[l]);
    xch_free_sets(s);
    if (s->xch_err_host) (void)hipHostFree(s->xch_err_host);
    s->rng.free();
    delete s;
    return IAF_OK;
}

// Back to a fresh start: the device is idle after the synchronisation, so the sets can simply be zeroed (epoch 0, no flags, no
// announcements, no sticky error) -- buffers a captured graph names stay where they are.
static int xch_reset_sets(iaf_stack_t* s) {
    HIP_TRY(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lk(s->xch_mu);
    for (auto& x : s->xch_sets) {
        HIP_TRY(hipMemsetD32((hipDeviceptr_t)x.buf, (int)x.pattern, x.bytes / 4));
        HIP_TRY(hipMemset(x.ctl, 0, IAF_XCTL_WORDS * sizeof(unsigned long long)));
    }
    for (auto& r : s->xch_retired_rows) HIP_TRY(hipMemsetD32((hipDeviceptr_t)r.first, (int)r.pattern, r.second / 4));     // (a captured graph may still name them)
    HIP_TRY(hipDeviceSynchronize());                         // (the fills ran on the null stream: a non-blocking stream's next launch is not ordered behind them)
    if (s->xch_err_host) *(volatile unsigned*)s->xch_err_host = 0u;
    return IAF_OK;
}

extern "C" int iaf_stack_set_halo_exchange(iaf_stack_t* s, int on) {
    if (!s) return IAF_ERR_NULL;
    if (s->resnet) return IAF_ERR_UNSUPPORTED;      // (iaf_stack_create_resnet: include/iaf_hip.h)
    s->xch_on = on != 0;
    return xch_reset_sets(s);                                // a fresh start either way: error words cleared
}

extern "C" int iaf_stack_set_free_bits_groups(iaf_stack_t* s, int groups) {
    if (!s) return IAF_ERR_NULL;
    if (groups < 1 || groups > IAF_MAX_FREE_BITS_GROUPS) return IAF_ERR_SHAPE;
    if (groups > 1 && s->variant != IAF_VARIANT_TF) return IAF_ERR_UNSUPPORTED;      // (the Theano objective is one scalar per layer, models.py:458-461)
    s->fb_groups = groups;
    return IAF_OK;
}
extern "C" int iaf_stack_get_free_bits_groups(const iaf_stack_t* s, int* groups) {
    if (!s || !groups) return IAF_ERR_NULL;
    *groups = s->fb_groups;
    return IAF_OK;
}

extern "C" int iaf_stack_set_halo_exchange_debug(iaf_stack_t* s, unsigned knobs) {
    if (!s) return IAF_ERR_NULL;
    if (s->resnet) return IAF_ERR_UNSUPPORTED;      // (iaf_stack_create_resnet: include/iaf_hip.h)
    s->xch_knob = knobs;
    return IAF_OK;
}

extern "C" int iaf_stack_exchange_errors(const iaf_stack_t* s, unsigned* errors) {
    if (!s || !errors) return IAF_ERR_NULL;
    *errors = 0;
    if (!s->xch_err_host) return IAF_OK;
    HIP_TRY(hipDeviceSynchronize());                         // (every launch so far has had its say)
    *errors = *(volatile unsigned*)s->xch_err_host;
    return IAF_OK;
}

extern "C" int iaf_stack_set_tuning(iaf_stack_t* s, int layer, int nt, int pxt, int wco, int ks) {
    if (!s) return IAF_ERR_NULL;
    if (layer < 0 || layer >= s->nlayers) return IAF_ERR_SHAPE;
    if (s->generic) return IAF_ERR_UNSUPPORTED;
    GemmLayer& L = s->L[layer];
    const bool is_out = (layer == s->depth_ar);
    if (nt < 1 || L.ncot % (nt * wco) != 0) return IAF_ERR_UNSUPPORTED;
    if (is_out && (nt % 2 != 0)) return IAF_ERR_UNSUPPORTED;
    if (!pick_kernel(nt, pxt, wco, ks, IN_PIXMAJOR, is_out ? EPI_OUT : EPI_HIDDEN)) return IAF_ERR_UNSUPPORTED;
    if (L.nchunk < ks) return IAF_ERR_UNSUPPORTED;
    L.nt = nt; L.pxt = pxt; L.wco = wco; L.ks = ks;
    L.user_tuned = true;
    return IAF_OK;
}

static bool bf3_select(const iaf_stack_t* s, GemmLayer& L, int epi, bool negate_taps, bool pix_input, long long P, int W);

// F32 or one of the two split arithmetics (F16X2 = BF16X3 everywhere but in the one-launch step kernels compiled with fp16 planes)
static inline bool prec_split(const iaf_stack_t* s) { return s->precision != IAF_PRECISION_F32; }
// the F16 step kernels are in use: the precision asks for them, every layer has the pack, no range failure has been seen
static inline bool f16_active(const iaf_stack_t* s) {
    if (!pack_f16_wanted(*s) || s->generic) return false;
    for (int l = 0; l < s->nlayers; ++l) if (!s->L[l].wp2) return false;
    return true;
}

extern "C" int iaf_stack_set_precision(iaf_stack_t* s, int precision) {
    if (!s) return IAF_ERR_NULL;
    if (precision != IAF_PRECISION_F32 && precision != IAF_PRECISION_BF16X3 && precision != IAF_PRECISION_F16X2) return IAF_ERR_SHAPE;
    bool new_pack = false;
    if (precision == IAF_PRECISION_F16X2) {
        if (s->generic || s->resnet) return IAF_ERR_UNSUPPORTED;      // (masked ResNet: no kernel of its launch sequence reads fp16 planes)
        for (int l = 0; l < s->nlayers; ++l) if (!s->L[l].wp3) return IAF_ERR_UNSUPPORTED;      // (c_in % 32: the same fragments, two planes)
        if (int rc = s->rng.alloc()) return rc;
        for (int l = 0; l < s->nlayers; ++l) {
            GemmLayer& L = s->L[l];
            if (L.wp2) continue;
            HIP_TRY(hipMalloc(&L.wp2, pack_bytes_split(L, NTAPS, 2)));
            new_pack = true;
        }
    }
    // (away from F16X2: the packs the other kernels read were written all along -- unless iaf_stack_set_packs dropped the bf16x3 one)
    return pack_set_precision(*s, PACK_STACK, precision, new_pack, s->rng.peek()) ? s->rng.rearm() : IAF_OK;
}

extern "C" int iaf_stack_range_errors(const iaf_stack_t* s, unsigned* errors) {
    if (!s || !errors) return IAF_ERR_NULL;
    return s->rng.read(errors);
}

// which packs a prep launch writes for layer L of stack s
static inline void stack_prep_packs(const iaf_stack_t* s, const GemmLayer& L, PrepLayer& P) {
    prep_layer_packs(P, L, pack_prep_writes(*s, PACK_STACK, f16_active(s), L.wp3 != nullptr, s->training), s->rng.dev);
}

// the forward epilogue of layer l: the output pair; in a masked ResNet the input conv and every block's conv2 write the residual stream
static int layer_epi(const iaf_stack_t* s, int l) {
    return l == s->depth_ar ? EPI_OUT : (s->resnet && l % 2 == 0) ? EPI_RES : EPI_HIDDEN;
}

extern "C" int iaf_stack_get_precision(const iaf_stack_t* s, int layer, int B, int H, int W) {
    if (!s || layer < 0 || layer >= s->nlayers) return IAF_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0) return IAF_ERR_SHAPE;
    GemmLayer t = s->L[layer];
    const bool is_out = (layer == s->depth_ar);
    // what a forward launch of this layer at this size will run (same decision function as the launch)
    return bf3_select(s, t, layer_epi(s, layer), false, !(is_out && s->depth_ar == 0) && (layer > 0 || !is_out),
                      (long long)B * H * W, W) ? IAF_PRECISION_BF16X3 : IAF_PRECISION_F32;
}

// the epilogue of layer l's data gradient (iaf_step_backward's walk): layer 0 ends in dz; in a masked ResNet the output pair and every
// block's conv1 write the residual stream's gradient
static int layer_dgrad_epi(const iaf_stack_t* s, int l) {
    return (s->resnet && l > 0 && (l == s->depth_ar || (l & 1))) ? EPI_DGRAD_RES : EPI_DGRAD;
}

extern "C" int iaf_stack_get_dgrad_precision(const iaf_stack_t* s, int layer, int B, int H, int W) {
    if (!s || layer < 0 || layer >= s->nlayers) return IAF_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0) return IAF_ERR_SHAPE;
    if (!s->training || s->generic) return IAF_ERR_NOT_PREPARED;
    GemmLayer t = s->T[layer];
    // what iaf_step_backward's data-gradient launch of this layer at this size will run (same decision function as the launch)
    return bf3_select(s, t, layer_dgrad_epi(s, layer), true, true, (long long)B * H * W, W) ? IAF_PRECISION_BF16X3 : IAF_PRECISION_F32;
}

extern "C" int iaf_stack_set_tuning_bf3(iaf_stack_t* s, int layer, int nt, int ppw, int pxt, int ks, int wco) {
    if (!s) return IAF_ERR_NULL;
    if (layer < 0 || layer >= s->nlayers) return IAF_ERR_SHAPE;
    GemmLayer& L = s->L[layer];
    if (nt == 0) { L.b_user_tuned = false; return IAF_OK; }      // back to the automatic choice
    const bool is_out = (layer == s->depth_ar);
    if (!L.wp3 || L.ncot % nt != 0 || (is_out && (nt & 1))) return IAF_ERR_UNSUPPORTED;
    if (wco < 1) wco = 1;
    if (L.ncot % (nt * wco) != 0) return IAF_ERR_UNSUPPORTED;
    if (!pick_bf3(nt, ppw, pxt, ks, IN_PIXMAJOR, is_out ? EPI_OUT : EPI_HIDDEN, wco)) return IAF_ERR_UNSUPPORTED;
    L.b_nt = nt; L.b_ppw = ppw; L.b_pxt = pxt; L.b_ks = ks; L.b_wco = wco; L.b_user_tuned = true;
    return IAF_OK;
}

// transposed bf16x3 packs of training layers, PACKT3_MAX layers per launch (iaf_pack_t3_kernel)
struct PackT3Batch {
    PackT3Args a;
    hipStream_t st;
    explicit PackT3Batch(hipStream_t s) : st(s) { memset(&a, 0, sizeof(a)); }
    int flush() {
        if (!a.n) return IAF_OK;
        hipLaunchKernelGGL(iaf_pack_t3_kernel, dim3((a.total + 255) / 256), dim3(256), 0, st, a);
        memset(&a, 0, sizeof(a));
        return (int)hipGetLastError();
    }
    // L: the FORWARD layer (wpt / wpt3 written for its transposed problem); ntp: 5 masked / 9 plain taps
    int add(const GemmLayer& L, int ntp) {
        if (!L.wpt || !L.wpt3) return IAF_OK;
        if (a.n == PACKT3_MAX) { int rc = flush(); if (rc) return rc; }
        PackT3Layer& q = a.L[a.n++];
        q.src = L.wpt; q.dst = L.wpt3; q.dst2 = L.wpt2; q.ntp = ntp; q.nct = L.nchunk; q.begin = a.total;
        a.total += (L.ncot / 2) * ntp * L.nchunk * 64;
        return IAF_OK;
    }
};

// dynamic LDS of a masked-stack prep launch (prep_tile_fast, iaf_kernels_prep.hpp): the largest tile [5 taps x c_in rows + 1 pad row per 8][16]
// among the TF-statement layers that keep split packs only; 0 = no such layer (IAF_PREP_DBG bit 1: never).  Up to 160 KiB are allowed once.
static unsigned prep_fast_floats(const PrepLayer* P, int n) {
    static const bool off = getenv("IAF_PREP_DBG") && (atoi(getenv("IAF_PREP_DBG")) & 2);
    if (off) return 0;
    unsigned m = 0;
    for (int i = 0; i < n; ++i) {
        const bool tf = P[i].variant == IAF_VARIANT_TF, split_only = (P[i].wp3 || P[i].wp2) && !P[i].wp && !P[i].wpt;
        const unsigned f = (unsigned)NTAPS * (unsigned)P[i].cin * 18u;
        if (tf && split_only && P[i].nchunk % 2 == 0 && f * 4u <= 96u * 1024u && f > m) m = f;
    }
    static bool once = false;
    if (m && !once) {
        if (hipFuncSetAttribute((const void*)iaf_prep_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess ||
            hipFuncSetAttribute((const void*)iaf_prep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess) { (void)hipGetLastError(); return 0; }
        once = true;
    }
    return m;
}

extern "C" int iaf_stack_prepare(iaf_stack_t* s, const float* const* V, const float* const* g, const float* const* b,
                                 void* stream) {
    if (!s || !V || !g || !b) return IAF_ERR_NULL;
    const int nconv = s->depth_ar + 2;
    for (int i = 0; i < nconv; ++i)
        if (!V[i] || !g[i] || !b[i]) return IAF_ERR_NULL;
    if (s->generic) {
        GenPrepArgs ga;
        memset(&ga, 0, sizeof(ga));
        ga.nlayers = s->nlayers;
        int ch = 0;
        for (int l = 0; l < s->nlayers; ++l) {
            const GemmLayer& L = s->L[l];
            GenPrepLayer& P = ga.L[l];
            P.V[0] = V[l]; P.g[0] = g[l]; P.b[0] = b[l];
            if (L.npair == 2) { P.V[1] = V[l + 1]; P.g[1] = g[l + 1]; P.b[1] = b[l + 1]; }
            P.w = L.wp; P.bias = L.bias; P.cin = L.cin; P.cout_each = L.cout / L.npair; P.npair = L.npair;
            P.zerodiag = L.zerodiag; P.ch_begin = ch;
            ch += L.cout;
        }
        hipLaunchKernelGGL(iaf_generic_prep_kernel, dim3(ch), dim3(256), 0, (hipStream_t)stream, ga);
        HIP_TRY(hipGetLastError());
        s->prepared = true;
        return IAF_OK;
    }
    PrepArgs a;
    memset(&a, 0, sizeof(a));
    a.nlayers = s->nlayers;
    int tiles = 0;
    for (int l = 0; l < s->nlayers; ++l) {
        const GemmLayer& L = s->L[l];
        PrepLayer& P = a.L[l];
        P.V[0] = V[l]; P.g[0] = g[l]; P.b[0] = b[l];
        if (L.npair == 2) { P.V[1] = V[l + 1]; P.g[1] = g[l + 1]; P.b[1] = b[l + 1]; }
        stack_prep_packs(s, L, P);
        prep_layer_geometry(P, L, tiles);
        P.variant = s->variant;
        tiles += L.ncot;
    }
    const unsigned ff = prep_fast_floats(a.L, a.nlayers);
    hipLaunchKernelGGL(iaf_prep_kernel, dim3(tiles), dim3(256), (size_t)ff * 4, (hipStream_t)stream, a, ff);
    HIP_TRY(hipGetLastError());
    if (s->training) {
        PackT3Batch tb((hipStream_t)stream);
        for (int l = 0; l < s->nlayers; ++l) { int rc = tb.add(s->L[l], NTAPS); if (rc) return rc; }
        int rc = tb.flush();
        if (rc) return rc;
    }
    s->prepared = true;
    return IAF_OK;
}

// ---- batched prepare: all stacks of a model in ONE launch (weights of every layer are known at step start)
struct iaf_prep_batch {
    std::vector<iaf_stack*> stacks;
    BatchTable<PrepLayer> t;       // one descriptor per layer of every stack
};

extern "C" int iaf_prep_batch_destroy(iaf_prep_batch_t* b) {
    if (!b) return IAF_ERR_NULL;
    b->t.destroy();
    delete b;
    return IAF_OK;
}

extern "C" int iaf_prep_batch_create(iaf_prep_batch_t** out, iaf_stack_t* const* stacks, int n) {
    if (!out || !stacks) return IAF_ERR_NULL;
    *out = nullptr;
    if (n <= 0) return IAF_ERR_SHAPE;
    std::vector<int> tiles;
    for (int i = 0; i < n; ++i) {
        if (!stacks[i]) return IAF_ERR_NULL;
        if (stacks[i]->generic) return IAF_ERR_UNSUPPORTED;
        for (int l = 0; l < stacks[i]->nlayers; ++l) tiles.push_back(stacks[i]->L[l].ncot);
    }
    iaf_prep_batch* b = new (std::nothrow) iaf_prep_batch();
    if (!b) return (int)hipErrorOutOfMemory;
    b->stacks.assign(stacks, stacks + n);
    if (int rc = b->t.create(tiles, false)) { iaf_prep_batch_destroy(b); return rc; }
    int li = 0;
    for (iaf_stack* s : b->stacks)
        for (int l = 0; l < s->nlayers; ++l, ++li) {
            PrepLayer& P = b->t.h[li];
            stack_prep_packs(s, s->L[l], P);
            prep_layer_geometry(P, s->L[l], b->t.begin[li]);
            P.variant = s->variant;
        }
    *out = b;
    return IAF_OK;
}

extern "C" int iaf_prep_batch_run(iaf_prep_batch_t* b, const float* const* V, const float* const* g,
                                  const float* const* bias, void* stream) {
    if (!b || !V || !g || !bias) return IAF_ERR_NULL;
    int li = 0, ci = 0;   // ci: running conv index over all stacks (depth_ar + 2 convs per stack)
    for (const iaf_stack* s : b->stacks) {
        for (int l = 0; l < s->nlayers; ++l, ++li) {
            const GemmLayer& L = s->L[l];
            const float* const* Vl = V + ci + l; const float* const* gl = g + ci + l; const float* const* bl = bias + ci + l;
            for (int e = 0; e < L.npair; ++e)
                if (!Vl[e] || !gl[e] || !bl[e]) return IAF_ERR_NULL;
            b->t.set(li, [&](PrepLayer& P) {
                for (int e = 0; e < L.npair; ++e) { P.V[e] = Vl[e]; P.g[e] = gl[e]; P.b[e] = bl[e]; }
                stack_prep_packs(s, L, P);     // iaf_stack_set_packs / _set_precision / _set_training / a range failure since the last run
            });
        }
        ci += s->depth_ar + 2;
    }
    hipStream_t st = (hipStream_t)stream;
    const PrepLayer* d_layers = nullptr;
    if (int rc = b->t.upload(st, &d_layers)) return rc;
    // (IAF_PREP_DBG, dev knob: bit 0 = tiles in blockIdx order instead of paired per XCD, bit 1 = round 5's tile function; same box, 20 stacks,
    //  fp16 packs: 13.4 us with both bits, 12.1 us with neither -- profiles/r06/experiments/prep_time_ab_same_box.txt)
    static const int prep_dbg = getenv("IAF_PREP_DBG") ? atoi(getenv("IAF_PREP_DBG")) : 0;
    const int xcdpair = (prep_dbg & 1) ? 0 : 1;
    const unsigned ff = prep_fast_floats(b->t.h, b->t.n);
    hipLaunchKernelGGL(iaf_prep_batch_kernel, dim3(xcdpair ? (b->t.ntiles + 15) / 16 * 16 : b->t.ntiles), dim3(256), (size_t)ff * 4, st, d_layers,
                       b->t.d_tile2layer, b->t.ntiles, xcdpair, ff);
    HIP_TRY(hipGetLastError());
    {
        PackT3Batch tb(st);
        for (const iaf_stack* s : b->stacks)
            if (s->training)
                for (int l = 0; l < s->nlayers; ++l) { int rc = tb.add(s->L[l], NTAPS); if (rc) return rc; }
        int rc = tb.flush();
        if (rc) return rc;
    }
    for (iaf_stack* s : b->stacks) s->prepared = true;
    return IAF_OK;
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

extern "C" size_t iaf_stack_workspace_bytes(const iaf_stack_t* s, int B, int H, int W) {
    if (!s || B <= 0 || H <= 0 || W <= 0) return 0;
    const size_t P = (size_t)B * H * W;
    // two ping-pong hidden buffers [P][n_h], kl elements [B,n_z,H,W], row sums [B*n_z]
    size_t bytes = 0;
    if (s->depth_ar > 0) bytes += (s->resnet ? 3 : 2) * align_up(P * s->n_h * sizeof(float), 256);      // (masked ResNet: raw stream, elu(stream), t_i)
    bytes += align_up(P * s->n_z * sizeof(float), 256);
    bytes += align_up((size_t)B * s->n_z * sizeof(float), 256);
    return bytes;
}

struct Ws {
    float* hbuf[3];       // [2]: masked ResNet only
    float* kl_elem;
    float* rowsum;
};

static int carve_ws(const iaf_stack_t* s, int B, int H, int W, void* ws, size_t ws_bytes, Ws* o) {
    if (!ws) return IAF_ERR_NULL;
    if (((uintptr_t)ws & 15) != 0 || ws_bytes < iaf_stack_workspace_bytes(s, B, H, W)) return IAF_ERR_WORKSPACE;
    const size_t P = (size_t)B * H * W;
    char* p = (char*)ws;
    o->hbuf[0] = o->hbuf[1] = o->hbuf[2] = nullptr;
    if (s->depth_ar > 0) {
        o->hbuf[0] = (float*)p; p += align_up(P * s->n_h * sizeof(float), 256);
        o->hbuf[1] = (float*)p; p += align_up(P * s->n_h * sizeof(float), 256);
        if (s->resnet) { o->hbuf[2] = (float*)p; p += align_up(P * s->n_h * sizeof(float), 256); }
    }
    o->kl_elem = (float*)p; p += align_up(P * s->n_z * sizeof(float), 256);
    o->rowsum = (float*)p;
    return IAF_OK;
}

// Launch-shape model.  At the BASELINE batch sizes the convs are latency-bound (a few thousand pixels for
// 256 CUs), so the shape is chosen to minimise the longest per-SIMD MFMA chain:
//   cycles(wave) = (5*nchunk/ks) steps * nt tiles * 4 MFMA * 32 cycles;  waves sharing a SIMD serialise;
//   T = rounds over the 256 CUs * (cycles(WG) + fixed prologue/epilogue cost).
// Ties go to fewer rounds, then less split-K, then bigger tiles (more operand reuse), then the earlier shape of k_conv_shapes.
static void auto_shape(GemmLayer& L, bool is_out, long long P, int W) {
    double best = 1e30;
    int bnt = 0, bs = -1;
    for (int si = 0; si < (int)std::size(k_conv_shapes); ++si) {
        const int pxt = k_conv_shapes[si].pxt, wco = k_conv_shapes[si].wco, ks = k_conv_shapes[si].ks;
        if (L.nchunk < ks) continue;
        for (int nt = 5; nt >= 1; --nt) {
            if (is_out && (nt & 1)) continue;
            if (L.ncot % (nt * wco) != 0) continue;
            GemmLayer t = L;
            t.nt = nt; t.pxt = pxt; t.wco = wco; t.ks = ks;
            if (conv_lds_bytes(t, W) > 160 * 1024) continue;
            const double wgs = (double)((P + 16 * pxt - 1) / (16 * pxt)) * (L.ncot / (nt * wco));
            const double rounds = ceil(wgs / 256.0);
            const double cyc_wave = ((L.full3x3 ? 9.0 : 5.0) * L.nchunk / ks) * nt * 128.0;
            const double waves = pxt * wco * ks;
            const double cyc_wg = cyc_wave * ceil(waves / 4.0);
            const double T = rounds * (cyc_wg + 6000.0) + 400.0 * (ks - 1) + 1e-3 * si - 1e-2 * nt;
            if (T < best) { best = T; bnt = nt; bs = si; }
        }
    }
    if (bs >= 0) { L.nt = bnt; L.pxt = k_conv_shapes[bs].pxt; L.wco = k_conv_shapes[bs].wco; L.ks = k_conv_shapes[bs].ks; }
}

// raise the dynamic-LDS cap once per kernel (never inside a stream capture: warm up first)
static int raise_lds_cap(const void* fn, size_t lds) {
    if (lds <= 48 * 1024) return 0;
    static std::mutex mu;
    static std::unordered_set<const void*> done;
    std::lock_guard<std::mutex> lk(mu);
    if (!done.count(fn)) {
        // (a kernel with static LDS of its own -- the fp16-plane data gradient's 32 bytes -- may ask for 160 KiB less that much)
        hipFuncAttributes fa;
        HIP_TRY(hipFuncGetAttributes(&fa, fn));
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - (int)fa.sharedSizeBytes));
        done.insert(fn);
    }
    return 0;
}

// IN_FUSED0 adds the double-halo z tile behind the hidden tile
static size_t bf3_fused_lds_bytes(int cin, int cin0, int W, int nt, int ppw, int pxt, int ks, int wco) {
    const int nslot = 16 * ppw * pxt + W + 1;
    const size_t tile = (size_t)(nslot + 1) * (3 * (cin / 8) + 2) * 16 + (size_t)(nslot + W + 1 + 1) * (3 * (cin0 / 8) + 2) * 16;
    const size_t red = ks > 1 ? (size_t)pxt * wco * ks * ppw * nt * 1024 : 0;
    return tile > red ? tile : red;
}
// can layer 0 be computed inside layer 1's bf16x3 kernel with this shape?
static bool fuse_shape_ok(const iaf_stack_t* s, int nt, int ppw, int pxt, int ks, int wco, int W) {
    if (s->depth_ar < 1 || s->variant != IAF_VARIANT_TF || s->generic || !prec_split(s) || !(s->packs & IAF_PACK_BF16X3)) return false;
    const GemmLayer& A = s->L[0];
    const GemmLayer& Bl = s->L[1];
    if (!A.wp3 || !Bl.wp3 || A.cin != 32) return false;
    const int epi = (s->depth_ar == 1) ? EPI_OUT : EPI_HIDDEN;
    if (Bl.ncot % (nt * wco) != 0 || (epi == EPI_OUT && (nt & 1))) return false;
    if (!pick_bf3(nt, ppw, pxt, ks, IN_FUSED0, epi, wco)) return false;
    const int nw = pxt * wco * ks, ntl = nw >= 8 ? 2 : 3;
    if (A.ncot > nw * ntl) return false;
    return bf3_fused_lds_bytes(Bl.cin, A.cin, W, nt, ppw, pxt, ks, wco) <= 160 * 1024;
}

// bf16x3 launch shape without a timing run (iaf_stack_autotune measures instead).  What the sweeps on one MI355X show
// (tools/bf3_sweep.py, profiles/r02/bf3_sweep_*.txt): below ~4096 pixels a conv launch is all prologue / exchange /
// epilogue latency and the exact-fp32 kernel is as fast or faster -> not selected; above, K-slicing over 4 waves with two
// pixel tiles per wave wins (two workgroups share a CU and overlap each other's phases), except for a single c_in pair
// (c_in = 32: 5 steps), where four waves along pixels without K-slicing do.
static bool auto_shape_bf3(GemmLayer& L, bool is_out, long long P, int W) {
    if (P < 4096) return false;
    static const int nts[3] = {5, 4, 2};
    const bool short_k = (L.cin / 32) == 1;
    for (int ni = 0; ni < 3; ++ni) {
        const int nt = nts[ni];
        if (L.ncot % nt != 0 || (is_out && (nt & 1))) continue;
        int ppw = short_k ? 1 : 2, pxt = short_k ? 4 : 1, ks = short_k ? 1 : 4;
        if (short_k && nt == 5 && L.ncot % 2 == 0) continue;          // c_in = 32 prefers nt = 2
        if (is_out && P >= 32768 && nt == 4) ppw = 4;
        if (!pick_bf3(nt, ppw, pxt, ks, IN_PIXMAJOR, is_out ? EPI_OUT : EPI_HIDDEN)) continue;
        if (bf3_lds_bytes(L.cin, W, nt, ppw, pxt, ks) > 160 * 1024) continue;
        L.b_nt = nt; L.b_ppw = ppw; L.b_pxt = pxt; L.b_ks = ks; L.b_wco = 1;
        return true;
    }
    return false;
}

// will a forward launch of this layer run the bf16x3 kernel?  (also fixes L.b_* to the shape it will use)
static bool bf3_select(const iaf_stack_t* s, GemmLayer& L, int epi, bool negate_taps, bool pix_input, long long P, int W) {
    if (!prec_split(s) || !L.wp3 || !(s->packs & IAF_PACK_BF16X3)) return false;        // (iaf_stack_set_packs: the bf16x3 pack is not kept up to date)
    const bool dgrad = (epi == EPI_DGRAD || epi == EPI_DGRAD_RES);
    if (negate_taps != dgrad) return false;                        // mirrored taps: the data gradient (transposed bf16x3 pack), only
    if (!(epi == EPI_HIDDEN || epi == EPI_RES || ((epi == EPI_OUT || dgrad) && pix_input))) return false;
    if (!L.b_user_tuned && L.tuned_P == P && L.tuned_W == W) {       // measured for exactly this problem size
        if (!L.tuned_bf3) return false;
        L.b_nt = L.t_nt; L.b_ppw = L.t_ppw; L.b_pxt = L.t_pxt; L.b_ks = L.t_ks; L.b_wco = L.t_wco;
    } else if (!L.b_user_tuned && !auto_shape_bf3(L, epi == EPI_OUT, P, W)) return false;
    if (!pick_bf3(L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, IN_PIXMAJOR, epi, L.b_wco)) return false;
    return bf3_lds_bytes(L.cin, W, L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, L.b_wco) <= 160 * 1024;
}

// launches the conv kernel for GEMM descriptor L (forward layer, or a transposed descriptor for dgrad)
static int launch_gemm(const iaf_stack_t* s, GemmLayer& L, int epi, bool negate_taps, int prof_id, ConvP& p, int inmode,
                       hipStream_t st, const int* force = nullptr) {
    conv_fn_t fn = nullptr;
    bool bf3 = false;
    // forward convs of the stack go to the bf16 matrix cores (bf16x3 split products, fp32-grade) when the layer has a
    // bf16x3 pack and a compiled shape covers it; everything else runs the exact-fp32 MFMA kernel
    if (force && force[0]) {            // shape fixed by the caller (the fused first layer decided on it)
        L.b_nt = force[0]; L.b_ppw = force[1]; L.b_pxt = force[2]; L.b_ks = force[3]; L.b_wco = force[4];
        fn = pick_bf3(L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, inmode, epi, L.b_wco);
        bf3 = fn != nullptr;
    } else if (bf3_select(s, L, epi, negate_taps, inmode == IN_PIXMAJOR, p.P, p.W)) {
        fn = pick_bf3(L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, inmode, epi, L.b_wco);
        bf3 = fn != nullptr;
    }
    if (!bf3 && inmode == IN_FUSED0) return IAF_ERR_UNSUPPORTED;   // (host logic error)
    if (!bf3 && !(s->packs & IAF_PACK_F32) && L.wp3) return IAF_ERR_NOT_PREPARED;   // iaf_stack_set_packs: this stack's fp32 pack is not kept up to date
    if (!bf3 && !L.user_tuned) auto_shape(L, epi == EPI_OUT, p.P, p.W);
    const int tm = bf3 ? 16 * L.b_ppw * L.b_pxt : 16 * L.pxt;
    const int yg = bf3 ? L.ncot / (L.b_nt * L.b_wco) : L.ncot / (L.nt * L.wco);
    const int nthreads = bf3 ? 64 * L.b_pxt * L.b_ks * L.b_wco : 64 * L.pxt * L.wco * L.ks;
    // a grid of at most one workgroup per CU has nothing to overlap a prologue with: use the double-depth weight ring
    if (!bf3 && epi == EPI_HIDDEN && inmode == IN_PIXMAJOR && ((p.P + tm - 1) / tm) * (L.ncot / (L.nt * L.wco)) <= 256)
        fn = pick_kernel(L.nt, L.pxt, L.wco, L.ks, inmode, EPI_HIDDEN_DEEP);
    if (!fn) fn = pick_kernel(L.nt, L.pxt, L.wco, L.ks, inmode, epi);
    if (!fn) return IAF_ERR_UNSUPPORTED;
    p.wp = bf3 ? (const float*)L.wp3 : L.wp; p.bias = L.bias; p.lim = L.lim;
    {   // tap geometry of the two statements of the operator (see ConvP); the data gradient runs the mirrored taps
        static const int tf_dh[NTAPS] = {0, 0, 1, 1, 1}, tf_dw[NTAPS] = {0, 1, -1, 0, 1};
        const int sgn = ((s->variant == IAF_VARIANT_THEANO) != negate_taps) ? -1 : 1;
        for (int t = 0; t < NTAPS; ++t) { p.tap_dh[t] = sgn * tf_dh[t]; p.tap_dw[t] = sgn * tf_dw[t]; }
        p.halo_before = (sgn < 0) ? p.W + 1 : 0;
        p.border = negate_taps ? nullptr : L.border;
    }
    p.cin = L.cin; p.cout = L.cout; p.nchunk = L.nchunk; p.ncot = L.ncot;
    p.cp = L.cin + 8;
    p.nslot = tm + p.W + 1;
    p.dbg = (prof_id >= 0 && s->dbg_layer == prof_id) ? s->dbg : nullptr;
    const size_t lds = !bf3 ? conv_lds_bytes(L, p.W)
                     : inmode == IN_FUSED0 ? bf3_fused_lds_bytes(L.cin, p.f_cin, p.W, L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, L.b_wco)
                                           : bf3_lds_bytes(L.cin, p.W, L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, L.b_wco);
    if (lds > 160 * 1024) return IAF_ERR_UNSUPPORTED;
    { int rc = raise_lds_cap((const void*)fn, lds); if (rc) return rc; }
    dim3 grid((p.P + tm - 1) / tm, yg);
    const bool prof = (prof_id >= 0 && s->prof_layer == prof_id && s->prof_n < s->prof_cap);
    iaf_stack* ms = const_cast<iaf_stack*>(s);
    if (prof) HIP_TRY(hipEventRecord(ms->prof_start[ms->prof_n], st));
    p.gx = (int)grid.x;
    p.lds_bytes = (int)lds;
    hipLaunchKernelGGL(fn, grid, dim3(nthreads), lds, st, p);
    if (prof) { HIP_TRY(hipEventRecord(ms->prof_stop[ms->prof_n], st)); ms->prof_n++; }
    return (int)hipGetLastError();
}

static int launch_conv(const iaf_stack_t* s, int layer, ConvP& p, int inmode, hipStream_t st, const int* force = nullptr) {
    return launch_gemm(s, const_cast<iaf_stack*>(s)->L[layer], layer == s->depth_ar ? EPI_OUT : EPI_HIDDEN, false, layer, p,
                       inmode, st, force);
}

static int check_dims(const iaf_stack_t* s, int B, int H, int W) {
    if (!s) return IAF_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0) return IAF_ERR_SHAPE;
    if ((long long)B * H * W > (1LL << 30) / 64) return IAF_ERR_SHAPE;
    if (!s->prepared) return IAF_ERR_NOT_PREPARED;
    return IAF_OK;
}

// the depth_ar hidden convs + the output pair as launch descriptors.  mode (in base) selects the final epilogue.
struct Launch { int layer; ConvP p; int inmode; int force[5]; };
// Should (and can) the first masked conv run inside the second one's kernel for this problem size?  -> shape in fz[5]
static bool fuse_decide(iaf_stack_t* s, long long P, int W, int* fz) {
    if (s->fuse_first == 0 || s->depth_ar < 1) return false;
    GemmLayer& L1 = s->L[1];
    if (s->fuse_first == 2 && L1.fz_P == P && L1.fz_W == W) {           // measured by iaf_stack_autotune
        for (int i = 0; i < 5; ++i) fz[i] = L1.fz[i];
        return L1.fz_on && fuse_shape_ok(s, fz[0], fz[1], fz[2], fz[3], fz[4], W);
    }
    if (s->fuse_first != 1) return false;       // "auto" without a measurement for this size: separate launches
    // "always": the shape layer 1 would run anyway, if it can carry the fused layer
    const bool is_out = (s->depth_ar == 1);
    GemmLayer t = L1;
    if (!bf3_select(s, t, is_out ? EPI_OUT : EPI_HIDDEN, false, true, P, W)) return false;
    fz[0] = t.b_nt; fz[1] = t.b_ppw; fz[2] = t.b_pxt; fz[3] = t.b_ks; fz[4] = t.b_wco;
    return fuse_shape_ok(s, fz[0], fz[1], fz[2], fz[3], fz[4], W);
}

static int build_stack(iaf_stack_t* s, ConvP base, int first_inmode, const float* ctx, const float* ctx2, const Ws& ws,
                       Launch* out, bool allow_fuse = true) {
    const float* cur = base.x;
    int inmode = first_inmode, n = 0;
    for (int l = 0; l < s->depth_ar; ++l) {
        ConvP p = base;
        p.x = cur;
        p.ctx = (l == 0) ? ctx : nullptr;       // context only after the first conv (layers.py:163)
        p.ctx2 = (l == 0) ? ctx2 : nullptr;
        p.y = ws.hbuf[l & 1];
        out[n++] = Launch{l, p, inmode, {0, 0, 0, 0, 1}};
        cur = p.y;
        inmode = IN_PIXMAJOR;
    }
    ConvP p = base;
    p.x = cur;
    out[n++] = Launch{s->depth_ar, p, inmode, {0, 0, 0, 0, 1}};
    // the first masked conv inside the second one's kernel (IN_FUSED0): one launch less, no HBM round trip of its output
    int fz[5];
    if (allow_fuse && n >= 2 && (first_inmode == IN_NCHW || first_inmode == IN_POSTERIOR) && fuse_decide(s, base.P, base.W, fz)) {
        Launch& a = out[0];
        Launch& b = out[1];
        b.p.f_wp = s->L[0].wp3; b.p.f_bias = s->L[0].bias; b.p.f_cin = s->L[0].cin;
        b.p.f_x = (first_inmode == IN_NCHW) ? a.p.x : nullptr;      // NULL: the posterior sample from qm / rm / ql / rl / eps
        b.p.f_ctx = a.p.ctx; b.p.f_ctx2 = a.p.ctx2;
        b.p.x = nullptr;
        b.inmode = IN_FUSED0;
        for (int i = 0; i < 5; ++i) b.force[i] = fz[i];
        for (int i = 1; i < n; ++i) out[i - 1] = out[i];
        --n;
    }
    return n;
}

// hsave: training -- every hidden activation into a buffer of its own (NCHW), where the generic backward reads it
static int run_stack_generic(iaf_stack_t* s, const ConvP& base, int first_inmode, const float* ctx, const float* ctx2,
                             const Ws& ws, hipStream_t st, float* const* hsave = nullptr) {
    const float* cur = base.x;
    for (int l = 0; l <= s->depth_ar; ++l) {
        const GemmLayer& L = s->L[l];
        GenConvP p;
        memset(&p, 0, sizeof(p));
        p.B = base.B; p.H = base.H; p.W = base.W; p.cin = L.cin; p.cout = L.cout; p.nz = s->n_z;
        p.w = L.wp; p.bias = L.bias;
        p.x = cur; p.posterior_in = (l == 0 && first_inmode == IN_POSTERIOR) ? 1 : 0;
        p.qm = base.qm; p.ql = base.ql; p.rm = base.rm; p.rl = base.rl; p.pm = base.pm; p.pl = base.pl; p.eps = base.eps;
        p.is_out = (l == s->depth_ar) ? 1 : 0;
        if (p.is_out) {
            p.mode = base.mode; p.zin = base.zin; p.out0 = base.out0; p.out1 = base.out1; p.kl_elem = base.kl_elem;
        } else {
            p.ctx = (l == 0) ? ctx : nullptr; p.ctx2 = (l == 0) ? ctx2 : nullptr;
            p.y = hsave ? hsave[l] : ws.hbuf[l & 1];
        }
        const size_t total = (size_t)p.B * (p.is_out ? p.nz : p.cout) * p.H * p.W;
        hipLaunchKernelGGL(iaf_generic_conv_kernel, ew_grid(total), dim3(256), 0, st, p);
        cur = p.y;
    }
    return (int)hipGetLastError();
}

// The whole step in one launch (iaf_step_fused.hpp): bf16x3 precision, a compiled geometry for (n_h, n_z, depth_ar, W) --
// everything else takes the layer-by-layer path.  All three statements of the operator (the Theano one runs on the image
// rotated by 180 degrees, where its taps are the TF ones).  Output rows per workgroup: 2 at 16 pixels per row; at 8,
// one row while that still leaves fewer than two workgroups per CU (less halo recompute per row otherwise).
// The halo-exchange form of the one-launch step (iaf_step_fused.hpp, XCH), where it applies: more than one row block per image, a
// geometry compiled for it and for the stack's statement (IAF_FUSE_XCH=0: dev knob)
static step_fn_t fused_step_xch(const iaf_stack_t* s, int H, int W, int R, size_t* lds, size_t* xrow) {
    static const bool xch_env = !(getenv("IAF_FUSE_XCH") && getenv("IAF_FUSE_XCH")[0] == '0');
    if (!xch_env || !s->xch_on || R <= 0 || (H + R - 1) / R < 2) return nullptr;
    step_fn_t f = pick_step(step_key(s, W, R, STEP_XCH), lds, xrow);
    return (f && *lds <= 160 * 1024) ? f : nullptr;
}

// The pair form of the one-launch step (iaf_step_fused.hpp, PAIR; 8-pixel rows): two workgroups per (image, block of R = 2 rows), each
// streaming half of the last hidden layer's and of the output pair's weights, their halves of the last hidden region swapped through
// the stack's exchange buffers (*prow bytes per half).  Where it is switched on it replaces the one-row-per-workgroup kernel: same number
// of workgroups, full MFMA tiles, 0.65 instead of 1.23 MB through each CU's port.
static step_fn_t fused_step_pair(const iaf_stack_t* s, int W, size_t* lds, size_t* prow) {
    // OPT-IN (knob 32 of iaf_stack_set_halo_exchange_debug, or IAF_FUSE_PAIR=1): measured on MI355X at B = 32 it LOSES to the
    // one-row kernel, 18.9 vs 17.0 us -- the K loops turned out to be bound by what ONE wave per SIMD can issue (~30 cycles per MFMA
    // with its loads and LDS reads), not by the port, and the hand-over exposes 3.9 k cycles (profiles/r05/experiments/pair_form.txt).
    static const bool pair_env = getenv("IAF_FUSE_PAIR") && getenv("IAF_FUSE_PAIR")[0] == '1';
    if (!(pair_env || (s->xch_knob & 32u)) || !s->xch_on || W != 8) return nullptr;
    step_fn_t f = pick_step(step_key(s, W, 2, STEP_PAIR), lds, prow);
    return (f && *lds <= 160 * 1024) ? f : nullptr;
}

// The exchange set of stream st, grown to [layer][B * nrb] rows of xrow bytes (pair form, depth_ar = 2: [B * nrb][2 halves] of xrow bytes): created on the stream's first such launch -- not
// inside a stream capture (there: the stream's set, else the newest one that is large enough, else NULL and the caller runs what
// it ran before; warm up before capturing, as for the LDS cap).  A set that grows keeps its counters; the new rows start as
// "nothing there yet" (IAF_XSENT).  Outgrown rows stay alive with the stack: a captured graph may still name them.
// pattern: the "not there yet" pattern of the kernels that will use the set (IAF_XSENT: bf16 planes, IAF_XSENT_F16: fp16 planes) -- a set
// serves one plane type; a stream that runs both has two sets.
static iaf_stack::XchSet* xch_prepare(iaf_stack_t* s, int B, int nrb, size_t xrow, hipStream_t st, unsigned pattern = IAF_XSENT) {
    std::lock_guard<std::mutex> lk(s->xch_mu);
    iaf_stack::XchSet* x = nullptr;
    for (auto& e : s->xch_sets) if (e.st == st && e.pattern == pattern) { x = &e; break; }
    const size_t need = (size_t)s->depth_ar * B * nrb * xrow > 256 ? (size_t)s->depth_ar * B * nrb * xrow : 256;   // (xrow = 0: only the counters are wanted)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cs);
    if (x && need <= x->bytes) {
        if (cs != hipStreamCaptureStatusNone) x->captured = true;
        return x;
    }
    if (cs != hipStreamCaptureStatusNone) {
        // no allocation inside a capture: a capture stream without a set of its own (torch.cuda.graph's internal stream after a
        // warm-up elsewhere) TAKES OVER the newest set that is large enough -- the set now belongs to the capture stream, so the
        // graph's replays share no rows and no counters with later eager launches on the stream it came from (those allocate a
        // fresh set on their next call; include/iaf_hip.h).  None large enough: the caller runs the recomputing kernel.
        // A set that a graph captured on ANOTHER stream already names is not taken (two graphs on two streams would share
        // its rows and counters, and concurrent replays race into bounded waits and NaN): the caller then runs the recomputing kernel.
        for (size_t i = s->xch_sets.size(); i-- > 0;) {
            iaf_stack::XchSet& e = s->xch_sets[i];
            if (need <= e.bytes && e.pattern == pattern && !e.captured) { e.st = st; e.captured = true; return &e; }
        }
        return nullptr;
    }
    if (!s->xch_err_host) {
        if (hipHostMalloc((void**)&s->xch_err_host, 64, hipHostMallocMapped) != hipSuccess) { s->xch_err_host = nullptr; return nullptr; }
        *(volatile unsigned*)s->xch_err_host = 0u;
        if (hipHostGetDevicePointer((void**)&s->xch_err_dev, s->xch_err_host, 0) != hipSuccess) {
            (void)hipHostFree(s->xch_err_host); s->xch_err_host = nullptr; s->xch_err_dev = nullptr;
            return nullptr;
        }
    }
    char* nb = nullptr;
    unsigned long long* nc = x ? x->ctl : nullptr;
    bool ok = hipMalloc((void**)&nb, need) == hipSuccess &&
              hipMemsetD32Async((hipDeviceptr_t)nb, (int)pattern, need / 4, st) == hipSuccess;    // (ordered in front of the launch)
    if (ok && !nc) ok = hipMalloc((void**)&nc, IAF_XCTL_WORDS * sizeof(unsigned long long)) == hipSuccess &&
                        hipMemsetAsync(nc, 0, IAF_XCTL_WORDS * sizeof(unsigned long long), st) == hipSuccess;
    if (!ok) {
        if (nb) (void)hipFree(nb);
        if (nc && !(x && x->ctl == nc)) (void)hipFree(nc);
        return nullptr;
    }
    if (!x) { s->xch_sets.emplace_back(); x = &s->xch_sets.back(); x->st = st; x->pattern = pattern; }
    if (x->buf) s->xch_retired_rows.push_back({x->buf, x->bytes, x->pattern});
    x->buf = nb; x->bytes = need; x->ctl = nc;
    return x;
}


// st / launching: the stream of an imminent launch (the halo-exchange buffers may be allocated for it); a query otherwise
static step_fn_t fused_step_plan(const iaf_stack_t* s, int B, int H, int W, int* R, size_t* lds, hipStream_t st = nullptr,
                                 bool launching = false) {
    static const int env = getenv("IAF_FUSE_STEP") ? atoi(getenv("IAF_FUSE_STEP")) : -1;       // dev knob: 0 / 1
    const int mode = env >= 0 ? env : s->fuse_step;
    if (!mode || s->generic || s->resnet || !prec_split(s)) return nullptr;      // (the masked ResNet runs layer by layer: run_resnet)
    if (s->depth_ar < 1 || s->depth_ar > 4 || (s->n_h & 15) || (s->n_z & 15)) return nullptr;
    if (s->fuse_first == 1) return nullptr;                  // the caller asked for the layer-by-layer variant with a fused first conv
    for (int l = 0; l < s->nlayers; ++l)                      // ... or pinned a per-layer launch shape: the layer-by-layer path is meant
        if (!s->L[l].wp3 || s->L[l].user_tuned || s->L[l].b_user_tuned) return nullptr;
    static const int forceR = getenv("IAF_FUSE_STEP_R") ? atoi(getenv("IAF_FUSE_STEP_R")) : 0;  // dev knob
    *R = forceR ? forceR : (W == 16 ? 2 : W == 4 ? 4 : ((long long)B * H >= 1024 ? 2 : 1));
    // Every workgroup streams the stack's whole weight set (1.2 MB at n_h = 160) out of L2, so the launch's L2 traffic
    // grows with the workgroup count while the layer-by-layer kernels amortise a weight fetch over more pixels as the batch
    // grows: measured, the one-launch step wins at 16-pixel rows up to B = 256 and at 8-pixel rows only while one row per
    // workgroup still fits a round or two of the chip (B = 32: 17 vs 22 us; B = 256: 69 vs 61 us).
    if (s->fs_force == 0) return nullptr;
    if (s->fs_force < 0 && mode != 2) {
        if (s->fs_P == (long long)B * H * W && s->fs_W == W) { if (!s->fs_on) return nullptr; }      // measured for this size
        else if (W == 8 && (long long)B * H >= 1024) return nullptr;
        else if (W == 4) {
            // one workgroup per image walks the whole weight set alone: ~12 us per MB of bf16x3 packs (n_h = 64, depth 4: 0.74 MB,
            // 12.5 us; n_h = 128: 2.2 MB, 27 us), while each layer-by-layer launch costs ~4.6 us of a replayed graph at this size
            double wmb = 0.0;
            for (int l = 0; l < s->nlayers; ++l) wmb += 5.0 * s->L[l].cin * s->L[l].cout * 6.0 * 1e-6;
            if (wmb * 12.3 > 4.6 * s->nlayers) return nullptr;
        }
    }
    if (!forceR || forceR == 2) {
        // 8-pixel rows: the pair form (R = 2 rows per PAIR of workgroups).  Without buffers for it (a capture that was not warmed up)
        // launch_fused_step runs the recomputing kernel of the same R instead.
        size_t pl = 0, prow = 0;
        if (step_fn_t fp = fused_step_pair(s, W, &pl, &prow)) {
            size_t rl = 0, rr = 0;
            if (pick_step(step_key(s, W, 2, STEP_RECOMPUTE), &rl, &rr) && rl <= 160 * 1024) {
                if (launching) (void)xch_prepare(const_cast<iaf_stack_t*>(s), B, (H + 1) / 2, prow, st);
                *R = 2; *lds = pl;
                return fp;
            }
        }
    }
    size_t row = 0;
    step_fn_t fn = pick_step(step_key(s, W, *R, STEP_RECOMPUTE), lds, &row);
    if (fn && *lds <= 160 * 1024) return fn;               // (launch_fused_step switches to the halo-exchange form where it applies)
    // geometries whose LDS regions only fit in the halo-exchange form (R + 1 rows per region instead of R + depth_ar): config 3's
    // n_h = 128 / 192 at 16-pixel rows
    size_t xl = 0, xrow = 0;
    step_fn_t fx = fused_step_xch(s, H, W, *R, &xl, &xrow);
    if (!fx) return nullptr;
    if (launching && !xch_prepare(const_cast<iaf_stack_t*>(s), B, (H + *R - 1) / *R, xrow, st)) return nullptr;
    *lds = xl;
    return fx;
}

extern "C" int iaf_stack_step_pairs(const iaf_stack_t* s, int B, int H, int W) {
    if (!s) return 0;
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    int R = 0;
    size_t lds = 0, pl = 0, prow = 0;
    step_fn_t fn = fused_step_plan(s, B, H, W, &R, &lds);
    return (fn && fn == fused_step_pair(s, W, &pl, &prow)) ? 1 : 0;
}

// 1: the one-launch step at this size runs a two-plane fp16 kernel (IAF_PRECISION_F16X2, a compiled geometry, no range failure so far)
extern "C" int iaf_stack_step_is_f16(const iaf_stack_t* s, int B, int H, int W) {
    if (!s || B <= 0 || H <= 0 || W <= 0 || !f16_active(s)) return 0;
    const int R = iaf_stack_step_is_fused(s, B, H, W);
    if (R <= 0 || iaf_stack_step_pairs(s, B, H, W)) return 0;
    size_t l = 0, x = 0, xl = 0, xr = 0;
    if (fused_step_xch(s, H, W, R, &xl, &xr)) return pick_step(step_key(s, W, R, STEP_XCH, STEP_F16X2), &l, &x) ? 1 : 0;
    static const int h8_env = getenv("IAF_STEP_HELPERS") ? atoi(getenv("IAF_STEP_HELPERS")) : -1;
    return (h8_env != 0 && pick_step(step_key(s, W, R, STEP_HELPERS, STEP_F16X2), &l, &x)) ? 1 : 0;
}

extern "C" int iaf_stack_step_exchanges(const iaf_stack_t* s, int B, int H, int W) {
    if (!s) return 0;
    const int R = iaf_stack_step_is_fused(s, B, H, W);
    size_t lds = 0, xrow = 0;
    return (R > 0 && fused_step_xch(s, H, W, R, &lds, &xrow)) ? 1 : 0;
}

// threads per workgroup of a one-launch step kernel = its launch bound (256, or 512 with helper waves: iaf_step_fused.hpp)
static int step_threads(step_fn_t fn) {
    static std::mutex mu;
    static std::map<const void*, int> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find((const void*)fn);
    if (it != cache.end()) return it->second;
    hipFuncAttributes a;
    int n = 256;
    if (hipFuncGetAttributes(&a, (const void*)fn) == hipSuccess && a.maxThreadsPerBlock >= 256) n = a.maxThreadsPerBlock;
    cache[(const void*)fn] = n;
    return n;
}

// kl_part: posterior mode only -- per-(row block, channel) sums of the KL elements, [B * nrb][n_z] (StepP::kl_part)
// fin (posterior mode, optional): where the block's free-bits results go if the launch can finish them itself (StepP::fin_*); *fin->done
// tells the caller whether it did -- else the caller runs launch_kl_from_parts behind the launch as before
struct StepFin { float* kl_obj; float* kl_cost; float kl_min; bool done; float* gate; };      // (the groups: the stack's fb_groups)
static int launch_fused_step(iaf_stack_t* s, step_fn_t fn, int R, size_t lds, const ConvP& base, int first_inmode, const float* ctx,
                             const float* ctx2, hipStream_t st, float* const* hsave = nullptr, float* kl_part = nullptr,
                             StepFin* fin = nullptr) {
    if (fin) fin->done = false;
    // A bounded wait of an earlier launch of this stack gave up (its outputs carry NaN): said once, as this call's status, and
    // the stack goes on with the kernels that recompute their halo rows until iaf_stack_set_halo_exchange re-arms the exchange.
    if (s->xch_on && s->xch_err_host && *(volatile unsigned*)s->xch_err_host) {
        s->xch_on = false;
        return IAF_ERR_EXCHANGE;
    }
    // An F16 launch (or the prep of its packs) met an operand beyond fp16's range (its outputs carry inf / NaN): said once, and the stack
    // goes on with the bf16x3 kernels -- behind another prepare where the bf16x3 pack was not being kept up to date.
    if (pack_range_report(*s, PACK_STACK, s->rng.peek())) return IAF_ERR_RANGE;
    const bool f16 = f16_active(s);
    bool f16_fn = false;                                     // the launch runs an F16 kernel (on the two-plane packs)
    StepP q;
    memset(&q, 0, sizeof(q));
    q.kl_part = kl_part;
    if (hsave)
        for (int l = 0; l < s->depth_ar && l < 4; ++l) q.hsave[l] = hsave[l];
    q.z = (first_inmode == IN_POSTERIOR) ? nullptr : base.x;
    q.ctx = ctx; q.ctx2 = ctx2;
    for (int l = 0; l < s->nlayers; ++l) { q.wp3[l] = s->L[l].wp3; q.bias[l] = s->L[l].bias; }      // (an F16 kernel: the two-plane packs, below)
    q.zin = base.zin; q.out0 = base.out0; q.out1 = base.out1; q.kl_elem = base.kl_elem;
    q.qm = base.qm; q.ql = base.ql; q.rm = base.rm; q.rl = base.rl; q.pm = base.pm; q.pl = base.pl; q.eps = base.eps;
    q.B = base.B; q.H = base.H; q.HW = base.HW; q.mode = base.mode;
    q.skip = base.mode == MODE_INVERSE ? base.inv_done : nullptr;
    q.nrb = (base.H + R - 1) / R;
    //  the posterior callers pass a hidden-activation buffer of the workspace ([B H W][n_h] floats) as kl_part
    // [B * nrb][n_z]: holds for every geometry compiled today (nrb <= H, n_z <= W n_h) -- enforced here for the ones to come
    if (kl_part && (size_t)q.nrb * s->n_z > (size_t)base.H * base.W * s->n_h) return IAF_ERR_WORKSPACE;
    if (s->variant != IAF_VARIANT_TF)                          // (the kernel variant was picked with the statement)
        for (int l = 0; l < s->nlayers; ++l) q.border[l] = s->L[l].border;
    q.dbg = (s->dbg_layer == -2) ? s->dbg : nullptr;
    // Halo exchange instead of halo recompute (TF statement, more than one row block per image, the geometries compiled for it;
    // IAF_FUSE_XCH=0: dev knob).  Its buffers are the stack's: allocated here on first use -- not inside a stream capture, where
    // the recomputing kernel runs instead (warm up before capturing, as for the LDS cap below).
    bool pair = false;
    {
        size_t pl = 0, prow = 0;
        step_fn_t fp = (R == 2) ? fused_step_pair(s, base.W, &pl, &prow) : nullptr;
        if (fn == fp && fp) {
            if (iaf_stack::XchSet* x = xch_prepare(s, base.B, q.nrb, prow, st)) {
                pair = true; lds = pl;
                q.xh = x->buf; q.xctl = x->ctl; q.xerr = s->xch_err_dev; q.xknob = s->xch_knob;
            } else {                                         // no buffers (inside a capture that was not warmed up): the recomputing kernel of the same R
                size_t row = 0;
                fn = pick_step(step_key(s, base.W, R, STEP_RECOMPUTE), &lds, &row);
                if (!fn) return IAF_ERR_NOT_PREPARED;
            }
        }
    }
    if (!pair) {
        size_t xl = 0, xrow = 0;
        if (step_fn_t fx = fused_step_xch(s, base.H, base.W, R, &xl, &xrow)) {
            // the exchange form on fp16 planes, where the stack asks for it and the geometry is compiled: rows of two planes, a set of its own
            size_t xl16 = 0, xrow16 = 0;
            step_fn_t fx16 = f16 ? pick_step(step_key(s, base.W, R, STEP_XCH, STEP_F16X2), &xl16, &xrow16) : nullptr;
            iaf_stack::XchSet* x16 = fx16 ? xch_prepare(s, base.B, q.nrb, xrow16, st, IAF_XSENT_F16) : nullptr;
            if (x16) {
                fn = fx16; lds = xl16; f16_fn = true;
                q.xh = x16->buf; q.xctl = x16->ctl; q.xerr = s->xch_err_dev; q.xknob = s->xch_knob;
            } else if (iaf_stack::XchSet* x = xch_prepare(s, base.B, q.nrb, xrow, st)) {
                fn = fx; lds = xl;
                q.xh = x->buf; q.xctl = x->ctl; q.xerr = s->xch_err_dev; q.xknob = s->xch_knob;
            } else if (fn == fx) {
                return IAF_ERR_NOT_PREPARED;                 // (a geometry that only exists in this form, and no buffers: fused_step_plan refuses that)
            }
        }
    }
    // a recomputing kernel: its form with helper waves, where one is compiled (the 8-pixel BASELINE geometry) -- for the posterior block
    // (the last workgroup's helpers do the free-bits reductions)
    // ... and since round 5 every mode of the step there: with the second hidden layer's left-over units in the helper waves (HLEFT) the
    // form with helpers is the faster one for the bare IAF step too (16.98 -> 16.50 us in situ, same box; round 4 without HLEFT: 16.62
    // without helpers, 16.89 with).  IAF_STEP_HELPERS=0 keeps the four-wave form (knob 16 only moves the free-bits finish into its own launch).
    static const int h8_env = getenv("IAF_STEP_HELPERS") ? atoi(getenv("IAF_STEP_HELPERS")) : -1;
    if (h8_env != 0 && !q.xh && !pair) {
        size_t hl = 0, hr = 0;
        if (step_fn_t fh = pick_step(step_key(s, base.W, R, STEP_HELPERS), &hl, &hr))
            if (hl == lds) fn = fh;
        // ... on fp16 planes (its own LDS layout: two planes per slot)
        size_t hl16 = 0, xr16 = 0;
        if (step_fn_t fh16 = f16 ? pick_step(step_key(s, base.W, R, STEP_HELPERS, STEP_F16X2), &hl16, &xr16) : nullptr) {
            fn = fh16; lds = hl16; f16_fn = true;
        }
    }
    if (f16_fn) {
        for (int l = 0; l < s->nlayers; ++l) q.wp3[l] = s->L[l].wp2;
        q.rng_err = s->rng.dev;
    } else if (!(s->packs & IAF_PACK_BF16X3)) {
        return IAF_ERR_NOT_PREPARED;                         // iaf_stack_set_packs: this stack's bf16x3 pack is not kept up to date
    }
    { int rc = raise_lds_cap((const void*)fn, lds); if (rc) return rc; }
    // The free-bits reductions inside the launch: kernels with helper waves, a table one workgroup can walk (the bounds of the
    // single-workgroup finish launch), n_z <= 64 channels and a set of counters for this stream (none inside a capture that was
    // not warmed up: then the finish launch follows as before).  IAF_KL_IN_LAUNCH=0: dev knob.
    if (fin && kl_part && base.mode == MODE_POSTERIOR && step_threads(fn) == 512 && s->n_z <= 64 &&
        (long long)base.B * q.nrb * s->n_z <= 16384 && (long long)base.B * s->n_z <= 8192) {
        static const bool fin_env = !(getenv("IAF_KL_IN_LAUNCH") && getenv("IAF_KL_IN_LAUNCH")[0] == '0');
        if (fin_env && !(s->xch_knob & 16u))                 // (test knob 16: the finish launch, to compare against)
            if (iaf_stack::XchSet* x = xch_prepare(s, base.B, q.nrb, 0, st, f16_fn ? IAF_XSENT_F16 : IAF_XSENT)) {
                q.fin_obj = fin->kl_obj; q.fin_cost = fin->kl_cost; q.fin_kl_min = fin->kl_min; q.fin_ctl = x->ctl + IAF_XCTL_FIN; q.fin_gate = fin->gate;
                q.fin_groups = s->fb_groups;
                fin->done = true;
            }
    }
    const bool prof = (s->prof_layer == -2 && s->prof_n < s->prof_cap);
    if (prof) HIP_TRY(hipEventRecord(s->prof_start[s->prof_n], st));
    hipLaunchKernelGGL(fn, dim3(base.B * q.nrb * (pair ? 2 : 1)), dim3(step_threads(fn)), lds, st, q);       // (512 where four helper waves sit beside the compute waves)
    if (prof) { HIP_TRY(hipEventRecord(s->prof_stop[s->prof_n], st)); s->prof_n++; }
    return (int)hipGetLastError();
}

// The rest of the posterior block's reductions behind a one-launch step that left its partial sums in part [B][nrb][Z]
// (tf_train.py:77-85): ONE 256-thread launch while one workgroup can walk the partials (B = 32: 8 k loads), a many-workgroup
// row-block sum in front of it beyond that (config 5, B = 256).  rowsum: [B * Z] floats of scratch.
static int launch_kl_from_parts(const float* part, float* rowsum, float* kl_obj, float* kl_cost, int B, int Z, int nrb, float kl_min,
                                float* gate, int groups, hipStream_t st) {
    const long long loads = (long long)B * nrb * Z;
    if (loads <= 16384) {
        hipLaunchKernelGGL(iaf_kl_finish_kernel, dim3(1), dim3(256), 0, st, part, kl_obj, kl_cost, B, Z, kl_min, gate, nrb, rowsum, groups);
    } else {
        const int n = B * Z;
        hipLaunchKernelGGL(iaf_kl_partsum_kernel, dim3((n + 255) / 256), dim3(256), 0, st, part, rowsum, n, Z, nrb);
        hipLaunchKernelGGL(iaf_kl_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)rowsum, kl_obj, kl_cost, B, Z, kl_min, gate, 0,
                           (float*)nullptr, groups);
    }
    return (int)hipGetLastError();
}

// The masked ResNet (ar.py:478-528), layer by layer; D = s->resnet blocks:
//   L[0]      EPI_RES     z (NCHW) -> h_0 = conv + context (raw)          and elu(h_0)
//   L[2i+1]   EPI_HIDDEN  elu(h_i) -> t_i = elu(conv1)
//   L[2i+2]   EPI_RES     t_i      -> h_{i+1} = h_i + 0.1 conv2 (raw)     and elu(h_{i+1}) unless i = D - 1
//   L[2D+1]   EPI_OUT     h_D (raw)  -> the (mean, logsd) pair under base.mode
// raw: the stream, updated in place (an element is read and written by one lane); h_last: where h_D goes (raw itself when evaluating).
// Evaluation: act, t are two scratch buffers, save == NULL.  Training: save[l] = what layer l + 1 reads, the activations the backward
// pass needs: save[2i] = elu(h_i), save[2i+1] = t_i, save[2D] = h_D.
static int run_resnet(iaf_stack_t* s, const ConvP& base, const float* ctx, const float* ctx2, float* raw, float* h_last, float* act,
                      float* t, float* const* save, hipStream_t st) {
    const int D = s->resnet;
    int rc;
    ConvP p = base;
    p.mode = 0;
    p.ctx = ctx; p.ctx2 = ctx2;
    p.y = raw; p.y2 = save ? save[0] : act;
    if ((rc = launch_gemm(s, s->L[0], EPI_RES, false, 0, p, IN_NCHW, st))) return rc;
    for (int i = 0; i < D; ++i) {
        const bool last = (i == D - 1);
        const float* a_i = save ? save[2 * i] : act;
        float* t_i = save ? save[2 * i + 1] : t;
        p = base;
        p.mode = 0;
        p.x = a_i; p.y = t_i;
        if ((rc = launch_gemm(s, s->L[2 * i + 1], EPI_HIDDEN, false, 2 * i + 1, p, IN_PIXMAJOR, st))) return rc;
        p = base;
        p.mode = 0;
        p.x = t_i; p.skip = raw;
        p.y = last ? h_last : raw;
        p.y2 = last ? nullptr : (save ? save[2 * i + 2] : act);
        if ((rc = launch_gemm(s, s->L[2 * i + 2], EPI_RES, false, 2 * i + 2, p, IN_PIXMAJOR, st))) return rc;
    }
    p = base;
    p.x = h_last;
    return launch_gemm(s, s->L[s->depth_ar], EPI_OUT, false, s->depth_ar, p, IN_PIXMAJOR, st);
}

static int run_stack(iaf_stack_t* s, ConvP base, int first_inmode, const float* ctx, const float* ctx2, const Ws& ws,
                     hipStream_t st) {
    if (s->generic) return run_stack_generic(s, base, first_inmode, ctx, ctx2, ws, st);
    if (s->resnet) {
        if (first_inmode != IN_NCHW) return IAF_ERR_UNSUPPORTED;
        return run_resnet(s, base, ctx, ctx2, ws.hbuf[0], ws.hbuf[0], ws.hbuf[1], ws.hbuf[2], nullptr, st);
    }
    if (first_inmode == IN_NCHW || first_inmode == IN_POSTERIOR) {
        int R = 0;
        size_t lds = 0;
        const bool aligned = (((uintptr_t)ctx | (uintptr_t)ctx2) & 15) == 0;      // it fetches the contexts 16 bytes at a time
        if (step_fn_t fn = aligned ? fused_step_plan(s, base.B, base.H, base.W, &R, &lds, st, true) : nullptr)
            return launch_fused_step(s, fn, R, lds, base, first_inmode, ctx, ctx2, st);
    }
    Launch ls[MAX_GEMM_LAYERS];
    const int n = build_stack(s, base, first_inmode, ctx, ctx2, ws, ls);
    for (int i = 0; i < n; ++i) {
        int rc = launch_conv(s, ls[i].layer, ls[i].p, ls[i].inmode, st, ls[i].force);
        if (rc) return rc;
    }
    return IAF_OK;
}

// `reps` launches between ONE event pair on `st`; *avg_ms = elapsed / reps.  Releases its events on every path.
template <class F>
static int time_reps(hipStream_t st, int reps, float* avg_ms, F&& launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = (int)hipEventCreate(&e0);
    if (!rc) rc = (int)hipEventCreate(&e1);
    if (!rc) rc = (int)hipEventRecord(e0, st);
    for (int r = 0; r < reps && !rc; ++r) rc = launch();
    if (!rc) rc = (int)hipEventRecord(e1, st);
    if (!rc) rc = (int)hipEventSynchronize(e1);
    float ms = 0.f;
    if (!rc) rc = (int)hipEventElapsedTime(&ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    *avg_ms = ms / (float)reps;
    return rc;
}

extern "C" int iaf_step_time_layer(iaf_stack_t* s, int layer, const float* z, const float* context, float* z_new,
                                   float* logsd, int B, int H, int W, void* workspace, size_t workspace_bytes, int reps,
                                   void* stream, float* avg_ms) {
    if (s && s->resnet) return IAF_ERR_UNSUPPORTED;      // (iaf_stack_create_resnet: include/iaf_hip.h; before any other answer)
    int rc = check_dims(s, B, H, W);
    if (rc) return rc;
    if (!z || !z_new || !logsd || !avg_ms || (s->depth_ar > 0 && !context)) return IAF_ERR_NULL;
    // layer = -1: the FUSED launch (first masked conv inside the second one's kernel), if the stack would use it at this size
    if (layer < -2 || layer >= s->nlayers || reps <= 0) return IAF_ERR_SHAPE;
    if (s->generic) return IAF_ERR_UNSUPPORTED;
    Ws ws;
    if ((rc = carve_ws(s, B, H, W, workspace, workspace_bytes, &ws))) return rc;
    hipStream_t st = (hipStream_t)stream;
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.B = B; p.H = H; p.W = W; p.HW = H * W; p.P = B * H * W;
    p.x = z; p.zin = z; p.out0 = z_new; p.out1 = logsd; p.mode = MODE_IAF;
    if (layer == -2) {                // the whole step as ONE launch (iaf_step_fused.hpp), if the stack runs it that way here
        int R = 0;
        size_t lds = 0;
        step_fn_t fn = fused_step_plan(s, B, H, W, &R, &lds, st, true);
        if (!fn) return IAF_ERR_UNSUPPORTED;
        if ((rc = launch_fused_step(s, fn, R, lds, p, IN_NCHW, context, nullptr, st))) return rc;
        const int saved = s->prof_layer;
        s->prof_layer = -1;
        rc = time_reps(st, reps, avg_ms, [&]() { return launch_fused_step(s, fn, R, lds, p, IN_NCHW, context, nullptr, st); });
        s->prof_layer = saved;
        return rc;
    }
    Launch ls[MAX_GEMM_LAYERS];
    int n = build_stack(s, p, IN_NCHW, context, nullptr, ws, ls, false);      // single layers are timed unfused
    for (int i = 0; i < n; ++i)                      // one full step: every layer's input is valid scratch afterwards
        if ((rc = launch_conv(s, ls[i].layer, ls[i].p, ls[i].inmode, st, ls[i].force))) return rc;
    if (layer == -1) {
        n = build_stack(s, p, IN_NCHW, context, nullptr, ws, ls, true);
        if (ls[0].inmode != IN_FUSED0) return IAF_ERR_UNSUPPORTED;
        layer = 0;
    }
    const int saved = s->prof_layer;
    s->prof_layer = -1;
    rc = time_reps(st, reps, avg_ms, [&]() { return launch_conv(s, ls[layer].layer, ls[layer].p, ls[layer].inmode, st, ls[layer].force); });
    s->prof_layer = saved;
    return rc;
}

// Launch-shape / kernel-family search for one problem size (the counterpart of the cuDNN algorithm search behind the
// reference's tf.nn.conv2d): every GEMM layer is timed as the exact-fp32 kernel (its automatic shape) and as every
// compiled bf16x3 shape, `reps` back-to-back launches per event pair on the caller's buffers; the winner is remembered
// for (B*H*W, W) and used by every later forward launch of that size.  chosen[l] = 0 (fp32 kernel) or
// nt*10000 + ppw*1000 + pxt*100 + ks*10 + wco; us[l] = its time.  Synchronises; do not call inside a stream capture.
extern "C" int iaf_stack_autotune(iaf_stack_t* s, const float* z, const float* context, float* z_new, float* logsd, int B,
                                  int H, int W, void* workspace, size_t workspace_bytes, int reps, void* stream,
                                  int* chosen, float* us) {
    if (s && s->resnet) return IAF_ERR_UNSUPPORTED;      // (iaf_stack_create_resnet: include/iaf_hip.h; before any other answer)
    int rc = check_dims(s, B, H, W);
    if (rc) return rc;
    if (s->generic) return IAF_OK;
    if (reps <= 0) return IAF_ERR_SHAPE;
    const long long P = (long long)B * H * W;
    const int saved_prec = s->precision;
    for (int l = 0; l < s->nlayers; ++l) {
        GemmLayer& L = s->L[l];
        const bool is_out = (l == s->depth_ar);
        L.tuned_P = -1;
        float best = 0.f, ms = 0.f;
        s->precision = IAF_PRECISION_F32;
        if ((rc = iaf_step_time_layer(s, l, z, context, z_new, logsd, B, H, W, workspace, workspace_bytes, reps, stream, &ms))) break;
        best = ms;
        int bsel[5] = {0, 0, 0, 0, 1};
        if (saved_prec != IAF_PRECISION_F32 && L.wp3 && (s->packs & IAF_PACK_BF16X3) && !(is_out && s->depth_ar == 0)) {
            s->precision = IAF_PRECISION_BF16X3;
            const bool ut = L.b_user_tuned;
            const int sv[5] = {L.b_nt, L.b_ppw, L.b_pxt, L.b_ks, L.b_wco};
            static const int nts[3] = {5, 4, 2};
            for (int si = 0; si < (int)std::size(k_bf3_shapes) && !rc; ++si)
                for (int ni = 0; ni < 3 && !rc; ++ni) {
                    const int nt = nts[ni], ppw = k_bf3_shapes[si].ppw, pxt = k_bf3_shapes[si].pxt, ks = k_bf3_shapes[si].ks;
                    const int wco = k_bf3_shapes[si].wco;
                    if (L.ncot % (nt * wco) != 0 || (is_out && (nt & 1))) continue;
                    if (!pick_bf3(nt, ppw, pxt, ks, IN_PIXMAJOR, is_out ? EPI_OUT : EPI_HIDDEN, wco)) continue;
                    if (bf3_lds_bytes(L.cin, W, nt, ppw, pxt, ks, wco) > 160 * 1024) continue;
                    L.b_nt = nt; L.b_ppw = ppw; L.b_pxt = pxt; L.b_ks = ks; L.b_wco = wco; L.b_user_tuned = true;
                    rc = iaf_step_time_layer(s, l, z, context, z_new, logsd, B, H, W, workspace, workspace_bytes, reps, stream, &ms);
                    if (!rc && ms < best) { best = ms; bsel[0] = nt; bsel[1] = ppw; bsel[2] = pxt; bsel[3] = ks; bsel[4] = wco; }
                }
            L.b_user_tuned = ut; L.b_nt = sv[0]; L.b_ppw = sv[1]; L.b_pxt = sv[2]; L.b_ks = sv[3]; L.b_wco = sv[4];
        }
        if (rc) break;
        L.tuned_P = P; L.tuned_W = W; L.tuned_bf3 = bsel[0] != 0;
        L.t_nt = bsel[0]; L.t_ppw = bsel[1]; L.t_pxt = bsel[2]; L.t_ks = bsel[3]; L.t_wco = bsel[4];
        if (chosen) chosen[l] = bsel[0] ? bsel[0] * 10000 + bsel[1] * 1000 + bsel[2] * 100 + bsel[3] * 10 + bsel[4] : 0;
        if (us) us[l] = 1e3f * best;
        L.tuned_us = 1e3f * best;
    }
    s->precision = saved_prec;
    // the whole step as one launch against the layer-by-layer launches just tuned: `reps` full steps back to back each way
    if (!rc && s->fuse_step) {
        s->fs_P = -1;
        int R = 0;
        size_t lds = 0;
        s->fs_force = 1;
        const bool possible = fused_step_plan(s, B, H, W, &R, &lds, (hipStream_t)stream, true) != nullptr;
        float t[2] = {0.f, 0.f};
        // Timed as `reps` steps captured once and replayed -- the way a sampling / training loop runs them.  Issued one by one,
        // the layer-by-layer path at the small levels is bound by the host's launch rate and the comparison reads the host, not
        // the kernels (n_h = 128 at 4x4: eager 5 launches lose to the one launch, replayed they win 23 vs 27 us).  If the
        // capture is refused (a stream already capturing in this thread), the eager timing stands in.
        hipStream_t cs = nullptr;
        const bool own = possible && hipStreamSynchronize((hipStream_t)stream) == hipSuccess &&
                         hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) == hipSuccess;
        // (no early return inside this loop: fs_force, the capture stream and the events are restored / released on every path)
        for (int mode = 0; mode < 2 && possible && !rc; ++mode) {
            s->fs_force = mode;
            hipEvent_t e0 = nullptr, e1 = nullptr;
            hipGraphExec_t ge = nullptr;
            do {
                if ((rc = iaf_step_forward(s, z, context, z_new, logsd, B, H, W, workspace, workspace_bytes, stream))) break;
                if ((rc = (int)hipStreamSynchronize((hipStream_t)stream))) break;
                if (own && hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                    int crc = 0;
                    for (int r = 0; r < reps && !crc; ++r)
                        crc = iaf_step_forward(s, z, context, z_new, logsd, B, H, W, workspace, workspace_bytes, cs);
                    hipGraph_t g = nullptr;
                    const bool ended = hipStreamEndCapture(cs, &g) == hipSuccess && g;
                    if (ended && !crc && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) ge = nullptr;
                    if (g) (void)hipGraphDestroy(g);
                    (void)hipGetLastError();
                }
                hipStream_t ts = ge ? cs : (hipStream_t)stream;
                if (ge) { (void)hipGraphLaunch(ge, cs); (void)hipStreamSynchronize(cs); }      // (the first replay uploads the graph)
                if ((rc = (int)hipEventCreate(&e0)) || (rc = (int)hipEventCreate(&e1)) || (rc = (int)hipEventRecord(e0, ts))) break;
                if (ge) (void)hipGraphLaunch(ge, cs);
                else
                    for (int r = 0; r < reps && !rc; ++r)
                        rc = iaf_step_forward(s, z, context, z_new, logsd, B, H, W, workspace, workspace_bytes, stream);
                (void)hipEventRecord(e1, ts);
                (void)hipEventSynchronize(e1);
                (void)hipEventElapsedTime(&t[mode], e0, e1);
            } while (0);
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            if (ge) (void)hipGraphExecDestroy(ge);
        }
        if (cs) (void)hipStreamDestroy(cs);
        s->fs_force = -1;
        if (!rc && possible) { s->fs_P = P; s->fs_W = W; s->fs_on = t[1] < t[0]; }
        if (!rc && possible && s->fs_on && chosen) for (int l = 0; l < s->nlayers; ++l) chosen[l] = -2;   // -2: part of the one-launch step
        if (!rc && possible && s->fs_on && us) { for (int l = 0; l < s->nlayers; ++l) us[l] = 0.f; us[s->nlayers - 1] = 1e3f * t[1] / (float)reps; }
    }
    // the first masked conv fused into the second one's kernel: every shape that can carry it, against the two separate
    // launches (+ the launch boundary between them, which back-to-back timing of single kernels does not see)
    if (!rc && s->depth_ar >= 1 && s->fuse_first != 0 && !(s->fs_P == P && s->fs_W == W && s->fs_on)) {
        GemmLayer& L1 = s->L[1];
        L1.fz_P = -1;
        const int saved_mode = s->fuse_first;
        float best = 1e30f, ms = 0.f;
        int bz[5] = {0, 0, 0, 0, 1};
        static const int nts[3] = {5, 4, 2};
        for (int si = 0; si < (int)std::size(k_bf3_shapes) && !rc; ++si)
            for (int ni = 0; ni < 3 && !rc; ++ni) {
                const int nt = nts[ni];
                const auto& sh = k_bf3_shapes[si];
                if (!fuse_shape_ok(s, nt, sh.ppw, sh.pxt, sh.ks, sh.wco, W)) continue;
                L1.fz_P = P; L1.fz_W = W; L1.fz_on = true;
                L1.fz[0] = nt; L1.fz[1] = sh.ppw; L1.fz[2] = sh.pxt; L1.fz[3] = sh.ks; L1.fz[4] = sh.wco;
                s->fuse_first = 2;
                rc = iaf_step_time_layer(s, -1, z, context, z_new, logsd, B, H, W, workspace, workspace_bytes, reps, stream, &ms);
                if (rc == IAF_ERR_UNSUPPORTED) { rc = IAF_OK; continue; }
                if (!rc && ms < best) { best = ms; for (int i = 0; i < 5; ++i) bz[i] = L1.fz[i]; }
            }
        s->fuse_first = saved_mode;
        const float separate = s->L[0].tuned_us + L1.tuned_us + 1.0f;        // ~1 us: the boundary a fused launch removes
        L1.fz_P = P; L1.fz_W = W;
        L1.fz_on = (bz[0] != 0) && (1e3f * best < 0.90f * separate);         // only on a clear win (single timings are noisy)
        for (int i = 0; i < 5; ++i) L1.fz[i] = bz[i];
        if (L1.fz_on && chosen) { chosen[0] = -1; chosen[1] = bz[0] * 10000 + bz[1] * 1000 + bz[2] * 100 + bz[3] * 10 + bz[4]; }
        if (L1.fz_on && us) { us[0] = 0.f; us[1] = 1e3f * best; }
    }
    return rc;
}

extern "C" int iaf_stack_set_packs(iaf_stack_t* s, int packs) {
    if (!s) return IAF_ERR_NULL;
    if (s->resnet) return IAF_ERR_UNSUPPORTED;      // (iaf_stack_create_resnet: include/iaf_hip.h)
    PackFacts f;
    f.generic = s->generic; f.training = s->training; f.f16_active = f16_active(s);
    f.all_split = true;            // only a stack whose every layer has a bf16x3 pack can do without the fp32 one
    for (int l = 0; l < s->nlayers; ++l) f.all_split &= s->L[l].wp3 != nullptr;
    return pack_stack_set_packs(*s, packs, f);
}

extern "C" int iaf_stack_set_fuse_step(iaf_stack_t* s, int mode) {
    if (!s) return IAF_ERR_NULL;
    if (s->resnet) return IAF_ERR_UNSUPPORTED;      // (iaf_stack_create_resnet: include/iaf_hip.h)
    if (mode < 0 || mode > 2) return IAF_ERR_SHAPE;
    s->fuse_step = mode;
    return IAF_OK;
}

extern "C" int iaf_stack_step_is_fused(const iaf_stack_t* s, int B, int H, int W) {
    if (!s || B <= 0 || H <= 0 || W <= 0) return 0;
    int R = 0;
    size_t lds = 0;
    return fused_step_plan(s, B, H, W, &R, &lds) ? R : 0;
}

extern "C" int iaf_stack_set_fuse_first(iaf_stack_t* s, int mode) {
    if (!s) return IAF_ERR_NULL;
    if (s->resnet) return IAF_ERR_UNSUPPORTED;      // (iaf_stack_create_resnet: include/iaf_hip.h)
    if (mode < 0 || mode > 2) return IAF_ERR_SHAPE;
    s->fuse_first = mode;
    return IAF_OK;
}

extern "C" int iaf_ar_multiconv2d_forward(iaf_stack_t* s, const float* z, const float* context, float* m_raw,
                                          float* s_raw, int B, int H, int W, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    int rc = check_dims(s, B, H, W);
    if (rc) return rc;
    if (!z || !m_raw || !s_raw || (s->depth_ar > 0 && !context)) return IAF_ERR_NULL;
    Ws ws;
    if ((rc = carve_ws(s, B, H, W, workspace, workspace_bytes, &ws))) return rc;
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.B = B; p.H = H; p.W = W; p.HW = H * W; p.P = B * H * W;
    p.x = z; p.out0 = m_raw; p.out1 = s_raw; p.mode = MODE_RAW;
    return run_stack(s, p, IN_NCHW, context, nullptr, ws, (hipStream_t)stream);
}

extern "C" int iaf_step_forward(iaf_stack_t* s, const float* z, const float* context, float* z_new, float* logsd,
                                int B, int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_dims(s, B, H, W);
    if (rc) return rc;
    if (!z || !z_new || !logsd || (s->depth_ar > 0 && !context)) return IAF_ERR_NULL;
    Ws ws;
    if ((rc = carve_ws(s, B, H, W, workspace, workspace_bytes, &ws))) return rc;
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.B = B; p.H = H; p.W = W; p.HW = H * W; p.P = B * H * W;
    p.x = z; p.zin = z; p.out0 = z_new; p.out1 = logsd; p.mode = MODE_IAF;
    return run_stack(s, p, IN_NCHW, context, nullptr, ws, (hipStream_t)stream);
}

// Inverse of the IAF step: given the flow OUTPUT z, find z0 with (z0 - m(z0))/exp(s(z0)) = z.
// m, s at a position depend only on z0 at earlier positions of the autoregressive order, so the Jacobi iteration
//   z0 <- z * exp(s(z0)) + m(z0)
// fixes at least one more position per sweep (exact after at most H*W*n_z sweeps) and, because the reference scales
// m and s by 0.1, contracts to fp32 precision in a handful of sweeps; every sweep is one full-width run of the conv
// stack instead of H*W*n_z dependent scalar steps.
// The sweeps of one inverse are QUEUED: the residual check (every check_every sweeps and after the last) runs on the device, raises a word
// the remaining sweep launches read (the one-launch step kernel returns at once: ~2 us per skipped sweep instead of a sweep) and a last
// small launch moves the result into z0 -- no host synchronisation inside the call, so it can be captured into a hipGraph.
// d_out (optional, device, two words): sweeps run (int) and the last residual (float, -1 if tol = 0).
static int step_inverse_queue(iaf_stack_t* s, const float* z, const float* context, float* z0, float* logsd, int B, int H, int W,
                              const Ws& ws, int max_sweeps, float tol, int check_every, hipStream_t st, unsigned* d_out) {
    const size_t n = (size_t)B * s->n_z * H * W;
    // ping-pong between the caller's z0 and the workspace's kl_elem plane, arranged so that the last sweep lands in z0
    float* buf[2] = {z0, ws.kl_elem};
    InvCtl* ctl = (InvCtl*)ws.rowsum;                     // [B*n_z] floats are free during the inverse (>= 8 words: n_z >= 16)
    unsigned* out = d_out ? d_out : (unsigned*)ws.rowsum + 8;
    const bool checking = (tol > 0.f && check_every > 0);
    HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(InvCtl), st));
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.B = B; p.H = H; p.W = W; p.HW = H * W; p.P = B * H * W;
    p.zin = z; p.out1 = logsd; p.mode = MODE_INVERSE;
    int R = 0;
    size_t lds = 0;
    const bool skipping = checking && !s->generic && fused_step_plan(s, B, H, W, &R, &lds) != nullptr &&
                          ((((uintptr_t)context) & 15) == 0);
    p.inv_done = skipping ? &ctl->done : nullptr;
    const float* cur = z;                                 // initial guess z0 = z (m = 0, s = 0)
    int rc, k = 0;
    for (int done = 0; done < max_sweeps; ++done) {
        float* dst = buf[(max_sweeps - 1 - done) & 1];
        p.x = cur; p.out0 = dst;
        if ((rc = run_stack(s, p, IN_NCHW, context, nullptr, ws, st))) return rc;
        if (checking && (++k == check_every || done + 1 == max_sweeps)) {
            k = 0;
            // (a SMALL grid: every workgroup ends in two agent-scope atomics on one line -- 4096 of them took 30 us, 128 take 3)
            const unsigned cg = (unsigned)((n + 8191) / 8192) < 128u ? (unsigned)((n + 8191) / 8192) : 128u;
            hipLaunchKernelGGL(iaf_inverse_check_kernel, dim3(cg), dim3(256), 0, st, (const float*)dst, cur, n, ctl, tol, (unsigned)(done + 1));
        }
        cur = dst;
    }
    hipLaunchKernelGGL(iaf_inverse_finish_kernel, ew_grid(n), dim3(256), 0, st, (const float*)buf[1], z0, n, (const InvCtl*)ctl, max_sweeps,
                       skipping ? 1 : 0, checking ? 1 : 0, out);
    return (int)hipGetLastError();
}

extern "C" int iaf_step_inverse_device(iaf_stack_t* s, const float* z, const float* context, float* z0, float* logsd, int B, int H,
                                       int W, void* workspace, size_t workspace_bytes, int max_sweeps, float tol, int check_every,
                                       void* stream, unsigned* d_sweeps_residual) {
    int rc = check_dims(s, B, H, W);
    if (rc) return rc;
    if (!z || !z0 || !logsd || (s->depth_ar > 0 && !context)) return IAF_ERR_NULL;
    if (max_sweeps <= 0 || check_every < 0 || tol < 0.f) return IAF_ERR_SHAPE;
    Ws ws;
    if ((rc = carve_ws(s, B, H, W, workspace, workspace_bytes, &ws))) return rc;
    return step_inverse_queue(s, z, context, z0, logsd, B, H, W, ws, max_sweeps, tol, check_every, (hipStream_t)stream, d_sweeps_residual);
}

extern "C" int iaf_step_inverse(iaf_stack_t* s, const float* z, const float* context, float* z0, float* logsd, int B, int H,
                                int W, void* workspace, size_t workspace_bytes, int max_sweeps, float tol, int check_every,
                                void* stream, int* sweeps_done, float* residual) {
    int rc = check_dims(s, B, H, W);
    if (rc) return rc;
    if (!z || !z0 || !logsd || (s->depth_ar > 0 && !context)) return IAF_ERR_NULL;
    if (max_sweeps <= 0 || check_every < 0 || tol < 0.f) return IAF_ERR_SHAPE;
    Ws ws;
    if ((rc = carve_ws(s, B, H, W, workspace, workspace_bytes, &ws))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = step_inverse_queue(s, z, context, z0, logsd, B, H, W, ws, max_sweeps, tol, check_every, st, nullptr))) return rc;
    if (sweeps_done) *sweeps_done = max_sweeps;
    if (residual) *residual = -1.f;
    const bool checking = (tol > 0.f && check_every > 0);
    if (!checking || (!sweeps_done && !residual)) return IAF_OK;
    // the two numbers, the call's only synchronisation (behind ALL of its launches; a stream capture cannot read them: see iaf_step_inverse_device)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cs);
    if (cs != hipStreamCaptureStatusNone) { if (sweeps_done) *sweeps_done = -1; return IAF_OK; }
    unsigned two[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(two, (unsigned*)ws.rowsum + 8, sizeof(two), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (sweeps_done) *sweeps_done = (int)two[0];
    if (residual) memcpy(residual, &two[1], sizeof(float));
    return IAF_OK;
}

extern "C" int iaf_posterior_block_forward(iaf_stack_t* s, const float* qz_mean, const float* qz_logsd,
                                           const float* rz_mean, const float* rz_logsd, const float* pz_mean,
                                           const float* pz_logsd, const float* up_context,
                                           const float* down_context, const float* eps, float kl_min, float* z_out,
                                           float* kl_obj, float* kl_cost, float* kl_elem, int B, int H, int W,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    if (s && s->resnet) return IAF_ERR_UNSUPPORTED;      // (iaf_stack_create_resnet: include/iaf_hip.h; before any other answer)
    int rc = check_dims(s, B, H, W);
    if (rc) return rc;
    if (!qz_mean || !qz_logsd || !rz_mean || !rz_logsd || !pz_mean || !pz_logsd || !eps || !z_out || !kl_obj ||
        !kl_cost)
        return IAF_ERR_NULL;
    if (s->depth_ar > 0 && (!up_context || !down_context)) return IAF_ERR_NULL;
    if (B % s->fb_groups != 0) return IAF_ERR_SHAPE;
    Ws ws;
    if ((rc = carve_ws(s, B, H, W, workspace, workspace_bytes, &ws))) return rc;
    hipStream_t st = (hipStream_t)stream;
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.B = B; p.H = H; p.W = W; p.HW = H * W; p.P = B * H * W;
    p.qm = qz_mean; p.ql = qz_logsd; p.rm = rz_mean; p.rl = rz_logsd; p.pm = pz_mean; p.pl = pz_logsd; p.eps = eps;
    p.out0 = z_out; p.out1 = nullptr; p.kl_elem = kl_elem ? kl_elem : ws.kl_elem; p.mode = MODE_POSTERIOR;
    // One-launch step: its final loop leaves per-(row block, channel) sums of the KL elements in the first hidden-activation
    // buffer of the workspace (which this path does not use: the activations stay in LDS) and ONE small launch finishes the
    // reductions; the [B, n_z, H, W] KL tensor is written only if the caller asked for it.
    if (!s->generic && s->depth_ar > 0) {
        int R = 0;
        size_t lds = 0;
        const bool aligned = (((uintptr_t)up_context | (uintptr_t)down_context) & 15) == 0;
        if (step_fn_t fn = aligned ? fused_step_plan(s, B, H, W, &R, &lds, st, true) : nullptr) {
            const int nrb = (H + R - 1) / R;
            p.kl_elem = kl_elem;
            StepFin fin = {kl_obj, kl_cost, kl_min, false, nullptr};
            if ((rc = launch_fused_step(s, fn, R, lds, p, IN_POSTERIOR, up_context, down_context, st, nullptr, ws.hbuf[0], &fin))) return rc;
            if (fin.done) return IAF_OK;                       // the launch's last workgroup did the block's reductions too
            return launch_kl_from_parts(ws.hbuf[0], ws.rowsum, kl_obj, kl_cost, B, s->n_z, nrb, kl_min, nullptr, s->fb_groups, st);
        }
    }
    if ((rc = run_stack(s, p, IN_POSTERIOR, up_context, down_context, ws, st))) return rc;
    const int rows = B * s->n_z;
    hipLaunchKernelGGL(iaf_kl_rowsum_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, p.kl_elem, ws.rowsum, rows, H * W);
    hipLaunchKernelGGL(iaf_kl_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)ws.rowsum, kl_obj, kl_cost, B, s->n_z, kl_min,
                       (float*)nullptr, 0, (float*)nullptr, s->fb_groups);
    return (int)hipGetLastError();
}

// free bits on given KL elements (tf_train.py:77-85; models.py:455-466): kl_elem [B,C,H,W] -> kl_obj [B], kl_cost [B];
// scratch: B*C floats.  (These three take no stack, yet stay in this unit, not iaf_model_ops.hip: they launch the two kernels of the
// posterior block above and of launch_kl_from_parts, and a kernel is launched only from the unit that defines it.)
static int kl_free_bits_impl(const float* kl_elem, float* kl_obj, float* kl_cost, float* gate, int B, int C, int HW, float kl_min,
                             float* scratch, void* stream, int groups = 1) {
    if (!kl_elem || !kl_obj || !kl_cost || !scratch) return IAF_ERR_NULL;
    if (B <= 0 || C <= 0 || HW <= 0 || groups < 1 || groups > IAF_MAX_FREE_BITS_GROUPS || B % groups != 0) return IAF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int rows = B * C;
    hipLaunchKernelGGL(iaf_kl_rowsum_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, kl_elem, scratch, rows, HW);
    hipLaunchKernelGGL(iaf_kl_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)scratch, kl_obj, kl_cost, B, C, kl_min, gate,
                       0, (float*)nullptr, groups);
    return (int)hipGetLastError();
}
extern "C" int iaf_kl_free_bits(const float* kl_elem, float* kl_obj, float* kl_cost, int B, int C, int HW, float kl_min,
                                float* scratch, void* stream) {
    return kl_free_bits_impl(kl_elem, kl_obj, kl_cost, nullptr, B, C, HW, kl_min, scratch, stream);
}
// ... and the per-channel gate of the free bits (1 where mean_b sum_hw kl > kl_min: where max() passes the gradient), [C]
extern "C" int iaf_kl_free_bits_gate(const float* kl_elem, float* kl_obj, float* kl_cost, float* gate, int B, int C, int HW,
                                     float kl_min, float* scratch, void* stream) {
    if (!gate) return IAF_ERR_NULL;
    return kl_free_bits_impl(kl_elem, kl_obj, kl_cost, gate, B, C, HW, kl_min, scratch, stream);
}
// ... with the free-bits mean per contiguous group of B / groups rows; gate [groups][C] or NULL
extern "C" int iaf_kl_free_bits_grouped(const float* kl_elem, float* kl_obj, float* kl_cost, float* gate_or_null, int B, int C, int HW,
                                        int groups, float kl_min, float* scratch, void* stream) {
    return kl_free_bits_impl(kl_elem, kl_obj, kl_cost, gate_or_null, B, C, HW, kl_min, scratch, stream, groups);
}

// ---------------------------------------------------------------------------------------------
// training: forward that keeps the hidden activations + backward
// ---------------------------------------------------------------------------------------------
extern "C" int iaf_stack_set_training(iaf_stack_t* s, int on) {
    if (!s) return IAF_ERR_NULL;
    if (!on) { s->training = false; return IAF_OK; }
    if (s->generic) {         // channel counts outside the MFMA path: the direct backward kernels (iaf_kernels_generic.hpp) need no extra packs
        s->training = true;
        return IAF_OK;
    }
    for (int l = 0; l < s->nlayers; ++l)
        if (int rc = gemm_layer_set_training(s->L[l], s->T[l], NTAPS, false)) return rc;
    s->training = true;
    pack_set_training(*s);    // (training keeps every pack: iaf_stack_set_packs refuses training stacks)
    return IAF_OK;
}

// pixel ranges of the weight-gradient GEMM: as many as keep the grid within ONE round of 256 workgroups
// (grid.x = 5 taps * ceil(cin/32) ci pairs), at least 64 pixels each, at most 16 (the partial buffer is sized for 16)
// ---- launch plan of the weight-gradient GEMM --------------------------------------------------------------------
// wide-load shape (BW, NB) for `cout` packed output channels: 16-byte dY loads when cout % 64 == 0, 8-byte ones otherwise
static bool wgrad_wide_shape(int cout, int* bw, int* nb) {
    static const char* env = getenv("IAF_WGRAD_WIDE");       // dev knob: "0" = off, "BW,NB" = forced
    if (env && env[0] == '0') return false;
    if (env && sscanf(env, "%d,%d", bw, nb) == 2) return cout % (*bw * *nb * 16) == 0;
    if (cout % 32 != 0) return false;
    if (cout % 64 == 0) {
        const int n = cout / 64;
        *bw = 4;
        *nb = (n % 3 == 0) ? 3 : (n % 2 == 0) ? 2 : 1;
        if (*nb > 1 || n == 1) return true;
    }
    const int n = cout / 32;
    *bw = 2;
    for (int c = 7; c >= 1; --c)
        if (n % c == 0) { *nb = c; break; }
    return true;
}

struct WgradPlan { int bw, nb, ncot, gx, gz, nrange, bf3_ncob; };   // bf3_ncob > 0: iaf_wgrad_bf3_kernel<bf3_ncob>; bw > 0: iaf_wgrad_wide_kernel<bw, nb>; else iaf_wgrad_kernel<ncot>
constexpr int WGRAD_MAX_RANGES = 32;             // what the partial buffers hold

// Pixel ranges (the K split across workgroups; the partial buffer holds 16): a workgroup has ~5 us of fixed cost
// (launch, first loads, the LDS reduction, its partial), equal-sized workgroups run in lockstep rounds, and two resident
// workgroups per CU hide each other's load latency.  Measured on the layer's convs at 16x16 and 8x8 (B=32): 8 ranges
// when an operand-block sweep already has >= 40 workgroups (the 9-tap convs), 16 otherwise (the masked stack).
// bf16x3 weight gradient (iaf_wgrad_bf3.hip): used when the conv computes in bf16x3 and the kernel's tiling covers it;
// IAF_WGRAD_BF3=0 keeps the fp32 MFMA kernels (dev knob for A/B runs)
static bool wgrad_bf3_enabled() {
    static const bool on = !(getenv("IAF_WGRAD_BF3") && getenv("IAF_WGRAD_BF3")[0] == '0');
    return on;
}

static WgradPlan wgrad_plan(long long P, int cin, int cout, int ntaps, bool bf3 = false) {
    WgradPlan w;
    memset(&w, 0, sizeof(w));
    if (bf3 && wgrad_bf3_enabled() && P % 8 == 0 && P >= 64 && (w.bf3_ncob = iaf_wgrad_bf3_ncob(cin, cout)) > 0) {
        // a workgroup per (tap row, 32 input channels, output block, pixel range): enough ranges for TWO workgroups per CU (the
        // kernel's split phase and MFMA phase overlap across co-resident workgroups, not within one), at least two K blocks
        // of 32 pixels each
        const int rows = ntaps == MAXTAPS ? 3 : 2;
        w.gx = rows * (cin / 32);
        w.gz = (cout / 16) / w.bf3_ncob;
        static const int force = getenv("IAF_WGRAD_NRANGE") ? atoi(getenv("IAF_WGRAD_NRANGE")) : 0;               // dev knob
        long long n = 512 / (w.gx * w.gz);                   // two full rounds of CUs, else one (320 workgroups: 29 us, 250: 27 us)
        if (n > WGRAD_MAX_RANGES) n = 256 / (w.gx * w.gz);
        if (force > 0) n = force;
        if (n > WGRAD_MAX_RANGES) n = WGRAD_MAX_RANGES;
        if (n > P / 64) n = P / 64;
        if (n < 1) n = 1;
        w.nrange = (int)n;
        return w;
    }
    w.bf3_ncob = 0;
    w.gx = ntaps * ((cin + 31) / 32);
    const bool off32 = P * (cin > cout ? cin : cout) * 4 < (1LL << 32);      // the wide kernel's operand offsets are 32-bit
    if (off32 && cin % 16 == 0 && wgrad_wide_shape(cout, &w.bw, &w.nb)) {
        w.gz = cout / (w.bw * w.nb * 16);
    } else {
        static const int cand[] = {14, 12, 10, 8, 7, 6, 5, 4, 3, 2, 1};
        w.bw = w.nb = 0;
        w.ncot = 1;
        for (int c : cand)
            if ((cout / 16) % c == 0) { w.ncot = c; break; }
        w.gz = (cout / 16) / w.ncot;
    }
    static const int force = getenv("IAF_WGRAD_NRANGE") ? atoi(getenv("IAF_WGRAD_NRANGE")) : 0;               // dev knob
    long long n;
    if (force > 0 && force <= 16 && force <= P / 16) n = force;
    else if (P / 64 >= 16) n = (w.gx * w.gz >= 40) ? 8 : 16;
    else if (P / 64 >= 8) n = 8;
    else {
        n = 512 / w.gx;
        if (n > P / 64) n = P / 64;
        if (n < 1) n = 1;
    }
    w.nrange = (int)n;
    return w;
}
static int wgrad_nrange(long long P, int cin, int ntaps, int cout, bool bf3) { return wgrad_plan(P, cin, cout, ntaps, bf3).nrange; }

struct TrainWs {
    float* h[MAX_GEMM_LAYERS];
    float* da[MAX_GEMM_LAYERS];      // d a_l (packed pixel-major), one per hidden layer: all still needed by the single reduce
    float* dy3;
    float* zpm;
    float* part[MAX_GEMM_LAYERS];    // per layer: weight-gradient partials [nrange][NTAPS][cin][cout]
    float* dWeff[MAX_GEMM_LAYERS];   // per layer: reduced effective-weight gradient [NTAPS][cin][cout]
    float* dbp[MAX_GEMM_LAYERS];     // per layer: [<=256 slabs][cout] column sums of dY
    float* dbrd[MAX_GEMM_LAYERS];    // Theano statement, per layer: [<=256 slabs][4][cout] border-channel weight gradient partials
    // posterior block: saved forward values and backward temporaries, all NCHW [P*n_z] unless noted
    float* logsd; float* klelem; float* z0; float* dzt; float* dkl; float* dz0;
    float* rowsum;   // [B*n_z]  (P*n_z floats reserved: B <= P)
    float* gate;     // [fb_groups][n_z]
    unsigned short* tapmask;   // [P] border bits for the weight gradient
};

static size_t train_ws_floats(const iaf_stack_t* s, long long P, TrainWs* o, float* base) {
    size_t off = 0;
    auto take = [&](size_t n) { float* q = base ? base + off : nullptr; off += (n + 63) / 64 * 64; return q; };
    TrainWs t;
    for (int l = 0; l < s->depth_ar; ++l) t.h[l] = take((size_t)P * s->n_h);
    for (int l = 0; l < s->depth_ar; ++l) t.da[l] = take((size_t)P * s->n_h);
    t.dy3 = take((size_t)P * 2 * s->n_z);
    t.zpm = take((size_t)P * s->n_z);
    for (int l = 0; l < s->nlayers; ++l) {
        t.part[l] = take((size_t)WGRAD_MAX_RANGES * NTAPS * s->L[l].cin * s->L[l].cout);
        t.dWeff[l] = take((size_t)NTAPS * s->L[l].cin * s->L[l].cout);
        t.dbp[l] = take((size_t)256 * s->L[l].cout);
        t.dbrd[l] = (s->variant != IAF_VARIANT_TF) ? take((size_t)256 * (NTAPS - 1) * s->L[l].cout) : nullptr;
    }
    t.logsd = take((size_t)P * s->n_z); t.klelem = take((size_t)P * s->n_z); t.z0 = take((size_t)P * s->n_z);
    t.dzt = take((size_t)P * s->n_z); t.dkl = take((size_t)P * s->n_z); t.dz0 = take((size_t)P * s->n_z);
    t.rowsum = take((size_t)P * s->n_z);
    t.gate = take((size_t)s->fb_groups * s->n_z);
    t.tapmask = (unsigned short*)take(((size_t)P + 1) / 2);
    if (o) *o = t;
    return off;
}

extern "C" size_t iaf_stack_train_workspace_bytes(const iaf_stack_t* s, int B, int H, int W) {
    if (!s || B <= 0 || H <= 0 || W <= 0) return 0;
    return train_ws_floats(s, (long long)B * H * W, nullptr, nullptr) * sizeof(float);
}

extern "C" int iaf_step_forward_train(iaf_stack_t* s, const float* z, const float* context, float* z_new, float* logsd,
                                      int B, int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_dims(s, B, H, W);
    if (rc) return rc;
    if (!s->training) return IAF_ERR_NOT_PREPARED;
    if (!z || !z_new || !logsd || !workspace || (s->depth_ar > 0 && !context)) return IAF_ERR_NULL;
    if (((uintptr_t)workspace & 15) != 0 || workspace_bytes < iaf_stack_train_workspace_bytes(s, B, H, W)) return IAF_ERR_WORKSPACE;
    TrainWs tw;
    train_ws_floats(s, (long long)B * H * W, &tw, (float*)workspace);
    hipStream_t st = (hipStream_t)stream;
    ConvP base;
    memset(&base, 0, sizeof(base));
    base.B = B; base.H = H; base.W = W; base.HW = H * W; base.P = B * H * W;
    base.zin = z; base.out0 = z_new; base.out1 = logsd; base.mode = MODE_IAF;
    base.x = z;
    if (s->generic) { Ws none; memset(&none, 0, sizeof(none)); return run_stack_generic(s, base, IN_NCHW, context, nullptr, none, st, tw.h); }
    // masked ResNet: the stream lives in da[0] (free until the backward pass), h_D and what every conv reads in h[] (run_resnet)
    if (s->resnet) return run_resnet(s, base, context, nullptr, tw.da[0], tw.h[2 * s->resnet], nullptr, nullptr, tw.h, st);
    {   // the one-launch step, writing the hidden activations of the owned rows where the backward expects them
        int R = 0;
        size_t lds = 0;
        const bool aligned = ((uintptr_t)context & 15) == 0;
        if (step_fn_t fn = aligned ? fused_step_plan(s, B, H, W, &R, &lds, st, true) : nullptr)
            return launch_fused_step(s, fn, R, lds, base, IN_NCHW, context, nullptr, st, tw.h);
    }
    const float* cur = z;
    int inmode = IN_NCHW;
    for (int l = 0; l < s->depth_ar; ++l) {       // like run_stack, but every hidden activation gets its own buffer
        ConvP p = base;
        p.mode = 0;
        p.x = cur;
        p.ctx = (l == 0) ? context : nullptr;
        p.y = tw.h[l];
        if ((rc = launch_conv(s, l, p, inmode, st))) return rc;
        cur = p.y;
        inmode = IN_PIXMAJOR;
    }
    ConvP p = base;
    p.x = cur;
    return launch_conv(s, s->depth_ar, p, inmode, st);
}

// 1-D grid over (operand block, pixel range, output block), see wgrad_decode
static dim3 wgrad_grid(WgradP& p, int gx, int gz) {
    p.gx = gx; p.gz = gz;
    return dim3(gx * gz * p.nrange);
}

template <int NCOT>
static void launch_wgrad_t(WgradP& p, const WgradPlan& w, hipStream_t st) {
    const dim3 grid = wgrad_grid(p, w.gx, w.gz);
    const size_t lds = (size_t)4 * NCOT * 4 * 64 * sizeof(float);
    (void)raise_lds_cap((const void*)iaf_wgrad_kernel<NCOT, 2>, lds);
    hipLaunchKernelGGL((iaf_wgrad_kernel<NCOT, 2>), grid, dim3(256), lds, st, p);
}

template <int BW, int NB>
static void launch_wgrad_wide_t(WgradP& p, const WgradPlan& w, hipStream_t st) {
    const size_t lds = (size_t)4 * BW * NB * 4 * 64 * sizeof(float);
    const dim3 grid = wgrad_grid(p, w.gx, w.gz);
    (void)raise_lds_cap((const void*)iaf_wgrad_wide_kernel<BW, NB, 2>, lds);
    hipLaunchKernelGGL((iaf_wgrad_wide_kernel<BW, NB, 2>), grid, dim3(256), lds, st, p);
}

static int launch_tapmask(unsigned short* mask, int B, int H, int W, hipStream_t st) {
    const int P = B * H * W;
    hipLaunchKernelGGL(iaf_tapmask_kernel, dim3((P + 255) / 256), dim3(256), 0, st, mask, H, W, P);
    return (int)hipGetLastError();
}

// The border table depends only on (B, H, W): built once per device and shape, then shared by every backward call
// (it was a 4 us launch per layer per step).  First use allocates and synchronises, which a capturing stream must
// not do: then the caller's workspace copy is filled in-stream instead.
static int tapmask_for(int B, int H, int W, hipStream_t st, unsigned short* ws_copy, const unsigned short** out) {
    struct Key { int dev, B, H, W; bool operator<(const Key& o) const { return memcmp(this, &o, sizeof(Key)) < 0; } };
    static std::mutex mu;
    static std::map<Key, unsigned short*> cache;
    Key k{0, B, H, W};
    HIP_TRY(hipGetDevice(&k.dev));
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(k);
    if (it != cache.end()) { *out = it->second; return 0; }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cs);
    if (cs != hipStreamCaptureStatusNone) {
        *out = ws_copy;
        return launch_tapmask(ws_copy, B, H, W, st);
    }
    unsigned short* buf = nullptr;
    HIP_TRY(hipMalloc((void**)&buf, ((size_t)B * H * W + 1) / 2 * 4));
    int rc = launch_tapmask(buf, B, H, W, st);
    if (!rc) rc = (int)hipStreamSynchronize(st);
    if (rc) { (void)hipFree(buf); return rc; }
    cache[k] = buf;
    *out = buf;
    return 0;
}

// tap_sign = -1: the Theano statement's taps look left / above (launch_gemm)
// bf3: run the GEMM on the bf16 matrix cores (iaf_wgrad_bf3.hip) where its tiling covers the conv (wgrad_plan)
static int launch_wgrad(const iaf_stack_t* s, const GemmLayer& L, const float* x, const float* dy, float* part,
                        const unsigned short* tapmask, int B, int H, int W, hipStream_t st, int tap_sign = 1, bool bf3 = false) {
    WgradP p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.dy = dy; p.part = part; p.tapmask = tapmask;
    p.B = B; p.H = H; p.W = W; p.HW = H * W; p.P = B * H * W;
    p.cin = L.cin; p.cout = L.cout;
    const int ntaps = L.full3x3 ? MAXTAPS : NTAPS;
    p.ntaps = ntaps;
    const WgradPlan w = wgrad_plan(p.P, L.cin, L.cout, ntaps, bf3);
    p.nrange = w.nrange;
    static const int tf_dh[NTAPS] = {0, 0, 1, 1, 1}, tf_dw[NTAPS] = {0, 1, -1, 0, 1};
    for (int t = 0; t < ntaps; ++t) {
        p.tap_dh[t] = L.full3x3 ? t / 3 - 1 : tap_sign * tf_dh[t];
        p.tap_dw[t] = L.full3x3 ? t % 3 - 1 : tap_sign * tf_dw[t];
    }
    if (w.bf3_ncob) {
        p.px_per_range = (int)(((long long)p.P + p.nrange - 1) / p.nrange + 31) / 32 * 32;
        for (int t = 0; t < ntaps; ++t) {                    // tap rows: equal dh, in order of first appearance
            int gi = 0;
            while (gi < p.ngroups && p.grp_dh[gi] != p.tap_dh[t]) ++gi;
            if (gi == p.ngroups) { p.grp_dh[gi] = p.tap_dh[t]; p.grp_n[gi] = 0; ++p.ngroups; }
            p.grp_tap[gi][p.grp_n[gi]++] = t;
        }
        p.gx = w.gx; p.gz = w.gz;
        (void)s;
        return iaf_launch_wgrad_bf3(&p, w.bf3_ncob, st);
    }
    p.px_per_range = (int)(((long long)p.P + p.nrange - 1) / p.nrange + 15) / 16 * 16;
    if (w.bw) {
        switch (w.bw * 10 + w.nb) {
            case 41: launch_wgrad_wide_t<4, 1>(p, w, st); break;
            case 42: launch_wgrad_wide_t<4, 2>(p, w, st); break;
            case 43: launch_wgrad_wide_t<4, 3>(p, w, st); break;
            case 21: launch_wgrad_wide_t<2, 1>(p, w, st); break;
            case 22: launch_wgrad_wide_t<2, 2>(p, w, st); break;
            case 23: launch_wgrad_wide_t<2, 3>(p, w, st); break;
            case 24: launch_wgrad_wide_t<2, 4>(p, w, st); break;
            case 25: launch_wgrad_wide_t<2, 5>(p, w, st); break;
            case 26: launch_wgrad_wide_t<2, 6>(p, w, st); break;
            case 27: launch_wgrad_wide_t<2, 7>(p, w, st); break;
            default: return IAF_ERR_UNSUPPORTED;       // (a forced IAF_WGRAD_WIDE shape that is not compiled)
        }
        (void)s;
        return (int)hipGetLastError();
    }
    switch (w.ncot) {
        case 14: launch_wgrad_t<14>(p, w, st); break;
        case 12: launch_wgrad_t<12>(p, w, st); break;
        case 7: launch_wgrad_t<7>(p, w, st); break;
        case 10: launch_wgrad_t<10>(p, w, st); break;
        case 8: launch_wgrad_t<8>(p, w, st); break;
        case 6: launch_wgrad_t<6>(p, w, st); break;
        case 5: launch_wgrad_t<5>(p, w, st); break;
        case 4: launch_wgrad_t<4>(p, w, st); break;
        case 3: launch_wgrad_t<3>(p, w, st); break;
        case 2: launch_wgrad_t<2>(p, w, st); break;
        default: launch_wgrad_t<1>(p, w, st); break;
    }
    (void)s;
    return (int)hipGetLastError();
}

extern "C" int iaf_step_backward(iaf_stack_t* s, const float* z, const float* context, const float* z_new,
                                 const float* logsd, const float* dz_new, const float* dlogsd, float* dz, float* dcontext,
                                 const float* const* V, const float* const* g, float* const* dV, float* const* dg,
                                 float* const* db, int B, int H, int W, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    int rc = check_dims(s, B, H, W);
    if (rc) return rc;
    if (!s->training) return IAF_ERR_NOT_PREPARED;
    if (!z || !z_new || !logsd || !dz_new || !dlogsd || !dz || !V || !g || !dV || !dg || !db || !workspace) return IAF_ERR_NULL;
    if (s->depth_ar > 0 && (!context || !dcontext)) return IAF_ERR_NULL;
    for (int i = 0; i < s->depth_ar + 2; ++i)
        if (!V[i] || !g[i] || !dV[i] || !dg[i] || !db[i]) return IAF_ERR_NULL;
    if (((uintptr_t)workspace & 15) != 0 || workspace_bytes < iaf_stack_train_workspace_bytes(s, B, H, W)) return IAF_ERR_WORKSPACE;
    const int P = B * H * W, d = s->depth_ar;
    TrainWs tw;
    train_ws_floats(s, P, &tw, (float*)workspace);
    hipStream_t st = (hipStream_t)stream;
    if (s->generic) {
        // channel counts outside the MFMA path: the same four passes as direct loops over NCHW tensors (iaf_kernels_generic.hpp)
        const size_t nzel = (size_t)P * s->n_z;
        hipLaunchKernelGGL(iaf_generic_bwd_affine_kernel, ew_grid(nzel), dim3(256), 0, st, z_new, logsd, dz_new, dlogsd, tw.dy3, s->n_z, H * W, nzel);
        const float* dy = tw.dy3;
        for (int l = d; l >= 0; --l) {
            const GemmLayer& L = s->L[l];
            GenGradP p;
            memset(&p, 0, sizeof(p));
            p.dy[0] = dy; p.dy_end[0] = L.cout; p.ndy = 1; p.dy_scale = 1.f;
            p.x = (l == 0) ? z : tw.h[l - 1];
            p.w = L.wp; p.ntaps = NTAPS; p.B = B; p.H = H; p.W = W; p.cin = L.cin; p.cout = L.cout;
            p.ndx = 1; p.dx_end[0] = L.cin;
            if (l == 0) { p.dx[0] = dz; p.dzn = dz_new; p.logsd = logsd; }
            else { p.dx[0] = tw.da[l - 1]; p.act_out = tw.h[l - 1]; p.dx_copy = (l - 1 == 0) ? dcontext : nullptr; }
            p.dW = tw.dWeff[l]; p.db = tw.dbp[l];
            hipLaunchKernelGGL(iaf_generic_dgrad_kernel, ew_grid((size_t)P * L.cin), dim3(256), 0, st, p);
            hipLaunchKernelGGL(iaf_generic_wgrad_kernel, dim3((unsigned)((size_t)NTAPS * L.cin * L.cout + L.cout)), dim3(256), 0, st, p);
            GenWnBwdP wn;
            memset(&wn, 0, sizeof(wn));
            const bool pair = (l == d);
            for (int k = 0; k < (pair ? 2 : 1); ++k) {
                const int ci = pair ? d + k : l;
                wn.V[k] = V[ci]; wn.g[k] = g[ci]; wn.dV[k] = dV[ci]; wn.dg[k] = dg[ci]; wn.db[k] = db[ci];
            }
            wn.dW = tw.dWeff[l]; wn.dbsum = tw.dbp[l];
            wn.cin = L.cin; wn.cout_each = pair ? s->n_z : L.cout; wn.npair = pair ? 2 : 1; wn.zerodiag = L.zerodiag; wn.ntaps = NTAPS;
            hipLaunchKernelGGL(iaf_generic_wn_bwd_kernel, dim3(L.cout), dim3(256), 0, st, wn);
            if (l > 0) dy = tw.da[l - 1];
        }
        return (int)hipGetLastError();
    }

    // (1) affine + log-det backward -> packed pixel-major dY of the output GEMM, pixel-major copy of z
    {
        const long long total = (long long)P * s->n_z;
        long long blocks = (total + 255) / 256;
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(iaf_bwd_affine_kernel, dim3((unsigned)blocks), dim3(256), 0, st, z, z_new, logsd, dz_new, dlogsd,
                           tw.dy3, tw.zpm, s->n_z, H * W, total);
    }
    ConvP base;
    memset(&base, 0, sizeof(base));
    base.B = B; base.H = H; base.W = W; base.HW = H * W; base.P = P;

    const int nslab = (P + 31) / 32 < 256 ? (P + 31) / 32 : 256;
    const int px_per_slab = (P + nslab - 1) / nslab;
    ReduceArgs ra;                                  // one reduce launch for all layers, after the walk
    memset(&ra, 0, sizeof(ra));
    ra.nslab = nslab; ra.P = P; ra.px_per_slab = px_per_slab;
    auto reduce_add = [&](int l, const float* dy) {   // partials -> dWeff[l], dY column sums -> dbp[l]
        const GemmLayer& L = s->L[l];
        ReduceLayer& r = ra.L[ra.n++];
        r.part = tw.part[l]; r.dW = tw.dWeff[l]; r.n4 = (size_t)NTAPS * L.cin * L.cout / 4;
        r.nrange = wgrad_nrange(P, L.cin, NTAPS, L.cout, prec_split(s));
        int nblk = (int)((r.n4 + 255) / 256);
        if (nblk > 256) nblk = 256;
        r.blk_begin = ra.nblk_total;
        ra.nblk_total += nblk;
        r.dy = dy; r.dbp = tw.dbp[l]; r.cout = L.cout; r.dbrd = tw.dbrd[l];
    };
    const int tap_sign = (s->variant == IAF_VARIANT_THEANO) ? -1 : 1;
    WnBwdArgs wa;
    memset(&wa, 0, sizeof(wa));
    auto wn_add = [&](int conv_index, int l, int n_out_each, int pack_stride, int pack_off) {
        const GemmLayer& L = s->L[l];
        WnBwdLayer& w = wa.L[wa.n];
        w.V = V[conv_index]; w.g = g[conv_index];
        w.dW = tw.dWeff[l]; w.dbp = tw.dbp[l];
        w.dV = dV[conv_index]; w.dg = dg[conv_index]; w.db = db[conv_index];
        w.cin = L.cin; w.cout = n_out_each; w.cout_packed = L.cout; w.nslab = nslab; w.zerodiag = L.zerodiag;
        w.pack_stride = pack_stride; w.pack_off = pack_off;
        w.dbrd = tw.dbrd[l]; w.variant = s->variant;
        wa.tile_begin[wa.n + 1] = wa.tile_begin[wa.n] + n_out_each / 16;
        wa.n++;
    };

    const unsigned short* tapmask = nullptr;
    if ((rc = tapmask_for(B, H, W, st, tw.tapmask, &tapmask))) return rc;
    ra.tapmask = tapmask;
    {
        static const int tf_dh[NTAPS] = {0, 0, 1, 1, 1}, tf_dw[NTAPS] = {0, 1, -1, 0, 1};
        for (int t = 1; t < NTAPS; ++t) ra.brd_bit[t - 1] = (tap_sign * tf_dh[t] + 1) * 3 + (tap_sign * tf_dw[t] + 1);
    }
    // (2) walk the layers backwards: data gradient (same conv kernel on W^T, mirrored taps), then weight gradient
    const float* dy = tw.dy3;                       // gradient w.r.t. the output of layer l (packed pixel-major)
    for (int l = d; l >= 0; --l) {
        const float* x_in = (l == 0) ? tw.zpm : tw.h[l - 1];     // what layer l read in the forward pass
        ConvP p = base;
        p.x = dy;
        const int epi = layer_dgrad_epi(s, l);
        if (l == 0) {                               // dz = W_0^T dY + dz_new e^{-logsd}
            p.mode = MODE_DGRAD_Z;
            p.qm = dz_new; p.ql = logsd; p.out0 = dz;
        } else if (s->resnet && l == d) {           // masked ResNet: the output pair read the RAW stream: d h_D = W_out^T dY -> da[0], the
                                                    // stream's gradient from here on (updated in place); 0.1 d h_D = dY of the last conv2
            p.mode = MODE_DGRAD_RAW;
            p.y = tw.da[0]; p.y2 = tw.da[l - 1];
        } else if (s->resnet && (l & 1)) {          // conv1 of block i = (l - 1) / 2: d h_i = d h_{i+1} + elu'(h_i) (W^T d t_i); 0.1 d h_i = dY
                                                    // of block i - 1's conv2; block 0: d h_0 is the input conv's dY itself, and d context
            p.mode = MODE_DGRAD_SKIP;
            p.zin = tw.h[l - 1]; p.skip = tw.da[0];
            p.y = tw.da[0]; p.y2 = (l > 1) ? tw.da[l - 1] : nullptr;
            p.out0 = (l == 1) ? dcontext : nullptr;
        } else {                                    // d a_{l-1} = (W_l^T dY) elu'(h_{l-1})   (+ NCHW copy = d context)
            p.mode = MODE_DGRAD_ELU;
            p.zin = tw.h[l - 1];
            p.y = tw.da[l - 1];
            p.out0 = (l - 1 == 0) ? dcontext : nullptr;
        }
        if ((rc = launch_gemm(s, s->T[l], epi, true, -1, p, IN_PIXMAJOR, st))) return rc;
        if ((rc = launch_wgrad(s, s->L[l], x_in, dy, tw.part[l], tapmask, B, H, W, st, tap_sign, prec_split(s)))) return rc;
        reduce_add(l, dy);
        if (l == d) {
            wn_add(d, l, s->n_z, 2, 0);       // layer_out_0 (mean tiles)
            wn_add(d + 1, l, s->n_z, 2, 1);   // layer_out_1 (logsd tiles)
        } else {
            wn_add(l, l, s->L[l].cout, 1, 0);
        }
        if (l > 0) dy = tw.da[l - 1];
    }
    hipLaunchKernelGGL(iaf_wgrad_reduce_multi_kernel, dim3(ra.nblk_total + ra.n * nslab), dim3(256), 0, st, ra);
    // (3) mask + weight-norm backward of every conv of the stack in one launch -- or left to iaf_wn_bwd_batch_run
    if (s->defer_wn) {
        s->pend_ws = (float*)workspace; s->pend_B = B; s->pend_H = H; s->pend_W = W;
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(iaf_wn_bwd_kernel, dim3(wa.tile_begin[wa.n]), dim3(256), 0, st, wa);
    return (int)hipGetLastError();
}

// ---- deferred weight-norm backward of many stacks in one launch ------------------------------------------------
extern "C" int iaf_stack_set_defer_weightnorm(iaf_stack_t* s, int on) {
    if (!s) return IAF_ERR_NULL;
    s->defer_wn = on != 0;
    s->pend_ws = nullptr;
    return IAF_OK;
}

struct iaf_wn_bwd_batch {
    std::vector<iaf_stack*> stacks;
    BatchTable<WnBwdLayer> t;      // one descriptor per conv of every stack, in the conv order of iaf_stack_prepare
};

extern "C" int iaf_wn_bwd_batch_destroy(iaf_wn_bwd_batch_t* b) {
    if (!b) return IAF_ERR_NULL;
    b->t.destroy();
    delete b;
    return IAF_OK;
}

extern "C" int iaf_wn_bwd_batch_create(iaf_wn_bwd_batch_t** out, iaf_stack_t* const* stacks, int n) {
    if (!out || !stacks) return IAF_ERR_NULL;
    *out = nullptr;
    if (n <= 0) return IAF_ERR_SHAPE;
    std::vector<int> tiles;
    for (int i = 0; i < n; ++i) {
        if (!stacks[i]) return IAF_ERR_NULL;
        if (stacks[i]->generic) return IAF_ERR_UNSUPPORTED;
        for (int c = 0; c < stacks[i]->depth_ar + 2; ++c)      // output pair: n_z / 16 tiles for each of its two convs
            tiles.push_back((c < stacks[i]->depth_ar ? stacks[i]->L[c].cout : stacks[i]->n_z) / 16);
    }
    iaf_wn_bwd_batch* b = new (std::nothrow) iaf_wn_bwd_batch();
    if (!b) return (int)hipErrorOutOfMemory;
    b->stacks.assign(stacks, stacks + n);
    if (int rc = b->t.create(tiles, true)) { iaf_wn_bwd_batch_destroy(b); return rc; }
    int ci = 0;
    for (const iaf_stack* s : b->stacks)
        for (int c = 0; c < s->depth_ar + 2; ++c, ++ci) {
            const int l = c < s->depth_ar ? c : s->depth_ar;
            const GemmLayer& L = s->L[l];
            WnBwdLayer& w = b->t.h[ci];
            const bool pair = (l == s->depth_ar);
            w.cin = L.cin; w.cout = pair ? s->n_z : L.cout; w.cout_packed = L.cout; w.zerodiag = L.zerodiag;
            w.pack_stride = pair ? 2 : 1; w.pack_off = pair ? c - s->depth_ar : 0;
            w.variant = s->variant;
        }
    *out = b;
    return IAF_OK;
}

extern "C" int iaf_wn_bwd_batch_run(iaf_wn_bwd_batch_t* b, const float* const* V, const float* const* g, float* const* dV,
                                    float* const* dg, float* const* db, void* stream) {
    if (!b || !V || !g || !dV || !dg || !db) return IAF_ERR_NULL;
    int ci = 0;
    for (const iaf_stack* s : b->stacks) {
        if (!s->defer_wn || !s->pend_ws) return IAF_ERR_NOT_PREPARED;      // no deferred backward pending on this stack
        const long long P = (long long)s->pend_B * s->pend_H * s->pend_W;
        TrainWs tw;
        train_ws_floats(s, P, &tw, s->pend_ws);
        const int nslab = (P + 31) / 32 < 256 ? (int)((P + 31) / 32) : 256;
        for (int c = 0; c < s->depth_ar + 2; ++c, ++ci) {
            if (!V[ci] || !g[ci] || !dV[ci] || !dg[ci] || !db[ci]) return IAF_ERR_NULL;
            const int l = c < s->depth_ar ? c : s->depth_ar;
            b->t.set(ci, [&](WnBwdLayer& w) {
                w.V = V[ci]; w.g = g[ci]; w.dV = dV[ci]; w.dg = dg[ci]; w.db = db[ci];
                w.dW = tw.dWeff[l]; w.dbp = tw.dbp[l]; w.dbrd = tw.dbrd[l]; w.nslab = nslab;
            });
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const WnBwdLayer* d_layers = nullptr;
    if (int rc = b->t.upload(st, &d_layers)) return rc;
    hipLaunchKernelGGL(iaf_wn_bwd_batch_kernel, dim3(b->t.ntiles), dim3(256), 0, st, d_layers, b->t.d_tile2layer, b->t.d_tile_begin);
    return (int)hipGetLastError();
}

extern "C" int iaf_posterior_block_forward_train(iaf_stack_t* s, const float* qz_mean, const float* qz_logsd,
                                                 const float* rz_mean, const float* rz_logsd, const float* pz_mean,
                                                 const float* pz_logsd, const float* up_context, const float* down_context,
                                                 const float* eps, float kl_min, float* z_out, float* kl_obj, float* kl_cost,
                                                 int B, int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
    if (s && s->resnet) return IAF_ERR_UNSUPPORTED;      // (iaf_stack_create_resnet: include/iaf_hip.h; before any other answer)
    int rc = check_dims(s, B, H, W);
    if (rc) return rc;
    if (!s->training) return IAF_ERR_NOT_PREPARED;
    if (!qz_mean || !qz_logsd || !rz_mean || !rz_logsd || !pz_mean || !pz_logsd || !eps || !z_out || !kl_obj || !kl_cost ||
        !workspace)
        return IAF_ERR_NULL;
    if (s->depth_ar > 0 && (!up_context || !down_context)) return IAF_ERR_NULL;
    if (B % s->fb_groups != 0) return IAF_ERR_SHAPE;
    if (((uintptr_t)workspace & 15) != 0 || workspace_bytes < iaf_stack_train_workspace_bytes(s, B, H, W)) return IAF_ERR_WORKSPACE;
    TrainWs tw;
    train_ws_floats(s, (long long)B * H * W, &tw, (float*)workspace);
    hipStream_t st = (hipStream_t)stream;
    ConvP base;
    memset(&base, 0, sizeof(base));
    base.B = B; base.H = H; base.W = W; base.HW = H * W; base.P = B * H * W;
    base.qm = qz_mean; base.ql = qz_logsd; base.rm = rz_mean; base.rl = rz_logsd; base.pm = pz_mean; base.pl = pz_logsd;
    base.eps = eps;
    base.out0 = z_out; base.out1 = tw.logsd; base.kl_elem = tw.klelem; base.mode = MODE_POSTERIOR;
    {
        int R = 0;
        size_t lds = 0;
        const bool aligned = (((uintptr_t)up_context | (uintptr_t)down_context) & 15) == 0;
        if (step_fn_t fn = aligned ? fused_step_plan(s, B, H, W, &R, &lds, st, true) : nullptr) {
            // (the backward never reads the KL tensor: its buffer takes the per-row-block partial sums instead)
            base.kl_elem = nullptr;
            StepFin fin = {kl_obj, kl_cost, kl_min, false, tw.gate};
            if ((rc = launch_fused_step(s, fn, R, lds, base, IN_POSTERIOR, up_context, down_context, st, tw.h, tw.klelem, &fin))) return rc;
            if (fin.done) return IAF_OK;
            return launch_kl_from_parts(tw.klelem, tw.rowsum, kl_obj, kl_cost, B, s->n_z, (H + R - 1) / R, kl_min, tw.gate, s->fb_groups, st);
        }
    }
    if (s->generic) {
        Ws none; memset(&none, 0, sizeof(none));
        if ((rc = run_stack_generic(s, base, IN_POSTERIOR, up_context, down_context, none, st, tw.h))) return rc;
    } else {
        const float* cur = nullptr;
        int inmode = IN_POSTERIOR;
        for (int l = 0; l < s->depth_ar; ++l) {
            ConvP p = base;
            p.x = cur;
            p.ctx = (l == 0) ? up_context : nullptr;
            p.ctx2 = (l == 0) ? down_context : nullptr;
            p.y = tw.h[l];
            if ((rc = launch_conv(s, l, p, inmode, st))) return rc;
            cur = p.y;
            inmode = IN_PIXMAJOR;
        }
        ConvP p = base;
        p.x = cur;
        if ((rc = launch_conv(s, s->depth_ar, p, inmode, st))) return rc;
    }
    const int rows = B * s->n_z;
    hipLaunchKernelGGL(iaf_kl_rowsum_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, tw.klelem, tw.rowsum, rows, H * W);
    hipLaunchKernelGGL(iaf_kl_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)tw.rowsum, kl_obj, kl_cost, B, s->n_z, kl_min, tw.gate, 0,
                       (float*)nullptr, s->fb_groups);
    return (int)hipGetLastError();
}

extern "C" int iaf_posterior_block_backward(iaf_stack_t* s, const float* qz_mean, const float* qz_logsd, const float* rz_mean,
                                            const float* rz_logsd, const float* pz_mean, const float* pz_logsd,
                                            const float* eps, float kl_min, const float* z, const float* dz,
                                            const float* dkl_obj, float* dmean, float* dlogsd_q, float* dpz_mean,
                                            float* dpz_logsd, float* dcontext, const float* const* V, const float* const* g,
                                            float* const* dV, float* const* dg, float* const* db, int B, int H, int W,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    if (s && s->resnet) return IAF_ERR_UNSUPPORTED;      // (iaf_stack_create_resnet: include/iaf_hip.h; before any other answer)
    int rc = check_dims(s, B, H, W);
    if (rc) return rc;
    if (!s->training) return IAF_ERR_NOT_PREPARED;
    if (!qz_mean || !qz_logsd || !rz_mean || !rz_logsd || !pz_mean || !pz_logsd || !eps || !z || !dkl_obj || !dmean ||
        !dlogsd_q || !dpz_mean || !dpz_logsd || !workspace)
        return IAF_ERR_NULL;
    if (B % s->fb_groups != 0) return IAF_ERR_SHAPE;
    if (((uintptr_t)workspace & 15) != 0 || workspace_bytes < iaf_stack_train_workspace_bytes(s, B, H, W)) return IAF_ERR_WORKSPACE;
    TrainWs tw;
    train_ws_floats(s, (long long)B * H * W, &tw, (float*)workspace);
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)B * s->n_z * H * W;
    // the free-bits gate [groups][n_z] was left in the workspace by iaf_posterior_block_forward_train (same kl_min, same groups)
    hipLaunchKernelGGL(iaf_post_bwd_pre_kernel, ew_grid(n), dim3(256), 0, st, qz_mean, qz_logsd, rz_mean, rz_logsd, pz_mean,
                       pz_logsd, eps, z, dz, tw.gate, dkl_obj, kl_min, tw.z0, tw.dzt, tw.dkl, dpz_mean, dpz_logsd, B, s->n_z,
                       H * W, n, s->fb_groups);
    if ((rc = (int)hipGetLastError())) return rc;
    // core: z := z0, (z_new, logsd) := saved forward values, incoming gradients := (dz_tot, dkl)
    if ((rc = iaf_step_backward(s, tw.z0, dcontext /* value unused */, z, tw.logsd, tw.dzt, tw.dkl, tw.dz0, dcontext, V, g, dV, dg,
                                db, B, H, W, workspace, workspace_bytes, stream)))
        return rc;
    hipLaunchKernelGGL(iaf_post_bwd_post_kernel, ew_grid(n), dim3(256), 0, st, qz_mean, rz_mean, tw.z0, tw.dz0, tw.dkl, dmean,
                       dlogsd_q, n);
    return (int)hipGetLastError();
}

extern "C" int iaf_layer_work(const iaf_stack_t* s, int layer, int B, int H, int W, double* live_flops,
                              double* dense_flops, double* bytes) {
    if (!s) return IAF_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || layer < 0 || layer >= s->nlayers) return IAF_ERR_SHAPE;
    const GemmLayer& L = s->L[layer];
    const double px = (double)B * H * W;
    if (live_flops) *live_flops = 2.0 * L.live_macs_per_px * px;
    if (dense_flops) *dense_flops = 2.0 * L.dense_macs_per_px * px;
    if (bytes) {
        double b = 4.0 * px * L.cin;                                     // activations in
        if (layer == s->depth_ar) b += 4.0 * px * (3.0 * s->n_z);         // z in, z_new out, logsd out
        else if (s->resnet && layer % 2 == 0)                             // EPI_RES: raw stream out, context (layer 0) or skip in, and
            b += 4.0 * px * L.cout * (layer == s->depth_ar - 1 ? 2.0 : 3.0);   // elu(stream) out unless the block is the last
        else b += 4.0 * px * L.cout * (layer == 0 ? 2.0 : 1.0);           // hidden out (+ context in)
        b += 4.0 * ((double)L.nchunk * NTAPS * L.ncot * 256 + L.cout);    // packed weights + bias, once
        *bytes = b;
    }
    return IAF_OK;
}

extern "C" int iaf_step_work(const iaf_stack_t* s, int B, int H, int W, double* live_flops, double* dense_flops,
                             double* bytes) {
    if (!s) return IAF_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0) return IAF_ERR_SHAPE;
    const double px = (double)B * H * W;
    double live = 0, dense = 0;
    for (int l = 0; l < s->nlayers; ++l) { live += s->L[l].live_macs_per_px; dense += s->L[l].dense_macs_per_px; }
    if (live_flops) *live_flops = 2.0 * live * px;
    if (dense_flops) *dense_flops = 2.0 * dense * px;
    // fused algorithmic bytes: z in, context in, z out, s out + raw weights once
    if (bytes) *bytes = 4.0 * (3.0 * s->n_z + (s->depth_ar > 0 ? s->n_h : 0)) * px + (double)s->weight_bytes;
    return IAF_OK;
}

#include "iaf_conv3x3_host.hpp"
