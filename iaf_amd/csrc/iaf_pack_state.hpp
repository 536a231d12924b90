// iaf_pack_state.hpp -- the ONE statement of the pack / precision / range protocol of the two host objects that own packed weights:
// iaf_stack (the masked stack, iaf_engine.hip) and iaf_conv3x3 (the plain convs, iaf_conv3x3_host.hpp).  Both embed PackState (as a base:
// s->packs, c->f16_off, ...) and take every decision about "which packs exist / which arithmetic runs" through the plain functions below.
// Nothing here needs HIP: the header includes include/iaf_hip.h and the C++ standard library only, and tests/c_abi/iaf_pack_state_walk.cpp
// walks the protocol on a CPU (tests/test_pack_state.py).  The HIP half -- the mapped pinned range word itself -- is RangeWord in
// iaf_engine.hip; the functions here are given the word's VALUE.
//
// The protocol.  An object has up to three packs of its weights: fp32 (IAF_PACK_F32), three bf16 planes (IAF_PACK_BF16X3), two fp16 planes
// (IAF_PACK_F16X2).  `packs` says which of them the prep launches keep up to date; a launch that needs another one returns
// IAF_ERR_NOT_PREPARED.  `precision` IAF_PRECISION_F16X2 asks for the fp16 planes; a launch on them that meets an operand beyond 65504 raises
// the range word.  The object's NEXT eager call sees it (pack_range_report): it returns IAF_ERR_RANGE once, the object runs bf16x3 from
// then on (f16_off), behind another prepare where the bf16x3 pack was not being kept, until set_precision(F16X2) re-arms it
// (pack_set_precision).  `prepared` falls whenever a pack that a launch may read next has not been kept up to date.
//
// Where the stack's and the conv's rules DIFFER (kept as they were; each row is a `kind` branch or one of the two set_packs functions below):
//
//                                   | stack (PACK_STACK)                               | conv (PACK_CONV)
//   --------------------------------+--------------------------------------------------+--------------------------------------------------
//   IAF_PACK_F16X2 in a mask        | refused (UNSUPPORTED) unless precision is F16X2; | accepted under any precision; IS the switch of the
//                                   | otherwise ignored: the fp16 pack is written      | fp16 pack (written when the bit is set AND fp16 is
//                                   | whenever fp16 is active (stored bit always set)  | active)
//   mask 0                          | IAF_ERR_SHAPE (as every mask without BF16X3 that | IAF_ERR_SHAPE
//                                   | is not exactly {F16X2} on an fp16-active stack)  |
//   mask without BF16X3             | only {F16X2} while fp16 is active, else SHAPE    | any non-empty mask; {F16X2} alone needs fp16 active
//                                   |                                                  | (UNSUPPORTED otherwise)
//   mask without F32                | needs a split pack on EVERY layer, not generic,  | {BF16X3 without F32} needs the split pack
//                                   | not training (UNSUPPORTED)                       | (UNSUPPORTED)
//   partial mask refused for        | generic, training                                | generic, masked, training, deconv-prepared
//   `prepared` falls in set_packs   | when the F32 or the BF16X3 bit CHANGES, either   | only when a pack is ADDED
//                                   | way                                              |
//   fp32 pack skipped by a prep     | only for layers that have a split pack           | whenever the bit is clear
//   bf16x3 pack skipped by a prep   | only while fp16 is active                        | whenever the bit is clear
//   transposed fp32 pack (wpt)      | written whenever it exists                       | written while training
//   range failure, BF16X3 not kept  | BF16X3 comes back (F32 stays as it was)          | ALL packs come back
//   leaving F16X2, BF16X3 not kept  | BF16X3 comes back, `prepared` falls              | nothing (the mask stays; {F16X2} alone then leaves no
//                                   |                                                  | pack a launch may read: NOT_PREPARED until set_packs)
#pragma once

#include "iaf_hip.h"

#define IAF_PACK_ALL (IAF_PACK_F32 | IAF_PACK_BF16X3 | IAF_PACK_F16X2)

enum PackKind { PACK_STACK, PACK_CONV };

struct PackState {
    int precision = IAF_PRECISION_BF16X3;
    int packs = IAF_PACK_ALL;      // IAF_PACK_* mask: which packs the prep launches keep up to date
    bool f16_off = false;          // a range failure was reported: bf16x3 until set_precision(F16X2) re-arms
    bool prepared = false;
};

// the precision asks for the fp16 planes and no range failure stands against them (f16_active / conv_f16_active add the object's own
// conditions: the pack exists, not generic, not masked)
static inline bool pack_f16_wanted(const PackState& st) { return st.precision == IAF_PRECISION_F16X2 && !st.f16_off; }

// what the object is, as far as set_packs cares
struct PackFacts {
    bool generic = false, training = false;
    bool all_split = false;        // stack: every layer has a bf16x3 pack; conv: it has one
    bool f16_active = false;
    bool masked = false, deconv = false;   // conv only
};

// iaf_stack_set_packs: the IAF_* code; st changes on IAF_OK only
static inline int pack_stack_set_packs(PackState& st, int packs, const PackFacts& f) {
    if (packs & ~IAF_PACK_ALL) return IAF_ERR_SHAPE;
    if ((packs & IAF_PACK_F16X2) && st.precision != IAF_PRECISION_F16X2) return IAF_ERR_UNSUPPORTED;
    if (!(packs & IAF_PACK_BF16X3) && !(packs == IAF_PACK_F16X2 && f.f16_active)) return IAF_ERR_SHAPE;
    if ((~packs & (IAF_PACK_F32 | IAF_PACK_BF16X3)) && (f.generic || f.training)) return IAF_ERR_UNSUPPORTED;
    if (!(packs & IAF_PACK_F32) && !f.all_split) return IAF_ERR_UNSUPPORTED;
    const int kept = (packs & (IAF_PACK_F32 | IAF_PACK_BF16X3)) | IAF_PACK_F16X2;
    if (kept != st.packs) st.prepared = false;               // the next prepare brings the pack set up to date
    st.packs = kept;
    return IAF_OK;
}

// iaf_conv3x3_set_packs
static inline int pack_conv_set_packs(PackState& st, int packs, const PackFacts& f) {
    if ((packs & ~IAF_PACK_ALL) || !packs) return IAF_ERR_SHAPE;
    if (packs != IAF_PACK_ALL && (f.generic || f.masked || f.training || f.deconv)) return IAF_ERR_UNSUPPORTED;
    if ((packs & IAF_PACK_BF16X3) && !(packs & IAF_PACK_F32) && !f.all_split) return IAF_ERR_UNSUPPORTED;
    if (packs == IAF_PACK_F16X2 && !f.f16_active) return IAF_ERR_UNSUPPORTED;
    if (packs & ~st.packs) st.prepared = false;              // a pack that was not kept up to date comes back: the next prepare fills it
    st.packs = packs;
    return IAF_OK;
}

// which packs of a layer a prep launch writes (rng_err goes with wp2); has_split: this layer has a bf16x3 pack
struct PackWrites { bool wp, wp3, wp2, wpt; };
static inline PackWrites pack_prep_writes(const PackState& st, PackKind kind, bool f16_active, bool has_split, bool training) {
    const bool f32 = st.packs & IAF_PACK_F32, bf3 = st.packs & IAF_PACK_BF16X3, f16 = st.packs & IAF_PACK_F16X2;
    if (kind == PACK_STACK) return {f32 || !has_split, bf3 || !f16_active, f16_active, true};
    return {f32, bf3, f16 && f16_active, training};
}

// the range word's value at the start of an eager call: true = return IAF_ERR_RANGE now (said once)
static inline bool pack_range_report(PackState& st, PackKind kind, unsigned word) {
    if (!pack_f16_wanted(st) || !word) return false;
    st.f16_off = true;
    if (!(st.packs & IAF_PACK_BF16X3)) {                     // the bf16x3 pack was not kept up to date: behind the next prepare
        st.packs = kind == PACK_STACK ? (st.packs | IAF_PACK_BF16X3) : IAF_PACK_ALL;
        st.prepared = false;
    }
    return true;
}

// set_precision, behind the object's own refusals and allocations.  new_f16_pack: the fp16 pack was allocated by this call; word: the
// range word's value.  Returns true if the word is to be cleared (re-armed after a range failure: synchronise, then zero it).
static inline bool pack_set_precision(PackState& st, PackKind kind, int precision, bool new_f16_pack, unsigned word) {
    bool rearm = false;
    if (precision == IAF_PRECISION_F16X2) {
        rearm = st.f16_off || word;
        st.f16_off = false;
        if (new_f16_pack || rearm || st.precision != IAF_PRECISION_F16X2) st.prepared = false;   // the fp16 pack has not been kept up to date
    } else if (kind == PACK_STACK && !(st.packs & IAF_PACK_BF16X3)) {
        st.packs |= IAF_PACK_BF16X3;                         // (the bf16x3 pack is wanted again)
        st.prepared = false;
    }
    st.precision = precision;
    return rearm;
}

// set_training(on) of an object on the MFMA path: training keeps every pack, the transposed ones are written by the next prepare
static inline void pack_set_training(PackState& st) {
    st.packs = IAF_PACK_ALL;
    st.prepared = false;
}
