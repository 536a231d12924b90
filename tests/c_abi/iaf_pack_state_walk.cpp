// Walks the pack / precision / range protocol of iaf_pack_state.hpp on a CPU (tests/test_pack_state.py compiles this with
// -fsanitize=address,undefined and runs it).  After every step: the IAF_* code or answer, packs, f16_off, prepared.
// The expected values are those of the stack's and the conv's entry points as they stood before the two shared this header.
#include "iaf_pack_state.hpp"

#include <cstdio>
#include <cstdlib>

static const int F32 = IAF_PACK_F32, BF3 = IAF_PACK_BF16X3, F16 = IAF_PACK_F16X2, ALL = IAF_PACK_ALL;
static const int OK = IAF_OK, SHAPE = IAF_ERR_SHAPE, UNSUP = IAF_ERR_UNSUPPORTED;
static int g_checks = 0;

#define EXPECT(got, want)                                                                              \
    do {                                                                                               \
        ++g_checks;                                                                                    \
        if ((long)(got) != (long)(want)) {                                                             \
            fprintf(stderr, "%s:%d: %s = %ld, expected %ld\n", __FILE__, __LINE__, #got, (long)(got), (long)(want)); \
            exit(1);                                                                                   \
        }                                                                                              \
    } while (0)
// the state after a step
#define STATE(st, prec_, packs_, off_, prepared_)                                                      \
    do { EXPECT((st).precision, prec_); EXPECT((st).packs, packs_); EXPECT((st).f16_off, off_); EXPECT((st).prepared, prepared_); } while (0)

static const int P_F32 = IAF_PRECISION_F32, P_BF3 = IAF_PRECISION_BF16X3, P_F16 = IAF_PRECISION_F16X2;

// a plain conv with a split pack, switched to the fp16 planes and prepared (what conv3x3_create + prepare leave)
static PackState conv_f16_prepared(PackFacts* f) {
    PackState st;
    STATE(st, P_BF3, ALL, false, false);
    EXPECT(pack_set_precision(st, PACK_CONV, P_F16, true, 0u), false);     // the fp16 pack is new: the next prepare fills it
    STATE(st, P_F16, ALL, false, false);
    st.prepared = true;
    *f = PackFacts();
    f->all_split = true; f->f16_active = true;
    return st;
}
// ... and the BASELINE stack (every layer has a split pack)
static PackState stack_f16_prepared(PackFacts* f) {
    PackState st;
    EXPECT(pack_set_precision(st, PACK_STACK, P_F16, true, 0u), false);
    STATE(st, P_F16, ALL, false, false);
    st.prepared = true;
    *f = PackFacts();
    f->all_split = true; f->f16_active = true;
    return st;
}

static void conv_fp16_only_range_failure() {
    PackFacts f;
    PackState st = conv_f16_prepared(&f);
    EXPECT(pack_conv_set_packs(st, F16, f), OK);
    STATE(st, P_F16, F16, false, true);                      // a pack dropped: nothing to refill
    EXPECT(pack_range_report(st, PACK_CONV, 0u), false);
    STATE(st, P_F16, F16, false, true);
    EXPECT(pack_range_report(st, PACK_CONV, 1u), true);      // said once ...
    STATE(st, P_F16, ALL, true, false);                      // ... bf16x3 from here on, every pack back behind another prepare
    EXPECT(pack_range_report(st, PACK_CONV, 1u), false);     // a second look reports nothing
    STATE(st, P_F16, ALL, true, false);
    EXPECT(pack_f16_wanted(st), false);
}

static void conv_bf16x3_kept_range_failure() {
    PackFacts f;
    PackState st = conv_f16_prepared(&f);
    EXPECT(pack_conv_set_packs(st, BF3 | F16, f), OK);
    STATE(st, P_F16, BF3 | F16, false, true);
    EXPECT(pack_range_report(st, PACK_CONV, 2u), true);
    STATE(st, P_F16, BF3 | F16, true, true);                 // packs and prepared untouched: the bf16x3 pack is up to date
    EXPECT(pack_range_report(st, PACK_CONV, 2u), false);
    // no report under another precision, whatever the word says
    PackState b;
    b.prepared = true;
    EXPECT(pack_range_report(b, PACK_CONV, 1u), false);
    STATE(b, P_BF3, ALL, false, true);
}

static void conv_set_packs_changes() {
    PackFacts f;
    PackState st = conv_f16_prepared(&f);
    EXPECT(pack_conv_set_packs(st, F32, f), OK);
    STATE(st, P_F16, F32, false, true);                      // removing does not clear prepared
    EXPECT(pack_conv_set_packs(st, F32, f), OK);
    STATE(st, P_F16, F32, false, true);
    EXPECT(pack_conv_set_packs(st, F32 | BF3, f), OK);
    STATE(st, P_F16, F32 | BF3, false, false);               // adding does
    st.prepared = true;
    EXPECT(pack_conv_set_packs(st, F16, f), OK);             // swapped: one dropped, one added
    STATE(st, P_F16, F16, false, false);
    st.prepared = true;
    // the F16X2 bit is accepted under any precision (the prep launches write the pack only while fp16 is active)
    PackState b;
    b.prepared = true;
    PackFacts fb;
    fb.all_split = true;
    EXPECT(pack_conv_set_packs(b, BF3 | F16, fb), OK);
    STATE(b, P_BF3, BF3 | F16, false, true);
}

static void conv_refused_masks() {
    PackFacts f;
    PackState st = conv_f16_prepared(&f);
    EXPECT(pack_conv_set_packs(st, 0, f), SHAPE);
    EXPECT(pack_conv_set_packs(st, 8, f), SHAPE);
    EXPECT(pack_conv_set_packs(st, ALL | 8, f), SHAPE);
    for (int which = 0; which < 4; ++which) {
        PackFacts g = f;
        (which == 0 ? g.generic : which == 1 ? g.masked : which == 2 ? g.training : g.deconv) = true;
        for (int m = 1; m < ALL; ++m) EXPECT(pack_conv_set_packs(st, m, g), UNSUP);      // every partial mask
        EXPECT(pack_conv_set_packs(st, ALL, g), OK);
        STATE(st, P_F16, ALL, false, true);
    }
    PackFacts nosplit = f;
    nosplit.all_split = false; nosplit.f16_active = false;
    EXPECT(pack_conv_set_packs(st, BF3, nosplit), UNSUP);          // bf16x3 without fp32 needs the split pack
    EXPECT(pack_conv_set_packs(st, BF3 | F16, nosplit), UNSUP);
    EXPECT(pack_conv_set_packs(st, F32 | BF3, nosplit), OK);
    PackFacts idle = f;
    idle.f16_active = false;
    EXPECT(pack_conv_set_packs(st, F16, idle), UNSUP);             // fp16 alone needs fp16 active
    STATE(st, P_F16, F32 | BF3, false, true);                      // refusals change nothing
}

static void stack_masks() {
    PackFacts f;
    f.all_split = true;
    PackState b;                                             // a bf16x3 stack
    b.prepared = true;
    EXPECT(pack_stack_set_packs(b, ALL, f), UNSUP);          // IAF_PACK_F16X2 under a non-F16X2 precision
    EXPECT(pack_stack_set_packs(b, F16, f), UNSUP);
    EXPECT(pack_stack_set_packs(b, ALL | 8, f), SHAPE);
    EXPECT(pack_stack_set_packs(b, 0, f), SHAPE);
    EXPECT(pack_stack_set_packs(b, F32, f), SHAPE);          // a mask without BF16X3 that is not fp16-only-and-active
    STATE(b, P_BF3, ALL, false, true);
    EXPECT(pack_stack_set_packs(b, F32 | BF3, f), OK);       // (the stored F16X2 bit is always set: the fp16 pack follows the precision)
    STATE(b, P_BF3, ALL, false, true);
    EXPECT(pack_stack_set_packs(b, BF3, f), OK);
    STATE(b, P_BF3, BF3 | F16, false, false);                // the stack clears prepared when a bit changes EITHER way
    b.prepared = true;
    EXPECT(pack_stack_set_packs(b, BF3, f), OK);
    STATE(b, P_BF3, BF3 | F16, false, true);
    EXPECT(pack_stack_set_packs(b, F32 | BF3, f), OK);
    STATE(b, P_BF3, ALL, false, false);
    b.prepared = true;
    PackFacts g = f;
    g.all_split = false;
    EXPECT(pack_stack_set_packs(b, BF3, g), UNSUP);          // without F32 when a layer lacks a split pack
    g = f; g.training = true;
    EXPECT(pack_stack_set_packs(b, BF3, g), UNSUP);          // a partial mask while training
    EXPECT(pack_stack_set_packs(b, F32 | BF3, g), OK);
    g = f; g.generic = true; g.all_split = false;
    EXPECT(pack_stack_set_packs(b, BF3, g), UNSUP);
    STATE(b, P_BF3, ALL, false, true);

    PackState st = stack_f16_prepared(&f);
    EXPECT(pack_stack_set_packs(st, F32, f), SHAPE);
    EXPECT(pack_stack_set_packs(st, F32 | F16, f), SHAPE);
    PackFacts idle = f;
    idle.f16_active = false;
    EXPECT(pack_stack_set_packs(st, F16, idle), SHAPE);      // fp16-only, not active
    g = f; g.training = true;
    EXPECT(pack_stack_set_packs(st, F16, g), UNSUP);
    EXPECT(pack_stack_set_packs(st, BF3 | F16, g), UNSUP);
    STATE(st, P_F16, ALL, false, true);
    EXPECT(pack_stack_set_packs(st, F16, f), OK);            // fp16-only and active
    STATE(st, P_F16, F16, false, false);
    st.prepared = true;
    EXPECT(pack_stack_set_packs(st, ALL, f), OK);
    STATE(st, P_F16, ALL, false, false);
}

static void stack_range_failure_bf16x3_dropped() {
    PackFacts f;
    PackState st = stack_f16_prepared(&f);
    EXPECT(pack_stack_set_packs(st, F16, f), OK);
    st.prepared = true;
    EXPECT(pack_range_report(st, PACK_STACK, 0u), false);
    EXPECT(pack_range_report(st, PACK_STACK, 2u), true);
    STATE(st, P_F16, BF3 | F16, true, false);                // the bf16x3 pack is back (the fp32 one stays dropped), behind another prepare
    EXPECT(pack_range_report(st, PACK_STACK, 2u), false);
    STATE(st, P_F16, BF3 | F16, true, false);
    // with the bf16x3 pack kept: nothing but f16_off
    PackState k = stack_f16_prepared(&f);
    EXPECT(pack_stack_set_packs(k, BF3 | F16, f), OK);
    k.prepared = true;
    EXPECT(pack_range_report(k, PACK_STACK, 1u), true);
    STATE(k, P_F16, BF3 | F16, true, true);
}

static void leaving_f16x2() {
    PackFacts f;
    PackState st = stack_f16_prepared(&f);
    EXPECT(pack_stack_set_packs(st, F16, f), OK);
    st.prepared = true;
    EXPECT(pack_set_precision(st, PACK_STACK, P_BF3, false, 0u), false);
    STATE(st, P_BF3, BF3 | F16, false, false);               // the stack's dropped bf16x3 pack comes back
    PackState k = stack_f16_prepared(&f);
    EXPECT(pack_set_precision(k, PACK_STACK, P_F32, false, 0u), false);
    STATE(k, P_F32, ALL, false, true);                       // nothing was dropped: the other packs were written all along
    PackState c = conv_f16_prepared(&f);
    EXPECT(pack_conv_set_packs(c, F16, f), OK);
    EXPECT(pack_set_precision(c, PACK_CONV, P_BF3, false, 0u), false);
    STATE(c, P_BF3, F16, false, true);                       // the conv's mask stays as it was set
}

static void rearm(PackKind kind) {
    PackFacts f;
    PackState st = kind == PACK_STACK ? stack_f16_prepared(&f) : conv_f16_prepared(&f);
    EXPECT(pack_set_precision(st, kind, P_F16, false, 0u), false);   // nothing to re-arm: a no-op
    STATE(st, P_F16, ALL, false, true);
    EXPECT(pack_range_report(st, kind, 1u), true);
    STATE(st, P_F16, ALL, true, true);
    EXPECT(pack_set_precision(st, kind, P_F16, false, 1u), true);    // true: the caller clears the word
    STATE(st, P_F16, ALL, false, false);
    EXPECT(pack_f16_wanted(st), true);
    st.prepared = true;
    EXPECT(pack_set_precision(st, kind, P_F16, false, 1u), true);    // a raised word nobody has looked at yet is cleared too
    STATE(st, P_F16, ALL, false, false);
    st.prepared = true;
    EXPECT(pack_set_precision(st, kind, P_BF3, false, 0u), false);
    STATE(st, P_BF3, ALL, false, true);
    EXPECT(pack_set_precision(st, kind, P_F16, false, 0u), false);   // back on the fp16 planes: their pack was not kept up to date
    STATE(st, P_F16, ALL, false, false);
}

static void training(PackKind kind) {
    PackFacts f;
    PackState st = kind == PACK_STACK ? stack_f16_prepared(&f) : conv_f16_prepared(&f);
    EXPECT(kind == PACK_STACK ? pack_stack_set_packs(st, F16, f) : pack_conv_set_packs(st, F16, f), OK);
    st.prepared = true;
    pack_set_training(st);
    STATE(st, P_F16, ALL, false, false);                     // training keeps every pack; the next prepare writes the transposed ones
}

static void prep_writes() {
    PackFacts f;
    PackState st = stack_f16_prepared(&f);
    auto same = [](PackWrites w, bool wp, bool wp3, bool wp2, bool wpt) {
        EXPECT(w.wp, wp); EXPECT(w.wp3, wp3); EXPECT(w.wp2, wp2); EXPECT(w.wpt, wpt);
    };
    same(pack_prep_writes(st, PACK_STACK, true, true, false), true, true, true, true);
    EXPECT(pack_stack_set_packs(st, BF3, f), OK);            // (no F16X2 bit given: the stack writes wp2 whenever fp16 is active)
    same(pack_prep_writes(st, PACK_STACK, true, true, false), false, true, true, true);
    same(pack_prep_writes(st, PACK_STACK, true, false, false), true, true, true, true);    // wp is skipped only where the layer has a wp3
    EXPECT(pack_stack_set_packs(st, F16, f), OK);
    same(pack_prep_writes(st, PACK_STACK, true, true, false), false, false, true, true);
    same(pack_prep_writes(st, PACK_STACK, false, true, false), false, true, false, true);  // wp3 is skipped only while fp16 is active
    PackState c = conv_f16_prepared(&f);
    same(pack_prep_writes(c, PACK_CONV, true, true, false), true, true, true, false);
    same(pack_prep_writes(c, PACK_CONV, false, true, true), true, true, false, true);
    EXPECT(pack_conv_set_packs(c, BF3 | F16, f), OK);
    same(pack_prep_writes(c, PACK_CONV, true, true, false), false, true, true, false);
    EXPECT(pack_conv_set_packs(c, F32, f), OK);
    same(pack_prep_writes(c, PACK_CONV, true, false, false), true, false, false, false);
}

int main() {
    conv_fp16_only_range_failure();
    conv_bf16x3_kept_range_failure();
    conv_set_packs_changes();
    conv_refused_masks();
    stack_masks();
    stack_range_failure_bf16x3_dropped();
    leaving_f16x2();
    rearm(PACK_STACK);
    rearm(PACK_CONV);
    training(PACK_STACK);
    training(PACK_CONV);
    prep_writes();
    printf("pack state walk ok: %d checks\n", g_checks);
    return 0;
}
