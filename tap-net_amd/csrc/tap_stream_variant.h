// tap_stream_variant.h -- which instantiation of a precedence-update ("stream wave") kernel a launch runs.
// Every launcher of such a kernel (transition.hip, transition_macs.hip, big.hip, macs_big.hip, macs3_big.hip, masks.hip)
// turns the facts of its MaskArgs (tap_masks.h: tap_mask_facts) and its own geometry into a triple (nc, mode, extra) with
// tap_stream_variant(), and launches the entry of its table below that equals it (tap_common.h: tap_launch_variant).  The
// MODE bits FULL and INPLACE compile guards out of the kernels (tap_transition.h), so their preconditions are checked here
// and only here.  Host-compilable (tests/host: checked against a restatement of the rules over the product of the facts).
#pragma once

#include <climits>
#include <cstddef>
#include <utility>

// ---- MODE bits of the stream-wave kernels (tap_transition.h: trans_stream_wave) ---------------------------------------
// MODE & 3: 0 = fp32 copy with the column-sum shadow, 1 = on the bit shadow, 2 = first step (shadow built in the launch);
// MODE & 4 (TAP_MODE_MERGED): the fp32 expansion walks the wave's two slabs as one run of rows (tap_masks.h:
// stream_wave_bits, where the A/B figures are) instead of slab by slab
// MODE & 8 / & 16 (TAP_MODE_C4_5 / _15): the window is the reference's own -- n = 10, rows = 30, nR = 20 (2D) / 60 (3D) --
// and its shape is compiled in (stream_wave_bits_r4: C4S)
// (both bits, TAP_MODE_C4_10: c4's window, n = 20, rows = 60, nR = 40 -- the MACS 2D step, transition_macs.hip)
// MODE & 32 (TAP_MODE_INPLACE, with MODE & 3 == 1 only): dyn_out holds the previous step's tensor (MaskArgs::inplace) --
// the stream waves write the cleared rows' zeros instead of expanding the slab
// MODE & 64 (TAP_MODE_FULL, with MODE & 3 == 1 and a compiled-in shape only): ptr, static and mask_in are all given and B is
// a multiple of the workgroup's envs -- the stream wave carries no code for absent inputs or idle slabs (tap_masks.h: FULL)
// k_mask_step (masks.hip) numbers its own: 0 .. 2 as MODE & 3, 3 / 4 = 1 / 2 on the two-word shadow (65 .. 128 rows).
constexpr int TAP_MODE_MERGED = 4, TAP_MODE_C4_5 = 8, TAP_MODE_C4_15 = 16, TAP_MODE_C4_10 = 24, TAP_MODE_INPLACE = 32, TAP_MODE_FULL = 64;
constexpr int tap_mode_shape(int D) { return D == 2 ? TAP_MODE_C4_5 : TAP_MODE_C4_15; }

// Loop form of the fp32 expansion in the MACS steps' stream waves (transition_macs.hip): 5 / 6 = shadow (given / built) |
// TAP_MODE_MERGED, the run-of-rows loop; 1 / 2 = slab by slab.  Round 6, same session, two runs each
// (profiles/r06_macs_merge_ab.txt), M env-steps/s, run-of-rows against slab-by-slab: MACS 2D (c4's shape) 518.6 / 518.0
// against 508.7 / 511.8 at B = 8 192, 461.8 / 482.5 against 467.7 / 482.8 at 32 768 (nontemporal stores from here on),
// 533.4 / 526.0 against 518.8 / 519.6 at 131 072 -- the run-of-rows loop at every batch, unlike the LB_GREEDY step
// (transition.hip), whose 2D windows lose 15-20 % with it once the stores are nontemporal; MACS 3D (c6's shape, nR = 60)
// 139.8 / 139.7 against 139.9 / 140.1 at B = 4 096, 195.2 / 195.6 against 197.2 / 197.8 at 32 768, 222.9 / 222.9 against
// 225.8 / 225.8 at 131 072 -- slab by slab, as for the LB_GREEDY step's 3D windows.  -DTAP_MACS_NOMERGE /
// -DTAP_MACS_MERGE_ALL force one form everywhere (A/B builds).
#if defined(TAP_MACS_NOMERGE)
constexpr int TAP_MACS_M1 = 1, TAP_MACS_M2 = 2, TAP_MACS3_M1 = 1, TAP_MACS3_M2 = 2;
#elif defined(TAP_MACS_MERGE_ALL)
constexpr int TAP_MACS_M1 = 5, TAP_MACS_M2 = 6, TAP_MACS3_M1 = 5, TAP_MACS3_M2 = 6;
#else
constexpr int TAP_MACS_M1 = 5, TAP_MACS_M2 = 6, TAP_MACS3_M1 = 1, TAP_MACS3_M2 = 2;
#endif

// ---- the choice ---------------------------------------------------------------------------------------------------
enum TapStreamKind {
    TAP_SV_TRANSITION,    // k_transition<D, G, nc, SW, mode>            (transition.hip: launch_transition_v)
    TAP_SV_MACS,          // k_transition_macs<G, nc, mode, extra = WC>  (transition_macs.hip: launch_transition_macs)
    TAP_SV_MACS3,         // k_transition_macs3<G, nc, mode, extra = WL> (transition_macs.hip: launch_transition_macs3)
    TAP_SV_BIG,           // k_big_transition<extra = HARD, nc, mode>    (big.hip: tap_big_transition)
    TAP_SV_MACS_WAVE,     // k_macs2d_wave_transition<nc, mode>          (macs_big.hip: tap_macs_wave_transition)
    TAP_SV_MACS3_WAVE,    // k_macs3d_wave_transition<nc, mode>          (macs3_big.hip: tap_macs3_wave_transition)
    TAP_SV_MASK_STEP,     // k_mask_step<nc, mode>                       (masks.hip: launch_mask_step)
    TAP_SV_KINDS
};

struct TapVariant {
    int nc, mode, extra;
    constexpr bool operator==(const TapVariant &o) const { return nc == o.nc && mode == o.mode && extra == o.extra; }
};

// what a launch's MaskArgs says (tap_masks.h: tap_mask_facts)
struct TapMaskFacts {
    int nc;            // columns per lane of the fast path (mask_fast_path_cols): 1, 2 or 4; 0 = the element-wise path
    int src;           // 1 = the step reads the bit shadow, 2 = it builds the shadow from fp32, 0 = fp32 copy
    bool inplace;      // MaskArgs::inplace with dyn_out given
    bool inputs;       // ptr, static_ and mask_in all given
    bool wt;           // write-through stores (MaskArgs::wt)
    int n, rows, update_rows, nR;
};

// what the launcher knows besides: window dimension, lanes per container, envs per workgroup, batch, container sides
struct TapLaunchFacts {
    int D, G, EPB, B, W, L;
    bool hard;
};

// the reference's own windows (n = 10), whose shape the LB_GREEDY step compiles in, and c4's (n = 20) for MACS 2D
constexpr bool tap_mode_shape_ok(const TapMaskFacts &m, int D)
{
    return m.n == 10 && m.rows == 30 && m.update_rows == 3 && m.nR == (D == 2 ? 20 : 60);
}
constexpr bool tap_mode_shape20_ok(const TapMaskFacts &m) { return m.n == 20 && m.rows == 60 && m.update_rows == 3 && m.nR == 40; }

constexpr TapVariant tap_stream_variant(int kind, const TapMaskFacts &m, const TapLaunchFacts &l)
{
    const bool fast = m.nc == 1 || m.nc == 2 || m.nc == 4;
    switch (kind) {
    case TAP_SV_BIG:            // the wave-per-container steps run on the bit shadow only: no element-wise path
    case TAP_SV_MACS_WAVE:
    case TAP_SV_MACS3_WAVE:
        return {m.nc == 1 || m.nc == 2 ? m.nc : 4, m.src == 1 ? 1 : 2, kind == TAP_SV_BIG ? (int)l.hard : 0};
    case TAP_SV_MASK_STEP: {
        const bool wide = m.src != 0 && m.rows > 64;                           // two words per column
        return fast ? TapVariant{m.nc, m.src + (wide ? 2 : 0), 0} : TapVariant{0, 0, 0};
    }
    default: break;
    }
    // the fused steps: the caller's dyn_out already holds the previous step's tensor (a stepper on ONE dyn buffer) --
    // only the cleared rows are written
    const bool inpl = m.src == 1 && m.inplace;
    int mode = 0;
    if (kind == TAP_SV_TRANSITION) {
        // 2D windows (nR = 2n columns: five store instructions per run at c2) take the run-of-rows expansion while the
        // stores are write-through; 3D windows and every launch beyond the write-through limit keep the slab-by-slab loops
        const int merged = l.D == 2 && m.wt ? TAP_MODE_MERGED : 0;
        mode = inpl ? 1 | TAP_MODE_INPLACE : m.src == 1 ? 1 | merged : m.src == 2 ? 2 | merged : 0;
        if (!fast) return {0, 0, 0};
        // the reference's own window on the bit shadow runs the instantiation with its shape compiled in ...
        if (m.nc == 1 && (mode & 3) != 0 && tap_mode_shape_ok(m, l.D)) {
            mode |= tap_mode_shape(l.D);
#ifndef TAP_NO_FULL                                                             // A/B builds
            // ... and, for a step on a shadow the caller hands in, without the code for absent inputs and idle slabs
            if ((mode & 3) == 1 && m.inputs && l.B % l.EPB == 0) mode |= TAP_MODE_FULL;
#endif
        }
        return {m.nc, mode, 0};
    }
    const bool m3 = kind == TAP_SV_MACS3;
    mode = inpl ? 1 | TAP_MODE_INPLACE : m.src == 1 ? (m3 ? TAP_MACS3_M1 : TAP_MACS_M1) : m.src == 2 ? (m3 ? TAP_MACS3_M2 : TAP_MACS_M2) : 0;
    if (m3) {
        // the reference's own 3D container (5 x 5, BASELINE c6; a 32-lane group) runs the instantiation with compile-time sides
        const int wl = l.G == 32 && l.W == 5 && l.L == 5 ? 5 : 0;
        return fast ? TapVariant{m.nc, mode, wl} : TapVariant{0, 0, wl};
    }
    if (!fast) return {0, 0, 0};
    // BASELINE configs[3] (c4: W = 7, windows of 20 nodes) on the bit shadow: the width and the window's shape compiled in
    if (l.G == 8 && m.nc == 1 && (mode & 3) != 0 && l.W == 7 && tap_mode_shape20_ok(m)) return {1, mode | TAP_MODE_C4_10, 7};
    return {m.nc, mode, 0};
}

// ---- what each launcher instantiates ------------------------------------------------------------------------------
// One table per launcher, over all its D / G; tap_variant_built() says which entries exist for one (D, G).
template <int KIND> struct TapVariants;

template <> struct TapVariants<TAP_SV_TRANSITION> {
    static constexpr int I = 1 | TAP_MODE_INPLACE, S2 = TAP_MODE_C4_5, S3 = TAP_MODE_C4_15, F = TAP_MODE_FULL;
    static constexpr TapVariant v[] = {
        {1, I}, {1, I | S2}, {1, I | S2 | F}, {1, I | S3}, {1, I | S3 | F},
        {1, 5}, {1, 5 | S2}, {1, 5 | S2 | F},
        {1, 1}, {1, 1 | S2}, {1, 1 | S2 | F}, {1, 1 | S3}, {1, 1 | S3 | F},
        {1, 6}, {1, 6 | S2},
        {1, 2}, {1, 2 | S2}, {1, 2 | S3},
        {1, 0},
        {2, I}, {2, 5}, {2, 1}, {2, 6}, {2, 2}, {2, 0},
        {4, I}, {4, 5}, {4, 1}, {4, 6}, {4, 2}, {4, 0},
        {0, 0},
    };
};

template <> struct TapVariants<TAP_SV_MACS> {
    static constexpr int I = 1 | TAP_MODE_INPLACE, M1 = TAP_MACS_M1, M2 = TAP_MACS_M2, C = TAP_MODE_C4_10;
    static constexpr TapVariant v[] = {
        {1, I, 0}, {1, I | C, 7}, {1, M1, 0}, {1, M1 | C, 7}, {1, M2, 0}, {1, M2 | C, 7}, {1, 0, 0},
        {2, I, 0}, {2, M1, 0}, {2, M2, 0}, {2, 0, 0},
        {4, I, 0}, {4, M1, 0}, {4, M2, 0}, {4, 0, 0},
        {0, 0, 0},
    };
};

template <> struct TapVariants<TAP_SV_MACS3> {
    static constexpr int I = 1 | TAP_MODE_INPLACE, M1 = TAP_MACS3_M1, M2 = TAP_MACS3_M2;
    static constexpr TapVariant v[] = {
        {1, I, 0}, {1, M1, 0}, {1, M2, 0}, {1, 0, 0}, {2, I, 0}, {2, M1, 0}, {2, M2, 0}, {2, 0, 0},
        {4, I, 0}, {4, M1, 0}, {4, M2, 0}, {4, 0, 0}, {0, 0, 0},
        {1, I, 5}, {1, M1, 5}, {1, M2, 5}, {1, 0, 5}, {2, I, 5}, {2, M1, 5}, {2, M2, 5}, {2, 0, 5},
        {4, I, 5}, {4, M1, 5}, {4, M2, 5}, {4, 0, 5}, {0, 0, 5},
    };
};

// (in the order that keeps each kernel's place in big.hip's code object: they load a constant PC-relative)
template <> struct TapVariants<TAP_SV_BIG> {
    static constexpr TapVariant v[] = {
        {4, 2, 0}, {4, 1, 0}, {2, 2, 0}, {2, 1, 0}, {1, 2, 0}, {1, 1, 0},
        {4, 2, 1}, {4, 1, 1}, {2, 2, 1}, {2, 1, 1}, {1, 2, 1}, {1, 1, 1},
    };
};

template <> struct TapVariants<TAP_SV_MACS_WAVE> {
    static constexpr TapVariant v[] = {{1, 1, 0}, {1, 2, 0}, {2, 1, 0}, {2, 2, 0}, {4, 1, 0}, {4, 2, 0}};
};
template <> struct TapVariants<TAP_SV_MACS3_WAVE> : TapVariants<TAP_SV_MACS_WAVE> {};

template <> struct TapVariants<TAP_SV_MASK_STEP> {
    static constexpr TapVariant v[] = {
        {1, 0}, {1, 1}, {1, 2}, {1, 3}, {1, 4}, {2, 0}, {2, 1}, {2, 2}, {2, 3}, {2, 4}, {4, 0}, {4, 1}, {4, 2}, {4, 3}, {4, 4},
        {0, 0},
    };
};

// entries of the tables above that a launcher instantiates for one window dimension D / lane group G (the others ignore both)
constexpr bool tap_variant_built(int kind, int D, int G, const TapVariant &v)
{
    switch (kind) {
    case TAP_SV_TRANSITION:
        return ((v.mode & TAP_MODE_MERGED) == 0 || D == 2) && ((v.mode & TAP_MODE_C4_10) == 0 || (v.mode & TAP_MODE_C4_10) == tap_mode_shape(D));
    case TAP_SV_MACS: return v.extra == 0 || G == 8;
    case TAP_SV_MACS3: return v.extra == 0 || G == 32;
    default: return true;
    }
}

// ---- launching the chosen entry -------------------------------------------------------------------------------------
// launch(TapVariantC<nc, mode, extra>{}) is instantiated for every entry built for (D, G) and called for the one equal to
// v; its result is returned, TAP_VARIANT_NONE when no entry equals v (tap_common.h: tap_launch_variant)
template <int NC, int MODE, int EXTRA> struct TapVariantC { static constexpr int nc = NC, mode = MODE, extra = EXTRA; };
constexpr int TAP_VARIANT_NONE = INT_MIN;

template <int KIND, int D, int G, size_t I, class Launch>
inline bool tap_variant_try(const TapVariant &v, Launch &launch, int &rc)
{
    constexpr TapVariant e = TapVariants<KIND>::v[I];
    if constexpr (tap_variant_built(KIND, D, G, e)) {
        if (v == e) { rc = launch(TapVariantC<e.nc, e.mode, e.extra>{}); return true; }
    }
    return false;
}

template <int KIND, int D, int G, class Launch, size_t... I>
inline int tap_variant_dispatch(const TapVariant &v, Launch &launch, std::index_sequence<I...>)
{
    int rc = TAP_VARIANT_NONE;
    (tap_variant_try<KIND, D, G, I>(v, launch, rc) || ...);
    return rc;
}

template <int KIND, int D = 0, int G = 0, class Launch>
inline int tap_variant_dispatch(const TapVariant &v, Launch &&launch)
{
    constexpr size_t N = sizeof(TapVariants<KIND>::v) / sizeof(TapVariant);
    return tap_variant_dispatch<KIND, D, G>(v, launch, std::make_index_sequence<N>{});
}
