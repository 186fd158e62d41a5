// tap_step_request.h -- the host side of one fused step (transition.hip): what a caller asks for, whether it may be asked,
// and which launcher carries it.  The three entry points (tap_transition, tap_transition_bits, tap_transition_first) and
// tap_stepper_step fill ONE TapStepRequest by field name; tap_step_request_check refuses it or not, tap_step_route picks
// the launches, and transition_impl acts on the answer.  Nothing here touches the device: the header is plain C++17 and
// compiles for the host alone (tests/host/step_request_host.cpp runs it against tests/stream_cases.py's model).
#pragma once

#include <cstdint>

#include "tapenv.h"

// ---- the window --------------------------------------------------------------------------------------------------------
// A (rows, nR) window has a bit shadow -- one 64-bit word per column for up to 64 rows, two up to 128, columns read four
// at a time (tap_dyn_bits; tap_masks.h: stream_wave_bits).  A window without one is carried as the fp32 tensor and its
// column sums.  rows and nR are positive (every caller has checked its shape).
inline bool tap_window_has_shadow(int rows, int nR) { return rows <= 128 && nR % 4 == 0 && nR <= 256; }

// ---- the container -----------------------------------------------------------------------------------------------------
// LB_GREEDY containers beyond the lane-per-cell kernels (more than 64 cells, or a 3D side above 8): big.hip, up to
// TAP_BIG_WG_CELLS cells (above 4 096: one workgroup per container with the height-map in its LDS)
constexpr int TAP_BIG_WG_CELLS = 16384;
inline bool tap_is_big(const tap_env_desc *d)
{
    return d->strategy == TAP_LB_GREEDY && (d->W * d->L > 64 || (d->D == 3 && (d->W > 8 || d->L > 8)));
}
// MACS / MUL 3D containers beyond the lane-per-cell kernel (more than 64 cells or a side above 8): macs3_big.hip, one
// thread per container on the same state (height-map, history, free-list bit-grid) + candidate lists in the scratch section
inline bool tap_is_big_macs3(const tap_env_desc *d)
{
    return d->strategy == TAP_MACS && d->D == 3 && (d->W * d->L > 64 || d->W > 8 || d->L > 8);
}

// ---- the request -------------------------------------------------------------------------------------------------------
enum TapStepForm {
    TAP_STEP_COPY,     // tap_transition: the fp32 tensor is copied, the column-sum shadow carries update_mask
    TAP_STEP_BITS,     // tap_transition_bits: the step reads and writes the bit shadow
    TAP_STEP_FIRST     // tap_transition_first: the step builds the bit shadow from the fp32 tensor it is given
};

// The by-products a decoding loop wants from the step's gather (tap_common.h: StepArgs::dec_static_out / tour_out): the
// fused kernels' placement waves write them; for the shapes that run as two launches k_step_aux does.  Null = not wanted.
struct TapStepAux {
    float *dec_static_out;
    int64_t *tour_out;
    int tour_stride, tour_col;
};

// Every buffer the three entry points take, by name (include/tapenv.h documents each).  A field its form does not use
// stays null: COPY has no bits_* / nonbinary_out, BITS no dyn_in / colsum_*, FIRST no bits_in / colsum_*.
struct TapStepRequest {
    int form;                                  // TapStepForm
    int n, R, rows, update_rows, static_rows;  // the window
    int flags;                                 // TAP_T_FRESH | TAP_T_RATIO
    const float *dyn_in;
    const unsigned long long *bits_in;
    const float *static_;
    const int64_t *ptr;
    const float *mask_in;                      // null = ones (the mask DRL.forward starts from, model.py:297): a stepper's first step only
    const float *colsum_in;
    float *dyn_out;
    float *colsum_out;
    unsigned long long *bits_out;
    float *current_out;
    float *mask_out;
    float *feature_out;
    float *ratio_out;
    int32_t *nonbinary_out;
    TapStepAux aux;                            // a stepper's by-products
    // dyn_out holds update_dynamic's INPUT (the stepper's previous step wrote it there): the lane-per-cell fused kernels then
    // write the cleared rows only; every other route writes the whole tensor, which is the same tensor
    int inplace;
};

// ---- may it be asked? ----------------------------------------------------------------------------------------------------
struct TapStepVerdict {
    int status;          // TAP_OK or TAP_E_INVALID
    const char *msg;     // what tap_last_error reports (no format directives); null with TAP_OK
};

// The argument checks of a step on B > 0 containers of dimension D: the list every form shares, then the form's own.
// from_stepper: the call comes from tap_stepper_step, whose first step may leave mask_in null; a public entry point may
// not.  (The descriptor's own checks, tap_desc_validate and tap_macs_validate, run before this one, and the alignment of
// the bit shadow's buffers after it: tap_masks.h, mask_bits_check.)
inline TapStepVerdict tap_step_request_check(const TapStepRequest &r, int B, int D, bool from_stepper, bool has_state)
{
    if (B == 0) return {TAP_OK, nullptr};    // an empty batch has no buffers to check
    if (!has_state || !r.static_ || !r.ptr || (!r.mask_in && !from_stepper) || !r.current_out || !r.mask_out || r.n < 1 || r.R < 1 ||
        r.rows < 1 || r.static_rows < 1 + D || r.update_rows < 0 || r.update_rows > 3 || ((r.flags & TAP_T_RATIO) && !r.ratio_out))
        return {TAP_E_INVALID, "bad transition arguments"};
    switch (r.form) {
    case TAP_STEP_COPY:
        if (!r.dyn_in || !r.colsum_in || !r.dyn_out || !r.colsum_out) return {TAP_E_INVALID, "bad transition arguments"};
        if (r.dyn_in == r.dyn_out) return {TAP_E_INVALID, "transition is out of place (pack.py:370)"};
        break;
    case TAP_STEP_BITS:
        if (!r.bits_in || !r.bits_out || r.bits_in == r.bits_out) return {TAP_E_INVALID, "bad transition_bits arguments"};
        break;
    default:
        if (!r.dyn_in || !r.bits_out || r.dyn_in == r.dyn_out) return {TAP_E_INVALID, "bad transition_first arguments"};
    }
    return {TAP_OK, nullptr};
}

// ---- which launches carry it? ----------------------------------------------------------------------------------------------
enum TapStepRoute {
    TAP_ROUTE_FUSED = 0,        // the lane-per-cell kernels: k_transition / k_transition_macs / k_transition_macs3, one launch
    TAP_ROUTE_WAVE_BIG = 1,     // one wavefront per container beside the stream waves: big.hip (handles fresh / ratio itself),
    TAP_ROUTE_WAVE_MACS2 = 2,   //   macs_big.hip and
    TAP_ROUTE_WAVE_MACS3 = 3,   //   macs3_big.hip (a fresh container and calc_ratio are launches of their own)
    TAP_ROUTE_TWO_LAUNCHES = 4  // reset? -> tap_mask_step / _bits / _first -> placement, ratio?, by-products
};

// What only the families' own files can tell: whether the container's tiles fit a workgroup's LDS next to the stream
// tiles.  The caller asks the family the container belongs to (transition.hip: transition_caps); the others stay false.
struct TapStepCaps {
    bool big_ok;             // tap_big_transition_ok
    bool macs_wave_ok;       // tap_macs_wave_transition_ok
    bool macs3_wave_ok;      // tap_macs3_wave_transition_ok
    bool macs_lanes_fit;     // the MACS lane kernels' lists fit beside the stream tiles (transition.hip: transition_caps)
    int macs2d_wave_from;    // tap_macs2d_wave_from(): the width at which MACS 2D hands over to its wave kernel (17)
};

// Shapes and strategies whose placement is one THREAD per container (legacy 'LB', LB_GREEDY and MACS 3D above 64 cells or
// with a 3D side above 8) or the wide MACS 2D form (17 .. 64 columns) have no lane-per-cell kernel that carries both halves
// of the step.  (For wide MACS one was built and measured in round 3 -- tap_macs_wide_wave as the placement waves of a
// k_transition_macs look-alike: 121 against 97 us per step at W = 20, n = 12, B = 8192, equal at W = 40: the placement is
// ~100 us of register-heavy work, the stream waves hide nothing and their wave slots cost a quarter of the resident envs.)
// On the bit shadow the wave-per-container kernels take those shapes in one launch; every fused kernel carries the
// one-word shadow only (rows <= 64).  What is left runs the same step as its two launches, so a caller drives every shape
// through one entry point.  The route reads the request's form and rows, nothing else of it.
inline TapStepRoute tap_step_route(const TapStepRequest &r, const tap_env_desc &d, const TapStepCaps &c)
{
    const bool on_bits = r.form != TAP_STEP_COPY, wide_macs2 = d.strategy == TAP_MACS && d.D == 2 && d.W > 16;
    if (on_bits && r.rows > 64) return TAP_ROUTE_TWO_LAUNCHES;
    if (on_bits) {
        if (tap_is_big(&d) && c.big_ok) return TAP_ROUTE_WAVE_BIG;
        if (wide_macs2 && d.W >= c.macs2d_wave_from && c.macs_wave_ok) return TAP_ROUTE_WAVE_MACS2;
        if (tap_is_big_macs3(&d) && c.macs3_wave_ok) return TAP_ROUTE_WAVE_MACS3;
    }
    if (d.strategy == TAP_LB || tap_is_big(&d) || tap_is_big_macs3(&d) || wide_macs2) return TAP_ROUTE_TWO_LAUNCHES;
    // the MACS placement keeps its lists in LDS: a container too tall (or an episode too long) for one workgroup's LDS next
    // to the stream tiles takes the two launches as well (the stand-alone step runs fewer envs per workgroup)
    if (d.strategy == TAP_MACS && !c.macs_lanes_fit) return TAP_ROUTE_TWO_LAUNCHES;
    return TAP_ROUTE_FUSED;
}
inline int tap_step_route_launches(TapStepRoute route) { return route == TAP_ROUTE_TWO_LAUNCHES ? 2 : 1; }
