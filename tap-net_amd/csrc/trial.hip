// trial.hip -- "what would calc_ratio be if this container took column c next?" for every selectable column of B
// containers in one launch, without committing anything: the scores the reference's greedy baseline
// generate_order_graph(..., find_order_type='best') (generate.py:1242-1292: best_to_pack) gets from one deep copy of
// the target Container per selectable node, add_new_block on the copy and calc_ratio.
//
// A trial is the placement wave of tap_waves.h without its stores: the lane group holds the container's height-map
// and counters in registers, gathers the candidate block from `static` with the same (int)v cast, applies the same
// admission rule (error bits 2 and 4), runs tap_place on the group's LDS slice and evaluates C / P / S from the
// updated registers (tap_waves.h:88-95, in fp64: what tap_env_ratio's ratio64_out reports after the committed step).
//
// Geometry: ONE WAVEFRONT PER CONTAINER, its 64 / G lane groups each trying a different column.  The wave loads the
// container once (every group its own copy of the height-map: tap_place reads the slice, never writes it, so the
// copies stay valid for every pass), ballots the mask row 64 columns at a time, and group g takes the g-th selectable
// column still left in the ballot: ceil(live / (64 / G)) passes per 64 columns -- one pass for the 2.6 live columns of
// 20 at W = 5 (G = 8, 8 groups), five for the 9.6 of 60 at 5 x 5 (G = 32, 2 groups) -- instead of nR placements.  The
// ballot is wave-uniform, so every lane runs every pass (the cross-lane operations of tap_place need the whole wave
// converged); a group without a column runs the placement with do_step = false on a clamped column and drops the
// result.  The running (score, column) pair lives in registers and is reduced across the groups by v_readlane of
// their first lanes: no workgroup barrier, no second launch, no store but the scores.
#include "tap_common.h"
#include "tap_place.h"

namespace {

constexpr int TAP_HIT_TRIAL = 25; // launch record (tapenv.h: tap_variant_hits), after tap_common.h's TapHitKind

struct TrialArgs {
    tap_env_desc d;
    const int32_t *hm;     // [B][cells]
    const int32_t *cnt;    // [B][4]
    const float *static_;  // (B, static_rows, nR)
    int static_rows, nR;
    const float *mask;     // (B, nR) or null = every column
    int fresh;
    double *scores;        // (B, nR) or null
    int64_t *best;         // (B,) or null
    const uint32_t *lut;
};

// first maximum of a row, compared in fp64: a later column replaces the running pair only when it is strictly larger,
// an earlier one also when it ties (the groups of a pass hold increasing columns, the passes run in column order)
__device__ __forceinline__ void trial_keep(double &best, int &bcol, double r, int c)
{
    if (r > best || (r == best && c < bcol)) { best = r; bcol = c; }
}

template <int D, int G, bool HARD>
__global__ void __launch_bounds__(TAP_BLOCK) k_trial_scores(TrialArgs a)
{
    __shared__ int s_hm[TAP_BLOCK];
    constexpr int NG = 64 / G;                                  // lane groups = columns tried per pass
    const int tid = threadIdx.x, lane = tid & 63, cell = lane % G, grp = lane / G;
    const int env = blockIdx.x * (TAP_BLOCK / 64) + TAP_WAVE_INDEX();
    if (env >= a.d.B) return;                                   // the whole wave leaves: nothing below spans waves
    const int W = a.d.W, L = a.d.L, cells = W * L, nR = a.nR;
    const bool incell = cell < cells;
    // the container, once: loads unconditional on clamped addresses, then the select (tap_waves.h)
    const int hm_l = a.hm[(size_t)env * cells + min(cell, cells - 1)];
    const int cv_l = a.cnt[(size_t)env * 4 + (cell & 3)];
    const int hm0 = (!a.fresh && incell) ? hm_l : 0;
    const int cv = (!a.fresh && cell < 4) ? cv_l : 0;
    const int gl0 = lane - cell;
    const Counters cnt0 = {__shfl(cv, gl0), __shfl(cv, gl0 + 1), __shfl(cv, gl0 + 2), __shfl(cv, gl0 + 3)};
    int *slice = s_hm + (tid - cell);
    slice[cell] = hm0;
    tap_wave_lds_sync();
    const PlaceCfg cfg = {W, L, a.d.H, a.d.flags, a.lut};
    const float *st = a.static_ + (size_t)env * a.static_rows * nR;
    const double ninf = -__builtin_huge_val();
    double best = ninf;                                         // group-uniform running pair
    int bcol = INT_MAX;
    for (int base = 0; base < nR; base += 64) {
        const int col = base + lane;
        const bool inr = col < nR;
        float mv = 1.f;
        if (a.mask) mv = a.mask[(size_t)env * nR + min(col, nR - 1)];
        const bool sel = inr && mv != 0.f;
        if (a.scores && inr && !sel) a.scores[(size_t)env * nR + col] = ninf;
        u64 live = __ballot(sel);                               // wave-uniform: the pass loop keeps the wave converged
        while (live) {
            u64 t = live;                                       // this group's column: the grp-th set bit
#pragma unroll
            for (int i = 0; i < NG - 1; ++i) if (i < grp) t &= t - 1;
            const bool mine = t != 0;
            const int c = mine ? base + __ffsll((long long)t) - 1 : 0;
            int dims[3] = {1, 1, 1};
            for (int k = 0; k < D; ++k) dims[k] = (int)st[(size_t)(1 + k) * nR + c];   // model.py:404-412, tools.py:3689
            const int bx = dims[0], by = D == 3 ? dims[1] : 1, bz = dims[D - 1];
            int hm = hm0, err = 0;
            Counters cnt = cnt0;
            bool do_step = mine;
            if (mine && cnt.count >= a.d.n_max) { err |= 2; do_step = false; }         // tools.py:3677 IndexError
            if (mine && (bx < 1 || by < 1 || bz < 1)) { err |= 4; do_step = false; }
            (void)tap_place<D, G, HARD>(cfg, slice, cell, hm, cnt, err, bx, by, bz, do_step);
            err = group_or<G>(err);
            const int gmax = group_max<G>(incell ? hm : 0);
            double C = 0.0, P = 0.0, S = 0.0;                   // tools.py:3887-3966 on the state a commit would write
            if (cnt.count != 0) {
                C = (double)cnt.valid / (double)((long long)W * L * gmax);
                P = (double)cnt.valid / (double)(cnt.empty + cnt.valid);
                S = (double)cnt.nstable / (double)cnt.count;
            }
            const double r = err ? -1.0 : tap_ratio_formula(a.d.ratio_mode, C, P, S);
            if (mine) {
                if (a.scores && cell == 0) a.scores[(size_t)env * nR + c] = r;
                trial_keep(best, bcol, r, c);
            }
#pragma unroll
            for (int i = 0; i < NG; ++i) live &= live - 1;      // the NG lowest columns are done
        }
    }
    if (a.best) {
        double wb = ninf;
        int wc = INT_MAX;
#pragma unroll
        for (int g = 0; g < NG; ++g) {                          // the groups' pairs, through their first lanes
            const double r = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(best), g * G),
                                              __builtin_amdgcn_readlane(__double2loint(best), g * G));
            trial_keep(wb, wc, r, __builtin_amdgcn_readlane(bcol, g * G));
        }
        if (lane == 0) a.best[env] = wc == INT_MAX ? 0 : wc;    // no selectable column: argmax of a row of -inf
    }
}

template <int D, int G> int launch_trial(tap_ctx *ctx, const TrialArgs &a, hipStream_t st)
{
    const int wpb = TAP_BLOCK / 64, grid = (a.d.B + wpb - 1) / wpb;
    const bool hard = (a.d.flags & TAP_F_HARD) != 0;
    if (hard) hipLaunchKernelGGL((k_trial_scores<D, G, true>), dim3(grid), dim3(TAP_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_trial_scores<D, G, false>), dim3(grid), dim3(TAP_BLOCK), 0, st, a);
    TAP_LAUNCH_CHECK(ctx, "k_trial_scores");
    tap_variant_hit(ctx, TAP_HIT_TRIAL, D, G, TapVariant{hard ? 1 : 0, a.mask ? 1 : 0, a.fresh ? 1 : 0}, 0);
    return TAP_OK;
}

int dispatch_trial(tap_ctx *ctx, const tap_env_desc *d, const TrialArgs &a, hipStream_t st)
{
    TAP_DISPATCH_DG(launch_trial, d, ctx, a, st);
}

} // namespace

extern "C" int tap_env_trial_scores(tap_ctx *ctx, const tap_env_desc *d, const void *state, const float *static_,
                                    int static_rows, int nR, const float *mask, int flags, double *scores_out,
                                    int64_t *best_out, void *stream)
{
    if (!d) return tap_fail(ctx, TAP_E_INVALID, "null descriptor");
    if (tap_place_at_semantics(d))
        return tap_fail(ctx, TAP_E_INVALID, "trial scores on a place-at descriptor: its blocks go to caller-chosen columns");
    int rc = tap_desc_validate(ctx, d);
    if (rc) return rc;
    if (flags & ~TAP_T_FRESH) return tap_fail(ctx, TAP_E_INVALID, "trial scores: bad flags %d", flags);
    if (d->strategy != TAP_LB_GREEDY || tap_is_big(d))
        return tap_fail(ctx, TAP_E_UNSUPPORTED, "trial scores run on the lane-per-cell LB_GREEDY kernels only (at most 64 "
                        "cells, 3D sides at most 8): step this shape or strategy on a copy of the blob");
    if (d->B == 0) return TAP_OK; // an empty batch has no buffers to check
    if (!state || !static_ || static_rows < 1 + d->D || nR < 1)
        return tap_fail(ctx, TAP_E_INVALID, "bad trial arguments");
    if (!scores_out && !best_out) return tap_fail(ctx, TAP_E_INVALID, "trial scores: no output given");
    EnvView v;
    tap_env_layout(d, const_cast<void *>(state), &v);           // only read: the kernel takes const pointers
    TrialArgs a = {};
    a.d = *d;
    a.hm = v.hm; a.cnt = v.cnt;
    a.static_ = static_; a.static_rows = static_rows; a.nR = nR;
    a.mask = mask;
    a.fresh = (flags & TAP_T_FRESH) ? 1 : 0;
    a.scores = scores_out; a.best = best_out;
    a.lut = ctx ? ctx->stab_lut : nullptr;
    return dispatch_trial(ctx, d, a, (hipStream_t)stream);
}
