// transition.hip -- one whole lock-step of DRL.forward's environment work in a single launch:
// update_dynamic + update_mask (pack.py:276-376, model.py:376-386) and the gather + add_new_block
// of model.py:404-465, optionally starting from a fresh container (Container.__init__) and
// optionally emitting calc_ratio (model.py:499-510).  gfx950 only.
//
// Why fuse: at the BASELINE batch sizes the placement moves ~0.9 MB per launch and is pure latency
// (two dependent loads, fp64 divides), while the precedence update streams ~40 MB and is HBM-bound.
// In one launch the placement's latency hides under the stream and a kernel boundary per step
// disappears.  A workgroup owns EPB = 8 consecutive envs (4 when an env needs 64 lanes) and is made
// of two kinds of waves: 4 stream waves, each copying EPB/4 dynamic slabs with 16-byte accesses
// (the slabs' loads interleaved so all are in flight together) and then updating their column sums
// and masks, and EPB*G/64 placement waves carrying the
// lane-per-cell groups (at raised priority, so their short dependent chain issues promptly).  The
// two kinds never exchange data, so there is no s_barrier: lane groups never span a wave and LDS
// hand-offs only need compiler ordering.  (A first version that let the same waves stream and then
// place showed no gain: every workgroup was in the same phase at the same time.)
// The common 2D step (the reference's window on the shadow, whole workgroups) has a third kind: one mask wave per
// workgroup runs update_mask for all its envs, off the stream waves' tail (tap_transition.h: trans_mask_wave).
// This file: the LB_GREEDY kernel and the tap_transition* entry points; the MACS / MUL kernels of the same shape live in
// transition_macs.hip (tap_transition_macs_launch), so that the two halves compile side by side.
#include <cstdlib>
#include <new>

#include "tap_common.h"
#include "tap_macs.h"
#include "tap_macs3.h"
#include "tap_masks.h"
#include "tap_place.h"
#include "tap_transition.h"
#include "tap_waves.h"

// (TAP_MASK_HOT_PARAMS, tap_masks.h: the load addresses of the stream waves -- and of the placement waves' gather, which
//  reads the same `ptr` and `static` -- arrive in SGPRs with the wave)
template <int D, int G, int NC, int SW, int MODE>
__global__ void __launch_bounds__((trans_threads<D, G, NC, SW, MODE>())) k_transition(TAP_MASK_HOT_PARAMS, TransArgs a)
{
    using Geo = TransGeom<G, SW>;
    constexpr int EPB = Geo::EPB, SPW = Geo::SPW, ENV_WAVES = Geo::ENV_WAVES;
    constexpr bool MASKW = trans_mask_wave<D, G, NC, SW, MODE>();   // one more wave, behind the stream waves: update_mask
    extern __shared__ float trans_lds[];
    __shared__ int s_old[64 * ENV_WAVES];
    __shared__ int s_new[64 * ENV_WAVES];
    // The wave's index in a SCALAR register (two-slab stream waves: 2D windows): everything a stream wave derives from it --
    // its envs, every load and store address -- is then scalar arithmetic + lane offsets instead of 64-bit vector
    // multiplies in front of the first load.  Round 6, same session: c2 1 380 -> 1 440 M
    // env-steps/s; c3 (one slab per wave) 545 -> 541 M, the MACS steps flat, the rolling step 530 -> 491 M -- so only here,
    // and only for SPW > 1.
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = TransGeom<G, SW>::SPW > 1 ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
    const int env_base = blockIdx.x * EPB;

#if defined(TAP_PROF) || defined(TAP_PROF_SWITCH)
    // decomposition switches (scripts/decompose_step.py): run only one kind of wave, or none ("empty kernel of the geometry")
    if (wave >= ENV_WAVES ? (a.flags & TAP_T_PROF_NOSTREAM) : (a.flags & TAP_T_PROF_NOPLACE)) return;
#endif
    if (wave >= ENV_WAVES) {
        const MaskArgs m = tap_mask_hot(a.m, (MODE & 3) == 1, TAP_MASK_HOT_NAMES);
        if constexpr (MASKW) {
            if (wave == ENV_WAVES + Geo::STREAM_WAVES) {     // at the stream waves' priority (raised ones starve the placement chain)
                mask_wave_bits<EPB, 5>(m, env_base, lane);
                return;
            }
        }
        trans_stream_wave<SPW, NC, MODE, MASKW>(m, env_base + (wave - ENV_WAVES) * SPW, lane,
                                            trans_lds + (size_t)(wave - ENV_WAVES) * SPW * 3 * h_nR);
        return;
    }

    // ---- placement waves (tools.py:3663-3744): their latency chain runs beside the stream --------
    __builtin_amdgcn_s_setprio(2);
    const int cell = tid % G;
    TL_STAMP(0);
    StepArgs sa = a.s;       // the gather's source is the update's: ptr, static and their sizes are already in SGPRs
    sa.ptr = h_ptr; sa.static_ = h_static; sa.nR = h_nR; sa.static_rows = h_static_rows; sa.d.B = h_B;
    tap_lb_place_wave<D, G>(sa, a.flags, a.ratio_out, env_base + tid / G, cell, lane,
                            s_old + (tid - cell), s_new + (tid - cell));
    TL_WAIT_VM();
    TL_STAMP(3);
}

#ifdef TAP_PROF
extern "C" int tap_prof_read_timeline(unsigned long long *out, int clear)
{
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(tap_prof_tl), sizeof(unsigned long long) * TAP_PROF_WGS * TAP_PROF_WAVES * 4);
    if (clear) {
        static unsigned long long zeros[TAP_PROF_WGS * TAP_PROF_WAVES * 4];
        (void)hipMemcpyToSymbol(HIP_SYMBOL(tap_prof_tl), zeros, sizeof(zeros));
    }
    return 0;
}
#endif

// (Round 4, measured and removed: ONE LANE per container for the 2D placement inside this kernel -- the corners walked
//  one after the other with the height-map in registers, no LDS, no cross-lane step -- to cut the placement's vector
//  instructions for large batches.  SQ_INSTS_VALU per launch at c2 went UP, 1.94 M -> 2.27 M (the corner and footprint
//  loops run predicated over 8 x 8 register cells on every lane), the step from 6.86 to 7.48 us at B = 8192 (the serial
//  chain of up to five scored corners becomes the launch's tail), and at B = 1 M nothing moved (877 against 898 M
//  env-steps/s): the saturated regime is not bound by vector issue -- 248 M vector instructions per 1.16 ms launch are
//  35 % of the SIMDs' issue slots.)
int tap_transition_macs_launch(tap_ctx *ctx, const tap_env_desc *d, const TransArgs &a, hipStream_t st);   // transition_macs.hip
// big.hip: LB_GREEDY containers above 64 cells -- one wavefront per container + stream waves, on the bit shadow
bool tap_big_transition_ok(const tap_ctx *ctx, const tap_env_desc *d, int nR);
int tap_big_transition(tap_ctx *ctx, const tap_env_desc *d, const TransArgs &a, hipStream_t st);
// macs_big.hip / macs3_big.hip: the wave-per-container MACS placements with the stream waves beside them (mask update +
// placement in one launch; a fresh container and calc_ratio stay launches of their own at the two ends of an episode)
bool tap_macs_wave_transition_ok(const tap_ctx *ctx, const tap_env_desc *d, int nR);
int tap_macs_wave_transition(tap_ctx *ctx, const tap_env_desc *d, const TransArgs &a, hipStream_t st);
bool tap_macs3_wave_transition_ok(const tap_ctx *ctx, const tap_env_desc *d, int nR);
int tap_macs3_wave_transition(tap_ctx *ctx, const tap_env_desc *d, const TransArgs &a, hipStream_t st);
int tap_macs2d_wave_from();                                                                                 // macs.hip

// the step of a wave-per-container shape on the bit shadow: a.m is filled in
static int transition_wave_launch(tap_ctx *ctx, const tap_env_desc *d, void *state, const TransArgs &a, TapStepRoute route, void *stream)
{
    if (route == TAP_ROUTE_WAVE_BIG) return tap_big_transition(ctx, d, a, (hipStream_t)stream);      // handles fresh / ratio itself
    int rc = TAP_OK;
    if ((a.flags & TAP_T_FRESH) && (rc = tap_env_reset(ctx, d, state, stream)) != TAP_OK) return rc;
    rc = route == TAP_ROUTE_WAVE_MACS2 ? tap_macs_wave_transition(ctx, d, a, (hipStream_t)stream)
                                       : tap_macs3_wave_transition(ctx, d, a, (hipStream_t)stream);
    if (rc == TAP_OK && (a.flags & TAP_T_RATIO)) rc = tap_env_ratio(ctx, d, state, a.ratio_out, nullptr, nullptr, stream);
    return rc;
}
int tap_macs_validate(tap_ctx *ctx, const tap_env_desc &d);                                                    // macs.hip

template <int D, int G, int SW>
static int launch_transition_v(tap_ctx *ctx, const TransArgs &a, hipStream_t st)
{
    constexpr int EPB = TransGeom<G, SW>::EPB;
    const int grid = (a.s.d.B + EPB - 1) / EPB;
    if (grid == 0) return TAP_OK;
    const size_t lds = (size_t)EPB * 3 * a.m.nR * sizeof(float);
    const TapVariant v = tap_stream_variant(TAP_SV_TRANSITION, tap_mask_facts(a.m), TapLaunchFacts{D, G, EPB, a.s.d.B, 0, 0, false});
    return tap_launch_variant<TAP_SV_TRANSITION, D, G>(ctx, "k_transition", v, a.m.wt, [&](auto k) -> int {
        using K = decltype(k);
        hipLaunchKernelGGL((k_transition<D, G, K::nc, SW, K::mode>), dim3(grid), dim3(trans_threads<D, G, K::nc, SW, K::mode>()), K::nc ? lds : 0, st,
                           TAP_MASK_HOT_ARGS(a.m), a);
        return TAP_OK;
    });
}

template <int D, int G> static int launch_transition(tap_ctx *ctx, const TransArgs &a, hipStream_t st)
{
    // Stream waves per workgroup of 8 envs.  2D windows (2 400-byte slabs at n = 10): 4, two slabs per wave (8: c2 1 349 ->
    // 1 216 M env-steps/s, 1 903 -> 1 753 M at B = 65 536).  3D windows (7 200-byte slabs): 8, one slab per wave -- c3
    // 507 -> 543 M at B = 4 096, 556 -> 598 M at 8 192, 549 -> 574 M at 16 384, 605 -> 620 M at 65 536, equal from 262 144
    // (round 5, on the kernels with the compiled-in window shape; round 4 had measured 4 as the best for both at c2's
    // shape only).
    return launch_transition_v<D, G, (D == 3 ? 8 : 4)>(ctx, a, st);
}

// the lane-per-cell fused kernels (tap_step_request.h: TAP_ROUTE_FUSED)
static int transition_dispatch(tap_ctx *ctx, const tap_env_desc *d, const TransArgs &a, void *stream)
{
    if (d->strategy == TAP_MACS) return tap_transition_macs_launch(ctx, d, a, (hipStream_t)stream);
    TAP_DISPATCH_DG(launch_transition, d, ctx, a, (hipStream_t)stream);
}

// What tap_step_route asks of the families' files (tap_step_request.h: TapStepCaps), each asked of the family whose
// container this is: the wave kernels' own fits, and for the MACS lane kernels, which keep their lists in LDS, whether a
// workgroup's envs fit its LDS (160 KiB on gfx950) next to the stream tiles
static TapStepCaps transition_caps(const tap_ctx *ctx, const tap_env_desc *d, int nR)
{
    TapStepCaps c = {};
    c.macs2d_wave_from = tap_macs2d_wave_from();
    if (tap_is_big(d)) c.big_ok = tap_big_transition_ok(ctx, d, nR);
    else if (d->strategy != TAP_MACS) return c;
    else if (d->D == 2 && d->W > 16) c.macs_wave_ok = tap_macs_wave_transition_ok(ctx, d, nR);
    else if (tap_is_big_macs3(d)) c.macs3_wave_ok = tap_macs3_wave_transition_ok(ctx, d, nR);
    else {
        const int G = tap_group_size(d), epb = G == 64 ? 4 : 8;
        const size_t words = d->D == 3 ? (size_t)macs3_group_words(G, d->n_max, d->H)
                                       : (size_t)macs_group_words(d->W <= 8 ? 8 : 16, d->H, d->n_max, d->W);
        c.macs_lanes_fit = (size_t)epb * 3 * nR * sizeof(float) + (size_t)epb * words * sizeof(int) <= tap_lds_limit(ctx);
    }
    return c;
}

// the by-products a decoding loop wants from the step's gather, for the shapes that run as two launches (the fused
// kernels' placement waves write them: tap_common.h, tap_step_aux)
__global__ void __launch_bounds__(TAP_BLOCK) k_step_aux(StepArgs s)
{
    const int env = blockIdx.x * TAP_BLOCK + threadIdx.x;
    if (env >= s.d.B) return;
    bool badp;
    const long praw = (long)s.ptr[env];
    const long p = tap_col(praw, s.nR, badp);
    float fv[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < s.d.D; ++k) {
        const float v = s.static_[((size_t)env * s.static_rows + 1 + k) * s.nR + p];
        fv[k] = badp ? 0.f : v;
    }
    tap_step_aux(s, env, s.d.D, fv, praw);
}

int tap_step_aux_launch(tap_ctx *ctx, const StepArgs &s, hipStream_t st)
{
    if (!(s.dec_static_out || s.tour_out || s.picked_out) || s.d.B == 0) return TAP_OK;
    hipLaunchKernelGGL(k_step_aux, dim3((s.d.B + TAP_BLOCK - 1) / TAP_BLOCK), dim3(TAP_BLOCK), 0, st, s);
    TAP_LAUNCH_CHECK(ctx, "k_step_aux");
    return TAP_OK;
}

extern "C" int tap_transition_launches(const tap_ctx *ctx, const tap_env_desc *d, int n, int R, int rows, int on_bits)
{
    if (!d || n < 1 || R < 1 || rows < 1) return TAP_E_INVALID;
    TapStepRequest r = {};
    r.form = on_bits ? TAP_STEP_BITS : TAP_STEP_COPY; r.rows = rows;
    return tap_step_route_launches(tap_step_route(r, *d, transition_caps(ctx, d, n * R)));
}

static int transition_tail(tap_ctx *ctx, const tap_env_desc *d, void *state, const TransArgs &a, void *stream)
{
    int rc = tap_env_step_gather(ctx, d, state, a.s.static_, a.s.static_rows, a.s.nR, a.s.ptr, nullptr, a.s.feature_out, stream);
    if (rc == TAP_OK && (a.flags & TAP_T_RATIO)) rc = tap_env_ratio(ctx, d, state, a.ratio_out, nullptr, nullptr, stream);
    return rc ? rc : tap_step_aux_launch(ctx, a.s, (hipStream_t)stream);
}

// One step, whatever its form and its caller: check, route, then the wave launch, the fused dispatch or the two launches.
static int transition_impl(tap_ctx *ctx, const tap_env_desc *d, void *state, const TapStepRequest &r, bool from_stepper, void *stream)
{
    int rc = tap_desc_validate(ctx, d);
    if (rc || d->B == 0) return rc;     // an empty batch has no buffers to check
    if (d->strategy == TAP_MACS && (rc = tap_macs_validate(ctx, *d)) != TAP_OK) return rc;
    const TapStepVerdict v = tap_step_request_check(r, d->B, d->D, from_stepper, state != nullptr);
    if (v.status != TAP_OK) return tap_fail(ctx, v.status, "%s", v.msg);
    TransArgs a = {};
    a.s.d = *d;
    tap_env_layout(d, state, &a.s.v);
    a.s.static_ = r.static_; a.s.static_rows = r.static_rows; a.s.nR = r.n * r.R; a.s.ptr = r.ptr;
    a.s.feature_out = r.feature_out; a.s.flen = tap_env_feature_len(d);
    a.s.lut = ctx ? ctx->stab_lut : nullptr;
    a.s.dec_static_out = r.aux.dec_static_out; a.s.tour_out = r.aux.tour_out;
    a.s.tour_stride = r.aux.tour_stride; a.s.tour_col = r.aux.tour_col;
    a.flags = r.flags;
    a.ratio_out = r.ratio_out;

    const TapStepRoute route = tap_step_route(r, *d, transition_caps(ctx, d, r.n * r.R));
    if (route == TAP_ROUTE_TWO_LAUNCHES) {
        if ((r.flags & TAP_T_FRESH) && (rc = tap_env_reset(ctx, d, state, stream)) != TAP_OK) return rc;
        if (r.form == TAP_STEP_COPY)
            rc = tap_mask_step(ctx, d->B, r.n, r.R, r.rows, r.update_rows, r.dyn_in, r.static_, r.static_rows, r.ptr, r.mask_in,
                               r.colsum_in, r.dyn_out, r.colsum_out, r.current_out, r.mask_out, stream);
        else if (r.form == TAP_STEP_BITS)
            rc = tap_mask_step_bits(ctx, d->B, r.n, r.R, r.rows, r.update_rows, r.bits_in, r.static_, r.static_rows, r.ptr, r.mask_in,
                                    r.bits_out, r.dyn_out, r.current_out, r.mask_out, stream);
        else
            rc = tap_mask_step_first(ctx, d->B, r.n, r.R, r.rows, r.update_rows, r.dyn_in, r.static_, r.static_rows, r.ptr, r.mask_in,
                                     r.bits_out, r.dyn_out, r.current_out, r.mask_out, r.nonbinary_out, stream);
        return rc ? rc : transition_tail(ctx, d, state, a, stream);
    }
    a.m = mask_args(r, d->B);
    if (route == TAP_ROUTE_FUSED) a.m.inplace = (r.inplace && r.dyn_out) ? 1 : 0;
    if (r.form != TAP_STEP_COPY && (rc = mask_bits_check(ctx, a.m)) != TAP_OK) return rc;
    return route == TAP_ROUTE_FUSED ? transition_dispatch(ctx, d, a, stream) : transition_wave_launch(ctx, d, state, a, route, stream);
}

extern "C" int tap_transition(tap_ctx *ctx, const tap_env_desc *d, void *state, int n, int R, int rows,
                              int update_rows, const float *dyn_in, const float *static_,
                              int static_rows, const int64_t *ptr, const float *mask_in,
                              const float *colsum_in, float *dyn_out, float *colsum_out,
                              float *current_out, float *mask_out, float *feature_out,
                              float *ratio_out, int flags, void *stream)
{
    TapStepRequest r = {};
    r.form = TAP_STEP_COPY;
    r.n = n; r.R = R; r.rows = rows; r.update_rows = update_rows; r.static_rows = static_rows; r.flags = flags;
    r.dyn_in = dyn_in; r.static_ = static_; r.ptr = ptr; r.mask_in = mask_in; r.colsum_in = colsum_in;
    r.dyn_out = dyn_out; r.colsum_out = colsum_out; r.current_out = current_out; r.mask_out = mask_out;
    r.feature_out = feature_out; r.ratio_out = ratio_out;
    // (this entry point has always asked for its mask ahead of the descriptor's checks)
    if (d && d->B > 0 && !mask_in) return tap_fail(ctx, TAP_E_INVALID, "%s", tap_step_request_check(r, d->B, d->D, false, state != nullptr).msg);
    return transition_impl(ctx, d, state, r, false, stream);
}

extern "C" int tap_transition_bits(tap_ctx *ctx, const tap_env_desc *d, void *state, int n, int R, int rows,
                                   int update_rows, const unsigned long long *bits_in, const float *static_,
                                   int static_rows, const int64_t *ptr, const float *mask_in,
                                   unsigned long long *bits_out, float *dyn_out, float *current_out,
                                   float *mask_out, float *feature_out, float *ratio_out, int flags,
                                   void *stream)
{
    TapStepRequest r = {};
    r.form = TAP_STEP_BITS;
    r.n = n; r.R = R; r.rows = rows; r.update_rows = update_rows; r.static_rows = static_rows; r.flags = flags;
    r.bits_in = bits_in; r.static_ = static_; r.ptr = ptr; r.mask_in = mask_in;
    r.bits_out = bits_out; r.dyn_out = dyn_out; r.current_out = current_out; r.mask_out = mask_out;
    r.feature_out = feature_out; r.ratio_out = ratio_out;
    return transition_impl(ctx, d, state, r, false, stream);
}

extern "C" int tap_transition_first(tap_ctx *ctx, const tap_env_desc *d, void *state, int n, int R, int rows,
                                    int update_rows, const float *dyn_in, const float *static_, int static_rows,
                                    const int64_t *ptr, const float *mask_in, unsigned long long *bits_out,
                                    float *dyn_out, float *current_out, float *mask_out, float *feature_out,
                                    float *ratio_out, int32_t *nonbinary_out, int flags, void *stream)
{
    TapStepRequest r = {};
    r.form = TAP_STEP_FIRST;
    r.n = n; r.R = R; r.rows = rows; r.update_rows = update_rows; r.static_rows = static_rows; r.flags = flags;
    r.dyn_in = dyn_in; r.static_ = static_; r.ptr = ptr; r.mask_in = mask_in;
    r.bits_out = bits_out; r.dyn_out = dyn_out; r.current_out = current_out; r.mask_out = mask_out;
    r.feature_out = feature_out; r.ratio_out = ratio_out; r.nonbinary_out = nonbinary_out;
    return transition_impl(ctx, d, state, r, false, stream);
}

// ---- tap_stepper: the step object of a decoding loop (tapenv.h) --------------------------------------------------
// Host-side only: the buffers stay the caller's; the stepper remembers them, alternates the two phases and tells
// the fused launch which by-products to write.  A step is then one C call with two arguments.
struct tap_stepper {
    tap_ctx *ctx;
    tap_env_desc d;
    void *state;
    int n, R, rows, update_rows, static_rows, steps;
    tap_stepper_buffers b;
    const float *static_;
    const float *dyn_in;                // step 0 builds the shadow from this fp32 tensor ...
    const unsigned long long *bits0;    // ... or reads this one (begin's own launch, or the caller's)
    const float *mask0;                 // the mask step 0 starts from (null = ones)
    int k;                              // index of the next step
    int keep;                           // TAP_SB_CONTINUE: step 0 does not start from a fresh container
    int copy_form;                      // the window has no bit shadow: `dynamic` is carried as the fp32 tensor + column sums
    int inplace;                        // dyn[0] == dyn[1]: ONE fp32 tensor, updated in place from the second step on
};

struct DeviceGuard { // the launches must be issued with the context's device current (callers may sit on another one)
    int prev, want;
    explicit DeviceGuard(int dev) : prev(-1), want(dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != want) (void)hipSetDevice(want);
    }
    ~DeviceGuard() { if (prev >= 0 && prev != want) (void)hipSetDevice(prev); }
};

extern "C" int tap_stepper_create(tap_ctx *ctx, const tap_env_desc *d, void *state, int n, int R, int rows,
                                  int update_rows, int static_rows, int steps, const tap_stepper_buffers *buf,
                                  tap_stepper **out)
{
    if (!ctx || !d || !buf || !out) return TAP_E_INVALID;
    int rc = tap_desc_validate(ctx, d);
    if (rc) return rc;
    if (n < 1 || R < 1 || rows < 1 || update_rows < 0 || update_rows > 3 || static_rows < 1 + d->D || steps < 1)
        return tap_fail(ctx, TAP_E_INVALID, "bad stepper arguments");
    if (d->B > 0) {                                  // an empty batch has no buffers to check
        if (!state) return tap_fail(ctx, TAP_E_INVALID, "bad stepper arguments");
        const bool shadow = tap_window_has_shadow(rows, n * R);
        for (int w = 0; w < 2; ++w)
            if ((shadow && !buf->bits[w]) || !buf->current[w] || !buf->mask[w])
                return tap_fail(ctx, TAP_E_INVALID, "stepper needs both phases of bits / current / mask");
        if (!shadow) {
            // a window beyond the bit shadow (nR % 4 != 0, nR > 256 or rows > 128): the step is tap_transition's fp32-copy
            // form on the column-sum shadow -- both phases of dyn and of colsum (B, 3, nR) are required
            if (!buf->dyn[0] || !buf->dyn[1] || !buf->colsum[0] || !buf->colsum[1] || buf->colsum[0] == buf->colsum[1])
                return tap_fail(ctx, TAP_E_INVALID, "a stepper for a window without a bit shadow needs both phases of dyn and colsum");
        }
        // dyn: both phases, or neither -- a caller whose encoder consumes the bit shadow skips the fp32 expansion of
        // update_dynamic's result (78 % of a c2 step's bytes); masks, placements and ratio do not depend on it
        if ((buf->dyn[0] == nullptr) != (buf->dyn[1] == nullptr))
            return tap_fail(ctx, TAP_E_INVALID, "stepper needs both phases of dyn, or neither (no fp32 expansion)");
        // dyn[0] == dyn[1] (windows with a bit shadow): ONE fp32 tensor for the whole episode.  The step never reads it (the
        // shadow carries `dynamic`), and update_dynamic's result differs from its input in the chosen rows only, so from
        // the second step on a step writes those rows' zeros instead of the whole tensor (the reference's clone, pack.py:368,
        // exists for autograd: a loop under no_grad -- validation, serving -- has no use for the previous tensors)
        if ((shadow && buf->bits[0] == buf->bits[1]) || (!shadow && buf->dyn[0] == buf->dyn[1]) || buf->current[0] == buf->current[1] ||
            buf->mask[0] == buf->mask[1] || !buf->ratio)
            return tap_fail(ctx, TAP_E_INVALID, "stepper phases must be distinct buffers (dyn may be one buffer on the bit shadow) and ratio is required");
    }
    if (buf->tour_stride < 0 || buf->tour_col0 < 0 || (buf->tour_stride > 0 && buf->tour_col0 + steps > buf->tour_stride))
        return tap_fail(ctx, TAP_E_INVALID, "stepper tour columns [col0, col0 + steps) must fit tour_stride");
    tap_stepper *s = new (std::nothrow) tap_stepper();
    if (!s) return tap_fail(ctx, TAP_E_INVALID, "out of host memory");
    s->ctx = ctx; s->d = *d; s->state = state;
    s->n = n; s->R = R; s->rows = rows; s->update_rows = update_rows; s->static_rows = static_rows; s->steps = steps;
    s->b = *buf;
    s->static_ = nullptr; s->dyn_in = nullptr; s->bits0 = nullptr; s->mask0 = nullptr; s->k = 0; s->keep = 0;
    s->copy_form = tap_window_has_shadow(rows, n * R) ? 0 : 1;
    s->inplace = (!s->copy_form && buf->dyn[0] && buf->dyn[0] == buf->dyn[1]) ? 1 : 0;
    *out = s;
    return TAP_OK;
}

extern "C" void tap_stepper_destroy(tap_stepper *s) { delete s; }

extern "C" int tap_stepper_begin(tap_stepper *s, const float *static_, const float *dyn_in, int flags, void *stream)
{
    if (!s) return TAP_E_INVALID;
    if ((!static_ || !dyn_in) && s->d.B > 0) return tap_fail(s->ctx, TAP_E_INVALID, "stepper_begin needs static and dynamic");
    if (s->d.B == 0) static_ = reinterpret_cast<const float *>(s); // any non-null token: "begun"
    s->static_ = static_;
    s->dyn_in = dyn_in;
    s->bits0 = nullptr;
    s->mask0 = nullptr;
    s->k = 0;
    s->keep = (flags & TAP_SB_CONTINUE) != 0;
    if (s->copy_form && s->d.B > 0) {
        // no bit shadow: the column sums of the fresh tensor and the masks DRL.forward starts from (model.py:297-307;
        // mask = ones) into phase 1, which step 0 reads -- two small launches, with or without TAP_SB_INITIAL_MASK
        DeviceGuard g(s->ctx->device);
        int rc = tap_dyn_colsum(s->ctx, s->d.B, s->n, s->n * s->R, s->rows, dyn_in, s->b.colsum[1], stream);
        // the incremental column sums are exact for 0/1 tensors only: count the other elements like the shadow builders do
        if (rc == TAP_OK && s->b.nonbinary)
            rc = tap_dyn_bits(s->ctx, s->d.B, s->n * s->R, s->rows, dyn_in, nullptr, s->b.nonbinary, stream);
        if (rc == TAP_OK)
            rc = tap_update_mask(s->ctx, s->d.B, s->n, s->R, nullptr, s->b.colsum[1], nullptr, s->b.current[1], s->b.mask[1], stream);
        if (rc != TAP_OK) { s->static_ = nullptr; return rc; }
        s->mask0 = s->b.mask[1];
        return TAP_OK;
    }
    if (!(flags & TAP_SB_INITIAL_MASK) || s->d.B == 0) return TAP_OK;
    // shadow + the masks DRL.forward starts from (model.py:297-307) in one launch that reads the tensor once; they
    // land in phase 1, which step 0 (writing phase 0) reads
    DeviceGuard g(s->ctx->device);
    const int rc = tap_mask_step_first(s->ctx, s->d.B, s->n, s->R, s->rows, 0, dyn_in, nullptr, 0, nullptr, nullptr,
                                       s->b.bits[1], nullptr, s->b.current[1], s->b.mask[1], s->b.nonbinary, stream);
    if (rc != TAP_OK) { s->static_ = nullptr; return rc; }
    s->bits0 = s->b.bits[1];
    s->mask0 = s->b.mask[1];
    return TAP_OK;
}

extern "C" int tap_stepper_begin_shadow(tap_stepper *s, const float *static_, const unsigned long long *bits, int flags)
{
    if (!s) return TAP_E_INVALID;
    if (s->copy_form) return tap_fail(s->ctx, TAP_E_UNSUPPORTED, "this window has no bit shadow: begin with tap_stepper_begin");
    if (s->d.B > 0 && (!static_ || !bits || bits == s->b.bits[0]))
        return tap_fail(s->ctx, TAP_E_INVALID, "stepper_begin_shadow needs static and a shadow that is not phase 0's buffer");
    if (s->d.B == 0) static_ = reinterpret_cast<const float *>(s);
    s->static_ = static_;
    s->dyn_in = nullptr;
    s->bits0 = bits;
    s->mask0 = nullptr;
    s->k = 0;
    s->keep = (flags & TAP_SB_CONTINUE) != 0;
    return TAP_OK;
}

extern "C" int tap_stepper_step(tap_stepper *s, const int64_t *ptr, void *stream)
{
    if (!s) return TAP_E_INVALID;
    if (!s->static_) return tap_fail(s->ctx, TAP_E_INVALID, "tap_stepper_begin has not been called");
    if (s->k >= s->steps) return tap_fail(s->ctx, TAP_E_STEPS, "the episode already took its %d steps", s->steps);
    if (s->d.B == 0) { s->k += 1; return TAP_OK; }
    const int k = s->k, w = k & 1, r = w ^ 1;
    const int flags = ((k == 0 && !s->keep) ? TAP_T_FRESH : 0) | (k == s->steps - 1 ? TAP_T_RATIO : 0);
    TapStepRequest q = {};
    q.n = s->n; q.R = s->R; q.rows = s->rows; q.update_rows = s->update_rows; q.static_rows = s->static_rows; q.flags = flags;
    q.static_ = s->static_; q.ptr = ptr; q.mask_in = k == 0 ? s->mask0 : s->b.mask[r];
    q.dyn_out = s->b.dyn[w]; q.current_out = s->b.current[w]; q.mask_out = s->b.mask[w];
    q.feature_out = s->b.feature; q.ratio_out = s->b.ratio;
    q.aux = {s->b.decoder_static, s->b.tour, s->b.tour_stride > 0 ? s->b.tour_stride : s->steps, s->b.tour_col0 + k};
    if (s->copy_form) {
        q.form = TAP_STEP_COPY;
        q.dyn_in = k == 0 ? s->dyn_in : s->b.dyn[r];
        q.colsum_in = s->b.colsum[k == 0 ? 1 : r]; q.colsum_out = s->b.colsum[w];
    } else if (k == 0 && !s->bits0) {
        q.form = TAP_STEP_FIRST;
        q.dyn_in = s->dyn_in; q.mask_in = nullptr;
        q.bits_out = s->b.bits[w]; q.nonbinary_out = s->b.nonbinary;
    } else {
        q.form = TAP_STEP_BITS;
        q.bits_in = k == 0 ? s->bits0 : s->b.bits[r]; q.bits_out = s->b.bits[w];
        q.inplace = (k > 0 && s->inplace) ? 1 : 0;
    }
    DeviceGuard g(s->ctx->device);
    const int rc = transition_impl(s->ctx, &s->d, s->state, q, true, stream);
    if (rc == TAP_OK) s->k = k + 1;
    return rc;
}

extern "C" int tap_stepper_steps_done(const tap_stepper *s) { return s ? s->k : TAP_E_INVALID; }
