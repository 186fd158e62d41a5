// policy.hip -- the decoding head: the line between the pointer network and step(ptr).  The reference does it in
// model.py:359-372: probs = softmax(logits + current_mask.log()), Categorical(probs).sample() inside a host loop that
// rejects unselectable picks (training) or torch.max (testing), then log_prob / prob.log().  Here ONE launch turns the
// network's logits (B, nR) and the stepper's current_mask into ptr, logp and (when wanted) probs, and a second small
// launch is the backward of logp with respect to the logits.
//
// Semantics per row (tapenv.h: tap_policy_pick has the contract): a column is selectable iff mask != 0; logits of
// unselectable columns never enter an arithmetic result (they are replaced by a select, so NaN and +-inf there change
// nothing); everything is fp64: m = max of the selectable logits, w_c = exp(l_c - m), S = sum of w.  Sampling takes a
// PRE-DRAWN uniform u in [0, 1): t = u * S and ptr = the first selectable column whose inclusive prefix sum of w is
// > t, the last selectable column when none is (t >= S) -- an unselectable column can never be returned, so the
// reference's rejection loop and its host synchronisation are gone.  Greedy takes the first selectable column whose
// logit equals m.  logp = (l_ptr - m) - log S.  A row without a selectable column: ptr 0, logp NaN, probs 0.
//
// Geometry.  nR <= 64: a LANE GROUP per row, G = 8 / 16 / 32 / 64 the smallest that holds the row, 64 / G rows per
// wavefront; loads unconditional on clamped addresses, then the select (trial.hip, tap_waves.h); the max by the DPP
// butterfly of tap_place.h, the fp64 inclusive scan in log2(G) shuffle-up steps, the pick a ballot of (cum > t) and a
// find-first-set.  nR > 64: ONE WAVEFRONT per row in 64-column chunks: a max pass, then the weight pass -- the same
// scan with a wave-uniform running prefix carried from chunk to chunk -- twice: once for S, which the threshold
// t = u * S needs before any column can be compared, and once for the pick (the same instructions in the same order,
// so both passes see bit-identical prefix sums; the row stays in the cache between them).  No LDS, no barrier, no
// atomics, plain stores.  A ragged last wave of the group form runs on a clamped row with its stores suppressed (the
// DPP steps need every lane); in the chunked form the whole wave leaves.
#include "tap_common.h"
#include "tap_decoder.h"
#include "tap_place.h"
#include "tap_pick.h"

namespace {

constexpr int TAP_HIT_POLICY_PICK = 26; // launch record (tapenv.h: tap_variant_hits), after trial.hip's 25

struct PickArgs {
    const float *logits; // (B, nR)
    const float *mask;   // (B, nR)
    const float *u;      // (B,) or null (greedy)
    int B, nR;
    int64_t *ptr;        // (B,)
    float *logp;         // (B,)
    float *probs;        // (B, nR) or null
};

// group_fmaxf, scan_up, wave_read, pick_logp, pick_chunk and draw_uniform: tap_pick.h (pointer.hip's fused launch runs them too)

template <int G, bool GREEDY>
__global__ void __launch_bounds__(TAP_BLOCK) k_policy_pick(PickArgs a)
{
    constexpr int EPB = TAP_BLOCK / G;
    constexpr u64 GM = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1);
    const int tid = threadIdx.x, lane = tid & 63, cell = lane % G, gl0 = lane - cell, nR = a.nR;
    const long long row = (long long)blockIdx.x * EPB + tid / G;
    const bool live = row < a.B;                                // a ragged last wave: clamped row, no store
    const size_t env = (size_t)(live ? row : a.B - 1);
    const bool inr = cell < nR;
    const size_t at = env * nR + min(cell, nR - 1);
    const float l_raw = a.logits[at], mv = a.mask[at];
    float uu = 0.f;
    if (!GREEDY) uu = a.u[env];
    const bool sel = inr && mv != 0.f;
    const float ninf = -__builtin_huge_valf();
    const float l = sel ? l_raw : ninf;                         // an unselectable logit goes no further
    const float m = group_fmaxf<G>(l);
    const u64 selb = (__ballot(sel) >> gl0) & GM;
    const bool any = selb != 0;
    const double w = sel ? exp((double)l - (double)m) : 0.0;
    const double cum = scan_up<G>(w, cell);
    const double S = __shfl(cum, G - 1, G);
    u64 q;
    if (GREEDY) q = __ballot(sel && l == m);
    else q = __ballot(sel && cum > (double)uu * S);
    q = (q >> gl0) & GM;
    const int p = q ? __ffsll((long long)q) - 1 : any ? 63 - __clzll((long long)selb) : 0;
    const float l_ptr = __shfl(l, gl0 + p);
    if (live && cell == 0) {
        a.ptr[env] = p;
        a.logp[env] = pick_logp(any, l_ptr, m, S);
    }
    if (a.probs && live && inr) a.probs[env * nR + cell] = any ? (float)(w / S) : 0.f;
}

template <bool GREEDY>
__global__ void __launch_bounds__(TAP_BLOCK) k_policy_pick_wide(PickArgs a)
{
    const int lane = threadIdx.x & 63, nR = a.nR;
    const long long row = (long long)blockIdx.x * (TAP_BLOCK / 64) + TAP_WAVE_INDEX();
    if (row >= a.B) return;                                     // the whole wave leaves: nothing below spans waves
    const size_t env = (size_t)row;
    const float *lrow = a.logits + env * nR, *mrow = a.mask + env * nR;
    const float ninf = -__builtin_huge_valf();
    float m = ninf;
    bool mine = false;
    for (int base = 0; base < nR; base += 64) {                 // the max pass
        const int col = base + lane, at = min(col, nR - 1);
        const float l_raw = lrow[at], mv = mrow[at];
        const bool sel = col < nR && mv != 0.f;
        m = fmaxf(m, sel ? l_raw : ninf);
        mine |= sel;
    }
    m = group_fmaxf<64>(m);
    const bool any = __ballot(mine) != 0;
    double S = 0.0;
    int p = -1;
    for (int base = 0; base < nR; base += 64) {                 // the weight pass, for S (and the greedy pick)
        const Chunk c = pick_chunk(lrow, mrow, base, lane, nR, m, S);
        if (GREEDY && p < 0) {
            const u64 q = __ballot(c.sel && c.l == m);
            if (q) p = base + __ffsll((long long)q) - 1;
        }
    }
    if (!GREEDY || a.probs) {                                   // the weight pass again, for the pick and the probabilities
        const double t = GREEDY ? 0.0 : (double)a.u[env] * S;
        double run = 0.0;
        int last = 0;
        for (int base = 0; base < nR; base += 64) {
            const Chunk c = pick_chunk(lrow, mrow, base, lane, nR, m, run);
            if (!GREEDY) {
                const u64 q = __ballot(c.sel && c.cum > t), sb = __ballot(c.sel);
                if (p < 0 && q) p = base + __ffsll((long long)q) - 1;   // the first chunk with a qualifying column decides
                if (sb) last = base + 63 - __clzll((long long)sb);
            }
            if (a.probs) { if (c.inr) a.probs[env * nR + base + lane] = any ? (float)(c.w / S) : 0.f; }
            else if (p >= 0) break;                             // wave-uniform
        }
        if (!GREEDY && p < 0) p = last;                         // t >= S: the last selectable column (0 on an empty row)
    }
    if (p < 0) p = 0;
    const float l_ptr = lrow[p];
    if (lane == 0) {
        a.ptr[env] = p;
        a.logp[env] = pick_logp(any, l_ptr, m, S);
    }
}

// ---- the DRAW and GIVEN forms (tapenv.h: tap_policy_pick_draw / tap_policy_pick_given) --------------------------------
// Kernels of their own beside the two above, which stay as they are: DRAW is the sampling form with the row's uniform
// computed inside the launch, GIVEN scores a caller's column.  Everything after u (DRAW) and everything up to S (GIVEN) is
// the sampling form's code in the sampling form's order, so the outputs are its bytes.
constexpr int FORM_DRAW = 2, FORM_GIVEN = 3;    // the launch record's variant field, beside GREEDY's 0 / 1

struct FormArgs {
    const float *logits;      // (B, nR)
    const float *mask;        // (B, nR)
    const long long *state;   // DRAW: int64[2] (seed, episode) on the device
    const int64_t *ptr_in;    // GIVEN: (B,)
    unsigned step, env_offset;
    int B, nR;
    int64_t *ptr;             // (B,) DRAW
    float *logp;              // (B,)
    float *probs;             // (B, nR) or null
    float *u_out;             // (B,) or null, DRAW
};

// GIVEN's column: -1 when the caller's value lies outside [0, nR) (it is never used as an address)
__device__ __forceinline__ int given_column(const FormArgs &a, size_t env)
{
    const int64_t p = a.ptr_in[env];
    return p >= 0 && p < (int64_t)a.nR ? (int)p : -1;
}

template <int G, int FORM>
__global__ void __launch_bounds__(TAP_BLOCK) k_policy_pick_form(FormArgs a)
{
    constexpr int EPB = TAP_BLOCK / G;
    constexpr u64 GM = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1);
    const int tid = threadIdx.x, lane = tid & 63, cell = lane % G, gl0 = lane - cell, nR = a.nR;
    const long long row = (long long)blockIdx.x * EPB + tid / G;
    const bool live = row < a.B;                                // a ragged last wave: clamped row, no store
    const size_t env = (size_t)(live ? row : a.B - 1);
    const bool inr = cell < nR;
    const size_t at = env * nR + min(cell, nR - 1);
    const float l_raw = a.logits[at], mv = a.mask[at];
    float uu = 0.f;
    int given = 0;
    if (FORM == FORM_DRAW) uu = draw_uniform(a, env);
    else given = given_column(a, env);
    const bool sel = inr && mv != 0.f;
    const float ninf = -__builtin_huge_valf();
    const float l = sel ? l_raw : ninf;                         // an unselectable logit goes no further
    const float m = group_fmaxf<G>(l);
    const u64 selb = (__ballot(sel) >> gl0) & GM;
    const bool any = selb != 0;
    const double w = sel ? exp((double)l - (double)m) : 0.0;
    const double cum = scan_up<G>(w, cell);
    const double S = __shfl(cum, G - 1, G);
    int p;
    bool ok = true;
    if (FORM == FORM_DRAW) {
        const u64 q = (__ballot(sel && cum > (double)uu * S) >> gl0) & GM;
        p = q ? __ffsll((long long)q) - 1 : any ? 63 - __clzll((long long)selb) : 0;
    } else {
        p = max(given, 0);
        ok = given >= 0 && ((selb >> p) & 1) != 0;             // outside the row or unselectable: logp NaN
    }
    const float l_ptr = __shfl(l, gl0 + p);
    if (live && cell == 0) {
        if (FORM == FORM_DRAW) {
            a.ptr[env] = p;
            if (a.u_out) a.u_out[env] = uu;
        }
        a.logp[env] = ok ? pick_logp(any, l_ptr, m, S) : __builtin_nanf("");
    }
    if (a.probs && live && inr) a.probs[env * nR + cell] = any ? (float)(w / S) : 0.f;
}

template <int FORM>
__global__ void __launch_bounds__(TAP_BLOCK) k_policy_pick_wide_form(FormArgs a)
{
    const int lane = threadIdx.x & 63, nR = a.nR;
    const long long row = (long long)blockIdx.x * (TAP_BLOCK / 64) + TAP_WAVE_INDEX();
    if (row >= a.B) return;                                     // the whole wave leaves: nothing below spans waves
    const size_t env = (size_t)row;
    const float *lrow = a.logits + env * nR, *mrow = a.mask + env * nR;
    const float ninf = -__builtin_huge_valf();
    float m = ninf;
    bool mine = false;
    for (int base = 0; base < nR; base += 64) {                 // the max pass
        const int col = base + lane, at = min(col, nR - 1);
        const float l_raw = lrow[at], mv = mrow[at];
        const bool sel = col < nR && mv != 0.f;
        m = fmaxf(m, sel ? l_raw : ninf);
        mine |= sel;
    }
    m = group_fmaxf<64>(m);
    const bool any = __ballot(mine) != 0;
    double S = 0.0;
    for (int base = 0; base < nR; base += 64) pick_chunk(lrow, mrow, base, lane, nR, m, S);   // the weight pass, for S
    int p = -1;
    bool ok = true;
    float uu = 0.f;
    if (FORM == FORM_GIVEN) {
        const int given = given_column(a, env);
        p = max(given, 0);
        ok = given >= 0 && mrow[p] != 0.f;
    } else {
        uu = draw_uniform(a, env);
    }
    if (FORM == FORM_DRAW || a.probs) {                         // the weight pass again, for the pick and the probabilities
        const double t = (double)uu * S;
        double run = 0.0;
        int last = 0;
        for (int base = 0; base < nR; base += 64) {
            const Chunk c = pick_chunk(lrow, mrow, base, lane, nR, m, run);
            if (FORM == FORM_DRAW) {
                const u64 q = __ballot(c.sel && c.cum > t), sb = __ballot(c.sel);
                if (p < 0 && q) p = base + __ffsll((long long)q) - 1;   // the first chunk with a qualifying column decides
                if (sb) last = base + 63 - __clzll((long long)sb);
            }
            if (a.probs) { if (c.inr) a.probs[env * nR + base + lane] = any ? (float)(c.w / S) : 0.f; }
            else if (p >= 0) break;                             // wave-uniform
        }
        if (FORM == FORM_DRAW && p < 0) p = last;               // t >= S: the last selectable column (0 on an empty row)
    }
    const float l_ptr = lrow[p];
    if (lane == 0) {
        if (FORM == FORM_DRAW) {
            a.ptr[env] = p;
            if (a.u_out) a.u_out[env] = uu;
        }
        a.logp[env] = ok ? pick_logp(any, l_ptr, m, S) : __builtin_nanf("");
    }
}

// dlogits of a column that was not picked: -g p, one fp32 rounding (the picked column's thread recomputes exactly this)
__device__ __forceinline__ float pick_bw_off(float g, float p) { return -(g * p); }

__global__ void __launch_bounds__(TAP_BLOCK) k_policy_pick_backward(const float *probs, const int64_t *ptr, const float *logp,
                                                                    const float *g, size_t total, int nR, float *dlogits)
{
    const size_t i = (size_t)blockIdx.x * TAP_BLOCK + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / (size_t)nR;
    const int c = (int)(i - b * (size_t)nR);
    const float lp = logp[b];
    if (lp != lp) { dlogits[i] = 0.f; return; }                 // an empty row (logp NaN) has no gradient
    const float gb = g[b];
    if (ptr[b] != (int64_t)c) { dlogits[i] = pick_bw_off(gb, probs[i]); return; }
    // the picked column: 1 - p[ptr] is the sum of the other probabilities, so the column is minus the fp64 sum of the
    // row's other fp32 RESULTS, rounded once -- the row then sums to zero within that one rounding, as the true gradient
    // does.  g * (1 - p[ptr]) leaves the roundings of every p in the row sum, and whatever reaches all columns alike
    // downstream (the attention's context) reads that residue as a gradient
    const float *row = probs + b * (size_t)nR;
    double s = 0.0;
    for (int j = 0; j < nR; ++j)
        if (j != c) s += (double)pick_bw_off(gb, row[j]);
    dlogits[i] = (float)-s;
}

template <int G> int launch_pick(tap_ctx *ctx, const PickArgs &a, bool greedy, hipStream_t st)
{
    constexpr int EPB = TAP_BLOCK / G;
    const int grid = (a.B + EPB - 1) / EPB;
    if (greedy) hipLaunchKernelGGL((k_policy_pick<G, true>), dim3(grid), dim3(TAP_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_policy_pick<G, false>), dim3(grid), dim3(TAP_BLOCK), 0, st, a);
    TAP_LAUNCH_CHECK(ctx, "k_policy_pick");
    tap_variant_hit(ctx, TAP_HIT_POLICY_PICK, 0, G, TapVariant{greedy ? 1 : 0, a.probs ? 1 : 0, 0}, 0);
    return TAP_OK;
}

int launch_pick_wide(tap_ctx *ctx, const PickArgs &a, bool greedy, hipStream_t st)
{
    const int wpb = TAP_BLOCK / 64, grid = a.B / wpb + (a.B % wpb ? 1 : 0);
    if (greedy) hipLaunchKernelGGL((k_policy_pick_wide<true>), dim3(grid), dim3(TAP_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_policy_pick_wide<false>), dim3(grid), dim3(TAP_BLOCK), 0, st, a);
    TAP_LAUNCH_CHECK(ctx, "k_policy_pick_wide");
    tap_variant_hit(ctx, TAP_HIT_POLICY_PICK, 0, 0, TapVariant{greedy ? 1 : 0, a.probs ? 1 : 0, 0}, 0);
    return TAP_OK;
}

template <int FORM> int launch_form(tap_ctx *ctx, const FormArgs &a, hipStream_t st)
{
    const int G = a.nR <= 8 ? 8 : a.nR <= 16 ? 16 : a.nR <= 32 ? 32 : a.nR <= 64 ? 64 : 0;
    const int rpb = TAP_BLOCK / (G ? G : 64), grid = a.B / rpb + (a.B % rpb ? 1 : 0);
    const dim3 g(grid), b(TAP_BLOCK);
    switch (G) {
    case 8: hipLaunchKernelGGL((k_policy_pick_form<8, FORM>), g, b, 0, st, a); break;
    case 16: hipLaunchKernelGGL((k_policy_pick_form<16, FORM>), g, b, 0, st, a); break;
    case 32: hipLaunchKernelGGL((k_policy_pick_form<32, FORM>), g, b, 0, st, a); break;
    case 64: hipLaunchKernelGGL((k_policy_pick_form<64, FORM>), g, b, 0, st, a); break;
    default: hipLaunchKernelGGL((k_policy_pick_wide_form<FORM>), g, b, 0, st, a); break;
    }
    TAP_LAUNCH_CHECK(ctx, G ? "k_policy_pick_form" : "k_policy_pick_wide_form");
    tap_variant_hit(ctx, TAP_HIT_POLICY_PICK, 0, G, TapVariant{FORM, a.probs ? 1 : 0, 0}, 0);
    return TAP_OK;
}

} // namespace

extern "C" int tap_policy_pick_draw(tap_ctx *ctx, const float *logits, const float *mask, const int64_t *state, uint32_t step,
                                    uint32_t env_offset, int B, int nR, int64_t *ptr_out, float *logp_out, float *probs_out,
                                    float *u_out, void *stream)
{
    if (B < 0 || nR < 1) return tap_fail(ctx, TAP_E_INVALID, "policy pick draw: B %d, nR %d", B, nR);
    if (B == 0) return TAP_OK;
    if (!logits || !mask || !ptr_out || !logp_out) return tap_fail(ctx, TAP_E_INVALID, "policy pick draw: null buffer");
    if (!state || ((uintptr_t)state & 7)) return tap_fail(ctx, TAP_E_INVALID, "policy pick draw: state must be an 8-byte aligned int64[2]");
    const FormArgs a = {logits, mask, (const long long *)state, nullptr, step, env_offset, B, nR, ptr_out, logp_out, probs_out, u_out};
    return launch_form<FORM_DRAW>(ctx, a, (hipStream_t)stream);
}

extern "C" int tap_policy_pick_given(tap_ctx *ctx, const float *logits, const float *mask, const int64_t *ptr_in, int B, int nR,
                                     float *logp_out, float *probs_out, void *stream)
{
    if (B < 0 || nR < 1) return tap_fail(ctx, TAP_E_INVALID, "policy pick given: B %d, nR %d", B, nR);
    if (B == 0) return TAP_OK;
    if (!logits || !mask || !logp_out) return tap_fail(ctx, TAP_E_INVALID, "policy pick given: null buffer");
    if (!ptr_in) return tap_fail(ctx, TAP_E_INVALID, "policy pick given: null ptr_in");
    const FormArgs a = {logits, mask, nullptr, ptr_in, 0, 0, B, nR, nullptr, logp_out, probs_out, nullptr};
    return launch_form<FORM_GIVEN>(ctx, a, (hipStream_t)stream);
}

extern "C" int tap_policy_pick(tap_ctx *ctx, const float *logits, const float *mask, const float *u, int B, int nR,
                               int flags, int64_t *ptr_out, float *logp_out, float *probs_out, void *stream)
{
    if (B < 0 || nR < 1) return tap_fail(ctx, TAP_E_INVALID, "policy pick: B %d, nR %d", B, nR);
    if (B == 0) return TAP_OK; // an empty batch has no buffers to check
    if (!logits || !mask || !ptr_out || !logp_out) return tap_fail(ctx, TAP_E_INVALID, "policy pick: null buffer");
    const bool greedy = (flags & TAP_P_GREEDY) != 0;
    if (greedy && u) return tap_fail(ctx, TAP_E_INVALID, "policy pick: TAP_P_GREEDY takes no uniforms");
    if (!greedy && !u) return tap_fail(ctx, TAP_E_INVALID, "policy pick: sampling needs the uniforms u (or TAP_P_GREEDY)");
    if (flags & ~TAP_P_GREEDY) return tap_fail(ctx, TAP_E_INVALID, "policy pick: bad flags %d", flags);
    const PickArgs a = {logits, mask, u, B, nR, ptr_out, logp_out, probs_out};
    hipStream_t st = (hipStream_t)stream;
    if (nR <= 8) return launch_pick<8>(ctx, a, greedy, st);
    if (nR <= 16) return launch_pick<16>(ctx, a, greedy, st);
    if (nR <= 32) return launch_pick<32>(ctx, a, greedy, st);
    if (nR <= 64) return launch_pick<64>(ctx, a, greedy, st);
    return launch_pick_wide(ctx, a, greedy, st);
}

extern "C" int tap_policy_pick_backward(tap_ctx *ctx, const float *probs, const int64_t *ptr, const float *logp,
                                        const float *g, int B, int nR, float *dlogits_out, void *stream)
{
    if (B < 0 || nR < 1) return tap_fail(ctx, TAP_E_INVALID, "policy pick backward: B %d, nR %d", B, nR);
    if (B == 0) return TAP_OK;
    if (!probs || !ptr || !logp || !g || !dlogits_out) return tap_fail(ctx, TAP_E_INVALID, "policy pick backward: null buffer");
    const size_t total = (size_t)B * (size_t)nR, blocks = (total + TAP_BLOCK - 1) / TAP_BLOCK;
    if (blocks > (size_t)INT_MAX) return tap_fail(ctx, TAP_E_UNSUPPORTED, "policy pick backward: %zu elements in one launch", total);
    hipLaunchKernelGGL(k_policy_pick_backward, dim3((unsigned)blocks), dim3(TAP_BLOCK), 0, (hipStream_t)stream, probs, ptr, logp,
                       g, total, nR, dlogits_out);
    TAP_LAUNCH_CHECK(ctx, "k_policy_pick_backward");
    tap_variant_hit(ctx, TAP_HIT_POLICY_PICK, 0, 0, TapVariant{0, 0, 1}, 0);
    return TAP_OK;
}
