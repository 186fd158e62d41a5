// transition_macs.hip -- the fused step of transition.hip (update_dynamic + update_mask + gather + add_new_block in one
// launch, pack.py:276-376, model.py:404-465) for the MACS / MUL placements: 2D up to 16 columns (tap_macs.h) and 3D
// (tap_macs3.h).  Same workgroup shape as k_transition: the envs' placement waves at raised priority beside 4 stream
// waves.  Its own translation unit so that it compiles beside transition.hip (the two were the build's long pole).
// gfx950 only.
#include <cstdlib>

#include "tap_common.h"
#include "tap_macs.h"
#include "tap_macs3.h"
#include "tap_masks.h"
#include "tap_place.h"
#include "tap_transition.h"
#include "tap_waves.h"

// ---- the same fusion for MACS / MUL 2D (tap_macs.h): G = 8/16 lanes per env ---------------------
// (Register cliff, measured in round 3: a workgroup is 5 waves and a CU gets 4 of them at B = 8192; at 71 VGPRs -- 7
//  waves per SIMD -- the step takes 17.8 us, at 85 -- 5 per SIMD, where the 20 waves only fit if the dispatcher spreads
//  them perfectly -- 23.6 us.  A window-maximum form of macs_adj (80 instead of 590 instructions, tie-break 5.1 k -> 2.6 k
//  cycles stand-alone) crossed that line and was dropped; amdgpu_waves_per_eu(7, 8) brings either form to 72 VGPRs but
//  costs 3 % by itself.)
constexpr int MACS_SW = 4;   // stream waves per workgroup of the MACS fused steps (8, measured in round 5: c4 503 -> 330 M
                             // env-steps/s, c6 140 -> 129 M -- the wave slots are worth more to the placement waves)
// WC: 0, or the container's width known at compile time (tap_macs_place; BASELINE configs[3]'s W = 7 with its n = 20 window)
template <int G, int NC, int MODE, int WC = 0>
__global__ void __launch_bounds__((TransGeom<G, MACS_SW>::THREADS)) k_transition_macs(TransArgs a)
{
    using Geo = TransGeom<G, MACS_SW>;
    constexpr int EPB = Geo::EPB, SPW = Geo::SPW, ENV_WAVES = Geo::ENV_WAVES;
    extern __shared__ float trans_lds[];
    // (the wave index stays a vector value here: in a scalar register -- transition.hip, where it is worth 4 % at c2 -- it
    //  measured flat on the MACS steps and 7 % SLOWER on the rolling step, round 6)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int env_base = blockIdx.x * EPB;
    const int B = a.s.d.B, W = WC ? WC : a.s.d.W, H = a.s.d.H;
    if (wave >= ENV_WAVES) {
        trans_stream_wave<SPW, NC, MODE>(a.m, env_base + (wave - ENV_WAVES) * SPW, lane,
                                     trans_lds + (size_t)(wave - ENV_WAVES) * SPW * 3 * a.m.nR);
        return;
    }
    __builtin_amdgcn_s_setprio(3);   // (2 -> 3: +2 % at c4; without a raised priority the step takes 23.5 instead of 18.0 us)
    int *macs_base = reinterpret_cast<int *>(trans_lds + (size_t)EPB * 3 * a.m.nR);
    const bool fresh = a.flags & TAP_T_FRESH;
    const int cell = tid % G, gl0 = lane - cell;
    const int env = env_base + tid / G;
    const bool ev = env < B, incell = cell < W;
    const MacsLds L = macs_lds(macs_base + (tid / G) * macs_group_words(G, H, a.s.d.n_max, W), G, H, macs_ems_cap(W, a.s.d.n_max));
    int hm = 0, cv = 0, bx = 1, bz = 1;
    if (ev) {
        if (!fresh) {
            if (incell) hm = a.s.v.hm[(size_t)env * W + cell];
            if (cell < 4) cv = a.s.v.cnt[(size_t)env * 4 + cell];
        }
        bool badp;
        const long praw = (long)a.s.ptr[env];
        const long p = tap_col(praw, a.s.nR, badp);
        const float vx = a.s.static_[((size_t)env * a.s.static_rows + 1) * a.s.nR + p];
        const float vz = a.s.static_[((size_t)env * a.s.static_rows + 2) * a.s.nR + p];
        bx = badp ? 0 : (int)vx;
        bz = badp ? 0 : (int)vz;
        if (cell == 0) { const float fv[2] = {badp ? 0.f : vx, badp ? 0.f : vz}; tap_step_aux(a.s, env, 2, fv, praw); }
    }
    Counters cnt = {__shfl(cv, gl0), __shfl(cv, gl0 + 1), __shfl(cv, gl0 + 2), __shfl(cv, gl0 + 3)};
    int err = 0;
    bool do_step = ev;
    if (ev && cnt.count >= a.s.d.n_max) { err |= 2; do_step = false; }
    if (ev && (bx < 1 || bz < 1)) { err |= 4; do_step = false; }
    L.hm[cell] = hm;
    for (int i = cell; i < H; i += G) L.taken[i] = 0;
    if (ev)
        for (int k = cell; k < cnt.count * 4 && k < a.s.d.n_max * 4; k += G) {
            const int i = k >> 2, f = k & 3;
            L.hist[k] = (f < 2 ? a.s.v.pos : a.s.v.blk)[(size_t)(i * 2 + (f & 1)) * B + env];
        }
    tap_wave_lds_sync();
    const int step = cnt.count;
    const PlaceCfg cfg = {W, 1, H, a.s.d.flags, nullptr};
    const Placement pl = tap_macs_place<G, WC>(cfg, L, cell, gl0, hm, cnt, err, bx, bz, do_step);
    err = group_or<G>(err);
    tap_wave_lds_sync();
    L.hm[cell] = hm;
    tap_wave_lds_sync();
    const int gmax = (a.flags & TAP_T_RATIO) ? group_max<G>(incell ? hm : 0) : 0;
    if (ev) {
        if (incell) a.s.v.hm[(size_t)env * W + cell] = hm;
        if (a.s.feature_out)
            tap_write_feature<2, G>(a.s.d.feature, W, 1, L.hm, cell, hm, a.s.feature_out + (size_t)env * a.s.flen);
        if (cell == 0) {
            if (do_step || fresh)
                reinterpret_cast<int4 *>(a.s.v.cnt)[env] = make_int4(cnt.valid, cnt.empty, cnt.nstable, cnt.count);
            if (do_step) {
                a.s.v.pos[(size_t)(step * 2) * B + env] = pl.x;
                a.s.v.pos[(size_t)(step * 2 + 1) * B + env] = pl.z;
                a.s.v.stable[(size_t)step * B + env] = (uint8_t)pl.stab;
                a.s.v.blk[(size_t)(step * 2) * B + env] = bx;
                a.s.v.blk[(size_t)(step * 2 + 1) * B + env] = bz;
            }
            if (fresh) a.s.v.err[env] = err;
            else if (err) a.s.v.err[env] |= err;
            if (a.flags & TAP_T_RATIO) {
                double C = 0.0, P = 0.0, S = 0.0;
                if (cnt.count != 0) {
                    C = (double)cnt.valid / (double)((long long)W * gmax);
                    P = (double)cnt.valid / (double)(cnt.empty + cnt.valid);
                    S = (double)cnt.nstable / (double)cnt.count;
                }
                a.ratio_out[env] = (float)tap_ratio_formula(a.s.d.ratio_mode, C, P, S);
            }
        }
    } else if (a.s.d.feature == TAP_FEAT_ZERO) {
        (void)group_min<G>(INT_MAX);
    }
}

// ---- and for MACS / MUL 3D (tap_macs3.h): G = 8..64 lanes per env --------------------------------
// WL: 0, or the side of a WL x WL container known at compile time (tap_macs3_place; instantiated for the reference's 5 x 5)
template <int G, int NC, int MODE, int WL = 0>
__global__ void __launch_bounds__((TransGeom<G, MACS_SW>::THREADS)) k_transition_macs3(TransArgs a)
{
    using Geo = TransGeom<G, MACS_SW>;
    constexpr int EPB = Geo::EPB, SPW = Geo::SPW, ENV_WAVES = Geo::ENV_WAVES;
    extern __shared__ float trans_lds[];
    // (the wave index stays a vector value here: in a scalar register -- transition.hip, where it is worth 4 % at c2 -- it
    //  measured flat on the MACS steps and 7 % SLOWER on the rolling step, round 6)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int env_base = blockIdx.x * EPB;
    if (wave >= ENV_WAVES) {
        trans_stream_wave<SPW, NC, MODE>(a.m, env_base + (wave - ENV_WAVES) * SPW, lane,
                                     trans_lds + (size_t)(wave - ENV_WAVES) * SPW * 3 * a.m.nR);
        return;
    }
    __builtin_amdgcn_s_setprio(2);
    int *macs_base = reinterpret_cast<int *>(trans_lds + (size_t)EPB * 3 * a.m.nR);
    const int grp = tid / G;
    tap_macs3_wave<G, WL>(a.s, a.flags, a.ratio_out, env_base + grp, tid % G, lane,
                          macs_base + grp * macs3_group_words(G, a.s.d.n_max, a.s.d.H));
}

template <int G> static int launch_transition_macs3(tap_ctx *ctx, const TransArgs &a, hipStream_t st)
{
    constexpr int EPB = TransGeom<G, MACS_SW>::EPB, THREADS = TransGeom<G, MACS_SW>::THREADS;
    const int grid = (a.s.d.B + EPB - 1) / EPB;
    if (grid == 0) return TAP_OK;
    const size_t lds = (size_t)EPB * 3 * a.m.nR * sizeof(float) +
                       (size_t)EPB * macs3_group_words(G, a.s.d.n_max, a.s.d.H) * sizeof(int);
    if (lds > tap_lds_limit(ctx)) return tap_fail(ctx, TAP_E_UNSUPPORTED, "transition(MACS 3D): %zu bytes of LDS needed", lds);
    const TapVariant v = tap_stream_variant(TAP_SV_MACS3, tap_mask_facts(a.m), TapLaunchFacts{3, G, EPB, a.s.d.B, a.s.d.W, a.s.d.L, false});
    return tap_launch_variant<TAP_SV_MACS3, 3, G>(ctx, "k_transition_macs3", v, a.m.wt, [&](auto k) -> int {
        using K = decltype(k);
        TAP_HIP_CHECK(ctx, tap_allow_lds(k_transition_macs3<G, K::nc, K::mode, K::extra>, lds));
        hipLaunchKernelGGL((k_transition_macs3<G, K::nc, K::mode, K::extra>), dim3(grid), dim3(THREADS), lds, st, a);
        return TAP_OK;
    });
}

int tap_macs_validate(tap_ctx *ctx, const tap_env_desc &d); // macs.hip

template <int G> static int launch_transition_macs(tap_ctx *ctx, const TransArgs &a, hipStream_t st)
{
    constexpr int EPB = TransGeom<G, MACS_SW>::EPB, THREADS = TransGeom<G, MACS_SW>::THREADS;
    const int grid = (a.s.d.B + EPB - 1) / EPB;
    if (grid == 0) return TAP_OK;
    const size_t lds = (size_t)EPB * 3 * a.m.nR * sizeof(float) +
                       (size_t)EPB * macs_group_words(G, a.s.d.H, a.s.d.n_max, a.s.d.W) * sizeof(int);
    if (lds > tap_lds_limit(ctx)) return tap_fail(ctx, TAP_E_UNSUPPORTED, "transition(MACS): %zu bytes of LDS needed", lds);
    const TapVariant v = tap_stream_variant(TAP_SV_MACS, tap_mask_facts(a.m), TapLaunchFacts{2, G, EPB, a.s.d.B, a.s.d.W, a.s.d.L, false});
    return tap_launch_variant<TAP_SV_MACS, 2, G>(ctx, "k_transition_macs", v, a.m.wt, [&](auto k) -> int {
        using K = decltype(k);
        TAP_HIP_CHECK(ctx, tap_allow_lds(k_transition_macs<G, K::nc, K::mode, K::extra>, lds));
        hipLaunchKernelGGL((k_transition_macs<G, K::nc, K::mode, K::extra>), dim3(grid), dim3(THREADS), lds, st, a);
        return TAP_OK;
    });
}


int tap_transition_macs_launch(tap_ctx *ctx, const tap_env_desc *d, const TransArgs &a0, hipStream_t st)
{
    // these launches last 17 us and more, so the fp32 expansion's stores stay write-through up to a higher limit than
    // the LB_GREEDY step's (tap_masks.h: store_stream; c4's 78.6 MB per launch: 480 against 441 M env-steps/s)
    TransArgs a = a0;
    a.m.wt = tap_write_through((size_t)a.m.B * a.m.rows * a.m.nR * sizeof(float), (size_t)128 << 20);
    const int Gs = tap_group_size(d);
    if (d->D == 3) {
        switch (Gs) {
        case 8: return launch_transition_macs3<8>(ctx, a, st);
        case 16: return launch_transition_macs3<16>(ctx, a, st);
        case 32: return launch_transition_macs3<32>(ctx, a, st);
        default: return launch_transition_macs3<64>(ctx, a, st);
        }
    }
    // (16 lanes per container for W <= 8 measured 2.3 x slower at c4: the per-lane work grows with G)
    return d->W <= 8 ? launch_transition_macs<8>(ctx, a, st) : launch_transition_macs<16>(ctx, a, st);
}
