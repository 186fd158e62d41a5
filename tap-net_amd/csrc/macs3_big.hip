// macs3_big.hip -- MACS / MUL 3D (tools.calc_one_position_mcs_3d, tools.py:2751-3165) for containers beyond the
// lane-per-cell kernel of tap_macs3.h: more than 64 cells or a side above 8 (e.g. --container_width 10 -> 10 x 10 x H,
// model.py:279).  ONE WAVEFRONT per container (tap_macs3_wave.h: the serial algorithm of tap_macs3_big.h run wave-uniformly on
// the container's LDS tile, its long loops shared by the lanes), on the same reduced state as the lane kernel (height-map,
// placement history, the free-list bit-grid in `occ`); one THREAD per container with the lists in the blob's scratch
// section when the tile does not fit the LDS.  Block fetch, admission, commit and feature of the step kernels are
// tap_step_seam.h's.  gfx950 only.
#include "tap_common.h"
#include "tap_place.h"
#include "tap_macs3_big.h"
#include "tap_macs3_wave.h"
#include "tap_masks.h"
#include "tap_transition.h"
#include "tap_episode.h"
#include "tap_step_seam.h"

static_assert(M3B_F_HARD == TAP_F_HARD && M3B_F_USE_P == TAP_F_USE_P && M3B_F_USE_S == TAP_F_USE_S &&
              M3B_F_ZERO == TAP_F_MCS_ZERO && M3B_F_TIE == TAP_F_MCS_TIE, "flag bits are passed through");

// EMS entries one step can hold (error bit 16 beyond): the level lists contribute up to two per changed (level, row,
// run), each placed block at most four beside it and its footprint's cells on top
__host__ __device__ inline int macs3_big_cap(int n_max) { return 128 + 8 * n_max; }

// scratch ints per container: ems[cap] (2 ints each) | lev[cells] | slots[cells] | lvh[n_max + 2] | lvr[n_max + 2]
// MACS 3D's own limit on a block (the step seam's `family_rejects`).  Sides larger than the container are rejected as
// invalid input, as in tap_macs3.h (the reference keeps such a block in its history at (0,0,0) and its later slices run
// out of range, tools.py:2858, 2914); footprints above 16 x 16 are beyond the stability test (tap_stable_wide.h)
__device__ __forceinline__ bool macs3_rejects(int W, int L, int bx, int by)
{
    return bx > W || by > L || bx > TAP_WIDE_MAX_SIDE || by > TAP_WIDE_MAX_SIDE;
}

size_t tap_macs3_big_scratch_ints(const tap_env_desc *d)
{
    return (size_t)2 * macs3_big_cap(d->n_max) + (size_t)2 * d->W * d->L + (size_t)2 * (d->n_max + 2);
}

__global__ void __launch_bounds__(TAP_BLOCK) k_macs3d_big_step(StepArgs a, int32_t *scratch, size_t scratch_ints, int lpw)
{
    const int env = tap_spread_env(lpw, a.d.B);                                  // containers spread over the waves (tap_common.h)
    const int B = a.d.B, W = a.d.W, L = a.d.L, H = a.d.H, cells = W * L;
    if (env < 0) return;
    const SeamBlock b = tap_seam_fetch(a, env);
    const int bx = b.bx, by = b.by, bz = b.bz;
    bool act;
    Counters c = tap_seam_load(a, env, false, act);
    int err = 0;
    const bool do_step = tap_seam_admit(act, c.count, a.d.n_max, bx, by, bz, macs3_rejects(W, L, bx, by), err);
    const int step = c.count;
    Placement pl = {0, 0, 0, 0, 0};
    if (do_step) {
        const int cap = macs3_big_cap(a.d.n_max);
        int32_t *sc = scratch + (size_t)env * scratch_ints;
        M3BState s;
        s.W = W; s.L = L; s.H = H; s.HW = (H + 63) / 64; s.flags = a.d.flags; s.cap = cap; s.step = step;
        s.hm = a.v.hm + (size_t)env * cells;
        s.occ = a.v.occ + (size_t)env * cells * s.HW;
        s.pos = a.v.pos + env; s.blk = a.v.blk + env; s.hs = (size_t)B;
        s.ems = reinterpret_cast<M3BEms *>(sc);
        s.lev = sc + 2 * cap;
        s.slots = s.lev + cells;
        s.lvh = s.slots + cells;
        s.lvr = s.lvh + a.d.n_max + 2;
        const uint32_t *lut = a.lut;
        int cnt[4] = {c.valid, c.empty, c.nstable, c.count};                     // (tap_macs3_big.h also compiles for the host)
        const M3BResult r = m3b_place(s, cnt, err, bx, by, bz,
                                      [lut](int fx, int fy, m3b_u64 eq) -> int { return tap_stable3d_any(lut, fx, fy, eq); });
        c = Counters{cnt[0], cnt[1], cnt[2], cnt[3] + 1};                        // tools.py:3713
        pl = Placement{r.placed, r.x, r.y, r.z, r.stab};
    }
    const SeamHist hist = {bx | (pl.placed << 16), by, bz};                      // failures too (tools.py:2843-2846)
    tap_seam_commit(a, env, do_step, false, c, step, pl, err, &hist);
}

// ---- one WAVEFRONT per container (tap_macs3_wave.h): the container's working set in the wave's LDS tile ---------------
// the tile at `base` (m3w_tile_u64 units): occ | rows | ems | hm | lev | slots | pxy | bs | be | history pos[3 n_max] | blk[3 n_max]
__device__ __forceinline__ M3WTile macs3d_wave_tile(m3b_u64 *base, int W, int L, int H, int flags, int n_max, int32_t *&hpos, int32_t *&hblk)
{
    const int cells = W * L, HW = (H + 63) / 64, cap = macs3_big_cap(n_max);
    M3WTile s;
    s.W = W; s.L = L; s.H = H; s.HW = HW; s.flags = flags; s.cap = cap; s.n_max = n_max; s.step = 0;
    s.occ = base;
    s.rows = s.occ + (size_t)cells * HW;
    s.ems = reinterpret_cast<M3BEms *>(s.rows + 64);
    s.hm = reinterpret_cast<int32_t *>(s.ems + cap);
    s.lev = s.hm + cells; s.slots = s.lev + cells; s.pxy = s.slots + cells; s.bs = s.pxy + cells; s.be = s.bs + 64;
    hpos = s.be + 64; hblk = hpos + 3 * n_max;                                   // the history so far, staged in the tile
    s.pos = hpos; s.blk = hblk; s.hs = 1;
    return s;
}

// one MACS 3D step of container `env` by one wavefront (every lane calls; env < B); base = the wave's LDS tile: load
// tile, fetch, admit, place on the tile (m3w_place), commit, feature; aux: the fused step, which also writes the gather's
// by-products
__device__ __forceinline__ void macs3d_wave_body(const StepArgs &a, int env, int lane, m3b_u64 *base, bool aux)
{
    const int B = a.d.B, W = a.d.W, L = a.d.L, H = a.d.H, cells = W * L, HW = (H + 63) / 64;
    int32_t *hpos, *hblk;                                                        // one round trip for all of the history
    M3WTile s = macs3d_wave_tile(base, W, L, H, a.d.flags, a.d.n_max, hpos, hblk);
    int32_t *ghm = a.v.hm + (size_t)env * cells;
    m3b_u64 *gocc = a.v.occ + (size_t)env * cells * HW;
    bool act;
    Counters c = tap_seam_load(a, env, false, act);
    for (int k = lane; k < cells; k += 64) s.hm[k] = ghm[k];
    for (int k = lane; k < 3 * min(c.count, a.d.n_max); k += 64) { hpos[k] = a.v.pos[(size_t)k * B + env]; hblk[k] = a.v.blk[(size_t)k * B + env]; }
    for (int k = lane; k < cells * HW; k += 64) s.occ[k] = gocc[k];
    const SeamBlock b = tap_seam_fetch(a, env);
    if (aux && lane == 0) tap_seam_aux(a, env, b);
    const int bx = b.bx, by = b.by, bz = b.bz;
    int err = 0;
    const bool do_step = tap_seam_admit(act, c.count, a.d.n_max, bx, by, bz, macs3_rejects(W, L, bx, by), err);
    const int step = c.count;
    Placement pl = {0, 0, 0, 0, 0};
    tap_wave_lds_sync();
    if (do_step) {                                                               // wave-uniform
        s.step = step;
        int cnt[4] = {c.valid, c.empty, c.nstable, c.count};                     // (tap_macs3_big.h also compiles for the host)
        const M3BResult r = m3w_place(s, cnt, err, bx, by, bz, a.lut, lane);
        c = Counters{cnt[0], cnt[1], cnt[2], cnt[3] + 1};                        // tools.py:3713
        pl = Placement{r.placed, r.x, r.y, r.z, r.stab};
        tap_wave_lds_sync();
        for (int k = lane; k < cells; k += 64) ghm[k] = s.hm[k];
        for (int k = lane; k < cells * HW; k += 64) gocc[k] = s.occ[k];
    }
    if (lane == 0) {
        const SeamHist hist = {bx | (pl.placed << 16), by, bz};                  // failures too (tools.py:2843-2846)
        tap_seam_commit(a, env, do_step, false, c, step, pl, err, &hist);
    }
    if (a.feature_out) {                                                         // of the new map, from the tile
        tap_wave_lds_sync();
        tap_seam_feature(a.d.feature, 3, W, L, s.hm, a.feature_out + (size_t)env * a.flen, lane, 64, [](int v) { return group_min<64>(v); });
    }
}

// ---- whole episodes: tools.calc_positions_mcs (tools.py:3213-3315) beyond the lane-per-cell kernel ------------------
// One wavefront per container as in the step kernel, its tile -- height-map, history, free-list bit-grid, lists --
// living in LDS across the n placements: nothing but the block list and the per-episode results touches memory, and no
// state blob exists.  A tour entry's block is fetched by lane t % 64 for 64 steps at a time, as in k_big_wave_episode
// (big.hip).  cnt[3] counts every entry of the container's list (S's denominator), and the history keeps failed entries
// too (tools.py:2843-2846), as in k_episode_macs3 (episode.hip).
__device__ __forceinline__ void macs3d_wave_episode_body(const EpisodeArgs &a, int tile_u64)
{
    extern __shared__ unsigned long long m3w_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;   // (a vector value, as in this file's other kernels: TAP_WAVE_INDEX() measured slower / flat in them, tap_common.h)
    const int env = (int)(blockIdx.x * (blockDim.x >> 6)) + wave;
    if (env >= a.B) return;                                                       // wave-uniform
    const int W = a.d.W, L = a.d.L, cells = W * L, HW = (a.d.H + 63) / 64, n = a.n;
    int32_t *hpos, *hblk;
    M3WTile s = macs3d_wave_tile(m3w_lds + (size_t)wave * tile_u64, W, L, a.d.H, a.d.flags, n, hpos, hblk);
    for (int c = lane; c < cells; c += 64) s.hm[c] = 0;
    for (int k = lane; k < cells * HW; k += 64) s.occ[k] = 0ull;                  // level_free_space of an empty container
    tap_wave_lds_sync();
    int cnt[4] = {0, 0, 0, 0};
    int err = 0;
    for (int t0 = 0; t0 < n; t0 += 64) {
        int mine[3] = {1, 1, 1}, merr = 0;
        bool min_ = false;
        if (t0 + lane < n) min_ = episode_block<3>(a, env, t0 + lane, true, mine, merr);
        err |= merr;                                                              // OR-ed over the wave below
        for (int j = 0; j < 64 && t0 + j < n; ++j) {
            const int t = t0 + j;
            const int bx = __shfl(mine[0], j), by = __shfl(mine[1], j), bz = __shfl(mine[2], j);
            const bool in = __shfl((int)min_, j) != 0;
            // (not tap_seam_admit: with it the loop around the placement was allocated 163 instead of 169 VGPRs and the 10 x 10
            // episodes measured 1 % (loose) and 3 % (tight build) slower; the tile holds n entries: never full)
            bool do_step = in;
            if (in && (bx < 1 || by < 1 || bz < 1 || bx > W || by > L || bx > TAP_WIDE_MAX_SIDE || by > TAP_WIDE_MAX_SIDE)) { err |= 4; do_step = false; }   // = macs3_rejects
            M3BResult r = {0, 0, 0, 0, 0};
            if (do_step) {                                                        // wave-uniform
                const int step = cnt[3];
                s.step = step;
                r = m3w_place(s, cnt, err, bx, by, bz, a.lut, lane);
                cnt[3] += 1;                                                      // tools.py:3713
                if (lane == 0) {                                                  // tools.py:2843-2846: failures too
                    hpos[step * 3] = r.x; hpos[step * 3 + 1] = r.y; hpos[step * 3 + 2] = r.z;
                    hblk[step * 3] = bx | (r.placed << 16); hblk[step * 3 + 1] = by; hblk[step * 3 + 2] = bz;
                }
                tap_wave_lds_sync();
            }
            if (lane == 0) {
                if (a.pos_out) {
                    int32_t *pp = a.pos_out + ((size_t)env * n + t) * 3;
                    pp[0] = r.x; pp[1] = r.y; pp[2] = r.z;
                }
                if (a.stable_out) a.stable_out[(size_t)env * n + t] = (uint8_t)r.stab;
            }
        }
    }
    int gmax = 0;
    for (int c = lane; c < cells; c += 64) gmax = max(gmax, s.hm[c]);
    gmax = group_max<64>(gmax);
    err = group_or<64>(err);
    const Counters cn = {cnt[0], cnt[1], cnt[2], cnt[3]};
    if (lane == 0) episode_finish(a, env, cn, gmax, err);
}

// Two builds of the same body.  Left alone the compiler takes 169 VGPRs for the loop around the placement (the step
// kernel: 127), which is the faster code but lets a SIMD hold two waves; held to four waves per SIMD it takes 128 and
// spills 14.  Measured (profiles/macs_wave_episode.json, ms per episode, loose / tight): 10 x 10, n = 10, B = 128
// 0.84 / 0.90, B = 4 096 1.79 / 1.20 (stepped: 1.59); 20 x 20, n = 30, B = 128 11.6 / 13.2, B = 4 096 23.6 / 26.6.
// The launcher takes the tight one only when more than two waves per SIMD would be resident (macs3d_episode_tight).
__global__ void __launch_bounds__(TAP_BLOCK) k_macs3d_wave_episode(EpisodeArgs a, int tile_u64) { macs3d_wave_episode_body(a, tile_u64); }
__global__ void __launch_bounds__(TAP_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 8))) k_macs3d_wave_episode_tight(EpisodeArgs a, int tile_u64)
{
    macs3d_wave_episode_body(a, tile_u64);
}

// Would a CU hold more waves than the loose build lets it?  What a CU would hold: the smaller of what the LDS admits
// (whole workgroups of `waves` tiles) and what the batch puts there.  What the loose build lets it hold: 4 SIMDs x
// (512 VGPRs / its own register count, in granules of 8), read from the code object once -- 8 waves at today's 169
// VGPRs -- so the rule follows the compiler.  Without a CU count (the query failed at create) the batch bound is
// unknown and the tight build, which is never slower than stepping, is taken whenever the LDS admits more.
static bool macs3d_episode_tight(const tap_ctx *ctx, int B, int waves, size_t tile)
{
    static const int loose_waves = [] {
        hipFuncAttributes fa;
        if (hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_macs3d_wave_episode)) != hipSuccess || fa.numRegs < 1) return 8;
        const int per_simd = 512 / ((fa.numRegs + 7) / 8 * 8);
        return 4 * (per_simd < 1 ? 1 : per_simd > 8 ? 8 : per_simd);
    }();
    const long by_lds = (long)(tap_lds_limit(ctx) / ((size_t)waves * tile)) * waves;
    const long by_batch = (ctx && ctx->cus > 0) ? ((long)B + ctx->cus - 1) / ctx->cus : by_lds;
    return (by_lds < by_batch ? by_lds : by_batch) > loose_waves;
}

// -> TAP_OK when launched; TAP_E_UNSUPPORTED when a container's tile does not fit the LDS or the wave kernels are
// switched off (the thread-per-container kernel steps those shapes)
int tap_macs3_wave_episode(tap_ctx *ctx, const EpisodeArgs &a, hipStream_t st)
{
    if (a.B == 0) return TAP_OK;
    if (a.n > TAP_WAVE_EPISODE_MAX_N) return tap_fail(ctx, TAP_E_UNSUPPORTED, "whole MACS / MUL episodes of more than %d blocks: step them with tap_env_step_gather", TAP_WAVE_EPISODE_MAX_N);
    const size_t tile_u64 = m3w_tile_u64(a.d.W * a.d.L, (a.d.H + 63) / 64, a.n, macs3_big_cap(a.n)), tile = tile_u64 * 8;
    const int waves = tap_wave_kernels_off() ? 0 : tap_waves_per_wg(ctx, tile);
    if (waves == 0)
        return tap_fail(ctx, TAP_E_UNSUPPORTED, "whole MACS / MUL episodes of %d x %d x %d containers, %d blocks: %s, step them with tap_env_step_gather",
                        a.d.W, a.d.L, a.d.H, a.n, tap_wave_kernels_off() ? "the wave kernels are switched off" : "the container's tile does not fit a workgroup's LDS");
    const bool tight = macs3d_episode_tight(ctx, a.B, waves, tile);
    auto *kernel = tight ? k_macs3d_wave_episode_tight : k_macs3d_wave_episode;
    TAP_HIP_CHECK(ctx, tap_allow_lds(kernel, (size_t)waves * tile));
    hipLaunchKernelGGL(kernel, dim3((a.B + waves - 1) / waves), dim3(waves * 64), (size_t)waves * tile, st, a, (int)tile_u64);
    TAP_LAUNCH_CHECK(ctx, "k_macs3d_wave_episode");
    tap_variant_hit(ctx, TAP_HIT_EPISODE_MACS3_WAVE, 3, 64, TapVariant{0, tight ? 1 : 0, waves}, 0);   // mode 1: the register-tight build
    return TAP_OK;
}

__global__ void __launch_bounds__(TAP_BLOCK) k_macs3d_wave_step(StepArgs a)
{
    extern __shared__ unsigned long long m3w_lds[];
    const int lane = threadIdx.x & 63, wave_in_wg = threadIdx.x >> 6;
    const int env = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (env >= a.d.B) return;                                                     // wave-uniform
    const int cells = a.d.W * a.d.L, HW = (a.d.H + 63) / 64;
    macs3d_wave_body(a, env, lane, m3w_lds + (size_t)wave_in_wg * m3w_tile_u64(cells, HW, a.d.n_max, macs3_big_cap(a.d.n_max)), false);
}

// The decoding step in ONE launch (round 5): a container's wavefront runs update_dynamic + update_mask of its own
// precedence slab on the bit shadow (tap_transition.h), then its placement.
template <int NC, int MODE>
__global__ void __launch_bounds__(TAP_BLOCK) k_macs3d_wave_transition(TransArgs a, int PW, int tile_u64)
{
    extern __shared__ unsigned long long m3w_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;   // (a vector value: TAP_WAVE_INDEX() measured slower / flat here, tap_common.h)
    const int env = blockIdx.x * PW + wave;
    if (env >= a.s.d.B) return;                                                   // wave-uniform
    // The wave first runs its container's precedence update (one slab: inputs in one round trip, write-through stores
    // that drain while the placement runs), then the placement.  Stream waves of their own, as in k_transition, would
    // occupy wave slots at this kernel's register count: with 4 + 2 waves per workgroup a CU held 8 placement waves
    // instead of 16 and the step took 218 against 148 us (MACS 3D 10 x 10, B = 4 096, round 5).
    trans_stream_wave<1, NC, MODE>(a.m, env, lane, reinterpret_cast<float *>(m3w_lds + (size_t)PW * tile_u64) + (size_t)wave * 3 * a.m.nR);
    macs3d_wave_body(a.s, env, lane, m3w_lds + (size_t)wave * tile_u64, true);
}

static int macs3d_transition_pw(const tap_ctx *ctx, const tap_env_desc *d, int nR)
{
    if (tap_wave_kernels_off()) return 0;
    const size_t tile = m3w_tile_u64(d->W * d->L, (d->H + 63) / 64, d->n_max, macs3_big_cap(d->n_max)) * 8;
    for (int pw = 4; pw >= 1; pw >>= 1)
        if ((size_t)pw * tile + (size_t)pw * 3 * nR * sizeof(float) <= tap_lds_limit(ctx)) return pw;
    return 0;
}

bool tap_macs3_wave_transition_ok(const tap_ctx *ctx, const tap_env_desc *d, int nR) { return macs3d_transition_pw(ctx, d, nR) > 0; }

int tap_macs3_wave_transition(tap_ctx *ctx, const tap_env_desc *d, const TransArgs &a, hipStream_t st)
{
    const int pw = macs3d_transition_pw(ctx, d, a.m.nR);
    if (pw == 0) return tap_fail(ctx, TAP_E_UNSUPPORTED, "no fused step for this container");
    if (!a.s.v.scratch || !a.s.v.occ) return tap_fail(ctx, TAP_E_INVALID, "MACS 3D above 64 cells: the state blob has no scratch section");
    const int tile_u64 = (int)m3w_tile_u64(d->W * d->L, (d->H + 63) / 64, d->n_max, macs3_big_cap(d->n_max));
    const size_t lds = (size_t)pw * tile_u64 * 8 + (size_t)pw * 3 * a.m.nR * sizeof(float);
    const dim3 g((d->B + pw - 1) / pw), blk(64 * pw);
    if (g.x == 0) return TAP_OK;
    const TapVariant v = tap_stream_variant(TAP_SV_MACS3_WAVE, tap_mask_facts(a.m), TapLaunchFacts{3, 64, pw, d->B, d->W, d->L, false});
    return tap_launch_variant<TAP_SV_MACS3_WAVE>(ctx, "k_macs3d_wave_transition", v, a.m.wt, [&](auto k) -> int {
        using K = decltype(k);
        TAP_HIP_CHECK(ctx, tap_allow_lds(k_macs3d_wave_transition<K::nc, K::mode>, lds));
        hipLaunchKernelGGL((k_macs3d_wave_transition<K::nc, K::mode>), g, blk, lds, st, a, pw, tile_u64);
        return TAP_OK;
    });
}

int tap_macs3_big_step(tap_ctx *ctx, const StepArgs &a, hipStream_t st)
{
    if (a.d.B == 0) return TAP_OK;
    if (!a.v.scratch || !a.v.occ) return tap_fail(ctx, TAP_E_INVALID, "MACS 3D above 64 cells: the state blob has no scratch section");
    {   // one wavefront per container when its working set fits a wave's share of the LDS
        const int cells = a.d.W * a.d.L, HW = (a.d.H + 63) / 64;
        const size_t tile = m3w_tile_u64(cells, HW, a.d.n_max, macs3_big_cap(a.d.n_max)) * 8;
        const int waves = tap_wave_kernels_off() ? 0 : tap_waves_per_wg(ctx, tile);
        if (waves > 0) {
            TAP_HIP_CHECK(ctx, tap_allow_lds(k_macs3d_wave_step, (size_t)waves * tile));
            hipLaunchKernelGGL(k_macs3d_wave_step, dim3((a.d.B + waves - 1) / waves), dim3(waves * 64), (size_t)waves * tile, st, a);
            TAP_LAUNCH_CHECK(ctx, "k_macs3d_wave_step");                            // (writes the feature itself)
            return TAP_OK;
        }
    }
    const int lpw = tap_spread_lpw(a.d.B);                                     // containers per wavefront (tap_common.h)
    hipLaunchKernelGGL(k_macs3d_big_step, dim3(tap_spread_grid(a.d.B, lpw, TAP_BLOCK)), dim3(TAP_BLOCK), 0, st, a, a.v.scratch,
                       tap_macs3_big_scratch_ints(&a.d), lpw);
    TAP_LAUNCH_CHECK(ctx, "k_macs3d_big_step");
    if (a.feature_out) return tap_big_feature(ctx, &a.d, a.v, a.feature_out, a.flen, st);   // tools.py:3716-3744
    return TAP_OK;
}

#ifdef M3W_PROF
extern "C" int tap_m3w_prof_read(unsigned long long *out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(m3w_prof), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(m3w_prof), z, sizeof z) != hipSuccess) return -1; }
    return 0;
}
#endif
