// tap_step_seam.h -- the bookkeeping around one placement, for the kernels in which ONE execution unit owns ONE
// container and `env` is uniform across the unit: a thread (k_big_step, k_macs2d_big_step, k_macs3d_big_step, k_lb_step),
// a wavefront (k_big_wave_step, k_macs2d_wave_step, k_macs3d_wave_step and their fused transitions) or a workgroup
// (k_big_wg_step, which is not moved onto it yet: big.hip says why).  A step body reads: load tile, fetch, load state,
// admit, place, commit, feature -- only the tile and the placement are the family's own.  The lane-group kernels (several containers per wavefront, clamped addresses, a load
// order tuned by measurement: tap_waves.h, tap_macs3.h, tap_macs_wide.h, macs.hip, transition_macs.hip, place_at.hip) are
// NOT on this seam.  The first part compiles for the host too (tests/host/step_seam_host.cpp).
#pragma once

#include <climits>
#include <cstdint>

#include "tapenv.h"

#if defined(__HIPCC__)
#define TAP_SEAM_HD __host__ __device__
#else
#define TAP_SEAM_HD
#endif

// May this container take the step?  Error bit 2: the container is full (tools.py:3677 IndexError); bit 4: a side is not
// positive, or the block breaks the family's own limit (`family_rejects`, one line in the family's file).  An idle
// container (act == false) is neither stepped nor flagged.
TAP_SEAM_HD inline bool tap_seam_admit(bool act, int count, int n_max, int bx, int by, int bz, bool family_rejects, int &err)
{
    if (!act) return false;
    const bool full = count >= n_max, bad = bx < 1 || by < 1 || bz < 1 || family_rejects;
    if (full) err |= 2;
    if (bad) err |= 4;
    return !full && !bad;
}

// get_heightmap's feature of one container (tools.py:3716-3744): `diff` (2D: hm[c + 1] - hm[c], W - 1 values; 3D: the x
// and y differences, 2 W L values), `zero` (minus the minimum) or `full`.  The unit's members take the cells first,
// first + stride, ...; min_reduce(v) returns the minimum of v over the unit and is called by every member (the identity
// for a single thread).  The 3D cell coordinates advance with the stride: no division per cell.
template <class MinReduce>
TAP_SEAM_HD inline void tap_seam_feature(int feature, int D, int W, int L, const int32_t *hm, float *out, int first, int stride,
                                         MinReduce min_reduce)
{
    const int cells = W * L;
    if (feature == TAP_FEAT_DIFF) {
        if (D == 2) {
            for (int c = first; c + 1 < W; c += stride) out[c] = (float)(hm[c + 1] - hm[c]);
            return;
        }
        int x = first / L, y = first - x * L;
        const int dx = stride / L, dy = stride - dx * L;
        for (int c = first; c < cells; c += stride) {
            out[c] = (float)(x > 0 ? hm[c] - hm[c - L] : 0);
            out[cells + c] = (float)(y > 0 ? hm[c] - hm[c - 1] : 0);
            x += dx; y += dy;
            if (y >= L) { y -= L; ++x; }
        }
        return;
    }
    int mn = 0;
    if (feature == TAP_FEAT_ZERO) {
        mn = INT_MAX;
        for (int c = first; c < cells; c += stride) mn = hm[c] < mn ? hm[c] : mn;
        mn = min_reduce(mn);
    }
    for (int c = first; c < cells; c += stride) out[c] = (float)(hm[c] - mn);
}

#if defined(__HIPCC__)
#include "tap_common.h"
#include "tap_place.h"

// Workgroups of how many wavefronts, each with a tile of tile_bytes in LDS: as many as the LDS holds tiles for, up to
// TAP_BLOCK / 64; 0 = one tile does not fit
inline int tap_waves_per_wg(const tap_ctx *ctx, size_t tile_bytes)
{
    int waves = TAP_BLOCK / 64;
    while (waves > 1 && (size_t)waves * tile_bytes > tap_lds_limit(ctx)) waves >>= 1;
    return (size_t)waves * tile_bytes <= tap_lds_limit(ctx) ? waves : 0;
}

// The step's block: its integer sides (by = 1 in 2D), and from a gather (model.py:404-412) the floats `static` holds, the
// raw column index and whether it lay outside [0, nR) -- then every side is 0 and admission raises bit 4.  f32 sides are
// truncated like the reference's int().
struct SeamBlock {
    int bx, by, bz;
    float fv[3];
    long ptr;
    bool badp;
};
__device__ __forceinline__ SeamBlock tap_seam_fetch(const StepArgs &a, int env)
{
    const int D = a.d.D;
    SeamBlock b = {0, 1, 0, {0.f, 0.f, 0.f}, 0, false};
    int s0, s1, s2 = 0;
    if (a.static_) {
        b.ptr = (long)a.ptr[env];
        const float *s = a.static_ + ((size_t)env * a.static_rows + 1) * a.nR + tap_col(b.ptr, a.nR, b.badp);
        b.fv[0] = b.badp ? 0.f : s[0];
        b.fv[1] = b.badp ? 0.f : s[a.nR];
        if (D == 3) b.fv[2] = b.badp ? 0.f : s[2 * (size_t)a.nR];
        s0 = (int)b.fv[0]; s1 = (int)b.fv[1]; s2 = (int)b.fv[2];
    } else if (a.blocks_dtype == TAP_DT_F32) {
        const float *s = (const float *)a.blocks + (size_t)env * D;
        s0 = (int)s[0]; s1 = (int)s[1];
        if (D == 3) s2 = (int)s[2];
    } else {
        const int32_t *s = (const int32_t *)a.blocks + (size_t)env * D;
        s0 = s[0]; s1 = s[1];
        if (D == 3) s2 = s[2];
    }
    b.bx = s0; b.by = D == 3 ? s1 : 1; b.bz = D == 3 ? s2 : s1;
    return b;
}

// the gather's by-products (tap_step_aux), by the unit's writer thread
__device__ __forceinline__ void tap_seam_aux(const StepArgs &a, int env, const SeamBlock &b)
{
    const float v[3] = {b.fv[0], b.fv[1], b.fv[2]};                              // (a plain array: tap_step_aux indexes it by a loop)
    if (a.static_) tap_step_aux(a, env, a.d.D, v, b.ptr);
}

// the container's counters and whether it steps at all; fresh (TAP_T_FRESH): the step starts from an empty container
__device__ __forceinline__ Counters tap_seam_load(const StepArgs &a, int env, bool fresh, bool &act)
{
    act = !a.active || a.active[env] != 0;
    const int4 cv = reinterpret_cast<const int4 *>(a.v.cnt)[env];
    return fresh ? Counters{0, 0, 0, 0} : Counters{cv.x, cv.y, cv.z, cv.w};
}

// What a step leaves in the state blob, by the unit's writer thread (lane 0, thread 0, the sole thread).  A step that was
// taken files its result at row `step` -- position and stable flag (zeros when nothing fitted), and in `blk` the history
// row the later MACS / legacy LB steps read, failures too (tools.py:2531-2533, 2843-2846); hist == nullptr: the family
// keeps none -- and the counters `cnt` the placement left (count already advanced).  Error bits are sticky, except that a
// fresh step overwrites whatever the blob held.
struct SeamHist {
    int x, y, z;
};
__device__ __forceinline__ void tap_seam_commit(const StepArgs &a, int env, bool do_step, bool fresh, const Counters &cnt, int step,
                                                const Placement &pl, int err, const SeamHist *hist)
{
    const int D = a.d.D;
    const size_t B = (size_t)a.d.B;
    if (do_step) {
        int32_t *q = a.v.pos + (size_t)step * D * B + env;
        q[0] = pl.x;
        if (D == 3) { q[B] = pl.y; q[2 * B] = pl.z; } else q[B] = pl.z;
        a.v.stable[(size_t)step * B + env] = (uint8_t)pl.stab;
        if (hist) {
            int32_t *h = a.v.blk + (size_t)step * D * B + env;
            h[0] = hist->x;
            if (D == 3) { h[B] = hist->y; h[2 * B] = hist->z; } else h[B] = hist->z;
        }
    }
    if (do_step || fresh) reinterpret_cast<int4 *>(a.v.cnt)[env] = make_int4(cnt.valid, cnt.empty, cnt.nstable, cnt.count);
    if (fresh) a.v.err[env] = err;
    else if (err) a.v.err[env] |= err;
}

// Container.calc_ratio (tools.py:3887-3966) of the state just committed; gmax = the highest column
__device__ __forceinline__ float tap_seam_ratio(const tap_env_desc &d, const Counters &cnt, int gmax)
{
    double C = 0.0, P = 0.0, S = 0.0;
    if (cnt.count != 0) {
        C = (double)cnt.valid / (double)((long long)d.W * d.L * gmax);
        P = (double)cnt.valid / (double)(cnt.empty + cnt.valid);
        S = (double)cnt.nstable / (double)cnt.count;
    }
    return (float)tap_ratio_formula(d.ratio_mode, C, P, S);
}
#endif
