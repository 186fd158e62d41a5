// big.hip -- LB_GREEDY (tools.py:2027-2351) for containers the lane-per-cell kernels do not cover: more than
// 64 cells, or a 3D side above 8 (the reference builds W x W containers for any --container_width,
// model.py:279).  Same height-map formulation as tap_place.h, written for ONE THREAD per
// container walking its own cells -- a correctness path for unusual shapes, not a fast one; every BASELINE
// shape takes the lane-per-cell kernels.  Limits: W*L <= 16 384 cells (above 4 096: one workgroup per container, at the
// end of this file); 3D block footprints up to 16 x 16 (beyond the 8 x 8 support masks: tap_stable_wide.h), larger ones
// raise error bit 4 (big_rejects); 2D blocks of any width.  What surrounds a placement -- block fetch, admission, commit,
// feature -- is tap_step_seam.h's; this file holds the placements and the tiles they work on.
#include "tap_common.h"
#include "tap_place.h"
#include "tap_stable_wide.h"
#include "tap_episode.h"
#include "tap_masks.h"
#include "tap_transition.h"
#include "tap_step_seam.h"

#include <type_traits>

// Register budget of the wave-per-container kernels.  The common placement (footprints within the support masks) needs
// 67 .. 83 VGPRs; the instantiation for wide footprints (tap_stable_wide.h: per-row extremes in 64-bit words inside the
// candidate loop) 131 .. 149 -- and a kernel is allocated the maximum over its paths, whether a wave takes them or not:
// with the wide code compiled in, the 10 x 10 step ran at 3 instead of 6 waves per SIMD, 22.9 against 19.8 us (c7,
// same-source A/B, round 5).  Holding the kernels to 5 waves per SIMD (96 VGPRs) leaves the common path unspilled and
// makes the rare wide path spill instead.
// Cells of the one-wavefront and thread-per-container kernels (the fallback's visited set is 64 words; the wave kernels
// pack x into 12 bits); larger containers, up to TAP_BIG_WG_CELLS (tap_common.h), take the one-workgroup-per-container kernels below.
constexpr int TAP_BIG_WAVE_CELLS = 4096;
// threads per container of those kernels, soft / hard rewards (measured at B = 1 024 over 256 / 512 / 1 024: DESIGN.md section 4)
constexpr int TAP_BIG_WG_THREADS_SOFT = 512, TAP_BIG_WG_THREADS_HARD = 1024;

#define TAP_BIG_REGS __attribute__((amdgpu_waves_per_eu(5, 8)))

struct BigCtx {
    int D, W, L, H, flags;
    const uint32_t *lut;
    int32_t *hm;    // this container's W*L heights (global memory)
    int32_t *keys;  // W*L ints of scratch (hard mode: candidate keys)
};

// max / support mask / sum over a footprint
// WIDE: the footprint is beyond the support mask (2D: wider than 64; 3D: a side above 8) -- maximum and sum only, the
// stability test reads the map again (big_stable).  A block's sides are the same on every lane of its container's
// wavefront, so the callers pick the instantiation once per placement: compiled into the common path (even out of line)
// the wide form cost the 10 x 10 step 15 % (c7: 23.1 against 20.1 us, round 5).
__device__ __forceinline__ bool big_is_wide(int D, int bx, int by)
{
    return D == 2 ? bx > 64 : (bx > 8 || by > 8);
}

template <bool WIDE>
__device__ static void big_scan(const BigCtx &c, int x, int y, int bx, int by, int &mx, u64 &eq, int &sum)
{
    mx = -1; eq = 0; sum = 0;
    if constexpr (WIDE) {
        for (int i = 0; i < bx; ++i)
            for (int j = 0; j < by; ++j) {
                const int h = c.hm[(x + i) * c.L + y + j];
                sum += h;
                mx = max(mx, h);
            }
        return;
    }
    for (int i = 0; i < bx; ++i)
        for (int j = 0; j < by; ++j) {
            const int h = c.hm[(x + i) * c.L + y + j];
            sum += h;
            const u64 bit = 1ull << (c.D == 2 ? i : i * 8 + j);
            if (h > mx) { mx = h; eq = bit; }
            else if (h == mx) eq |= bit;
        }
}

// the wide form out of line
__device__ __forceinline__ int big_stable_wide(const int32_t *hm, int L, int x, int y, int bx, int by, int mx)
{
    return tap_stable3d_wide([&](int i, int j) { return hm[(x + i) * L + y + j]; }, bx, by, mx);
}

// tools.is_stable_2d / is_stable of a footprint resting at level z = mx > 0 (eq: big_scan's support mask).  Beyond the
// masks' reach -- 2D blocks wider than 64, 3D sides of 9 .. 16 -- the height-map is read again (tap_stable_wide.h)
template <bool WIDE>
__device__ __forceinline__ int big_stable(const BigCtx &c, int x, int y, int bx, int by, int mx, u64 eq)
{
    if constexpr (WIDE) {
        if (c.D == 2) {
            int lead = 0, trail = 0;                                             // tools.py:839-868: leading / trailing unsupported columns
            while (lead < bx && c.hm[(x + lead) * c.L + y] != mx) ++lead;
            while (trail < bx && c.hm[(x + bx - 1 - trail) * c.L + y] != mx) ++trail;
            return (2 * lead < bx) && (2 * trail < bx);
        }
        return big_stable_wide(c.hm, c.L, x, y, bx, by, mx);
    } else {
        return c.D == 2 ? tap_stable2d(bx, eq) : tap_stable3d_any(c.lut, bx, by, eq);
    }
}

// is cell (x, y) a left-bottom corner, and of which class (tools.py:2067-2078 2D; 2219-2246 3D, appendix B)
__device__ static bool big_corner(const BigCtx &c, int x, int y, int &cls)
{
    const int L = c.L;
    cls = 0;
    if (c.D == 2) return x == 0 || c.hm[x] != c.hm[x - 1];
    if (x == 0 && y == 0) return true;
    auto HM = [&](int a, int b) { return c.hm[a * L + b]; };
    const int h = HM(x, y);
    const int hxm = x > 0 ? HM(x - 1, y) : 0, hym = y > 0 ? HM(x, y - 1) : 0;
    const int hxym = (x > 0 && y > 0) ? HM(x - 1, y - 1) : 0, hxmm = x > 1 ? HM(x - 2, y) : 0;
    const int dx = x > 0 ? h - hxm : 0, dx_ym = (x > 0 && y > 0) ? hym - hxym : 0, dx_xm = x > 1 ? hxm - hxmm : 0;
    const int dy = y > 0 ? h - hym : 0, dy_xm = (x > 0 && y > 0) ? hxm - hxym : 0;
    const bool rej1 = (y > 0) && (dx_ym != 0) && (h == hym) && (dx == dx_ym);   // :2234-2237
    const bool c1 = (dx != 0) && !rej1;
    const bool rej2 = (x > 0) && (dy_xm != 0) && (h == hxm) && (dx == dx_xm);   // :2241-2244 (sic dx)
    const bool c2 = !c1 && (dy != 0) && !rej2;
    if (c1) { cls = 1; return true; }
    if (c2) { cls = 2; return true; }
    return false;
}

__device__ static long big_key(const BigCtx &c, int x, int y, int z, int cls)
{
    return (((long)z * c.L + y) * 3 + cls) * c.W + x;                            // sort order (z, y, class, x)
}

// one placement; the caller advances the step counter.  -> placed?
template <bool WIDE>
__device__ static Placement big_place_t(const BigCtx &c, Counters &cnt, int &err, int bx, int by, int bz)
{
    const int W = c.W, L = c.L, cells = W * L;
    const bool hard = (c.flags & TAP_F_HARD) != 0;
    const PlaceCfg cfg = {W, L, c.H, c.flags, c.lut};
    const int vol = bx * by * bz;
    int gmax = 0;
    for (int i = 0; i < cells; ++i) gmax = max(gmax, c.hm[i]);
    Placement res = {0, 0, 0, 0, 0};
    int emp_w = 0;
    double best = -1.0;
    long bestkey = LONG_MAX;
    if (!hard) {
        bool stop2d = false;
        for (int x = 0; x < W && !stop2d; ++x)
            for (int y = 0; y < L; ++y) {
                int cls;
                if (!big_corner(c, x, y, cls)) continue;
                if (c.D == 2 && x + bx > W) { stop2d = true; break; }          // :2076 stops at the first overflow
                if (x + bx > W || y + by > L) continue;                          // :2255-2256
                int mx, sum; u64 eq;
                big_scan<WIDE>(c, x, y, bx, by, mx, eq, sum);
                const int z = mx;
                if (z >= c.H) err |= 1;                                          // :2109 would raise IndexError
                const int stab = z == 0 ? 1 : big_stable<WIDE>(c, x, y, bx, by, z, eq);
                const int emp = cnt.empty + bx * by * z - sum;
                const double r = tap_score(cfg, cnt, vol, gmax, z, bz, emp, stab);
                const long key = big_key(c, x, y, z, cls);
                if (r > best || (r == best && key < bestkey)) {
                    best = r; bestkey = key; res.placed = 1; res.x = x; res.y = y; res.z = z; res.stab = stab; emp_w = emp;
                }
            }
    } else {
        // keys of the in-bounds corners; then the reference's sequential walk in key order with the shared
        // visited set (tools.py:2100-2121, 2284-2297, 2320-2327) -- see tap_place for the lane-parallel form
        bool stop2d = false;
        for (int x = 0; x < W; ++x)
            for (int y = 0; y < L; ++y) {
                int cls;
                long k = LONG_MAX;
                if (!stop2d && big_corner(c, x, y, cls)) {
                    if (c.D == 2 && x + bx > W) stop2d = true;
                    else if (x + bx <= W && y + by <= L) { int mx, sum; u64 eq; big_scan<WIDE>(c, x, y, bx, by, mx, eq, sum); k = big_key(c, x, y, mx, cls); }
                }
                c.keys[x * L + y] = k > INT_MAX ? INT_MAX : (int)k;
            }
        long last = -1;
        int vis_z = -1;
        // visited spots of the current level: bit (x*L + y), cells <= 4096
        u64 visited[64];
        for (;;) {
            int kmin = INT_MAX;
            for (int i = 0; i < cells; ++i) { const int k = c.keys[i]; if ((long)k > last && k < kmin) kmin = k; }
            if (kmin == INT_MAX) break;
            last = kmin;
            const int X0 = kmin % W;
            int t = kmin / W; t /= 3;
            const int Y0 = t % L, z = t / L;
            if (z != vis_z) { vis_z = z; for (int i = 0; i < (cells + 63) / 64; ++i) visited[i] = 0; }
            bool ok = false;
            int sx = 0, sy = 0, sstab = 0, semp = 0;
            for (int _x = X0; _x + bx <= W && !ok; ++_x)
                for (int _y = Y0; _y + by <= L && !ok; ++_y) {
                    const int sp = _x * L + _y;
                    if ((visited[sp >> 6] >> (sp & 63)) & 1ull) continue;        // :2105
                    int mx, sum; u64 eq;
                    big_scan<WIDE>(c, _x, _y, bx, by, mx, eq, sum);
                    if (z > 0 && mx < z) continue;                               // :2106 nothing underneath
                    visited[sp >> 6] |= 1ull << (sp & 63);                       // :2107
                    if (z >= c.H) { err |= 1; continue; }                        // :2109 IndexError
                    if (mx > z) continue;                                        // :2109 not free
                    const int st = z == 0 ? 1 : big_stable<WIDE>(c, _x, _y, bx, by, z, eq);
                    if (!st) continue;                                           // :2112-2114
                    ok = true; sx = _x; sy = _y; sstab = st; semp = cnt.empty + bx * by * z - sum;
                }
            if (ok) {
                const double r = tap_score(cfg, cnt, vol, gmax, z, bz, semp, sstab);
                if (r > best) { best = r; res.placed = 1; res.x = sx; res.y = sy; res.z = z; res.stab = sstab; emp_w = semp; }
            }
        }
    }
    if (res.placed) {                                                            // tools.py:2167-2174
        for (int i = 0; i < bx; ++i) for (int j = 0; j < by; ++j) c.hm[(res.x + i) * L + res.y + j] = res.z + bz;
        cnt.valid += vol;
        cnt.empty = emp_w;
        cnt.nstable += res.stab;
        if (res.z + bz > c.H) err |= 1;                                          // :2169 numpy clips silently
    } else {
        res.x = res.y = res.z = res.stab = 0;
    }
    return res;
}

__device__ static Placement big_place(const BigCtx &c, Counters &cnt, int &err, int bx, int by, int bz)
{
    return big_is_wide(c.D, bx, by) ? big_place_t<true>(c, cnt, err, bx, by, bz) : big_place_t<false>(c, cnt, err, bx, by, bz);
}

// LB_GREEDY's own limit on a block (the step seam's `family_rejects`): a 3D footprint beyond the support masks THAT FITS
// (one that does not fit finds no position and is filed as a failure); not looked at once the container is full
__device__ __forceinline__ bool big_rejects(const tap_env_desc &d, int count, int bx, int by)
{
    return count < d.n_max && d.D == 3 && (bx > TAP_WIDE_MAX_SIDE || by > TAP_WIDE_MAX_SIDE) && bx <= d.W && by <= d.L;
}

__global__ void __launch_bounds__(TAP_BLOCK) k_big_step(StepArgs a, int32_t *scratch, int lpw)
{
    const int env = tap_spread_env(lpw, a.d.B);                                  // containers spread over the waves (tap_common.h)
    if (env < 0) return;
    const int D = a.d.D, W = a.d.W, L = a.d.L, cells = W * L;
    int32_t *hm = a.v.hm + (size_t)env * cells;
    const SeamBlock b = tap_seam_fetch(a, env);
    bool act;
    Counters cnt = tap_seam_load(a, env, false, act);
    int err = 0;
    const bool do_step = tap_seam_admit(act, cnt.count, a.d.n_max, b.bx, b.by, b.bz, big_rejects(a.d, cnt.count, b.bx, b.by), err);
    const int step = cnt.count;
    Placement pl = {0, 0, 0, 0, 0};
    if (do_step) {
        const BigCtx c = {D, W, L, a.d.H, a.d.flags, a.lut, hm, scratch + (size_t)env * cells};
        pl = big_place(c, cnt, err, b.bx, b.by, b.bz);
        cnt.count += 1;                                                          // tools.py:3713
    }
    tap_seam_commit(a, env, do_step, false, cnt, step, pl, err, nullptr);
    if (a.feature_out) tap_seam_feature(a.d.feature, D, W, L, hm, a.feature_out + (size_t)env * a.flen, 0, 1, [](int v) { return v; });
}

// ---- soft rewards: one WAVEFRONT per container (round 4) ----------------------------------------------------------------
// In soft mode every corner candidate is scored independently and the winner is the first maximum in (z, y, class, x)
// order (tools.py:2161-2165, 2336-2340): lanes take the cells c = lane, lane + 64, ..., keep their best (ratio, key),
// and one wave-wide reduction on (ratio desc, key asc) picks the placement -- the container's height-map sits in the
// wave's LDS tile.  (One thread per container ran 4 096 containers as 64 wavefronts, each the union of 64 control
// flows: 265 us per step at 10 x 10 x 50, 1.9 ms with hard rewards.)  The thread-per-container kernel above remains for
// containers whose tiles do not fit a workgroup's LDS (hard rewards above 2 560 cells).
// HARD: the tile also holds, per cell, the corner key and the position's (max height under the footprint, stable) pair
// and height sum: 4 ints per cell instead of 1.
// One LB_GREEDY placement of a container whose height-map sits in the wave's LDS tile `hm` (HARD: 4 ints per cell, see
// k_big_wave_step): every lane of the wavefront calls this.  Updates the tile (and the global copy `ghm` when given),
// valid / empty / stable in `cnt` and the error bits; the caller advances cnt.count and files the result.  The returned
// placement is the same on every lane.
template <bool HARD, bool WIDE>
__device__ __forceinline__ Placement big_wave_place_t(const tap_env_desc &d, const uint32_t *lut, int32_t *hm, int32_t *ghm, int lane,
                                                      int gmax, Counters &cnt, int &err, int bx, int by, int bz)
{
    const int D = d.D, W = d.W, L = d.L, cells = W * L;
    const BigCtx c = {D, W, L, d.H, d.flags, lut, hm, nullptr};
    const PlaceCfg cfg = {W, L, d.H, d.flags, lut};
    const int vol = bx * by * bz;
    double best = -1.0;
    long bestkey = LONG_MAX;
    int bxy = 0, bzv = 0, bstab = 0, bemp = 0;
    double wr;
    long wk;
    if (!HARD) {
    for (int cell = lane; cell < cells; cell += 64) {
        const int x = cell / L, y = cell - x * L;
        int cls;
        if (!big_corner(c, x, y, cls)) continue;
        if (x + bx > W || y + by > L) continue;                              // :2076 (2D: every later corner overflows too), :2255-2256
        int mx, sum; u64 eq;
        big_scan<WIDE>(c, x, y, bx, by, mx, eq, sum);
        const int z = mx;
        if (z >= d.H) err |= 1;                                            // :2109 would raise IndexError
        const int stab = z == 0 ? 1 : big_stable<WIDE>(c, x, y, bx, by, z, eq);
        const int emp = cnt.empty + bx * by * z - sum;
        const double r = tap_score(cfg, cnt, vol, gmax, z, bz, emp, stab);
        const long key = big_key(c, x, y, z, cls);
        if (r > best || (r == best && key < bestkey)) { best = r; bestkey = key; bxy = x | (y << 12); bzv = z; bstab = stab; bemp = emp; }
    }
    // first maximum in key order over the wave
    wr = best;
    wk = bestkey;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double r2 = __hiloint2double(__shfl_xor(__double2hiint(wr), o), __shfl_xor(__double2loint(wr), o));
        const long k2 = ((long)__shfl_xor((int)(wk >> 32), o) << 32) | (unsigned)__shfl_xor((int)wk, o);
        if (r2 > wr || (r2 == wr && k2 < wk)) { wr = r2; wk = k2; }
    }
    } else {
        // The reference walks the corners in key order and slides each one (x up, then y up from the corner) to the
        // first position that is supported, free and stable, skipping positions an earlier walk of the same level
        // visited (tools.py:2100-2121, 2284-2297, 2320-2327).  A position settles at level z iff the maximum under its
        // footprint IS z and it is stable, so it can settle at one level only and "visited" only matters for
        // positions that settled: per position (max, stable, sum) once, then per corner one wave-wide minimum over
        // the order index x * L + y of the settling, untaken positions of its rectangle.
        int32_t *keys = hm + cells, *pms = keys + cells, *psum = pms + cells;
        for (int cell = lane; cell < cells; cell += 64) {
            const int x = cell / L, y = cell - x * L;
            int cls, k = INT_MAX, ms = -1, sm = 0;
            if (x + bx <= W && y + by <= L) {
                int mx; u64 eq;
                big_scan<WIDE>(c, x, y, bx, by, mx, eq, sm);
                const int st = mx == 0 ? 1 : big_stable<WIDE>(c, x, y, bx, by, mx, eq);
                ms = (mx << 1) | st;
                if (big_corner(c, x, y, cls)) { const long kk = big_key(c, x, y, mx, cls); k = kk > INT_MAX ? INT_MAX : (int)kk; }
            }
            keys[cell] = k; pms[cell] = ms; psum[cell] = sm;
        }
        tap_wave_lds_sync();
        wr = -1.0; wk = 0;
        int last = -1;
        for (;;) {
            int kmin = INT_MAX;
            for (int cell = lane; cell < cells; cell += 64) { const int k = keys[cell]; if (k > last && k < kmin) kmin = k; }
            kmin = group_min<64>(kmin);
            if (kmin == INT_MAX) break;
            last = kmin;
            const int X0 = kmin % W;
            int t = kmin / W; t /= 3;
            const int Y0 = t % L, z = t / L;
            if (z >= d.H) { err |= 1; continue; }                          // :2109 IndexError at the corner's own position
            int first = INT_MAX;
            for (int cell = lane; cell < cells; cell += 64) {
                const int x = cell / L, y = cell - x * L;
                const int ms = pms[cell];
                if (x >= X0 && y >= Y0 && ms == ((z << 1) | 1) && cell < first) first = cell;   // ms < 0: out of bounds or taken
            }
            first = group_min<64>(first);
            if (first == INT_MAX) continue;
            if (lane == 0) pms[first] = -2;                                  // settled: no later walk stops here
            const int sx = first / L, sy = first - sx * L, semp = cnt.empty + bx * by * z - psum[first];
            const double r = tap_score(cfg, cnt, vol, gmax, z, bz, semp, 1);
            if (r > wr) { wr = r; bxy = sx | (sy << 12); bzv = z; bstab = 1; bemp = semp; }    // first maximum in walk order
            tap_wave_lds_sync();
        }
        best = wr; bestkey = wk;                                             // every lane holds the winner
    }
    const bool placed = wr > 0.0;
    const u64 wm = __ballot(placed && best == wr && bestkey == wk);          // keys are unique: one lane
    const int src = wm ? __ffsll((long long)wm) - 1 : 0;
    const int pxy = __shfl(bxy, src), pz = __shfl(bzv, src), pstab = __shfl(bstab, src), pemp = __shfl(bemp, src);
    const int px = pxy & 4095, py = pxy >> 12;
    unsigned eall = (unsigned)err;
    eall = (unsigned)group_or<64>((int)eall);
    err = (int)eall;
    tap_wave_lds_sync();
    if (placed) {                                                            // tools.py:2167-2174
        for (int f = lane; f < bx * by; f += 64) {
            const int i = f / by, j = f - i * by;
            const int cidx = (px + i) * L + py + j;
            hm[cidx] = pz + bz;
            if (ghm) ghm[cidx] = pz + bz;
        }
        cnt.valid += vol;
        cnt.empty = pemp;
        cnt.nstable += pstab;
        if (pz + bz > d.H) err |= 1;                                       // :2169 numpy clips silently
    }
    Placement res = {0, 0, 0, 0, 0};
    if (placed) { res.placed = 1; res.x = px; res.y = py; res.z = pz; res.stab = pstab; }
    return res;
}

template <bool HARD>
__device__ __forceinline__ Placement big_wave_place(const tap_env_desc &d, const uint32_t *lut, int32_t *hm, int32_t *ghm, int lane,
                                                    int gmax, Counters &cnt, int &err, int bx, int by, int bz)
{
    if (__builtin_expect(big_is_wide(d.D, bx, by), 0))                            // wave-uniform, rare
        return big_wave_place_t<HARD, true>(d, lut, hm, ghm, lane, gmax, cnt, err, bx, by, bz);
    return big_wave_place_t<HARD, false>(d, lut, hm, ghm, lane, gmax, cnt, err, bx, by, bz);
}

// One lock-step of one container by one wavefront (every lane calls), on the step seam: load tile, fetch, admit, place,
// commit, feature.  `hm` = the wave's LDS tile.  flags (TAP_T_FRESH: the step starts from an empty container;
// TAP_T_RATIO: emit calc_ratio) as in the fused lane-per-cell step.
template <bool HARD>
__device__ __forceinline__ void big_wave_step_body(const StepArgs &a, int env, int lane, int32_t *hm, int flags, float *ratio_out)
{
    const int D = a.d.D, W = a.d.W, L = a.d.L, cells = W * L;
    const bool fresh = (flags & TAP_T_FRESH) != 0;
    int32_t *ghm = a.v.hm + (size_t)env * cells;
    int gmax = 0;
    if (fresh) { for (int c = lane; c < cells; c += 64) { hm[c] = 0; ghm[c] = 0; } }
    else for (int c = lane; c < cells; c += 64) { const int h = ghm[c]; hm[c] = h; gmax = max(gmax, h); }
    const SeamBlock b = tap_seam_fetch(a, env);
    if (lane == 0) tap_seam_aux(a, env, b);
    bool act;
    Counters cnt = tap_seam_load(a, env, fresh, act);
    int err = 0;
    const bool do_step = tap_seam_admit(act, cnt.count, a.d.n_max, b.bx, b.by, b.bz, big_rejects(a.d, cnt.count, b.bx, b.by), err);
    const int step = cnt.count;
    Placement pl = {0, 0, 0, 0, 0};
    gmax = group_max<64>(gmax);
    tap_wave_lds_sync();
    if (do_step) {                                                               // wave-uniform
        pl = big_wave_place<HARD>(a.d, a.lut, hm, ghm, lane, gmax, cnt, err, b.bx, b.by, b.bz);
        if (pl.placed) gmax = max(gmax, pl.z + b.bz);
        cnt.count += 1;                                                          // tools.py:3713
        tap_wave_lds_sync();
    }
    if (lane == 0) {
        tap_seam_commit(a, env, do_step, fresh, cnt, step, pl, err, nullptr);
        if ((flags & TAP_T_RATIO) && ratio_out) ratio_out[env] = tap_seam_ratio(a.d, cnt, gmax);
    }
    if (a.feature_out)
        tap_seam_feature(a.d.feature, D, W, L, hm, a.feature_out + (size_t)env * a.flen, lane, 64, [](int v) { return group_min<64>(v); });
}

template <bool HARD>
__global__ void __launch_bounds__(TAP_BLOCK) TAP_BIG_REGS k_big_wave_step(StepArgs a)
{
    extern __shared__ int32_t big_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;   // (a vector value: TAP_WAVE_INDEX() measured slower / flat here, tap_common.h)
    const int env = (int)(blockIdx.x * (blockDim.x >> 6)) + wave;               // 1 .. 4 wavefronts per workgroup (tap_big_step)
    if (env >= a.d.B) return;                                                     // wave-uniform
    big_wave_step_body<HARD>(a, env, lane, big_lds + (size_t)wave * a.d.W * a.d.L * (HARD ? 4 : 1), 0, nullptr);
}

// ---- the whole decoding step in ONE launch (round 5): a workgroup = PW placement wavefronts (one container each, as
// above) + ceil(PW / 2) stream waves running update_dynamic + update_mask of the same containers on the bit shadow
// (tap_transition.h: trans_stream_wave), side by side as in k_transition -- the two kinds exchange nothing, so there is
// no barrier.  MODE 1: on the bit shadow; 2: the episode's first step (shadow built in the launch).  Round 4 ran these
// shapes as a mask launch + a placement launch (+ reset / calc_ratio launches at the ends of an episode): 10 x 10 x 50,
// B = 4 096, graph-replayed step 19.5 us (c7).  Measured against it: the container's own wavefront running its slab
// first and then the placement (no stream waves: 12 instead of 8 placement waves per CU at this kernel's 141 VGPRs)
// -- 25.0 us: the placement is short enough here that the serial slab shows; the MACS forms (macs_big.hip,
// macs3_big.hip), whose placements last 40 .. 150 us, are built that way.
template <bool HARD, int NC, int MODE>
__global__ void __launch_bounds__(384) TAP_BIG_REGS k_big_transition(TransArgs a, int PW)
{
    extern __shared__ int32_t big_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;   // (a vector value: TAP_WAVE_INDEX() measured slower / flat here, tap_common.h)
    const int cells = a.s.d.W * a.s.d.L, tile = cells * (HARD ? 4 : 1);
    const int base = blockIdx.x * PW;
    if (wave < PW) {
        const int env = base + wave;
        if (env >= a.s.d.B) return;                                               // wave-uniform
        __builtin_amdgcn_s_setprio(2);
        big_wave_step_body<HARD>(a.s, env, lane, big_lds + (size_t)wave * tile, a.flags, a.ratio_out);
        return;
    }
    const int sw = wave - PW;
    MaskArgs m = a.m;
    m.B = min(m.B, base + PW);                                                    // this workgroup's containers only
    float *slds = reinterpret_cast<float *>(big_lds + (size_t)PW * tile) + (size_t)sw * 2 * 3 * m.nR;
    trans_stream_wave<2, NC, MODE>(m, base + 2 * sw, lane, slds);
}

// ---- whole episodes (round 5): tools.calc_positions_lb_greedy (tools.py:2393-2449) for containers above 64 cells ----
// pack.reward, pack.render and -- in hard mode, inside their acceptance loops -- both instance generators
// (generate.py:908, 112) pack a whole block list from an empty container.  One wavefront per container as in the step
// kernel, the height-map tile living in LDS across the n placements: nothing but the block list and the per-episode
// results touches memory (round 4 stepped these shapes with n launches from the host, and generate.pack_blocks
// refused them).  A tour entry's block is fetched by lane t % 64 for 64 steps at a time (two dependent loads once per
// 64 placements instead of once per placement).
template <bool HARD>
__global__ void __launch_bounds__(TAP_BLOCK) TAP_BIG_REGS k_big_wave_episode(EpisodeArgs a)
{
    extern __shared__ int32_t big_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;   // (a vector value: TAP_WAVE_INDEX() measured slower / flat here, tap_common.h)
    const int env = (int)(blockIdx.x * (blockDim.x >> 6)) + wave;
    const int D = a.d.D, W = a.d.W, L = a.d.L, cells = W * L, n = a.n;
    if (env >= a.B) return;                                                       // wave-uniform
    int32_t *hm = big_lds + (size_t)wave * cells * (HARD ? 4 : 1);
    for (int c = lane; c < cells; c += 64) hm[c] = 0;
    tap_wave_lds_sync();
    Counters cnt = {0, 0, 0, 0};
    int err = 0, gmax = 0;
    for (int t0 = 0; t0 < n; t0 += 64) {
        int mine[3] = {1, 1, 1}, merr = 0;
        bool min_ = false;
        if (t0 + lane < n) {
            if (D == 2) min_ = episode_block<2>(a, env, t0 + lane, true, mine, merr);
            else min_ = episode_block<3>(a, env, t0 + lane, true, mine, merr);
        }
        err |= merr;                                                              // OR-ed over the wave in big_wave_place / below
        for (int j = 0; j < 64 && t0 + j < n; ++j) {
            const int t = t0 + j;
            const int b0 = __shfl(mine[0], j), b1 = __shfl(mine[1], j), b2 = __shfl(mine[2], j);
            const bool in = __shfl((int)min_, j) != 0;
            const int bx = b0, by = D == 3 ? b1 : 1, bz = D == 3 ? b2 : b1;
            const bool do_step = tap_seam_admit(in, cnt.count, a.d.n_max, bx, by, bz, big_rejects(a.d, cnt.count, bx, by), err);
            Placement pl = {0, 0, 0, 0, 0};
            if (do_step) {                                                        // wave-uniform
                pl = big_wave_place<HARD>(a.d, a.lut, hm, nullptr, lane, gmax, cnt, err, bx, by, bz);
                if (pl.placed) gmax = max(gmax, pl.z + bz);
                cnt.count += 1;                                                   // tools.py:3713
                tap_wave_lds_sync();
            }
            if (lane == 0) {
                if (a.pos_out) {
                    int32_t *pp = a.pos_out + ((size_t)env * n + t) * D;
                    pp[0] = pl.x;
                    if (D == 3) { pp[1] = pl.y; pp[2] = pl.z; } else pp[1] = pl.z;
                }
                if (a.stable_out) a.stable_out[(size_t)env * n + t] = (uint8_t)pl.stab;
            }
        }
    }
    err = group_or<64>(err);
    if (lane == 0) episode_finish(a, env, cnt, gmax, err);
}

// ---- containers above 4 096 cells: one WORKGROUP per container ---------------------------------------------------------
// The one-wavefront kernels above hold a container in one wave's LDS tile and the thread-per-container fallback keeps a
// 4 096-bit visited set, so W*L stopped at 4 096 cells; the reference builds a W x W map for any --container_width,
// scaled by --unit (model.py:279, pack.py:123).  Here NT = 512 (soft) / 1 024 (hard rewards) threads share one
// container up to 16 384 cells: its height-map lives in the workgroup's LDS for the whole step (64 KiB at 16 384 cells),
// every thread takes the cells tid, tid + NT, ... and the selections of big_wave_place_t become a wave-level reduction
// followed by a cross-wave one through LDS -- double-buffered, so one __syncthreads per round.
// HARD: one word per position beside the map in LDS (128 KiB at 16 384 cells; big_wg_place_t), from which the corner
// keys are recomputed, and the height sum under a settling position is summed by the workgroup when the walk stops there
// -- nothing per cell outside the LDS, so the whole-episode kernel needs no memory of its own either.
// The 32-bit corner key ((z L + y) 3 + cls) W + x stays below 2^31 at H <= 4 000 and W*L <= TAP_BIG_WG_CELLS.

// cross-wave scratch of one workgroup: two buffers (alternating rounds) of per-wave entries
struct BigWgRed {
    double r[2][16];
    long k[2][16];
    int v[2][16][5];
};

template <int NT>
struct BigWg {
    static constexpr int NW = NT / 64;
    BigWgRed *red;
    int par;     // buffer of the next round (the same on every thread)
    int wave, lane;
    // op over the workgroup; every thread gets the result
    template <class Op>
    __device__ __forceinline__ int all(int v, Op op)
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
        int *r = &red->v[par][0][0];
        if (lane == 0) r[wave] = v;
        __syncthreads();
        int w = r[0];
#pragma unroll
        for (int i = 1; i < NW; ++i) w = op(w, r[i]);
        par ^= 1;
        return w;
    }
    __device__ __forceinline__ int min(int v) { return all(v, [](int a, int b) { return a < b ? a : b; }); }
    __device__ __forceinline__ int max(int v) { return all(v, [](int a, int b) { return a > b ? a : b; }); }
    __device__ __forceinline__ int sum(int v) { return all(v, [](int a, int b) { return a + b; }); }
    __device__ __forceinline__ int orr(int v) { return all(v, [](int a, int b) { return a | b; }); }
};

// One LB_GREEDY placement of a container whose height-map `hm` sits in the workgroup's LDS (HARD: followed by cells ints
// of the per-position word below); every thread calls this.  Same contract as
// big_wave_place_t: updates the map (and `ghm` when given), valid / empty / stable in `cnt` and the error bits (OR-ed over
// the workgroup on return); the caller advances cnt.count.  The placement is the same on every thread.
template <int NT, bool HARD, bool WIDE>
__device__ __forceinline__ Placement big_wg_place_t(BigWg<NT> &g, const tap_env_desc &d, const uint32_t *lut, int32_t *hm,
                                                    int32_t *ghm, int gmax, Counters &cnt, int &err, int bx, int by, int bz)
{
    const int D = d.D, W = d.W, L = d.L, cells = W * L, tid = threadIdx.x;
    const BigCtx c = {D, W, L, d.H, d.flags, lut, hm, nullptr};
    const PlaceCfg cfg = {W, L, d.H, d.flags, lut};
    const int vol = bx * by * bz;
    double wr = -1.0;
    int px = 0, py = 0, pz = 0, pstab = 0, pemp = 0;
    if (!HARD) {
        double best = -1.0;
        long bestkey = LONG_MAX;
        int bx_ = 0, by_ = 0, bzv = 0, bstab = 0, bemp = 0;
        for (int cell = tid; cell < cells; cell += NT) {
            const int x = cell / L, y = cell - x * L;
            int cls;
            if (!big_corner(c, x, y, cls)) continue;
            if (x + bx > W || y + by > L) continue;                              // :2076 (2D: every later corner overflows too), :2255-2256
            int mx, sum; u64 eq;
            big_scan<WIDE>(c, x, y, bx, by, mx, eq, sum);
            const int z = mx;
            if (z >= d.H) err |= 1;                                            // :2109 would raise IndexError
            const int stab = z == 0 ? 1 : big_stable<WIDE>(c, x, y, bx, by, z, eq);
            const int emp = cnt.empty + bx * by * z - sum;
            const double r = tap_score(cfg, cnt, vol, gmax, z, bz, emp, stab);
            const long key = big_key(c, x, y, z, cls);
            if (r > best || (r == best && key < bestkey)) { best = r; bestkey = key; bx_ = x; by_ = y; bzv = z; bstab = stab; bemp = emp; }
        }
        // first maximum on (ratio desc, key asc): over the wave, then over the waves
        double r = best;
        long k = bestkey;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double r2 = __hiloint2double(__shfl_xor(__double2hiint(r), o), __shfl_xor(__double2loint(r), o));
            const long k2 = ((long)__shfl_xor((int)(k >> 32), o) << 32) | (unsigned)__shfl_xor((int)k, o);
            if (r2 > r || (r2 == r && k2 < k)) { r = r2; k = k2; }
        }
        const u64 wm = __ballot(best == r && bestkey == k);                     // keys are unique: one lane (or none placed)
        const int src = wm ? __ffsll((long long)wm) - 1 : 0;
        const int v0 = __shfl(bx_, src), v1 = __shfl(by_, src), v2 = __shfl(bzv, src), v3 = __shfl(bstab, src), v4 = __shfl(bemp, src);
        const int p = g.par;
        if (g.lane == 0) {
            g.red->r[p][g.wave] = r; g.red->k[p][g.wave] = k;
            int *v = g.red->v[p][g.wave];
            v[0] = v0; v[1] = v1; v[2] = v2; v[3] = v3; v[4] = v4;
        }
        __syncthreads();
        int win = 0;
        wr = g.red->r[p][0];
        long wk = g.red->k[p][0];
        for (int w = 1; w < BigWg<NT>::NW; ++w) {
            const double r2 = g.red->r[p][w];
            const long k2 = g.red->k[p][w];
            if (r2 > wr || (r2 == wr && k2 < wk)) { wr = r2; wk = k2; win = w; }
        }
        const int *v = g.red->v[p][win];
        px = v[0]; py = v[1]; pz = v[2]; pstab = v[3]; pemp = v[4];
        g.par ^= 1;
    } else {
        // big_wave_place_t's walk (tools.py:2100-2121, 2284-2297, 2320-2327): per position one word, then per corner in
        // key order the first settling, untaken position of its rectangle in the order x * L + y.  The word packs what
        // both scans need -- (max << 5) | taken << 4 | corner << 3 | class << 1 | stable, -1 out of bounds -- so the
        // corner keys are recomputed from it (a few integer operations per cell) instead of being kept per cell: the map
        // and the words are 2 ints per cell of LDS, 128 KiB at 16 384 cells.  max is clamped to 2^25: such a level is
        // far beyond H <= 4 000 (its key exceeds 2^31 and is never walked, as big_key's clamp does).
        int32_t *pw = hm + cells;
        for (int cell = tid; cell < cells; cell += NT) {
            const int x = cell / L, y = cell - x * L;
            int w = -1;
            if (x + bx <= W && y + by <= L) {
                int mx, sm, cls; u64 eq;
                big_scan<WIDE>(c, x, y, bx, by, mx, eq, sm);
                const int st = mx == 0 ? 1 : big_stable<WIDE>(c, x, y, bx, by, mx, eq);
                const bool corner = big_corner(c, x, y, cls);
                w = (min(mx, 1 << 25) << 5) | (corner ? 8 | (cls << 1) : 0) | st;
            }
            pw[cell] = w;
        }
        __syncthreads();
        long last = -1;
        for (;;) {
            long kmin = LONG_MAX;
            for (int cell = tid; cell < cells; cell += NT) {
                const int w = pw[cell];
                if (w < 0 || !(w & 8)) continue;
                const int x = cell / L, y = cell - x * L;
                const long k = big_key(c, x, y, w >> 5, (w >> 1) & 3);
                if (k > last && k < kmin) kmin = k;
            }
            const int k32 = g.min(kmin > INT_MAX ? INT_MAX : (int)kmin);
            if (k32 == INT_MAX) break;
            last = k32;
            const int X0 = k32 % W;
            int t = k32 / W; t /= 3;
            const int Y0 = t % L, z = t / L;
            if (z >= d.H) { err |= 1; continue; }                                // :2109 IndexError at the corner's own position
            int first = INT_MAX;
            for (int cell = X0 * L + tid; cell < cells; cell += NT) {           // positions x >= X0 only
                const int y = cell - (cell / L) * L;
                const int w = pw[cell];
                if (y >= Y0 && w >= 0 && (w & 17) == 1 && (w >> 5) == z) { first = cell; break; }   // settles at z, untaken
            }
            first = g.min(first);
            if (first == INT_MAX) continue;
            const int sx = first / L, sy = first - sx * L;
            int s = 0;
            for (int f = tid; f < bx * by; f += NT) { const int i = f / by, j = f - i * by; s += hm[(sx + i) * L + sy + j]; }
            s = g.sum(s);                                                        // (its barrier orders the store below after
            if (tid == 0) pw[first] |= 16;                                       //  every read of this walk) settled: taken
            const int semp = cnt.empty + bx * by * z - s;
            const double r = tap_score(cfg, cnt, vol, gmax, z, bz, semp, 1);
            if (r > wr) { wr = r; px = sx; py = sy; pz = z; pstab = 1; pemp = semp; }    // first maximum in walk order
        }
    }
    const bool placed = wr > 0.0;
    err = g.orr(err);
    if (placed) {                                                                // tools.py:2167-2174
        for (int f = tid; f < bx * by; f += NT) {
            const int i = f / by, j = f - i * by;
            const int cidx = (px + i) * L + py + j;
            hm[cidx] = pz + bz;
            if (ghm) ghm[cidx] = pz + bz;
        }
        cnt.valid += vol;
        cnt.empty = pemp;
        cnt.nstable += pstab;
        if (pz + bz > d.H) err |= 1;                                           // :2169 numpy clips silently
    }
    __syncthreads();
    Placement res = {0, 0, 0, 0, 0};
    if (placed) { res.placed = 1; res.x = px; res.y = py; res.z = pz; res.stab = pstab; }
    return res;
}

template <int NT, bool HARD>
__device__ __forceinline__ Placement big_wg_place(BigWg<NT> &g, const tap_env_desc &d, const uint32_t *lut, int32_t *hm,
                                                  int32_t *ghm, int gmax, Counters &cnt, int &err, int bx, int by, int bz)
{
    if (__builtin_expect(big_is_wide(d.D, bx, by), 0))                            // workgroup-uniform, rare
        return big_wg_place_t<NT, HARD, true>(g, d, lut, hm, ghm, gmax, cnt, err, bx, by, bz);
    return big_wg_place_t<NT, HARD, false>(g, d, lut, hm, ghm, gmax, cnt, err, bx, by, bz);
}

// tap_env_step / tap_env_step_gather: one lock-step of container blockIdx.x (gather / block, placement, state and
// results out, feature), as k_big_step.  NOT on the step seam (tap_step_seam.h), on a measurement: with the seam's fetch and
// admission in front of it the placement was compiled differently and hard rewards on 2D 8 192 x 100 ran 2 .. 3 % slower
// at every batch size (soft rewards 5 .. 6 % faster, 3D hard 1 % faster; cause not found).  This body is the
// pre-seam one, instruction for instruction.
template <int NT, bool HARD>
__global__ void __launch_bounds__(NT) k_big_wg_step(StepArgs a)
{
    extern __shared__ int32_t big_lds[];
    __shared__ BigWgRed red;
    BigWg<NT> g = {&red, 0, (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63)};
    const int env = blockIdx.x, tid = threadIdx.x;
    const int B = a.d.B, D = a.d.D, W = a.d.W, L = a.d.L, cells = W * L;
    int32_t *hm = big_lds, *ghm = a.v.hm + (size_t)env * cells;
    int gmax = 0;
    for (int c = tid; c < cells; c += NT) { const int h = ghm[c]; hm[c] = h; gmax = max(gmax, h); }
    gmax = g.max(gmax);                                                          // (its barrier publishes the tile)
    int dims[3] = {1, 1, 1};
    if (a.static_) {                                                             // model.py:404-412
        bool badp;
        const long p = tap_col((long)a.ptr[env], a.nR, badp);
        for (int k = 0; k < D; ++k) dims[k] = badp ? 0 : (int)a.static_[((size_t)env * a.static_rows + 1 + k) * a.nR + p];
    } else if (a.blocks_dtype == TAP_DT_F32) {
        for (int k = 0; k < D; ++k) dims[k] = (int)((const float *)a.blocks)[(size_t)env * D + k];
    } else {
        for (int k = 0; k < D; ++k) dims[k] = ((const int32_t *)a.blocks)[(size_t)env * D + k];
    }
    const bool act = !a.active || a.active[env] != 0;
    const int4 cv = reinterpret_cast<const int4 *>(a.v.cnt)[env];
    Counters cnt = {cv.x, cv.y, cv.z, cv.w};
    const int bx = dims[0], by = D == 3 ? dims[1] : 1, bz = dims[D - 1];
    int err = 0;
    bool do_step = act;
    if (act && cnt.count >= a.d.n_max) { err |= 2; do_step = false; }
    if (act && (bx < 1 || by < 1 || bz < 1)) { err |= 4; do_step = false; }
    if (act && do_step && (D == 3 && (bx > TAP_WIDE_MAX_SIDE || by > TAP_WIDE_MAX_SIDE) && bx <= W && by <= L)) {
        err |= 4; do_step = false;                                               // footprint beyond the support masks
    }
    if (do_step) {                                                               // workgroup-uniform
        const int step = cnt.count;
        const Placement pl = big_wg_place<NT, HARD>(g, a.d, a.lut, hm, ghm, gmax, cnt, err, bx, by, bz);
        cnt.count += 1;                                                          // tools.py:3713
        if (tid == 0) {
            reinterpret_cast<int4 *>(a.v.cnt)[env] = make_int4(cnt.valid, cnt.empty, cnt.nstable, cnt.count);
            int32_t *q = a.v.pos + (size_t)step * D * B + env;
            q[0] = pl.x;
            if (D == 3) { q[B] = pl.y; q[2 * (size_t)B] = pl.z; } else q[B] = pl.z;
            a.v.stable[(size_t)step * B + env] = (uint8_t)pl.stab;
        }
    }
    if (tid == 0 && err) a.v.err[env] |= err;
    if (a.feature_out) {                                                         // tools.py:3716-3744, threads over the cells
        float *out = a.feature_out + (size_t)env * a.flen;
        if (a.d.feature == TAP_FEAT_DIFF) {
            if (D == 2) { for (int c = tid; c + 1 < W; c += NT) out[c] = (float)(hm[c + 1] - hm[c]); }
            else
                for (int c = tid; c < cells; c += NT) {
                    const int x = c / L, y = c - x * L;
                    out[c] = (float)(x > 0 ? hm[c] - hm[c - L] : 0);
                    out[cells + c] = (float)(y > 0 ? hm[c] - hm[c - 1] : 0);
                }
        } else {
            int mn = 0;
            if (a.d.feature == TAP_FEAT_ZERO) {
                mn = INT_MAX;
                for (int c = tid; c < cells; c += NT) mn = min(mn, hm[c]);
                mn = g.min(mn);
            }
            for (int c = tid; c < cells; c += NT) out[c] = (float)(hm[c] - mn);
        }
    }
}

// tap_pack_blocks / tap_episode_reward / tap_episode_scores: a whole episode of container blockIdx.x with its height-map
// in LDS across the n placements, as k_big_wave_episode (every thread reads the tour entry of the step itself: the
// same address on all of them)
template <int NT, bool HARD>
__global__ void __launch_bounds__(NT) k_big_wg_episode(EpisodeArgs a)
{
    extern __shared__ int32_t big_lds[];
    __shared__ BigWgRed red;
    BigWg<NT> g = {&red, 0, (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63)};
    const int env = blockIdx.x, tid = threadIdx.x;
    const int D = a.d.D, W = a.d.W, L = a.d.L, cells = W * L, n = a.n;
    int32_t *hm = big_lds;
    for (int c = tid; c < cells; c += NT) hm[c] = 0;
    __syncthreads();
    Counters cnt = {0, 0, 0, 0};
    int err = 0, gmax = 0;
    for (int t = 0; t < n; ++t) {
        int dims[3];
        const bool in = D == 2 ? episode_block<2>(a, env, t, true, dims, err) : episode_block<3>(a, env, t, true, dims, err);
        const int bx = dims[0], by = D == 3 ? dims[1] : 1, bz = D == 3 ? dims[2] : dims[1];
        const bool do_step = tap_seam_admit(in, cnt.count, a.d.n_max, bx, by, bz, big_rejects(a.d, cnt.count, bx, by), err);
        Placement pl = {0, 0, 0, 0, 0};
        if (do_step) {                                                            // workgroup-uniform
            pl = big_wg_place<NT, HARD>(g, a.d, a.lut, hm, nullptr, gmax, cnt, err, bx, by, bz);
            if (pl.placed) gmax = max(gmax, pl.z + bz);
            cnt.count += 1;                                                       // tools.py:3713
        }
        if (tid == 0) {
            if (a.pos_out) {
                int32_t *pp = a.pos_out + ((size_t)env * n + t) * D;
                pp[0] = pl.x;
                if (D == 3) { pp[1] = pl.y; pp[2] = pl.z; } else pp[1] = pl.z;
            }
            if (a.stable_out) a.stable_out[(size_t)env * n + t] = (uint8_t)pl.stab;
        }
    }
    if (tid == 0) episode_finish(a, env, cnt, gmax, err);
}

// threads per container of the workgroup kernels (A/B builds, tap_ab_env: TAP_BIG_WG_THREADS = 256 / 512 / 1024, read once)
static int big_wg_threads(bool hard)
{
    static const int forced = [] {
        const char *e = tap_ab_env("TAP_BIG_WG_THREADS");
        const int v = e ? atoi(e) : 0;
        return (v == 256 || v == 512 || v == 1024) ? v : 0;
    }();
    return forced ? forced : hard ? TAP_BIG_WG_THREADS_HARD : TAP_BIG_WG_THREADS_SOFT;
}

static size_t big_wg_lds(const tap_env_desc &d) { return (size_t)d.W * d.L * sizeof(int32_t) * ((d.flags & TAP_F_HARD) ? 2 : 1); }

template <class Launch>
static int big_wg_dispatch(tap_ctx *ctx, const tap_env_desc &d, Launch launch)
{
    const size_t lds = big_wg_lds(d);
    if (lds + sizeof(BigWgRed) > tap_lds_limit(ctx))
        return tap_fail(ctx, TAP_E_UNSUPPORTED, "%d x %d containers%s: the height-map does not fit a workgroup's LDS", d.W, d.L,
                        (d.flags & TAP_F_HARD) ? " with hard rewards" : "");
    const bool hard = (d.flags & TAP_F_HARD) != 0;
    switch (big_wg_threads(hard)) {
    case 256: return hard ? launch(std::integral_constant<int, 256>(), std::true_type(), lds) : launch(std::integral_constant<int, 256>(), std::false_type(), lds);
    case 1024: return hard ? launch(std::integral_constant<int, 1024>(), std::true_type(), lds) : launch(std::integral_constant<int, 1024>(), std::false_type(), lds);
    default: return hard ? launch(std::integral_constant<int, 512>(), std::true_type(), lds) : launch(std::integral_constant<int, 512>(), std::false_type(), lds);
    }
}

static int big_wg_step(tap_ctx *ctx, const StepArgs &a, hipStream_t st)
{
    return big_wg_dispatch(ctx, a.d, [&](auto nt, auto hard, size_t lds) -> int {
        constexpr int NT = decltype(nt)::value;
        constexpr bool H = decltype(hard)::value;
        TAP_HIP_CHECK(ctx, tap_allow_lds(k_big_wg_step<NT, H>, lds));
        hipLaunchKernelGGL((k_big_wg_step<NT, H>), dim3(a.d.B), dim3(NT), lds, st, a);
        TAP_LAUNCH_CHECK(ctx, "k_big_wg_step");
        return TAP_OK;
    });
}

static int big_wg_episode(tap_ctx *ctx, const EpisodeArgs &a, hipStream_t st)
{
    return big_wg_dispatch(ctx, a.d, [&](auto nt, auto hard, size_t lds) -> int {
        constexpr int NT = decltype(nt)::value;
        constexpr bool H = decltype(hard)::value;
        TAP_HIP_CHECK(ctx, tap_allow_lds(k_big_wg_episode<NT, H>, lds));
        hipLaunchKernelGGL((k_big_wg_episode<NT, H>), dim3(a.B), dim3(NT), lds, st, a);
        TAP_LAUNCH_CHECK(ctx, "k_big_wg_episode");
        return TAP_OK;
    });
}

int tap_big_episode(tap_ctx *ctx, const EpisodeArgs &a, hipStream_t st)
{
    if (a.B == 0) return TAP_OK;
    if (a.d.W * a.d.L > TAP_BIG_WAVE_CELLS) return big_wg_episode(ctx, a, st);   // one workgroup per container
    const bool hard = (a.d.flags & TAP_F_HARD) != 0;
    const size_t tile = (size_t)a.d.W * a.d.L * sizeof(int32_t) * (hard ? 4 : 1);
    const int waves = tap_wave_kernels_off() ? 0 : tap_waves_per_wg(ctx, tile);
    const size_t lds = (size_t)waves * tile;
    if (waves == 0)
        return tap_fail(ctx, TAP_E_UNSUPPORTED, "whole episodes of %d x %d containers%s: the height-map tile does not fit a workgroup's "
                                                "LDS, step them with tap_env_step_gather", a.d.W, a.d.L, hard ? " with hard rewards" : "");
    const dim3 g((a.B + waves - 1) / waves);
    if (hard) {
        TAP_HIP_CHECK(ctx, tap_allow_lds(k_big_wave_episode<true>, lds));
        hipLaunchKernelGGL(k_big_wave_episode<true>, g, dim3(waves * 64), lds, st, a);
    } else {
        TAP_HIP_CHECK(ctx, tap_allow_lds(k_big_wave_episode<false>, lds));
        hipLaunchKernelGGL(k_big_wave_episode<false>, g, dim3(waves * 64), lds, st, a);
    }
    TAP_LAUNCH_CHECK(ctx, "k_big_wave_episode");
    return TAP_OK;
}

// get_heightmap's feature of the current maps, one wavefront per container, lanes over the cells (it was one thread per
// container until the end of round 4: 74 .. 340 us per call at 10x10 .. 20x20, more than the MACS 3D placement it follows)
__global__ void __launch_bounds__(TAP_BLOCK) k_big_feature(tap_env_desc d, EnvView v, float *out, int flen)
{
    const int lane = threadIdx.x & 63;
    const int env = (int)(((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (env >= d.B) return;                                                       // wave-uniform
    tap_seam_feature(d.feature, d.D, d.W, d.L, v.hm + (size_t)env * d.W * d.L, out + (size_t)env * flen, lane, 64,
                     [](int v) { return group_min<64>(v); });
}

int tap_big_step(tap_ctx *ctx, const StepArgs &a, void *state, hipStream_t st)
{
    const int grid = (a.d.B + TAP_BLOCK - 1) / TAP_BLOCK;
    if (grid == 0) return TAP_OK;
    (void)state;
    if (a.d.W * a.d.L > TAP_BIG_WAVE_CELLS) return big_wg_step(ctx, a, st);     // one workgroup per container
    const bool hard = (a.d.flags & TAP_F_HARD) != 0;
    const size_t tile = (size_t)a.d.W * a.d.L * sizeof(int32_t) * (hard ? 4 : 1);
    const int waves = tap_wave_kernels_off() ? 0 : tap_waves_per_wg(ctx, tile);
    const size_t lds = (size_t)waves * tile;
    if (waves > 0) {                                                             // one wavefront per container
        const dim3 g((a.d.B + waves - 1) / waves);
        if (hard) {
            TAP_HIP_CHECK(ctx, tap_allow_lds(k_big_wave_step<true>, lds));
            hipLaunchKernelGGL(k_big_wave_step<true>, g, dim3(waves * 64), lds, st, a);
        } else {
            TAP_HIP_CHECK(ctx, tap_allow_lds(k_big_wave_step<false>, lds));
            hipLaunchKernelGGL(k_big_wave_step<false>, g, dim3(waves * 64), lds, st, a);
        }
        TAP_LAUNCH_CHECK(ctx, "k_big_wave_step");
        return TAP_OK;
    }
    const int lpw = tap_spread_lpw(a.d.B);
    hipLaunchKernelGGL(k_big_step, dim3(tap_spread_grid(a.d.B, lpw, TAP_BLOCK)), dim3(TAP_BLOCK), 0, st, a, a.v.scratch, lpw);
    TAP_LAUNCH_CHECK(ctx, "k_big_step");
    return TAP_OK;
}

// placement wavefronts per workgroup of the fused step for this shape, 0 = no fused kernel (the tile does not fit)
static int big_transition_pw(const tap_ctx *ctx, const tap_env_desc *d, int nR)
{
    if (tap_wave_kernels_off() || d->strategy != TAP_LB_GREEDY || d->W * d->L > TAP_BIG_WAVE_CELLS) return 0;   // (above: two launches)
    const bool hard = (d->flags & TAP_F_HARD) != 0;
    const size_t tile = (size_t)d->W * d->L * sizeof(int32_t) * (hard ? 4 : 1);
    for (int pw = 4; pw >= 1; pw >>= 1)
        if ((size_t)pw * tile + (size_t)((pw + 1) / 2) * 2 * 3 * nR * sizeof(float) <= tap_lds_limit(ctx)) return pw;
    return 0;
}

bool tap_big_transition_ok(const tap_ctx *ctx, const tap_env_desc *d, int nR) { return big_transition_pw(ctx, d, nR) > 0; }

int tap_big_transition(tap_ctx *ctx, const tap_env_desc *d, const TransArgs &a, hipStream_t st)
{
    const int pw = big_transition_pw(ctx, d, a.m.nR);
    if (pw == 0) return tap_fail(ctx, TAP_E_UNSUPPORTED, "no fused step for this container");
    const bool hard = (d->flags & TAP_F_HARD) != 0;
    const size_t tile = (size_t)d->W * d->L * sizeof(int32_t) * (hard ? 4 : 1);
    const int sw = (pw + 1) / 2;
    const size_t lds = (size_t)pw * tile + (size_t)sw * 2 * 3 * a.m.nR * sizeof(float);
    const dim3 g((d->B + pw - 1) / pw), blk(64 * (pw + sw));
    if (g.x == 0) return TAP_OK;
    const TapVariant v = tap_stream_variant(TAP_SV_BIG, tap_mask_facts(a.m), TapLaunchFacts{d->D, 64, pw, d->B, d->W, d->L, hard});
    return tap_launch_variant<TAP_SV_BIG>(ctx, "k_big_transition", v, a.m.wt, [&](auto k) -> int {
        using K = decltype(k);
        TAP_HIP_CHECK(ctx, tap_allow_lds(k_big_transition<(K::extra != 0), K::nc, K::mode>, lds));
        hipLaunchKernelGGL((k_big_transition<(K::extra != 0), K::nc, K::mode>), g, blk, lds, st, a, pw);
        return TAP_OK;
    });
}

int tap_big_feature(tap_ctx *ctx, const tap_env_desc *d, const EnvView &v, float *out, int flen, hipStream_t st)
{
    if (d->B == 0) return TAP_OK;
    const int wpb = TAP_BLOCK / 64;
    hipLaunchKernelGGL(k_big_feature, dim3((d->B + wpb - 1) / wpb), dim3(TAP_BLOCK), 0, st, *d, v, out, flen);
    TAP_LAUNCH_CHECK(ctx, "k_big_feature");
    return TAP_OK;
}
