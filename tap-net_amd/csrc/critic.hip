// critic.hip -- the state critic on the bit shadow: the reference's realCritic (trainer.py:18-94) after its GRU step, with
// everything that depends on the parameters alone folded out of it (tapenv.h: tap_critic_value has the contract).  The
// static encoder is a 1x1 convolution of S = 2-4 rows, so W's action on static_hidden is G0 . x per column; the dynamic
// encoder meets a 0/1 tensor, so W's action on dynamic_hidden is the sum of a few columns of M (H, rows) -- the scalar
// loop over set bits of encode.hip --; every context is static_hidden . p with sum p = 1, i.e. Es (x . p) + bs: S numbers
// per env.  A call reads x (B, S, nR) and the shadow and writes B values: no static_hidden, no dynamic_hidden, no
// concatenation, no GEMM.
//
// Geometry.  A wavefront per env, four envs per workgroup, lanes along the hidden rows: HPL = H / 64 rows per lane
// (row = lane + 64 i).  The n process blocks of an env are serial and stay inside its wavefront.  Per block: a sweep
// over the columns -- U[j, c] = g[j] + the M[j, r] of the set rows + G0[j, :] . x[:, c], then v[j] tanh(U + q[j]), a
// lane's own rows in order, an xor butterfly -> s[c] --, then the softmax and the S sums x . p with lanes along the
// columns, then q for the next block from S fmafs per row.  M is staged once per workgroup in an [r][j] LDS copy with
// an odd stride (MALL = 1); where rows (H + 1) floats exceed 32 KB the copy holds ONE slab of 64 hidden rows at a time
// (MALL = 0), the sweeps run per slab (one row per lane, s[c] adds the slabs in order) and the workgroup refills it
// between them.  U is RESIDENT in the wavefront's LDS ([c][j], stride H + 1) where M, the four U and the per-env vectors
// fit 64 KB -- block 0 writes it, the later blocks read it -- and is recomputed per block where they do not; its sum
// order is the same either way.  64 KB: two workgroups per CU beside each other of gfx950's 160 KB when U is resident,
// four or more when it is not.  A wavefront of the last workgroup that has no env repeats the batch's last env and
// stores nothing, so every barrier is reached by all four.  Every order is fixed by the shape: two calls give the same
// bytes.  No atomics.
//
// Backward: the blocks in descending order, U recomputed in every one; per block dxbar from dz or the later block's
// dq, ds through the softmax with lanes along the columns, then the sweep: dA = ds v (1 - tanh^2), dq[j] = sum_c dA,
// dv[j] += ds tanh.  dU = the sum of the blocks' dA is accumulated in the wavefront's LDS where it fits (RESIDENT = 1,
// the same test as the forward's with dv's partials added) and leaves as float4s, (B, H, nR) columns fastest -- the
// layout tap_encode_bits_backward takes as g --; where it does not fit every block's ds is kept in the caller's scratch
// and a second sweep, columns outside and blocks inside, recomputes the tanh and writes dU_out once, a float4 per lane
// and four columns.  dv leaves as one partial per workgroup in the caller's scratch, added in workgroup order by a
// second launch.
//
// Launch record (tapenv.h: tap_variant_hits): (31, RESIDENT, HPL, PLANES, MALL, BACKWARD, 0).
#include <algorithm>

#include "tap_bitshadow.h"
#include "tap_common.h"

namespace {

constexpr int TAP_HIT_CRITIC = 31; // launch record, after heightmap.hip's 30
constexpr int CR_NW = TAP_BLOCK / 64;       // envs per workgroup: one per wavefront
constexpr int CR_MAXS = 8, CR_MAXN = 8;     // static rows, process blocks
constexpr size_t CR_LDS_BUDGET = 64 * 1024;
constexpr size_t CR_M_ALL = 32 * 1024;      // the whole of M is staged up to here, one 64-row slab at a time above

struct CrGeom {
    int planes, hpl, mall, resident, blocks;
    size_t lds;
};
inline CrGeom cr_geom(int B, int nR, int rows, int H, bool backward)
{
    CrGeom g;
    g.planes = tap_bit_planes(rows);
    g.hpl = H / 64;
    g.mall = (H == 64 || (size_t)rows * (H + 1) * sizeof(float) <= CR_M_ALL) ? 1 : 0;
    // M (or a slab of it), s / p / ds per wavefront; the backward adds the wavefronts' dv
    const size_t base = (size_t)rows * ((g.mall ? H : 64) + 1) + (size_t)CR_NW * nR + (backward ? (size_t)CR_NW * H : 0);
    const size_t u = (size_t)CR_NW * nR * (H + 1);
    g.resident = (base + u) * sizeof(float) <= CR_LDS_BUDGET ? 1 : 0;
    g.lds = (base + (g.resident ? u : 0)) * sizeof(float);             // base alone is at most 41 KB
    g.blocks = (B + CR_NW - 1) / CR_NW;
    return g;
}

struct CrArgs {
    const float *x;                 // (B, S, nR)
    const unsigned long long *bits; // (B, planes, nR)
    const float *G, *g, *M;         // (3 H, S), (3 H,), (H, rows)
    const float *q0, *v, *w2, *b2;  // (B or 1, H), (H,), (H,), (1,)
    float *value, *z, *p, *xbar, *q; // (B,), (B, H), (B, n, nR), (B, n, S), (B, n, H): the forward's outputs; p, q the backward's inputs
    const float *dz;                // backward: (B, H)
    float *dU, *dq, *part, *dsg;    // backward: (B, H, nR), (B, n, H), (blocks, H), and (B, n, nR) where dU is not resident
    int B, nR, rows, S, n, planes, mall, resident, q0s;
};

// the lane's rows of the attention's segment: v, g, and G's S columns in registers (unused ones never read)
template <int HPL>
struct CrRows {
    float vv[HPL], gk[HPL], G0[HPL][CR_MAXS];
    unsigned long long m0, m1;
    __device__ __forceinline__ void load(const CrArgs &a, int lane)
    {
#pragma unroll
        for (int h = 0; h < HPL; ++h) {
            const int j = h * 64 + lane;
            vv[h] = a.v[j];
            gk[h] = a.g[j];
#pragma unroll
            for (int i = 0; i < CR_MAXS; ++i) G0[h][i] = i < a.S ? a.G[(size_t)j * a.S + i] : 0.f;
        }
        m0 = tap_rows_mask0(a.rows);
        m1 = tap_rows_mask1(a.rows);
    }

    // U[64 (h0 + i) + lane, c] of env b for i < R and every column c in ascending order, use(c, u) on each:
    // g, then the M columns of the set rows in ascending order (plane 0 before plane 1), then the S fmafs.  lw holds the
    // rows from slab h0 on at stride MS.  The next column's shadow words and x values are loaded before this column's
    // bit loop.
    template <int R, int H0, class F>
    __device__ __forceinline__ void sweep(const CrArgs &a, const float *lw, int MS, int b, int lane, F &&use) const
    {
        const int nR = a.nR, S = a.S;
        const unsigned long long *wp = a.bits + (size_t)b * (a.planes * nR);
        const float *xp = a.x + (size_t)b * S * nR;
        unsigned long long w0n = wp[0], w1n = a.planes == 2 ? wp[nR] : 0ull;
        float xn[CR_MAXS];
#pragma unroll
        for (int i = 0; i < CR_MAXS; ++i) xn[i] = i < S ? xp[i * nR] : 0.f;
        for (int c = 0; c < nR; ++c) {
            const unsigned long long w0 = w0n & m0, w1 = w1n & m1;
            float xv[CR_MAXS];
#pragma unroll
            for (int i = 0; i < CR_MAXS; ++i) xv[i] = xn[i];
            const int cn = min(c + 1, nR - 1);
            w0n = wp[cn];
            w1n = a.planes == 2 ? wp[nR + cn] : 0ull;
#pragma unroll
            for (int i = 0; i < CR_MAXS; ++i)
                if (i < S) xn[i] = xp[i * nR + cn];
            float u[R];
#pragma unroll
            for (int i = 0; i < R; ++i) u[i] = gk[H0 + i];
            // tap_add_set_rows' loop, written out: through the helper HPL = 4 takes 1 (forward) and 2 (backward) more VGPRs
            const unsigned piece[4] = {(unsigned)w0, (unsigned)(w0 >> 32), (unsigned)w1, (unsigned)(w1 >> 32)};
#pragma unroll
            for (int p = 0; p < 4; ++p) {                                  // ascending rows: plane 0 before plane 1
                unsigned y = (unsigned)__builtin_amdgcn_readfirstlane((int)piece[p]);
                while (y) {                                                // scalar: one trip per SET row
                    const int r = 32 * p + __builtin_ctz(y);
                    y &= y - 1;
                    const float *lp = lw + r * MS + lane;
#pragma unroll
                    for (int i = 0; i < R; ++i) u[i] = u[i] + lp[i * 64];
                }
            }
#pragma unroll
            for (int k = 0; k < CR_MAXS; ++k)
                if (k < S) {
#pragma unroll
                    for (int i = 0; i < R; ++i) u[i] = fmaf(G0[H0 + i][k], xv[k], u[i]);
                }
            use(c, u);
        }
    }
    // the same for ONE row per lane, of slab h (h is a constant after unrolling)
    template <class F>
    __device__ __forceinline__ void sweep1(int h, const CrArgs &a, const float *lw, int MS, int b, int lane, F &&use) const
    {
        if (h == 0) sweep<1, 0>(a, lw, MS, b, lane, use);
        else if (h == 1) sweep<1, (HPL > 1 ? 1 : 0)>(a, lw, MS, b, lane, use);
        else if (h == 2) sweep<1, (HPL > 2 ? 2 : 0)>(a, lw, MS, b, lane, use);
        else sweep<1, (HPL > 3 ? 3 : 0)>(a, lw, MS, b, lane, use);
    }
};

// rows [seg H + 64 h + lane] of (G, g) applied to S numbers: g, then one fmaf per k in ascending order
template <int HPL>
__device__ __forceinline__ void cr_affine(const CrArgs &a, int seg, const float (&xb)[CR_MAXS], int lane, float (&out)[HPL])
{
    constexpr int H = 64 * HPL;
#pragma unroll
    for (int h = 0; h < HPL; ++h) {
        const int j = seg * H + h * 64 + lane;
        float t = a.g[j];
#pragma unroll
        for (int k = 0; k < CR_MAXS; ++k)
            if (k < a.S) t = fmaf(a.G[(size_t)j * a.S + k], xb[k], t);
        out[h] = t;
    }
}

template <int HPL>
__global__ void __launch_bounds__(TAP_BLOCK) k_critic_value(CrArgs a)
{
    constexpr int H = 64 * HPL, US = H + 1;
    extern __shared__ float cr_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = TAP_WAVE_INDEX();
    const int nR = a.nR, S = a.S, n = a.n;
    const int MS = (a.mall ? H : 64) + 1;
    float *lw = cr_lds, *sl = lw + a.rows * MS + wave * nR;
    float *Ul = lw + a.rows * MS + CR_NW * nR + (size_t)wave * nR * US;   // (resident only)
    const int braw = (int)blockIdx.x * CR_NW + wave;
    const bool live = braw < a.B;                                         // wave-uniform
    const int b = live ? braw : a.B - 1;
    const float *xp = a.x + (size_t)b * S * nR;
    CrRows<HPL> rw;
    rw.load(a, lane);
    float qq[HPL];
#pragma unroll
    for (int h = 0; h < HPL; ++h) {
        qq[h] = a.q0[(size_t)b * a.q0s + h * 64 + lane];
        if (live) a.q[(size_t)b * n * H + h * 64 + lane] = qq[h];
    }
    if (a.mall) {
        tap_fill_chunk(a.M, lw, 0, H, H, a.rows, tid);
        __syncthreads();
    }
    float xb[CR_MAXS];
    for (int i = 0; i < n; ++i) {
        // s[c] = sum_j v[j] tanh(U[j, c] + q_i[j]) -> sl[c]
        if (a.resident && i > 0) {
            for (int c = 0; c < nR; ++c) {
                const float *up = Ul + c * US + lane;
                float p = rw.vv[0] * tanhf(up[0] + qq[0]);
#pragma unroll
                for (int h = 1; h < HPL; ++h) p = p + rw.vv[h] * tanhf(up[h * 64] + qq[h]);
                p = tap_wave_sum(p);
                if (lane == 0) sl[c] = p;
            }
        } else if (a.mall) {
            rw.template sweep<HPL, 0>(a, lw, MS, b, lane, [&](int c, float (&u)[HPL]) {
                if (a.resident) {
#pragma unroll
                    for (int h = 0; h < HPL; ++h) Ul[c * US + h * 64 + lane] = u[h];
                }
                float p = rw.vv[0] * tanhf(u[0] + qq[0]);
#pragma unroll
                for (int h = 1; h < HPL; ++h) p = p + rw.vv[h] * tanhf(u[h] + qq[h]);
                p = tap_wave_sum(p);
                if (lane == 0) sl[c] = p;
            });
        } else {
#pragma unroll
            for (int h = 0; h < HPL; ++h) {
                __syncthreads();                                           // the previous slab has been consumed
                tap_fill_chunk(a.M, lw, h * 64, 64, 64, a.rows, tid);
                __syncthreads();
                auto use = [&](int c, float (&u)[1]) {
                    if (a.resident) Ul[c * US + h * 64 + lane] = u[0];
                    const float p = tap_wave_sum(rw.vv[h] * tanhf(u[0] + qq[h]));
                    if (lane == 0) sl[c] = h == 0 ? p : sl[c] + p;
                };
                rw.sweep1(h, a, lw, MS, b, lane, use);
            }
        }
        tap_wave_lds_sync();
        // p_i = softmax over ALL nR columns, lanes along the columns
        float m = -INFINITY;
        for (int c = lane; c < nR; c += 64) m = fmaxf(m, sl[c]);
        m = tap_wave_max(m);
        float zs = 0.f;
        for (int c = lane; c < nR; c += 64) {
            const float e = expf(sl[c] - m);
            sl[c] = e;
            zs = zs + e;
        }
        zs = tap_wave_sum(zs);
        // xbar_i[k] = sum_c p_i[c] x[k, c]: a lane's own columns in order, then the butterfly
        float part[CR_MAXS];
#pragma unroll
        for (int k = 0; k < CR_MAXS; ++k) part[k] = 0.f;
        for (int c = lane; c < nR; c += 64) {
            const float pc = sl[c] / zs;
            if (live) a.p[((size_t)b * n + i) * nR + c] = pc;
#pragma unroll
            for (int k = 0; k < CR_MAXS; ++k)
                if (k < S) part[k] = part[k] + pc * xp[k * nR + c];
        }
#pragma unroll
        for (int k = 0; k < CR_MAXS; ++k) {
            xb[k] = 0.f;
            if (k < S) {
                xb[k] = tap_wave_sum(part[k]);
                if (live && lane == 0) a.xbar[((size_t)b * n + i) * S + k] = xb[k];
            }
        }
        tap_wave_lds_sync();                                                    // sl has been consumed
        if (i + 1 < n) {
            cr_affine<HPL>(a, 1, xb, lane, qq);
            if (live) {
#pragma unroll
                for (int h = 0; h < HPL; ++h) a.q[((size_t)b * n + i + 1) * H + h * 64 + lane] = qq[h];
            }
        }
    }
    // z = g2 + G2 . xbar; value = b2 + sum_j w2[j] max(z[j], 0)
    float zz[HPL];
    cr_affine<HPL>(a, 2, xb, lane, zz);
    float t = a.w2[lane] * fmaxf(zz[0], 0.f);
#pragma unroll
    for (int h = 1; h < HPL; ++h) t = t + a.w2[h * 64 + lane] * fmaxf(zz[h], 0.f);
    t = tap_wave_sum(t);
    if (live) {
#pragma unroll
        for (int h = 0; h < HPL; ++h) a.z[(size_t)b * H + h * 64 + lane] = zz[h];
        if (lane == 0) a.value[b] = a.b2[0] + t;
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------
template <int HPL>
__global__ void __launch_bounds__(TAP_BLOCK) k_critic_value_bw(CrArgs a)
{
    constexpr int H = 64 * HPL, US = H + 1;
    extern __shared__ float cr_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = TAP_WAVE_INDEX();
    const int nR = a.nR, S = a.S, n = a.n;
    const int MS = (a.mall ? H : 64) + 1;
    float *lw = cr_lds, *sl = lw + a.rows * MS + wave * nR, *dvl = lw + a.rows * MS + CR_NW * nR;
    float *Ul = dvl + CR_NW * H + (size_t)wave * nR * US;                 // (resident only) the env's dU, [c][j]
    const int braw = (int)blockIdx.x * CR_NW + wave;
    const bool live = braw < a.B;                                         // wave-uniform
    const int b = live ? braw : a.B - 1;
    const float *xp = a.x + (size_t)b * S * nR;
    float *dUg = a.dU + (size_t)b * H * nR;
    CrRows<HPL> rw;
    rw.load(a, lane);
    float dd[HPL], dv[HPL];                                               // dz, then the later block's dq; the env's dv
#pragma unroll
    for (int h = 0; h < HPL; ++h) {
        dd[h] = a.dz[(size_t)b * H + h * 64 + lane];
        dv[h] = 0.f;
    }
    if (a.mall) {
        tap_fill_chunk(a.M, lw, 0, H, H, a.rows, tid);
        __syncthreads();
    }
    for (int i = n - 1; i >= 0; --i) {
        const int seg = i == n - 1 ? 2 : 1;
        const float *pp = a.p + ((size_t)b * n + i) * nR;
        // dxbar_i[k] = sum_j G[seg H + j, k] d[j]: a lane's rows in order, then the butterfly
        float dx[CR_MAXS];
#pragma unroll
        for (int k = 0; k < CR_MAXS; ++k) {
            dx[k] = 0.f;
            if (k < S) {
                float t = a.G[(size_t)(seg * H + lane) * S + k] * dd[0];
#pragma unroll
                for (int h = 1; h < HPL; ++h) t = t + a.G[(size_t)(seg * H + h * 64 + lane) * S + k] * dd[h];
                dx[k] = tap_wave_sum(t);
            }
        }
        // dp[c] = sum_k dxbar[k] x[k, c]; ds = p (dp - sum_c p dp) -> sl[c], lanes along the columns
        float dot = 0.f;
        for (int c = lane; c < nR; c += 64) {
            float dp = 0.f;
#pragma unroll
            for (int k = 0; k < CR_MAXS; ++k)
                if (k < S) dp = dp + dx[k] * xp[k * nR + c];
            sl[c] = dp;
            dot = dot + pp[c] * dp;
        }
        dot = tap_wave_sum(dot);
        for (int c = lane; c < nR; c += 64) {
            const float ds = pp[c] * (sl[c] - dot);
            sl[c] = ds;
            if (!a.resident && live) a.dsg[((size_t)b * n + i) * nR + c] = ds;  // the second pass reads it
        }
        tap_wave_lds_sync();
        // the sweep: th = tanh(U + q_i); dv += ds th; dA = ds v (1 - th^2) -> dU; dq_i[j] = sum_c dA[j, c]
        float qq[HPL], dq[HPL];
#pragma unroll
        for (int h = 0; h < HPL; ++h) {
            qq[h] = a.q[((size_t)b * n + i) * H + h * 64 + lane];
            dq[h] = 0.f;
        }
        const bool first = i == n - 1;
        auto put = [&](int c, int h, float d) {                            // resident: dU[64 h + lane, c] (+)= d
            if (a.resident) {
                float *up = Ul + c * US + h * 64 + lane;
                *up = first ? d : *up + d;
            }
        };
        if (a.mall) {
            rw.template sweep<HPL, 0>(a, lw, MS, b, lane, [&](int c, float (&u)[HPL]) {
                const float ds = sl[c];
#pragma unroll
                for (int h = 0; h < HPL; ++h) {
                    const float th = tanhf(u[h] + qq[h]);
                    dv[h] = dv[h] + ds * th;
                    const float d = ds * rw.vv[h] * (1.f - th * th);
                    put(c, h, d);
                    dq[h] = dq[h] + d;
                }
            });
        } else {
#pragma unroll
            for (int h = 0; h < HPL; ++h) {
                __syncthreads();                                           // the previous slab has been consumed
                tap_fill_chunk(a.M, lw, h * 64, 64, 64, a.rows, tid);
                __syncthreads();
                auto use = [&](int c, float (&u)[1]) {
                    const float ds = sl[c];
                    const float th = tanhf(u[0] + qq[h]);
                    dv[h] = dv[h] + ds * th;
                    const float d = ds * rw.vv[h] * (1.f - th * th);
                    put(c, h, d);
                    dq[h] = dq[h] + d;
                };
                rw.sweep1(h, a, lw, MS, b, lane, use);
            }
        }
#pragma unroll
        for (int h = 0; h < HPL; ++h) {
            if (live) a.dq[((size_t)b * n + i) * H + h * 64 + lane] = dq[h];
            dd[h] = dq[h];
        }
        tap_wave_lds_sync();                                                    // sl has been consumed
    }
#pragma unroll
    for (int h = 0; h < HPL; ++h) dvl[wave * H + h * 64 + lane] = live ? dv[h] : 0.f;
    if (a.resident) {
        tap_wave_lds_sync();
        if (live) {
            // the env's dU, Ul[c * US + j], to dU_out[j * nR + c] as float4s: consecutive lanes consecutive 16-byte pieces
            const int q4 = nR >> 2;
            for (int idx = lane; idx < H * q4; idx += 64) {
                const int j = idx / q4, k4 = idx - j * q4;
                const float *up = Ul + (4 * k4) * US + j;
                *reinterpret_cast<float4 *>(dUg + (size_t)j * nR + 4 * k4) = make_float4(up[0], up[US], up[2 * US], up[3 * US]);
            }
        }
    }
    if (!a.resident) {
        // dU does not fit the LDS: a second sweep, columns outside and blocks inside -- U once per column, the blocks' dA
        // added in the first pass's (descending) order in registers -- so that dU_out is written ONCE, a float4 per lane
        // and four columns
        __syncthreads();                                                   // every block's ds has been written
        float qa[CR_MAXN][HPL];
#pragma unroll
        for (int i = 0; i < CR_MAXN; ++i)
#pragma unroll
            for (int h = 0; h < HPL; ++h) qa[i][h] = i < n ? a.q[((size_t)b * n + i) * H + h * 64 + lane] : 0.f;
        const float *dsp = a.dsg + (size_t)b * n * nR;
        auto col = [&](int c, int h, float u, float4 &acc) {
            float d = 0.f;
#pragma unroll
            for (int i = CR_MAXN - 1; i >= 0; --i)
                if (i < n) {
                    const float th = tanhf(u + qa[i][h]);
                    d = d + dsp[i * nR + c] * rw.vv[h] * (1.f - th * th);
                }
            const int k = c & 3;                                           // wave-uniform
            if (k == 0) acc.x = d;
            else if (k == 1) acc.y = d;
            else if (k == 2) acc.z = d;
            else {
                acc.w = d;
                if (live) *reinterpret_cast<float4 *>(dUg + (size_t)(h * 64 + lane) * nR + c - 3) = acc;
            }
        };
        if (a.mall) {
            float4 acc[HPL];
            rw.template sweep<HPL, 0>(a, lw, MS, b, lane, [&](int c, float (&u)[HPL]) {
#pragma unroll
                for (int h = 0; h < HPL; ++h) col(c, h, u[h], acc[h]);
            });
        } else {
#pragma unroll
            for (int h = 0; h < HPL; ++h) {
                __syncthreads();                                           // the previous slab has been consumed
                tap_fill_chunk(a.M, lw, h * 64, 64, 64, a.rows, tid);
                __syncthreads();
                float4 acc;
                rw.sweep1(h, a, lw, MS, b, lane, [&](int c, float (&u)[1]) { col(c, h, u[0], acc); });
            }
        }
    }
    __syncthreads();
    // this workgroup's dv: its wavefronts in order
    for (int j = tid; j < H; j += TAP_BLOCK) {
        float s = dvl[j];
#pragma unroll
        for (int w = 1; w < CR_NW; ++w) s = s + dvl[w * H + j];
        a.part[(size_t)blockIdx.x * H + j] = s;
    }
}

// dv[j] = part[0][j] + part[1][j] + ...: workgroup order, the same bytes every call (pointer.hip's reduce with one output;
// one kernel for both was tried and left: DESIGN 7f)
__global__ void __launch_bounds__(TAP_BLOCK) k_critic_value_bw_reduce(const float *part, int blocks, int H, float *dv)
{
    const int i = (int)blockIdx.x * TAP_BLOCK + (int)threadIdx.x;
    if (i >= H) return;
    float s = 0.f;
    for (int k0 = 0; k0 < blocks; k0 += 32) {                              // runs of 32, then the runs: shorter chains of roundings
        float p = 0.f;
        for (int k = k0; k < min(blocks, k0 + 32); ++k) p = p + part[(size_t)k * H + i];
        s = s + p;
    }
    dv[i] = s;
}

// the checks of both entries in the order of pointer.hip's ptr_check: dimensions, then the empty batch, then the caller's
// null check, then the shapes without a kernel
int cr_check_dims(tap_ctx *ctx, const char *what, int B, int nR, int rows, int H, int S, int n)
{
    if (B < 0 || nR < 1 || rows < 1 || H < 1 || S < 1 || n < 1)
        return tap_fail(ctx, TAP_E_INVALID, "%s: B %d, nR %d, rows %d, H %d, S %d, blocks %d", what, B, nR, rows, H, S, n);
    return TAP_OK;
}
inline bool cr_shape_ok(int nR, int rows, int H, int S, int n)
{
    return tap_has_bit_shadow(rows, nR) && (H == 64 || H == 128 || H == 256) && S <= CR_MAXS && n <= CR_MAXN;
}
int cr_check_shape(tap_ctx *ctx, const char *what, int nR, int rows, int H, int S, int n, int q0_stride)
{
    if (!cr_shape_ok(nR, rows, H, S, n) || (q0_stride != 0 && q0_stride != H))
        return tap_fail(ctx, TAP_E_UNSUPPORTED,
                        "%s: rows %d, nR %d, H %d, S %d, blocks %d, q0 stride %d (needs a bit shadow: rows <= 128, nR %% 4 == 0, "
                        "nR <= 256; H 64, 128 or 256; S <= 8; blocks <= 8; q0 stride 0 or H)", what, rows, nR, H, S, n, q0_stride);
    return TAP_OK;
}

template <class K1, class K2, class K4>
inline void cr_launch(int hpl, K1 k1, K2 k2, K4 k4, const CrGeom &geo, hipStream_t st, const CrArgs &a)
{
    if (hpl == 1) hipLaunchKernelGGL(k1, dim3((unsigned)geo.blocks), dim3(TAP_BLOCK), geo.lds, st, a);
    else if (hpl == 2) hipLaunchKernelGGL(k2, dim3((unsigned)geo.blocks), dim3(TAP_BLOCK), geo.lds, st, a);
    else hipLaunchKernelGGL(k4, dim3((unsigned)geo.blocks), dim3(TAP_BLOCK), geo.lds, st, a);
}

} // namespace

extern "C" int tap_critic_value(tap_ctx *ctx, const float *x, const unsigned long long *bits, int B, int nR, int rows, int H, int S,
                                int blocks, const float *G, const float *g, const float *M, const float *q0, int q0_stride,
                                const float *v, const float *w2, const float *b2, float *value_out, float *z_out, float *p_out,
                                float *xbar_out, float *q_out, void *stream)
{
    int rc = cr_check_dims(ctx, "critic value", B, nR, rows, H, S, blocks);
    if (rc != TAP_OK) return rc;
    if (B == 0) return TAP_OK; // an empty batch has no buffers to check
    if (!x || !bits || !G || !g || !M || !q0 || !v || !w2 || !b2 || !value_out || !z_out || !p_out || !xbar_out || !q_out)
        return tap_fail(ctx, TAP_E_INVALID, "critic value: null buffer");
    if ((rc = cr_check_shape(ctx, "critic value", nR, rows, H, S, blocks, q0_stride)) != TAP_OK) return rc;
    if (tap_misaligned(bits, 8) || tap_any_misaligned({x, G, g, M, q0, v, w2, b2, value_out, z_out, p_out, xbar_out, q_out}, 4))
        return tap_fail(ctx, TAP_E_INVALID, "critic value: bits must be 8-byte and the float buffers 4-byte aligned");
    const CrGeom geo = cr_geom(B, nR, rows, H, false);
    const CrArgs a = {x, bits, G, g, M, q0, v, w2, b2, value_out, z_out, p_out, xbar_out, q_out, nullptr, nullptr, nullptr, nullptr, nullptr,
                      B, nR, rows, S, blocks, geo.planes, geo.mall, geo.resident, q0_stride};
    cr_launch(geo.hpl, k_critic_value<1>, k_critic_value<2>, k_critic_value<4>, geo, (hipStream_t)stream, a);
    TAP_LAUNCH_CHECK(ctx, "k_critic_value");
    tap_variant_hit(ctx, TAP_HIT_CRITIC, geo.resident, geo.hpl, TapVariant{geo.planes, geo.mall, 0}, 0);
    return TAP_OK;
}

extern "C" size_t tap_critic_value_backward_scratch(int B, int nR, int rows, int H, int S, int blocks)
{
    if (B < 1 || nR < 1 || rows < 1 || H < 1 || S < 1 || blocks < 1 || !cr_shape_ok(nR, rows, H, S, blocks)) return 0;
    const CrGeom geo = cr_geom(B, nR, rows, H, true);                      // dv's partials, then every block's ds where dU is not resident
    return ((size_t)geo.blocks * (size_t)H + (geo.resident ? 0 : (size_t)B * blocks * nR)) * sizeof(float);
}

extern "C" int tap_critic_value_backward(tap_ctx *ctx, const float *x, const unsigned long long *bits, int B, int nR, int rows, int H,
                                         int S, int blocks, const float *G, const float *g, const float *M, const float *v,
                                         const float *q, const float *p, const float *dz, float *dU_out, float *dq_out,
                                         float *dv_out, void *scratch, size_t scratch_bytes, void *stream)
{
    int rc = cr_check_dims(ctx, "critic value backward", B, nR, rows, H, S, blocks);
    if (rc != TAP_OK) return rc;
    if (B == 0) return TAP_OK; // (an empty batch leaves the outputs as they are)
    if (!x || !bits || !G || !g || !M || !v || !q || !p || !dz || !dU_out || !dq_out || !dv_out)
        return tap_fail(ctx, TAP_E_INVALID, "critic value backward: null buffer");
    if ((rc = cr_check_shape(ctx, "critic value backward", nR, rows, H, S, blocks, 0)) != TAP_OK) return rc;
    const size_t need = tap_critic_value_backward_scratch(B, nR, rows, H, S, blocks);
    if (!scratch || scratch_bytes < need)
        return tap_fail(ctx, TAP_E_INVALID, "critic value backward: scratch of %zu bytes, %zu needed", scratch ? scratch_bytes : (size_t)0, need);
    if (tap_misaligned(bits, 8) || tap_misaligned(dU_out, 16) ||        // dU leaves as float4s
        tap_any_misaligned({x, G, g, M, v, q, p, dz, dU_out, dq_out, dv_out, scratch}, 4))
        return tap_fail(ctx, TAP_E_INVALID, "critic value backward: bits must be 8-byte, dU 16-byte and the other float buffers 4-byte aligned");
    const CrGeom geo = cr_geom(B, nR, rows, H, true);
    const CrArgs a = {x, bits, G, g, M, nullptr, v, nullptr, nullptr, nullptr, nullptr, const_cast<float *>(p), nullptr,
                      const_cast<float *>(q), dz, dU_out, dq_out, static_cast<float *>(scratch),
                      static_cast<float *>(scratch) + (size_t)geo.blocks * H, B, nR, rows, S, blocks, geo.planes, geo.mall, geo.resident, 0};
    hipStream_t st = (hipStream_t)stream;
    cr_launch(geo.hpl, k_critic_value_bw<1>, k_critic_value_bw<2>, k_critic_value_bw<4>, geo, st, a);
    TAP_LAUNCH_CHECK(ctx, "k_critic_value_bw");
    hipLaunchKernelGGL(k_critic_value_bw_reduce, dim3((unsigned)((H + TAP_BLOCK - 1) / TAP_BLOCK)), dim3(TAP_BLOCK), 0, st,
                       static_cast<const float *>(scratch), geo.blocks, H, dv_out);
    TAP_LAUNCH_CHECK(ctx, "k_critic_value_bw_reduce");
    tap_variant_hit(ctx, TAP_HIT_CRITIC, geo.resident, geo.hpl, TapVariant{geo.planes, geo.mall, 1}, 0);
    return TAP_OK;
}
