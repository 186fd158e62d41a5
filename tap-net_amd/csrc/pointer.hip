// pointer.hip -- the pointer network on the bit shadow: the reference's probs, last_hh = self.pointer(static_hidden,
// dynamic_hidden, decoder_hidden, last_hh) (model.py:356-358; classes Attention and Pointer, model.py:38-138) after its
// GRU step, with everything that does not depend on the step folded out of it (tapenv.h: tap_pointer_scores has the
// contract).  static_hidden is constant during an episode, so W's action on it is ONE projection per episode (`proj`);
// dynamic_hidden = conv.weight . bits + conv.bias with bits in {0, 1}, so W's action on it is the sum of a few columns
// of a small folded matrix M (3 Hd, rows) -- the scalar loop over set bits of encode.hip --; the context is a convex
// combination of columns and folds the same way.  A step then reads proj (3 Hd nR floats per env) and the shadow and
// writes nR logits per env: no dynamic_hidden, no concatenation, no GEMM.
//
// Geometry.  The 3 Hd rows of U = proj + k + M . bits are three independent segments -- 0: the attention's, 1: the
// pointer's, 2: the context's -- and each is needed in a phase of its own: s and the softmax from segment 0, then
// t = U2 . attn from segment 2, then the logits from segment 1 and t.  So every element of proj is read ONCE, by the
// phase that needs it, and proj is laid out segment-major, (B, 3, nR, Hd), hidden fastest: a wavefront takes a column,
// lanes along the hidden rows (HPL = 1 or 2 rows per lane, row = lane + 64 i), and each of its loads is 256 contiguous
// bytes; the loads of four of its columns are issued before the first column's bit loop and consumed after it.  The column's shadow word is wave-uniform; a lane's
// addend per set row is one conflict-free LDS read from an [r][x] copy of the segment's folded weights (row stride
// odd).  A workgroup (4 wavefronts) takes a run of consecutive envs, and the phases are its OUTER loops: the LDS holds
// one chunk (64 HPL hidden rows) of one segment of M at a time, filled once per phase and chunk for the whole run, so
// that M + the per-env vectors stay under 60 KB whatever the shape.  The per-column sums over the hidden rows are a
// lane's own terms in order, then an xor butterfly, then the chunks in order; the softmax over the columns is one
// wavefront per env; t adds the four wavefronts' column partials in wavefront order.  Every order is fixed by the
// shape: two calls give the same bytes.  No atomics.
//
// Backward: the same three phases in the order 1, 2, 0 (the gradient reaches the pointer's segment first, then t's,
// then the attention's), recomputing U, A and G; dU leaves in (B, 3 Hd, nR) -- the layout tap_encode_bits_backward
// takes as g, which then gives dM and dk -- through an LDS tile [hidden row][column] per env and pass of columns, stored
// as float4s like k_encode_bits' output; dva / dvp as one partial per workgroup in the caller's scratch, added in
// workgroup order by a second launch.
//
// The static-rows form (tapenv.h: tap_pointer_scores_static) is the same kernels with another source for the static term
// of U: static_hidden is a 1x1 convolution of the S = 1..8 rows xs of `static`, so proj[b, x, c] = g[x] + G[x, :] . xs[b, :, c]
// with G = Ws Es (3 Hd, S) and g = Ws bs -- S multiply-adds per element in place of a load (critic.hip computes its U this
// way).  PtrSeg's SS parameter chooses: PTR_PROJ loads proj; SS = 2, 3, 4 keeps a lane's HPL SS values of G in registers;
// SS = 0 takes any S <= 8 from an LDS copy [i][hidden] of the chunk's G.  xs[b, :, c] is wave-uniform and is loaded
// PTR_AHEAD columns ahead, where the proj form loads proj.  Everything after the static term -- the bit loop, the phases,
// every order of summation, the dU tile, the reduce -- is the proj form's code, so a proj that equals P bit for bit gives
// the same bytes.
#include <algorithm>

#include "tap_bitshadow.h"
#include "tap_common.h"
#include "tap_pick.h"

namespace {

constexpr int TAP_HIT_POINTER = 28; // launch record (tapenv.h: tap_variant_hits), after encode.hip's 27
constexpr int PTR_NW = TAP_BLOCK / 64;
constexpr int PTR_AHEAD = 4;                // columns whose proj loads a wavefront issues ahead
constexpr size_t PTR_LDS_BUDGET = 60 * 1024;

struct PtrGeom {
    int planes, hpl, hck, nch; // shadow planes; hidden rows per lane, per chunk; chunks per segment
    int epb, blocks;           // consecutive envs per workgroup; workgroups
    int ct;                    // backward: columns per pass of the dU tile, min(nR, 4096 / hck)
    size_t lds;                // bytes of dynamic LDS
};
constexpr int PTR_PROJ = -1;                 // PtrSeg's SS: the static term of U is loaded from proj
constexpr int PTR_SMAX = 8;                  // static rows of the static-rows form, as in critic.hip
inline int ptr_static_ss(int S) { return S >= 2 && S <= 4 ? S : 0; }      // the instantiation that takes S static rows
inline size_t ptr_lds_floats(int nR, int rows, int Hd, int hck, int epb, int ct, int gcopy = 0)
{
    // the folded weights of a chunk, s / attn / logits (or dattn / ds), the wavefronts' partials, t (or dt); the backward
    // adds (ct > 0) the dva / dvp partials and the dU tile of a pass; the static-rows form with SS = 0 its copy of a
    // chunk's G (gcopy = S hck)
    return (size_t)rows * (hck + 1) + (size_t)epb * nR + (size_t)PTR_NW * epb * hck + (size_t)epb * Hd +
           (ct ? (size_t)PTR_NW * hck + (size_t)hck * (ct + 1) : 0) + (size_t)gcopy;
}
// S = 0: the proj form; S >= 1: the static-rows form with S static rows
inline PtrGeom ptr_geom(int B, int nR, int rows, int Hd, bool backward, int S = 0)
{
    PtrGeom g;
    g.planes = tap_bit_planes(rows);
    g.hpl = (g.planes == 1 && Hd > 64) ? 2 : 1;
    g.hck = 64 * g.hpl;
    g.nch = Hd / g.hck;
    g.ct = backward ? std::min(nR, 4096 / g.hck) : 0;
    const int gcopy = S > 0 && ptr_static_ss(S) == 0 ? S * g.hck : 0;      // at most 4 KB
    g.epb = std::max(1, B / 1024);                                         // about four workgroups per CU before a second env
    while (g.epb > 1 && ptr_lds_floats(nR, rows, Hd, g.hck, g.epb, g.ct, gcopy) * sizeof(float) > PTR_LDS_BUDGET) g.epb >>= 1;
    g.blocks = (B + g.epb - 1) / g.epb;
    g.lds = ptr_lds_floats(nR, rows, Hd, g.hck, g.epb, g.ct, gcopy) * sizeof(float); // at most 60 KB: a lone env needs under 56 KB (+ gcopy: under 59 KB)
    return g;
}

struct PtrArgs {
    const float *proj;              // (B, 3, nR, Hd)
    const unsigned long long *bits; // (B, planes, nR)
    const float *M, *k;             // (3 Hd, rows), (3 Hd,)
    const float *q, *va, *vp;       // (B, Hd), (Hd,), (Hd,)
    float *logits, *attn, *t;       // (B, nR), (B, nR), (B, Hd): the forward's outputs, the backward's inputs (logits unused there)
    const float *g;                 // backward: (B, nR)
    float *dU, *dq, *part;          // backward: (B, 3 Hd, nR), (B, Hd), (blocks, 2, Hd)
    int B, nR, rows, Hd, planes, epb, ct;
};
// the static-rows form: proj is null; P = gs + Gs . xs takes its place
struct PtrArgsStatic : PtrArgs {
    const float *xs;                // (B, S, nR)
    const float *Gs, *gs;           // (3 Hd, S), (3 Hd,)
    int S;
};
// the fused form (tap_pointer_pick_static): the static-rows form with xs strided per env and the head's inputs and outputs.
// logits may be null; attn and t are not written
constexpr int PTR_NOPICK = 0, PTR_GREEDY = 1, PTR_DRAW = 2;   // the launch record's FORM field: the head's variant numbers
struct PtrArgsPick : PtrArgsStatic {
    size_t xs_env_stride;           // floats between consecutive envs of xs: >= S nR
    const float *mask;              // (B, nR)
    const long long *state;         // DRAW: int64[2] (seed, episode) on the device
    unsigned step, env_offset;      // DRAW
    int64_t *ptr;                   // (B,)
    float *logp;                    // (B,)
};

// the static term of U in the static-rows form: what a phase keeps of its chunk's G and g, a column's xs, and
// P[x0 + lane + 64 i, c] = g, then fmaf(G[., s], xs[b, s, c], .) for s ascending (tap_critic_value's order)
// (XST: env b's rows start at xs + b es instead of xs + b S nR -- the fused form's strided xs)
template <int HPL, int SS, bool XST = false>
struct PtrStat {
    static constexpr int HCK = 64 * HPL, NX = SS > 0 ? SS : PTR_SMAX;
    struct Xs { float x[NX]; };
    const float *xs, *G, *g;
    float *lg;                      // SS == 0: lg[s * HCK + hl] = G[x0 + hl][s]
    int S;
    size_t es;                      // XST only
    float gg[HPL], gw[HPL][SS > 0 ? SS : 1];

    template <class A> __device__ __forceinline__ void init(const A &a, float *lds_g)
    {
        xs = a.xs; G = a.Gs; g = a.gs; S = a.S; lg = lds_g;
        if constexpr (XST) es = a.xs_env_stride;
    }
    // between the caller's barriers, like PtrSeg::fill
    __device__ __forceinline__ void fill(int x0, int tid, int lane)
    {
#pragma unroll
        for (int i = 0; i < HPL; ++i) gg[i] = g[x0 + i * 64 + lane];
        if constexpr (SS > 0) {
#pragma unroll
            for (int i = 0; i < HPL; ++i)
#pragma unroll
                for (int s = 0; s < SS; ++s) gw[i][s] = G[(size_t)(x0 + i * 64 + lane) * SS + s];
        } else {
            for (int i = tid; i < HCK * S; i += TAP_BLOCK) {
                const int hl = i / S, s = i - hl * S;
                lg[s * HCK + hl] = G[(size_t)x0 * S + i];
            }
        }
    }
    __device__ __forceinline__ void load(int b, int nR, int c, Xs &x) const
    {
        const float *xp = xs + (XST ? (size_t)b * es : (size_t)b * S * nR) + c;
#pragma unroll
        for (int s = 0; s < NX; ++s) x.x[s] = (SS > 0 || s < S) ? xp[(size_t)s * nR] : 0.f;
    }
    __device__ __forceinline__ void term(int lane, float (&u)[HPL], const Xs &x) const
    {
#pragma unroll
        for (int i = 0; i < HPL; ++i) {
            float p = gg[i];
            if constexpr (SS > 0) {
#pragma unroll
                for (int s = 0; s < SS; ++s) p = fmaf(gw[i][s], x.x[s], p);
            } else {
#pragma unroll
                for (int s = 0; s < PTR_SMAX; ++s)
                    if (s < S) p = fmaf(lg[s * HCK + i * 64 + lane], x.x[s], p);   // wave-uniform
            }
            u[i] = p;
        }
    }
};
template <int HPL, bool XST>
struct PtrStat<HPL, PTR_PROJ, XST> { // the proj form keeps nothing
    struct Xs {};
    __device__ __forceinline__ void init(const PtrArgs &, float *) {}
    __device__ __forceinline__ void fill(int, int, int) {}
    __device__ __forceinline__ void term(int, float (&)[HPL], const Xs &) const {}
};

// what a phase keeps of its segment's chunk: the LDS copy of the folded weights and the lane's k (and, in the static-rows
// form, st)
template <int HPL, int SS = PTR_PROJ, bool XST = false>
struct PtrSeg {
    static constexpr int HCK = 64 * HPL, S = HCK + 1;
    using Xs = typename PtrStat<HPL, SS, XST>::Xs;
    const float *lw;
    float kk[HPL];
    unsigned long long m0, m1;
    PtrStat<HPL, SS, XST> st;

    // M[x0 + hl][r] -> lw[r * S + hl]: global reads in memory order, LDS writes at the odd stride S.  The caller's barriers
    // stand before (the previous chunk has been consumed) and after.
    __device__ void fill(const PtrArgs &a, float *lds, int seg, int ch, int tid, int lane)
    {
        const int x0 = seg * a.Hd + ch * HCK;
        tap_fill_chunk(a.M, lds, x0, HCK, HCK, a.rows, tid);
#pragma unroll
        for (int i = 0; i < HPL; ++i) kk[i] = a.k[x0 + i * 64 + lane];
        lw = lds;
        m0 = tap_rows_mask0(a.rows);
        m1 = tap_rows_mask1(a.rows);
        st.fill(x0, tid, lane);
    }

    // U[x0 + lane + 64 i, c] of env b = proj + (k + the M columns of the set rows, ascending), in two halves: load()
    // issues the loads of the column's shadow word(s) and proj values (static-rows form: the column's xs, and st.term()
    // makes P of them in proj's place), finish() runs the scalar loop over the set bits and adds its sum to proj
    __device__ __forceinline__ void load(const PtrArgs &a, int b, int seg, int ch, int c, int lane, float (&u)[HPL],
                                         unsigned long long (&w)[2], Xs &x) const
    {
        const unsigned long long *wp = a.bits + (size_t)b * (a.planes * a.nR);
        w[0] = wp[c];
        w[1] = a.planes == 2 ? wp[a.nR + c] : 0ull;
        if constexpr (SS == PTR_PROJ) {
            const float *pp = a.proj + (((size_t)b * 3 + seg) * a.nR + c) * a.Hd + ch * HCK + lane;
#pragma unroll
            for (int i = 0; i < HPL; ++i) u[i] = pp[i * 64];
        } else {
            st.load(b, a.nR, c, x);
        }
    }
    __device__ __forceinline__ void finish(int lane, float (&u)[HPL], const unsigned long long (&w)[2]) const
    {
        float acc[HPL];
#pragma unroll
        for (int i = 0; i < HPL; ++i) acc[i] = kk[i];
        tap_add_set_rows<HPL>(lw, S, lane, w[0] & m0, w[1] & m1, acc);
#pragma unroll
        for (int i = 0; i < HPL; ++i) u[i] = u[i] + acc[i];
    }

    // the wavefront's columns of env b in [cbeg, cend) (cbeg + wave, + 4, ...) in ascending order, use(c, u) on each.  The proj loads of
    // PTR_AHEAD columns are issued before the first of them is consumed: a wavefront alone keeps 256 HPL PTR_AHEAD
    // bytes in flight (one column at a time left the step waiting on memory latency, not bandwidth: DESIGN 7f)
    template <class F>
    __device__ __forceinline__ void columns(const PtrArgs &a, int b, int seg, int ch, int cbeg, int cend, int wave, int lane,
                                            F &&use) const
    {
        for (int c0 = cbeg + wave; c0 < cend; c0 += PTR_NW * PTR_AHEAD) {
            float u[PTR_AHEAD][HPL];
            unsigned long long w[PTR_AHEAD][2];
            Xs xv[PTR_AHEAD];
#pragma unroll
            for (int j = 0; j < PTR_AHEAD; ++j) load(a, b, seg, ch, min(c0 + j * PTR_NW, cend - 1), lane, u[j], w[j], xv[j]);
#pragma unroll
            for (int j = 0; j < PTR_AHEAD; ++j) {
                const int c = c0 + j * PTR_NW;
                if (c < cend) {                                            // wave-uniform
                    st.term(lane, u[j], xv[j]);
                    finish(lane, u[j], w[j]);
                    use(c, u[j]);
                }
            }
        }
    }
};

// the four wavefronts' partials tp[(wave * E + e) * HCK + jl], added in wavefront order
__device__ __forceinline__ float ptr_add_waves(const float *tp, int E, int HCK, int e, int jl)
{
    float v = tp[(size_t)e * HCK + jl];
#pragma unroll
    for (int w = 1; w < PTR_NW; ++w) v = v + tp[((size_t)w * E + e) * HCK + jl];
    return v;
}

// the head on a row of logits in the LDS, by one wavefront: k_policy_pick_wide<true> (PTR_GREEDY) / k_policy_pick_wide_form<2>
// (PTR_DRAW) without probs -- the max pass, the weight pass for S (and the greedy pick), DRAW's second weight pass --, the row
// read from lrow where those read global memory.  On rows of at most 64 columns the lane-group kernels write the same bytes
// (tapenv.h: tap_pointer_pick_static)
template <int FORM>
__device__ __forceinline__ void ptr_pick_row(const PtrArgsPick &a, const float *lrow, size_t env, int lane)
{
    const int nR = a.nR;
    const float *mrow = a.mask + env * nR;
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
        if (FORM == PTR_GREEDY && p < 0) {
            const u64 q = __ballot(c.sel && c.l == m);
            if (q) p = base + __ffsll((long long)q) - 1;
        }
    }
    if (FORM == PTR_DRAW) {                                     // the weight pass again, for the pick
        const double t = (double)draw_uniform(a, env) * S;
        double run = 0.0;
        int last = 0;
        for (int base = 0; base < nR; base += 64) {
            const Chunk c = pick_chunk(lrow, mrow, base, lane, nR, m, run);
            const u64 q = __ballot(c.sel && c.cum > t), sb = __ballot(c.sel);
            if (p < 0 && q) p = base + __ffsll((long long)q) - 1;   // the first chunk with a qualifying column decides
            if (sb) last = base + 63 - __clzll((long long)sb);
            if (p >= 0) break;                                  // wave-uniform
        }
        if (p < 0) p = last;                                    // t >= S: the last selectable column (0 on an empty row)
    }
    if (p < 0) p = 0;
    const float l_ptr = lrow[p];
    if (lane == 0) {
        a.ptr[env] = p;
        a.logp[env] = pick_logp(any, l_ptr, m, S);
    }
}

// every forward form.  FORM = PTR_NOPICK: tap_pointer_scores / _static -- A is PtrArgs (SS = PTR_PROJ, the proj form) or
// PtrArgsStatic (SS = 0, 2, 3, 4).  FORM = PTR_GREEDY / PTR_DRAW: the fused form (A = PtrArgsPick, tap_pointer_pick_static) --
// xs strided, attn and t stay in the LDS, and the head runs on the LDS row of logits where the others store it
template <int HPL, int SS = PTR_PROJ, class A = PtrArgs, int FORM = PTR_NOPICK>
__global__ void __launch_bounds__(TAP_BLOCK) k_pointer_scores(A a)
{
    constexpr int HCK = 64 * HPL, S = HCK + 1;
    constexpr bool PICK = FORM != PTR_NOPICK;
    extern __shared__ float ptr_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = TAP_WAVE_INDEX();
    const int nR = a.nR, Hd = a.Hd, E = a.epb, nch = Hd / HCK;
    float *lw = ptr_lds, *sl = lw + a.rows * S, *tp = sl + E * nR, *tl = tp + PTR_NW * E * HCK;
    const int e0 = (int)blockIdx.x * E, ne = min(E, a.B - e0);
    PtrSeg<HPL, SS, PICK> sg;
    sg.st.init(a, tl + E * Hd);

    // phase 1, segment 0: s[c] = sum_j va[j] tanh(U[j, c] + q[j]) -> sl[e][c]
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();
        sg.fill(a, lw, 0, ch, tid, lane);
        float vv[HPL];
#pragma unroll
        for (int i = 0; i < HPL; ++i) vv[i] = a.va[ch * HCK + i * 64 + lane];
        __syncthreads();
        for (int e = 0; e < ne; ++e) {
            float qq[HPL];
#pragma unroll
            for (int i = 0; i < HPL; ++i) qq[i] = a.q[(size_t)(e0 + e) * Hd + ch * HCK + i * 64 + lane];
            sg.columns(a, e0 + e, 0, ch, 0, nR, wave, lane, [&](int c, float (&u)[HPL]) {
                float p = vv[0] * tanhf(u[0] + qq[0]);
#pragma unroll
                for (int i = 1; i < HPL; ++i) p = p + vv[i] * tanhf(u[i] + qq[i]);
                p = tap_wave_sum(p);
                if (lane == 0) sl[e * nR + c] = ch == 0 ? p : sl[e * nR + c] + p;
            });
        }
    }
    __syncthreads();
    // attn = softmax over ALL nR columns: a wavefront per env, lanes along the columns
    for (int e = wave; e < ne; e += PTR_NW) {
        float m = -INFINITY;
        for (int c = lane; c < nR; c += 64) m = fmaxf(m, sl[e * nR + c]);
        m = tap_wave_max(m);
        float z = 0.f;
        for (int c = lane; c < nR; c += 64) {
            const float x = expf(sl[e * nR + c] - m);
            sl[e * nR + c] = x;
            z = z + x;
        }
        z = tap_wave_sum(z);
        for (int c = lane; c < nR; c += 64) {
            const float x = sl[e * nR + c] / z;
            sl[e * nR + c] = x;
            if constexpr (!PICK) a.attn[(size_t)(e0 + e) * nR + c] = x;
        }
    }
    // phase 2, segment 2: t[j] = sum_c attn[c] U[2 Hd + j, c] -> tl[e][j]
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();                                                   // (the first one publishes attn)
        sg.fill(a, lw, 2, ch, tid, lane);
        __syncthreads();
        for (int e = 0; e < ne; ++e) {
            float tw[HPL];
#pragma unroll
            for (int i = 0; i < HPL; ++i) tw[i] = 0.f;
            sg.columns(a, e0 + e, 2, ch, 0, nR, wave, lane, [&](int c, float (&u)[HPL]) {
                const float at = sl[e * nR + c];
#pragma unroll
                for (int i = 0; i < HPL; ++i) tw[i] = tw[i] + at * u[i];
            });
#pragma unroll
            for (int i = 0; i < HPL; ++i) tp[(wave * E + e) * HCK + i * 64 + lane] = tw[i];
        }
        __syncthreads();
        for (int i = tid; i < ne * HCK; i += TAP_BLOCK) {
            const int e = i / HCK, jl = i - e * HCK;
            const float v = ptr_add_waves(tp, E, HCK, e, jl);
            tl[e * Hd + ch * HCK + jl] = v;
            if constexpr (!PICK) a.t[(size_t)(e0 + e) * Hd + ch * HCK + jl] = v;
        }
    }
    // phase 3, segment 1: logits[c] = sum_j vp[j] tanh(U[Hd + j, c] + t[j]) -> sl[e][c] (attn has been consumed)
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();
        sg.fill(a, lw, 1, ch, tid, lane);
        float vv[HPL];
#pragma unroll
        for (int i = 0; i < HPL; ++i) vv[i] = a.vp[ch * HCK + i * 64 + lane];
        __syncthreads();
        for (int e = 0; e < ne; ++e) {
            float tt[HPL];
#pragma unroll
            for (int i = 0; i < HPL; ++i) tt[i] = tl[e * Hd + ch * HCK + i * 64 + lane];
            sg.columns(a, e0 + e, 1, ch, 0, nR, wave, lane, [&](int c, float (&u)[HPL]) {
                float p = vv[0] * tanhf(u[0] + tt[0]);
#pragma unroll
                for (int i = 1; i < HPL; ++i) p = p + vv[i] * tanhf(u[i] + tt[i]);
                p = tap_wave_sum(p);
                if (lane == 0) sl[e * nR + c] = ch == 0 ? p : sl[e * nR + c] + p;
            });
        }
    }
    __syncthreads();
    if constexpr (!PICK) {
        for (int i = tid; i < ne * nR; i += TAP_BLOCK) a.logits[(size_t)e0 * nR + i] = sl[i];
    } else {
        if (a.logits)
            for (int i = tid; i < ne * nR; i += TAP_BLOCK) a.logits[(size_t)e0 * nR + i] = sl[i];
        // the head: a wavefront per env, as the softmax above (sl is only read from here on)
        for (int e = wave; e < ne; e += PTR_NW) ptr_pick_row<FORM>(a, sl + e * nR, (size_t)(e0 + e), lane);
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------
// the backward's dU tile of a pass, tile[hl * TS + column] (TS odd: the wavefronts' writes, lanes along hl, are
// conflict-free), to dst[hl * nR + column] as float4s, consecutive threads consecutive 16-byte pieces; ncol % 4 == 0.
// A barrier before (the tile is complete) and after (the next pass may overwrite it).
__device__ __forceinline__ void ptr_store_tile(const float *tile, int TS, int ncol, int HCK, float *dst, int nR, int tid)
{
    __syncthreads();
    const int q4 = ncol >> 2, total = HCK * q4;
    for (int j = tid; j < total; j += TAP_BLOCK) {
        const int hl = j / q4, k4 = j - hl * q4;
        const float *t = tile + hl * TS + 4 * k4;
        *reinterpret_cast<float4 *>(dst + (size_t)hl * nR + 4 * k4) = make_float4(t[0], t[1], t[2], t[3]);
    }
    __syncthreads();
}

template <int HPL, int SS = PTR_PROJ, class A = PtrArgs>
__global__ void __launch_bounds__(TAP_BLOCK) k_pointer_scores_bw(A a)
{
    constexpr int HCK = 64 * HPL, S = HCK + 1;
    extern __shared__ float ptr_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = TAP_WAVE_INDEX();
    const int nR = a.nR, Hd = a.Hd, E = a.epb, nch = Hd / HCK;
    float *lw = ptr_lds, *dl = lw + a.rows * S, *tp = dl + E * nR, *dtl = tp + PTR_NW * E * HCK, *vp4 = dtl + E * Hd;
    float *tile = vp4 + PTR_NW * HCK;
    const int CT = a.ct, TS = CT + 1;                                      // columns per pass of the dU tile
    const int e0 = (int)blockIdx.x * E, ne = min(E, a.B - e0);
    float *part = a.part + (size_t)blockIdx.x * 2 * Hd;                    // this workgroup's dva (Hd), then dvp (Hd)
    PtrSeg<HPL, SS> sg;
    sg.st.init(a, tile + HCK * TS);

    // phase 1, segment 1: G = U + t; dvp += g tanh(G); dG = g vp (1 - tanh^2) = dU[Hd + j]; dt[j] = sum_c dG[j, c]
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();
        sg.fill(a, lw, 1, ch, tid, lane);
        float vv[HPL], dv[HPL];
#pragma unroll
        for (int i = 0; i < HPL; ++i) { vv[i] = a.vp[ch * HCK + i * 64 + lane]; dv[i] = 0.f; }
        __syncthreads();
        for (int e = 0; e < ne; ++e) {
            const int b = e0 + e;
            float tt[HPL], dw[HPL];
#pragma unroll
            for (int i = 0; i < HPL; ++i) { tt[i] = a.t[(size_t)b * Hd + ch * HCK + i * 64 + lane]; dw[i] = 0.f; }
            for (int cb = 0; cb < nR; cb += CT) {
                const int ncol = min(CT, nR - cb);
                sg.columns(a, b, 1, ch, cb, cb + ncol, wave, lane, [&](int c, float (&u)[HPL]) {
                    const float gc = a.g[(size_t)b * nR + c];
#pragma unroll
                    for (int i = 0; i < HPL; ++i) {
                        const float th = tanhf(u[i] + tt[i]);
                        dv[i] = dv[i] + gc * th;
                        const float d = gc * vv[i] * (1.f - th * th);
                        tile[(i * 64 + lane) * TS + c - cb] = d;
                        dw[i] = dw[i] + d;
                    }
                });
                ptr_store_tile(tile, TS, ncol, HCK, a.dU + ((size_t)b * 3 * Hd + Hd + ch * HCK) * nR + cb, nR, tid);
            }
#pragma unroll
            for (int i = 0; i < HPL; ++i) tp[(wave * E + e) * HCK + i * 64 + lane] = dw[i];
        }
#pragma unroll
        for (int i = 0; i < HPL; ++i) vp4[wave * HCK + i * 64 + lane] = dv[i];
        __syncthreads();
        for (int i = tid; i < ne * HCK; i += TAP_BLOCK) {
            const int e = i / HCK, jl = i - e * HCK;
            dtl[e * Hd + ch * HCK + jl] = ptr_add_waves(tp, E, HCK, e, jl);
        }
        for (int jl = tid; jl < HCK; jl += TAP_BLOCK) part[Hd + ch * HCK + jl] = ptr_add_waves(vp4, 1, HCK, 0, jl);
    }
    // phase 2, segment 2: dU[2 Hd + j, c] = attn[c] dt[j]; dattn[c] = sum_j dt[j] U[2 Hd + j, c] -> dl[e][c]
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();                                                   // (the first one publishes dt)
        sg.fill(a, lw, 2, ch, tid, lane);
        __syncthreads();
        for (int e = 0; e < ne; ++e) {
            const int b = e0 + e;
            float dt[HPL];
#pragma unroll
            for (int i = 0; i < HPL; ++i) dt[i] = dtl[e * Hd + ch * HCK + i * 64 + lane];
            for (int cb = 0; cb < nR; cb += CT) {
                const int ncol = min(CT, nR - cb);
                sg.columns(a, b, 2, ch, cb, cb + ncol, wave, lane, [&](int c, float (&u)[HPL]) {
                    const float at = a.attn[(size_t)b * nR + c];
                    float p = dt[0] * u[0];
#pragma unroll
                    for (int i = 1; i < HPL; ++i) p = p + dt[i] * u[i];
#pragma unroll
                    for (int i = 0; i < HPL; ++i) tile[(i * 64 + lane) * TS + c - cb] = at * dt[i];
                    p = tap_wave_sum(p);
                    if (lane == 0) dl[e * nR + c] = ch == 0 ? p : dl[e * nR + c] + p;
                });
                ptr_store_tile(tile, TS, ncol, HCK, a.dU + ((size_t)b * 3 * Hd + 2 * Hd + ch * HCK) * nR + cb, nR, tid);
            }
        }
    }
    __syncthreads();
    // the softmax: ds[c] = attn[c] (dattn[c] - sum_c' attn[c'] dattn[c']), a wavefront per env
    for (int e = wave; e < ne; e += PTR_NW) {
        const float *at = a.attn + (size_t)(e0 + e) * nR;
        float z = 0.f;
        for (int c = lane; c < nR; c += 64) z = z + at[c] * dl[e * nR + c];
        z = tap_wave_sum(z);
        for (int c = lane; c < nR; c += 64) dl[e * nR + c] = at[c] * (dl[e * nR + c] - z);
    }
    // phase 3, segment 0: A = U + q; dva += ds tanh(A); dA = ds va (1 - tanh^2) = dU[j]; dq[j] = sum_c dA[j, c]
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();                                                   // (the first one publishes ds)
        sg.fill(a, lw, 0, ch, tid, lane);
        float vv[HPL], dv[HPL];
#pragma unroll
        for (int i = 0; i < HPL; ++i) { vv[i] = a.va[ch * HCK + i * 64 + lane]; dv[i] = 0.f; }
        __syncthreads();
        for (int e = 0; e < ne; ++e) {
            const int b = e0 + e;
            float qq[HPL], dw[HPL];
#pragma unroll
            for (int i = 0; i < HPL; ++i) { qq[i] = a.q[(size_t)b * Hd + ch * HCK + i * 64 + lane]; dw[i] = 0.f; }
            for (int cb = 0; cb < nR; cb += CT) {
                const int ncol = min(CT, nR - cb);
                sg.columns(a, b, 0, ch, cb, cb + ncol, wave, lane, [&](int c, float (&u)[HPL]) {
                    const float ds = dl[e * nR + c];
#pragma unroll
                    for (int i = 0; i < HPL; ++i) {
                        const float th = tanhf(u[i] + qq[i]);
                        dv[i] = dv[i] + ds * th;
                        const float d = ds * vv[i] * (1.f - th * th);
                        tile[(i * 64 + lane) * TS + c - cb] = d;
                        dw[i] = dw[i] + d;
                    }
                });
                ptr_store_tile(tile, TS, ncol, HCK, a.dU + ((size_t)b * 3 * Hd + ch * HCK) * nR + cb, nR, tid);
            }
#pragma unroll
            for (int i = 0; i < HPL; ++i) tp[(wave * E + e) * HCK + i * 64 + lane] = dw[i];
        }
#pragma unroll
        for (int i = 0; i < HPL; ++i) vp4[wave * HCK + i * 64 + lane] = dv[i];
        __syncthreads();
        for (int i = tid; i < ne * HCK; i += TAP_BLOCK) {
            const int e = i / HCK, jl = i - e * HCK;
            a.dq[(size_t)(e0 + e) * Hd + ch * HCK + jl] = ptr_add_waves(tp, E, HCK, e, jl);
        }
        for (int jl = tid; jl < HCK; jl += TAP_BLOCK) part[ch * HCK + jl] = ptr_add_waves(vp4, 1, HCK, 0, jl);
    }
}

// dva[j] = part[0][0][j] + part[1][0][j] + ..., dvp likewise: workgroup order, the same bytes every call
__global__ void __launch_bounds__(TAP_BLOCK) k_pointer_scores_bw_reduce(const float *part, int blocks, int Hd, float *dva, float *dvp)
{
    const int i = (int)blockIdx.x * TAP_BLOCK + (int)threadIdx.x;
    if (i >= 2 * Hd) return;
    float s = 0.f;
    for (int k0 = 0; k0 < blocks; k0 += 32) {                              // runs of 32, then the runs: shorter chains of roundings
        float p = 0.f;
        for (int k = k0; k < min(blocks, k0 + 32); ++k) p = p + part[(size_t)k * 2 * Hd + i];
        s = s + p;
    }
    if (i < Hd) dva[i] = s;
    else dvp[i - Hd] = s;
}

// ---- host ----------------------------------------------------------------------------------------------------------
// one call of the family, as its five entries describe it: the name in messages, which entry (the proj form has no S),
// the dimensions, and which kernel: the forward (form = PTR_NOPICK, or the pick's PTR_GREEDY / PTR_DRAW) or the backward
enum PtrKind { PTR_K_PROJ, PTR_K_STATIC, PTR_K_PICK };
struct PtrCall {
    const char *what;
    PtrKind kind;
    int B, nR, rows, Hd, S;         // S = 0 in the proj form
    bool backward;
    int form;
};
inline bool ptr_shape_ok(int nR, int rows, int Hd) { return tap_has_bit_shadow(rows, nR) && (Hd == 64 || Hd == 128 || Hd == 256); }
inline PtrGeom ptr_geom(const PtrCall &c) { return ptr_geom(c.B, c.nR, c.rows, c.Hd, c.backward, c.S); }
inline size_t ptr_scratch_bytes(int B, int nR, int rows, int Hd, int S)   // the backward's dva / dvp partials
{
    return (size_t)ptr_geom(B, nR, rows, Hd, true, S).blocks * 2 * (size_t)Hd * sizeof(float);
}

// the checks of all five entries, in tap_policy_pick's order: dimensions (the pick: and its form), then the empty batch --
// TAP_OK, and the entry returns --, then the null check of `need`, the entry's own `extra` checks, the shapes without a
// kernel, the backward's scratch, and the alignment of the a4 / a8 / a16 lists (a null optional buffer is aligned)
template <class Extra>
int ptr_check(tap_ctx *ctx, const PtrCall &c, TapPtrList need, TapPtrList a4, TapPtrList a8, TapPtrList a16, const void *scratch, size_t scratch_bytes,
              Extra &&extra)
{
    const bool proj = c.kind == PTR_K_PROJ;
    if (c.B < 0 || c.nR < 1 || c.rows < 1 || c.Hd < 1 || (!proj && c.S < 1))
        return proj ? tap_fail(ctx, TAP_E_INVALID, "%s: B %d, nR %d, rows %d, Hd %d", c.what, c.B, c.nR, c.rows, c.Hd)
                    : tap_fail(ctx, TAP_E_INVALID, "%s: B %d, nR %d, rows %d, Hd %d, S %d", c.what, c.B, c.nR, c.rows, c.Hd, c.S);
    if (c.kind == PTR_K_PICK && c.form != PTR_GREEDY && c.form != PTR_DRAW) return tap_fail(ctx, TAP_E_INVALID, "%s: form %d", c.what, c.form);
    if (c.B == 0) return TAP_OK; // an empty batch has no buffers to check (and leaves a backward's outputs as they are)
    for (const void *p : need)
        if (!p) return tap_fail(ctx, TAP_E_INVALID, "%s: null buffer", c.what);
    if (const int rc = extra(); rc != TAP_OK) return rc;
    if (!ptr_shape_ok(c.nR, c.rows, c.Hd) || c.S > PTR_SMAX)
        return proj ? tap_fail(ctx, TAP_E_UNSUPPORTED, "%s: rows %d, nR %d, Hd %d (needs a bit shadow: rows <= 128, nR %% 4 == 0, nR <= 256; Hd 64, 128 or 256)",
                               c.what, c.rows, c.nR, c.Hd)
                    : tap_fail(ctx, TAP_E_UNSUPPORTED, "%s: rows %d, nR %d, Hd %d, S %d (needs a bit shadow: rows <= 128, nR %% 4 == 0, nR <= 256; Hd 64, 128 or 256; S <= 8)",
                               c.what, c.rows, c.nR, c.Hd, c.S);
    if (c.backward) {
        const size_t have = scratch ? scratch_bytes : (size_t)0, needed = ptr_scratch_bytes(c.B, c.nR, c.rows, c.Hd, c.S);
        if (!scratch || have < needed) return tap_fail(ctx, TAP_E_INVALID, "%s: scratch of %zu bytes, %zu needed", c.what, have, needed);
    }
    if (tap_any_misaligned(a4, 4) || tap_any_misaligned(a8, 8) || tap_any_misaligned(a16, 16)) {
        const char *rule = c.backward ? "bits must be 8-byte, dU 16-byte and the other float buffers 4-byte aligned" // dU leaves as float4s
                           : c.kind == PTR_K_PICK ? "bits and ptr_out must be 8-byte and the float buffers 4-byte aligned"
                                                  : "bits must be 8-byte and the float buffers 4-byte aligned";
        return tap_fail(ctx, TAP_E_INVALID, "%s: %s", c.what, rule);
    }
    return TAP_OK;
}
inline int ptr_check(tap_ctx *ctx, const PtrCall &c, TapPtrList need, TapPtrList a4, TapPtrList a8, TapPtrList a16, const void *scratch = nullptr,
                     size_t scratch_bytes = 0)
{
    return ptr_check(ctx, c, need, a4, a8, a16, scratch, scratch_bytes, [] { return TAP_OK; });
}

// what every form's kernel takes, by name; the entry adds its own fields (everything else stays null / 0)
template <class A>
A ptr_args(const PtrCall &c, const PtrGeom &geo, const unsigned long long *bits, const float *M, const float *k, const float *q,
           const float *va, const float *vp)
{
    A a{};
    a.bits = bits; a.M = M; a.k = k; a.q = q; a.va = va; a.vp = vp;
    a.B = c.B; a.nR = c.nR; a.rows = c.rows; a.Hd = c.Hd;
    a.planes = geo.planes; a.epb = geo.epb; a.ct = geo.ct;
    return a;
}

// the launch of the instantiation (HPL, SS) of the forward k_pointer_scores<., ., A, FORM> or the backward: HPL from the
// geometry; SS = PTR_PROJ with PtrArgs, else the static rows' 0, 2, 3 or 4
template <int V> using PtrInt = std::integral_constant<int, V>;
template <class A, int FORM = PTR_NOPICK, bool BW = false>
void ptr_launch(const PtrGeom &geo, hipStream_t st, const A &a)
{
    auto one = [&](auto hpl, auto ss) {
        constexpr int HPL = decltype(hpl)::value, SS = decltype(ss)::value;
        const dim3 grid((unsigned)geo.blocks), block(TAP_BLOCK);
        if constexpr (BW) hipLaunchKernelGGL((k_pointer_scores_bw<HPL, SS, A>), grid, block, geo.lds, st, a);
        else hipLaunchKernelGGL((k_pointer_scores<HPL, SS, A, FORM>), grid, block, geo.lds, st, a);
    };
    auto with = [&](auto ss) {
        if (geo.hpl == 1) one(PtrInt<1>{}, ss);
        else one(PtrInt<2>{}, ss);
    };
    if constexpr (std::is_same_v<A, PtrArgs>) with(PtrInt<PTR_PROJ>{});
    else
        switch (ptr_static_ss(a.S)) {
        case 2: with(PtrInt<2>{}); break;
        case 3: with(PtrInt<3>{}); break;
        case 4: with(PtrInt<4>{}); break;
        default: with(PtrInt<0>{}); break;
        }
}

// the launch record (tapenv.h: tap_variant_hits): (28, FORM, HPL, PLANES, NCH, BACKWARD, S) -- with S = 0 what tap_variant_hit
// makes of TapVariant{planes, nch, backward} and wt = 0
void ptr_hit(tap_ctx *ctx, const PtrGeom &geo, const PtrCall &c)
{
    const int32_t key[7] = {TAP_HIT_POINTER, c.form, geo.hpl, geo.planes, geo.nch, c.backward ? 1 : 0, c.S};
    tap_variant_hit_key(ctx, key);
}

// a checked call: the launch, the backward's second launch (dva | dvp from the workgroups' partials), the record
template <class A, int FORM = PTR_NOPICK, bool BW = false>
int ptr_run(tap_ctx *ctx, const PtrCall &c, const PtrGeom &geo, const A &a, void *stream, float *dva = nullptr, float *dvp = nullptr)
{
    static const char *const fw[] = {"k_pointer_scores", "k_pointer_scores (static rows)", "k_pointer_scores (pick)"};
    static const char *const bw[] = {"k_pointer_scores_bw", "k_pointer_scores_bw (static rows)"};
    hipStream_t st = (hipStream_t)stream;
    ptr_launch<A, FORM, BW>(geo, st, a);
    TAP_LAUNCH_CHECK(ctx, (BW ? bw : fw)[c.kind]);
    if constexpr (BW) {
        hipLaunchKernelGGL(k_pointer_scores_bw_reduce, dim3((unsigned)((2 * c.Hd + TAP_BLOCK - 1) / TAP_BLOCK)), dim3(TAP_BLOCK), 0, st,
                           static_cast<const float *>(a.part), geo.blocks, c.Hd, dva, dvp);
        TAP_LAUNCH_CHECK(ctx, "k_pointer_scores_bw_reduce");
    }
    ptr_hit(ctx, geo, c);
    return TAP_OK;
}

} // namespace

extern "C" int tap_pointer_scores(tap_ctx *ctx, const float *proj, const unsigned long long *bits, int B, int nR, int rows, int Hd,
                                  const float *M, const float *k, const float *q, const float *va, const float *vp,
                                  float *logits_out, float *attn_out, float *t_out, void *stream)
{
    const PtrCall c = {"pointer scores", PTR_K_PROJ, B, nR, rows, Hd, 0, false, PTR_NOPICK};
    const int rc = ptr_check(ctx, c, {proj, bits, M, k, q, va, vp, logits_out, attn_out, t_out},
                             {proj, M, k, q, va, vp, logits_out, attn_out, t_out}, {bits}, {});
    if (rc != TAP_OK || B == 0) return rc;
    const PtrGeom geo = ptr_geom(c);
    PtrArgs a = ptr_args<PtrArgs>(c, geo, bits, M, k, q, va, vp);
    a.proj = proj;
    a.logits = logits_out; a.attn = attn_out; a.t = t_out;
    return ptr_run(ctx, c, geo, a, stream);
}

extern "C" size_t tap_pointer_scores_backward_scratch(int B, int nR, int rows, int Hd)
{
    if (B < 1 || nR < 1 || rows < 1 || Hd < 1 || !ptr_shape_ok(nR, rows, Hd)) return 0;
    return ptr_scratch_bytes(B, nR, rows, Hd, 0);
}

extern "C" int tap_pointer_scores_backward(tap_ctx *ctx, const float *proj, const unsigned long long *bits, int B, int nR, int rows,
                                           int Hd, const float *M, const float *k, const float *q, const float *va, const float *vp,
                                           const float *attn, const float *t, const float *g, float *dU_out, float *dq_out,
                                           float *dva_out, float *dvp_out, void *scratch, size_t scratch_bytes, void *stream)
{
    const PtrCall c = {"pointer scores backward", PTR_K_PROJ, B, nR, rows, Hd, 0, true, PTR_NOPICK};
    const int rc = ptr_check(ctx, c, {proj, bits, M, k, q, va, vp, attn, t, g, dU_out, dq_out, dva_out, dvp_out},
                             {proj, M, k, q, va, vp, attn, t, g, dU_out, dq_out, dva_out, dvp_out, scratch}, {bits}, {dU_out}, scratch,
                             scratch_bytes);
    if (rc != TAP_OK || B == 0) return rc;
    const PtrGeom geo = ptr_geom(c);
    PtrArgs a = ptr_args<PtrArgs>(c, geo, bits, M, k, q, va, vp);
    a.proj = proj;
    a.attn = const_cast<float *>(attn); a.t = const_cast<float *>(t); a.g = g;
    a.dU = dU_out; a.dq = dq_out; a.part = static_cast<float *>(scratch);
    return ptr_run<PtrArgs, PTR_NOPICK, true>(ctx, c, geo, a, stream, dva_out, dvp_out);
}

// host only: what ptr_geom gives the five entries, for tests that must know which geometry a batch runs with
extern "C" int tap_pointer_scores_geometry(int B, int nR, int rows, int Hd, int S, int backward, int32_t out[4])
{
    if (!out) return TAP_E_INVALID;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (B < 1 || nR < 1 || rows < 1 || Hd < 1 || S < 0) return TAP_E_INVALID;
    if (!ptr_shape_ok(nR, rows, Hd) || S > PTR_SMAX) return TAP_E_UNSUPPORTED;
    const PtrGeom geo = ptr_geom(B, nR, rows, Hd, backward != 0, S);
    out[0] = geo.epb;
    out[1] = geo.blocks;
    out[2] = (int32_t)geo.lds;
    out[3] = geo.ct;
    return TAP_OK;
}

extern "C" int tap_pointer_scores_static(tap_ctx *ctx, const float *xs, const unsigned long long *bits, int B, int nR, int rows, int Hd,
                                         int S, const float *G, const float *g, const float *M, const float *k, const float *q,
                                         const float *va, const float *vp, float *logits_out, float *attn_out, float *t_out,
                                         void *stream)
{
    const PtrCall c = {"pointer scores static", PTR_K_STATIC, B, nR, rows, Hd, S, false, PTR_NOPICK};
    const int rc = ptr_check(ctx, c, {xs, bits, G, g, M, k, q, va, vp, logits_out, attn_out, t_out},
                             {xs, G, g, M, k, q, va, vp, logits_out, attn_out, t_out}, {bits}, {});
    if (rc != TAP_OK || B == 0) return rc;
    const PtrGeom geo = ptr_geom(c);
    PtrArgsStatic a = ptr_args<PtrArgsStatic>(c, geo, bits, M, k, q, va, vp);
    a.xs = xs; a.Gs = G; a.gs = g; a.S = S;
    a.logits = logits_out; a.attn = attn_out; a.t = t_out;
    return ptr_run(ctx, c, geo, a, stream);
}

extern "C" size_t tap_pointer_scores_static_backward_scratch(int B, int nR, int rows, int Hd, int S)
{
    if (B < 1 || nR < 1 || rows < 1 || Hd < 1 || S < 1 || S > PTR_SMAX || !ptr_shape_ok(nR, rows, Hd)) return 0;
    return ptr_scratch_bytes(B, nR, rows, Hd, S);
}

extern "C" int tap_pointer_scores_static_backward(tap_ctx *ctx, const float *xs, const unsigned long long *bits, int B, int nR, int rows,
                                                  int Hd, int S, const float *G, const float *g, const float *M, const float *k,
                                                  const float *q, const float *va, const float *vp, const float *attn, const float *t,
                                                  const float *grad, float *dU_out, float *dq_out, float *dva_out, float *dvp_out,
                                                  void *scratch, size_t scratch_bytes, void *stream)
{
    const PtrCall c = {"pointer scores static backward", PTR_K_STATIC, B, nR, rows, Hd, S, true, PTR_NOPICK};
    const int rc = ptr_check(ctx, c, {xs, bits, G, g, M, k, q, va, vp, attn, t, grad, dU_out, dq_out, dva_out, dvp_out},
                             {xs, G, g, M, k, q, va, vp, attn, t, grad, dU_out, dq_out, dva_out, dvp_out, scratch}, {bits}, {dU_out},
                             scratch, scratch_bytes);
    if (rc != TAP_OK || B == 0) return rc;
    const PtrGeom geo = ptr_geom(c);
    PtrArgsStatic a = ptr_args<PtrArgsStatic>(c, geo, bits, M, k, q, va, vp);
    a.xs = xs; a.Gs = G; a.gs = g; a.S = S;
    a.attn = const_cast<float *>(attn); a.t = const_cast<float *>(t); a.g = grad;
    a.dU = dU_out; a.dq = dq_out; a.part = static_cast<float *>(scratch);
    return ptr_run<PtrArgsStatic, PTR_NOPICK, true>(ctx, c, geo, a, stream, dva_out, dvp_out);
}

extern "C" int tap_pointer_pick_static(tap_ctx *ctx, const float *xs, size_t xs_env_stride, const unsigned long long *bits, int B, int nR,
                                       int rows, int Hd, int S, const float *G, const float *g, const float *M, const float *k,
                                       const float *q, const float *va, const float *vp, const float *mask, int form,
                                       const int64_t *state, uint32_t step, uint32_t env_offset, int64_t *ptr_out, float *logp_out,
                                       float *logits_out, void *stream)
{
    static_assert(PTR_GREEDY == TAP_PICK_GREEDY && PTR_DRAW == TAP_PICK_DRAW, "the entry's forms are the kernels'");
    const PtrCall c = {"pointer pick static", PTR_K_PICK, B, nR, rows, Hd, S, false, form};
    const int rc = ptr_check(ctx, c, {xs, bits, G, g, M, k, q, va, vp, mask, ptr_out, logp_out},
                             {xs, G, g, M, k, q, va, vp, mask, logp_out, logits_out}, {bits, ptr_out}, {}, nullptr, 0, [&] {
        if (form == TAP_PICK_DRAW && (!state || tap_misaligned(state, 8)))
            return tap_fail(ctx, TAP_E_INVALID, "pointer pick static: state must be an 8-byte aligned int64[2]");
        if (xs_env_stride < (size_t)S * (size_t)nR)
            return tap_fail(ctx, TAP_E_INVALID, "pointer pick static: xs_env_stride %zu below S * nR = %zu", xs_env_stride, (size_t)S * (size_t)nR);
        return (int)TAP_OK;
    });
    if (rc != TAP_OK || B == 0) return rc;
    const PtrGeom geo = ptr_geom(c);
    PtrArgsPick a = ptr_args<PtrArgsPick>(c, geo, bits, M, k, q, va, vp);
    a.xs = xs; a.Gs = G; a.gs = g; a.S = S;
    a.logits = logits_out;          // may be null; attn and t are not written
    a.xs_env_stride = xs_env_stride; a.mask = mask;
    a.state = (const long long *)state; a.step = step; a.env_offset = env_offset;
    a.ptr = ptr_out; a.logp = logp_out;
    return form == PTR_GREEDY ? ptr_run<PtrArgsPick, PTR_GREEDY>(ctx, c, geo, a, stream) : ptr_run<PtrArgsPick, PTR_DRAW>(ctx, c, geo, a, stream);
}
