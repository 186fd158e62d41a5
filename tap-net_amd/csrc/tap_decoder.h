// tap_decoder.h -- what the decoder-step kernels share (decoder.hip: k_decoder_step; heightmap.hip: k_decoder_step_hm): the
// tile geometry, the weight-block fill and the multiply-accumulate of a (64 rows x NG gates) x (DEC_E envs) register
// tile; the step's own pieces -- seed read, h tile, GRU cell with the two dropout masks, q -- on the kernels' argument
// structs; the body of the element-wise backward.  decoder.hip's opening comment describes the geometry.
#pragma once
#include "tap_common.h"

#include <type_traits>

namespace {

constexpr int DEC_E = 4;                    // envs per wavefront
constexpr int DEC_TE = (TAP_BLOCK / 64) * DEC_E;   // envs per workgroup
constexpr int DEC_KC = 32;                  // terms per weight block
constexpr int DEC_WS = DEC_KC + 4;          // row stride of the weight block in the LDS, floats
constexpr int DEC_WROWS = 3 * 64;           // rows of the largest weight block: 64 hidden rows x 3 gates
static_assert((64 * DEC_KC) % TAP_BLOCK == 0 && (DEC_TE * DEC_KC) % TAP_BLOCK == 0, "the fills' trip counts are fixed");

// rows [g * gstride + row0 + (0 .. 63)] for g < NG, terms [k0, k0 + kn) of a row-major matrix of row length ld ->
// lw[(g * 64 + r) * DEC_WS + k], zeros up to DEC_KC.  Global reads along the rows, LDS writes of a 32-lane half on 32
// consecutive banks.  The caller's barriers stand before (the previous block has been consumed) and after.
template <int NG>
__device__ __forceinline__ void dec_fill_weights(float *lw, const float *W, int ld, int gstride, int row0, int k0, int kn, int tid)
{
    constexpr int N = NG * 64 * DEC_KC / TAP_BLOCK;                        // a fixed trip count: the loads of a block are all
    float v[N];                                                            // issued before the first LDS write waits for one
#pragma unroll
    for (int it = 0; it < N; ++it) {
        const int i = it * TAP_BLOCK + tid, r = i / DEC_KC, k = i - r * DEC_KC;
        const int row = (r >> 6) * gstride + row0 + (r & 63);
        v[it] = k < kn ? W[(unsigned)(row * ld + k0 + k)] : 0.f;              // (a weight matrix has at most 3 * 256 * 272 elements)
    }
#pragma unroll
    for (int it = 0; it < N; ++it) {
        const int i = it * TAP_BLOCK + tid, r = i / DEC_KC, k = i - r * DEC_KC;
        lw[r * DEC_WS + k] = v[it];
    }
}

// acc[g][e] = fmaf(w[g][k], act[e][k], acc[g][e]) over 4 * k4n terms in ascending order
template <int NG>
__device__ __forceinline__ void dec_mac(const float *lw, const float *act, int astride, int k4n, int lane, float (&acc)[NG][DEC_E])
{
    for (int k4 = 0; k4 < k4n; ++k4) {
        float4 w[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) w[g] = *reinterpret_cast<const float4 *>(lw + (g * 64 + lane) * DEC_WS + 4 * k4);
#pragma unroll
        for (int e = 0; e < DEC_E; ++e) {
            const float4 x = *reinterpret_cast<const float4 *>(act + e * astride + 4 * k4);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                float s = acc[g][e];
                s = fmaf(w[g].x, x.x, s);
                s = fmaf(w[g].y, x.y, s);
                s = fmaf(w[g].z, x.z, s);
                s = fmaf(w[g].w, x.w, s);
                acc[g][e] = s;
            }
        }
    }
}

__device__ __forceinline__ float dec_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

inline bool dec_hd_ok(int Hd) { return Hd == 64 || Hd == 128 || Hd == 256; }
inline bool dec_misaligned(const void *p) { return ((uintptr_t)p & 3) != 0; }

// ---- dropout inside the launch (tapenv.h: tap_decoder_step_dropout has the definition) ---------------------------------
// What the dropout form of a step kernel takes beside the plain form's arguments.  state = (seed, episode) lives on the
// device: the launch reads it there, so a captured graph draws new masks on every replay.
struct DecDropArgs {
    const long long *state;                 // int64[2]: seed, episode
    unsigned long long *keep;               // (B, 2, Hd / 64): plane 0 drop_rnn, plane 1 drop_hh; bit j % 64 of word j / 64 = row j kept
    float *rnn_out;                         // (B, Hd) the dropped GRU output (what q was formed from), or null
    unsigned step, env_offset, thr_rnn, thr_hh;   // keep iff word >= thr
    float s_rnn, s_hh;                      // float32(1 / (1 - p))
};

// Philox4x32-10 (Salmon et al., SC'11; the standard constants) -> its output words 0 and 1
__device__ __forceinline__ uint2 dec_philox2(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint2(c0, c1);
}

// the two keep predicates of (env b of the call, hidden row j): counter (env_offset + b, j, step, episode mod 2^32), key
// (seed mod 2^32, seed >> 32); word 0 decides drop_rnn, word 1 drop_hh
__device__ __forceinline__ void dec_keep(const DecDropArgs &d, unsigned seed_lo, unsigned seed_hi, unsigned episode, int b, int j,
                                         bool &keep_rnn, bool &keep_hh)
{
    const uint2 w = dec_philox2(d.env_offset + (unsigned)b, (unsigned)j, d.step, episode, seed_lo, seed_hi);
    keep_rnn = w.x >= d.thr_rnn;
    keep_hh = w.y >= d.thr_hh;
}

// ---- the step's pieces, shared by k_decoder_step and k_decoder_step_hm -------------------------------------------------
// What the pieces read of a step kernel's argument struct: DecArgs and HmArgs derive from it and add their own inputs.
struct DecCellArgs {
    const float *h;                         // (B, Hd) or null
    const float *c, *w_hh, *b_hh, *wq;      // (3 Hd,), (3 Hd, Hd), (3 Hd,), (Hd, Hd)
    float *h_out, *q_out, *gates_out;       // (B, Hd), (B, Hd), (B, 4, Hd) or null
    int B, Hd;
};

// the dropout form of an argument struct is the struct plus a DecDropArgs member d: this is what DROP means, to the kernels
// and to every piece below
template <typename A, typename = void> struct dec_has_drop : std::false_type {};
template <typename A> struct dec_has_drop<A, std::enable_if_t<std::is_same<decltype(A::d), DecDropArgs>::value>> : std::true_type {};

struct DecSeed {
    unsigned lo, hi, episode;
};

// the launch's (seed, episode), read from device memory; the plain form reads nothing
template <typename A>
__device__ __forceinline__ DecSeed dec_seed(const A &a)
{
    static_assert(std::is_base_of<DecCellArgs, A>::value, "a step kernel's arguments derive from DecCellArgs");
    DecSeed s = {0, 0, 0};
    if constexpr (dec_has_drop<A>::value) {
        const unsigned long long seed = (unsigned long long)a.d.state[0];
        s.lo = (unsigned)seed;
        s.hi = (unsigned)(seed >> 32);
        s.episode = (unsigned)(unsigned long long)a.d.state[1];
    }
    return s;
}

// the tile's h rows (zeros for a null h and for the envs past the batch) -> hl; the caller's next barrier publishes them
__device__ __forceinline__ void dec_load_h(const DecCellArgs &a, float *hl, int e0, int tid)
{
    const int B = a.B, Hd = a.Hd;
    const bool have_h = a.h != nullptr;
#pragma unroll 4
    for (int i = tid; i < DEC_TE * Hd; i += TAP_BLOCK) {
        const int e = i / Hd, k = i - e * Hd;
        hl[i] = (have_h && e0 + e < B) ? a.h[(size_t)(e0 + e) * Hd + k] : 0.f;
    }
}

// The GRU cell of the 64-row chunk jc for the wavefront's DEC_E envs, from the finished sums gi and gh: r, z, n and h'; under
// dropout the two masks applied where h' leaves the registers, the wavefront's 64 rows of an env one ballot = one keep word;
// h' (as q reads it) to the hn tile, h_out and the gates to global memory.
template <typename A>
__device__ __forceinline__ void dec_cell(const A &a, const DecSeed &s, const float (&gi)[3][DEC_E], const float (&gh)[3][DEC_E],
                                         const float *hl, float *hn, int e0, int ew, int jc, int lane)
{
    const int B = a.B, Hd = a.Hd, j = jc * 64 + lane;
#pragma unroll
    for (int e = 0; e < DEC_E; ++e) {
        const int b = e0 + ew + e;
        const float r = dec_sigmoid(gi[0][e] + gh[0][e]), z = dec_sigmoid(gi[1][e] + gh[1][e]);
        const float n = tanhf(gi[2][e] + r * gh[2][e]);
        const float hv = (1.f - z) * n + z * hl[(ew + e) * Hd + j];
        float h_rnn = hv, h_hh = hv;
        if constexpr (dec_has_drop<A>::value) {
            bool keep_rnn, keep_hh;
            dec_keep(a.d, s.lo, s.hi, s.episode, b, j, keep_rnn, keep_hh);
            h_rnn = keep_rnn ? hv * a.d.s_rnn : 0.f;
            h_hh = keep_hh ? hv * a.d.s_hh : 0.f;
            const unsigned long long w_rnn = __ballot(keep_rnn), w_hh = __ballot(keep_hh);   // the wavefront's 64 rows of env b
            if (b < B) {
                if (lane == 0) {
                    unsigned long long *kw = a.d.keep + (size_t)b * 2 * (Hd / 64) + jc;
                    kw[0] = w_rnn;
                    kw[Hd / 64] = w_hh;
                }
                if (a.d.rnn_out) a.d.rnn_out[(size_t)b * Hd + j] = h_rnn;
            }
        }
        hn[(ew + e) * Hd + j] = h_rnn;
        if (b < B) {
            a.h_out[(size_t)b * Hd + j] = h_hh;
            if (a.gates_out) {
                float *go = a.gates_out + (size_t)b * 4 * Hd + j;
                go[0] = r;
                go[Hd] = z;
                go[2 * Hd] = n;
                go[3 * Hd] = gh[2][e];
            }
        }
    }
}

// q = Wq . h' from the hn tile: the first block's barrier completes h' of the tile
__device__ __forceinline__ void dec_q(const DecCellArgs &a, float *lw, const float *hn, int e0, int ew, int lane, int tid)
{
    const int B = a.B, Hd = a.Hd;
    for (int jc = 0; jc < Hd / 64; ++jc) {
        const int j = jc * 64 + lane;
        float acc[1][DEC_E];
#pragma unroll
        for (int e = 0; e < DEC_E; ++e) acc[0][e] = 0.f;
        for (int k0 = 0; k0 < Hd; k0 += DEC_KC) {
            __syncthreads();
            dec_fill_weights<1>(lw, a.wq, Hd, 0, jc * 64, k0, DEC_KC, tid);
            __syncthreads();
            dec_mac<1>(lw, hn + ew * Hd + k0, Hd, DEC_KC / 4, lane, acc);
        }
#pragma unroll
        for (int e = 0; e < DEC_E; ++e)
            if (e0 + ew + e < B) a.q_out[(size_t)(e0 + ew + e) * Hd + j] = acc[0][e];
    }
}

// ---- the element-wise backward of a step, from the saved gates ----------------------------------------------------------
// from h' = (1 - z) n + z h, n = tanh(gi_n + r gh_n), r / z = sigmoid(gi + gh): per element
//   carry = g z;  da_n = g (1 - z) (1 - n^2);  dgh_n = da_n r;  da_r = da_n gh_n r (1 - r);  da_z = g (h - n) z (1 - z)
// DROP = false: g = g_h (g_r, keep and the scales are not read).  DROP = true, a step that ran with dropout: last_hh =
// drop_hh(h') and rnn_out = drop_rnn(h') both hang on h', so the gradient arriving at h' is g = keep_hh s_hh g_h + keep_rnn
// s_rnn g_r (g_r = g_q . wq, the caller's matmul), each product and the sum rounded; a dropped element contributes an exact zero
// The body of decoder.hip's two kernels, which keep an argument list each: the plain one's listing is then what it was
template <bool DROP>
__device__ __forceinline__ void dec_step_bw(const float *gates, const float *h, const float *g_h, const float *g_r, const unsigned long long *keep,
                                            float s_rnn, float s_hh, float *dgi, float *dghn, float *carry, size_t total, int Hd)
{
    const size_t i = (size_t)blockIdx.x * TAP_BLOCK + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / (size_t)Hd;
    const int j = (int)(i - b * (size_t)Hd);
    bool keep_rnn = true, keep_hh = true;
    if constexpr (DROP) {
        const int nw = Hd >> 6;
        const unsigned long long *kw = keep + b * 2 * (size_t)nw + (j >> 6);
        keep_rnn = (kw[0] >> (j & 63)) & 1;
        keep_hh = (kw[nw] >> (j & 63)) & 1;
    }
    const float *gp = gates + b * 4 * (size_t)Hd + j;
    const float r = gp[0], z = gp[Hd], n = gp[2 * Hd], ghn = gp[3 * Hd];
    float g;
    if constexpr (DROP)
        g = (keep_hh ? s_hh * g_h[i] : 0.f) + (keep_rnn ? s_rnn * g_r[i] : 0.f);
    else
        g = g_h[i];
    const float hp = h ? h[i] : 0.f;
    const float dan = g * (1.f - z) * (1.f - n * n);
    float *dp = dgi + b * 3 * (size_t)Hd + j;
    dp[0] = dan * ghn * (r * (1.f - r));
    dp[Hd] = g * (hp - n) * (z * (1.f - z));
    dp[2 * Hd] = dan;
    dghn[i] = dan * r;
    carry[i] = g * z;
}

// the host side's checks of a dropout launch's own arguments
inline bool dec_drop_null(const void *state, const void *keep) { return !state || !keep; }
inline bool dec_drop_misaligned(const void *state, const void *keep) { return (((uintptr_t)state | (uintptr_t)keep) & 7) != 0; }

} // namespace
